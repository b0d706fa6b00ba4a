"""examples/phong_headless --deferred (depth pre-pass, readback_varyings, shade_varyings_host on the C++ host mirror) writes
the bytes of the forward run of the same example."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_deferred_example_writes_the_forward_runs_bytes(tmp_path):
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "phong_headless"])
    exe = os.path.join(ROOT, "examples", "phong_headless")
    W, H = 160, 96
    mesh = scenes.displaced_sphere(n=24)
    tex = scenes.checker_texture(64, 8)
    mp, tp = str(tmp_path / "mesh.f32"), str(tmp_path / "tex.rgba")
    mesh.tofile(mp)
    tex.tofile(tp)
    outs = {}
    for mode in ("forward", "deferred"):
        op, pp = str(tmp_path / (mode + ".rgba")), str(tmp_path / (mode + ".ppm"))
        args = [exe, mp, str(mesh.shape[0]), tp, "64", str(W), str(H), op, pp] + (["--deferred"] if mode == "deferred" else [])
        out = subprocess.run(args, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        outs[mode] = (open(op, "rb").read(), open(pp, "rb").read())
    assert outs["deferred"][0] == outs["forward"][0] and outs["deferred"][1] == outs["forward"][1]
    img = np.frombuffer(outs["forward"][0], np.uint8).reshape(H, W, 4)
    assert len(np.unique(img.reshape(-1, 4), axis=0)) > 50       # (a shaded sphere, not two blank frames)
