"""examples/phong_headless --list --deferred --materials (upload_materials + shade_items_host on the C++ host mirror): the
frame it writes is the Python path's -- draw_list depth-only, readback_varyings, shade_items under the same materials --
byte for byte, its digest line is the plain --list --deferred run's, and without the flag nothing changes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_materials_example_writes_the_python_paths_bytes(tmp_path):
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "phong_headless"])
    exe = os.path.join(ROOT, "examples", "phong_headless")
    W, H, n = 160, 96, 7
    mesh = scenes.displaced_sphere(n=12)
    tex = scenes.checker_texture(64, 8)
    mp, tp = str(tmp_path / "mesh.f32"), str(tmp_path / "tex.rgba")
    mesh.tofile(mp)
    tex.tofile(tp)
    outs = {}
    for mode, extra in (("materials", ["--materials"]), ("plain", [])):
        op = str(tmp_path / (mode + ".rgba"))
        out = subprocess.run([exe, mp, str(mesh.shape[0]), tp, "64", str(W), str(H), op, "--instances", str(n), "--list", "--deferred"] + extra, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        outs[mode] = (out.stdout, np.fromfile(op, np.uint8).reshape(H, W, 4))
    digest = [l for l in outs["materials"][0].split("\n") if l.startswith("tris_in=")]
    assert digest and digest == [l for l in outs["plain"][0].split("\n") if l.startswith("tris_in=")]
    assert "materials: n=%d" % n in outs["materials"][0] and "materials:" not in outs["plain"][0]
    assert (outs["materials"][1] != outs["plain"][1]).any()

    # the Python path: the example's camera, grid of models and materials
    eye = (0.0, 1.0, 3.0)
    r = fr.Renderer(W, H)
    texs = [tex, tex.copy(), tex.copy()]
    texs[1][..., 0], texs[2][..., 1] = 255 - tex[..., 0], 255 - tex[..., 1]
    for slot, t in enumerate(texs):
        r.set_texture(slot, np.ascontiguousarray(t))
    r.set_uniforms(view=fr.set_look_at(eye, (0, 0, 0), (0, 1, 0)), proj=fr.set_perspective(np.float32(3.14159274101257324) * np.float32(0.25), np.float32(W) / np.float32(H), 0.1, 100.0),
                   view_pos=eye, texture_slot=0)
    cols = int(np.ceil(np.sqrt(n)))
    s = np.float32(1.0) / np.float32(cols)
    models = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1))
    for i in range(n):
        models[i, [0, 5, 10]] = s
        models[i, 12] = ((np.float32(i % cols) + np.float32(0.5)) * s - np.float32(0.5)) * np.float32(3.0)
        models[i, 13] = ((np.float32(i // cols) + np.float32(0.5)) * s - np.float32(0.5)) * np.float32(2.0)
        models[i, 14] = np.float32(-0.25) * np.float32(i % 3)
    mats = np.zeros(n, fr.MATERIAL_DTYPE)
    k = np.arange(n)
    mats["texture_slot"] = k % 3
    mats["ambient_strength"], mats["specular_strength"] = np.float32(0.1), np.float32(0.5)
    mats["flat_color"] = np.stack([((k + c) % 4).astype(np.float32) / np.float32(3.0) for c in range(3)] + [np.ones(n, np.float32)], axis=1)
    m = r.upload_mesh(mesh, fr.VS_PHONG)
    dl = r.upload_draw_list([m] * n, models)
    r.clear((30, 30, 30, 255), 0.0)
    r.draw_list(dl, fr.PS_DEPTH)
    r.shade_items(fr.PS_PHONG, r.readback_varyings(fill=0.0), r.upload_materials(mats))
    c, _, _ = r.readback()
    np.testing.assert_array_equal(outs["materials"][1], c)
    assert len(np.unique(c.reshape(-1, 4), axis=0)) > 50
    r.close()
