"""examples/phong_headless --list --visible (frr::Renderer::visible_pixels on the C++ host mirror): the printed counts are the
histogram, over the item ranges, of the ids of the frame the run wrote -- the same frame through the Python host mirror, whose
colour equals the run's PPM -- and the PPM is, byte for byte, that of the run without --visible."""
import os
import re
import subprocess

import numpy as np
import pytest

from .visible_scenes import NONE, want_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_list_example_prints_the_visible_pixels_of_every_item(tmp_path):
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    from f_renderer_amd.assets import Model, load_tga
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "phong_headless"])
    exe = os.path.join(ROOT, "examples", "phong_headless")
    obj, tga = (os.path.join(ROOT, "tests", "golden", n) for n in ("cube.obj", "checker24.tga"))
    cw, ch, n = 160, 96, 12
    runs = {}
    for mode, extra in (("plain", []), ("visible", ["--visible"])):
        op, pp = str(tmp_path / (mode + ".rgba")), str(tmp_path / (mode + ".ppm"))
        out = subprocess.run([exe, "--assets", obj, tga, str(cw), str(ch), op, pp, "--instances", str(n), "--list"] + extra, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        runs[mode] = (out.stdout, open(op, "rb").read(), open(pp, "rb").read())
    assert runs["visible"][1] == runs["plain"][1] and runs["visible"][2] == runs["plain"][2]      # nothing written to the PPM changes
    assert "visible pixels" not in runs["plain"][0]
    rows = re.findall(r"^item (\d+): first id (\d+), triangles (\d+), visible pixels (\d+)$", runs["visible"][0], re.M)
    assert [int(x[0]) for x in rows] == list(range(n))
    first, count, pixels = (np.array([int(x[k]) for x in rows], np.int64) for k in (1, 2, 3))
    # the run's frame through the Python mirror: the grid of examples/phong_headless.cpp
    vertices, faces = Model(obj).indexed_inputs()
    F = np.float32
    cols = 4
    s = F(1.0) / F(cols)
    models = np.tile(np.eye(4, dtype=F).reshape(16), (n, 1))
    for i in range(n):
        models[i, [0, 5, 10]] = s
        models[i, 12] = ((F(i % cols) + F(0.5)) * s - F(0.5)) * F(3.0)
        models[i, 13] = ((F(i // cols) + F(0.5)) * s - F(0.5)) * F(2.0)
        models[i, 14] = F(-0.25) * F(i % 3)
    r = fr.Renderer(cw, ch)
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(cw, ch)
    r.set_texture(0, load_tga(tga))
    r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
    mesh = r.upload_mesh_indexed(vertices, faces, fr.VS_PHONG)
    r.clear((30, 30, 30, 255), 0.0)
    r.draw_list(r.upload_draw_list([mesh] * n, models), fr.PS_PHONG)
    c, _, t = r.readback()
    assert c.tobytes() == runs["visible"][1]                                                      # the ids are those of the PPM run's frame
    lf, lc = r.item_ranges()
    assert first.tolist() == lf.tolist() and count.tolist() == lc.tolist()
    want = want_counts(t, (0, cw), (0, ch), bounds=np.append(first, first[-1] + count[-1]))
    assert pixels.tolist() == want.tolist() and pixels.sum() == (t != NONE).sum() > 1000
    assert "items that own no pixel: %d of %d" % (int((want == 0).sum()), n) in runs["visible"][0]
    r.close()
