"""examples/phong_headless --list --boxes: the box-query loop from a C++ host (frr::Renderer::list_bounds, query_boxes and
draw_list_if): the objects' boxes tested against an occluder's depth with no proxy pass, only the objects it keeps drawn."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_example_skips_hidden_objects_and_draws_the_same_frame(tmp_path):
    import f_renderer_amd as fr
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "phong_headless"])
    exe = os.path.join(ROOT, "examples", "phong_headless")
    obj, tga = (os.path.join(ROOT, "tests", "golden", n) for n in ("cube.obj", "checker24.tga"))
    n = 12
    out = subprocess.run([exe, "--assets", obj, tga, "160", "120", str(tmp_path / "o.rgba"), "--instances", str(n), "--list", "--boxes"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    print(out.stdout)
    m = re.search(r"^boxes: skipped (\d+) of (\d+) items, colour equal: (\w+), depth equal: (\w+)$", out.stdout, re.M)
    assert m, out.stdout
    skipped, total = int(m.group(1)), int(m.group(2))
    assert total == n and 1 <= skipped < n and m.group(3) == "yes" and m.group(4) == "yes"
    items = re.findall(r"^item (\d+): (none|outside|hidden|kept|unbounded), value (\d+), visible pixels (\d+)$", out.stdout, re.M)
    assert len(items) == n
    for _, status, value, vis in items:
        assert int(vis) <= int(value) and (int(value) == 0) == (status in ("none", "outside", "hidden"))
    assert sum(int(i[2]) == 0 for i in items) == skipped and any(int(i[3]) > 0 for i in items)
    assert os.path.getsize(tmp_path / "o.rgba") == 160 * 120 * 4
    bad = subprocess.run([exe, "--assets", obj, tga, "160", "120", str(tmp_path / "x.rgba"), "--boxes"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--boxes goes with" in bad.stderr
