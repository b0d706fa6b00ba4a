"""FrameBuffer::draw_line without a GPU: the restatement itself (tests/lines_reference.py, the walk of renderer.rs:540-588)
against hand-checked pixel lists; the kernels' per-iteration arithmetic compiled for the host (frr_host_line_pixels) and the
two host mirrors (Python FrameBuffer.draw_line, C++ FrameBuffer::draw_line) against the restatement."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import lines_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HAND = {
    (0, 0, 3, 1): [(0, 0), (1, 0), (2, 0), (2, 1), (3, 1)],
    (0, 0, 2, 2): [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2)],
    (2, 5, 6, 5): [(2, 5), (3, 5), (4, 5), (5, 5)],
    (4, 1, 4, 4): [(4, 1), (4, 2), (4, 3)],
    (1, 1, 4, 7): [(1, 1), (1, 2), (2, 2), (2, 3), (2, 4), (3, 4), (3, 5), (3, 6), (4, 6), (4, 7)],
}
SMALL = list(itertools.product(range(13), repeat=4))          # every segment with coordinates in 0..12: 28,561
WIDE = (3, 5, 70003, 66000)                                   # both extents above 2^16: i * minor needs 64 bits


def _random(n, hi, seed):
    g = np.random.default_rng(seed)
    return [tuple(int(v) for v in s) for s in g.integers(0, hi + 1, (n, 4))]


def max_index(x1, y1, x2, y2, W):
    """the largest linear pixel index of the walk, by the closed forms (what the library validates a list with)"""
    x1, x2 = min(x1, x2), max(x1, x2)
    y1, y2 = min(y1, y2), max(y1, y2)
    if x1 == x2 and y1 == y2:
        return y1 * W + x1
    if x1 == x2:
        return (y2 - 1) * W + x1
    if y1 == y2:
        return y1 * W + x2 - 1
    return y2 * W + x2


def test_restatement_hand_lists():
    for seg, want in HAND.items():
        assert R.line_pixels(*seg) == want
        assert R.line_pixels(seg[2], seg[3], seg[0], seg[1]) == want      # either direction


def test_restatement_falling_line_is_the_rising_one():
    assert R.line_pixels(3, 0, 0, 1) == R.line_pixels(0, 0, 3, 1) == HAND[(0, 0, 3, 1)]
    assert R.line_pixels(0, 9, 7, 2) == R.line_pixels(0, 2, 7, 9)


def test_restatement_wrapped_segment():
    W, H = 10, 6
    px = R.line_pixels(8, 1, 13, 3)
    assert max(x for x, _ in px) == 13 >= W and not R.panics(8, 1, 13, 3, W, H)
    img = R.draw_line(np.zeros((H, W, 4), np.uint8), 8, 1, 13, 3, (9, 9, 9, 9))
    assert img[4, 3].tolist() == [9, 9, 9, 9]                  # (13, 3) is pixel (3, 4)
    assert sorted(np.flatnonzero(img[..., 0])) == sorted(y * W + x for x, y in px)
    assert R.panics(8, 1, 13, 5, W, H)                         # (13, 5): index 63 >= 60
    with pytest.raises(IndexError):
        R.draw_line(np.zeros((H, W, 4), np.uint8), 8, 1, 13, 5, (9, 9, 9, 9))


def test_restatement_counts_and_largest_index():
    """the facts the library relies on: pixel counts, no pixel twice, indices rising, the largest-index forms"""
    for seg in SMALL[::7] + _random(100, 3000, 1):
        x1, y1, x2, y2 = seg
        dx, dy = abs(x2 - x1), abs(y2 - y1)
        idx = R.line_indices(*seg, 20)
        assert len(idx) == (1 if dx == dy == 0 else dy if dx == 0 else dx if dy == 0 else dx + dy + 1)
        assert all(b > a for a, b in zip(idx, idx[1:]))
        assert max(idx) == max_index(*seg, 20)
        assert R.panics(*seg, 20, 9) == (max_index(*seg, 20) >= 20 * 9)


def _host_pixels(L, seg, W, buf):
    n = L.frr_host_line_pixels(*seg, W, buf, len(buf))
    assert 0 <= n <= len(buf)
    return list(buf[:n])


def test_host_line_pixels_equal_the_restatement():
    import f_renderer_amd as fr
    L = fr.lib()
    buf = (C.c_uint64 * 300000)()
    for W in (5, 13, 20):
        for seg in SMALL:
            assert _host_pixels(L, seg, W, buf) == R.line_indices(*seg, W), (seg, W)
    for seg in _random(300, 40000, 2) + [WIDE, (WIDE[1], WIDE[0], WIDE[3], WIDE[2])]:
        assert _host_pixels(L, seg, 1920, buf) == R.line_indices(*seg, 1920), seg
    # the count alone (no buffer), and a short buffer
    assert L.frr_host_line_pixels(1, 1, 4, 7, 20, None, 0) == 10
    short = (C.c_uint64 * 4)()
    assert L.frr_host_line_pixels(1, 1, 4, 7, 20, short, 3) == 10 and list(short) == R.line_indices(1, 1, 4, 7, 20)[:3] + [0]


def _check_framebuffer(draw_one, W, H, segs):
    """draw_one(seg) -> sorted painted indices, or None if it raised"""
    raised = 0
    for seg in segs:
        got = draw_one(seg)
        if max_index(*seg, W) >= W * H:
            assert got is None and R.panics(*seg, W, H), seg
            raised += 1
        else:
            assert got == R.line_indices(*seg, W), seg       # (indices rise along the walk: sorted == write order)
    return raised


SETS = [(5, 13, SMALL), (13, 13, SMALL), (20, 13, SMALL), (640, 400, _random(300, 600, 3) + list(HAND)),
        (2048, 1024, _random(300, 40000, 2))]


def test_python_framebuffer_draw_line():
    import f_renderer_amd as fr
    for W, H, segs in SETS:
        fb = fr.FrameBuffer.new(W, H)

        def draw_one(seg):
            try:
                fb.draw_line(*seg, (255, 255, 255, 255))
            except IndexError:
                fb.clear()
                return None
            idx = np.flatnonzero(fb.buffer[..., 3]).tolist()
            fb.buffer.reshape(-1, 4)[idx] = 0
            return idx
        raised = _check_framebuffer(draw_one, W, H, segs)
        assert (raised > 0) == (W not in (13, 20))             # (coordinates 0..12 stay inside 13 rows of 13 or more)
    fb = fr.FrameBuffer.new(8, 8)
    fb.draw_line(3, 0, 0, 1, (1, 2, 3, 4))                      # colour and addressing
    assert [fb.get_pixel(x, y).tolist() for x, y in HAND[(0, 0, 3, 1)]] == [[1, 2, 3, 4]] * 5 and fb.get_data().sum() == 50


def test_cpp_framebuffer_draw_line(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "lines_host")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "lines_host.cpp")])
    for W, H, segs in SETS:
        a, o = str(tmp_path / "segs.u32"), str(tmp_path / "out.u32")
        np.array(segs, np.uint32).tofile(a)
        subprocess.check_call([exe, str(W), str(H), a, o])
        out = np.fromfile(o, np.uint32).tolist()
        res, at = [], 0
        for _ in segs:
            threw, n = out[at], out[at + 1]
            res.append(None if threw else out[at + 2:at + 2 + n])
            at += 2 + n
        assert at == len(out)
        it = iter(res)
        raised = _check_framebuffer(lambda seg: next(it), W, H, segs)
        assert (raised > 0) == (W not in (13, 20))


def test_calls_fail_cleanly_without_a_ctx():
    import f_renderer_amd as fr
    L = fr.lib()
    lid = C.c_int(-7)
    xyxy, rgba = np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    assert L.frr_lines_upload(None, xyxy.ctypes.data, rgba.ctypes.data, 1, C.byref(lid)) == fr.FRR_ERR_INVALID and lid.value == -7
    assert L.frr_lines_bind_device(None, 256, 256, 1, C.byref(lid)) == fr.FRR_ERR_INVALID and lid.value == -7
    assert L.frr_lines_free(None, 0) == fr.FRR_ERR_INVALID
    assert L.frr_draw_lines(None, 0) == fr.FRR_ERR_INVALID
    assert L.frr_draw_wireframe(None, rgba.ctypes.data) == fr.FRR_ERR_INVALID
    assert fr.Renderer.KERNELS[-2:] == ("k_lines_mark", "k_lines_paint") and fr.Renderer.KERNELS.index("k_bin_seg") == 7
