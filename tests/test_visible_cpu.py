"""Visible pixel counts without a GPU: the C boundary (three symbols and an enum, plain C99) and the host build of the
kernel's span logic -- the unit search, the run heads, the run lengths (frr_host_visible_counts) -- against the plain NumPy
restatement: np.bincount of np.searchsorted over the item boundaries per item, np.bincount of the ids per triangle.  The id
arrays are the oracle's frames of the draw lists of tests/drawlist_scenes.py, whose figures are pinned here so that a scene
that drifts to triviality is noticed, and made-up arrays for the span's edge cases.  Every expected value is an integer."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from . import drawlist_scenes as D
from .visible_scenes import NONE, bounds_of, want_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = D.W, D.H
SYMBOLS = ["frr_visible_pixels", "frr_visible_pixels_host", "frr_host_visible_counts"]


def test_symbols_exported_and_header_is_c99(tmp_path):
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    L = C.CDLL(fr.build())
    for s in SYMBOLS:
        assert hasattr(L, s), f"libfrr_hip.so does not export {s}"
        assert s in _native.SIGNATURES and getattr(fr.lib(), s).argtypes == _native.SIGNATURES[s][1]
    assert fr.lib().frr_abi_version() == 4 and (fr.PER_ITEM, fr.PER_TRIANGLE) == (0, 1)
    # the constant the binding exposes is the kernel's, and k_visible is the last name of the profile
    hdr = open(os.path.join(ROOT, "f_renderer_amd", "csrc", "frr_visible.h")).read()
    assert int(re.search(r"VIS_LDS_BINS = (\d+);", hdr).group(1)) == fr.VISIBLE_LDS_BINS
    assert fr.Renderer.PROFILE_ORDER[:len(fr.Renderer.KERNELS)] == fr.Renderer.KERNELS and fr.Renderer.PROFILE_ORDER[-1] == "k_visible"
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "visible.c"
    src.write_text('#include "frr.h"\n'
                   "int use(frr_ctx *c, void *dev, const uint32_t *ids, const uint32_t *b)\n{\n"
                   "    uint32_t out[4]; uint64_t n = 0; frr_visible_unit u = FRR_PER_TRIANGLE;\n"
                   "    int rc = frr_visible_pixels(c, FRR_PER_ITEM, 0, 8, 0, 8, dev, 4) + frr_visible_pixels_host(c, (int)u, 0, 8, 0, 8, out, 4, &n);\n"
                   "    return rc + (int)frr_host_visible_counts(ids, 64, 0, 8, 0, 8, b, 3, out, 4) + (FRR_ABI_VERSION == 4 ? 0 : 1);\n}\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _both(fr, ids, wr, hr, per, base=0, entries=None):
    """per item and per triangle, host build against NumPy; returns the per-item and the per-triangle counts"""
    b = bounds_of(per, base)
    gi, _ = fr.host_visible_counts(ids, wr, hr, bounds=b, entries=entries)
    np.testing.assert_array_equal(gi, want_counts(ids, wr, hr, bounds=b, entries=entries))
    T = int(b[-1])
    gt, _ = fr.host_visible_counts(ids, wr, hr, units=T, entries=entries)
    np.testing.assert_array_equal(gt, want_counts(ids, wr, hr, units=T, entries=entries))
    return gi, gt


FIGURES = {"tie": [0, 477], "clipped": [187, 315, 1872, 203, 0, 1520, 322], "empties": [0, 222, 0, 0, 253, 0],
           "sizes": [121, 104, 112, 115, 165, 128, 34]}


@pytest.mark.parametrize("name", D.NAMES)
def test_scenes_against_numpy(oracle, name):
    import f_renderer_amd as fr
    f, _, per = D.oracle_frame(oracle, name)
    gi, gt = _both(fr, f.tri_id, (0, W), (0, H), per)
    assert gi.size == D.scene(name).nitems and gt.size == sum(per)
    drawn = int((f.tri_id != NONE).sum())
    assert int(gi.sum()) == int(gt.sum()) == drawn                       # one pass from id 0: every drawn entry is some item's
    b = bounds_of(per)
    assert [int(gt[b[k]:b[k + 1]].sum()) for k in range(len(per))] == gi.tolist()   # the triangles of an item add up to the item
    if name in FIGURES:
        assert gi.tolist() == FIGURES[name]
    if name == "many":
        assert gi.size == 300 and sum(per) == 590 and drawn == 837
        assert int(((gi == 0) & (np.array(per) > 0)).sum()) == 49 and int(gi.max()) == 12 and int((gt > 0).sum()) == 390
    if name == "clipped":
        assert per[4] > 0 and gi[4] == 0                                 # the wholly off-screen item: set up, owns nothing
    if name in ("none", "all_empty"):
        assert drawn == 0 and not gi.any() and gt.size == 0 and gi.size == (0 if name == "none" else 3)


@pytest.mark.parametrize("name", ["many", "clipped", "sizes"])
def test_sub_windows(oracle, name):
    """x0 > 0, y0 > 0 and widths of 1, 63, 64, 65 and 128 entries: the window's own indexing (row stride x1), the last span
    of a row shorter than a wave, one span, a span and one lane"""
    import f_renderer_amd as fr
    f, _, per = D.oracle_frame(oracle, name)
    for x0, x1, y0, y1 in [(0, 1, 0, H), (5, 6, 3, 40), (0, 63, 0, H), (1, 64, 0, 50), (0, 64, 2, H), (3, 67, 0, H), (0, 65, 7, 90),
                           (20, 85, 10, 11), (0, W, 0, H), (0, W, 31, 33), (37, W, 11, 77)]:
        gi, gt = _both(fr, f.tri_id, (x0, x1), (y0, y1), per)
        assert gi.sum() == gt.sum() <= (x1 - x0) * (y1 - y0)


def test_entries_smaller_and_larger_than_the_units(oracle):
    import f_renderer_amd as fr
    f, _, per = D.oracle_frame(oracle, "many")
    full_i, full_t = _both(fr, f.tri_id, (0, W), (0, H), per)
    for e in (1, 7, 299, 300, 301, 590, 1000):
        gi, gt = _both(fr, f.tri_id, (0, W), (0, H), per, entries=e)
        assert gi.size == gt.size == e
        np.testing.assert_array_equal(gi[:300], full_i[:e])              # the dropped units are counted nowhere ...
        np.testing.assert_array_equal(gt[:590], full_t[:e])
        assert not gi[300:].any() and not gt[590:].any()                 # ... and the tail is zero
    out, adds = fr.host_visible_counts(f.tri_id, (0, W), (0, H), bounds=bounds_of(per), entries=0)
    assert out.size == 0 and adds == 0


def test_a_pass_behind_others_counts_only_its_own_ids():
    """ids of an earlier pass (below the first boundary), of a later one (at and behind the last) and 0xFFFFFFFF count for
    no item; per triangle they all count"""
    import f_renderer_amd as fr
    rng = np.random.default_rng(7)
    ids = rng.integers(0, 120, W * H).astype(np.uint32)
    ids[rng.random(W * H) < 0.2] = NONE
    per = [3, 0, 10, 1, 0, 0, 30, 6]
    gi, gt = _both(fr, ids, (0, W), (0, H), per, base=40)
    assert gi.sum() == ((ids >= 40) & (ids < 90)).sum() and gt.sum() == (ids < 90).sum()
    assert gi[1] == gi[4] == gi[5] == 0


def test_span_edge_cases():
    import f_renderer_amd as fr
    n = 64 * 6
    wr, hr = (0, 64), (0, 6)
    # ids that alternate lane by lane: every lane is a run head
    alt = (np.arange(n) % 2).astype(np.uint32) * 5
    out, adds = fr.host_visible_counts(alt, wr, hr, units=6)
    assert out.tolist() == [n // 2, 0, 0, 0, 0, n // 2] and adds == n
    out, adds = fr.host_visible_counts(alt, wr, hr, bounds=[0, 1, 5, 9])       # ... and the items alternate with them
    assert out.tolist() == [n // 2, 0, n // 2] and adds == n
    out, adds = fr.host_visible_counts(alt, wr, hr, bounds=[0, 6])             # ... while one item makes one run of a span
    assert out.tolist() == [n] and adds == 6
    # a span of one id: one head, one add of 64
    one = np.full(n, 3, np.uint32)
    out, adds = fr.host_visible_counts(one, wr, hr, units=4)
    assert out.tolist() == [0, 0, 0, n] and adds == 6
    out, adds = fr.host_visible_counts(one, (0, 1), (0, 1), units=4)           # (and a window of one entry)
    assert out.tolist() == [0, 0, 0, 1] and adds == 1
    # ids that are not monotonic along the row: the span's ends name item 0, its middle item 2
    row = np.array([1] * 20 + [9] * 24 + [0] * 20, np.uint32)
    out, adds = fr.host_visible_counts(row, wr, (0, 1), bounds=[0, 2, 5, 12])
    assert out.tolist() == [40, 0, 24] and adds == 3
    # nothing drawn anywhere
    out, adds = fr.host_visible_counts(np.full(n, NONE, np.uint32), wr, hr, units=10)
    assert not out.any() and adds == 0
    out, adds = fr.host_visible_counts(np.full(n, NONE, np.uint32), wr, hr, bounds=[0, 4, 4, 4000000000])
    assert not out.any() and adds == 0
    # the largest ids: a boundary table that ends at 0xFFFFFFFF
    big = np.array([NONE - 1, NONE - 1, NONE, 0xFFFFFFF0], np.uint32)
    out, adds = fr.host_visible_counts(big, (0, 4), (0, 1), bounds=[0xFFFFFFF0, 0xFFFFFFF1, NONE])
    assert out.tolist() == [1, 2] and adds == 2
    # bad arguments
    for bad_wr, bad_hr, kw in (((-1, 4), hr, dict(units=4)), ((4, 4), hr, dict(units=4)), (wr, (2, 1), dict(units=4)), (wr, (0, 7), dict(units=4)),
                               (wr, hr, dict(bounds=[3, 2, 5]))):
        with pytest.raises(fr.FrrError):
            fr.host_visible_counts(one, bad_wr, bad_hr, **kw)


def test_random_arrays_against_numpy():
    import f_renderer_amd as fr
    rng = np.random.default_rng(20261020)
    for k in range(60):
        w, h = int(rng.integers(1, 200)), int(rng.integers(1, 12))
        nitems = int(rng.integers(1, 50))
        per = rng.integers(0, 9, nitems)
        per[rng.random(nitems) < 0.3] = 0
        base = int(rng.integers(0, 30))
        T = base + int(per.sum())
        run = int(rng.integers(1, 40))
        ids = np.repeat(rng.integers(0, T + 10, (w * h + run - 1) // run), run)[:w * h].astype(np.uint32)
        ids[rng.random(w * h) < 0.1] = NONE
        x0 = int(rng.integers(0, w))
        _both(fr, ids, (x0, w), (0, h), per, base=base, entries=[None, 3, nitems + 5][k % 3])


def test_span_logic_stand_alone_under_sanitizers(tmp_path, oracle):
    """the same host code (frr_visible.h compiles with no HIP) in a program of its own under the address and
    undefined-behaviour sanitizers, over the `many` and `clipped` frames and their sub-windows: it compares with the plain
    per-entry loop itself and exits 0 only if every count agrees and no sanitizer has reported anything"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "visible_host")
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "visible_host.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("many", "clipped"):
        f, _, per = D.oracle_frame(oracle, name)
        ids, bnd = tmp_path / (name + ".ids"), tmp_path / (name + ".bounds")
        np.asarray(f.tri_id, np.uint32).tofile(ids)
        bounds_of(per).tofile(bnd)
        r = subprocess.run([exe, str(W), str(H), str(ids), str(bnd)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("visible_host: ok"), r.stdout
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
