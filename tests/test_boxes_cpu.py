"""Box queries without a GPU: the C boundary, the host build of the rule (frr_host_query_boxes: the header the kernels compile)
against the NumPy restatement of tests/box_reference.py value for value, the rule's conservativeness against both CPU
oracles, and the header in a program of its own under the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import box_reference as R
from . import box_scenes as B
from . import drawlist_scenes as D
from . import query_reference as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = B.W, B.H
SYMBOLS = ["frr_drawlist_bounds", "frr_query_boxes", "frr_query_boxes_host", "frr_host_query_boxes"]


def both(mvps, lo_hi, flags, window, depth, row_owned=None, entries=None, size=(W, H)):
    """the library's host build and the restatement agree, value for value; returns (out, status_rect_level)"""
    import f_renderer_amd as fr
    got = fr.host_query_boxes(mvps, lo_hi, flags, size, window, depth, row_owned, entries)
    want = R.query(mvps, lo_hi, flags, size, window, depth, row_owned, entries)
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"status / rectangle / level, window {window}")
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"values, window {window}")
    return got


def test_symbols_exported_and_header_is_c99(tmp_path):
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    L = C.CDLL(fr.build())
    for s in SYMBOLS:
        assert hasattr(L, s), f"libfrr_hip.so does not export {s}"
        assert s in _native.SIGNATURES and getattr(fr.lib(), s).argtypes == _native.SIGNATURES[s][1]
    assert callable(fr.Renderer.query_boxes) and callable(fr.Renderer.list_bounds)
    assert fr.Renderer.PROFILE_APPENDED == ("k_boxes",)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "boxes.c"
    src.write_text('#include "frr.h"\n'
                   "int use(frr_ctx *c, void *dev)\n{\n"
                   "    float lo_hi[12], mvp[32], depth[64]; uint32_t fl[2], out[4]; uint64_t n = 0; int32_t srl[12]; uint8_t own[1] = {1};\n"
                   "    int rc = frr_drawlist_bounds(c, 0, lo_hi, fl, 2, &n) + frr_query_boxes(c, 0, 0, 8, 0, 8, dev, 4) + frr_query_boxes_host(c, 0, 0, 8, 0, 8, out, 4, &n);\n"
                   "    return rc + (int)frr_host_query_boxes(mvp, lo_hi, fl, 2, 8, 8, 0, 8, 0, 8, depth, 64, own, out, 4, srl);\n}\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


@pytest.mark.parametrize("name", B.NAMES)
def test_host_rule_equals_restatement(oracle, name):
    """every scene, every window, and the world-2 ownership masks of both layouts, against the cover's depth"""
    sc = B.scene(name)
    lo_hi, flags = B.bounds(sc)
    m, d = B.mvps(sc), B.cover_depth(oracle)
    seen = set()
    for win in B.WINDOWS:
        _, srl = both(m, lo_hi, flags, win, d)
        seen |= {(int(s[0]), int(s[5])) for s in srl}
    for mask in B.ROW_MASKS.values():
        both(m, lo_hi, flags, B.FULL, d, row_owned=mask)
        both(m, lo_hi, flags, (3, 125, 5, 91), d, row_owned=mask)
    both(m, lo_hi, flags, B.FULL, d, entries=max(sc.nitems - 2, 0))
    both(m, lo_hi, flags, B.FULL, d, entries=sc.nitems + 5)
    if name == "sizes":   # rectangles of every level the frame has, the whole window among them
        assert {lv for st, lv in seen if st in (R.HIDDEN, R.KEPT)} >= {2, 3, 4, 5}, seen
    if name == "nonfinite":
        assert {st for st, _ in seen} >= {R.UNBOUNDED}, seen


def test_host_rule_special_cases(oracle):
    """a translation by 1e6, depths with NaN / -0.0 / +-inf, an exact tie, flags, and a window of one pixel"""
    d = B.cover_depth(oracle)
    m, lo_hi, flags = B.far_translation()
    both(m, lo_hi, flags, B.FULL, d)
    sc = B.scene("prototype")
    lo_hi, flags = B.bounds(sc)
    m = B.mvps(sc)
    for name, dd in B.special_depths(oracle).items():
        out, srl = both(m, lo_hi, flags, B.FULL, dd)
        if name == "all_nan":     # a NaN depth has the key below everything: nothing is hidden
            assert not (srl[:, 0] == R.HIDDEN).any()
        if name == "all_inf":     # nothing finite passes against +inf: every bounded item on screen is hidden
            assert not (srl[:, 0] == R.KEPT).any() and (srl[:, 0] == R.HIDDEN).sum() >= 20
    # the exact tie: a depth equal to the item's own bound keeps it, one ulp above hides it
    i = 1                                         # behind the cover
    _, srl = both(m[i:i + 1], lo_hi[i:i + 1], flags[i:i + 1], B.FULL, d)
    assert srl[0, 0] == R.HIDDEN
    lo, hi = np.float32(0.0), np.float32(4.0)     # the item's bound zub, by bisection on the verdict over constant depths
    for _ in range(64):
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if mid in (lo, hi):
            break
        _, s = both(m[i:i + 1], lo_hi[i:i + 1], flags[i:i + 1], B.FULL, np.full(W * H, mid, np.float32))
        if s[0, 0] == R.HIDDEN:
            hi = mid
        else:
            lo = mid
    zub = lo                                      # the largest depth that keeps: the tie
    _, s = both(m[i:i + 1], lo_hi[i:i + 1], flags[i:i + 1], B.FULL, np.full(W * H, zub, np.float32))
    assert s[0, 0] == R.KEPT
    _, s = both(m[i:i + 1], lo_hi[i:i + 1], flags[i:i + 1], B.FULL, np.full(W * H, np.nextafter(zub, np.float32(9)), np.float32))
    assert s[0, 0] == R.HIDDEN
    assert R.zkey(zub) == int(R.zkey_depth(np.array([zub], np.float32))[0])
    # flags: an empty mesh is NONE, a non-finite box UNBOUNDED with the window's pixels, whatever the numbers
    out, srl = both(m[:2], lo_hi[:2], np.array([2, 1], np.uint32), (3, 125, 5, 91), d)
    assert list(srl[:, 0]) == [R.NONE, R.UNBOUNDED] and list(out) == [0, 122 * 86]
    out, srl = both(m[:1], lo_hi[:1], flags[:1], (40, 41, 50, 51), np.zeros(W * H, np.float32))
    assert srl[0, 0] in (R.KEPT, R.OUTSIDE) and out[0] <= 1
    import f_renderer_amd as fr
    with pytest.raises(fr.FrrError):
        fr.host_query_boxes(m, lo_hi, flags, (W, H), (0, W + 1, 0, H), d)
    with pytest.raises(fr.FrrError):
        fr.host_query_boxes(m, lo_hi, flags, (W, H), (-1, W - 1, 0, H), d)


_OWN = {}


def own_counts(oracle):
    """per item of `prototype`: the entries the item's own mesh, drawn alone over the cover's depth, changes -- on both oracles"""
    if not _OWN:
        sc, d = B.scene("prototype"), B.cover_depth(oracle)
        _, setup, per = D.oracle_list_loop(oracle, sc, "DEPTH")
        _OWN["c"] = Q.per_item_sums(Q.counts_c(oracle, d, setup), per)
        _OWN["np"] = Q.per_item_sums(Q.counts_np(d, setup), per)
    return _OWN["c"], _OWN["np"]


def test_rule_is_conservative_against_both_oracles(oracle):
    """hidden => the item's own mesh changes no entry; what it changes <= out[i]; and the scene's condition, asserted and
    nowhere softened: at least 8 items hidden, 8 kept that do own pixels, one UNBOUNDED, one OUTSIDE"""
    sc = B.scene("prototype")
    lo_hi, flags = B.bounds(sc)
    out, srl = both(B.mvps(sc), lo_hi, flags, B.FULL, B.cover_depth(oracle))
    st = srl[:, 0]
    for own in own_counts(oracle):
        assert not ((st == R.HIDDEN) & (own > 0)).any(), (st, own)
        assert not ((out == 0) & (own > 0)).any(), (out, own)
        assert (own <= out).all(), (out, own)
        assert (st == R.HIDDEN).sum() >= 8 and ((st == R.KEPT) & (own > 0)).sum() >= 8, (st, own)
    assert (st == R.UNBOUNDED).sum() >= 1 and (st == R.OUTSIDE).sum() >= 1, st
    np.testing.assert_array_equal(*own_counts(oracle))


def test_header_stand_alone_under_sanitizers(oracle, tmp_path):
    """tests/boxes_host.cpp: the header's host build (no HIP) in a program of its own under the address and
    undefined-behaviour sanitizers, over the prototype scene in every window and with ownership masks; it prints one value
    per item and case, which have to be the restatement's"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "boxes_host")
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "boxes_host.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    d = B.cover_depth(oracle)
    for name in ("prototype", "nonfinite"):
        sc = B.scene(name)
        lo_hi, flags = B.bounds(sc)
        m = B.mvps(sc)
        paths = {}
        for key, arr in (("mvp", m), ("box", lo_hi), ("flags", flags), ("depth", d)):
            paths[key] = str(tmp_path / (name + "." + key))
            np.ascontiguousarray(arr).tofile(paths[key])
        r = subprocess.run([exe, str(W), str(H), paths["mvp"], paths["box"], paths["flags"], paths["depth"]], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        lines = r.stdout.strip().split("\n")
        assert lines[-1].startswith("boxes_host: ok"), r.stdout
        cases = [(win, None) for win in B.WINDOWS] + [(B.FULL, B.ROW_MASKS[k]) for k in sorted(B.ROW_MASKS)]
        assert len(lines) == len(cases) + 1
        for line, (win, mask) in zip(lines, cases):
            want, _ = R.query(m, lo_hi, flags, (W, H), win, d, mask, entries=sc.nitems + 3)
            assert [int(v) for v in line.split()] == [int(v) for v in want], (win, mask)
