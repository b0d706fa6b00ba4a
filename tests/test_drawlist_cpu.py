"""Draw lists without a GPU: the C boundary (seven symbols, plain C99), the host build of the device's item search against
a NumPy restatement, the properties of the lists that tests/test_gpu_drawlist.py relies on -- checked on the oracle -- and
the agreement of the two CPU restatements on every one of those lists (as tests/test_instanced_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_np as onp

from . import cull_scenes as CS
from . import drawlist_scenes as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["frr_drawlist_upload", "frr_drawlist_free", "frr_geometry_list", "frr_draw_list", "frr_geometry_item_ranges",
           "frr_host_list_item"]          # + the type frr_draw_item: the seventh name of the section


def test_symbols_exported_and_header_is_c99(tmp_path):
    import shutil
    import subprocess
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    L = C.CDLL(fr.build())
    for s in SYMBOLS:
        assert hasattr(L, s), f"libfrr_hip.so does not export {s}"
        assert s in _native.SIGNATURES and getattr(fr.lib(), s).argtypes == _native.SIGNATURES[s][1]
    assert C.sizeof(_native.DrawItem) == 72
    assert fr.lib().frr_abi_version() == 4
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "list.c"
    src.write_text('#include "frr.h"\n'
                   "int use(frr_ctx *c, const uint32_t *f, const uint32_t *n)\n{\n"
                   "    frr_draw_item it[2] = {{0, 0, {1.0f}}, {1, 0, {1.0f}}};\n"
                   "    int l = -1; uint64_t k = 0, m = 0; uint32_t first[2], count[2];\n"
                   "    int rc = frr_drawlist_upload(c, it, 2, &l) + frr_geometry_list(c, l, &k);\n"
                   "    rc += frr_draw_list(c, l, FRR_PS_DEPTH, 0, 8, 0, 8) + frr_geometry_item_ranges(c, first, count, 2, &m);\n"
                   "    rc += (int)frr_host_list_item(f, n, 2, 3u) + (int)sizeof(frr_draw_item);\n"
                   "    return rc + frr_drawlist_free(c, l) + (FRR_ABI_VERSION == 4 ? 0 : 1);\n}\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


# ---- the item search ---------------------------------------------------------------------------------------------------

def _tables():
    """at least 2,000 tables of 1..600 items, 30 % of them empty; leading, trailing and consecutive empties, all empty, one item"""
    rng = np.random.default_rng(20260713)
    out = []
    for k in range(2000):
        n = int(rng.integers(1, 601))
        nt = rng.integers(1, 40, n).astype(np.uint32)
        nt[rng.random(n) < 0.3] = 0
        kind = k % 8
        if kind == 1:
            nt[:int(rng.integers(1, 4))] = 0                       # leading
        elif kind == 2:
            nt[-int(rng.integers(1, 4)):] = 0                      # trailing
        elif kind == 3 and n > 4:
            a = int(rng.integers(0, n - 3))
            nt[a:a + 3] = 0                                        # consecutive
            nt[a + 3] = max(int(nt[a + 3]), 1)
        elif kind == 4 and k % 64 == 4:
            nt[:] = 0                                              # all empty
        out.append(nt)
    out += [np.array([0], np.uint32), np.array([7], np.uint32), np.array([0, 0, 0], np.uint32), np.array([0, 5, 0, 0, 3, 0], np.uint32),
            np.array([1 << 26, 0, (1 << 26) - 1], np.uint32)]
    return out


def _want(first, ntris, t):
    """the NumPy restatement: the ends are non-decreasing; the item is the first whose end lies behind t"""
    end = first.astype(np.int64) + ntris
    i = np.searchsorted(end, t, side="right")
    ok = i < first.size
    ic = np.minimum(i, first.size - 1)
    ok &= (first[ic] <= t) & (t < end[ic])
    return np.where(ok, ic, -1)


def _naive_first(first, t):
    """'the first item with first <= t' (wrong)"""
    return np.array([int(np.nonzero(first <= x)[0][0]) if (first <= x).any() else -1 for x in t])


def _naive_last(first, t):
    """'the last item with first <= t' (wrong where the last items are empty, and beyond the total)"""
    return np.searchsorted(first, t, side="right") - 1


def test_host_list_item_is_the_searchsorted_restatement():
    import f_renderer_amd as fr
    tables = _tables()
    assert len(tables) >= 2000
    first_differs = last_differs = False
    seen = set()
    for nt in tables:
        first = (np.cumsum(nt, dtype=np.uint64) - nt).astype(np.uint32)
        total = int(nt.sum(dtype=np.uint64))
        b = np.concatenate([first.astype(np.int64), first.astype(np.int64) + nt, [total]])
        t = np.unique(np.concatenate([b - 1, b, b + 1, [total + 5, 0xFFFFFFFF, 0]]))
        t = t[(t >= 0) & (t <= 0xFFFFFFFF)]
        want = _want(first, nt, t)
        got = np.array([fr.host_list_item(first, nt, int(x)) for x in t])
        np.testing.assert_array_equal(got, want)
        assert (want[t >= total] == -1).all() and (want[t < total] >= 0).all()
        assert (nt[want[want >= 0]] > 0).all()                                     # an empty item never owns an input
        if first.size <= 64:                                                       # (the naive rules, on the small tables)
            inside = t < total
            first_differs |= bool((_naive_first(first, t)[inside] != want[inside]).any())
            last_differs |= bool((_naive_last(first, t) != want).any())
        seen |= {"lead"} if nt[0] == 0 else set()
        seen |= {"trail"} if nt[-1] == 0 else set()
        seen |= {"all"} if total == 0 else set()
        seen |= {"single"} if nt.size == 1 else set()
        seen |= {"run"} if nt.size > 2 and ((nt[:-2] == 0) & (nt[1:-1] == 0) & (nt[2:] == 0)).any() else set()
    assert seen == {"lead", "trail", "all", "single", "run"}
    assert first_differs and last_differs                                          # the test can tell both naive rules from the right one


# ---- the lists ---------------------------------------------------------------------------------------------------------

def _first_input_count(oracle, sc, i, t):
    """triangles the oracle emits for input t of item i alone"""
    f = oracle.Frame(D.W, D.H)
    f.clear(*D.CLEAR)
    f.draw(np.ascontiguousarray(sc.item_tris(i)[t:t + 1]), getattr(oracle, "VS_" + sc.vs), oracle.PS_DEPTH,
           oracle.make_uniforms(model=sc.models[i], **D.uniform_kw(oracle, sc, "DEPTH")))
    return int(f.counters.tris_setup)


def test_scene_properties(oracle):
    assert D.scene("sizes").ntris == D.SIZES and D.scene("sizes_rev").ntris == D.SIZES[::-1] and D.scene("empties").ntris == D.EMPTIES
    many = D.scene("many")
    assert many.nitems == 300 and set(many.ntris) == {1, 2, 3} and len(many.meshes) == 3
    ends = np.cumsum(many.ntris)
    assert all(np.unique(np.searchsorted(ends, np.arange(w, min(w + 64, ends[-1])), side="right")).size > 1 for w in range(0, ends[-1], 64))
    for name in D.BOUNDARY:
        f, setup, per = D.oracle_frame(oracle, name)
        sc = D.scene(name)
        assert f.counters.tris_in == sum(sc.ntris) and len(per) == sc.nitems and setup.shape[0] == sum(per) == f.counters.tris_setup
        owners = np.unique(np.searchsorted(np.cumsum(per), f.tri_id[f.tri_id != 0xFFFFFFFF], side="right"))
        assert owners.size > 1                                                          # more than one item is visible
    # clipped: fans; the off-screen item is set up and owns nothing; the spiky item's first and last inputs are fans
    f, setup, per = D.oracle_frame(oracle, "clipped")
    sc = D.scene("clipped")
    assert f.counters.tris_setup > f.counters.tris_in
    lo = sum(per[:4])
    ids = f.tri_id[f.tri_id != 0xFFFFFFFF]
    assert per[4] == sc.ntris[4] and not ((ids >= lo) & (ids < lo + per[4])).any()
    assert per[2] > sc.ntris[2] and per[3] > sc.ntris[3]                                # near plane, side plane
    assert _first_input_count(oracle, sc, 5, 0) > 1 and _first_input_count(oracle, sc, 5, sc.ntris[5] - 1) > 1
    # place: the first input of item 1 is a fan and the list's triangle first[1] owns pixels
    f, setup, per = D.oracle_frame(oracle, "place")
    sc = D.scene("place")
    assert _first_input_count(oracle, sc, 1, 0) > 1
    assert (f.tri_id == per[0]).sum() >= 1
    own = np.unique(np.searchsorted(np.cumsum(per), f.tri_id[f.tri_id != 0xFFFFFFFF], side="right"))
    assert own.tolist() == [0, 1, 2]
    # tie: the later item owns every tied pixel
    f, _, per = D.oracle_frame(oracle, "tie")
    ids = f.tri_id[f.tri_id != 0xFFFFFFFF]
    assert ids.size > 50 and per[0] == per[1] and (ids >= per[0]).all()
    # mirrored: the visible triangles of a closed mesh face the camera; those of item 0 have one sign of the cull
    # determinant, those of item 2 (the same mesh under a matrix of negative determinant) the other
    f, _, per = D.oracle_frame(oracle, "mirrored")
    sc = D.scene("mirrored")
    assert per == sc.ntris                                                              # unclipped: id - first = input
    first = np.cumsum([0] + per)
    ids = f.tri_id[f.tri_id != 0xFFFFFFFF]
    signs = []
    for i in (0, 2):
        mine = np.unique(ids[(ids >= first[i]) & (ids < first[i + 1])]) - first[i]
        d = CS.Scene(sc.item_tris(i), sc.vs, sc.ps, sc.models[i]).det()[mine]
        major = np.sign(np.sign(d).sum())                      # (a triangle on the silhouette may own a pixel edge on)
        assert mine.size > 10 and (d != 0).all() and (np.sign(d) == major).mean() > 0.9
        signs.append(major)
    assert signs[0] == -signs[1]
    assert D.oracle_frame(oracle, "none")[0].counters.tris_in == 0 and D.oracle_frame(oracle, "all_empty")[0].counters.tris_in == 0


@pytest.mark.parametrize("name", D.NAMES)
def test_c_oracle_and_numpy_oracle_agree(oracle, name):
    sc = D.scene(name)
    f, setup_c, per = D.oracle_frame(oracle, name)
    K = oracle.vs_num_varyings(getattr(oracle, "VS_" + sc.vs))
    color = np.zeros((D.H, D.W, 4), np.uint8)
    color[...] = D.CLEAR[0]
    depth, tid = np.full(D.W * D.H, D.CLEAR[1], np.float32), np.full(D.W * D.H, 0xFFFFFFFF, np.uint32)
    from . import instanced_scenes as S
    kw = S.camera_kw(onp) if sc.lit else {}
    if sc.ps == "PHONG":
        kw["tex"] = S.texture()
    setup_np, cov, base = [], 0, 0
    for i in range(sc.nitems):
        if not sc.ntris[i]:
            assert per[i] == 0
            continue
        s, c = onp.draw(D.W, D.H, sc.item_tris(i), getattr(onp, "VS_" + sc.vs), getattr(onp, "PS_" + sc.ps), onp.Uniforms(model=sc.models[i], **kw),
                        color, depth, tid, tri_id_base=base)
        assert len(s) == per[i]
        setup_np += s
        cov += c
        base += len(s)
    assert cov == f.counters.frag_covered and len(setup_np) == setup_c.shape[0]
    for i, tri in enumerate(setup_np):
        for k in range(3):
            assert tuple(setup_c[i, k]["spi"]) == tuple(tri[k]["spi"])
            assert np.array(tri[k]["spf"], np.float32).view(np.uint32).tolist() == setup_c[i, k]["spf"].view(np.uint32).tolist()
            assert np.float32(tri[k]["rhw"]).view(np.uint32) == setup_c[i, k]["rhw"].view(np.uint32)
            if K:
                np.testing.assert_array_equal(tri[k]["ctx"].view(np.uint32), setup_c[i, k]["ctx"][:K].view(np.uint32))
    np.testing.assert_array_equal(tid, f.tri_id)
    np.testing.assert_array_equal(depth.view(np.uint32), f.depth.view(np.uint32))
    np.testing.assert_array_equal(color, f.color)
