"""frr_shade_items without a GPU: the C boundary (frr_material's layout against the ctypes struct and the NumPy dtype, the new
symbols, plain C99), the materials rule of frr_rules.h, the host build of the kernel's per-entry item lookup
(frr_host_entry_items) against np.searchsorted, the same code stand-alone under the host sanitizers, and the expectation of
the GPU tests itself: construction A (the definition on the NumPy oracle) equals construction B (the reference's loop with a
ps_uniform per object on the C oracle) on every scene tests/test_gpu_shade_items.py uses."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_np as onp
from . import drawlist_scenes as D
from . import items_scenes as IT
from . import materials_rule as M
from .visible_scenes import NONE, bounds_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = D.W, D.H
SYMBOLS = ["frr_materials_upload", "frr_materials_bind_device", "frr_materials_free", "frr_shade_items", "frr_shade_items_host", "frr_host_entry_items"]
OFFSETS = {"texture_slot": 0, "ambient_strength": 4, "specular_strength": 8, "reserved": 12, "flat_color": 16, "user": 32}


def test_abi_layout_symbols_and_c99(tmp_path):
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    L = C.CDLL(fr.build())
    for s in SYMBOLS:
        assert hasattr(L, s), f"libfrr_hip.so does not export {s}"
        assert s in _native.SIGNATURES and getattr(fr.lib(), s).argtypes == _native.SIGNATURES[s][1]
    assert fr.lib().frr_abi_version() == 4
    assert C.sizeof(_native.Material) == fr.MATERIAL_DTYPE.itemsize == 64 and _native.MATERIAL_USER == 8
    for name, off in OFFSETS.items():
        assert getattr(_native.Material, name).offset == off == fr.MATERIAL_DTYPE.fields[name][1], name
    assert [n for n, _ in _native.Material._fields_] == list(fr.MATERIAL_DTYPE.names) == list(OFFSETS)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "items.c"
    asserts = "".join(f"_Static_assert(offsetof(frr_material, {n}) == {o}, \"{n}\");\n" for n, o in OFFSETS.items())
    src.write_text('#include <stddef.h>\n#include "frr.h"\n_Static_assert(sizeof(frr_material) == 64, "64 bytes");\n' + asserts +
                   "int use(frr_ctx *c, void *dev, const float *host, const uint32_t *ids, const uint32_t *b, uint32_t *items)\n{\n"
                   "    frr_material m[2] = {{0, 0.1f, 0.5f, 0, {1, 1, 1, 1}, {0}}, {FRR_MAX_TEXTURES - 1, 0, 0, 0, {0}, {0}}}; int t = -1, d = -1;\n"
                   "    int rc = frr_materials_upload(c, m, 2, &t) + frr_materials_bind_device(c, dev, 2, &d);\n"
                   "    rc += frr_shade_items(c, FRR_PS_PHONG, 0, 8, 0, 8, dev, 64, 8, t) + frr_shade_items_host(c, FRR_PS_FLAT, 0, 8, 0, 8, host, 64, 0, d);\n"
                   "    rc += frr_materials_free(c, t) + frr_materials_free(c, d) + (int)sizeof(m[0].user) / (int)sizeof(float) - FRR_MATERIAL_USER;\n"
                   "    return rc + (int)frr_host_entry_items(ids, 64, 0, 8, 0, 8, b, 3, items) + (FRR_ABI_VERSION == 4 ? 0 : 1);\n}\n")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    # ... and the calls alone as C99 (which has no _Static_assert)
    c99 = tmp_path / "items99.c"
    c99.write_text("\n".join(l for l in src.read_text().split("\n") if not l.startswith("_Static_assert")))
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c99)])


# ---- the materials rule ------------------------------------------------------------------------------------------------
def rule_queries():
    """(query, expected code, expected `which`)"""
    q = []
    for use in (M.UPLOAD, M.BIND):
        q += [(M.table(use, 0, 0), M.OK, -1), (M.table(use, 0, 1), M.INVALID, -1), (M.table(use, 4096, 1), M.OK, -1), (M.table(use, 4096, 0), M.OK, -1)]
    # alignment: a bound table is read with 16-byte loads; a host array may lie anywhere
    for off in range(1, 16):
        q += [(M.table(M.BIND, 4096 + off, 3), M.INVALID, -1), (M.table(M.BIND, 4096 + off, 0), M.INVALID, -1), (M.table(M.UPLOAD, 4096 + off, 3), M.OK, -1)]
    # the table against the pass: one entry short, exact, longer, no items, an empty table
    q += [(M.table(M.SHADE, 4096, 6, 7), M.INVALID, -1), (M.table(M.SHADE, 4096, 7, 7), M.OK, -1), (M.table(M.SHADE, 4096, 9, 7), M.OK, -1),
          (M.table(M.SHADE, 0, 0, 0), M.OK, -1), (M.table(M.SHADE, 0, 0, 1), M.INVALID, -1)]
    # a lit shader needs every named slot filled; a user or unlit shader does not; "too short" comes first
    for slots in range(16):
        for filled in range(16):
            missing = slots & ~filled
            first = -1 if not missing else next(s for s in range(4) if (missing >> s) & 1)
            q.append((M.table(M.SHADE, 4096, 3, 3, True, slots, filled), M.INVALID if missing else M.OK, first))
            q.append((M.table(M.SHADE, 4096, 3, 3, False, slots, filled), M.OK, -1))
            q.append((M.table(M.SHADE, 4096, 2, 3, True, slots, filled), M.INVALID, -1))
    return q


def test_materials_rule():
    got = M.ask([M.ok(s, r) for s in (-2 ** 31, -1, 0, 1, 2, 3, 4, 5, 2 ** 31 - 1) for r in (0, 1, -1, 2 ** 31 - 1)])
    want = [(1 if 0 <= s <= 3 and r == 0 else 0) for s in (-2 ** 31, -1, 0, 1, 2, 3, 4, 5, 2 ** 31 - 1) for r in (0, 1, -1, 2 ** 31 - 1)]
    assert [g[0] for g in got] == want
    qs = rule_queries()
    for (q, code, which), (gc, text) in zip(qs, M.ask([q for q, _, _ in qs])):
        msg, gw = text.rsplit("|", 1)
        assert gc == code and int(gw) == which and (code == M.OK) == (msg == ""), (q, gc, text)
    short = M.ask([M.table(M.SHADE, 4096, 2, 3, True, 15, 0)])[0][1]
    assert "fewer entries" in short and "slot" in M.ask([M.table(M.SHADE, 4096, 3, 3, True, 15, 0)])[0][1]


def test_materials_rule_under_the_undefined_behaviour_sanitizer():
    exe = M.build(("-fsanitize=undefined", "-fno-sanitize-recover=all"))
    if exe is None:
        pytest.skip("the host compiler's UBSan runtime is not installed")
    qs = [q for q, _, _ in rule_queries()] + [M.ok(s, r) for s in (-2 ** 31, -1, 0, 3, 4, 2 ** 31 - 1) for r in (0, 1)]
    assert M.ask(qs, exe) == M.ask(qs)


# ---- the per-entry item lookup -------------------------------------------------------------------------------------------
def _lookup(fr, ids, wr, hr, bounds):
    got, rounds = fr.host_entry_items(ids, wr, hr, bounds)
    want = IT.want_items(ids, wr, hr, bounds)
    np.testing.assert_array_equal(got, want)
    wrounds, hist = IT.want_rounds(want, wr, hr)
    assert rounds == wrounds
    return got, rounds, hist


ALL_WINDOWS = [(x0, x0 + w) for w in (1, 63, 64, 65, 100, 128) for x0 in (0, 17)]   # (x1 is the row stride: an id ARRAY has no width)
WINDOWS = [w for w in ALL_WINDOWS if w[1] <= W]                                      # ... a frame has


@pytest.mark.parametrize("name", ["sizes", "many", "empties", "clipped", "place"])
def test_scenes_against_searchsorted(oracle, name):
    import f_renderer_amd as fr
    f, _, per = D.oracle_frame(oracle, name, "DEPTH" if name == "place" else None)
    b = bounds_of(per)
    got, rounds, hist = _lookup(fr, f.tri_id, (0, W), (0, H), b)
    drawn = f.tri_id != NONE
    assert (got[drawn] != NONE).all() and (got[~drawn] == NONE).all()    # one pass from id 0: every drawn entry is some item's
    empty = np.nonzero(np.asarray(per) == 0)[0]
    assert not np.isin(got, empty).any()                                 # an item that emitted nothing owns no entry
    if name == "many":
        assert max(hist) >= 3 and rounds > 2 * sum(v for k, v in hist.items() if k)   # the item changes inside every wave
    for wr in WINDOWS:
        _lookup(fr, f.tri_id, wr, (0, H), b)
    _lookup(fr, f.tri_id, (37, W), (11, 77), b)


def test_synthetic_id_arrays():
    import f_renderer_amd as fr
    rng = np.random.default_rng(20261021)

    def ids_of(T, run, hole=0.1):
        a = np.repeat(rng.integers(0, T + 10, (W * H + run - 1) // run), run)[:W * H].astype(np.uint32)
        a[rng.random(W * H) < hole] = NONE
        return a
    # boundaries that repeat: empty items first, in a row, last; ids of an earlier pass (below 40) and of nobody mixed in
    per = [0, 0, 3, 0, 0, 0, 10, 1, 0, 30, 6, 0, 0]
    b = bounds_of(per, 40)
    for run in (1, 3, 17, 64, 200):
        ids = ids_of(int(b[-1]), run)
        for wr in ALL_WINDOWS:
            got, _, _ = _lookup(fr, ids, wr, (0, 9), b)
            assert not np.isin(got, np.nonzero(np.asarray(per) == 0)[0]).any()
    # one item
    ids = ids_of(60, 5)
    got, rounds, hist = _lookup(fr, ids, (0, W), (0, H), [10, 50])
    assert set(np.unique(got)) == {0, NONE} and set(hist) <= {0, 1}
    # 5,000 items of 0..3 ids: more than any LDS copy of the boundaries holds
    per = rng.integers(0, 4, 5000)
    b = bounds_of(per, 7)
    for run in (1, 2, 40):
        ids = ids_of(int(b[-1]), run, hole=0.05)
        for wr in ALL_WINDOWS:
            _lookup(fr, ids, wr, (0, 12), b)
    got, rounds, hist = _lookup(fr, ids_of(int(b[-1]), 1), (0, W), (0, H), b)
    assert max(hist) > 32                                                # nearly every lane of a span its own item
    # nothing drawn; no items; the largest ids
    got, rounds, _ = _lookup(fr, np.full(W * H, NONE, np.uint32), (0, W), (0, H), [0, 4, 4, 4000000000])
    assert rounds == 0 and (got == NONE).all()
    got, rounds = fr.host_entry_items(ids_of(50, 3), (0, W), (0, H), [5])
    assert rounds == 0 and (got == NONE).all()
    big = np.array([NONE - 1, NONE - 1, NONE, 0xFFFFFFF0], np.uint32)
    got, rounds = fr.host_entry_items(big, (0, 4), (0, 1), [0xFFFFFFF0, 0xFFFFFFF1, NONE])
    assert got.tolist() == [1, 1, NONE, 0] and rounds == 2
    # ids that are not monotonic along the row: the span's ends name item 0, its middle item 2
    row = np.array([1] * 20 + [9] * 24 + [0] * 20, np.uint32)
    got, rounds = fr.host_entry_items(row, (0, 64), (0, 1), [0, 2, 5, 12])
    assert got.tolist() == [0] * 20 + [2] * 24 + [0] * 20 and rounds == 2
    # bad arguments
    one = np.zeros(64 * 6, np.uint32)
    for wr, hr, bb in (((-1, 4), (0, 6), [0, 4]), ((4, 4), (0, 6), [0, 4]), ((0, 64), (2, 1), [0, 4]), ((0, 64), (0, 7), [0, 4]), ((0, 64), (0, 6), [3, 2, 5])):
        with pytest.raises(fr.FrrError):
            fr.host_entry_items(one, wr, hr, bb)


def test_item_lookup_stand_alone_under_sanitizers(tmp_path, oracle):
    """the same host code (frr_visible.h compiles with no HIP) in a program of its own under the address and
    undefined-behaviour sanitizers: it compares with the plain per-entry scan itself and exits 0 only if every item and every
    round count agrees and no sanitizer has reported anything"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "items_host")
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "items_host.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    rng = np.random.default_rng(3)
    cases = []
    for name in ("many", "clipped", "empties"):
        f, _, per = D.oracle_frame(oracle, name)
        cases.append((name, np.asarray(f.tri_id, np.uint32), bounds_of(per)))
    per = rng.integers(0, 4, 5000)
    ids = rng.integers(0, int(per.sum()) + 30, W * H).astype(np.uint32)
    ids[rng.random(W * H) < 0.1] = NONE
    cases.append(("synthetic", ids, bounds_of(per, 9)))
    for name, a, b in cases:
        pi, pb = tmp_path / (name + ".ids"), tmp_path / (name + ".bounds")
        a.tofile(pi)
        b.tofile(pb)
        r = subprocess.run([exe, str(W), str(H), str(pi), str(pb)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.startswith("items_host: ok"), r.stdout
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


# ---- the expectation itself -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ps", [(n, "PHONG") for n in IT.SCENES] + [(n, p) for p in ("BLINN", "FLAT") for n in ("many", "clipped", "place", "none")])
def test_the_two_constructions_agree(oracle, name, ps):
    """A, the definition restated on the NumPy oracle (a ranged shade per item over the depth-only frame), is byte for byte B,
    the reference's loop with a ps_uniform per object on the C oracle -- and so are the ids and the per-item counts"""
    sc, kw, e = IT.depth_only(name)
    fb, per = IT.expected_B(name, ps)
    assert list(e.n_emit) == per
    np.testing.assert_array_equal(e.tri_id, fb.tri_id)
    a = IT.expected_A(name, getattr(onp, "PS_" + ps))
    np.testing.assert_array_equal(a, fb.color)
    if sc.nitems > 1 and sum(per):
        # the materials matter: under material 0 alone the frame differs
        one = IT.expected_A(name, getattr(onp, "PS_" + ps), mats=np.repeat(IT.materials(1), sc.nitems))
        assert (one != a).any()
