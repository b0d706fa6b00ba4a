"""Occlusion queries without a GPU: the C boundary (three symbols, plain C99), the depth test the kernel and the host share
(frr_rules.h: fragment_passes), the expected counts of tests/query_reference.py on both CPU oracles with their figures
pinned -- so that a scene that drifts to triviality is noticed -- and the conditions the GPU tests' scenes rest on."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import drawlist_scenes as D
from . import predicate_scenes as P
from . import query_reference as Q
from .conftest import assert_depth_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = D.W, D.H
SYMBOLS = ["frr_query_pixels", "frr_query_pixels_host", "frr_host_fragment_passes"]


def test_symbols_exported_and_header_is_c99(tmp_path):
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    L = C.CDLL(fr.build())
    for s in SYMBOLS:
        assert hasattr(L, s), f"libfrr_hip.so does not export {s}"
        assert s in _native.SIGNATURES and getattr(fr.lib(), s).argtypes == _native.SIGNATURES[s][1]
    assert fr.lib().frr_abi_version() == 4
    assert fr.Renderer.PROFILE_ORDER[:len(fr.Renderer.KERNELS)] == fr.Renderer.KERNELS and fr.Renderer.PROFILE_ORDER[-1] == "k_visible"
    assert callable(fr.Renderer.query_pixels)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "query.c"
    src.write_text('#include "frr.h"\n'
                   "int use(frr_ctx *c, void *dev)\n{\n"
                   "    uint32_t out[4]; uint64_t n = 0; frr_visible_unit u = FRR_PER_TRIANGLE;\n"
                   "    int rc = frr_query_pixels(c, FRR_PER_ITEM, 0, 8, 0, 8, dev, 4) + frr_query_pixels_host(c, (int)u, 0, 8, 0, 8, out, 4, &n);\n"
                   "    return rc + frr_host_fragment_passes(1.0f, 0.5f) + (FRR_ABI_VERSION == 4 ? 0 : 1);\n}\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_fragment_passes_in_the_library():
    """the library's host build of the comparison: ties, +-0, +-inf, NaN on either side, subnormals"""
    import f_renderer_amd as fr
    fp = fr.lib().frr_host_fragment_passes
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    sub = np.array([1], np.uint32).view(np.float32)[0]
    vals = [np.float32(v) for v in (0.0, -0.0, 1.0, -1.0, 0.25, sub, -sub, inf, -inf, 3.0e38)]
    for a in vals:
        assert fp(a, a) == 1 and fp(nan, a) == 1 and fp(a, nan) == 1
        for b in vals:
            assert fp(a, b) == (0 if a < b else 1), (a, b)
    assert fp(nan, nan) == 1 and fp(np.float32(0.0), np.float32(-0.0)) == 1 and fp(np.float32(-0.0), np.float32(0.0)) == 1
    assert fp(sub, np.float32(2) * sub) == 0 and fp(np.float32(2) * sub, sub) == 1


@pytest.mark.parametrize("sanitize", [False, True])
def test_fragment_passes_stand_alone(tmp_path, sanitize):
    """the same comparison (frr_rules.h compiles with no HIP) in a program of its own, plain and under the address and
    undefined-behaviour sanitizers"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "query_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitize else []
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror"] + san + ["-o", exe, os.path.join(ROOT, "tests", "query_host.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("query_host: ok"), (r.stdout, r.stderr)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr


@pytest.mark.parametrize("occ,probe", list(Q.PAIRS))
def test_the_two_oracles_agree_and_the_figures_hold(oracle, occ, probe):
    d0, setup, per, pt, pi = Q.pair(oracle, occ, probe)
    np.testing.assert_array_equal(Q.counts_np(d0, setup), pt)
    want = Q.PAIRS[(occ, probe)]
    if want is not None:
        assert pi.tolist() == want
    else:
        assert int(pi.sum()) == 531 and int((pi == 0).sum()) == 137
        assert int(Q.pair(oracle, None, probe)[4].sum()) == 881
    assert int(pi.sum()) == int(pt.sum()) and len(pt) == sum(per)


def test_figures_against_a_cleared_depth_and_what_they_show(oracle):
    for probe, want in Q.CLEARED.items():
        assert Q.pair(oracle, None, probe)[4].tolist() == want
    # clipped on same_mesh: items 5 and 6 partly occluded, item 4 off-screen
    q, c = Q.PAIRS[("same_mesh", "clipped")], Q.CLEARED["clipped"]
    assert 0 < q[5] < c[5] and 0 < q[6] < c[6] and q[4] == c[4] == 0 and q[:4] == c[:4]
    # sizes on clipped: item 2 fully hidden, item 3 partly
    q, c = Q.PAIRS[("clipped", "sizes")], Q.CLEARED["sizes"]
    assert q[2] == 0 < c[2] and 0 < q[3] < c[3]
    # sizes on sizes: what is visible passes again (ties pass), and nothing else does
    f, _, per = D.oracle_frame(oracle, "sizes", "DEPTH")
    assert Q.PAIRS[("sizes", "sizes")] == P.item_counts(f.tri_id, per).tolist()
    # tie on tie: both items pass everywhere, one of them owns the pixels
    f, _, per = D.oracle_frame(oracle, "tie", "DEPTH")
    assert P.item_counts(f.tri_id, per).tolist() == [0, 477] and Q.PAIRS[("tie", "tie")] == [477, 477]


def test_drawing_only_what_the_query_passed_gives_the_same_frame(oracle):
    """sizes on clipped: the frame that draws only the items with q >= 1 has the colour and depth of the one that draws all"""
    q = Q.pair(oracle, "clipped", "sizes")[4]
    sc = D.scene("sizes")
    frames = []
    for kept in (np.ones(sc.nitems, bool), q >= 1):
        f = oracle.Frame(W, H)
        f.clear(*D.CLEAR)
        D.oracle_list_loop(oracle, D.scene("clipped"), "PHONG", frame=f)
        D.oracle_list_loop(oracle, sc, "PHONG", frame=f, keep=P.oracle_keep(sc, kept))
        frames.append(f)
    assert (q == 0).any()
    assert_depth_equal(frames[1].depth, frames[0].depth)
    np.testing.assert_array_equal(frames[1].color, frames[0].color)


def test_box_proxy():
    from f_renderer_amd import scenes
    for m in D.scene("sizes").meshes + D.scene("gouraud").meshes:
        box = scenes.box_proxy(m.tris)
        assert box.shape == (12, 3, 8) and box.dtype == np.float32 and not box[:, :, 3:].any()
        p = m.tris[:, :, :3].reshape(-1, 3)
        lo, hi = box[:, :, :3].reshape(-1, 3).min(axis=0), box[:, :, :3].reshape(-1, 3).max(axis=0)
        assert (p >= lo).all() and (p <= hi).all()                               # the box contains every vertex
        np.testing.assert_array_equal(lo, p.min(axis=0))
        np.testing.assert_array_equal(hi, p.max(axis=0))
        big = scenes.box_proxy(m.tris, inflate=0.25)[:, :, :3].reshape(-1, 3)
        assert (big.min(axis=0) < lo).all() and (big.max(axis=0) > hi).all()     # inflate grows it on every side
        # twelve triangles that close the box: every corner is used, every face twice
        corners = {tuple(v) for v in box[:, :, :3].reshape(-1, 3)}
        assert len(corners) <= 8
    assert scenes.box_proxy(np.zeros((0, 3, 8), np.float32)).shape == (0, 3, 8)


def test_the_box_scene_of_the_gpu_test(oracle):
    """A condition on the scene, not a guarantee of the method: on the oracle every item whose box counts 0 counts 0 itself;
    at least one item is dropped, one kept, one partly occluded."""
    cover, probe, boxes = Q.box_scenes()
    d0 = D.oracle_list_loop(oracle, cover, "DEPTH")[0].depth
    _, own_setup, own_per = D.oracle_list_loop(oracle, probe, "DEPTH")
    q_own = Q.per_item_sums(Q.counts_c(oracle, d0, own_setup), own_per)
    _, setup, per = D.oracle_list_loop(oracle, boxes, "DEPTH")
    q_box = Q.per_item_sums(Q.counts_c(oracle, d0, setup), per)
    clear_box = Q.per_item_sums(Q.counts_c(oracle, np.full(W * H, D.CLEAR[1], np.float32), setup), per)
    assert (q_own[q_box == 0] == 0).all()
    assert (q_box == 0).any() and (q_box > 0).any() and ((q_box > 0) & (q_box < clear_box)).any()
