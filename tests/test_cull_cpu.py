"""Face culling (frr_set_cull) without a GPU: the host build of the device's determinant against an independent NumPy
restatement -- bit for bit, on hand cases and on near-collinear triples where a contracted or reassociated implementation
would show --, the properties of the scenes tests/test_gpu_cull.py relies on, the sub-mesh definition tied to the oracle's
per-input setup lists, and the C / C++ boundary."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from . import cull_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_hand_cases():
    import f_renderer_amd as fr
    d = {k: S.det_f32(np.array(v, np.float32)) for k, v in S.HAND_CASES.items()}
    for k, v in S.HAND_CASES.items():
        _same_bits(fr.host_cull_det(np.array(v, np.float32)), d[k])
    assert d["ccw"] == 1.0 and d["cw"] == -1.0                      # counter-clockwise in NDC (y up) is positive
    assert d["ccw_one_w_negative"] > 0 > d["cw_one_w_negative"]     # across w = 0 the sign is still a defined rule
    assert d["repeated_vertex"] == 0.0 and np.isnan(d["nan"]) and np.isnan(d["inf_minus_inf"])
    for k in ("repeated_vertex", "nan", "inf_minus_inf"):           # d == 0 and NaN: kept under every mode
        assert S.keeps(d[k], S.NEG) and S.keeps(d[k], S.POS) and S.keeps(d[k], S.NONE)
    assert S.keeps(d["ccw"], S.NEG) and not S.keeps(d["ccw"], S.POS)
    assert S.keeps(d["cw"], S.POS) and not S.keeps(d["cw"], S.NEG)


def test_near_collinear_triples_bit_for_bit():
    import f_renderer_amd as fr
    clip = S.near_collinear()
    assert clip.shape == (4096, 3, 4)
    want = S.det_f32(clip)
    # the set can see an implementation that contracts or reassociates: the float32 sign is not the exact sign
    exact = np.array([S.exact_sign(c) for c in clip])
    differ = float((np.sign(want).astype(int) != exact).mean())
    print("float32 sign differs from the exact sign for %.1f %% of the triples; d == 0 for %.1f %%" % (100 * differ, 100 * float((want == 0).mean())))
    assert differ >= 0.25
    _same_bits([fr.host_cull_det(c) for c in clip], want)


@pytest.mark.parametrize("mode", [S.NEG, S.POS])
@pytest.mark.parametrize("name", S.ADMITTED)
def test_admission_condition(name, mode):
    """no GPU test can pass by culling nothing or everything: each mode drops at least a quarter and keeps at least a quarter"""
    sc = S.scene(name)
    keep = S.keep_mask(sc, mode)
    print(name, mode, "keeps", int(keep.sum()), "of", sc.ntris)
    assert keep.sum() * 4 >= sc.ntris and (~keep).sum() * 4 >= sc.ntris


def test_scene_counts():
    d = S.scene("torus").det()
    assert ((d > 0).sum(), (d < 0).sum(), (d == 0).sum()) == (104, 136, 0)
    d = S.scene("sphere").det()
    assert ((d > 0).sum(), (d < 0).sum(), (d == 0).sum()) == (335, 161, 16)   # 16 at the poles: kept under both modes
    assert S.keep_mask(S.scene("sphere"), S.NEG).sum() == 351 and S.keep_mask(S.scene("sphere"), S.POS).sum() == 177
    # the same mesh under a mirrored model matrix faces the other way
    a, b = S.scene("small_torus_left").det(), S.scene("small_torus_mirrored").det()
    assert ((a > 0) != (b > 0)).sum() >= 100 and (a != 0).all() and (b != 0).all()
    # the near-collinear mesh: both signs and zeros in numbers
    d = S.scene("collinear").det()
    assert min((d > 0).sum(), (d < 0).sum(), (d == 0).sum()) >= 400


def test_patterns_are_realised():
    for p, n in S.pattern_cases():
        sc = S.scene("pat_%s_%d" % (p, n))
        np.testing.assert_array_equal(~S.keep_mask(sc, S.NEG), S.pattern(p, n))
        assert sc.ntris == n
    assert S.keep_mask(S.scene("pat_last_kept_513"), S.NEG).nonzero()[0].tolist() == [512]
    assert not S.keep_mask(S.scene("pat_all_257"), S.NEG).any()
    assert not S.keep_mask(S.scene("pat_block_513"), S.NEG)[256:512].any()


def _per_input(oracle, sc):
    u = S.uniforms(oracle, sc)
    return [oracle.geometry_processing(S.W, S.H, t, getattr(oracle, "VS_" + sc.vs), u) for t in sc.tris]


def test_clipped_scene_culls_and_keeps_fans(oracle):
    sc = S.scene("clipped")
    n = np.array([s.shape[0] for s in _per_input(oracle, sc)])
    for mode in (S.NEG, S.POS):
        keep = S.keep_mask(sc, mode)
        assert (n[~keep] > 1).sum() >= 20 and (n[keep] > 1).sum() >= 20      # fans of more than one triangle on both sides
        assert (n[~keep] == 1).any() and (n[keep] == 1).any()
    k = S.keep_mask(sc, S.NEG)
    assert (k[:-1] != k[1:]).sum() >= 100                                     # interleaved


@pytest.mark.parametrize("mode", [S.NEG, S.POS])
@pytest.mark.parametrize("name", ["torus", "sphere", "clipped"])
def test_submesh_is_the_selected_rows_of_the_per_input_lists(oracle, name, mode):
    """the oracle's setup list of mesh[keep] == the full mesh's per-input setup lists selected by keep: culling an input
    removes its triangles and nothing else, in both CPU restatements of the reference"""
    sc = S.scene(name)
    keep = S.keep_mask(sc, mode)
    per = _per_input(oracle, sc)
    rows = [per[i] for i in np.nonzero(keep)[0]]
    want = np.concatenate(rows) if rows else np.zeros((0, 3), oracle.VERTEX_DTYPE)
    f, setup = S.oracle_frame(oracle, name, mode)
    assert setup.shape[0] == want.shape[0] == f.counters.tris_setup
    assert setup.tobytes() == want.tobytes()
    assert f.counters.tris_in == keep.sum()
    full = S.oracle_frame(oracle, name, S.NONE)[0]
    assert f.counters.tris_setup < full.counters.tris_setup and 0 < f.counters.frag_covered < full.counters.frag_covered


def test_symbols_and_headers_compile(tmp_path):
    import ctypes as C
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    L = C.CDLL(fr.build())
    for s in ("frr_set_cull", "frr_host_cull_det"):
        assert hasattr(L, s), f"libfrr_hip.so does not export {s}"
        assert s in _native.SIGNATURES and getattr(fr.lib(), s).argtypes == _native.SIGNATURES[s][1]
    assert fr.lib().frr_abi_version() == 4
    assert (fr.CULL_NONE, fr.CULL_NEG, fr.CULL_POS) == (0, 1, 2) == (S.NONE, S.NEG, S.POS)
    assert fr.lib().frr_set_cull(None, 1) == fr.FRR_ERR_INVALID
    gcc, gxx = shutil.which("gcc"), shutil.which("g++")
    if gcc is None or gxx is None:
        pytest.skip("no gcc / g++")
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "f_renderer_amd", "host")]
    c = tmp_path / "cull.c"
    c.write_text('#include "frr.h"\n'
                 "int use(frr_ctx *c, const float *clip)\n{\n"
                 "    frr_cull m = FRR_CULL_POS;\n"
                 "    int rc = frr_set_cull(c, FRR_CULL_NEG) + frr_set_cull(c, (int)m) + frr_set_cull(c, FRR_CULL_NONE);\n"
                 "    return rc + (frr_host_cull_det(clip) < 0.0f) + (FRR_ABI_VERSION == 4 ? 0 : 1);\n}\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only"] + inc + [str(c)])
    cpp = tmp_path / "cull.cpp"
    cpp.write_text('#include "frr_renderer.hpp"\n'
                   "void use(frr::Renderer &r, const frr::Mesh &m)\n{\n"
                   "    r.set_cull(FRR_CULL_NEG);\n    r.draw(m, FRR_PS_DEPTH);\n    r.set_cull(FRR_CULL_NONE);\n}\n")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only"] + inc + [str(cpp)])
