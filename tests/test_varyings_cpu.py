"""frr_resolve_varyings / frr_readback_varyings without a GPU: the expected values the GPU tests use (tests/varyings_scenes.py,
the NumPy oracle's interpolated ctx) are tied to the C oracle, the scenes are shown to exercise what they claim, and the new
entry points exist, are declared in plain C and refuse a NULL ctx."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_np as onp
from . import varyings_scenes as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expected_ctx_quantised_is_the_c_oracles_colour(oracle):
    """FRR_PS_COLOR is quantize(ctx[0..3], 1): on every owned pixel the helper's ctx gives the C oracle's RGBA8, and both
    oracles name the same owner everywhere -- for one draw and for a frame of two."""
    a, b = V.basic()[0], V.second()
    for meshes, e in (((a,), V.basic()[1]), ((a, b), V.two_draws())):
        f = oracle.Frame(V.W, V.H)
        f.clear(V.BG, 0.0)
        for m in meshes:
            f.draw(m, oracle.VS_CLIP_COLOR, oracle.PS_COLOR, oracle.make_uniforms(), tri_id_base=int(f.counters.tris_setup))
        np.testing.assert_array_equal(f.tri_id, e.tri_id)
        own = e.owned()
        assert own.sum() > 2000
        rgba = onp.quantize(np.concatenate([e.ctx[own], np.ones((int(own.sum()), 1), np.float32)], axis=1))
        np.testing.assert_array_equal(rgba, f.color.reshape(-1, 4)[own])
        np.testing.assert_array_equal(e.color, f.color)
        assert np.isnan(e.ctx[~own]).all()                       # nothing landed there


def test_scene_conditions_hold():
    tris, e = V.basic()
    info = V.check_scene(e, tris, onp.VS_CLIP_COLOR, onp.Uniforms())
    assert info["fan_owners"] >= 3
    # the frames of the other tests compare something too
    for r in (V.two_draws(), V.second_alone(), V.sub_window(), V.phong()[2], V.gouraud()[2], V.indexed()[2]):
        own = r.owned()[:r.entries]
        assert len(np.unique(r.tri_id[:r.entries][own])) >= 60 and 0.05 <= 1.0 - own.mean() <= 0.75
        assert not np.isnan(r.ctx[:r.entries][own]).any()
    two = V.two_draws()
    assert (two.owned(0) & ~two.owned(1)).mean() > 0.1 and two.owned(1).mean() > 0.1      # both draws keep pixels


def test_user_shader_expectation_is_a_signed_copy():
    """user_expected: varying k = SIGN[k] * colour SRC[k], exact because the clipper and the interpolation treat every
    varying alone and negation commutes with IEEE +, -, * -- shown here on the oracle itself for one clipped triangle."""
    tris, e = V.basic()
    u = onp.Uniforms()
    for i in range(len(tris)):                                    # (the first triangle the clipper turns into a fan)
        t = tris[i:i + 1].copy()
        pos = onp.geometry_processing(V.W, V.H, t[0], onp.VS_CLIP_COLOR, u)
        if len(pos) > 1:
            break
    neg_in = t.copy()
    neg_in[..., 4:7] *= -1
    neg = onp.geometry_processing(V.W, V.H, neg_in[0], onp.VS_CLIP_COLOR, u)
    assert len(pos) > 1 and len(pos) == len(neg)
    for a, b in zip(pos, neg):
        for va, vb in zip(a, b):
            V.assert_bits_equal(va["ctx"], -vb["ctx"])
    w = V.user_expected(e, V.WIDE_SRC, V.WIDE_SIGN)
    assert w.shape == (V.W * V.H, 16) and (w[e.owned()][:, 3] == -e.ctx[e.owned()][:, 2]).all()


def test_symbols_are_built_and_bound():
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    L = C.CDLL(fr.build())
    for s in ("frr_resolve_varyings", "frr_readback_varyings", "frr_geometry_num_varyings"):
        assert hasattr(L, s), f"libfrr_hip.so does not export {s}"
        assert s in _native.SIGNATURES
    assert hasattr(fr.Renderer, "resolve_varyings") and hasattr(fr.Renderer, "readback_varyings")


def test_header_with_the_new_prototypes_is_plain_c99(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "vary.c"
    src.write_text('#include "frr.h"\n'
                   "int use(frr_ctx *c, void *dev, float *host)\n"
                   "{ return frr_resolve_varyings(c, 0, 4, 0, 4, dev, 16u) + frr_readback_varyings(c, 0, 4, 0, 4, host, 16u); }\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_cpp_mirror_with_the_new_methods_compiles(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = tmp_path / "vary.cpp"
    src.write_text('#include "f_renderer_amd/host/frr_renderer.hpp"\n'
                   "int use(frr::Renderer &r, void *dev) { std::vector<float> v; r.resolve_varyings(dev, 16); r.resolve_varyings(dev, 16, {0, 4}, {0, 4});\n"
                   "  return r.readback_varyings(v) + r.readback_varyings(v, {0, 4}, {0, 4}, 1.0f); }\n")
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", ROOT, str(src)])


def test_calls_fail_cleanly_without_a_ctx():
    import f_renderer_amd as fr
    L = fr.lib()
    buf = np.full(16 * 3, 7.0, np.float32)
    assert L.frr_resolve_varyings(None, 0, 4, 0, 4, 256, 16) == fr.FRR_ERR_INVALID
    assert L.frr_readback_varyings(None, 0, 4, 0, 4, buf.ctypes.data, 16) == fr.FRR_ERR_INVALID
    assert (buf == 7.0).all()
    assert L.frr_geometry_num_varyings(None) == fr.FRR_ERR_INVALID
    assert fr.lib().frr_abi_version() == 4                       # additive: the ABI version stays
