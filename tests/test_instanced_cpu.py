"""Instanced passes without a GPU: the C boundary (six symbols, plain C99), the host build of the device's per-instance
matrix product, the properties of the scenes that tests/test_gpu_instanced.py relies on -- checked on the oracle -- and the
agreement of the two CPU restatements on every one of those scenes (as tests/test_oracle_cross.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_np as onp

from . import instanced_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["frr_instances_upload", "frr_instances_bind_device", "frr_instances_free", "frr_geometry_instanced",
           "frr_draw_instanced", "frr_host_instance_mvp"]


def test_symbols_exported_and_header_is_c99(tmp_path):
    import shutil
    import subprocess
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    L = C.CDLL(fr.build())
    for s in SYMBOLS:
        assert hasattr(L, s), f"libfrr_hip.so does not export {s}"
        assert s in _native.SIGNATURES and getattr(fr.lib(), s).argtypes == _native.SIGNATURES[s][1]
    assert fr.lib().frr_abi_version() == 4
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "inst.c"
    src.write_text('#include "frr.h"\n'
                   "int use(frr_ctx *c, const float *m, const void *d, float *o)\n{\n"
                   "    int a = -1, b = -1; uint64_t n = 0;\n"
                   "    int rc = frr_instances_upload(c, m, 2, &a) + frr_instances_bind_device(c, d, 2, &b);\n"
                   "    rc += frr_geometry_instanced(c, 0, a, &n) + frr_draw_instanced(c, 0, b, FRR_PS_DEPTH, 0, 8, 0, 8);\n"
                   "    frr_host_instance_mvp(m, m + 16, m + 32, o);\n"
                   "    return rc + frr_instances_free(c, a) + frr_instances_free(c, b) + (FRR_ABI_VERSION == 4 ? 0 : 1);\n}\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def _matmul_f32(a, b):
    """a * b, column-major [16] float32, every element ((a0*b0 + a1*b1) + a2*b2) + a3*b3 in float32"""
    a, b = a.reshape(4, 4), b.reshape(4, 4)               # [column][row]
    out = np.empty((4, 4), np.float32)
    with np.errstate(all="ignore"):
        for c in range(4):
            for r in range(4):
                out[c, r] = ((a[0, r] * b[c, 0] + a[1, r] * b[c, 1]) + a[2, r] * b[c, 2]) + a[3, r] * b[c, 3]
    return out.reshape(16)


def _matrices():
    rng = np.random.default_rng(20240611)
    out = []
    for k in range(300):
        m = rng.standard_normal((3, 16)).astype(np.float32)
        kind = k % 6
        if kind == 1:
            m[rng.integers(0, 3)] *= np.float32(1e-41)                              # one factor of denormal entries
        elif kind == 2:
            m *= np.float32(1e18)                                                   # products near and past f32 max
        elif kind == 3:
            m[2, 4:8] = -m[2, 0:4]                                                  # cancelling: x * a + x * (-a) ...
            m[0, 4:8] = m[0, 0:4]
            m[1, 1] = m[1, 0]
        elif kind == 4:
            m[rng.integers(0, 3), rng.integers(0, 16)] = np.float32(1e-45) * rng.integers(1, 9)   # single denormals among normals
            m[1] *= np.float32(3e-20)
        elif kind == 5:
            m[0] = np.round(m[0] * 8) / 8                                            # exact sums beside inexact ones
            m[2, rng.integers(0, 16)] = np.float32(3.0e38)
        out.append(m)
    from f_renderer_amd import scenes
    import f_renderer_amd as fr
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(S.W, S.H)
    for mdl in S.clipped_models():
        out.append(np.stack([fr.set_perspective(fovy, aspect, zn, zf), fr.set_look_at(eye, at, up), mdl]))
    return out


def test_host_instance_mvp_is_the_written_out_association():
    import f_renderer_amd as fr
    mats = _matrices()
    assert len(mats) >= 300
    seen_denormal = seen_inf = False
    for proj, view, model in mats:
        got = fr.host_instance_mvp(proj, view, model)
        want = _matmul_f32(_matmul_f32(proj, view), model)
        both_nan = np.isnan(got) & np.isnan(want)
        np.testing.assert_array_equal(got.view(np.uint32)[~both_nan], want.view(np.uint32)[~both_nan])
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        fin = np.isfinite(got) & (got != 0)
        seen_denormal |= bool((np.abs(got[fin]) < np.float32(1.1754944e-38)).any())
        seen_inf |= bool(np.isinf(got).any())
    assert seen_denormal and seen_inf
    # the other association differs on some of them: the test can tell the two apart
    assert any(_matmul_f32(p, _matmul_f32(v, m)).tobytes() != _matmul_f32(_matmul_f32(p, v), m).tobytes() for p, v, m in mats)


def test_scene_properties(oracle):
    f, setup, per = S.oracle_frame(oracle, "clipped")
    sc = S.scene("clipped")
    assert f.counters.tris_setup > f.counters.tris_in == sc.ntris * sc.ninst           # fans
    assert setup.shape[0] == f.counters.tris_setup == sum(per)
    lo = sum(per[:4])                                                                   # instance 4 is wholly off-screen: the reference
    off, ids = setup[lo:lo + per[4]], f.tri_id[f.tri_id != 0xFFFFFFFF]                  # still sets its triangles up (renderer.rs:117-174
    assert per[4] == sc.ntris and (off["spi"][..., 0] < 0).all()                        # rejects none of them), beyond the left edge
    assert not ((ids >= lo) & (ids < lo + per[4])).any()
    assert any(p > sc.ntris for p in per)                                               # an instance through a frustum plane
    assert (f.tri_id[f.tri_id != 0xFFFFFFFF] >= sc.ntris * sc.ninst).any()              # ids beyond the input count are on screen
    for name in ("tie_clip", "tie_phong"):
        f, _, per = S.oracle_frame(oracle, name)
        ids = f.tri_id[f.tri_id != 0xFFFFFFFF]
        assert ids.size > 50 and per[0] == per[1] == per[2] and (ids >= per[0] + per[1]).all()   # the last instance wins every tie
    assert any(S.scene(n).ntris % 64 and 64 % S.scene(n).ntris for n in S.NAMES if S.scene(n).ntris)
    for n, k in S.BOUNDARY:
        f, _, per = S.oracle_frame(oracle, "b%dx%d" % (n, k))
        assert f.counters.tris_in == n * k and f.counters.frag_covered > 0 and len(per) == k
        owners = np.unique(np.searchsorted(np.cumsum(per), f.tri_id[f.tri_id != 0xFFFFFFFF], side="right"))
        assert owners.size >= min(k, 2)                                                 # more than one instance is visible
    assert S.oracle_frame(oracle, "none")[0].counters.tris_in == 0 and S.oracle_frame(oracle, "empty_mesh")[0].counters.tris_in == 0


@pytest.mark.parametrize("name", S.NAMES)
def test_c_oracle_and_numpy_oracle_agree(oracle, name):
    sc = S.scene(name)
    f, setup_c, per = S.oracle_frame(oracle, name)
    K = oracle.vs_num_varyings(getattr(oracle, "VS_" + sc.vs))
    color = np.zeros((S.H, S.W, 4), np.uint8)
    color[...] = S.CLEAR[0]
    depth, tid = np.full(S.W * S.H, S.CLEAR[1], np.float32), np.full(S.W * S.H, 0xFFFFFFFF, np.uint32)
    kw = S.camera_kw(onp) if sc.lit else {}
    if sc.ps == "PHONG":
        kw["tex"] = S.texture()
    setup_np, cov, base = [], 0, 0
    for i in range(sc.ninst):
        s, c = onp.draw(S.W, S.H, sc.tris, getattr(onp, "VS_" + sc.vs), getattr(onp, "PS_" + sc.ps), onp.Uniforms(model=sc.models[i], **kw),
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
