"""Face culling (frr_set_cull).  A geometry pass under a cull mode is by definition the plain pass over the sub-mesh of the
inputs the mode keeps, so every frame here is held, bit for bit, to the oracle's frame of `mesh[keep]` (tests/cull_scenes.py:
keep from oracle_np.vertex_shader and a NumPy restatement of the determinant) AND to the library's own plain draw of the
uploaded sub-mesh: triangle ids, depth bits, RGBA8, the setup list, tris_setup / frag_covered / frag_nan; tris_in counts the
inputs submitted.  tests/test_cull_cpu.py asserts that no scene used here is culled entirely or not at all."""
import functools

import numpy as np
import pytest

from . import cull_scenes as S
from . import user_shaders
from .conftest import assert_depth_equal, owned_pixel_rows
from .test_gpu_streams import _Alias

pytestmark = pytest.mark.gpu
W, H = S.W, S.H
NO_ID = 0xFFFFFFFF


def _renderer(fr, sc, options=(), stream=None):
    r = fr.Renderer(W, H, stream=stream)
    for k, v in options:
        r.set_option(k, v)
    r.set_texture(0, S.texture())
    if sc.lit:
        r.set_uniforms(texture_slot=0, **S.camera_kw(fr))
    return r


def _ids(fr, sc, vs_id=None, ps_id=None, ps=None):
    return (getattr(fr, "VS_" + sc.vs) if vs_id is None else vs_id), (getattr(fr, "PS_" + (ps or sc.ps)) if ps_id is None else ps_id)


def _frame(r, mesh, ps_id, mode, setup=True):
    """clear, one draw under `mode`, everything read back"""
    r.set_cull(mode)
    r.clear(*S.CLEAR)
    r.draw(mesh, ps_id)
    c, d, t = r.readback()
    return dict(c=c, d=d, t=t, st=r.stats(), setup=r.setup_triangles() if setup else None)


def _assert_frame(got, f, rows=None):
    rows = slice(None) if rows is None else rows
    np.testing.assert_array_equal(got["t"].reshape(H, W)[rows], f.tri_id.reshape(H, W)[rows])
    assert_depth_equal(got["d"].reshape(H, W)[rows], f.depth.reshape(H, W)[rows])
    np.testing.assert_array_equal(got["c"][rows], f.color[rows])


def _assert_setup(g, want, K):
    assert g.shape[0] == want.shape[0]
    np.testing.assert_array_equal(g["spi"], want["spi"])
    for name in ("spf", "rhw"):
        np.testing.assert_array_equal(g[name].view(np.uint32), want[name].view(np.uint32))
    np.testing.assert_array_equal(g["ctx"][..., :K].view(np.uint32), want["ctx"][..., :K].view(np.uint32))


def _assert_oracle(oracle, got, f, osetup, sc):
    _assert_frame(got, f)
    _assert_setup(got["setup"], osetup, oracle.vs_num_varyings(getattr(oracle, "VS_" + sc.vs)))
    st = got["st"]
    assert st["tris_in"] == sc.ntris and st["draws"] == 1
    assert st["tris_setup"] == f.counters.tris_setup == osetup.shape[0]
    assert st["frag_covered"] == f.counters.frag_covered and st["frag_nan"] == f.counters.frag_nan


def _assert_same(a, b):
    """a culled frame of the mesh against the plain frame of the sub-mesh"""
    np.testing.assert_array_equal(a["t"], b["t"])
    np.testing.assert_array_equal(a["d"].view(np.uint32), b["d"].view(np.uint32))
    np.testing.assert_array_equal(a["c"], b["c"])
    np.testing.assert_array_equal(a["setup"], b["setup"])
    for k in ("tris_setup", "frag_covered", "frag_nan"):
        assert a["st"][k] == b["st"][k], k


@functools.lru_cache(maxsize=None)
def _phong_sid():
    """the user pair is registered once per process (the registry is the process's; hiprtc takes seconds per program)"""
    import f_renderer_amd as fr
    r = fr.Renderer(32, 32)
    sid = r.register_shader(user_shaders.PHONG, 8, 8)
    r.close()
    return sid


def _check(oracle, name, mode, options=(), vs_id=None, ps_id=None, indexed=False):
    """the scene drawn under `mode` == the oracle's frame of mesh[keep] == the library's plain draw of mesh[keep]"""
    import f_renderer_amd as fr
    from . import indexed_scenes as I
    sc = S.scene(name)
    of, osetup = S.oracle_frame(oracle, name, mode)
    keep = S.keep_mask(sc, mode)
    r = _renderer(fr, sc, options)
    vs_id, ps_id = _ids(fr, sc, vs_id, ps_id)
    if indexed:
        v, f = I.index_mesh(sc.tris)
        assert v.shape[0] < 3 * sc.ntris
        mesh, sub = r.upload_mesh_indexed(v, f, vs_id), r.upload_mesh_indexed(v, np.ascontiguousarray(f[keep]), vs_id)
    else:
        mesh, sub = r.upload_mesh(sc.tris, vs_id), r.upload_mesh(np.ascontiguousarray(sc.tris[keep]), vs_id)
    got = _frame(r, mesh, ps_id, mode)
    _assert_oracle(oracle, got, of, osetup, sc)
    plain = _frame(r, sub, ps_id, fr.CULL_NONE)
    assert plain["st"]["tris_in"] == keep.sum()
    _assert_same(got, plain)
    r.close()
    return got["st"]


# ---- main scenes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [S.NEG, S.POS])
@pytest.mark.parametrize("name", S.MAIN)
def test_main_scenes(oracle, name, mode):
    st = _check(oracle, name, mode)
    assert 0 < st["tris_setup"] < st["tris_in"] and st["frag_covered"] > 1000 and st["replays"] == 0


@pytest.mark.parametrize("name", S.MAIN)
def test_cull_none_after_a_culled_pass_is_the_never_culled_frame(oracle, name):
    import f_renderer_amd as fr
    sc = S.scene(name)
    r = _renderer(fr, sc)
    vs_id, ps_id = _ids(fr, sc)
    mesh = r.upload_mesh(sc.tris, vs_id)
    culled = _frame(r, mesh, ps_id, fr.CULL_POS)
    _assert_oracle(oracle, culled, *S.oracle_frame(oracle, name, S.POS), sc)
    full = _frame(r, mesh, ps_id, fr.CULL_NONE)
    _assert_oracle(oracle, full, *S.oracle_frame(oracle, name, S.NONE), sc)
    assert full["st"]["tris_setup"] > culled["st"]["tris_setup"]
    r.close()


def test_invalid_mode_is_refused_and_leaves_the_mode_in_force(oracle):
    import f_renderer_amd as fr
    sc = S.scene("torus")
    r = _renderer(fr, sc)
    mesh = r.upload_mesh(sc.tris, fr.VS_GOURAUD)
    r.set_cull(fr.CULL_NEG)
    for bad in (3, -1, 1 << 20):
        assert r._lib.frr_set_cull(r._ctx, bad) == fr.FRR_ERR_INVALID
    with pytest.raises(fr.FrrError):
        r.set_cull(7)
    r.clear(*S.CLEAR)                       # (frr_clear does not reset the mode either)
    r.draw(mesh, fr.PS_COLOR)
    c, d, t = r.readback()
    got = dict(c=c, d=d, t=t, st=r.stats(), setup=r.setup_triangles())
    _assert_oracle(oracle, got, *S.oracle_frame(oracle, "torus", S.NEG), sc)
    r.close()


# ---- lane and block patterns -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pat,n", S.pattern_cases())
def test_lane_and_block_patterns(oracle, pat, n):
    """which lanes of a wave and which blocks of the pass survive: every other lane, lanes 0 and 63 of every wave, a whole
    wave, a whole 256-input block (block sum 0), only the last input, nothing.  The surviving lanes of a wave are no run of
    consecutive slots: their records and varyings leave through the slot list."""
    import f_renderer_amd as fr
    name = "pat_%s_%d" % (pat, n)
    st = _check(oracle, name, S.NEG)
    want = n - int(S.pattern(pat, n).sum())
    assert st["tris_in"] == n and st["tris_setup"] == want        # (every input of these sheets is unclipped: one triangle each)
    if pat != "all":
        return
    # an empty list: the passes that consume it write nothing
    import torch
    sc = S.scene(name)
    r = _renderer(fr, sc)
    mesh = r.upload_mesh(sc.tris, fr.VS_CLIP_COLOR)
    buf = torch.full((W * H, 3), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.set_cull(fr.CULL_NEG)
    r.clear(*S.CLEAR)
    r.draw(mesh, fr.PS_COLOR)
    r.draw_wireframe((255, 200, 0, 255))
    r.resolve_varyings(buf.data_ptr(), W * H)
    c, d, t = r.readback()
    assert (t == NO_ID).all() and (d == S.CLEAR[1]).all() and (c == np.array(S.CLEAR[0], np.uint8)).all()
    assert (buf.cpu().numpy() == -7.5).all()
    assert r.setup_triangles().shape[0] == 0 and r.stats()["frag_covered"] == 0
    r.close()


def test_wireframe_has_no_edges_of_culled_inputs(oracle):
    import f_renderer_amd as fr
    from . import lines_reference as R
    sc = S.scene("torus")
    of, osetup = S.oracle_frame(oracle, "torus", S.NEG)
    color = (255, 200, 0, 255)
    r = _renderer(fr, sc)
    r.set_cull(fr.CULL_NEG)
    r.clear(*S.CLEAR)
    r.draw(r.upload_mesh(sc.tris, fr.VS_GOURAUD), fr.PS_COLOR)
    r.draw_wireframe(color)
    c, d, t = r.readback()
    segs = [(tri[e][0], tri[e][1], tri[(e + 1) % 3][0], tri[(e + 1) % 3][1]) for tri in osetup["spi"] for e in range(3)
            if all(0 <= p[0] < W and 0 <= p[1] < H for p in (tri[e], tri[(e + 1) % 3]))]
    xyxy = np.array(segs, np.uint32).reshape(-1, 4)
    assert len(xyxy) > 100
    np.testing.assert_array_equal(t, of.tri_id)
    np.testing.assert_array_equal(c, R.draw_lines(of.color.copy(), xyxy, np.tile(np.array(color, np.uint8), (len(xyxy), 1))))
    r.close()


# ---- clipped inputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [S.NEG, S.POS])
@pytest.mark.parametrize("clip_queue", [0, 1])
def test_clipped_inputs(oracle, clip_queue, mode):
    """culled and kept clipped inputs interleaved (the culled ones include fans of several triangles): a culled one gets no
    fan slots and is never queued, whoever expands the kept ones -- the geometry blocks or the clip kernel"""
    st = _check(oracle, "clipped", mode, options=(("clip_queue", clip_queue),))
    assert st["tris_setup"] > int(S.keep_mask(S.scene("clipped"), mode).sum()) and st["replays"] == 0


@pytest.mark.parametrize("clip_queue", [0, 1])
def test_clipped_pass_replayed_with_grown_work_lists(oracle, clip_queue):
    st = _check(oracle, "clipped", S.NEG, options=(("clip_queue", clip_queue), ("fan_capacity", 16), ("bin_capacity", 64)))
    assert st["replays"] > 0


@pytest.mark.parametrize("clip_queue", [0, 1])
def test_replay_runs_under_the_mode_of_the_call(oracle, clip_queue):
    """frr_geometry under CULL_NEG into a fan space far too small, then the mode changes, then frr_raster: the raster pass is
    verified, the geometry pass is found to have overflowed and is replayed -- under the mode it was called with"""
    import f_renderer_amd as fr
    sc = S.scene("clipped")
    of, osetup = S.oracle_frame(oracle, "clipped", S.NEG)
    assert S.oracle_frame(oracle, "clipped", S.POS)[0].tri_id.tobytes() != of.tri_id.tobytes()
    r = _renderer(fr, sc, options=(("clip_queue", clip_queue), ("fan_capacity", 16), ("bin_capacity", 64)))
    mesh = r.upload_mesh(sc.tris, fr.VS_CLIP_COLOR)
    r.set_cull(fr.CULL_NEG)
    r.clear(*S.CLEAR)
    r.geometry_processing(mesh)
    r.set_cull(fr.CULL_POS)
    r.rasterization((0, W), (0, H), fr.PS_COLOR)
    r.set_cull(fr.CULL_NONE)
    c, d, t = r.readback()
    got = dict(c=c, d=d, t=t, st=r.stats(), setup=r.setup_triangles())
    assert got["st"]["replays"] > 0
    _assert_oracle(oracle, got, of, osetup, sc)
    r.close()


# ---- other mesh and shader kinds ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [S.NEG, S.POS])
def test_indexed_mesh(oracle, mode):
    assert _check(oracle, "torus", mode, indexed=True)["frag_covered"] > 1000


@pytest.mark.parametrize("mode", [S.NEG, S.POS])
def test_user_vertex_shader(oracle, mode):
    """the run-time compiled build of the geometry kernels: the built-in Phong vertex shader restated as a user shader"""
    assert _check(oracle, "sphere", mode, vs_id=_phong_sid())["frag_covered"] > 1000


@pytest.mark.parametrize("mode", [S.NEG, S.POS])
def test_instanced_pass_with_a_mirrored_instance(oracle, mode):
    """the determinant is taken per (instance, triangle) under the instance's matrices: under a mirrored model matrix the same
    mesh faces the other way.  == the oracle's loop of culled draws == the library's loop of plain culled draws"""
    import f_renderer_amd as fr
    a, b = S.scene("small_torus_left"), S.scene("small_torus_mirrored")
    models = np.stack([a.model, b.model])
    ka, kb = S.keep_mask(a, mode), S.keep_mask(b, mode)
    assert (ka != kb).sum() >= 100
    of = oracle.Frame(W, H)
    of.clear(*S.CLEAR)
    osetup = np.concatenate([S.oracle_draw(oracle, of, a, mode), S.oracle_draw(oracle, of, b, mode)])
    r = _renderer(fr, a)
    mesh = r.upload_mesh(a.tris, fr.VS_GOURAUD)
    inst = r.upload_instances(models)
    r.set_cull(mode)
    r.clear(*S.CLEAR)
    r.draw_instanced(mesh, inst, fr.PS_COLOR)
    c, d, t = r.readback()
    got = dict(c=c, d=d, t=t, st=r.stats(), setup=r.setup_triangles())
    _assert_frame(got, of)
    _assert_setup(got["setup"], osetup, 3)
    assert got["st"]["tris_in"] == 2 * a.ntris and got["st"]["tris_setup"] == of.counters.tris_setup == ka.sum() + kb.sum()
    assert got["st"]["frag_covered"] == of.counters.frag_covered
    ids = t[t != NO_ID]
    assert (ids < ka.sum()).sum() > 300 and (ids >= ka.sum()).sum() > 300         # both instances are on screen
    r.clear(*S.CLEAR)
    setups = []
    for m in models:
        r.set_uniforms(model=m)
        r.draw(mesh, fr.PS_COLOR)
        setups.append(r.setup_triangles())
    c2, d2, t2 = r.readback()
    _assert_same(got, dict(c=c2, d=d2, t=t2, st=r.stats(), setup=np.concatenate(setups)))
    r.close()


# ---- alternative paths and ordering ------------------------------------------------------------------------------------

@pytest.mark.parametrize("option", [("raster_sweep", 1), ("bin_atomics", 1), ("frames_in_flight", 1), ("frames_in_flight", 2)])
@pytest.mark.parametrize("name,mode", [("torus", S.NEG), ("clipped", S.POS)])
def test_other_paths(oracle, option, name, mode):
    _check(oracle, name, mode, options=(option,))


def test_caller_bound_targets(oracle):
    import torch
    import f_renderer_amd as fr
    sc = S.scene("sphere")
    of, _ = S.oracle_frame(oracle, "sphere", S.POS)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        X = tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32))
    st.synchronize()
    r = _renderer(fr, sc, stream=st.cuda_stream)
    r.bind_targets(*(x.data_ptr() for x in X))
    r.set_cull(fr.CULL_POS)
    r.clear(*S.CLEAR)
    r.draw(r.upload_mesh(sc.tris, fr.VS_PHONG), fr.PS_PHONG)
    r.sync()
    c, d, t = (x.cpu().numpy() for x in X)
    _assert_frame(dict(c=c.view(np.uint8).reshape(H, W, 4), d=d, t=t.view(np.uint32).ravel()), of)
    assert r.stats()["tris_setup"] == of.counters.tris_setup
    r.close()


def test_one_frame_with_a_mode_per_draw(oracle):
    """the ids of a later draw continue behind the SURVIVORS of the earlier ones"""
    import f_renderer_amd as fr
    seq = [("torus", S.NEG), ("sphere", S.POS), ("small_torus_left", S.NONE), ("torus", S.POS)]
    of = oracle.Frame(W, H)
    of.clear(*S.CLEAR)
    ends = []
    for name, mode in seq:
        S.oracle_draw(oracle, of, S.scene(name), mode)
        ends.append(int(of.counters.tris_setup))
    ids = of.tri_id[of.tri_id != NO_ID]
    assert ends[-1] < sum(S.scene(n).ntris for n, _ in seq)
    for lo, hi in zip([0] + ends[:-1], ends):
        assert ((ids >= lo) & (ids < hi)).any()              # every draw owns pixels
    r = _renderer(fr, S.scene("torus"))
    meshes = {n: r.upload_mesh(S.scene(n).tris, getattr(fr, "VS_" + S.scene(n).vs)) for n in {n for n, _ in seq}}
    r.clear(*S.CLEAR)
    for name, mode in seq:
        r.set_cull(mode)
        r.set_uniforms(model=np.eye(4, dtype=np.float32).reshape(16) if S.scene(name).model is None else S.scene(name).model)
        r.draw(meshes[name], getattr(fr, "PS_" + S.scene(name).ps))
    c, d, t = r.readback()
    _assert_frame(dict(c=c, d=d, t=t), of)
    st = r.stats()
    assert st["tris_in"] == sum(S.scene(n).ntris for n, _ in seq) and st["draws"] == len(seq)
    assert st["tris_setup"] == ends[-1] and st["frag_covered"] == of.counters.frag_covered
    r.close()


def test_raster_after_geometry_uses_the_list_as_it_was_built(oracle):
    """frr_geometry under a mode, the mode changed, two raster windows: the list is the one that was built"""
    import f_renderer_amd as fr
    sc = S.scene("torus")
    wins = [(0, 64, 0, H), (0, W, 0, 40)]
    r = _renderer(fr, sc)
    mesh = r.upload_mesh(sc.tris, fr.VS_GOURAUD)
    for win in wins:
        of = oracle.Frame(W, H)
        of.clear(*S.CLEAR)
        S.oracle_draw(oracle, of, sc, S.NEG, window=win)
        r.set_cull(fr.CULL_NEG)
        r.clear(*S.CLEAR)
        assert r.geometry_processing(mesh, count=True) == of.counters.tris_setup
        r.set_cull(fr.CULL_POS)
        r.rasterization(win[:2], win[2:], fr.PS_COLOR)
        c, d, t = r.readback()
        _assert_frame(dict(c=c, d=d, t=t), of)
    r.close()


# ---- partition ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("rank,world", [(0, 2), (1, 2), (0, 3), (1, 3), (2, 3)])
def test_partitioned(oracle, rank, world, blocked):
    """geometry filtered by tile-row ownership on top of the cull: the rank's rows are the oracle's, ids stay global, and the
    filtered list is not handed out"""
    import f_renderer_amd as fr
    sc = S.scene("clipped")
    of, _ = S.oracle_frame(oracle, "clipped", S.NEG)
    r = _renderer(fr, sc)
    r.set_partition(rank, world, blocked)
    got = _frame(r, r.upload_mesh(sc.tris, fr.VS_CLIP_COLOR), fr.PS_COLOR, fr.CULL_NEG, setup=False)
    own = owned_pixel_rows(H, rank, world, blocked)
    assert own.any() and (got["t"].reshape(H, W)[own] != NO_ID).any()
    _assert_frame(got, of, own)
    assert got["st"]["tris_in"] == sc.ntris and got["st"]["tris_setup"] == of.counters.tris_setup
    with pytest.raises(fr.FrrError) as e:
        r.setup_triangles()
    assert e.value.code == fr.FRR_ERR_INVALID
    r.close()


# ---- a pass proven under one mode says nothing about another ----------------------------------------------------------

def _proof_scene():
    """VS_CLIP_COLOR: 40 small triangles with d < 0 and 400 that cover most of the frame with d > 0.  Under CULL_POS the pass
    needs a few dozen (triangle, tile) records, unculled thousands."""
    from f_renderer_amd import scenes

    def tris(n, seed, r_ndc):
        u = scenes.splitmix_u01(seed, 10 * n).reshape(n, 10)
        w = 1.0 + 3.0 * u[:, 0]
        cx, cy = 0.5 * (2.0 * u[:, 1] - 1.0), 0.5 * (2.0 * u[:, 2] - 1.0)
        out = np.empty((n, 3, 4), np.float64)
        for k in range(3):
            out[:, k, 0] = (cx + r_ndc * (2.0 * u[:, 3 + 2 * k] - 1.0)) * w
            out[:, k, 1] = (cy + r_ndc * (2.0 * u[:, 4 + 2 * k] - 1.0)) * w
            out[:, k, 2], out[:, k, 3] = 0.5 * w, w
        return out.astype(np.float32)
    pos = np.concatenate([tris(40, 21, 0.04), tris(400, 22, 0.5)])
    col = scenes.splitmix_u01(23, pos.shape[0] * 9).reshape(-1, 3, 3).astype(np.float32)
    return S.Scene(S.flipped(np.concatenate([pos, col], axis=2), np.arange(440) < 40), "CLIP_COLOR", "COLOR")


def test_pass_proven_under_cull_pos_is_verified_again_under_cull_none(oracle):
    """tiny work lists; the pass is drawn (verified, proven) under CULL_POS, then under CULL_NONE, which needs far more
    records; its frame is consumed through frr_frame_fence only -- no frr_sync, no read-back -- and must be whole"""
    import torch
    import f_renderer_amd as fr
    sc = _proof_scene()
    frames = {}
    for mode in (S.POS, S.NONE):
        frames[mode] = oracle.Frame(W, H)
        frames[mode].clear(*S.CLEAR)
        S.oracle_draw(oracle, frames[mode], sc, mode)
    assert frames[S.POS].counters.tris_setup == 40 and frames[S.NONE].counters.tris_setup == 440
    tiny = (("bin_capacity", 256),)
    for mode, overflows in ((S.POS, False), (S.NONE, True)):       # on a fresh ctx: the culled pass fits, the plain one does not
        r = _renderer(fr, sc, tiny)
        got = _frame(r, r.upload_mesh(sc.tris, fr.VS_CLIP_COLOR), fr.PS_COLOR, mode, setup=False)
        assert (got["st"]["replays"] >= 1) == overflows, (mode, got["st"])
        r.close()
    st = torch.cuda.Stream()
    r = _renderer(fr, sc, tiny, stream=st.cuda_stream)
    mesh = r.upload_mesh(sc.tris, fr.VS_CLIP_COLOR)

    def fenced_copy():
        r.frame_fence(st.cuda_stream)
        pc, pd, pt = r.target_ptrs()
        with torch.cuda.stream(st):
            return tuple(torch.as_tensor(_Alias(p, (H, W), ts), device="cuda").clone() for p, ts in ((pc, "<i4"), (pd, "<f4"), (pt, "<i4")))
    copies = []
    for mode in (S.POS, S.POS, S.NONE, S.NONE, S.POS):             # (two frames each: the passes alternate between workspace sets)
        r.set_cull(mode)
        r.clear(*S.CLEAR)
        r.draw(mesh, fr.PS_COLOR)
        copies.append((mode, fenced_copy()))
    torch.cuda.synchronize()
    for mode, (c, d, t) in copies:
        f = frames[mode]
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32).ravel(), f.tri_id)
        np.testing.assert_array_equal(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), f.color)
        assert_depth_equal(d.cpu().numpy(), f.depth)
    r.close()


# ---- the device's predicate --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [S.NEG, S.POS])
def test_device_predicate_is_the_hosts_on_near_collinear_triples(oracle, mode):
    """4,096 triples on which the float32 sign differs from the exact one for a quarter: drawn as a VS_CLIP mesh, the inputs
    that survive on the device are those frr_host_cull_det keeps"""
    import f_renderer_amd as fr
    sc = S.scene("collinear")
    host = np.array([fr.host_cull_det(c) for c in sc.tris], np.float32)
    keep = S.keeps(host, mode)
    np.testing.assert_array_equal(keep, S.keep_mask(sc, mode))
    of, osetup = S.oracle_frame(oracle, "collinear", mode)
    assert osetup.shape[0] == keep.sum()                            # (all inside the frustum: one triangle per kept input)
    st = _check(oracle, "collinear", mode)
    assert st["tris_in"] == 4096 and st["tris_setup"] == keep.sum() and 1000 < keep.sum() < 3100
