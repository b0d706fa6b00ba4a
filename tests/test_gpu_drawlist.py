"""Draw lists (frr_drawlist_upload / frr_geometry_list / frr_draw_list / frr_geometry_item_ranges): many meshes, each under
its own model matrix, in ONE geometry pass.  By definition that is the reference's setup loop over objects
(phong.rs:319-359), so every frame here is held, bit for bit, to the oracle's loop of draws (tests/drawlist_scenes.py):
triangle ids, depth, RGBA8, the setup list, tris_in / tris_setup / frag_covered / frag_nan / draws."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle_np as onp

from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import shade_scenes as SH
from . import user_shaders
from . import varyings_scenes as V
from .conftest import assert_depth_equal, owned_pixel_rows

pytestmark = pytest.mark.gpu
W, H = D.W, D.H
NONE = 0xFFFFFFFF


def _renderer(fr, sc, options=(), stream=None):
    r = fr.Renderer(W, H, stream=stream)
    for k, v in options:
        r.set_option(k, v)
    r.set_texture(0, S.texture())
    if sc.lit:
        r.set_uniforms(texture_slot=0, **S.camera_kw(fr))
    return r


def _err(r):
    return r._lib.frr_last_error(r._ctx).decode()


def _meshes(r, sc, vs_id, kinds=None):
    """one library mesh per distinct mesh of the scene; kinds[k]: "plain" (default), "indexed", "dev", "dev_indexed" """
    import torch
    out = []
    for k, m in enumerate(sc.meshes):
        kind = kinds[k] if kinds else "plain"
        if kind == "plain":
            out.append(r.upload_mesh(m.tris, vs_id))
        elif kind == "indexed":
            out.append(r.upload_mesh_indexed(m.indexed[0], m.indexed[1], vs_id))
        elif kind == "dev":
            dt = torch.from_numpy(m.tris).to("cuda")
            torch.cuda.synchronize()
            out.append(r.bind_mesh_device(dt.data_ptr(), m.ntris, vs_id, keepalive=dt))
        else:
            v, f = m.indexed
            dv, di = torch.from_numpy(v).to("cuda"), torch.from_numpy(f.view(np.int32)).to("cuda")
            torch.cuda.synchronize()
            out.append(r.bind_mesh_device_indexed(dv.data_ptr(), v.shape[0], di.data_ptr(), f.shape[0], vs_id, keepalive=(dv, di)))
    return out


def _upload(r, sc, meshes):
    dl = r.upload_draw_list([meshes[w] for w in sc.which], sc.models)
    assert dl.nitems == sc.nitems and dl.ntris == sum(sc.ntris)
    return dl


def _read(r, setup=True):
    c, d, t = r.readback()
    return dict(c=c, d=d, t=t, st=r.stats(), setup=r.setup_triangles() if setup else None)


def _list_frame(r, dl, ps_id, setup=True):
    r.clear(*D.CLEAR)
    r.draw_list(dl, ps_id)
    return _read(r, setup)


def _loop(r, sc, meshes, ps_id):
    """the only way without a list: one set_uniforms(model) + draw per item"""
    r.clear(*D.CLEAR)
    setups = []
    for i in range(sc.nitems):
        r.set_uniforms(model=sc.models[i])
        r.draw(meshes[sc.which[i]], ps_id)
        setups.append(r.setup_triangles())
    c, d, t = r.readback()
    return dict(c=c, d=d, t=t, st=r.stats(), setup=np.concatenate(setups) if setups else None)


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


def _assert_same(a, b):
    """two frames of the library, byte for byte"""
    for k in "tdc":
        np.testing.assert_array_equal(a[k].view(np.uint32) if k == "d" else a[k], b[k].view(np.uint32) if k == "d" else b[k])
    if a["setup"] is not None and b["setup"] is not None:
        np.testing.assert_array_equal(a["setup"], b["setup"])
    for k in ("tris_in", "tris_setup", "frag_covered", "frag_nan"):
        assert a["st"][k] == b["st"][k], k


def _assert_stats(st, sc, of, per):
    assert st["tris_in"] == sum(sc.ntris) and st["draws"] == 1
    assert st["tris_setup"] == of.counters.tris_setup == sum(per) and st["frag_covered"] == of.counters.frag_covered
    assert st["frag_nan"] == of.counters.frag_nan


def _assert_ranges(r, per, base=0, cap=None):
    first, count = r.item_ranges(cap)
    n = len(per) if cap is None else min(cap, len(per))
    want_first = base + np.cumsum([0] + list(per))[:-1]
    np.testing.assert_array_equal(first, want_first[:n].astype(np.uint32))
    np.testing.assert_array_equal(count, np.array(per[:n], np.uint32))


@functools.lru_cache(maxsize=None)
def _phong_sid():
    """the user pair is registered once per process (the registry is the process's; hiprtc takes seconds per program)"""
    import f_renderer_amd as fr
    r = fr.Renderer(32, 32)
    sid = r.register_shader(user_shaders.PHONG, 8, 8)
    r.close()
    return sid


def _check(oracle, name, options=(), ps=None, vs_id=None, ps_id=None, kinds=None, loop=True, ranges=True):
    """the list in one pass == the oracle's loop of draws == the library's loop of set_uniforms(model) + draw"""
    import f_renderer_amd as fr
    sc = D.scene(name)
    of, osetup, per = D.oracle_frame(oracle, name, ps)
    r = _renderer(fr, sc, options=options)
    vs_id = getattr(fr, "VS_" + sc.vs) if vs_id is None else (_phong_sid() if vs_id == "user" else vs_id)
    ps_id = getattr(fr, "PS_" + (ps or sc.ps)) if ps_id is None else (_phong_sid() if ps_id == "user" else ps_id)
    meshes = _meshes(r, sc, vs_id, kinds)
    dl = _upload(r, sc, meshes)
    g = _list_frame(r, dl, ps_id)
    _assert_frame(g, of)
    _assert_setup(g["setup"], osetup, oracle.vs_num_varyings(getattr(oracle, "VS_" + sc.vs)))
    _assert_stats(g["st"], sc, of, per)
    if ranges:
        _assert_ranges(r, per)
    if loop and sc.nitems and sum(sc.ntris):
        gl = _loop(r, sc, meshes, ps_id)
        _assert_same(g, gl)
        assert gl["st"]["draws"] == sc.nitems
    r.free_draw_list(dl)
    r.close()
    return g["st"]


# ---- boundaries of block (256) and wave (64) ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", D.BOUNDARY)
def test_block_and_wave_boundaries(oracle, name):
    """item sizes around the block and the wave, in both orders; 300 items of 1..3 triangles, so the item changes inside every
    wave; empty items first, in a row and last"""
    st = _check(oracle, name)
    assert st["frag_covered"] > 0 and st["replays"] == 0


def test_one_item_is_the_plain_draw(oracle):
    assert _check(oracle, "one")["frag_covered"] > 0


@pytest.mark.parametrize("name", ["none", "all_empty"])
def test_no_items_and_only_empty_items_draw_nothing(oracle, name):
    st = _check(oracle, name, loop=False)
    assert st["draws"] == 1 and st["tris_in"] == 0 and st["tris_setup"] == 0 and st["frag_covered"] == 0


# ---- clipping ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip_queue", [-1, 1, 0])
def test_clipped_items_become_fans(oracle, clip_queue):
    """items through the near plane and a side plane, one wholly off-screen, one whose first and last inputs are clipped: fans,
    expanded by the geometry blocks themselves or by the clip kernel (one wave per input: its item is wave-uniform)"""
    st = _check(oracle, "clipped", options=(("clip_queue", clip_queue),))
    assert st["tris_setup"] > st["tris_in"] and st["replays"] == 0


def test_clipped_list_replayed_with_grown_work_lists(oracle):
    """fan space and (triangle, tile) lists far too small: the pass is replayed inside the library -- the matrix table is
    filled again inside the replayed command -- and the frame is unchanged"""
    st = _check(oracle, "clipped", options=(("fan_capacity", 16), ("bin_capacity", 64)))
    assert st["replays"] > 0


# ---- kinds of mesh -----------------------------------------------------------------------------------------------------

def test_plain_indexed_and_device_bound_meshes_in_one_list(oracle):
    st = _check(oracle, "mix", kinds=["plain", "indexed", "dev", "dev_indexed"])
    assert st["frag_covered"] > 0


# ---- equivalences on the GPU -------------------------------------------------------------------------------------------

def test_a_list_over_one_mesh_is_the_instanced_pass(oracle):
    import f_renderer_amd as fr
    sc = D.scene("same_mesh")
    r = _renderer(fr, sc)
    meshes = _meshes(r, sc, fr.VS_PHONG)
    g = _list_frame(r, _upload(r, sc, meshes), fr.PS_PHONG)
    r.clear(*D.CLEAR)
    r.draw_instanced(meshes[0], r.upload_instances(sc.models), fr.PS_PHONG)
    gi = _read(r)
    _assert_same(g, gi)
    assert g["setup"].tobytes() == gi["setup"].tobytes() and g["st"]["draws"] == gi["st"]["draws"] == 1
    _assert_frame(g, D.oracle_frame(oracle, "same_mesh")[0])
    r.close()


def test_the_later_item_wins_a_depth_tie(oracle):
    """two items with the same mesh and matrix: every fragment ties, equal depth replaces (renderer.rs:363)"""
    import f_renderer_amd as fr
    _check(oracle, "tie")
    sc = D.scene("tie")
    per = D.oracle_frame(oracle, "tie")[2]
    r = _renderer(fr, sc)
    g = _list_frame(r, _upload(r, sc, _meshes(r, sc, fr.VS_PHONG)), fr.PS_DEPTH, setup=False)
    ids = g["t"][g["t"] != NONE]
    assert ids.size > 50 and (ids >= per[0]).all() and (ids < sum(per)).all()
    r.close()


# ---- shaders -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["clip_vs", "clip_color", "gouraud", "user", "user_vs_builtin_ps"])
def test_shaders(oracle, case):
    """a vertex shader that reads no matrix, the other built-in pairs, and the run-time compiled build of the same kernels: a
    user pair whose vertex shader reads u.mvp AND u.model, under its own and under the built-in pixel shader"""
    if case == "user":
        st = _check(oracle, "clipped", vs_id="user", ps_id="user")
    elif case == "user_vs_builtin_ps":
        st = _check(oracle, "mix", vs_id="user", kinds=["plain", "indexed", "plain", "indexed"])
    elif case == "clip_vs":
        st = _check(oracle, case, kinds=["plain", "indexed"])
    else:
        st = _check(oracle, case)
    assert st["frag_covered"] > 0


def test_a_list_that_mixes_vertex_shaders_is_refused():
    import f_renderer_amd as fr
    sc = D.scene("gouraud")
    r = _renderer(fr, sc)
    a, b = r.upload_mesh(sc.meshes[0].tris, fr.VS_GOURAUD), r.upload_mesh(sc.meshes[1].tris, fr.VS_PHONG)
    with pytest.raises(fr.FrrError) as e:
        r.upload_draw_list([a, a, b, a], sc.models)
    assert e.value.code == fr.FRR_ERR_INVALID and "item 2" in str(e.value) and "item 2" in _err(r)
    r.close()


# ---- frames in flight, other paths, raster windows ---------------------------------------------------------------------

@pytest.mark.parametrize("option", [("frames_in_flight", 1), ("frames_in_flight", 2), ("overlap", 0), ("overlap", 1), ("raster_sweep", 1), ("bin_atomics", 1)])
def test_other_paths(oracle, option):
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    of, _, per = D.oracle_frame(oracle, "clipped")
    r = _renderer(fr, sc, options=(option,))
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    for _ in range(3):                         # consecutive frames alternate between target sets, streams and workspace sets
        g = _list_frame(r, dl, fr.PS_PHONG, setup=False)
        _assert_frame(g, of)
        _assert_stats(g["st"], sc, of, per)
    r.close()


def test_one_list_geometry_two_raster_windows(oracle):
    """renderer.rs:269-271: one setup list, several ranges"""
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    wins = [(0, 64, 0, H), (0, W, 0, 40)]
    r = _renderer(fr, sc)
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    r.clear(*D.CLEAR)
    n = r.geometry_list(dl, count=True)
    for win in wins:
        r.rasterization(win[:2], win[2:], fr.PS_PHONG)
    of = oracle.Frame(W, H)
    of.clear(*D.CLEAR)
    pers = [D.oracle_list_loop(oracle, sc, frame=of, window=win, tri_id_base=0)[2] for win in wins]   # (one setup list: the same ids in both windows)
    assert n == sum(pers[0])
    _assert_frame(_read(r, setup=False), of)
    _assert_ranges(r, pers[0])
    r.close()


def test_plain_list_plain_in_one_frame(oracle):
    """the ids of a draw continue behind the whole list pass, and the pass's behind the draw before it; item_ranges are frame-global"""
    import f_renderer_amd as fr
    sc, other = D.scene("clipped"), D.scene("one")
    kw = D.uniform_kw(oracle, sc, "PHONG")
    of = oracle.Frame(W, H)
    of.clear(*D.CLEAR)
    u = oracle.make_uniforms(model=other.models[0], **kw)
    of.draw(other.item_tris(0), oracle.VS_PHONG, oracle.PS_PHONG, u)
    n_a = int(of.counters.tris_setup)
    per = D.oracle_list_loop(oracle, sc, frame=of)[2]
    n_b = int(of.counters.tris_setup)
    of.draw(other.item_tris(0), oracle.VS_PHONG, oracle.PS_PHONG, oracle.make_uniforms(model=sc.models[1], **kw), tri_id_base=n_b)
    r = _renderer(fr, sc)
    ma = r.upload_mesh(other.item_tris(0), fr.VS_PHONG)
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    r.clear(*D.CLEAR)
    r.set_uniforms(model=other.models[0])
    r.draw(ma, fr.PS_PHONG)
    _assert_ranges(r, [n_a])                                     # a plain pass: one item
    r.draw_list(dl, fr.PS_PHONG)
    _assert_ranges(r, per, base=n_a)
    r.set_uniforms(model=sc.models[1])
    r.draw(ma, fr.PS_PHONG)
    g = _read(r, setup=False)
    _assert_frame(g, of)
    assert g["st"]["tris_setup"] == of.counters.tris_setup and g["st"]["draws"] == 3 and g["st"]["tris_in"] == 2 * other.ntris[0] + sum(sc.ntris)
    r.close()


# ---- the proven-pass rule ----------------------------------------------------------------------------------------------

def _proof_lists():
    """A: two items wholly off-screen, which need no (triangle, tile) record at all; B: the same meshes -- the same item and
    triangle counts -- in view"""
    off = S.clipped_models()[4]
    meshes = [D.Mesh(S.patch(100)), D.Mesh(S.patch(100))]
    a = D.Scene(meshes, [0, 1], np.stack([off, off]), "PHONG", "PHONG")
    b = D.Scene(meshes, [0, 1], S.clipped_models()[[1, 5]], "PHONG", "PHONG")
    return a, b


def test_a_pass_proven_for_one_list_is_verified_again_for_the_list_that_gets_its_id(oracle):
    """Tiny work lists.  List A is drawn until its pass is proven, then freed; list B gets A's id, has A's item and triangle
    counts and needs far more records.  B's frame is consumed through frr_frame_fence only -- no frr_sync, no read-back -- and
    must be whole: B's pass has to be verified (and replayed) although a pass with the same id, counts, uniforms and window is
    proven.  Checked against a build whose DrawSig carried the list's id but not its generation: there B's pass is taken
    for proven, its tile kernel cancels itself and this test fails with B's frame still clear."""
    import torch
    import f_renderer_amd as fr
    from .test_gpu_shade import _Alias
    sa, sb = _proof_lists()
    fa, fb = D.oracle_list_loop(oracle, sa)[0], D.oracle_list_loop(oracle, sb)[0]
    assert (fa.tri_id == NONE).all() and (fb.tri_id != NONE).sum() > 500
    tiny = (("bin_capacity", 64),)
    for sc, overflows in ((sa, False), (sb, True)):                # on a fresh ctx: A fits, B does not
        r = _renderer(fr, sc, tiny)
        g = _list_frame(r, _upload(r, sc, _meshes(r, sc, fr.VS_PHONG)), fr.PS_PHONG, setup=False)
        assert (g["st"]["replays"] >= 1) == overflows, g["st"]
        r.close()
    st = torch.cuda.Stream()
    r = _renderer(fr, sa, tiny, stream=st.cuda_stream)
    meshes = _meshes(r, sa, fr.VS_PHONG)

    def fenced_copy():
        r.frame_fence(st.cuda_stream)
        pc, pd, pt = r.target_ptrs()
        with torch.cuda.stream(st):
            return tuple(torch.as_tensor(_Alias(p, (H, W), ts), device="cuda").clone() for p, ts in ((pc, "<i4"), (pd, "<f4"), (pt, "<i4")))
    copies = []
    la = _upload(r, sa, meshes)
    for _ in range(4):                                             # (the passes alternate between workspace sets)
        r.clear(*D.CLEAR)
        r.draw_list(la, fr.PS_PHONG)
        copies.append((fa, fenced_copy()))
    ida = la.id
    r.free_draw_list(la)
    lb = _upload(r, sb, meshes)
    assert lb.id == ida
    for _ in range(2):
        r.clear(*D.CLEAR)
        r.draw_list(lb, fr.PS_PHONG)
        copies.append((fb, fenced_copy()))
    torch.cuda.synchronize()
    for f, (c, d, t) in copies:
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32).ravel(), f.tri_id)
        np.testing.assert_array_equal(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), f.color)
        assert_depth_equal(d.cpu().numpy(), f.depth)
    r.close()


# ---- culling -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["NEG", "POS"])
@pytest.mark.parametrize("replay", [False, True])
def test_cull_is_evaluated_per_item_under_its_matrices(oracle, mode, replay):
    """a list with a mirrored item under CULL_NEG / CULL_POS == the oracle over the sub-meshes the mode keeps per item; tiny work
    lists: the replay runs under the mode of the call"""
    import f_renderer_amd as fr
    sc = D.scene("mirrored")
    cull = getattr(fr, "CULL_" + mode)
    keep = D.cull_keep(sc, cull)
    assert all(0 < k.sum() < k.size for k in keep)
    of, osetup, per = D.oracle_list_loop(oracle, sc, keep=keep)
    r = _renderer(fr, sc, options=(("bin_capacity", 64),) if replay else ())
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_GOURAUD))
    r.set_cull(cull)
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_COLOR)
    r.set_cull(fr.CULL_NONE)                                       # (a replay must not pick this up)
    g = _read(r)
    _assert_frame(g, of)
    _assert_setup(g["setup"], osetup, 3)
    assert g["st"]["tris_in"] == sum(sc.ntris) and g["st"]["tris_setup"] == sum(per) and g["st"]["frag_covered"] == of.counters.frag_covered
    assert (g["st"]["replays"] > 0) == replay
    _assert_ranges(r, per)
    r.close()


# ---- partition ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocked", [False, True])
def test_partitioned_ranks_stitch_to_the_oracle_frame(oracle, blocked):
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    of, _, per = D.oracle_frame(oracle, "clipped", "DEPTH")
    seen = np.zeros(H, bool)
    for rank in (0, 1):
        r = _renderer(fr, sc)
        r.set_partition(rank, 2, blocked)
        dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
        g = _list_frame(r, dl, fr.PS_DEPTH, setup=False)
        own = owned_pixel_rows(H, rank, 2, blocked)
        assert own.any() and (g["t"].reshape(H, W)[own] != NONE).any()
        _assert_frame(g, of, own)
        seen |= own
        # the filtered setup list serves neither read-back
        n = C.c_uint64()
        assert r._lib.frr_geometry_item_ranges(r._ctx, None, None, 0, C.byref(n)) == fr.FRR_ERR_INVALID
        assert r._lib.frr_readback_setup(r._ctx, None, 0, C.byref(n)) == fr.FRR_ERR_INVALID
        r.clear(*D.CLEAR)
        r.geometry_list(dl)
        r.rasterization((0, W), (0, H), fr.PS_DEPTH)
        _assert_ranges(r, per)
        assert r.setup_triangles().shape[0] == sum(per)
        _assert_frame(_read(r, setup=False), of, own)
        r.close()
    assert seen.all()


# ---- item_ranges -------------------------------------------------------------------------------------------------------

def test_item_ranges_after_instanced_and_plain_passes_and_with_a_small_cap(oracle):
    import f_renderer_amd as fr
    isc = S.scene("clipped")
    per = S.oracle_frame(oracle, "clipped")[2]
    r = _renderer(fr, isc)
    mesh = r.upload_mesh(isc.tris, fr.VS_PHONG)
    n = C.c_uint64()
    assert r._lib.frr_geometry_item_ranges(r._ctx, None, None, 0, C.byref(n)) == fr.FRR_ERR_INVALID     # before any geometry pass
    r.clear(*D.CLEAR)
    r.draw_instanced(mesh, r.upload_instances(isc.models), fr.PS_PHONG)
    _assert_ranges(r, per)                                        # per instance
    _assert_ranges(r, per, cap=2)
    r.set_uniforms(model=isc.models[3])
    r.draw(mesh, fr.PS_PHONG)
    _assert_ranges(r, [per[3]], base=sum(per))                    # a plain pass: one item, behind the instanced pass
    first = np.full(4, 77, np.uint32)
    assert r._lib.frr_geometry_item_ranges(r._ctx, first.ctypes.data, None, 0, C.byref(n)) == fr.FRR_OK and n.value == 1 and (first == 77).all()
    sc = D.scene("empties")
    lper = D.oracle_frame(oracle, "empties")[2]
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    r.clear(*D.CLEAR)
    r.geometry_list(dl)
    for cap in (None, 0, 1, 3, 6, 9):
        _assert_ranges(r, lper, cap=cap)
    r.close()


# ---- the `place` rule --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _place_expected():
    """the place list by the NumPy oracle (which keeps every pixel's interpolated varyings)"""
    sc = D.scene("place")
    kw = S.camera_kw(onp)
    e = SH.render([(sc.item_tris(i), onp.VS_PHONG, onp.Uniforms(model=sc.models[i], **kw)) for i in range(3)], ps=V.zero_ps, size=(W, H), bg=D.CLEAR[0])
    return sc, kw, e


def test_the_place_rule_from_item_ranges(oracle):
    """phong.rs:319-381 as one draw_list(PS_DEPTH) + one resolve + three ranged shades whose cuts -- the reference's `<=` -- come
    from item_ranges: byte for byte the three-draw recipe of INTEGRATION 1d, and the oracle with the texture chosen per setup index"""
    import torch
    import f_renderer_amd as fr
    sc, kw, e = _place_expected()
    texs = D.place_textures()
    n0, n1, n2 = e.n_emit
    cut0, cut1 = n0 + 1, n0 + n1 + 1
    ranges = [(0, cut0), (cut0, cut1 - cut0), (cut1, NONE - cut1)]
    assert all(SH.range_pixels(e, rg) >= 20 for rg in ranges) and (e.tri_id == n0).sum() >= 1
    r = _renderer(fr, sc)
    for slot, tex in enumerate(texs):
        r.set_texture(slot, tex)
    meshes = _meshes(r, sc, fr.VS_PHONG)
    dl = _upload(r, sc, meshes)

    def shade(buf, cuts):
        a, b = cuts
        for slot, (first, count) in enumerate(((0, a), (a, b - a), (b, NONE - b))):
            r.set_uniforms(texture_slot=slot)
            r.shade_varyings(fr.PS_PHONG, buf.data_ptr(), W * H, 8, ids=(first, count))
        r.set_uniforms(texture_slot=0)
    # one list pass
    buf = torch.full((W * H, 8), V.SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), W * H)
    first, count = r.item_ranges()
    assert first.tolist() == [0, n0, n0 + n1] and count.tolist() == [n0, n1, n2]
    shade(buf, (int(first[1]) + 1, int(first[2]) + 1))
    got = _read(r, setup=False)
    V.assert_bits_equal(buf.cpu().numpy(), e.buffer())
    # the three-draw recipe: a resolve and a count read-back after each draw
    buf3 = torch.full((W * H, 8), V.SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.clear(*D.CLEAR)
    ns = []
    for i in range(3):
        r.set_uniforms(model=sc.models[i])
        r.draw(meshes[i], fr.PS_DEPTH)
        r.resolve_varyings(buf3.data_ptr(), W * H)
        ns.append(r.stats()["tris_setup"])
    shade(buf3, (ns[0] + 1, ns[1] + 1))
    got3 = _read(r, setup=False)
    for k in "tc":
        np.testing.assert_array_equal(got[k], got3[k])
    np.testing.assert_array_equal(got["d"].view(np.uint32), got3["d"].view(np.uint32))
    np.testing.assert_array_equal(got["t"], e.tri_id)
    assert_depth_equal(got["d"], e.depth)
    want = SH.shaded(e, [(onp.PS_PHONG, SH.oracle_uniforms(kw, texs[k]), ranges[k]) for k in range(3)], start=SH.background((W, H), D.CLEAR[0]))
    np.testing.assert_array_equal(got["c"], want)
    # the boundary triangle (emission index n0, the first of item 1) carries item 0's texture
    edge = np.nonzero(e.tri_id == n0)[0]
    alt = SH.shaded(e, [(onp.PS_PHONG, SH.oracle_uniforms(kw, texs[1]), (n0, 1))], start=want.copy())
    assert (alt.reshape(-1, 4)[edge] != want.reshape(-1, 4)[edge]).any()
    r.close()


# ---- downstream consumers ----------------------------------------------------------------------------------------------

def test_wireframe_after_a_list_pass(oracle):
    """draw_wireframe of the list's setup list == tests/lines_reference.py over the read-back setup list"""
    import f_renderer_amd as fr
    from . import lines_reference as R
    sc = D.scene("clipped")
    of, osetup, _ = D.oracle_frame(oracle, "clipped")
    color = (255, 200, 0, 255)
    r = _renderer(fr, sc)
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_PHONG)
    r.draw_wireframe(color)
    c, d, t = r.readback()
    setup = r.setup_triangles()
    np.testing.assert_array_equal(setup["spi"], osetup["spi"])
    segs, skipped = [], 0
    for tri in setup["spi"]:
        for k in range(3):
            (xa, ya), (xb, yb) = tri[k], tri[(k + 1) % 3]
            if 0 <= xa < W and 0 <= xb < W and 0 <= ya < H and 0 <= yb < H:
                segs.append((xa, ya, xb, yb))
            else:
                skipped += 1
    xyxy = np.array(segs, np.uint32).reshape(-1, 4)
    assert skipped > 0 and len(xyxy) > 0
    np.testing.assert_array_equal(t, of.tri_id)
    assert_depth_equal(d, of.depth)
    np.testing.assert_array_equal(c, R.draw_lines(of.color.copy(), xyxy, np.tile(np.array(color, np.uint8), (len(xyxy), 1))))
    r.close()


def test_resolve_varyings_after_a_list_pass():
    import torch
    import f_renderer_amd as fr
    sc, kw, e = _place_expected()
    r = _renderer(fr, sc)
    buf = torch.full((W * H, 8), V.SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.clear(*D.CLEAR)
    r.geometry_list(_upload(r, sc, _meshes(r, sc, fr.VS_PHONG)))
    r.rasterization((0, W), (0, H), fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), W * H)
    c, d, t = r.readback()
    np.testing.assert_array_equal(t, e.tri_id)
    assert_depth_equal(d, e.depth)
    V.assert_bits_equal(buf.cpu().numpy(), e.buffer())
    r.close()


# ---- lifetime and errors -----------------------------------------------------------------------------------------------

def test_freeing_a_named_mesh_kills_the_list_for_good(oracle):
    import f_renderer_amd as fr
    sc = D.scene("one")
    of = D.oracle_frame(oracle, "one")[0]
    r = _renderer(fr, sc)
    L, ctx = r._lib, r._ctx
    keep, gone = r.upload_mesh(sc.item_tris(0), fr.VS_PHONG), r.upload_mesh(S.patch(9), fr.VS_PHONG)
    models = np.stack([sc.models[0], sc.models[0]])
    dl, other = r.upload_draw_list([keep, gone], models), r.upload_draw_list([keep], sc.models)
    _list_frame(r, dl, fr.PS_PHONG, setup=False)
    gid = gone.id
    gone.free()
    assert L.frr_draw_list(ctx, dl.id, fr.PS_PHONG, 0, W, 0, H) == fr.FRR_ERR_INVALID and "freed" in _err(r)
    assert L.frr_geometry_list(ctx, dl.id, None) == fr.FRR_ERR_INVALID
    again = r.upload_mesh(S.patch(9), fr.VS_PHONG)
    assert again.id == gid                                          # the id is reused ...
    assert L.frr_draw_list(ctx, dl.id, fr.PS_PHONG, 0, W, 0, H) == fr.FRR_ERR_INVALID   # ... and the list stays dead
    _assert_frame(_list_frame(r, other, fr.PS_PHONG, setup=False), of)                # a list that does not name it lives on
    lid = dl.id
    r.free_draw_list(dl)                                            # freeing a dead list still works
    assert L.frr_drawlist_free(ctx, lid) == fr.FRR_ERR_INVALID      # a double free
    r.close()


def test_errors_leave_the_ctx_drawing(oracle):
    import torch
    import f_renderer_amd as fr
    from f_renderer_amd import _native
    sc = D.scene("one")
    of = D.oracle_frame(oracle, "one")[0]
    r = _renderer(fr, sc)
    L, ctx = r._lib, r._ctx
    mesh = r.upload_mesh(sc.item_tris(0), fr.VS_PHONG)
    lid = C.c_int(-7)
    assert L.frr_drawlist_upload(ctx, None, 2, C.byref(lid)) == fr.FRR_ERR_INVALID and lid.value == -7               # NULL, nitems > 0
    with pytest.raises(fr.FrrError) as e:
        r.upload_draw_list([mesh], sc.models, reserved=1)
    assert e.value.code == fr.FRR_ERR_INVALID and "item 0" in str(e.value)
    item = (_native.DrawItem * 1)()
    item[0].mesh = 99
    assert L.frr_drawlist_upload(ctx, C.cast(item, C.c_void_p), 1, C.byref(lid)) == fr.FRR_ERR_INVALID and lid.value == -7   # unknown mesh
    for bad in (-1, 99):
        assert L.frr_draw_list(ctx, bad, fr.PS_PHONG, 0, W, 0, H) == fr.FRR_ERR_INVALID
        assert L.frr_geometry_list(ctx, bad, None) == fr.FRR_ERR_INVALID
        assert L.frr_drawlist_free(ctx, bad) == fr.FRR_ERR_INVALID
    # the order-key limit on the sum: one device-bound VS_CLIP mesh of 2^24 triangles (registered, never drawn); eight items that
    # name it are 2^27 inputs -- refused at upload, before anything is allocated -- seven upload fine
    big = torch.empty((1 << 24) * 12, dtype=torch.float32, device="cuda")
    bm = r.bind_mesh_device(big.data_ptr(), 1 << 24, fr.VS_CLIP, keepalive=big)
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(16), (8, 1))
    with pytest.raises(fr.FrrError) as e:
        r.upload_draw_list([bm] * 8, eye)
    assert e.value.code == fr.FRR_ERR_UNSUPPORTED
    seven = r.upload_draw_list([bm] * 7, eye[:7])
    assert seven.ntris == 7 << 24
    r.free_draw_list(seven)
    bm.free()
    del big
    _assert_frame(_list_frame(r, r.upload_draw_list([mesh], sc.models), fr.PS_PHONG, setup=False), of)
    r.close()


def test_cpp_host_draws_a_list(tmp_path):
    """frr::Renderer::upload_draw_list + geometry_list + item_ranges (frr_renderer.hpp; examples/phong_headless --list): the
    compiled host's list frame is its own instanced frame of the same objects, byte for byte"""
    import os
    import subprocess
    import f_renderer_amd as fr
    from f_renderer_amd.assets import Model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s", "phong_headless"])
    obj, tga = (os.path.join(root, "tests", "golden", n) for n in ("cube.obj", "checker24.tga"))
    n, ntris = 9, Model(obj).indexed_inputs()[1].shape[0]
    outs = []
    for k, extra in enumerate((["--list"], [])):
        op = str(tmp_path / ("out%d.rgba" % k))
        out = subprocess.run([os.path.join(root, "examples", "phong_headless"), "--assets", obj, tga, "320", "180", op, "--instances", str(n)] + extra,
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        outs.append((out.stdout, np.fromfile(op, np.uint8)))
    assert "list: n=%d tris_in=%d last_first=%d" % (n, n * ntris, (n - 1) * ntris) in outs[0][0]
    assert outs[0][1].size == 320 * 180 * 4 and np.unique(outs[0][1].reshape(-1, 4), axis=0).shape[0] > 50
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
