"""Box queries on the device: frr_drawlist_bounds against NumPy's min / max, and frr_query_boxes / frr_query_boxes_host
against the host build of the rule (frr_host_query_boxes) on the frame's read-back depth and against the NumPy restatement of
tests/box_reference.py, byte for byte.  Frames are those of tests/drawlist_scenes.py, 128 x 96: four tile columns, three tile
rows."""
import numpy as np
import pytest

from . import box_reference as R
from . import box_scenes as B
from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import predicate_scenes as P
from .conftest import assert_depth_equal
from .test_gpu_drawlist import _err, _meshes, _phong_sid, _renderer, _upload
from .test_gpu_query import SENTINEL, STAT_KEYS, _buffer, _fenced

pytestmark = pytest.mark.gpu
W, H = B.W, B.H
WG_SHARE = 1024          # triangles per workgroup and step of the bounds kernel (frr_boxes.h: BOX_WG_TRIS)
BOUNDS_SIZES = [1, 63, 64, 65, 255, 256, 257, 3 * WG_SHARE + 7]


def _list(fr, sc, r=None, kinds=None, options=(), stream=None):
    r = r or _renderer(fr, sc, options=options, stream=stream)
    dl = _upload(r, sc, _meshes(r, sc, getattr(fr, "VS_" + sc.vs), kinds))
    return r, dl


def _assert_bounds(r, dl, sc):
    lo_hi, flags = r.list_bounds(dl)
    want_b, want_f = B.bounds(sc)
    np.testing.assert_array_equal(flags, want_f)
    ok = want_f == 0
    np.testing.assert_array_equal(lo_hi[ok].view(np.uint32), want_b[ok].view(np.uint32))
    return lo_hi, flags


def _with_cover(fr, sc, options=(), stream=None, clear=D.CLEAR):
    """a ctx with the cover drawn (depth only) and the scene's list uploaded with its bounds"""
    r, dl = _list(fr, sc, options=options, stream=stream)
    _, cover = _list(fr, B.cover_scene(), r=r)
    _assert_bounds(r, dl, sc)
    r.clear(*clear)
    r.draw_list(cover, fr.PS_DEPTH)
    return r, dl, cover


def _expected(fr, sc, depth, window=B.FULL, mask=None, entries=None):
    """the restatement and the library's host build over `depth`, which agree"""
    lo_hi, flags = B.bounds(sc)
    m = B.mvps(sc)
    want, _ = R.query(m, lo_hi, flags, (W, H), window, depth, mask, entries)
    host, _ = fr.host_query_boxes(m, lo_hi, flags, (W, H), window, depth, mask, entries)
    np.testing.assert_array_equal(host, want)
    return want


def _assert_query(fr, r, dl, sc, window=B.FULL, mask=None, depth=None):
    """host form, device form with a tail of three entries and one entry short, against the rule over the read-back depth"""
    d = r.readback()[1] if depth is None else depth
    n = sc.nitems
    want = _expected(fr, sc, d, window, mask)
    got = r.query_boxes(dl, window=window)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, want)
    big, small = _buffer(n + 3), _buffer(max(n - 1, 1))
    r.query_boxes(dl, out_ptr=big.data_ptr(), entries=n + 3, window=window)
    if n > 1:
        r.query_boxes(dl, out_ptr=small.data_ptr(), entries=n - 1, window=window)
    gb, gs = _fenced(r, [big, small])
    np.testing.assert_array_equal(gb[:n + 3], np.concatenate([want, [0, 0, 0]]))
    if n > 1:
        np.testing.assert_array_equal(gs[:n - 1], want[:-1])        # a unit >= out_entries is written nowhere
    return want


# ---- 1. bounds ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunks", [0, 1, 2])
def test_bounds_of_meshes_around_the_wave_and_the_workgroup_share(chunks):
    """chunks: option box_bounds_chunks -- with 1 and 2 workgroups per mesh the largest mesh takes four and two trips of the
    kernel's stride loop"""
    import f_renderer_amd as fr
    meshes = [D.Mesh(S.patch(n) * np.float32(1 + 0.1 * k) - np.float32(0.01 * k)) for k, n in enumerate(BOUNDS_SIZES)]
    sc = D.Scene(meshes, range(len(meshes)), S.grid_models(len(meshes)), "PHONG", "PHONG")
    r, dl = _list(fr, sc, options=(("box_bounds_chunks", chunks),))
    a = _assert_bounds(r, dl, sc)
    b = _assert_bounds(r, dl, sc)                                   # a second call computes it again: the same bytes
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    r.close()


def test_bounds_of_an_indexed_mesh_ignore_an_unreferenced_vertex_and_device_bound_meshes():
    import f_renderer_amd as fr
    v, f = S.patch_grid(5, 3)
    outlier = np.zeros((1, v.shape[1]), np.float32)
    outlier[0, :3] = (900.0, -700.0, 1.0e6)
    v2 = np.ascontiguousarray(np.concatenate([v[:7], outlier, v[7:]]), np.float32)
    f2 = np.ascontiguousarray(np.where(f >= 7, f + 1, f), np.uint32)
    tris = np.ascontiguousarray(v2[f2.astype(np.int64)])
    assert np.abs(tris[:, :, :3]).max() < 100
    meshes = [D.Mesh(tris, indexed=(v2, f2)), D.Mesh(S.patch(100)), D.Mesh(tris, indexed=(v2, f2)), D.Mesh(S.patch(300))]
    sc = D.Scene(meshes, [0, 1, 2, 3, 1], S.grid_models(5), "GOURAUD", "COLOR")
    r, dl = _list(fr, sc, kinds=["indexed", "dev", "dev_indexed", "plain"])
    _assert_bounds(r, dl, sc)
    r.close()


def test_bounds_flags_nan_inf_and_empty_meshes():
    import f_renderer_amd as fr
    nan, inf = S.patch(70).copy(), S.patch(130).copy()
    nan[69, 2, 1] = np.nan
    inf[3, 0, 2] = -np.inf
    meshes = [D.Mesh(S.patch(9)), D.Mesh(nan), D.empty(), D.Mesh(inf)]
    sc = D.Scene(meshes, [0, 1, 2, 3, 2, 0], S.grid_models(6), "PHONG", "PHONG")
    r, dl = _list(fr, sc)
    _, flags = _assert_bounds(r, dl, sc)
    assert flags.tolist() == [0, 1, 2, 1, 2, 0]
    r.clear(*D.CLEAR)
    np.testing.assert_array_equal(r.query_boxes(dl) == 0, [False, False, True, False, True, False])   # a non-finite box is unbounded, an empty mesh nothing
    assert r.query_boxes(dl)[1] == W * H
    r.close()


def test_bounds_of_257_items_over_three_meshes_and_of_no_items():
    import f_renderer_amd as fr
    meshes = [D.Mesh(S.patch(5)), D.Mesh(S.patch(64) * np.float32(2)), D.Mesh(S.patch(700) + np.float32(0.25))]
    which = [(i * 7 + i // 5) % 3 for i in range(257)]
    sc = D.Scene(meshes, which, np.tile(S.grid_models(1), (257, 1)), "PHONG", "PHONG")
    r, dl = _list(fr, sc)
    _assert_bounds(r, dl, sc)
    none = D.Scene([D.Mesh(S.patch(5))], [], np.zeros((0, 16), np.float32), "PHONG", "PHONG")
    _, dl0 = _list(fr, none, r=r)
    lo_hi, flags = r.list_bounds(dl0)
    assert lo_hi.shape == (0, 6) and flags.size == 0
    r.clear(*D.CLEAR)
    b = _buffer(3)
    r.query_boxes(dl0, out_ptr=b.data_ptr(), entries=3)
    np.testing.assert_array_equal(_fenced(r, [b])[0][:3], [0, 0, 0])
    r.close()


def test_errors():
    import f_renderer_amd as fr
    sc = B.scene("clipped")
    r, dl = _list(fr, sc)
    r.clear(*D.CLEAR)
    b = _buffer(sc.nitems)
    with pytest.raises(fr.FrrError) as e:                           # no table yet
        r.query_boxes(dl, out_ptr=b.data_ptr(), entries=sc.nitems)
    assert e.value.code == fr.FRR_ERR_INVALID and "frr_drawlist_bounds" in _err(r)
    r.list_bounds(dl)
    for win in ((0, W + 1, 0, H), (5, 5, 0, H), (0, W, 9, 3), (0, 40000, 0, H)):
        with pytest.raises(fr.FrrError) as e:
            r.query_boxes(dl, window=win)
        assert e.value.code == fr.FRR_ERR_INVALID, win
    with pytest.raises(fr.FrrError) as e:
        r.query_boxes(dl, window=(-1, W - 1, 0, H))
    assert e.value.code == fr.FRR_ERR_UNSUPPORTED
    with pytest.raises(fr.FrrError) as e:
        r.query_boxes(dl, out_ptr=b.data_ptr() + 2, entries=2)
    assert e.value.code == fr.FRR_ERR_INVALID
    assert r._lib.frr_query_boxes(r._ctx, dl.id, 0, W, 0, H, None, 0) == fr.FRR_OK      # no entries: nothing happens
    clip = D.scene("clip_vs")                                       # FRR_VS_CLIP inputs: no object space
    _, dlc = _list(fr, clip, r=r)
    with pytest.raises(fr.FrrError) as e:
        r.list_bounds(dlc)
    assert e.value.code == fr.FRR_ERR_UNSUPPORTED and "clip coordinates" in _err(r)
    with pytest.raises(fr.FrrError) as e:                           # ... and no table was stored
        r.query_boxes(dlc)
    assert e.value.code == fr.FRR_ERR_INVALID
    for bad in (-1, 99):
        assert r._lib.frr_query_boxes(r._ctx, bad, 0, W, 0, H, b.data_ptr(), 1) == fr.FRR_ERR_INVALID
        assert r._lib.frr_drawlist_bounds(r._ctx, bad, None, None, 0, None) == fr.FRR_ERR_INVALID
    # a list under a user vertex shader: it may move a vertex anywhere
    sid = _phong_sid()
    um = r.upload_mesh(sc.meshes[0].tris, sid)
    dlu = r.upload_draw_list([um] * 2, sc.models[:2])
    with pytest.raises(fr.FrrError) as e:
        r.list_bounds(dlu)
    assert e.value.code == fr.FRR_ERR_UNSUPPORTED and "user vertex shader" in _err(r)
    with pytest.raises(fr.FrrError) as e:                           # ... and no table was stored
        r.query_boxes(dlu)
    assert e.value.code == fr.FRR_ERR_INVALID and "frr_drawlist_bounds" in _err(r)
    # a dead list -- one of its meshes was freed -- with and without a table
    dm = [r.upload_mesh(sc.meshes[0].tris, fr.VS_PHONG) for _ in range(2)]
    dead_with, dead_without = r.upload_draw_list(dm, sc.models[:2]), r.upload_draw_list(dm[:1], sc.models[:1])
    r.list_bounds(dead_with)
    dm[0].free()
    for dead in (dead_with, dead_without):
        with pytest.raises(fr.FrrError) as e:
            r.list_bounds(dead)
        assert e.value.code == fr.FRR_ERR_INVALID and "dead" in _err(r)
        with pytest.raises(fr.FrrError) as e:
            r.query_boxes(dead, out_ptr=b.data_ptr(), entries=1)
        assert e.value.code == fr.FRR_ERR_INVALID and "dead" in _err(r)
        with pytest.raises(fr.FrrError) as e:
            r.query_boxes(dead)
        assert e.value.code == fr.FRR_ERR_INVALID
    with pytest.raises(fr.FrrError):
        r.set_option("box_bounds_chunks", 1025)
    lid = dl.id
    r.free_draw_list(dl)
    assert r._lib.frr_query_boxes(r._ctx, lid, 0, W, 0, H, b.data_ptr(), 1) == fr.FRR_ERR_INVALID
    assert r._lib.frr_drawlist_bounds(r._ctx, lid, None, None, 0, None) == fr.FRR_ERR_INVALID
    # a refused call leaves the ctx drawing
    r2, dl2, cover = _with_cover(fr, B.scene("prototype"))
    with pytest.raises(fr.FrrError):
        r2.query_boxes(dl2, window=(0, W + 1, 0, H))
    _assert_query(fr, r2, dl2, B.scene("prototype"))
    r.close()
    r2.close()


# ---- 2. the command ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", B.NAMES)
def test_scenes_and_windows(oracle, name):
    import f_renderer_amd as fr
    sc = B.scene(name)
    r, dl, _ = _with_cover(fr, sc)
    d = r.readback()[1]
    assert_depth_equal(d, B.cover_depth(oracle))
    st0 = r.stats()
    c0, _, t0 = r.readback()
    for win in B.WINDOWS:
        _assert_query(fr, r, dl, sc, window=win, depth=d)
    c1, d1, t1 = r.readback()                                       # colour, depth, ids and the statistics are untouched
    np.testing.assert_array_equal(c0, c1)
    np.testing.assert_array_equal(t0, t1)
    np.testing.assert_array_equal(d.view(np.uint32), d1.view(np.uint32))
    st1 = r.stats()
    assert all(st0[k] == st1[k] for k in STAT_KEYS + ("replays",)), (st0, st1)
    r.close()


def test_special_depths_through_the_depth_target(oracle):
    """NaN, -0.0 and +-inf entries in the depth the command reads: caller-bound targets filled by the caller"""
    import torch
    import f_renderer_amd as fr
    sc = B.scene("prototype")
    r, dl = _list(fr, sc)
    r.list_bounds(dl)
    for name, dd in B.special_depths(oracle).items():
        col, ids = torch.zeros((H, W), dtype=torch.int32, device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda")
        dep = torch.from_numpy(dd.reshape(H, W).copy()).to("cuda")
        torch.cuda.synchronize()
        r.bind_targets(col.data_ptr(), dep.data_ptr(), ids.data_ptr())
        want = _expected(fr, sc, dd)
        np.testing.assert_array_equal(r.query_boxes(dl), want, err_msg=name)
        np.testing.assert_array_equal(r.query_boxes(dl, window=(3, 125, 5, 91)), _expected(fr, sc, dd, (3, 125, 5, 91)), err_msg=name)
        r.sync()
    r.close()


def test_a_translation_by_a_million_where_the_matrix_is_composed_under_cancellation(oracle):
    """the moved camera through set_uniforms, the two far models as a list: the device composes (proj * view) * model itself,
    and its answer is the host build's and the restatement's over the same matrices, byte for byte"""
    import f_renderer_amd as fr
    sc, proj, view, eye = B.far_scene()
    r = _renderer(fr, sc)
    r.set_uniforms(view=view, proj=proj, view_pos=eye)
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    _, cover = _list(fr, B.cover_scene(), r=r)
    _assert_bounds(r, dl, sc)
    m, lo_hi, flags = B.far_translation()
    for k in range(sc.nitems):                                      # the library's own host composition is the restatement's
        np.testing.assert_array_equal(fr.host_instance_mvp(proj, view, sc.models[k]).view(np.uint32), m[k].view(np.uint32))
    depths = [np.full(W * H, D.CLEAR[1], np.float32), np.full(W * H, 0.3, np.float32), np.full(W * H, 0.36, np.float32), B.cover_depth(oracle)]
    seen = set()
    for d, clear in zip(depths, (D.CLEAR[1], 0.3, 0.36, None)):
        if clear is None:                                           # the cover, drawn under the demo camera
            r.set_uniforms(**S.camera_kw(fr))
            r.clear(*D.CLEAR)
            r.draw_list(cover, fr.PS_DEPTH)
            r.set_uniforms(view=view, proj=proj, view_pos=eye)
            assert_depth_equal(r.readback()[1], d)
        else:
            r.clear(D.CLEAR[0], clear)
        for win in (B.FULL, (3, 125, 5, 91)):
            want, srl = R.query(m, lo_hi, flags, (W, H), win, d)
            host, _ = fr.host_query_boxes(m, lo_hi, flags, (W, H), win, d)
            np.testing.assert_array_equal(host, want)
            np.testing.assert_array_equal(r.query_boxes(dl, window=win), want, err_msg=str((clear, win)))
            b = _buffer(sc.nitems)
            r.query_boxes(dl, out_ptr=b.data_ptr(), entries=sc.nitems, window=win)
            np.testing.assert_array_equal(_fenced(r, [b])[0][:sc.nitems], want)
            seen |= {int(v) for v in srl[:, 0]}
    assert seen >= {R.HIDDEN, R.KEPT}, seen
    r.close()


@pytest.mark.parametrize("size", [(700, 500), (32767, 40)])
def test_larger_frames_use_the_pyramid_levels_above_the_tile(size):
    """the 128 x 96 frame ends at level 5, one cell per tile; these frames need levels up to 8 and 13 (k_box_top), with extents that
    are no multiples of a tile.  The depth is the caller's: a ramp along x under noise, so that the verdicts differ along the frame."""
    import torch
    import f_renderer_amd as fr
    Wb, Hb = size
    sc = B.scene("prototype")
    r = fr.Renderer(Wb, Hb)
    r.set_uniforms(**S.camera_kw(fr))
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    r.list_bounds(dl)
    rng = np.random.default_rng(20261021)
    d = (0.15 + 0.35 * np.arange(Wb, dtype=np.float32)[None, :] / Wb + 0.02 * rng.random((Hb, Wb), dtype=np.float32)).astype(np.float32)
    col, ids = torch.zeros((Hb, Wb), dtype=torch.int32, device="cuda"), torch.zeros((Hb, Wb), dtype=torch.int32, device="cuda")
    dep = torch.from_numpy(d).to("cuda")
    torch.cuda.synchronize()
    r.bind_targets(col.data_ptr(), dep.data_ptr(), ids.data_ptr())
    lo_hi, flags = B.bounds(sc)
    m = B.mvps(sc)
    levels = set()
    for win in ((0, Wb, 0, Hb), (3, Wb - 2, 5, Hb - 1), (Wb // 2 - 65, Wb // 2 + 66, Hb // 2 - 16, Hb // 2 + 17)):
        want, srl = R.query(m, lo_hi, flags, size, win, d.reshape(-1))
        host, _ = fr.host_query_boxes(m, lo_hi, flags, size, win, d.reshape(-1))
        np.testing.assert_array_equal(host, want)
        np.testing.assert_array_equal(r.query_boxes(dl, window=win), want, err_msg=str(win))
        levels |= {int(v[5]) for v in srl if v[0] in (R.HIDDEN, R.KEPT)}
        if win[1] - win[0] > 200:
            assert (srl[:, 0] == R.HIDDEN).any() and (srl[:, 0] == R.KEPT).any(), srl[:, 0]
    assert max(levels) >= (12 if Wb > 30000 else 7), levels           # the rectangles read the levels built above the tile's, to the top
    r.sync()
    r.close()


@pytest.mark.parametrize("clear_depth", [0.25, float("nan")])
def test_clear_depths_a_pending_clear_and_two_passes(oracle, clear_depth):
    import f_renderer_amd as fr
    sc = B.scene("prototype")
    r, dl, cover = _with_cover(fr, sc, clear=(D.CLEAR[0], clear_depth))
    want = _assert_query(fr, r, dl, sc)
    # a pending clear: nothing has been drawn yet, the query settles it first
    r.clear(D.CLEAR[0], clear_depth)
    b = _buffer(sc.nitems)
    r.query_boxes(dl, out_ptr=b.data_ptr(), entries=sc.nitems)
    got = _fenced(r, [b])[0][:sc.nitems]
    np.testing.assert_array_equal(got, _expected(fr, sc, np.full(W * H, clear_depth, np.float32)))
    assert_depth_equal(r.readback()[1], np.full(W * H, clear_depth, np.float32))
    # after two passes in a frame
    _, hid = _list(fr, P.scene("hidden"), r=r)
    r.draw_list(cover, fr.PS_DEPTH)
    r.draw_list(hid, fr.PS_DEPTH)
    after = _assert_query(fr, r, dl, sc)
    assert want.shape == after.shape
    r.close()


def test_stream_order_a_later_occluder_is_not_seen(oracle):
    import f_renderer_amd as fr
    sc = B.scene("prototype")
    r, dl = _list(fr, sc)
    _, cover = _list(fr, B.cover_scene(), r=r)
    r.list_bounds(dl)
    n = sc.nitems
    cleared = np.full(W * H, D.CLEAR[1], np.float32)
    before, behind = _expected(fr, sc, cleared), _expected(fr, sc, B.cover_depth(oracle))
    assert (before != behind).any()
    r.clear(*D.CLEAR)
    b0, b1 = _buffer(n), _buffer(n)
    r.query_boxes(dl, out_ptr=b0.data_ptr(), entries=n)
    r.draw_list(cover, fr.PS_DEPTH)                                 # occludes, behind the first query
    r.query_boxes(dl, out_ptr=b1.data_ptr(), entries=n)
    g0, g1 = _fenced(r, [b0, b1])
    np.testing.assert_array_equal(g0[:n], before)
    np.testing.assert_array_equal(g1[:n], behind)
    r.close()


@pytest.mark.parametrize("fif", [1, 2])
def test_frames_in_flight_are_tested_against_their_own_depth(oracle, fif):
    import f_renderer_amd as fr
    sc = B.scene("prototype")
    r, dl = _list(fr, sc, options=(("frames_in_flight", fif),))
    _, cover = _list(fr, B.cover_scene(), r=r)
    _, hid = _list(fr, P.scene("hidden"), r=r)
    r.list_bounds(dl)
    n = sc.nitems
    occs = [cover, hid, None, cover]
    depths = [B.cover_depth(oracle), D.oracle_list_loop(oracle, P.scene("hidden"), "DEPTH")[0].depth, np.full(W * H, D.CLEAR[1], np.float32), B.cover_depth(oracle)]
    bufs = [_buffer(n) for _ in occs]
    for occ, b in zip(occs, bufs):                                  # no host wait between the frames
        r.clear(*D.CLEAR)
        if occ is not None:
            r.draw_list(occ, fr.PS_DEPTH)
        r.query_boxes(dl, out_ptr=b.data_ptr(), entries=n)
    for g, d in zip(_fenced(r, bufs), depths):
        np.testing.assert_array_equal(g[:n], _expected(fr, sc, d))
    r.close()


def test_caller_bound_targets_two_in_flight(oracle):
    import torch
    import f_renderer_amd as fr
    st = torch.cuda.Stream()
    sc = B.scene("prototype")
    r, dl = _list(fr, sc, options=(("bound_targets_in_flight", 1),), stream=st.cuda_stream)
    _, cover = _list(fr, B.cover_scene(), r=r)
    _, hid = _list(fr, P.scene("hidden"), r=r)
    r.list_bounds(dl)
    sets = [tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32)) for _ in range(2)]
    torch.cuda.synchronize()
    n = sc.nitems
    bufs = [_buffer(n), _buffer(n)]
    for k, occ in enumerate((cover, hid)):
        r.frame_wait(st.cuda_stream)
        r.bind_targets(*(x.data_ptr() for x in sets[k]))
        r.clear(*D.CLEAR)
        r.draw_list(occ, fr.PS_DEPTH)
        r.query_boxes(dl, out_ptr=bufs[k].data_ptr(), entries=n)
    got = _fenced(r, bufs)
    np.testing.assert_array_equal(got[0][:n], _expected(fr, sc, B.cover_depth(oracle)))
    np.testing.assert_array_equal(got[1][:n], _expected(fr, sc, D.oracle_list_loop(oracle, P.scene("hidden"), "DEPTH")[0].depth))
    r.close()


def test_behind_a_failed_pass_it_writes_nothing_and_is_replayed_with_it(oracle):
    """an open geometry pass whose fans do not fit the tiny fan space fails on the device -- flagged where the first command that
    reads the pass scans its block sums, here a visible_pixels; the box query behind that is cancelled -- the buffer keeps the
    sentinel -- and runs again with the replay at the next synchronisation point"""
    import f_renderer_amd as fr
    sc = B.scene("prototype")
    assert sum(D.oracle_frame(oracle, "clipped", "DEPTH")[2]) > sum(D.scene("clipped").ntris) + 16
    r, dl, _ = _with_cover(fr, sc, options=(("fan_capacity", 16), ("bin_capacity", 64)))
    _, fails = _list(fr, D.scene("clipped"), r=r)
    r.sync()
    replays = r.stats()["replays"]
    n = sc.nitems
    b = _buffer(n)
    v = _buffer(D.scene("clipped").nitems)
    r.geometry_list(fails)                                          # left open: nothing verifies it
    r.visible_pixels("item", out_ptr=v.data_ptr(), entries=D.scene("clipped").nitems)   # reads the pass: its scan flags the failure
    r.query_boxes(dl, out_ptr=b.data_ptr(), entries=n)
    np.testing.assert_array_equal(_fenced(r, [b])[0][:n], np.full(n, SENTINEL, np.uint32))
    r.sync()
    assert r.stats()["replays"] > replays
    np.testing.assert_array_equal(_fenced(r, [b])[0][:n], _expected(fr, sc, B.cover_depth(oracle)))
    r.close()


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("rank", [0, 1])
def test_partition_world_two_is_the_ranks_own_answer(oracle, rank, blocked):
    import f_renderer_amd as fr
    sc = B.scene("prototype")
    r, dl = _list(fr, sc)
    _, cover = _list(fr, B.cover_scene(), r=r)
    r.list_bounds(dl)
    r.set_partition(rank, 2, blocked)
    r.clear(*D.CLEAR)
    r.geometry_list(cover)
    r.rasterization((0, W), (0, H), fr.PS_DEPTH)
    mask = B.ROW_MASKS[(rank, blocked)]
    # (window-local tile rows: three of them in the first two windows, one -- rank 0's in both layouts -- in the third)
    for win, wmask in ((B.FULL, mask), ((3, 125, 5, 91), mask), ((0, W, 40, 60), [1 if rank == 0 else 0])):
        _assert_query(fr, r, dl, sc, window=win, mask=wmask)
    r.close()


def test_two_runs_give_the_same_bytes(oracle):
    import f_renderer_amd as fr
    sc = B.scene("prototype")
    outs = []
    for _ in range(2):
        r, dl, _ = _with_cover(fr, sc)
        outs.append(r.query_boxes(dl, entries=sc.nitems + 2).tobytes())
        r.close()
    assert outs[0] == outs[1]


# ---- 3. end to end -----------------------------------------------------------------------------------------------------

def test_query_then_draw_what_it_keeps_equals_drawing_everything(oracle):
    """clear; draw the cover; query_boxes(items) -> buf; draw_list_if(items, buf): colour and depth are the oracle's loop over
    all items, and what each item then owns is at most what the query promised"""
    import f_renderer_amd as fr
    sc = B.scene("prototype")
    r, dl = _list(fr, sc)
    _, cover = _list(fr, B.cover_scene(), r=r)
    r.list_bounds(dl)
    n = sc.nitems
    buf = _buffer(n)
    r.clear(*D.CLEAR)
    r.draw_list(cover, fr.PS_PHONG)
    r.query_boxes(dl, out_ptr=buf.data_ptr(), entries=n)
    r.draw_list_if(dl, buf.data_ptr(), n, fr.PS_PHONG)
    c, d, _ = r.readback()
    owned = r.visible_pixels("item")
    f, _, _ = D.oracle_list_loop(oracle, B.cover_scene(), "PHONG")
    f, _, _ = D.oracle_list_loop(oracle, sc, "PHONG", frame=f)
    np.testing.assert_array_equal(c, f.color)
    assert_depth_equal(d, f.depth)
    promised = _fenced(r, [buf])[0][:n]
    assert (promised == 0).sum() >= 8 and (owned <= promised).all(), (owned, promised)
    r.close()
