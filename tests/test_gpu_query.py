"""Occlusion queries on the device (frr_query_pixels / frr_query_pixels_host): the fragments of the latest geometry pass that
pass the depth test against the depth target as it stands, per item or per triangle, with nothing drawn.  Every expected
value is an exact integer of tests/query_reference.py: per setup triangle, the entries that the oracle's rasterization of that
triangle alone changes on a copy of the depth.  Frames are those of tests/drawlist_scenes.py, 128 x 96: four tile columns and
three tile rows; option visible_lds_bins = 1 sends the per-item adds to global memory."""
import ctypes as C

import numpy as np
import pytest

from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import predicate_scenes as P
from . import query_reference as Q
from .conftest import assert_depth_equal, owned_pixel_rows
from .test_gpu_drawlist import _assert_frame, _err, _meshes, _phong_sid, _read, _renderer, _upload

pytestmark = pytest.mark.gpu
W, H = D.W, D.H
SENTINEL = 0x5A5A5A5A
PATHS = [0, 1]     # visible_lds_bins: the LDS histogram, and 1 (every pass with more than one item adds to global memory)
TINY = (("fan_capacity", 16), ("bin_capacity", 64))
STAT_KEYS = ("tris_in", "tris_setup", "bin_entries", "frag_covered", "frag_nan", "draws")


def _setup(fr, name, options=(), kinds=None, vs_id=None, stream=None, r=None):
    sc = P.scene(name)
    r = r or _renderer(fr, sc, options=options, stream=stream)
    dl = _upload(r, sc, _meshes(r, sc, getattr(fr, "VS_" + sc.vs) if vs_id is None else vs_id, kinds))
    return sc, r, dl


def _buffer(entries, value=SENTINEL):
    import torch
    b = torch.full((max(entries, 1),), value, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return b


def _fenced(r, bufs):
    """the buffers on the host, read on a created stream behind frame_fence"""
    import torch
    st = torch.cuda.Stream()
    r.frame_fence(st.cuda_stream)
    with torch.cuda.stream(st):
        out = [b.to("cpu", non_blocking=False) for b in bufs]
    st.synchronize()
    return [o.numpy().view(np.uint32) for o in out]


def _assert_query(r, per_tri, per, base=0, window=None, device=True):
    """both units, host form and device form (with a tail of three entries, and one entry short), against the per-triangle
    counts of the probe pass, whose first id is `base`"""
    wi = Q.per_item_sums(per_tri, per)
    wt = np.concatenate([np.zeros(base, np.uint32), per_tri]).astype(np.uint32)
    gi = r.query_pixels("item", window=window)
    gt = r.query_pixels("triangle", window=window)
    assert gi.dtype == gt.dtype == np.uint32
    np.testing.assert_array_equal(gi, wi)
    np.testing.assert_array_equal(gt, wt)
    if device:
        n, T = wi.size, wt.size
        bi, bt, si, st = _buffer(n + 3), _buffer(T + 3), _buffer(max(n - 1, 1)), _buffer(max(T - 1, 1))
        r.query_pixels("item", window=window, out_ptr=bi.data_ptr(), entries=n + 3)
        r.query_pixels("triangle", window=window, out_ptr=bt.data_ptr(), entries=T + 3)
        if n > 1:
            r.query_pixels("item", window=window, out_ptr=si.data_ptr(), entries=n - 1)
        if T > 1:
            r.query_pixels("triangle", window=window, out_ptr=st.data_ptr(), entries=T - 1)
        di, dt, dsi, dst = _fenced(r, [bi, bt, si, st])
        np.testing.assert_array_equal(di[:n + 3], np.concatenate([wi, [0, 0, 0]]))
        np.testing.assert_array_equal(dt[:T + 3], np.concatenate([wt, [0, 0, 0]]))
        if n > 1:
            np.testing.assert_array_equal(dsi[:n - 1], wi[:-1])          # a unit >= out_entries is counted nowhere
        if T > 1:
            np.testing.assert_array_equal(dst[:T - 1], wt[:-1])
    return gi, gt


def _occluded_probe(fr, oracle, occ, probe, options=(), kinds=None):
    """a ctx with the occluder list drawn (depth only) and the probe list's geometry pass run on top"""
    _, r, dl_occ = _setup(fr, occ, options=options)
    _, _, dl_probe = _setup(fr, probe, kinds=kinds, r=r)
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    base = int(D.oracle_frame(oracle, occ, "DEPTH")[0].counters.tris_setup)
    r.geometry_list(dl_probe)
    return r, dl_occ, dl_probe, base


# ---- 1. the pairs of the reference, both units, both forms, both paths -------------------------------------------------

@pytest.mark.parametrize("bins", PATHS)
@pytest.mark.parametrize("occ,probe", list(Q.PAIRS))
def test_pairs(oracle, occ, probe, bins):
    import f_renderer_amd as fr
    d0, setup, per, pt, pi = Q.pair(oracle, occ, probe)
    r, _, _, base = _occluded_probe(fr, oracle, occ, probe, options=(("visible_lds_bins", bins),))
    gi, _ = _assert_query(r, pt, per, base)
    if Q.PAIRS[(occ, probe)] is not None:
        assert gi.tolist() == Q.PAIRS[(occ, probe)]
    assert_depth_equal(r.readback()[1], d0)                         # the depth it was asked against, untouched
    r.close()


# ---- 2. the raster paths -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("option", [("raster_sweep", 1), ("bin_atomics", 1)] + [("raster_nw", nw) for nw in (3, 4, 6, 8, 16)])
def test_raster_paths(oracle, option):
    import f_renderer_amd as fr
    for occ, probe in (("clipped", "sizes"), ("same_mesh", "clipped")):
        _, _, per, pt, _ = Q.pair(oracle, occ, probe)
        r, _, _, base = _occluded_probe(fr, oracle, occ, probe, options=(option,))
        _assert_query(r, pt, per, base, device=False)
        r.close()


# ---- 3. a sub-window with partial tiles; one triangle over all twelve tiles --------------------------------------------

def test_sub_window_with_partial_tiles(oracle):
    import f_renderer_amd as fr
    win = (5, 101, 3, 70)
    occ, probe = D.scene("clipped"), D.scene("sizes")
    of, _, _ = D.oracle_list_loop(oracle, occ, "DEPTH", window=win)
    scratch = oracle.Frame(W, H)
    scratch.clear(*D.CLEAR)
    _, setup, per = D.oracle_list_loop(oracle, probe, "DEPTH", frame=scratch, window=win)
    pt = Q.counts_c(oracle, of.depth, setup, window=win)
    pi = Q.per_item_sums(pt, per)
    assert 0 < int(pi.sum()) < int(Q.pair(oracle, None, "sizes")[4].sum()) and (pi == 0).any()
    _, r, dl_occ = _setup(fr, "clipped")
    _, _, dl_probe = _setup(fr, "sizes", r=r)
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH, width_range=win[:2], height_range=win[2:])
    r.geometry_list(dl_probe)
    _assert_query(r, pt, per, int(of.counters.tris_setup), window=win)
    r.close()


def test_one_triangle_over_all_twelve_tiles(oracle):
    import f_renderer_amd as fr
    big = np.zeros((1, 3, 4), np.float32)
    big[0, :, :] = [[-3.0, -1.0, 0.5, 1.0], [1.0, -1.0, 0.5, 1.0], [1.0, 3.0, 0.5, 1.0]]   # covers the frame
    d0 = D.oracle_frame(oracle, "clipped", "DEPTH")[0].depth
    f = oracle.Frame(W, H)
    f.clear(*D.CLEAR)
    setup = f.draw(big, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms(), keep_setup=True)
    pt = Q.counts_c(oracle, d0, setup)
    assert len(setup) >= 1 and W * H > int(pt.sum()) > W * H // 2
    _, r, dl_occ = _setup(fr, "clipped")
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    base = int(r.stats()["tris_setup"])
    r.geometry_processing(r.upload_mesh(big, fr.VS_CLIP))
    _assert_query(r, pt, [len(setup)], base)
    r.close()


@pytest.mark.parametrize("option", [None, ("raster_nw", 4), ("bin_atomics", 1)])
def test_records_outside_the_span_algebra_are_swept(oracle, option):
    """triangles with vertices tens of thousands of pixels away (the clipper keeps them): their records lie outside SPAN_SAFE
    and take the brute-force form inside the span kernel, next to records that take the spans"""
    import f_renderer_amd as fr
    from . import limit_scenes as L
    tris = L.jitter_w(L.pixel_soup(40, W, H, (64, 48), (80, 60), (3000.0, 20000.0), 5), 6)
    d0 = D.oracle_frame(oracle, "clipped", "DEPTH")[0].depth
    f = oracle.Frame(W, H)
    f.clear(*D.CLEAR)
    setup = f.draw(tris, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms(), keep_setup=True)
    far = np.abs(setup["spi"]).reshape(len(setup), -1).max(axis=1) > L.SPAN_SAFE
    pt = Q.counts_c(oracle, d0, setup)
    assert (far & (pt > 0)).sum() >= 3 and (~far & (pt > 0)).sum() >= 3
    assert (pt < Q.counts_c(oracle, np.full(W * H, D.CLEAR[1], np.float32), setup)).sum() >= 5      # partly occluded ones
    _, r, dl_occ = _setup(fr, "clipped", options=(option,) if option else ())
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    base = int(r.stats()["tris_setup"])
    r.geometry_processing(r.upload_mesh(tris, fr.VS_CLIP))
    _assert_query(r, pt, [len(setup)], base, device=False)
    r.close()


# ---- 4. more items than the LDS histogram takes ------------------------------------------------------------------------

def test_more_items_than_the_lds_histogram_takes(oracle):
    import f_renderer_amd as fr
    n = fr.VISIBLE_LDS_BINS + 100
    sc = D.Scene([D.Mesh(S.patch(1))], [0] * n, S.grid_models(n), "PHONG", "DEPTH")
    d0 = D.oracle_frame(oracle, "clipped", "DEPTH")[0].depth
    _, setup, per = D.oracle_list_loop(oracle, sc, "DEPTH")
    pt = Q.counts_c(oracle, d0, setup)
    pi = Q.per_item_sums(pt, per)
    assert (pi > 0).sum() > 50 and (pi[fr.VISIBLE_LDS_BINS:] > 0).any() and ((pi == 0) & (np.array(per) > 0)).sum() > 100
    _, r, dl_occ = _setup(fr, "clipped")
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    base = int(r.stats()["tris_setup"])
    r.geometry_processing_instanced(r.upload_mesh(S.patch(1), fr.VS_PHONG), r.upload_instances(S.grid_models(n)))
    gi, gt = _assert_query(r, pt, per, base)
    assert gi.size == n
    # the same through the LDS path: entries up to the cap
    np.testing.assert_array_equal(r.query_pixels("item", entries=fr.VISIBLE_LDS_BINS), gi[:fr.VISIBLE_LDS_BINS])
    r.close()


# ---- 5. NaN, -0.0 and +inf ---------------------------------------------------------------------------------------------

def test_against_a_nan_clear_every_covered_fragment_passes(oracle):
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "clipped")
    r.clear(D.CLEAR[0], float("nan"))
    r.geometry_list(dl)
    q = r.query_pixels("item")
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_DEPTH)
    alone = D.oracle_frame(oracle, "clipped", "DEPTH")[0]
    assert r.stats()["frag_covered"] == alone.counters.frag_covered == int(q.sum()) > 0
    r.close()


@pytest.mark.parametrize("depth", [-0.0, float("inf"), 0.5])
def test_clear_depths(oracle, depth):
    import f_renderer_amd as fr
    _, setup, per = D.oracle_frame(oracle, "clipped", "DEPTH")
    pt = Q.counts_c(oracle, np.full(W * H, depth, np.float32), setup)
    assert (depth != float("inf")) == (int(pt.sum()) > 0)
    sc, r, dl = _setup(fr, "clipped")
    r.clear(D.CLEAR[0], depth)
    r.geometry_list(dl)
    _assert_query(r, pt, per, device=False)
    r.close()


def test_nan_rhw_fragments_pass_and_a_depth_that_holds_nan(oracle):
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    from .test_gpu_edge import NAN_TRIS
    Wn, Hn = 160, 120
    tris = NAN_TRIS[[3, 4, 0, 1, 2]]                                # the NaN fan last: it owns its pixels, their depth is NaN
    f = oracle.Frame(Wn, Hn)
    f.clear()
    setup = f.draw(tris, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms(), keep_setup=True)
    assert f.counters.frag_nan > 0 and np.isnan(f.depth).any()
    more = scenes.random_clip_triangles(300, Wn, Hn, seed=17)
    g = oracle.Frame(Wn, Hn)
    g.clear()
    setup_more = g.draw(more, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms(), keep_setup=True)

    def counts(depth, setup):
        fr_ = oracle.Frame(Wn, Hn)
        out = np.zeros(len(setup), np.uint32)
        for t in range(len(setup)):
            fr_.depth[:] = depth
            fr_.tri_id[:] = Q.NONE
            fr_.rasterization((0, Wn), (0, Hn), setup[t], oracle.PS_DEPTH, 0, oracle.make_uniforms(), tri_id=Q.MARK)
            out[t] = int((fr_.tri_id == Q.MARK).sum())
        return out
    r = fr.Renderer(Wn, Hn)
    mesh, mesh_more = r.upload_mesh(tris, fr.VS_CLIP), r.upload_mesh(more, fr.VS_CLIP)
    # the NaN-rhw fragments of the probe pass itself, against a clear depth nothing else would beat
    r.clear((30, 30, 30, 255), 1.0e30)
    r.geometry_processing(mesh)
    want = counts(np.full(Wn * Hn, 1.0e30, np.float32), setup)
    assert int(want.sum()) > 0
    np.testing.assert_array_equal(r.query_pixels("triangle"), want)
    # a depth that holds NaN after the scene was drawn: everything passes there
    r.clear()
    r.draw(mesh, fr.PS_DEPTH)
    r.geometry_processing(mesh_more)
    want = counts(f.depth, setup_more)
    assert int(want.sum()) > int(counts(np.where(np.isnan(f.depth), np.float32(1.0e30), f.depth), setup_more).sum())
    np.testing.assert_array_equal(r.query_pixels("triangle"), np.concatenate([np.zeros(len(setup), np.uint32), want]))
    np.testing.assert_array_equal(r.query_pixels("item"), [int(want.sum())])
    r.close()


# ---- 6. what it leaves alone, and what it composes with ----------------------------------------------------------------

@pytest.mark.parametrize("option", [None, ("bin_atomics", 1)])
def test_targets_and_statistics_untouched(oracle, option):
    import f_renderer_amd as fr
    frames = []
    for query in (False, True):
        _, r, dl_occ = _setup(fr, "clipped", options=(option,) if option else ())
        _, _, dl_probe = _setup(fr, "sizes", r=r)
        r.clear(*D.CLEAR)
        r.draw_list(dl_occ, fr.PS_PHONG)
        r.geometry_list(dl_probe)
        if query:
            b = _buffer(16)
            r.query_pixels("item", out_ptr=b.data_ptr(), entries=16)
            r.query_pixels("triangle")
        frames.append(_read(r, setup=False))
        r.close()
    a, b = frames
    for k in "tc":
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["d"].view(np.uint32), b["d"].view(np.uint32))
    for k in STAT_KEYS:
        assert a["st"][k] == b["st"][k], k


def test_geometry_query_raster_equals_draw(oracle):
    import f_renderer_amd as fr
    _, _, per, pt, _ = Q.pair(oracle, "clipped", "sizes")
    frames = []
    for query in (False, True):
        _, r, dl_occ = _setup(fr, "clipped")
        _, _, dl_probe = _setup(fr, "sizes", r=r)
        r.clear(*D.CLEAR)
        r.draw_list(dl_occ, fr.PS_PHONG)
        if query:
            r.geometry_list(dl_probe)
            np.testing.assert_array_equal(r.query_pixels("item"), Q.per_item_sums(pt, per))
            r.rasterization((0, W), (0, H), fr.PS_PHONG)
        else:
            r.draw_list(dl_probe, fr.PS_PHONG)
        frames.append(_read(r))
        r.close()
    a, b = frames
    for k in "tc":
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["d"].view(np.uint32), b["d"].view(np.uint32))
    np.testing.assert_array_equal(a["setup"], b["setup"])
    for k in STAT_KEYS:
        assert a["st"][k] == b["st"][k], k


def test_a_query_between_two_draws_sees_the_first_and_not_the_second(oracle):
    import f_renderer_amd as fr
    _, _, per, pt, pi = Q.pair(oracle, "clipped", "sizes")
    _, r, dl_occ = _setup(fr, "clipped")
    _, _, dl_probe = _setup(fr, "sizes", r=r)
    _, _, dl_late = _setup(fr, "same_mesh", r=r)
    n = len(per)
    b = _buffer(n)
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    r.geometry_list(dl_probe)
    r.query_pixels("item", out_ptr=b.data_ptr(), entries=n)
    r.draw_list(dl_late, fr.PS_DEPTH)                               # occludes more of the probe, behind the query
    np.testing.assert_array_equal(_fenced(r, [b])[0][:n], pi)
    r.close()


@pytest.mark.parametrize("fif", [1, 2])
def test_frames_in_flight_count_against_their_own_depth(oracle, fif):
    import f_renderer_amd as fr
    occs = ["clipped", "same_mesh", "sizes", "clipped"]
    _, r, _ = _setup(fr, "clipped", options=(("frames_in_flight", fif),))
    lists = {name: _setup(fr, name, r=r)[2] for name in set(occs)}
    n = D.scene("sizes").nitems
    bufs = [_buffer(n) for _ in occs]
    for occ, b in zip(occs, bufs):                                  # no host wait between the frames
        r.clear(*D.CLEAR)
        r.draw_list(lists[occ], fr.PS_DEPTH)
        r.geometry_list(lists["sizes"])
        r.query_pixels("item", out_ptr=b.data_ptr(), entries=n)
    got = _fenced(r, bufs)
    for occ, g in zip(occs, got):
        np.testing.assert_array_equal(g[:n], Q.pair(oracle, occ, "sizes")[4])
    r.close()


def test_caller_bound_targets(oracle):
    import torch
    import f_renderer_amd as fr
    st = torch.cuda.Stream()
    _, r, dl_occ = _setup(fr, "clipped", options=(("bound_targets_in_flight", 1),), stream=st.cuda_stream)
    _, _, dl_other = _setup(fr, "same_mesh", r=r)
    _, _, dl_probe = _setup(fr, "sizes", r=r)
    sets = [tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32)) for _ in range(2)]
    torch.cuda.synchronize()
    n = D.scene("sizes").nitems
    bufs = [_buffer(n), _buffer(n)]
    for k, dl in enumerate((dl_occ, dl_other)):
        r.frame_wait(st.cuda_stream)
        r.bind_targets(*(x.data_ptr() for x in sets[k]))
        r.clear(*D.CLEAR)
        r.draw_list(dl, fr.PS_DEPTH)
        r.geometry_list(dl_probe)
        r.query_pixels("item", out_ptr=bufs[k].data_ptr(), entries=n)
    got = _fenced(r, bufs)
    np.testing.assert_array_equal(got[0][:n], Q.pair(oracle, "clipped", "sizes")[4])
    np.testing.assert_array_equal(got[1][:n], Q.pair(oracle, "same_mesh", "sizes")[4])
    r.close()


# ---- 7. replay ---------------------------------------------------------------------------------------------------------

def test_tiny_work_lists_are_grown_by_replays(oracle):
    import f_renderer_amd as fr
    _, _, per, pt, _ = Q.pair(oracle, "same_mesh", "clipped")
    r, _, _, base = _occluded_probe(fr, oracle, "same_mesh", "clipped", options=TINY)
    _assert_query(r, pt, per, base)
    assert r.stats()["replays"] > 0
    r.close()


def test_a_query_behind_a_failed_geometry_pass_is_replayed_with_it(oracle):
    """The probe pass's fan space is far too small, and nothing before the query looks at it: the query's first launch is
    cancelled on the device (it writes nothing, not even the zeros), its own verification finds the failure, and the replay
    runs the pass and the query again.  The device form's counts are exact afterwards."""
    import f_renderer_amd as fr
    _, _, per, pt, pi = Q.pair(oracle, "same_mesh", "clipped")
    r, _, _, base = _occluded_probe(fr, oracle, "same_mesh", "clipped", options=(("fan_capacity", 16),))
    n = len(per)
    b = _buffer(n)
    r.query_pixels("item", out_ptr=b.data_ptr(), entries=n)
    r.sync()
    assert r.stats()["replays"] > 0
    np.testing.assert_array_equal(_fenced(r, [b])[0][:n], pi)
    r.close()


def test_a_query_behind_a_failed_open_pass_leaves_the_sentinel_until_sync(oracle):
    """A query whose raster signature is proven is not verified inside the call, so behind a failed pass that nobody has looked
    at it stays cancelled until the next synchronisation point.  Four warm-up frames of one command shape -- draw the
    occluders, a geometry pass that is left open, the probe's geometry pass, the query -- need no fan space at all and prove
    the signatures on both workspace sets.  The fifth frame has the same shape, but its open pass is the `clipped` list, whose
    fans do not fit the tiny fan space: that pass fails on the device, and the probe's pass, k_visible_prep and k_query behind
    it are cancelled.  Read behind a stream fence alone the buffer still holds the sentinel -- not the zeros, not a count;
    frr_sync grows the fan space and replays the three commands, and then the counts are exact."""
    import f_renderer_amd as fr
    _, _, per, pt, pi = Q.pair(oracle, "sizes", "sizes")
    for name in ("sizes", "same_mesh"):                             # the warm-up passes emit their inputs as they are: no fans
        sc = D.scene(name)
        assert D.oracle_frame(oracle, name, "DEPTH")[2] == sc.ntris
    assert sum(D.oracle_frame(oracle, "clipped", "DEPTH")[2]) > sum(D.scene("clipped").ntris) + 16   # the open pass needs more fans than there are
    _, r, dl_occ = _setup(fr, "sizes", options=(("fan_capacity", 16),))
    _, _, dl_fits = _setup(fr, "same_mesh", r=r)
    _, _, dl_fails = _setup(fr, "clipped", r=r)
    n = len(per)

    def frame(dl_open, b):
        r.clear(*D.CLEAR)
        r.draw_list(dl_occ, fr.PS_DEPTH)
        r.geometry_list(dl_open)                                    # left open: nothing rasterizes it
        r.geometry_list(dl_occ)                                     # the probe: the occluders' own list
        r.query_pixels("item", out_ptr=b.data_ptr(), entries=n)
    for _ in range(4):
        b = _buffer(n)
        frame(dl_fits, b)
        np.testing.assert_array_equal(_fenced(r, [b])[0][:n], pi)
    r.sync()
    assert r.stats()["replays"] == 0
    b = _buffer(n)
    frame(dl_fails, b)
    np.testing.assert_array_equal(_fenced(r, [b])[0][:n], np.full(n, SENTINEL, np.uint32))   # nothing written, not even the zeros
    r.sync()
    assert r.stats()["replays"] > 0
    np.testing.assert_array_equal(_fenced(r, [b])[0][:n], pi)
    r.close()


# ---- 8. partition ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_ranks_add_up(oracle, world, blocked):
    import f_renderer_amd as fr
    d0, setup, per, pt, pi = Q.pair(oracle, "clipped", "sizes")
    total_i, total_t = np.zeros(len(per), np.uint64), np.zeros(len(pt), np.uint64)
    base = int(D.oracle_frame(oracle, "clipped", "DEPTH")[0].counters.tris_setup)
    for rank in range(world):
        _, r, dl_occ = _setup(fr, "clipped")
        _, _, dl_probe = _setup(fr, "sizes", r=r)
        r.set_partition(rank, world, blocked)
        r.clear(*D.CLEAR)
        r.geometry_list(dl_occ)
        r.rasterization((0, W), (0, H), fr.PS_DEPTH)
        r.geometry_list(dl_probe)
        own = owned_pixel_rows(H, rank, world, blocked)
        want = Q.counts_c(oracle, d0, setup, row_mask=own)
        gi, gt = r.query_pixels("item"), r.query_pixels("triangle")
        np.testing.assert_array_equal(gt[base:], want)
        np.testing.assert_array_equal(gi, Q.per_item_sums(want, per))
        total_i += gi
        total_t += gt[base:]
        # after a draw that filtered the setup list: refused, where frr_visible_pixels is
        r.draw_list(dl_probe, fr.PS_DEPTH)
        one = np.zeros(1, np.uint32)
        assert r._lib.frr_query_pixels_host(r._ctx, fr.PER_ITEM, 0, W, 0, H, one.ctypes.data, 1, None) == fr.FRR_ERR_INVALID
        assert r._lib.frr_visible_pixels_host(r._ctx, fr.PER_ITEM, 0, W, 0, H, one.ctypes.data, 1, None) == fr.FRR_ERR_INVALID
        r.close()
    np.testing.assert_array_equal(total_i, pi)
    np.testing.assert_array_equal(total_t, pt)


# ---- 9. passes of every kind -------------------------------------------------------------------------------------------

def test_instanced_and_plain_passes(oracle):
    import f_renderer_amd as fr
    sc = D.scene("same_mesh")
    _, _, per, pt, pi = Q.pair(oracle, "clipped", "same_mesh")
    _, r, dl_occ = _setup(fr, "clipped")
    mesh = r.upload_mesh(sc.meshes[0].tris, fr.VS_PHONG)
    inst = r.upload_instances(sc.models)
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    base = int(r.stats()["tris_setup"])
    r.geometry_processing_instanced(mesh, inst)                     # the units are the instances
    _assert_query(r, pt, per, base)
    r.set_uniforms(model=sc.models[3])                              # a plain pass: one unit
    r.geometry_processing(mesh)
    b = np.concatenate([[0], np.cumsum(per)])
    _assert_query(r, pt[b[3]:b[4]], [per[3]], base + sum(per))
    r.close()


def test_indexed_and_device_bound_meshes_and_a_user_vertex_shader(oracle):
    import f_renderer_amd as fr
    _, _, per, pt, _ = Q.pair(oracle, "sizes", "mix")
    r, _, _, base = _occluded_probe(fr, oracle, "sizes", "mix", kinds=["plain", "indexed", "dev", "dev_indexed"])
    _assert_query(r, pt, per, base, device=False)
    r.close()
    _, _, per, pt, _ = Q.pair(oracle, "clipped", "sizes")
    _, r, dl_occ = _setup(fr, "clipped")
    _, _, dl_probe = _setup(fr, "sizes", vs_id=_phong_sid(), r=r)
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    base = int(r.stats()["tris_setup"])
    r.geometry_list(dl_probe)
    _assert_query(r, pt, per, base, device=False)
    r.close()


@pytest.mark.parametrize("mode", ["NEG", "POS"])
def test_a_culled_pass(oracle, mode):
    import f_renderer_amd as fr
    sc = D.scene("mirrored")
    d0 = D.oracle_frame(oracle, "clipped", "DEPTH")[0].depth
    keep = D.cull_keep(sc, getattr(fr, "CULL_" + mode))
    assert all(0 < k.sum() < k.size for k in keep)
    _, setup, per = D.oracle_list_loop(oracle, sc, "DEPTH", keep=keep)
    pt = Q.counts_c(oracle, d0, setup)
    assert int(pt.sum()) > 0
    _, r, dl_occ = _setup(fr, "clipped")
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    base = int(r.stats()["tris_setup"])
    r.set_uniforms(**S.camera_kw(fr))
    _, _, dl_probe = _setup(fr, "mirrored", r=r)
    r.set_cull(getattr(fr, "CULL_" + mode))
    r.geometry_list(dl_probe)
    _assert_query(r, pt, per, base, device=False)
    r.close()


def test_a_predicated_pass_counts_zero_for_dropped_items(oracle):
    import torch
    import f_renderer_amd as fr
    kept = P.masks(D.scene("sizes").nitems)["alternating"]
    d0 = D.oracle_frame(oracle, "clipped", "DEPTH")[0].depth
    _, setup, per = P.expected(oracle, "sizes", kept, "DEPTH")
    pt = Q.counts_c(oracle, d0, setup)
    pi = Q.per_item_sums(pt, per)
    assert (pi[~np.asarray(kept)] == 0).all() and (pi[np.asarray(kept)] > 0).any()
    _, r, dl_occ = _setup(fr, "clipped")
    _, _, dl_probe = _setup(fr, "sizes", r=r)
    keep = torch.from_numpy(np.asarray(kept).astype(np.int32)).to("cuda")
    torch.cuda.synchronize()
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    base = int(r.stats()["tris_setup"])
    r.geometry_list_if(dl_probe, keep.data_ptr(), keep.numel())
    _assert_query(r, pt, per, base, device=False)
    r.close()


# ---- 10. end to end: the counts decide the draw, with no host wait -----------------------------------------------------

@pytest.mark.parametrize("proxy", ["own", "box"])
def test_the_counts_decide_the_draw_with_no_host_wait(oracle, proxy):
    import f_renderer_amd as fr
    occ, sc, box = (D.scene("clipped"), D.scene("sizes"), None) if proxy == "own" else Q.box_scenes()
    n = sc.nitems
    # expected: the occluders, then all of the probe list
    want = oracle.Frame(W, H)
    want.clear(*D.CLEAR)
    D.oracle_list_loop(oracle, occ, "PHONG", frame=want)
    D.oracle_list_loop(oracle, sc, "PHONG", frame=want)
    r = _renderer(fr, sc)
    dl_occ = _upload(r, occ, _meshes(r, occ, fr.VS_PHONG))
    dl_probe = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    dl_query = dl_probe if proxy == "own" else _upload(r, box, _meshes(r, box, fr.VS_PHONG))
    b = _buffer(n, 0)                                               # (zeros: a read that ran ahead of the query would drop everything)
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_PHONG)
    r.geometry_list(dl_query)
    r.query_pixels("item", out_ptr=b.data_ptr(), entries=n)
    r.draw_list_if(dl_probe, b.data_ptr(), n, fr.PS_PHONG, min_value=1)
    g = _read(r, setup=False)
    q = _fenced(r, [b])[0][:n]
    assert (q == 0).any() and (q > 0).any()                         # something was skipped, something drawn
    if proxy == "own":
        np.testing.assert_array_equal(q, Q.pair(oracle, "clipped", "sizes")[4])
    assert_depth_equal(g["d"], want.depth)
    np.testing.assert_array_equal(g["c"], want.color)
    _, count = r.item_ranges()
    assert (count[q == 0] == 0).all() and (count[q > 0] > 0).all()   # the skipped items emitted nothing
    r.close()


# ---- 11. errors --------------------------------------------------------------------------------------------------------

def test_errors_leave_the_ctx_drawing(oracle):
    import f_renderer_amd as fr
    _, _, per, pt, pi = Q.pair(oracle, "clipped", "sizes")
    sc, r, dl_occ = _setup(fr, "clipped")
    _, _, dl_probe = _setup(fr, "sizes", r=r)
    L, ctx = r._lib, r._ctx
    n = len(per)
    b = _buffer(n + 1)
    p = b.data_ptr()
    host = np.zeros(n, np.uint32)
    # before any geometry pass
    assert L.frr_query_pixels(ctx, fr.PER_ITEM, 0, W, 0, H, p, n) == fr.FRR_ERR_INVALID and "geometry" in _err(r)
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    r.geometry_list(dl_probe)

    def still_counts():
        np.testing.assert_array_equal(r.query_pixels("item"), pi)
    for fn, buf in ((L.frr_query_pixels, p), (L.frr_query_pixels_host, host.ctypes.data)):
        tail = () if fn is L.frr_query_pixels else (None,)
        for win, code in (((-1, W - 1, 0, H), fr.FRR_ERR_UNSUPPORTED), ((10, 5, 0, H), fr.FRR_ERR_INVALID), ((0, W, 7, 7), fr.FRR_ERR_INVALID),
                          ((0, W + 1, 0, H), fr.FRR_ERR_INVALID), ((0, W, 0, H + 1), fr.FRR_ERR_INVALID)):
            assert fn(ctx, fr.PER_ITEM, *win, buf, n, *tail) == code, win
            assert L.frr_visible_pixels(ctx, fr.PER_ITEM, *win, p, n) == code
        assert fn(ctx, fr.PER_ITEM, 0, W, 0, H, None, n, *tail) == fr.FRR_ERR_INVALID and "NULL" in _err(r)
        assert fn(ctx, fr.PER_ITEM, 0, W, 0, H, buf + 2, n, *tail) == fr.FRR_ERR_INVALID and "aligned" in _err(r)
        assert fn(ctx, 7, 0, W, 0, H, buf, n, *tail) == fr.FRR_ERR_INVALID and "unit" in _err(r)
        assert fn(ctx, fr.PER_ITEM, 0, W, 0, H, None, 0, *tail) == fr.FRR_OK          # no entries: nothing happens
        still_counts()
    # a frr_clear since the pass, an empty pass, a pass without items: FRR_OK and zeros
    r.clear(*D.CLEAR)
    np.testing.assert_array_equal(r.query_pixels("item"), np.zeros(n, np.uint32))
    assert r.query_pixels("triangle").size == 0
    r.query_pixels("item", out_ptr=p, entries=n + 1)
    np.testing.assert_array_equal(_fenced(r, [b])[0][:n + 1], np.zeros(n + 1, np.uint32))
    r.geometry_processing(r.upload_mesh(np.zeros((0, 3, 8), np.float32), fr.VS_PHONG))
    np.testing.assert_array_equal(r.query_pixels("item"), [0])
    r.geometry_list(r.upload_draw_list([], np.zeros((0, 16), np.float32)))
    assert r.query_pixels("item").size == 0
    b2 = _buffer(3)
    r.query_pixels("item", out_ptr=b2.data_ptr(), entries=3)
    np.testing.assert_array_equal(_fenced(r, [b2])[0][:3], [0, 0, 0])
    r.clear(*D.CLEAR)
    r.draw_list(dl_occ, fr.PS_DEPTH)
    r.geometry_list(dl_probe)
    still_counts()
    r.close()
