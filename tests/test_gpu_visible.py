"""Visible pixel counts on the device (frr_visible_pixels / frr_visible_pixels_host): the triangle-id target of a window as
counts per item of the latest geometry pass, or per triangle of the frame.  Every expected value is an exact integer: the
NumPy histogram (tests/visible_scenes.py) of the oracle's frame and of the library's own readback() ids.  Frames are those of
tests/drawlist_scenes.py, 128 x 96; option visible_lds_bins = 1 sends the same frames down the global-memory path."""
import functools

import numpy as np
import pytest

from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import user_shaders
from .conftest import owned_pixel_rows
from .visible_scenes import NONE, bounds_of, want_counts

pytestmark = pytest.mark.gpu
W, H = D.W, D.H
FULL = ((0, W), (0, H))
SENTINEL = 0x5A5A5A5A
PATHS = [0, 1]            # visible_lds_bins: the default (LDS histogram), and 1 (every pass with more than one unit adds to global memory)


def _renderer(fr, sc, options=(), stream=None):
    r = fr.Renderer(W, H, stream=stream)
    for k, v in options:
        r.set_option(k, v)
    r.set_texture(0, S.texture())
    if sc is None or sc.lit:
        r.set_uniforms(texture_slot=0, **S.camera_kw(fr))
    return r


def _list(r, fr, sc, vs_id=None, kinds=None):
    import torch
    vs_id = getattr(fr, "VS_" + sc.vs) if vs_id is None else vs_id
    meshes = []
    for k, m in enumerate(sc.meshes):
        kind = kinds[k] if kinds else "plain"
        if kind == "plain":
            meshes.append(r.upload_mesh(m.tris, vs_id))
        elif kind == "indexed":
            meshes.append(r.upload_mesh_indexed(m.indexed[0], m.indexed[1], vs_id))
        else:
            dt = torch.from_numpy(m.tris).to("cuda")
            torch.cuda.synchronize()
            meshes.append(r.bind_mesh_device(dt.data_ptr(), m.ntris, vs_id, keepalive=dt))
    return r.upload_draw_list([meshes[w] for w in sc.which], sc.models), meshes


def _buffers(entries, n=1):
    """n device buffers of `entries` u32 holding a sentinel, ready before anything the library enqueues"""
    import torch
    bufs = [torch.full((max(entries, 1),), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    return bufs if n > 1 else bufs[0]


def _host(buf, entries=None):
    import torch
    torch.cuda.synchronize()
    a = buf.cpu().numpy().view(np.uint32)
    return a if entries is None else a[:entries]


def _fenced(r, bufs):
    """the buffers on the host, read on a created stream behind frame_fence (not torch's default stream: its handle is 0)"""
    import torch
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    r.frame_fence(st.cuda_stream)
    with torch.cuda.stream(st):
        out = [b.to("cpu", non_blocking=False) for b in bufs]
    st.synchronize()
    return [o.numpy().view(np.uint32) for o in out]


def _lib_bounds(r):
    first, count = r.item_ranges()
    return np.append(first, first[-1] + count[-1]).astype(np.uint32) if first.size else None, first, count


def _assert_counts(r, ids, win=FULL, bounds="lib", T=None, device=True):
    """both units, host form and device form (with a tail of three entries), against the NumPy histogram of `ids` over `win`;
    bounds: the item boundaries, or "lib": from item_ranges().  Returns (per item, per triangle)."""
    wr, hr = win
    lb, first, count = _lib_bounds(r)
    if isinstance(bounds, str):
        bounds = lb
    n = first.size
    if T is None:
        T = int(r.stats()["tris_setup"])
    wi = want_counts(ids, wr, hr, bounds=bounds) if n else np.zeros(0, np.uint32)
    wt = want_counts(ids, wr, hr, units=T)
    gi = r.visible_pixels("item", width_range=wr, height_range=hr)
    gt = r.visible_pixels("triangle", width_range=wr, height_range=hr)
    assert gi.dtype == gt.dtype == np.uint32
    np.testing.assert_array_equal(gi, wi)
    np.testing.assert_array_equal(gt, wt)
    if device:
        bi, bt = _buffers(n + 3), _buffers(T + 3)
        r.visible_pixels("item", out_ptr=bi.data_ptr(), entries=n + 3, width_range=wr, height_range=hr)
        r.visible_pixels("triangle", out_ptr=bt.data_ptr(), entries=T + 3, width_range=wr, height_range=hr)
        di, dt = _fenced(r, [bi, bt])
        np.testing.assert_array_equal(di[:n + 3], np.concatenate([wi, [0, 0, 0]]))
        np.testing.assert_array_equal(dt[:T + 3], np.concatenate([wt, [0, 0, 0]]))
    return gi, gt


@functools.lru_cache(maxsize=None)
def _phong_sid():
    import f_renderer_amd as fr
    r = fr.Renderer(32, 32)
    sid = r.register_shader(user_shaders.PHONG, 8, 8)
    r.close()
    return sid


# ---- 1. every draw-list scene, both units, both forms, both paths -------------------------------------------------------

@pytest.mark.parametrize("bins", PATHS)
@pytest.mark.parametrize("name", D.NAMES)
def test_draw_list_scenes(oracle, name, bins):
    import f_renderer_amd as fr
    sc = D.scene(name)
    of, _, per = D.oracle_frame(oracle, name)
    r = _renderer(fr, sc, options=(("visible_lds_bins", bins),))
    dl, _ = _list(r, fr, sc)
    r.clear(*D.CLEAR)
    r.draw_list(dl, getattr(fr, "PS_" + sc.ps))
    t = r.readback()[2]
    np.testing.assert_array_equal(t, of.tri_id)
    gi, gt = _assert_counts(r, of.tri_id, bounds=bounds_of(per), T=sum(per))       # the oracle's frame and its item sizes
    gi2, gt2 = _assert_counts(r, t, device=False)                                  # the library's own ids and item_ranges()
    assert gi.tolist() == gi2.tolist() and gt.tolist() == gt2.tolist()
    assert gi.size == sc.nitems and gt.size == sum(per) and int(gi.sum()) == int((t != NONE).sum())
    if name == "many":
        assert int(((gi == 0) & (np.array(per) > 0)).sum()) == 49 and int(gi.max()) == 12 and int((gt > 0).sum()) == 390
    # entries below the number of units: the dropped units are counted nowhere
    if sc.nitems > 1:
        np.testing.assert_array_equal(r.visible_pixels("item", entries=sc.nitems - 1), gi[:-1])
        np.testing.assert_array_equal(r.visible_pixels("triangle", entries=1), np.concatenate([gt, [0]])[:1])   # (no triangle at all: the tail)
    r.close()


# ---- 2. every kind of pass ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", PATHS)
def test_instanced_pass_and_plain_draw(oracle, bins):
    import f_renderer_amd as fr
    sc = D.scene("same_mesh")
    of, _, per = D.oracle_frame(oracle, "same_mesh")
    r = _renderer(fr, sc, options=(("visible_lds_bins", bins),))
    mesh = r.upload_mesh(sc.meshes[0].tris, fr.VS_PHONG)
    r.clear(*D.CLEAR)
    r.draw_instanced(mesh, r.upload_instances(sc.models), fr.PS_PHONG)             # the instances are the items
    gi, _ = _assert_counts(r, of.tri_id, bounds=bounds_of(per), T=sum(per))
    assert gi.size == 7 and (gi > 0).all()
    r.clear(*D.CLEAR)
    r.set_uniforms(model=sc.models[2])
    r.draw(mesh, fr.PS_PHONG)                                                      # a plain pass: one item
    t = r.readback()[2]
    gi, gt = _assert_counts(r, t)
    assert gi.tolist() == [int((t != NONE).sum())] and gi[0] > 0 and gt.sum() == gi[0]
    r.close()


@pytest.mark.parametrize("case", ["mix", "user", "culled"])
def test_indexed_device_bound_user_shader_and_culled_passes(oracle, case):
    import f_renderer_amd as fr
    name = {"mix": "mix", "user": "clipped", "culled": "mirrored"}[case]
    sc = D.scene(name)
    r = _renderer(fr, sc)
    sid = _phong_sid() if case == "user" else None
    dl, _ = _list(r, fr, sc, vs_id=sid, kinds=["plain", "indexed", "dev", "indexed"] if case == "mix" else None)
    if case == "culled":
        r.set_cull(fr.CULL_NEG)
    r.clear(*D.CLEAR)
    r.draw_list(dl, sid if case == "user" else getattr(fr, "PS_" + sc.ps))
    t = r.readback()[2]
    gi, gt = _assert_counts(r, t)
    of, _, per = D.oracle_frame(oracle, name)
    if case == "culled":                                                           # counts are over the surviving ids
        first, count = r.item_ranges()
        assert count.sum() < sum(per) and gt.size == count.sum() and gi.sum() == (t != NONE).sum() > 0
    else:
        np.testing.assert_array_equal(t, of.tri_id)
        np.testing.assert_array_equal(gi, want_counts(of.tri_id, *FULL, bounds=bounds_of(per)))
    r.close()


# ---- 3. more units than the LDS path takes, no hook -----------------------------------------------------------------------

def test_more_items_than_the_lds_histogram_takes():
    import f_renderer_amd as fr
    n = fr.VISIBLE_LDS_BINS + 100
    r = _renderer(fr, None)
    mesh = r.upload_mesh(S.patch(1), fr.VS_PHONG)
    r.clear(*D.CLEAR)
    r.draw_instanced(mesh, r.upload_instances(S.grid_models(n)), fr.PS_DEPTH)
    t = r.readback()[2]
    gi, gt = _assert_counts(r, t)                    # (the ids of such passes are held to the oracle by tests/test_gpu_instanced.py)
    assert gi.size == n and gt.size >= n and (gi > 0).sum() > 100 and gi.sum() == (t != NONE).sum()
    # the same frame through the LDS path: entries up to the cap
    np.testing.assert_array_equal(r.visible_pixels("item", entries=fr.VISIBLE_LDS_BINS), gi[:fr.VISIBLE_LDS_BINS])
    np.testing.assert_array_equal(r.visible_pixels("triangle", entries=fr.VISIBLE_LDS_BINS), gt[:fr.VISIBLE_LDS_BINS])
    r.close()


# ---- 4. two passes in one frame ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", PATHS)
def test_two_passes_in_one_frame(bins):
    import f_renderer_amd as fr
    a, b = D.scene("sizes"), D.scene("clipped")
    r = _renderer(fr, a, options=(("visible_lds_bins", bins),))
    la, _ = _list(r, fr, a)
    lb, _ = _list(r, fr, b)
    r.clear(*D.CLEAR)
    r.draw_list(la, fr.PS_PHONG)
    ba, _, _ = _lib_bounds(r)
    r.draw_list(lb, fr.PS_PHONG)
    bb, _, _ = _lib_bounds(r)
    t = r.readback()[2]
    assert ba[0] == 0 and bb[0] == ba[-1] > 0
    gi, gt = _assert_counts(r, t, bounds=bb, T=int(bb[-1]))                         # per item: the latest pass only
    assert gi.size == b.nitems and gt.size == bb[-1] and gt.sum() == (t != NONE).sum() > gi.sum() > 0
    for bnd in (ba, bb):                                                           # per triangle: the whole frame, summed over each pass's ranges
        sums = [int(gt[bnd[k]:bnd[k + 1]].sum()) for k in range(bnd.size - 1)]
        assert sums == want_counts(t, *FULL, bounds=bnd).tolist()
    assert sum(int(gt[ba[k]:ba[k + 1]].sum()) for k in range(ba.size - 1)) > 0     # the first pass still owns pixels
    r.close()


# ---- 5. stream order -----------------------------------------------------------------------------------------------------

def test_a_count_is_ordered_between_the_draws_around_it():
    import f_renderer_amd as fr
    sc = D.scene("sizes")
    r = _renderer(fr, sc)
    dl, meshes = _list(r, fr, sc)
    r.set_uniforms(model=sc.models[0])
    # the frame once with read-backs: the ids before and after a second draw of item 0's mesh under item 0's matrix, which
    # ties with item 0 everywhere and, being later, takes every pixel item 0 owned
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_DEPTH)
    first, count = r.item_ranges()
    t1 = r.readback()[2]
    r.draw(meshes[0], fr.PS_DEPTH)
    t2 = r.readback()[2]
    T1, T2 = int(first[-1] + count[-1]), int(r.stats()["tris_setup"])
    # ... and again with no host wait between the commands
    A, B = _buffers(T2, 2)
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_DEPTH)
    r.visible_pixels("triangle", out_ptr=A.data_ptr(), entries=T2)
    r.draw(meshes[0], fr.PS_DEPTH)
    r.visible_pixels("triangle", out_ptr=B.data_ptr(), entries=T2)
    r.sync()
    a, b = _host(A, T2), _host(B, T2)
    np.testing.assert_array_equal(a, want_counts(t1, *FULL, units=T1, entries=T2))
    np.testing.assert_array_equal(b, want_counts(t2, *FULL, units=T2))
    assert a[:count[0]].sum() == 121 and b[:count[0]].sum() == 0 and b[T1:].sum() >= 121 and a[T1:].sum() == 0
    r.close()


# ---- 6. sub-windows -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", PATHS)
def test_sub_windows(bins):
    import f_renderer_amd as fr
    sc = D.scene("many")
    r = _renderer(fr, sc, options=(("visible_lds_bins", bins),))
    dl, _ = _list(r, fr, sc)
    some = 0
    for x0, x1, y0, y1 in [(0, 1, 0, H), (5, 6, 3, 40), (0, 63, 0, H), (1, 64, 0, 50), (3, 67, 0, H), (0, 65, 7, 90), (37, W, 11, 77), (0, W, 0, H)]:
        r.clear(*D.CLEAR)
        r.geometry_list(dl)
        r.rasterization((x0, x1), (y0, y1), fr.PS_PHONG)
        t = r.readback()[2]                                   # entry (cy - y0) * x1 + (cx - x0) of the flat target
        gi, gt = _assert_counts(r, t, win=((x0, x1), (y0, y1)), device=(x1 - x0) in (63, 65, W - 37))
        idx = (np.arange(y1 - y0)[:, None] * x1 + np.arange(x1 - x0)[None, :]).reshape(-1)
        assert gi.sum() == gt.sum() == (t[idx] != NONE).sum()
        some += int(gi.sum())
    assert some > 1000
    r.close()


# ---- 7. replay -------------------------------------------------------------------------------------------------------------

def test_counts_are_replayed_with_a_failed_pass(oracle):
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    of, _, per = D.oracle_frame(oracle, "clipped")
    r = _renderer(fr, sc, options=(("fan_capacity", 16), ("bin_capacity", 64)))
    dl, _ = _list(r, fr, sc)
    n, T = sc.nitems, sum(per)
    early, early_t, late, late_t = _buffers(max(n, T) + 2, 4)
    r.clear(*D.CLEAR)
    r.geometry_list(dl)                                           # the fan space overflows on the device
    r.visible_pixels("item", out_ptr=early.data_ptr(), entries=n + 2)        # nothing is drawn yet: cancelled or replayed, it ends all zero
    r.visible_pixels("triangle", out_ptr=early_t.data_ptr(), entries=T + 2)
    r.rasterization(*FULL, fr.PS_PHONG)                           # repairs: geometry, the counts and the raster pass run again
    r.visible_pixels("item", out_ptr=late.data_ptr(), entries=n + 2)
    r.visible_pixels("triangle", out_ptr=late_t.data_ptr(), entries=T + 2)
    r.sync()
    assert r.stats()["replays"] > 0
    np.testing.assert_array_equal(r.readback()[2], of.tri_id)
    assert not _host(early, n + 2).any() and not _host(early_t, T + 2).any()
    np.testing.assert_array_equal(_host(late, n + 2), want_counts(of.tri_id, *FULL, bounds=bounds_of(per), entries=n + 2))
    np.testing.assert_array_equal(_host(late_t, T + 2), want_counts(of.tri_id, *FULL, units=T, entries=T + 2))
    # after a clear the id target holds nothing of the pass: zeros, n items, no triangles
    r.clear(*D.CLEAR)
    gi, gt = r.visible_pixels("item"), r.visible_pixels("triangle")
    assert gi.size == n and not gi.any() and gt.size == 0
    buf = _buffers(n + 2)
    r.visible_pixels("item", out_ptr=buf.data_ptr(), entries=n + 2)
    r.sync()
    assert not _host(buf, n + 2).any()
    np.testing.assert_array_equal(r.readback()[2], np.full(W * H, NONE, np.uint32))
    r.close()


# ---- 8. target sets and partitions ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("fif", [2, 1])
def test_two_frames_count_into_their_own_buffers(oracle, fif):
    import f_renderer_amd as fr
    a, b = D.scene("sizes"), D.scene("empties")
    (fa, _, pa), (fb, _, pb) = D.oracle_frame(oracle, "sizes"), D.oracle_frame(oracle, "empties")
    r = _renderer(fr, a, options=(("frames_in_flight", fif),))
    la, _ = _list(r, fr, a)
    lb, _ = _list(r, fr, b)
    for _ in range(2):
        A, B = _buffers(8, 2)
        r.clear(*D.CLEAR)
        r.draw_list(la, fr.PS_PHONG)
        r.visible_pixels("item", out_ptr=A.data_ptr(), entries=8)
        r.clear(*D.CLEAR)
        r.draw_list(lb, fr.PS_PHONG)
        r.visible_pixels("item", out_ptr=B.data_ptr(), entries=8)
        ga, gb = _fenced(r, [A, B])
        assert ga[:8].tolist() == [121, 104, 112, 115, 165, 128, 34, 0] and gb[:8].tolist() == [0, 222, 0, 0, 253, 0, 0, 0]
    np.testing.assert_array_equal(r.readback()[2], fb.tri_id)
    r.close()


def test_caller_bound_targets(oracle):
    import torch
    import f_renderer_amd as fr
    sc = D.scene("sizes")
    of, _, per = D.oracle_frame(oracle, "sizes")
    r = _renderer(fr, sc)
    c_ = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    d_ = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    t_ = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
    dl, _ = _list(r, fr, sc)
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_PHONG)
    gi, _ = _assert_counts(r, of.tri_id, bounds=bounds_of(per), T=sum(per))
    assert gi.tolist() == [121, 104, 112, 115, 165, 128, 34]
    np.testing.assert_array_equal(_host(t_), of.tri_id)
    r.close()


@pytest.mark.parametrize("world,blocked", [(2, False), (2, True), (3, False), (3, True)])
def test_partitioned_ranks_count_their_own_rows_and_add_up(oracle, world, blocked):
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    of, _, per = D.oracle_frame(oracle, "clipped")
    bnd, T = bounds_of(per), sum(per)
    tot_i, tot_t = np.zeros(sc.nitems, np.int64), np.zeros(T, np.int64)
    for rank in range(world):
        rows = owned_pixel_rows(H, rank, world, blocked)
        mine = np.where(np.repeat(rows, W), of.tri_id, NONE).astype(np.uint32)
        r = _renderer(fr, sc, options=(("visible_lds_bins", rank % 2),))
        r.set_partition(rank, world, blocked)
        dl, _ = _list(r, fr, sc)
        r.clear(*D.CLEAR)
        r.geometry_list(dl)                                       # (never filters)
        r.rasterization(*FULL, fr.PS_PHONG)
        gi, gt = _assert_counts(r, mine, bounds=bnd, T=T)
        tot_i += gi
        tot_t += gt
        if rank == 0:
            r.clear(*D.CLEAR)
            r.draw_list(dl, fr.PS_PHONG)                          # filters the setup list: where item_ranges() fails
            for unit in ("item", "triangle"):
                with pytest.raises(fr.FrrError) as e:
                    r.visible_pixels(unit)
                assert e.value.code == fr.FRR_ERR_INVALID
            with pytest.raises(fr.FrrError):
                r.item_ranges()
        r.close()
    np.testing.assert_array_equal(tot_i, want_counts(of.tri_id, *FULL, bounds=bnd))
    np.testing.assert_array_equal(tot_t, want_counts(of.tri_id, *FULL, units=T))


# ---- 9. nothing else moves -----------------------------------------------------------------------------------------------

def test_targets_and_statistics_are_untouched():
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    r = _renderer(fr, sc)
    dl, _ = _list(r, fr, sc)
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_PHONG)
    c0, d0, t0 = r.readback()
    s0 = r.stats()
    buf = _buffers(64)
    for bins in PATHS:
        r.set_option("visible_lds_bins", bins)
        for unit in ("item", "triangle"):
            r.visible_pixels(unit, out_ptr=buf.data_ptr(), entries=64)
            r.visible_pixels(unit)
            r.visible_pixels(unit, width_range=(3, 67), height_range=(0, H))
    c1, d1, t1 = r.readback()
    assert c0.tobytes() == c1.tobytes() and d0.tobytes() == d1.tobytes() and t0.tobytes() == t1.tobytes() and r.stats() == s0
    a = r.visible_pixels("triangle")
    assert a.tobytes() == r.visible_pixels("triangle").tobytes()                   # integer adds: the same bytes every time
    r.close()


# ---- 10. errors ----------------------------------------------------------------------------------------------------------

def test_errors():
    import f_renderer_amd as fr
    sc = D.scene("sizes")
    r = _renderer(fr, sc)
    buf = _buffers(16)
    p = buf.data_ptr()

    def code(*a, **kw):
        with pytest.raises(fr.FrrError) as e:
            r.visible_pixels(*a, **kw)
        return e.value.code

    assert code("item") == fr.FRR_ERR_INVALID and code("triangle", out_ptr=p, entries=16) == fr.FRR_ERR_INVALID     # before any geometry pass
    dl, _ = _list(r, fr, sc)
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_PHONG)
    want = r.visible_pixels("item")
    for unit in (2, -1):
        assert code(unit, out_ptr=p, entries=16) == fr.FRR_ERR_INVALID and code(unit) == fr.FRR_ERR_INVALID
    for kw in (dict(width_range=(-1, W - 1)), dict(width_range=(-5, 20))):                                         # x0 < 0
        assert code("item", out_ptr=p, entries=16, **kw) == fr.FRR_ERR_UNSUPPORTED and code("item", **kw) == fr.FRR_ERR_UNSUPPORTED
    for kw in (dict(width_range=(5, 5)), dict(width_range=(9, 4)), dict(height_range=(7, 7)), dict(height_range=(9, 2)),   # empty, inverted
               dict(width_range=(0, W + 1)), dict(height_range=(0, H + 1)),                                       # larger than the FrameBuffer
               dict(width_range=(32700, 32768)), dict(height_range=(32700, 32768)), dict(height_range=(-32769, -32700)),   # outside i16
               dict(width_range=(W, 2 * W), height_range=(0, H))):                                                # the depth index leaves the buffer
        assert code("item", out_ptr=p, entries=16, **kw) == fr.FRR_ERR_INVALID, kw
        assert code("triangle", **kw) == fr.FRR_ERR_INVALID, kw
    L, ctx = r._lib, r._ctx
    assert L.frr_visible_pixels(ctx, 0, 0, W, 0, H, None, 16) == fr.FRR_ERR_INVALID                                # NULL
    assert L.frr_visible_pixels(ctx, 0, 0, W, 0, H, p + 2, 4) == fr.FRR_ERR_INVALID                                # not 4-byte aligned
    assert L.frr_visible_pixels_host(ctx, 1, 0, W, 0, H, None, 16, None) == fr.FRR_ERR_INVALID
    assert L.frr_visible_pixels(None, 0, 0, W, 0, H, p, 16) == fr.FRR_ERR_INVALID
    # out_entries == 0: FRR_OK, and nothing happens -- whatever the pointer
    assert L.frr_visible_pixels(ctx, 0, 0, W, 0, H, None, 0) == fr.FRR_OK and L.frr_visible_pixels(ctx, 1, 0, W, 0, H, p + 2, 0) == fr.FRR_OK
    assert L.frr_visible_pixels_host(ctx, 0, 0, W, 0, H, None, 0, None) == fr.FRR_OK
    assert L.frr_visible_pixels(ctx, 5, 0, W, 0, H, None, 0) == fr.FRR_ERR_INVALID                                 # (the other checks still apply)
    r.sync()
    assert (_host(buf) == SENTINEL).all()                                                                          # no refused call wrote anything
    np.testing.assert_array_equal(r.visible_pixels("item"), want)
    with pytest.raises(fr.FrrError):
        r.set_option("visible_lds_bins", fr.VISIBLE_LDS_BINS + 1)
    with pytest.raises(fr.FrrError):
        r.set_option("visible_lds_bins", -1)
    # the profile knows the kernel, behind the kernels it knew before
    r.profile_enable(True, kernels=("k_visible",))
    r.profile_reset()
    r.visible_pixels("item", out_ptr=p, entries=16)
    r.sync()
    assert r.profile_get("k_visible")[1] == 1 and r.profile_get("k_raster")[1] == 0
    r.close()
