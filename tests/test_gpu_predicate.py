"""Predicated list passes (frr_geometry_list_if / frr_draw_list_if): a list pass that keeps item i iff keep[i] >= min_value,
read from the caller's device buffer on the library's streams.  By definition that is the list pass with the mesh of every
dropped item replaced by an empty mesh, so every frame here is held, bit for bit, to the oracle's loop over the kept items
(tests/predicate_scenes.py): depth bits, triangle ids, RGBA8, the setup list, item_ranges, per-item visible_pixels,
tris_setup / frag_covered / frag_nan / draws, and tris_in equal to the list's FULL input count."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import predicate_scenes as P
from . import varyings_scenes as V
from .conftest import assert_depth_equal, owned_pixel_rows
from .test_gpu_drawlist import (_assert_frame, _assert_ranges, _assert_same, _assert_setup, _err, _list_frame, _meshes, _phong_sid, _read,
                                _renderer, _upload)
from .test_gpu_streams import _Alias

pytestmark = pytest.mark.gpu
W, H = P.W, P.H
NONE = P.NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _values(v):
    """a device buffer of one u32 per item (torch has int32: the same bits); a bool mask becomes 0 / 1"""
    import torch
    a = np.asarray(v).astype(np.uint32)
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def _if_frame(r, dl, buf, ps_id, min_value=1, setup=True):
    r.clear(*D.CLEAR)
    r.draw_list_if(dl, buf.data_ptr(), buf.numel(), ps_id, min_value=min_value)
    return _read(r, setup)


def _assert_pred(r, g, sc, exp, K=8, ranges=True):
    """the frame `g` of a predicated pass and what the pass left behind, against expected() = (frame, setup, per item)"""
    of, osetup, per = exp
    _assert_frame(g, of)
    if g["setup"] is not None:
        _assert_setup(g["setup"], osetup, K)
    st = g["st"]
    assert st["tris_in"] == sum(sc.ntris) and st["draws"] == 1, st          # dropped items' inputs included
    assert st["tris_setup"] == of.counters.tris_setup == sum(per) and st["frag_covered"] == of.counters.frag_covered
    assert st["frag_nan"] == of.counters.frag_nan
    if ranges:
        _assert_ranges(r, per)                                              # every item; a dropped one: count 0, first = where it would start
        np.testing.assert_array_equal(r.visible_pixels("item"), P.item_counts(of.tri_id, per))


def _setup(fr, name, options=(), vs="PHONG", kinds=None, stream=None):
    sc = P.scene(name)
    r = _renderer(fr, sc, options=options, stream=stream)
    vs_id = _phong_sid() if vs == "user" else getattr(fr, "VS_" + sc.vs)
    dl = _upload(r, sc, _meshes(r, sc, vs_id, kinds))
    return sc, r, dl


# ---- boundaries of block (256) and wave (64) ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", D.BOUNDARY)
def test_block_and_wave_boundaries(oracle, name):
    """all kept, none kept, the first, the last, every other and a random half of the items, on item sizes around the block and
    the wave in both orders, on 300 items of 1..3 triangles (the flag changes inside every wave) and with empty items; on
    `sizes` also the 256-triangle item alone dropped, and 255 and 257 dropped around it: dropped and kept runs end inside a
    block and inside a wave, and some waves are dropped whole"""
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, name)
    cases = [(k, m) for n, k, m in P.gpu_cases() if n == name and not k.startswith("min")]
    assert len(cases) == (8 if name == "sizes" else 6)
    for label, kept in cases:
        exp = P.expected(oracle, name, kept)
        g = _if_frame(r, dl, _values(kept), fr.PS_PHONG)
        _assert_pred(r, g, sc, exp)
        assert g["st"]["replays"] == 0, label
        if label == "all":                       # ... is frr_draw_list of the same list, statistics included
            gl = _list_frame(r, dl, fr.PS_PHONG)
            _assert_same(g, gl)
            assert g["st"] == gl["st"] and g["st"]["frag_covered"] > 0
        elif label == "none":
            assert (g["t"] == NONE).all() and g["st"]["tris_setup"] == 0 and g["st"]["frag_covered"] == 0
            np.testing.assert_array_equal(g["c"].reshape(-1, 4), np.tile(np.array(D.CLEAR[0], np.uint8), (W * H, 1)))
    r.close()


def test_none_kept_between_two_plain_draws(oracle):
    """a pass that keeps nothing leaves the frame as it was, every item with count 0 and first = the frame's running count, and
    a later plain draw of the frame continues the ids from there"""
    import f_renderer_amd as fr
    sc, other = P.scene("sizes"), D.scene("one")
    kw = D.uniform_kw(oracle, sc, "PHONG")
    of = oracle.Frame(W, H)
    of.clear(*D.CLEAR)
    of.draw(other.item_tris(0), oracle.VS_PHONG, oracle.PS_PHONG, oracle.make_uniforms(model=other.models[0], **kw))
    n_a = int(of.counters.tris_setup)
    of.draw(other.item_tris(0), oracle.VS_PHONG, oracle.PS_PHONG, oracle.make_uniforms(model=sc.models[1], **kw), tri_id_base=n_a)
    assert n_a > 0
    r = _renderer(fr, sc)
    ma = r.upload_mesh(other.item_tris(0), fr.VS_PHONG)
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_PHONG))
    zeros = _values(np.zeros(sc.nitems, bool))
    r.clear(*D.CLEAR)
    r.set_uniforms(model=other.models[0])
    r.draw(ma, fr.PS_PHONG)
    r.draw_list_if(dl, zeros.data_ptr(), sc.nitems, fr.PS_PHONG)
    first, count = r.item_ranges()
    assert first.tolist() == [n_a] * sc.nitems and count.tolist() == [0] * sc.nitems
    assert r.visible_pixels("item").tolist() == [0] * sc.nitems
    r.set_uniforms(model=sc.models[1])
    r.draw(ma, fr.PS_PHONG)
    g = _read(r, setup=False)
    _assert_frame(g, of)
    assert g["st"]["draws"] == 3 and g["st"]["tris_in"] == 2 * other.ntris[0] + sum(sc.ntris) and g["st"]["tris_setup"] == of.counters.tris_setup
    r.close()


# ---- the threshold -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_value", P.THRESHOLD_MINS)
def test_threshold_is_an_unsigned_comparison(oracle, min_value):
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "sizes")
    assert sc.nitems == len(P.THRESHOLD_VALUES)
    kept = P.kept_of(P.THRESHOLD_VALUES, min_value)
    assert kept.tolist() == {6: [0, 0, 0, 1, 1, 1, 1], 0: [1] * 7, 0x80000001: [0, 0, 0, 0, 0, 0, 1]}[min_value]
    g = _if_frame(r, dl, _values(np.array(P.THRESHOLD_VALUES, np.uint32)), fr.PS_PHONG, min_value=min_value)
    _assert_pred(r, g, sc, P.expected(oracle, "sizes", kept))
    r.close()


# ---- clipping ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip_queue", [-1, 1, 0])
def test_clipped_items(oracle, clip_queue):
    """the item whose first and last inputs are clipped dropped, and the only one kept; the item through the near plane
    dropped: a dropped clipped input takes no fan slot -- the setup list and tris_setup are the oracle's"""
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "clipped", options=(("clip_queue", clip_queue),))
    full = P.expected(oracle, "clipped", np.ones(sc.nitems, bool))[2]
    for label, kept in P.clipped_masks().items():
        exp = P.expected(oracle, "clipped", kept)
        g = _if_frame(r, dl, _values(kept), fr.PS_PHONG)
        _assert_pred(r, g, sc, exp)
        assert g["st"]["replays"] == 0 and sum(exp[2]) < sum(full), label
    assert full[P.CLIPPED_SPIKY] > sc.ntris[P.CLIPPED_SPIKY] and full[P.CLIPPED_NEAR] != sc.ntris[P.CLIPPED_NEAR]   # those items do clip
    r.close()


TINY = (("fan_capacity", 16), ("bin_capacity", 64))


def test_replay_reads_the_keep_buffer_again(oracle):
    """fan space and (triangle, tile) lists far too small: the pass is replayed inside the library, keep table and all"""
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "clipped", options=TINY)
    kept = P.clipped_masks()["drop_near"]
    g = _if_frame(r, dl, _values(kept), fr.PS_PHONG)
    assert g["st"]["replays"] > 0
    _assert_pred(r, g, sc, P.expected(oracle, "clipped", kept))
    r.close()


def test_a_predicated_pass_is_never_taken_as_proven(oracle):
    """Tiny work lists, one list, one buffer.  With everything dropped the pass needs nothing of the lists and completes, four
    times over (the passes alternate between workspace sets).  Then the buffer is filled with ones on a created stream, the
    library is told to wait for that stream, and the same call -- same list, same pointer, same window and uniforms -- is
    made again: it needs far more than the lists hold.  Its frame is read through frr_frame_fence and a copy on that stream
    alone and must be whole: a pass taken as proven would cancel its tile kernel and leave the frame clear."""
    import torch
    import f_renderer_amd as fr
    name = "clipped"
    sc = P.scene(name)
    f_none = P.expected(oracle, name, np.zeros(sc.nitems, bool))[0]
    f_all = P.expected(oracle, name, np.ones(sc.nitems, bool))[0]
    assert (f_none.tri_id == NONE).all() and (f_all.tri_id != NONE).sum() > 500
    for kept, overflows in ((np.zeros(sc.nitems, bool), False), (np.ones(sc.nitems, bool), True)):   # on a fresh ctx
        _, r, dl = _setup(fr, name, options=TINY)
        g = _if_frame(r, dl, _values(kept), fr.PS_PHONG, setup=False)
        assert (g["st"]["replays"] >= 1) == overflows, g["st"]
        r.close()
    st = torch.cuda.Stream()
    _, r, dl = _setup(fr, name, options=TINY)
    buf = _values(np.zeros(sc.nitems, bool))

    def fenced_copy():
        r.frame_fence(st.cuda_stream)
        pc, pd, pt = r.target_ptrs()
        with torch.cuda.stream(st):
            return tuple(torch.as_tensor(_Alias(p, (H, W), ts), device="cuda").clone() for p, ts in ((pc, "<i4"), (pd, "<f4"), (pt, "<i4")))
    copies = []
    for _ in range(4):
        r.clear(*D.CLEAR)
        r.draw_list_if(dl, buf.data_ptr(), sc.nitems, fr.PS_PHONG)
        copies.append((f_none, fenced_copy()))
    with torch.cuda.stream(st):                                    # (behind the fence: the earlier passes have read the buffer)
        buf.fill_(1)
    for _ in range(2):
        r.frame_wait(st.cuda_stream)
        r.clear(*D.CLEAR)
        r.draw_list_if(dl, buf.data_ptr(), sc.nitems, fr.PS_PHONG)
        copies.append((f_all, fenced_copy()))
    torch.cuda.synchronize()
    for f, (c, d, t) in copies:
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32).ravel(), f.tri_id)
        np.testing.assert_array_equal(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), f.color)
        assert_depth_equal(d.cpu().numpy(), f.depth)
    r.close()


# ---- stream order ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("fif", [1, 2])
def test_counts_of_one_frame_decide_the_next_with_no_host_wait(oracle, fif, overlap):
    """draw_list, visible_pixels into B, clear, draw_list_if(B): nothing between them but stream order.  The second frame is the
    oracle's over the items that owned a pixel -- and, in depth and colour, the first frame again.  Then B is zeroed on a
    fenced stream after the call has returned: the frame is still that of the counts."""
    import torch
    import f_renderer_amd as fr
    counts = P.hidden_counts(oracle)
    sc, r, dl = _setup(fr, "hidden", options=(("frames_in_flight", fif), ("overlap", overlap)))
    full = P.expected(oracle, "hidden", np.ones(sc.nitems, bool))
    exp = P.expected(oracle, "hidden", counts > 0)
    B = _values(np.zeros(sc.nitems, np.uint32))                    # (zeros: a read that ran ahead of the count would drop everything)
    st = torch.cuda.Stream()
    for _ in range(2):                                             # twice: both frames in flight, both workspace sets
        r.clear(*D.CLEAR)
        r.draw_list(dl, fr.PS_PHONG)
        r.visible_pixels("item", out_ptr=B.data_ptr(), entries=sc.nitems)
        r.clear(*D.CLEAR)
        r.draw_list_if(dl, B.data_ptr(), sc.nitems, fr.PS_PHONG)
        r.frame_fence(st.cuda_stream)
        with torch.cuda.stream(st):
            seen = B.clone()
            B.zero_()
        g = _read(r)                                               # (a synchronisation point)
        np.testing.assert_array_equal(seen.cpu().numpy().view(np.uint32), counts)
        _assert_pred(r, g, sc, exp)
        assert_depth_equal(g["d"], full[0].depth)
        np.testing.assert_array_equal(g["c"], full[0].color)
        assert g["st"]["tris_setup"] < full[0].counters.tris_setup
        st.synchronize()                                           # (B is zero again before the next count is issued)
    r.close()


# ---- other paths -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("option", [("raster_sweep", 1), ("bin_atomics", 1)])
def test_other_paths(oracle, option):
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "clipped", options=(option,))
    for kept in (P.clipped_masks()["drop_spiky"], P.masks(sc.nitems)["alternating"]):
        g = _if_frame(r, dl, _values(kept), fr.PS_PHONG)
        _assert_pred(r, g, sc, P.expected(oracle, "clipped", kept))
    r.close()


def test_caller_bound_targets_in_flight(oracle):
    """three caller-bound target sets in rotation under bound_targets_in_flight, a different mask every frame, each frame read
    through a fence alone"""
    import torch
    import f_renderer_amd as fr
    st = torch.cuda.Stream()
    sc, r, dl = _setup(fr, "clipped", options=(("bound_targets_in_flight", 1),), stream=st.cuda_stream)
    sets = [tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32)) for _ in range(3)]
    ms = list(P.clipped_masks().values()) + [P.masks(sc.nitems)["alternating"], P.masks(sc.nitems)["all"]]
    bufs = [_values(m) for m in ms]
    copies = []
    for k, m in enumerate(ms):
        r.frame_wait(st.cuda_stream)
        r.bind_targets(*(x.data_ptr() for x in sets[k % 3]))
        r.clear(*D.CLEAR)
        r.draw_list_if(dl, bufs[k].data_ptr(), sc.nitems, fr.PS_PHONG)
        r.frame_fence(st.cuda_stream)
        with torch.cuda.stream(st):
            copies.append(tuple(x.clone() for x in sets[k % 3]))
    torch.cuda.synchronize()
    for m, (c, d, t) in zip(ms, copies):
        f = P.expected(oracle, "clipped", m)[0]
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32).ravel(), f.tri_id)
        np.testing.assert_array_equal(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), f.color)
        assert_depth_equal(d.cpu().numpy(), f.depth)
    r.close()


# ---- meshes and shaders ------------------------------------------------------------------------------------------------

def test_plain_indexed_and_device_bound_items_dropped_in_turn(oracle):
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "mix", kinds=["plain", "indexed", "dev", "dev_indexed"])
    for i in range(sc.nitems):
        kept = np.arange(sc.nitems) != i
        g = _if_frame(r, dl, _values(kept), fr.PS_PHONG)
        _assert_pred(r, g, sc, P.expected(oracle, "mix", kept))
    r.close()


@pytest.mark.parametrize("case", ["user", "user_vs_builtin_ps"])
def test_user_shaders(oracle, case):
    """the run-time compiled build of the same kernels: a user vertex-and-pixel-shader list, and a user-VS list under the
    built-in pixel shader"""
    import f_renderer_amd as fr
    if case == "user":
        sc, r, dl = _setup(fr, "clipped", vs="user")
        name, kept, ps_id = "clipped", P.clipped_masks()["drop_spiky"], _phong_sid()
    else:
        sc, r, dl = _setup(fr, "mix", vs="user", kinds=["plain", "indexed", "plain", "indexed"])
        name, kept, ps_id = "mix", np.arange(sc.nitems) != 1, fr.PS_PHONG
    g = _if_frame(r, dl, _values(kept), ps_id)
    _assert_pred(r, g, sc, P.expected(oracle, name, kept))
    assert g["st"]["frag_covered"] > 0
    r.close()


@pytest.mark.parametrize("mode", ["NEG", "POS"])
@pytest.mark.parametrize("drop_mirrored", [True, False])
def test_cull_still_applies_to_the_kept_items(oracle, mode, drop_mirrored):
    import f_renderer_amd as fr
    sc = P.scene("mirrored")
    cull = getattr(fr, "CULL_" + mode)
    kept = np.array([True, True, not drop_mirrored])
    keep = [ck & ik for ck, ik in zip(D.cull_keep(sc, cull), P.oracle_keep(sc, kept))]
    exp = D.oracle_list_loop(oracle, sc, keep=keep)
    r = _renderer(fr, sc)
    dl = _upload(r, sc, _meshes(r, sc, fr.VS_GOURAUD))
    r.set_cull(cull)
    g = _if_frame(r, dl, _values(kept), fr.PS_COLOR)
    r.set_cull(fr.CULL_NONE)
    _assert_pred(r, g, sc, exp, K=3)
    assert 0 < exp[2][0] < sc.ntris[0] and (exp[2][2] == 0) == drop_mirrored
    r.close()


# ---- downstream consumers ----------------------------------------------------------------------------------------------

def test_one_predicated_geometry_two_raster_windows(oracle):
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "clipped")
    kept = P.clipped_masks()["drop_near"]
    wins = [(0, 64, 0, H), (0, W, 0, 40)]
    buf = _values(kept)
    r.clear(*D.CLEAR)
    n = r.geometry_list_if(dl, buf.data_ptr(), sc.nitems, count=True)
    for win in wins:
        r.rasterization(win[:2], win[2:], fr.PS_PHONG)
    of = oracle.Frame(W, H)
    of.clear(*D.CLEAR)
    pers = [D.oracle_list_loop(oracle, sc, frame=of, window=win, tri_id_base=0, keep=P.oracle_keep(sc, kept))[2] for win in wins]
    assert n == sum(pers[0])
    _assert_frame(_read(r, setup=False), of)
    _assert_ranges(r, pers[0])
    r.close()


def test_wireframe_after_a_predicated_pass(oracle):
    import f_renderer_amd as fr
    from . import lines_reference as R
    sc, r, dl = _setup(fr, "clipped")
    kept = P.clipped_masks()["drop_spiky"]
    of, osetup, _ = P.expected(oracle, "clipped", kept)
    color = (255, 200, 0, 255)
    buf = _values(kept)
    r.clear(*D.CLEAR)
    r.draw_list_if(dl, buf.data_ptr(), sc.nitems, fr.PS_PHONG)
    r.draw_wireframe(color)
    c, d, t = r.readback()
    setup = r.setup_triangles()
    np.testing.assert_array_equal(setup["spi"], osetup["spi"])
    segs = []
    for tri in setup["spi"]:
        for k in range(3):
            (xa, ya), (xb, yb) = tri[k], tri[(k + 1) % 3]
            if 0 <= xa < W and 0 <= xb < W and 0 <= ya < H and 0 <= yb < H:
                segs.append((xa, ya, xb, yb))
    xyxy = np.array(segs, np.uint32).reshape(-1, 4)
    assert len(xyxy) > 0
    np.testing.assert_array_equal(t, of.tri_id)
    assert_depth_equal(d, of.depth)
    np.testing.assert_array_equal(c, R.draw_lines(of.color.copy(), xyxy, np.tile(np.array(color, np.uint8), (len(xyxy), 1))))
    r.close()


def test_resolve_and_ranged_shade_per_kept_item(oracle):
    """draw_list_if(PS_DEPTH) + resolve_varyings + one ranged shade_varyings per item from item_ranges == the forward frame;
    a dropped item's range has count 0 and shading it writes nothing"""
    import torch
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "clipped")
    kept = P.clipped_masks()["drop_near"]
    of, _, per = P.expected(oracle, "clipped", kept)
    buf = _values(kept)
    vary = torch.full((W * H, 8), V.SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.clear(*D.CLEAR)
    r.draw_list_if(dl, buf.data_ptr(), sc.nitems, fr.PS_DEPTH)
    r.resolve_varyings(vary.data_ptr(), W * H)
    first, count = r.item_ranges()
    assert count.tolist() == per and count[P.CLIPPED_NEAR] == 0
    before = r.readback()[0].copy()
    r.shade_varyings(fr.PS_PHONG, vary.data_ptr(), W * H, 8, ids=(int(first[P.CLIPPED_NEAR]), int(count[P.CLIPPED_NEAR])))
    np.testing.assert_array_equal(r.readback()[0], before)          # the dropped item: nothing
    for i in range(sc.nitems):
        r.shade_varyings(fr.PS_PHONG, vary.data_ptr(), W * H, 8, ids=(int(first[i]), int(count[i])))
    g = _read(r, setup=False)
    _assert_frame(g, of)
    assert (before != of.color).any()
    r.close()


# ---- partition ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocked", [False, True])
def test_partitioned_ranks_stitch_and_their_counts_add_up(oracle, blocked):
    import f_renderer_amd as fr
    name = "clipped"
    kept = P.clipped_masks()["drop_spiky"]
    of, _, per = P.expected(oracle, name, kept, "DEPTH")
    seen, total = np.zeros(H, bool), np.zeros(len(per), np.uint64)
    for rank in (0, 1):
        sc, r, dl = _setup(fr, name)
        r.set_partition(rank, 2, blocked)
        buf = _values(kept)
        g = _if_frame(r, dl, buf, fr.PS_DEPTH, setup=False)        # the partition filter of the draw
        own = owned_pixel_rows(H, rank, 2, blocked)
        assert own.any() and (g["t"].reshape(H, W)[own] != NONE).any()
        _assert_frame(g, of, own)
        seen |= own
        n = C.c_uint64()
        assert r._lib.frr_geometry_item_ranges(r._ctx, None, None, 0, C.byref(n)) == fr.FRR_ERR_INVALID   # (a filtered list)
        r.clear(*D.CLEAR)
        r.geometry_list_if(dl, buf.data_ptr(), sc.nitems)
        r.rasterization((0, W), (0, H), fr.PS_DEPTH)
        _assert_ranges(r, per)
        total += r.visible_pixels("item")
        _assert_frame(_read(r, setup=False), of, own)
        r.close()
    assert seen.all()
    np.testing.assert_array_equal(total, P.item_counts(of.tri_id, per))


# ---- errors ------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_ctx_drawing(oracle):
    import torch
    import f_renderer_amd as fr
    sc, r, dl = _setup(fr, "clipped")
    L, ctx = r._lib, r._ctx
    kept = P.clipped_masks()["drop_spiky"]
    exp = P.expected(oracle, "clipped", kept)
    buf = _values(kept)
    p, n = buf.data_ptr(), sc.nitems

    def still_draws():
        _assert_pred(r, _if_frame(r, dl, buf, fr.PS_PHONG), sc, exp)

    def refused(rc, word):
        assert rc == fr.FRR_ERR_INVALID and word in _err(r), (rc, _err(r))
        still_draws()
    r.clear(*D.CLEAR)
    for bad in (-1, 99):                                            # an unknown list, as frr_draw_list answers
        assert L.frr_draw_list(ctx, bad, fr.PS_PHONG, 0, W, 0, H) == fr.FRR_ERR_INVALID
        want = _err(r)
        refused(L.frr_draw_list_if(ctx, bad, p, n, 1, fr.PS_PHONG, 0, W, 0, H), want)
        refused(L.frr_geometry_list_if(ctx, bad, p, n, 1, None), want)
    refused(L.frr_draw_list_if(ctx, dl.id, p, n - 1, 1, fr.PS_PHONG, 0, W, 0, H), "keep_entries")
    refused(L.frr_geometry_list_if(ctx, dl.id, p, 0, 1, None), "keep_entries")
    refused(L.frr_draw_list_if(ctx, dl.id, None, n, 1, fr.PS_PHONG, 0, W, 0, H), "NULL")
    refused(L.frr_geometry_list_if(ctx, dl.id, None, n, 1, None), "NULL")
    refused(L.frr_draw_list_if(ctx, dl.id, p + 2, n, 1, fr.PS_PHONG, 0, W, 0, H), "aligned")
    refused(L.frr_geometry_list_if(ctx, dl.id, p + 1, n, 1, None), "aligned")
    # window and shader errors are those of frr_draw_list
    for args in ((fr.PS_PHONG, 10, 5, 0, H), (fr.PS_PHONG, 0, W + 1, 0, H), (fr.PS_COLOR, 0, W, 0, H), (99, 0, W, 0, H)):
        r.clear(*D.CLEAR)
        rc_plain = L.frr_draw_list(ctx, dl.id, *args)
        want = _err(r)
        r.clear(*D.CLEAR)
        assert rc_plain != fr.FRR_OK and L.frr_draw_list_if(ctx, dl.id, p, n, 1, *args) == rc_plain and _err(r) == want
        still_draws()
    # a list without items is a valid pass that emits nothing, and its buffer may be NULL
    none = r.upload_draw_list([], np.zeros((0, 16), np.float32))
    r.clear(*D.CLEAR)
    assert L.frr_draw_list_if(ctx, none.id, None, 0, 1, fr.PS_PHONG, 0, W, 0, H) == fr.FRR_OK
    cnt = C.c_uint64(7)
    assert L.frr_geometry_list_if(ctx, none.id, None, 0, 1, C.byref(cnt)) == fr.FRR_OK and cnt.value == 0
    st = r.stats()
    assert st["draws"] == 2 and st["tris_in"] == 0 and st["tris_setup"] == 0
    still_draws()
    # a freed list, and one killed by freeing a mesh it names
    lid = none.id
    r.free_draw_list(none)
    refused(L.frr_draw_list_if(ctx, lid, None, 0, 1, fr.PS_PHONG, 0, W, 0, H), "bad draw list id")
    gone = r.upload_mesh(S.patch(9), fr.VS_PHONG)
    dead = r.upload_draw_list([gone], sc.models[:1])
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gone.free()
    refused(L.frr_draw_list_if(ctx, dead.id, one.data_ptr(), 1, 1, fr.PS_PHONG, 0, W, 0, H), "dead")
    refused(L.frr_geometry_list_if(ctx, dead.id, one.data_ptr(), 1, 1, None), "dead")
    r.close()


# ---- the C++ host and the example --------------------------------------------------------------------------------------

def test_cpp_example_reuses_the_counts_of_a_frame(tmp_path):
    """examples/phong_headless --list --visible --reuse (frr::Renderer::draw_list_if): a narrow frame, so that the outer
    columns of the grid of objects are off screen -- the second frame drops them and is, in colour, the first again; what the
    run prints and writes without --reuse stays what it was"""
    import f_renderer_amd as fr
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "phong_headless"])
    exe = os.path.join(ROOT, "examples", "phong_headless")
    obj, tga = (os.path.join(ROOT, "tests", "golden", n) for n in ("cube.obj", "checker24.tga"))
    cw, ch, n = 64, 160, 12
    runs = {}
    for mode, extra in (("visible", []), ("reuse", ["--reuse"])):
        op = str(tmp_path / (mode + ".rgba"))
        out = subprocess.run([exe, "--assets", obj, tga, str(cw), str(ch), op, "--instances", str(n), "--list", "--visible"] + extra,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        runs[mode] = (out.stdout, open(op, "rb").read())
    assert runs["reuse"][1] == runs["visible"][1] and runs["reuse"][0].startswith(runs["visible"][0])
    assert "reuse:" not in runs["visible"][0]
    m = re.search(r"^reuse: dropped (\d+) of (\d+) items, colour equal: (\w+)$", runs["reuse"][0], re.M)
    assert m, runs["reuse"][0]
    dropped, total, equal = int(m.group(1)), int(m.group(2)), m.group(3)
    assert total == n and 1 <= dropped < n and equal == "yes"
    assert "items that own no pixel: %d of %d" % (dropped, n) in runs["reuse"][0]
    out = subprocess.run([exe, "--assets", obj, tga, str(cw), str(ch), str(tmp_path / "x.rgba"), "--list", "--reuse"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--reuse goes with" in out.stderr
