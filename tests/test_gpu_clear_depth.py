"""Draws over a clear depth other than 0.0 against the C oracle (scenes and classes: tests/clear_depth_scenes.py; their
input conditions are also checked without a GPU by tests/test_clear_depth_oracle.py).  The bar is test_gpu_parity's: ids,
depth bits (a NaN has to be a NaN), RGBA8 and the statistics equal the oracle's, no tolerance.

frr_clear's depth is the first key of every pixel of a fused-clear draw (tile_load_keys), the start of all four levels of
the hierarchical-z tables (the halved 4-pixel cells included), what both resolves and tile_fill_clear write where nobody
won, what k_clear and the bring-up-to-date of a partitioned rank's other rows write, and per-frame state that travels with
two frames in flight, with replays and with the deferred clear of a target set bound earlier.  With a clear to +0.0 no
triangle of positive rhw is ever culled against the clear constant, no fragment ties with it, no fragment of negative rhw
wins a pixel unless a NaN fragment came before it, and the depth buffer never starts from a NaN.  Early-z runs with
fragment counting OFF only, so every case that can runs both ways (frag_covered is compared while counting is on).
"""
import numpy as np
import pytest

from . import clear_depth_scenes as cs
from . import user_shaders
from .conftest import assert_depth_equal, owned_pixel_rows

pytestmark = pytest.mark.gpu

W0, H0 = cs.SIZES[0]
_SIZE_IDS = [f"{w}x{h}" for w, h in cs.SIZES]


def _renderer(W, H, options=(), partition=None, stream=None):
    import f_renderer_amd as fr
    r = fr.Renderer(W, H, stream=stream)
    for k, v in dict(options).items():
        r.set_option(k, v)
    if partition:
        r.set_partition(partition[0], partition[1], blocked=partition[2])
    return r


def _same_images(c, d, t, f, note):
    np.testing.assert_array_equal(np.asarray(t, np.uint32).ravel(), f.tri_id, err_msg=f"{note}: triangle ids differ")
    assert_depth_equal(d, f.depth, err_msg=f"{note}: depth bits differ")
    if c is not None:
        np.testing.assert_array_equal(c, f.color, err_msg=f"{note}: RGBA8 differs")


def _same(r, f, count, note):
    """The context's frame equals the oracle's: images and statistics."""
    c, d, t = r.readback()
    _same_images(c, d, t, f, note)
    st, oc = r.stats(), f.counters.as_dict()
    assert st["tris_setup"] == oc["tris_setup"] and st["tris_in"] == oc["tris_in"] and st["frag_nan"] == oc["frag_nan"], (note, st, oc)
    if count:
        assert st["frag_covered"] == oc["frag_covered"], (note, st, oc)
    return st


def _two_frames_both_ways(oracle, r, W, H, cls, variants=cs.VARIANTS):
    """Per variant, with counting on and off: two frames in a row, so that the second starts from the first's content."""
    import f_renderer_amd as fr
    clear = cs.clear_depths(oracle, W, H)[cls]
    for variant in variants:
        f = cs.oracle_frame(oracle, W, H, clear, variant)
        vs, ps = cs.shaders(fr, variant)
        m = r.upload_mesh(cs.mesh(variant), vs)
        for count in (True, False):
            r.set_count_fragments(count)
            for k in range(2):
                r.clear(cs.RGBA, clear)
                r.draw(m, ps)
                _same(r, f, count, f"{cls} {variant} count={count} frame {k}")


# ---- a: every class on the default path --------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", cs.CLASSES)
@pytest.mark.parametrize("variant", cs.VARIANTS)
@pytest.mark.parametrize("size", cs.SIZES, ids=_SIZE_IDS)
def test_every_clear_depth_on_the_default_path(oracle, size, variant, cls):
    W, H = size
    r = _renderer(W, H)
    try:
        _two_frames_both_ways(oracle, r, W, H, cls, (variant,))
    finally:
        r.close()


# ---- b: the alternative paths ------------------------------------------------------------------------------------------------

PATHS = {"sweep": {"raster_sweep": 1}, "eager": {"clear_eager": 1}, "atomics": {"bin_atomics": 1}, "nw3": {"raster_nw": 3},
         "nw16": {"raster_nw": 16}, "tile_order2": {"tile_order": 2}}


@pytest.mark.parametrize("cls", cs.PATH_CLASSES)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_clear_depth_on_the_alternative_paths(oracle, path, cls):
    """raster_sweep: the clear is a kernel of its own and the keys are loaded from the buffer; clear_eager: the same for the
    span kernel; bin_atomics: the CSR binning; three and sixteen waves per tile; a shuffled tile order."""
    r = _renderer(W0, H0, PATHS[path])
    try:
        _two_frames_both_ways(oracle, r, W0, H0, cls)
    finally:
        r.close()


# ---- c: two draws in one frame -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", cs.PATH_CLASSES)
@pytest.mark.parametrize("variant", cs.VARIANTS)
def test_second_draw_loads_the_clear_negative_depths_and_nans(oracle, variant, cls):
    """The scene split in halves: only the first draw carries the clear; the second loads its keys from a depth buffer that
    holds the clear value, negative depths and NaNs."""
    import f_renderer_amd as fr
    clear = cs.clear_depths(oracle, W0, H0)[cls]
    tris = cs.mesh(variant)
    h = tris.shape[0] // 2
    ovs, ops = cs.shaders(oracle, variant)
    f = oracle.Frame(W0, H0)
    f.clear(cs.RGBA, clear)
    u = oracle.make_uniforms()
    f.draw(tris[:h], ovs, ops, u)
    with np.errstate(invalid="ignore"):
        assert np.isnan(f.depth).any() and (f.depth < 0).any() and (f.tri_id == cs.NOBODY).any()
    f.draw(tris[h:], ovs, ops, u, tri_id_base=int(f.counters.tris_setup))
    vs, ps = cs.shaders(fr, variant)
    r = _renderer(W0, H0)
    try:
        a, b = r.upload_mesh(tris[:h], vs), r.upload_mesh(tris[h:], vs)
        for count in (True, False):
            r.set_count_fragments(count)
            r.clear(cs.RGBA, clear)
            r.draw(a, ps)
            r.draw(b, ps)
            st = _same(r, f, count, f"{cls} {variant} count={count}")
            assert st["draws"] == 2
    finally:
        r.close()


# ---- d: a sub-window draw behind a pending clear -----------------------------------------------------------------------------

@pytest.mark.parametrize("cls", cs.PATH_CLASSES)
def test_sub_window_draw_behind_a_pending_clear(oracle, cls):
    """The window is smaller than the frame, so the clear is settled by k_clear (the whole buffer holds the clear depth) and
    the draw, with the depth stride x1, loads its keys from it."""
    import f_renderer_amd as fr
    clear = cs.clear_depths(oracle, W0, H0)[cls]
    x0, x1, y0, y1 = cs.SUB_WINDOW
    r = _renderer(W0, H0)
    try:
        for variant in cs.VARIANTS:
            f = cs.oracle_frame(oracle, W0, H0, clear, variant, window=cs.SUB_WINDOW)
            vs, ps = cs.shaders(fr, variant)
            m = r.upload_mesh(cs.mesh(variant), vs)
            for count in (True, False):
                r.set_count_fragments(count)
                r.clear(cs.RGBA, clear)
                r.draw(m, ps, (x0, x1), (y0, y1))
                _same(r, f, count, f"{cls} {variant} count={count}")
    finally:
        r.close()


# ---- e: a window with x0 < 0 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", ["mid", "nan"])
@pytest.mark.parametrize("variant", cs.VARIANTS)
def test_negative_x0_window_over_a_clear_depth(oracle, variant, cls):
    """k_raster_entries: one thread per depth ENTRY replays the reference's loop, starting from what k_clear left there."""
    import f_renderer_amd as fr
    clear = cs.clear_depths(oracle, W0, H0)[cls]
    x0, x1, y0, y1 = cs.NEG_WINDOW
    tris = cs.scene_shifted()
    if variant == "color":
        tris = cs.ls.with_colors(tris, 71)
    f = cs.oracle_frame(oracle, W0, H0, clear, variant, window=cs.NEG_WINDOW, tris=tris)
    assert f.counters.frag_nan > 0 and (f.tri_id != cs.NOBODY).sum() > 1000
    vs, ps = cs.shaders(fr, variant)
    r = _renderer(W0, H0)
    try:
        m = r.upload_mesh(tris, vs)
        for k in range(2):
            r.clear(cs.RGBA, clear)
            r.draw(m, ps, (x0, x1), (y0, y1))
            _same(r, f, True, f"{cls} {variant} frame {k}")
    finally:
        r.close()


# ---- f: partition ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", cs.PATH_CLASSES)
@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_ranks_over_a_clear_depth(oracle, world, blocked, cls):
    """Own rows equal the oracle's; after readback the rows of the other ranks hold the clear values, the depth's bits the
    clear depth's (k_clear_unowned_rows).  Depth-only with counting off, PS_COLOR with counting on."""
    import f_renderer_amd as fr
    clear = cs.clear_depths(oracle, W0, H0)[cls]
    for variant, count in (("depth", False), ("color", True)):
        f = cs.oracle_frame(oracle, W0, H0, clear, variant)
        oc = f.counters.as_dict()
        vs, ps = cs.shaders(fr, variant)
        covered = 0
        for rank in range(world):
            r = _renderer(W0, H0, partition=(rank, world, blocked))
            try:
                r.set_count_fragments(count)
                m = r.upload_mesh(cs.mesh(variant), vs)
                for _ in range(2):
                    r.clear(cs.RGBA, clear)
                    r.draw(m, ps)
                c, d, t = r.readback()
                st = r.stats()
            finally:
                r.close()
            note = f"{cls} {variant} rank {rank}/{world} blocked={blocked}"
            assert st["tris_setup"] == oc["tris_setup"], (note, st, oc)
            covered += st["frag_covered"]
            own = np.repeat(owned_pixel_rows(H0, rank, world, blocked), W0)
            np.testing.assert_array_equal(t[own], f.tri_id[own], err_msg=note)
            assert_depth_equal(d[own], f.depth[own], err_msg=note)
            np.testing.assert_array_equal(c.reshape(-1, 4)[own], f.color.reshape(-1, 4)[own], err_msg=note)
            assert (t[~own] == cs.NOBODY).all(), note
            assert (c.reshape(-1, 4)[~own] == np.array(cs.RGBA, np.uint8)).all(), note
            rest = d[~own]
            assert rest.size and (np.isnan(rest).all() if cls == "nan" else (rest.view(np.uint32) == cs.bits(clear)).all()), note
        if count:
            assert covered == oc["frag_covered"], (cls, variant, world, blocked)


# ---- g: replay ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", ["mid", "pos_inf"])
@pytest.mark.parametrize("variant", cs.VARIANTS)
@pytest.mark.parametrize("count", [True, False])
def test_replayed_draw_starts_from_the_same_clear_depth(oracle, count, variant, cls):
    """Work lists far too small for the scene: the draw overflows them and is replayed; the replay must carry the clear again."""
    import f_renderer_amd as fr
    clear = cs.clear_depths(oracle, W0, H0)[cls]
    f = cs.oracle_frame(oracle, W0, H0, clear, variant)
    vs, ps = cs.shaders(fr, variant)
    r = _renderer(W0, H0, {"bin_capacity": 300, "fan_capacity": 16})
    try:
        r.set_count_fragments(count)
        m = r.upload_mesh(cs.mesh(variant), vs)
        r.clear(cs.RGBA, clear)
        r.draw(m, ps)
        st = _same(r, f, count, f"{cls} {variant} count={count}")
        assert st["replays"] > 0, st
        r.clear(cs.RGBA, clear)
        r.draw(m, ps)
        _same(r, f, count, f"{cls} {variant} count={count}, the lists grown")
    finally:
        r.close()


# ---- h: two frames in flight -------------------------------------------------------------------------------------------------

FLIGHT = ("mid", "nan", "pos_inf", "neg_mid", "neg_inf")      # five classes over two scenes: every pairing within ten frames


def _flight_plan(oracle, W, H, variant, frames=10):
    cd = cs.clear_depths(oracle, W, H)
    plan = []
    for i in range(frames):
        clear = cd[FLIGHT[i % len(FLIGHT)]]
        plan.append((i % 2, clear, cs.oracle_frame(oracle, W, H, clear, variant, which=i % 2)))
    return plan


@pytest.mark.parametrize("variant", cs.VARIANTS)
def test_own_targets_in_flight_with_a_clear_depth_per_frame(oracle, variant):
    """Two scenes AND the clear depth alternate from frame to frame, no host synchronisation in between; every frame is read
    on the caller's stream through frr_frame_fence + frr_target_ptrs and must be the oracle's frame with ITS clear depth."""
    import torch
    import f_renderer_amd as fr
    from .test_gpu_streams import _Alias
    W, H = W0, H0
    plan = _flight_plan(oracle, W, H, variant)
    vs, ps = cs.shaders(fr, variant)
    st = torch.cuda.Stream()
    r = _renderer(W, H, {"frames_in_flight": 2}, stream=st.cuda_stream)
    try:
        r.set_count_fragments(False)
        meshes = [r.upload_mesh(cs.mesh(variant, k), vs) for k in (0, 1)]
        taken, ptrs = [], set()
        for i, (which, clear, _) in enumerate(plan):
            r.clear(cs.RGBA, clear)
            r.draw(meshes[which], ps)
            r.frame_fence(st.cuda_stream)
            pc, pd, pt = r.target_ptrs()
            ptrs.add(pd)
            with torch.cuda.stream(st):
                taken.append((torch.as_tensor(_Alias(pc, (H, W), "<i4"), device="cuda").clone(),
                              torch.as_tensor(_Alias(pd, (H, W), "<f4"), device="cuda").clone(),
                              torch.as_tensor(_Alias(pt, (H, W), "<i4"), device="cuda").clone()))
        torch.cuda.synchronize()
        assert len(ptrs) == 2                         # two target sets
        for i, (c, d, t) in enumerate(taken):
            _same_images(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), d.cpu().numpy(), t.cpu().numpy().view(np.uint32),
                         plan[i][2], f"frame {i} (scene {plan[i][0]}, clear {plan[i][1]!r})")
    finally:
        r.close()


@pytest.mark.parametrize("variant", cs.VARIANTS)
def test_bound_targets_in_flight_with_a_clear_depth_per_frame(oracle, variant):
    """The same with three caller-bound target sets in rotation (option bound_targets_in_flight): the deferred clear of a set
    bound earlier carries its own frame's depth.  203 x 121: rows of a bound set that are not 16-byte aligned."""
    import torch
    import f_renderer_amd as fr
    W, H = cs.SIZES[1]
    plan = _flight_plan(oracle, W, H, variant)
    vs, ps = cs.shaders(fr, variant)
    r = _renderer(W, H, {"bound_targets_in_flight": 1})
    try:
        r.set_count_fragments(False)
        meshes = [r.upload_mesh(cs.mesh(variant, k), vs) for k in (0, 1)]
        sets = [tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32)) for _ in range(3)]
        st = torch.cuda.Stream()
        taken = []
        for i, (which, clear, _) in enumerate(plan):
            c_, d_, t_ = sets[i % 3]
            r.frame_wait(st.cuda_stream)              # the copies that still read this set (three frames back) come first
            r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
            r.clear(cs.RGBA, clear)
            r.draw(meshes[which], ps)
            r.frame_fence(st.cuda_stream)
            with torch.cuda.stream(st):
                taken.append((c_.clone(), d_.clone(), t_.clone()))
        torch.cuda.synchronize()
        for i, (c, d, t) in enumerate(taken):
            _same_images(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), d.cpu().numpy(), t.cpu().numpy().view(np.uint32),
                         plan[i][2], f"frame {i} (scene {plan[i][0]}, clear {plan[i][1]!r})")
    finally:
        r.close()


# ---- i: a pending clear overridden by a second one ---------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["default", "sweep"])
def test_second_clear_before_the_draw_holds(oracle, path):
    """clear(a); clear(b); draw: the frame starts from b -- fused into the tile kernel, or settled by k_clear (raster_sweep)."""
    import f_renderer_amd as fr
    cd = cs.clear_depths(oracle, W0, H0)
    other = (1, 2, 3, 4)
    r = _renderer(W0, H0, PATHS[path] if path != "default" else {})
    try:
        r.set_count_fragments(False)
        m = r.upload_mesh(cs.scene(), fr.VS_CLIP)
        for first, second in (("pos_inf", "mid"), ("mid", "pos_inf"), ("nan", "neg_mid"), ("neg_mid", "nan")):
            r.clear(other, cd[first])
            r.clear(cs.RGBA, cd[second])
            r.draw(m, fr.PS_DEPTH)
            _same(r, cs.oracle_frame(oracle, W0, H0, cd[second], "depth"), False, f"{path}: {first} then {second}")
    finally:
        r.close()


# ---- j: a user shader ---------------------------------------------------------------------------------------------------------

def test_user_shader_over_a_clear_depth(oracle):
    """The run-time compiled tile kernel of a user shader pair (the built-in VS_CLIP_COLOR / PS_COLOR restated)."""
    cd = cs.clear_depths(oracle, W0, H0)
    r = _renderer(W0, H0)
    try:
        sid = r.register_shader(user_shaders.VERTEX_COLOR, 7, 3)
        m = r.upload_mesh(cs.scene_color(), sid)
        for cls in ("mid", "pos_inf"):
            f = cs.oracle_frame(oracle, W0, H0, cd[cls], "color")
            for count in (True, False):
                r.set_count_fragments(count)
                r.clear(cs.RGBA, cd[cls])
                r.draw(m, sid)
                _same(r, f, count, f"user shader, {cls} count={count}")
    finally:
        r.close()
