"""The tile kernel's early exit from the cull loop (frr_raster.h: span_order_bins2, step 1 of k_raster_span) must not
change any output: a heavy tile stops fetching cull records at the first step from which on every record's depth bound
lies below the smallest depth in the tile.  Depth bits, ids and RGBA8 are compared with the C oracle, no tolerance.

Every scene is a 64 x 64 frame whose tile (0, 0) holds a few hundred records (more than the 256 a tile culls straight from
registers, so they go through the near-first copy in >= 10 steps): two near triangles (rhw = 1 and 1.25) that cover the
tile, submitted first, then small far ones (rhw in [0.1, 0.5]) -- after the first steps everything left is behind the tile.
(The reference's clipper turns a triangle that straddles a frustum plane into a fan: the near pair lies inside the
viewport, a few of the far ones cross its left or upper edge and arrive as fans.)  Fragment counting is off unless a case says otherwise (the counted frame culls
nothing and never exits early)."""
import numpy as np
import pytest

from .conftest import assert_depth_equal
from .limit_scenes import clip_from_pixels

pytestmark = pytest.mark.gpu

W = H = 64
CLEAR = (30, 30, 30, 255)
N_FAR = 350


def _near(y_off=0.0):
    """[2, 3, 4]: two triangles, rhw = 1 and 1.25, that each cover all of tile (0, 0) (x + y < 64: half the viewport)."""
    px = np.array([[0.0, 64.0, 0.0], [0.0, 64.0, 0.0]])
    py = np.array([[0.0, 0.0, 64.0], [0.0, 0.0, 64.0]]) + y_off
    return clip_from_pixels(px, py, W, H, w=np.array([[1.0], [0.8]]))


def _far(n, seed, y_off=0.0, x_lo=2.0, x_hi=30.0):
    """[n, 3, 4]: small triangles, 2 .. 9 pixels across, centred at x in [x_lo, x_hi), y in [2, 30) -- by default inside
    tile (0, 0); w in [2, 10] per triangle (+- 5 % per vertex)."""
    rng = np.random.default_rng(seed)
    c = np.array([x_lo, 2.0]) + np.array([x_hi - x_lo, 28.0]) * rng.random((n, 1, 2))
    v = c + (2.0 * rng.random((n, 3, 2)) - 1.0) * (1.0 + 3.5 * rng.random((n, 1, 1)))
    w = (2.0 + 8.0 * rng.random((n, 1))) * (1.0 + 0.05 * (2.0 * rng.random((n, 3)) - 1.0))
    return clip_from_pixels(v[..., 0], v[..., 1] + y_off, W, H, w=w)


def _elsewhere(seed, y_off=0.0):
    """[12, 3, 4]: a few triangles over the other three tiles (light tiles beside the heavy one)."""
    rng = np.random.default_rng(seed)
    c = np.array([[48.0, 16.0], [16.0, 48.0], [48.0, 48.0]])[rng.integers(0, 3, 12)][:, None, :]
    v = c + (2.0 * rng.random((12, 3, 2)) - 1.0) * 12.0
    return clip_from_pixels(v[..., 0], v[..., 1] + y_off, W, H, w=1.0 + 3.0 * rng.random((12, 1)))


def _base(n_far=N_FAR, seed=11, y_off=0.0):
    return np.concatenate([_near(y_off), _far(n_far, seed, y_off), _elsewhere(seed + 1, y_off)], axis=0)


_base_cache = {}


def _base_frame(oracle):
    """The base scene and the oracle's frame of it (computed once, never written to)."""
    if "f" not in _base_cache:
        tris = _base()
        f = oracle.Frame(W, H)
        f.clear(CLEAR, 0.0)
        f.draw(tris, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms())
        # the scene does what the docstring says: the near pair owns every pixel of tile (0, 0), all far ones are hidden
        assert set(np.unique(f.tri_id.reshape(H, W)[:32, :32]).tolist()) <= {0, 1}
        _base_cache["tris"], _base_cache["f"] = tris, f
    return _base_cache["tris"], _base_cache["f"]


def _renderer(options=(), counting=False):
    """(Four waves per tile unless a case names a shape: the default for a grid of four tiles is the 16-wave shape, whose
    waves fetch the first 16 steps before any fragment lands -- there the exit rarely fires.)"""
    import f_renderer_amd as fr
    r = fr.Renderer(W, H)
    for k, v in {"raster_nw": 4, **dict(options)}.items():
        r.set_option(k, v)
    r.set_count_fragments(counting)
    return r


def _assert_equal(r, f, nan_ok=False):
    c, d, t = r.readback()
    np.testing.assert_array_equal(t, f.tri_id, err_msg="triangle-id buffer differs")
    if nan_ok:   # (which quiet-NaN pattern 0 * inf gives is the machine's, conftest.assert_depth_equal)
        assert_depth_equal(d, f.depth)
    else:
        np.testing.assert_array_equal(d.view(np.uint32), f.depth.view(np.uint32), err_msg="depth bits differ")
    np.testing.assert_array_equal(c, f.color, err_msg="RGBA8 differs")
    s = r.stats()
    assert s["tris_setup"] == f.counters.tris_setup and s["frag_nan"] == f.counters.frag_nan
    return s


def _check(oracle, tris, options=(), window=None, clear_depth=0.0, nan_ok=False):
    import f_renderer_amd as fr
    f = oracle.Frame(W, H)
    f.clear(CLEAR, clear_depth)
    f.draw(tris, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms(), window=window)
    r = _renderer(options)
    try:
        r.clear(CLEAR, clear_depth)
        if window is None:
            r.draw(r.upload_mesh(tris, fr.VS_CLIP), fr.PS_DEPTH)
        else:
            r.draw(r.upload_mesh(tris, fr.VS_CLIP), fr.PS_DEPTH, window[:2], window[2:])
        _assert_equal(r, f, nan_ok)
    finally:
        r.close()
    return f


@pytest.mark.parametrize("nw", [3, 4, 8, 16])
def test_base_scene_every_shape(oracle, nw):
    """Case 1: the tile kernel's shapes by name; at 16 waves a wave stages 16 triangles, so a cull step is 16 records."""
    import f_renderer_amd as fr
    tris, f = _base_frame(oracle)
    r = _renderer({"raster_nw": nw})
    try:
        r.clear(CLEAR, 0.0)
        r.draw(r.upload_mesh(tris, fr.VS_CLIP), fr.PS_DEPTH)
        _assert_equal(r, f)
    finally:
        r.close()


@pytest.mark.parametrize("vertex", [1, 2])
def test_nan_w_submitted_late(oracle, vertex):
    """Case 2: a far triangle with a NaN w at the end of the list.  Its record carries the all-ones bound, so it is never
    skipped, and the NaN pass walks all records of the tile whatever the main loop fetched."""
    tris = _base()
    nan_tri = clip_from_pixels(np.array([[4.0, 28.0, 6.0]]), np.array([[5.0, 9.0, 27.0]]), W, H, w=6.0)
    nan_tri[0, vertex, 3] = np.nan
    tris = np.concatenate([tris, nan_tri, _far(8, 99)], axis=0)
    f = _check(oracle, tris, nan_ok=True)
    assert f.counters.frag_nan > 0, "the scene has no NaN fragment"


def test_vertex_beyond_span_safe(oracle):
    """Case 3a: far triangles with a vertex beyond +-8191, submitted late, are swept, never z-culled -- and so never skipped
    (the clipper makes fans of them; the fans keep the far vertex).  One is behind the near pair, one in front of it."""
    tris = _base()
    sliver = clip_from_pixels(np.array([[3.0, 9000.0, 5.0], [2.0, 30.0, -9000.0]]), np.array([[4.0, 5000.0, 20.0], [29.0, 28.0, -7000.0]]), W, H,
                              w=np.array([[5.0], [0.5]]))
    tris = np.concatenate([tris, sliver, _far(8, 98)], axis=0)
    f = _check(oracle, tris)
    spi = oracle.Frame(W, H).draw(tris, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms(), keep_setup=True)["spi"].astype(np.int64)
    unsafe = np.abs(spi).max(axis=(1, 2)) > 8191
    in_tile = (spi[..., 0].min(1) < 32) & (spi[..., 0].max(1) > 0) & (spi[..., 1].min(1) < 32) & (spi[..., 1].max(1) > 0)
    assert (unsafe & in_tile).sum() >= 2, "no unsafe record in the heavy tile"
    shown = np.unique(f.tri_id.reshape(H, W)[:32, :32])
    assert np.isin(np.nonzero(unsafe)[0], shown).any(), "no unsafe triangle owns a pixel of the heavy tile"


def test_window_beyond_span_safe(oracle):
    """Case 3b: the same scene 8,200 rows further down, drawn through the window that holds it: a window beyond +-8191
    sends every triangle to the sweep (win_safe == 0) and the exit is off altogether."""
    y_off = 8200.0
    tris = _base(y_off=y_off)
    f = _check(oracle, tris, window=(0, W, 8200, 8200 + H))
    assert (f.tri_id != 0xFFFFFFFF).sum() > 1024


def test_second_draw_without_clear(oracle):
    """Case 4: the scene drawn twice with no clear in between: the second pass starts from the depth buffer, its minima
    from zero and `dirty`; every fragment of the near pair ties with what is there and passes (the later id wins)."""
    import f_renderer_amd as fr
    tris, _ = _base_frame(oracle)
    f = oracle.Frame(W, H)
    f.clear(CLEAR, 0.0)
    u = oracle.make_uniforms()
    f.draw(tris, oracle.VS_CLIP, oracle.PS_DEPTH, u)
    f.draw(tris, oracle.VS_CLIP, oracle.PS_DEPTH, u, tri_id_base=int(f.counters.tris_setup))
    r = _renderer()
    try:
        m = r.upload_mesh(tris, fr.VS_CLIP)
        r.clear(CLEAR, 0.0)
        r.draw(m, fr.PS_DEPTH)
        r.draw(m, fr.PS_DEPTH)
        _assert_equal(r, f)
    finally:
        r.close()
    assert f.tri_id.reshape(H, W)[:32, :32].min() >= len(tris)


@pytest.mark.parametrize("clear_depth", [0.3, 2.0, -1.0])
def test_clear_depth_other_than_zero(oracle, clear_depth):
    """Case 5: clears to 0.3 (hides some of the far triangles by itself), to 2.0 (nearer than everything: the exit may fire
    at the first fetch, nothing is drawn) and to -1.0."""
    tris, _ = _base_frame(oracle)
    f = _check(oracle, tris, clear_depth=clear_depth)
    if clear_depth == 2.0:
        assert (f.tri_id == 0xFFFFFFFF).all()


def test_counted_frame_never_exits(oracle):
    """Case 6: with fragment counting on, every record's coverage is counted: the counters equal the oracle's and the image
    is the one of the uncounted frame."""
    import f_renderer_amd as fr
    tris, f = _base_frame(oracle)
    r = _renderer(counting=True)
    try:
        r.clear(CLEAR, 0.0)
        r.draw(r.upload_mesh(tris, fr.VS_CLIP), fr.PS_DEPTH)
        s = _assert_equal(r, f)
        assert s["frag_covered"] == f.counters.frag_covered and s["tris_in"] == f.counters.tris_in
    finally:
        r.close()


def test_partial_tiles(oracle):
    """Case 7: a 40 x 40 window: tile (0, 0) is whole, the other three are partial (their pixels beyond the window hold
    all-ones keys: there the exit may simply never fire)."""
    tris, _ = _base_frame(oracle)
    heavy_edge = _far(400, 21, x_lo=31.0, x_hi=39.0)   # 400 more around x = 35: tile (1, 0), eight pixels wide, is heavy too
    near_edge = clip_from_pixels(np.array([[24.0, 64.0, 64.0], [24.0, 64.0, 24.0]]), np.array([[0.0, 0.0, 40.0], [0.0, 40.0, 40.0]]), W, H, w=1.0)
    _check(oracle, np.concatenate([tris[:2], near_edge, tris[2:], heavy_edge], axis=0), window=(0, 40, 0, 40))


@pytest.mark.parametrize("late_near", [False, True])
def test_lumped_last_group(oracle, late_near):
    """Case 8: about 2,500 records, 79 steps of 32: steps from 63 on share the last suffix entry.  late_near: one small
    triangle at rhw = 2 -- nearer than the near pair, but its key's bucket (exponent bits 0000) sorts it LAST, into the
    lumped group: the suffix maxima are taken over the real keys, so no step before it may end the loop."""
    parts = [_near(), _far(2500, 31), _elsewhere(32)]
    if late_near:
        parts.append(clip_from_pixels(np.array([[10.0, 22.0, 12.0]]), np.array([[9.0, 12.0, 24.0]]), W, H, w=0.5))
    tris = np.concatenate(parts, axis=0)
    f = _check(oracle, tris)
    if late_near:
        assert (f.tri_id == f.counters.tris_setup - 1).sum() > 30, "the late near triangle owns no pixels"   # (submitted last)


def test_shaded_flat(oracle):
    """Case 9: the base scene through PS_FLAT (the shaded resolve; pixel keys carry order keys, not emission indices)."""
    import f_renderer_amd as fr
    tris, _ = _base_frame(oracle)
    f = oracle.Frame(W, H)
    f.clear(CLEAR, 0.0)
    f.draw(tris, oracle.VS_CLIP, oracle.PS_FLAT, oracle.make_uniforms())
    r = _renderer()
    try:
        r.clear(CLEAR, 0.0)
        r.draw(r.upload_mesh(tris, fr.VS_CLIP), fr.PS_FLAT)
        _assert_equal(r, f)
    finally:
        r.close()
