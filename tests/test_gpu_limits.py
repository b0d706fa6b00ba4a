"""Frames at the tile-count and coordinate limits against the C oracle (scenes: tests/limit_scenes.py; their input
conditions are also checked without a GPU by tests/test_limits_oracle.py).  The bar is test_gpu_parity's: ids, depth bits,
RGBA8 and the statistics equal the oracle's, no tolerance.  Which binning path ran is asserted from the launch counts of
frr_profile_get.

  3a  large grids: 36,864 owned tiles (the LDS histogram's limit, staging area shrunk to 960 records), 37,056 (the first grid on
      the global-atomic CSR path by itself), 65,280 (magic division at its upper edge), 65,536 (plain division, window beyond
      SPAN_SAFE), the last one on a 2-rank partition (segmented, window beyond SPAN_SAFE), and frames one and two tiles wide
      with coordinates up to the i16 edge
  3b  windows far from a small frame: ending at / starting at / straddling +-8191, at +32767 and at -32768, at negative x0
      and wholly at negative y, on every raster / binning path
  3c  windows outside the accepted range stay rejected and leave the context usable
"""
import numpy as np
import pytest

from . import limit_scenes as ls
from .conftest import assert_depth_equal, owned_pixel_rows
from .test_gpu_parity import _assert_frame_equal

pytestmark = pytest.mark.gpu

CLEAR = (30, 30, 30, 255)


def _launches(r):
    return {k: r.profile_get(k)[1] for k in r.KERNELS}


def _assert_path(r, path, passes, note):
    """path "seg": k_bin_seg ran for every pass and the CSR kernels never; "csr": the reverse."""
    n = _launches(r)
    msg = f"{note}; launches {n}; stats {r.stats()}"
    if path == "seg":
        assert n["k_bin_seg"] >= passes and n["k_bin_count"] == 0 and n["k_bin_fill"] == 0, msg
    else:
        assert n["k_bin_count"] >= passes and n["k_bin_fill"] >= passes and n["k_tile_scan"] >= passes and n["k_bin_seg"] == 0, msg
    assert n["k_raster"] >= passes, msg


def _renderer(W, H, options=(), partition=None):
    import f_renderer_amd as fr
    r = fr.Renderer(W, H)
    r.set_option("frames_in_flight", 1)          # one target set: half the memory of an 8192 x 8192 context
    for k, v in dict(options).items():
        r.set_option(k, v)
    if partition:
        r.set_partition(partition[0], partition[1], blocked=partition[2])
    r.profile_enable(True)
    return r


# ---- 3a: large grids ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case_d(oracle):
    """Case D's scene and oracle frame (8192 x 8192; 805 MB), shared with case E."""
    c = ls.render_large(oracle, "D")
    yield c
    c.clear()


def _draw_large(r, c):
    import f_renderer_amd as fr
    r.clear(CLEAR, 0.0)
    r.draw(r.upload_mesh(c["depth_tris"], fr.VS_CLIP), fr.PS_DEPTH)
    r.draw(r.upload_mesh(c["color_tris"], fr.VS_CLIP_COLOR), fr.PS_COLOR)


@pytest.mark.parametrize("name", sorted(ls.LARGE))
def test_large_grid_equals_oracle(oracle, request, name):
    """One context per case, a depth-only draw and a VS_CLIP_COLOR / PS_COLOR draw into the same frame (both key kinds; the
    second pass is not fused with the clear).  The case's input conditions are asserted from the oracle first."""
    W, H, path = ls.LARGE[name]
    c = request.getfixturevalue("case_d") if name == "D" else ls.render_large(oracle, name)
    f = c["frame"]
    assert f.counters.frag_nan == 0
    got = ls.large_conditions(name, f, c["spi_depth"], c["spi_color"], c["hot"])
    r = _renderer(W, H)
    try:
        _draw_large(r, c)
        _assert_frame_equal(r, f)
        st = r.stats()
        assert st["draws"] == 2
        if name == "A":
            # >= 1,000,000 records through at most 256 chunk workgroups with 960 staged records each: the staging area
            # overflows at least fourfold on average (PutMixed's direct-to-memory branch)
            assert st["bin_entries"] >= 1_000_000, (st, got)
        _assert_path(r, path, 2, f"case {name}: replays {st['replays']}, conditions {got}")
    finally:
        r.close()


@pytest.mark.parametrize("blocked", [False, True])
def test_large_grid_case_e_partition_of_two_stitches_to_the_oracle(oracle, case_d, blocked):
    """Case D's frame on a 2-rank partition: 32,768 owned tiles, so the segmented binning with a window beyond SPAN_SAFE.
    Each rank owns one of the two hot tiles.  Stitched as in test_tile_partition_stitch, against the oracle."""
    W, H, _ = ls.LARGE["D"]
    c, f = case_d, case_d["frame"]
    oc = f.counters.as_dict()
    ls.large_conditions("D", f, c["spi_depth"], c["spi_color"], c["hot"])
    acc_t = np.full(W * H, 0xFFFFFFFF, np.uint32).reshape(H, W)
    acc_d = np.zeros(W * H, np.float32).reshape(H, W)
    acc_c = np.empty((H, W, 4), np.uint8)
    acc_c[...] = CLEAR
    covered = 0
    for rank in range(2):
        r = _renderer(W, H, partition=(rank, 2, blocked))
        try:
            _draw_large(r, c)
            col, d, t = r.readback()
            st = r.stats()
            assert st["tris_setup"] == oc["tris_setup"] and st["tris_in"] == oc["tris_in"] and st["frag_nan"] == 0, (st, oc)
            covered += st["frag_covered"]
            own = owned_pixel_rows(H, rank, 2, blocked)
            t, d = t.reshape(H, W), d.reshape(H, W)
            assert (t[~own] == 0xFFFFFFFF).all()
            acc_t[own], acc_d[own], acc_c[own] = t[own], d[own], col[own]
            _assert_path(r, "seg", 2, f"case E rank {rank} blocked {blocked}: replays {st['replays']}")
        finally:
            r.close()
        del col, d, t
    np.testing.assert_array_equal(acc_t.ravel(), f.tri_id, err_msg="stitched triangle ids differ")
    assert_depth_equal(acc_d, f.depth)
    np.testing.assert_array_equal(acc_c, f.color, err_msg="stitched RGBA8 differs")
    assert covered == oc["frag_covered"]


# ---- 3b: far windows on small frames ------------------------------------------------------------------------------------

# (the default shape of a grid of at most 256 tiles is the 16-wave one already: raster_nw = 4 is added to run another)
PATHS = {"default": {}, "sweep": {"raster_sweep": 1}, "nw16": {"raster_nw": 16}, "nw4": {"raster_nw": 4, "raster_occ": 6},
         "atomics": {"bin_atomics": 1}}
_far_cache = {}


def _far(oracle, name, variant):
    if (name, variant) not in _far_cache:
        c = ls.render_far(oracle, name, variant)
        assert c["frame"].counters.frag_nan == 0
        c["conditions"] = ls.far_conditions(name, c["frame"], c["spi"])
        _far_cache[(name, variant)] = c
    return _far_cache[(name, variant)]


def _draw_far(r, c):
    import f_renderer_amd as fr
    x0, x1, y0, y1 = c["window"]
    r.clear(CLEAR, 0.0)
    r.draw(r.upload_mesh(c["tris"], getattr(fr, "VS_" + c["vs"])), getattr(fr, "PS_" + c["ps"]), (x0, x1), (y0, y1))


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", sorted(ls.FAR_WINDOWS))
def test_far_window_equals_oracle(oracle, name, path):
    """Every far window on every path.  A window that reaches beyond +-8191 sends every triangle of the pass to the sweep
    (win_safe == 0); inside it, triangles on both sides of 8191 share the pass.

    x_negative_to_positive, the window (-200, 300) x (0, 400): the depth stride 300 is smaller than the width 500, so pixel
    (lx >= 300, ly) and pixel (lx - 300, ly + 1) share one depth entry (renderer.rs:362) and the reference runs both pixels'
    fragments through it in submission order.  Before k_raster_entries 24,826 to 31,597 of the 262,144 id entries differed
    from the oracle here, on every path."""
    c = _far(oracle, name, "depth")
    r = _renderer(c["W"], c["H"], PATHS[path])
    try:
        _draw_far(r, c)
        _assert_frame_equal(r, c["frame"])
        _assert_path(r, "csr" if path in ("sweep", "atomics") else "seg", 1, f"{name} {path}: {c['conditions']}")
    finally:
        r.close()


@pytest.mark.parametrize("variant", ["color", "fans"])
@pytest.mark.parametrize("name", sorted(ls.FAR_WINDOWS))
def test_far_window_shaded_and_clipped_fans(oracle, name, variant):
    """The same windows with vertex colours through PS_COLOR, and with the w-jittered soup whose far-plane crossings are
    clipped into fans (the setup records are compared as well)."""
    c = _far(oracle, name, variant)
    r = _renderer(c["W"], c["H"])
    try:
        _draw_far(r, c)
        _assert_frame_equal(r, c["frame"])
        g = r.setup_triangles()
        assert g.shape[0] == c["spi"].shape[0]
        np.testing.assert_array_equal(g["spi"], c["spi"])
    finally:
        r.close()


def test_far_window_reused_for_two_passes_over_one_geometry(oracle):
    """frr_geometry once, then two raster passes over the same far window (legal without a partition, renderer.rs:269-271):
    depth-only, then PS_FLAT -- every fragment of the second pass ties with the first and passes (renderer.rs:363)."""
    import f_renderer_amd as fr
    name = "xy_straddle_8191"
    c = _far(oracle, name, "depth")
    W, H, (x0, x1, y0, y1) = ls.FAR_WINDOWS[name]
    f = oracle.Frame(W, H)
    f.clear()
    for ps, flat in ((oracle.PS_DEPTH, (1, 1, 1, 1)), (oracle.PS_FLAT, (0.2, 0.4, 0.6, 1.0))):
        f.draw(c["tris"], oracle.VS_CLIP, ps, oracle.make_uniforms(flat_color=flat), window=(x0, x1, y0, y1))
    r = _renderer(W, H)
    try:
        r.clear(CLEAR, 0.0)
        n = r.geometry_processing(r.upload_mesh(c["tris"], fr.VS_CLIP), count=True)
        assert n == c["spi"].shape[0]
        r.rasterization((x0, x1), (y0, y1), fr.PS_DEPTH)
        r.set_uniforms(flat_color=(0.2, 0.4, 0.6, 1.0))
        r.rasterization((x0, x1), (y0, y1), fr.PS_FLAT)
        _assert_frame_equal(r, f, stats=False)
        st = r.stats()
        assert st["tris_setup"] == n and st["frag_covered"] == f.counters.frag_covered and st["frag_nan"] == 0, st
        _assert_path(r, "seg", 2, name)
    finally:
        r.close()


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["xy_straddle_8191", "y_start_minus_32768", "y_negative_near", "x_end_32767"])
def test_far_window_partitioned_stitches_to_the_oracle(oracle, name, world, blocked):
    """A partitioned far window: the ranks own WINDOW-LOCAL tile rows (frr_owned_rows), whatever y0 is."""
    c = _far(oracle, name, "depth")
    f, oc = c["frame"], c["frame"].counters.as_dict()
    W, H, (x0, x1, y0, y1) = ls.FAR_WINDOWS[name]
    assert x1 >= x1 - x0                      # (no two window rows share a depth index: the ranks' parts are disjoint)
    index = ls.window_depth_index(c["window"])
    acc_t = np.full(W * H, 0xFFFFFFFF, np.uint32)
    acc_d = np.zeros(W * H, np.float32)
    covered = 0
    for rank in range(world):
        r = _renderer(W, H, partition=(rank, world, blocked))
        try:
            _draw_far(r, c)
            _, d, t = r.readback()
            st = r.stats()
            assert st["tris_setup"] == oc["tris_setup"], (st, oc)
            covered += st["frag_covered"]
            own = owned_pixel_rows(y1 - y0, rank, world, blocked)
            bands = r.owned_rows((y0, y1))
            rows = np.zeros(y1 - y0, bool)
            for a, b in bands:
                rows[a:b] = True
            np.testing.assert_array_equal(rows, own, err_msg="frr_owned_rows differs from the partition rule")
            mine = np.zeros(W * H, bool)
            mine[index[own].ravel()] = True
            assert (t[~mine] == 0xFFFFFFFF).all()
            acc_t[mine], acc_d[mine] = t[mine], d[mine]
        finally:
            r.close()
    np.testing.assert_array_equal(acc_t, f.tri_id)
    assert_depth_equal(acc_d, f.depth)
    assert covered == oc["frag_covered"]


# ---- 3c: rejections stay rejections --------------------------------------------------------------------------------------

def test_windows_outside_the_accepted_range_stay_rejected(oracle):
    """x1 = 32768 and y0 = -32769: FRR_ERR_UNSUPPORTED; a window larger than the FrameBuffer and one whose depth index would
    leave the buffer: FRR_ERR_INVALID (the reference panics there).  The context stays usable: a valid far-window draw
    after each of them still matches the oracle."""
    import f_renderer_amd as fr
    c = _far(oracle, "y_straddle_8191", "depth")
    W, H = c["W"], c["H"]
    assert (W, H) == (512, 512)
    r = _renderer(W, H)
    try:
        m = r.upload_mesh(c["tris"], fr.VS_CLIP)
        r.clear(CLEAR, 0.0)
        for wr, hr, code in (((32768 - 100, 32768), (0, 100), fr.FRR_ERR_UNSUPPORTED),
                             ((0, 100), (-32769, -32700), fr.FRR_ERR_UNSUPPORTED),
                             ((0, W + 1), (0, 10), fr.FRR_ERR_INVALID),
                             ((0, 10), (8000, 8000 + H + 1), fr.FRR_ERR_INVALID),
                             ((8000, 8400), (0, 400), fr.FRR_ERR_INVALID)):      # (399 * 8400 + 400 > 512 * 512)
            with pytest.raises(fr.FrrError) as e:
                r.draw(m, fr.PS_DEPTH, wr, hr)
            assert e.value.code == code, (wr, hr, str(e.value))
            x0, x1, y0, y1 = c["window"]
            r.clear(CLEAR, 0.0)
            r.draw(m, fr.PS_DEPTH, (x0, x1), (y0, y1))
            _assert_frame_equal(r, c["frame"])
    finally:
        r.close()
