"""The scenes of the limits tests (tests/limit_scenes.py) on the CPU: the two oracles agree on windows far from the origin,
the partition rule and the exchange plan hold for windows that do not start at row 0, and every scene test_gpu_limits.py
renders meets its input conditions for the oracle alone -- which is what makes the GPU tests test what they say."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_np as onp
from . import arg_rules
from . import limit_scenes as ls


@pytest.mark.parametrize("name", sorted(ls.FAR_WINDOWS))
def test_c_and_numpy_oracles_agree_on_far_windows(oracle, name):
    """C oracle == NumPy oracle, bit for bit, on every far window: ids, depth bits, colour and the coverage count, with
    vertices on +-8190..8193 and on the i16 edge, and slivers whose i32 edge functions wrap (renderer.rs:329-331)."""
    c = ls.render_far(oracle, name, "color", n_soup=300)
    f, W, H = c["frame"], c["W"], c["H"]
    assert f.counters.frag_nan == 0
    color = np.zeros((H, W, 4), np.uint8)
    color[...] = (30, 30, 30, 255)
    depth, tid = np.zeros(W * H, np.float32), np.full(W * H, 0xFFFFFFFF, np.uint32)
    setup_np, cov = onp.draw(W, H, c["tris"], onp.VS_CLIP_COLOR, onp.PS_COLOR, onp.Uniforms(), color, depth, tid, window=c["window"])
    assert len(setup_np) == c["spi"].shape[0]
    np.testing.assert_array_equal(np.array([[v["spi"] for v in t] for t in setup_np], np.int32), c["spi"])
    assert cov == f.counters.frag_covered and cov > 0
    np.testing.assert_array_equal(tid, f.tri_id)
    np.testing.assert_array_equal(depth.view(np.uint32), f.depth.view(np.uint32))
    np.testing.assert_array_equal(color, f.color)


def _bands(L, y0, y1, rank, world, blocked):
    a, b = C.c_int32(), C.c_int32()
    n = L.frr_partition_rows(y0, y1, rank, world, blocked, 0, C.byref(a), C.byref(b))
    assert n >= 0
    out = []
    for k in range(n):
        assert L.frr_partition_rows(y0, y1, rank, world, blocked, k, C.byref(a), C.byref(b)) == n
        out.append((a.value, b.value))
    return out


@pytest.mark.parametrize("y0", [-32768, -8200, -1, 0, 1, 8191, 32000])
def test_partition_rule_and_exchange_plan_at_far_and_negative_windows(y0):
    """frr_partition_rows == multigpu.tile_row_owner applied to WINDOW-LOCAL rows wherever the window starts, and
    frr_exchange_plan tiles the window's plane exactly once with offsets relative to the window's first row (they index a
    plane whose row 0 is the window's row y0: the render target's and the final image's local addressing, renderer.rs:323)."""
    import f_renderer_amd as fr
    from f_renderer_amd import _native as N
    from f_renderer_amd.multigpu import tile_row_owner
    L = fr.lib()
    SEND, RECV, COPY = 0, 1, 2
    row_elems = 37
    for wh in (1, 33, 300, 767):
        y1 = y0 + wh
        if y1 > 32767:
            continue
        tiles_y = (wh + 31) // 32
        for world in (1, 2, 3, 5, 8):
            for blocked in (0, 1):
                owner = np.asarray(tile_row_owner(tiles_y, world, bool(blocked)))[np.arange(wh) // 32]
                got = np.full(wh, -1)
                for rank in range(world):
                    for a, b in _bands(L, y0, y1, rank, world, blocked):
                        assert 0 <= a < b <= wh and (got[a:b] == -1).all()
                        got[a:b] = rank
                np.testing.assert_array_equal(got, owner, err_msg=f"y0={y0} wh={wh} world={world} blocked={blocked}")
                assert [_bands(L, y0, y1, r, world, blocked) for r in range(world)] == \
                       [_bands(L, 0, wh, r, world, blocked) for r in range(world)]          # a function of the height alone

                def plan(rank, root):
                    ops = (N.Xfer * 64)()
                    n = L.frr_exchange_plan(y0, y1, row_elems, rank, world, blocked, root, ops, 64)
                    assert 0 <= n <= 64
                    return [(ops[i].kind, ops[i].peer, int(ops[i].offset), int(ops[i].count)) for i in range(n)]

                for root in {0, world - 1}:
                    rootp = plan(root, root)
                    covered = np.zeros(wh * row_elems, np.uint8)
                    for kind, peer, off, cnt in rootp:
                        assert kind in (RECV, COPY) and (peer == root) == (kind == COPY)
                        assert off + cnt <= covered.size, "an offset leaves the window's plane: not window-relative"
                        covered[off:off + cnt] += 1
                        rows = owner[off // row_elems:(off + cnt) // row_elems]
                        assert off % row_elems == 0 and cnt % row_elems == 0 and (rows == peer).all()
                    assert covered.min() == 1 and covered.max() == 1
                    for r in range(world):
                        if r != root:
                            mine = plan(r, root)
                            assert all(k == SEND and p == root for k, p, _, _ in mine)
                            assert [(o, c) for _, _, o, c in mine] == [(o, c) for k, p, o, c in rootp if k == RECV and p == r]


@pytest.mark.parametrize("variant", ls.FAR_VARIANTS)
@pytest.mark.parametrize("name", sorted(ls.FAR_WINDOWS))
def test_far_window_scenes_meet_their_conditions(oracle, name, variant):
    """Section 3b's conditions for the oracle alone: at least 5,000 drawn pixels, none outside the window, and at least 20
    triangles on each side of 8191 where the window contains it; the fan variant does contain fans."""
    c = ls.render_far(oracle, name, variant)
    assert c["frame"].counters.frag_nan == 0
    got = ls.far_conditions(name, c["frame"], c["spi"])
    if variant == "fans":
        assert c["spi"].shape[0] > c["tris"].shape[0] + 100, (c["spi"].shape[0], c["tris"].shape[0], got)
    W, H, (x0, x1, y0, y1) = ls.FAR_WINDOWS[name]
    assert x1 > x0 and y1 > y0 and arg_rules.ask([arg_rules.window(arg_rules.RASTER, W, H, x0, x1, y0, y1)]) == [(arg_rules.OK, "")]   # frr_raster accepts it, and it is not empty
    for axis, (lo, hi) in enumerate(((x0, x1), (y0, y1))):
        for v in ls.BOUNDARY_VALUES:
            if lo - 3 <= v <= hi + 3:
                assert ls.hits(c["spi"], v, axis) >= 20, (name, "xy"[axis], v, got)


def test_boundary_generator_lands_on_every_value(oracle):
    """The boundary generator on a 512 x 512 viewport: every requested value, in x, in y and in both, is where at least 20
    vertices of the oracle's setup list really are (the f32 rounding of the viewport transform moves none of them)."""
    tris, spi = ls.boundary(oracle, 512, 512, ls.BOUNDARY_VALUES, ls.BOUNDARY_VALUES, (256.0, 256.0), seed=3, n_each=2)
    both = len(ls.BOUNDARY_VALUES)
    for v in ls.BOUNDARY_VALUES:
        assert ls.hits(spi, v, 0) >= 2 + 2 * both and ls.hits(spi, v, 1) >= 2 + 2 * both, v
        assert int(((spi[:, :, 0] == v) & (spi[:, :, 1] == v)).any(axis=1).sum()) >= 2, v


@pytest.mark.parametrize("name", sorted(ls.LARGE))
def test_large_grid_scenes_meet_their_conditions(oracle, name):
    """Section 3a's conditions for the oracle alone (case A with 20,000 of its 800,000 random triangles; the 1,000,000
    binning records of the full count are asserted on the GPU, from the oracle's boxes and from frr_stats).  Case E is
    case D's scene: its two hot tiles lie in tile rows 62 and 187, one for each rank of a 2-rank partition in both layouts."""
    c = ls.render_large(oracle, name, n_random=20000)
    assert c["frame"].counters.frag_nan == 0
    got = ls.large_conditions(name, c["frame"], c["spi_depth"], c["spi_color"], c["hot"], a_full=False)
    W, H, path = ls.LARGE[name]
    tiles = ((W + 31) // 32) * ((H + 31) // 32)
    assert (tiles <= ls.BIN_LDS_MAX_TILES) == (path == "seg"), got
    assert c["spi_color"].shape[0] > c["color_tris"].shape[0] + 100     # clipped fans in the colour draw
    if name == "D":
        from f_renderer_amd.multigpu import tile_row_owner
        rows = [int(h[1]) // 32 for h in c["hot"]]
        for blocked in (False, True):
            owner = tile_row_owner((H + 31) // 32, 2, blocked)
            assert sorted(owner[r] for r in rows) == [0, 1]
