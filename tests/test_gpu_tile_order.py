"""Option tile_order (which workgroup of the tile kernel takes which tile: 0 fixed, 1 heaviest first by the records of
an earlier pass, 2 a seeded random permutation).  Tiles are independent, so the order must not change a bit of any
result: colour, depth, triangle ids and the counters are compared across the three orders -- on the golden configs
(against the committed digests too), on partitioned ranks, across a replay after a list overflow, and with two frames in
flight whose mesh changes between frames (the recorded costs are then stale)."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_frames", os.path.join(HERE, "golden", "make_frames.py"))
make_frames = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_frames)
with open(os.path.join(HERE, "golden", "frames.json")) as _fh:
    GOLDEN = json.load(_fh)

ORDERS = (0, 1, 2)
FRAMES = 4   # two frames in flight alternate between two workspace sets: passes 3 and 4 order by what passes 1 and 2 recorded


def _renderer(cfg, order):
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    r = fr.Renderer(cfg["W"], cfg["H"])
    r.set_option("tile_order", order)
    kw = {}
    if cfg["cam"]:
        eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(cfg["W"], cfg["H"])
        kw = dict(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye)
    if cfg["tex"] is not None:
        r.set_texture(0, cfg["tex"])
        kw["texture_slot"] = 0
    r.set_uniforms(flat_color=cfg["flat_color"], **kw)
    return r


def _frames(r, m, ps, n=FRAMES):
    for _ in range(n):
        r.clear()
        r.draw(m, ps)
    c, d, t = r.readback()
    return c.copy(), d.view(np.uint32).copy(), t.copy(), r.stats()


def _assert_same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    assert a[3] == b[3]


@pytest.mark.parametrize("name,size", [("cfg1", "reduced"), ("cfg2", "reduced"), ("cfg3", "reduced"), ("cfg3b", "reduced"),
                                       ("cfg4", "reduced"), ("cfg5", "reduced"), ("headline", "reduced"), ("headline", "full")])
def test_golden_configs_do_not_depend_on_the_tile_order(name, size):
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    cfg = scenes.build_config(name, reduced=size == "reduced")
    g = GOLDEN[name][size]
    vs, ps = getattr(fr, "VS_" + cfg["vs"]), getattr(fr, "PS_" + cfg["ps"])
    got = {}
    for order in ORDERS:
        r = _renderer(cfg, order)
        got[order] = _frames(r, r.upload_mesh(cfg["mesh"], vs), ps)
        r.close()
    c, d, t, st = got[0]
    assert make_frames.sha(d.view(np.float32)) == g["sha256_depth"] and make_frames.sha(t) == g["sha256_tri_id"]
    assert make_frames.sha(c) == g["sha256_rgba8"]
    assert st["tris_setup"] == g["tris_setup"] and st["frag_covered"] == g["frag_covered"]
    for order in ORDERS[1:]:
        _assert_same(got[order], got[0])


@pytest.mark.parametrize("blocked", [False, True])
def test_partitioned_ranks_do_not_depend_on_the_tile_order(oracle, blocked):
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    W, H, world = 400, 300, 3
    tris = scenes.random_clip_triangles(60000, W, H, seed=91, spread=1.1)
    f = oracle.Frame(W, H)
    f.clear()
    f.draw(tris, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms())
    for rank in range(world):
        got = {}
        for order in ORDERS:
            r = fr.Renderer(W, H)
            r.set_option("tile_order", order)
            r.set_partition(rank, world, blocked=blocked)
            got[order] = _frames(r, r.upload_mesh(tris, fr.VS_CLIP), fr.PS_DEPTH)
            rows = r.owned_rows((0, H))
            r.close()
        for order in ORDERS[1:]:
            _assert_same(got[order], got[0])
        _, d, t, _ = got[1]
        for y0, y1 in rows:
            np.testing.assert_array_equal(t[y0 * W:y1 * W], f.tri_id[y0 * W:y1 * W])
            np.testing.assert_array_equal(d[y0 * W:y1 * W], f.depth.view(np.uint32)[y0 * W:y1 * W])


def test_replayed_frames_do_not_depend_on_the_tile_order(oracle):
    """The (triangle, tile) lists fit the first mesh but not the second: after three frames of the first (costs recorded),
    the first attempt of the second mesh's pass overflows, and the library grows the lists and replays it (in the fixed
    order); the passes after it order their tiles again."""
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    W, H = 320, 200
    a = scenes.random_clip_triangles(4000, W, H, seed=92, spread=1.1)
    b = scenes.random_clip_triangles(40000, W, H, seed=93, spread=1.1)
    f = oracle.Frame(W, H)
    f.clear()
    f.draw(b, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms())
    got = {}
    for order in ORDERS:
        r = fr.Renderer(W, H)
        r.set_option("tile_order", order)
        r.set_option("bin_capacity", 16384)
        ma, mb = r.upload_mesh(a, fr.VS_CLIP), r.upload_mesh(b, fr.VS_CLIP)
        for _ in range(3):
            r.clear()
            r.draw(ma, fr.PS_DEPTH)
        r.clear()
        r.draw(mb, fr.PS_DEPTH)
        r.sync()
        assert r.stats()["replays"] >= 1
        got[order] = _frames(r, mb, fr.PS_DEPTH, n=3)
        r.close()
    for order in ORDERS[1:]:
        _assert_same(got[order], got[0])
    np.testing.assert_array_equal(got[1][2], f.tri_id)
    np.testing.assert_array_equal(got[1][1], f.depth.view(np.uint32))


def test_stale_costs_after_a_mesh_change_do_not_change_the_frame(oracle):
    """Two frames in flight (own targets, the default); three frames of one mesh record its costs, then the mesh changes:
    the next passes order their tiles by the old mesh's costs.  Every frame of the new mesh is the oracle's."""
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    W, H = 480, 270
    a = scenes.random_clip_triangles(50000, W, H, seed=95, spread=1.1)
    b = scenes.random_clip_triangles(30000, W, H, seed=96, spread=1.0)
    b[..., 0] *= 0.3                 # its load sits in the middle third of the columns: other tiles are heavy now
    f = oracle.Frame(W, H)
    f.clear()
    f.draw(b, oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms())
    got = {}
    for order in ORDERS:
        r = fr.Renderer(W, H)
        r.set_option("tile_order", order)
        ma, mb = r.upload_mesh(a, fr.VS_CLIP), r.upload_mesh(b, fr.VS_CLIP)
        for _ in range(3):
            r.clear()
            r.draw(ma, fr.PS_DEPTH)
        seen = []
        for _ in range(3):
            r.clear()
            r.draw(mb, fr.PS_DEPTH)
            c, d, t = r.readback()
            seen.append((c.copy(), d.view(np.uint32).copy(), t.copy(), r.stats()))
        r.close()
        got[order] = seen
        for s in seen:
            np.testing.assert_array_equal(s[2], f.tri_id)
            np.testing.assert_array_equal(s[1], f.depth.view(np.uint32))
    for order in ORDERS[1:]:
        for x, y in zip(got[order], got[0]):
            _assert_same(x, y)


def test_tile_order_option_rejects_unknown_values():
    import f_renderer_amd as fr
    r = fr.Renderer(64, 48)
    for v in (0, 1, 2):
        r.set_option("tile_order", v)
    for v in (-1, 3):
        with pytest.raises(Exception):
            r.set_option("tile_order", v)
    r.close()


def test_heavy_first_order_is_built_and_taken():
    """The parity tests above hold only if the built orders are actually taken: on the headline frame the passes after
    the first one of each workspace set take heavy first (tile_order 1) or the random order (2), never with 0; above
    4,096 tiles heavy first keeps the fixed order while the random order still goes."""
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    cfg = scenes.build_config("headline")
    passes = {}
    for order in ORDERS:
        r = _renderer(cfg, order)
        m = r.upload_mesh(cfg["mesh"], fr.VS_CLIP)
        _frames(r, m, fr.PS_DEPTH)
        passes[order] = r.tile_order_passes()
        r.close()
    assert passes[0] == 0
    assert passes[1] >= FRAMES - 2          # the first pass on each of the two workspace sets has no recorded costs
    assert passes[2] == FRAMES
    W, H = 2240, 2048                       # 70 x 64 = 4,480 tiles
    tris = scenes.random_clip_triangles(20000, W, H, seed=97, spread=1.1)
    for order, want in ((1, 0), (2, FRAMES)):
        r = fr.Renderer(W, H)
        r.set_option("tile_order", order)
        _frames(r, r.upload_mesh(tris, fr.VS_CLIP), fr.PS_DEPTH)
        assert r.tile_order_passes() == want
        r.close()
