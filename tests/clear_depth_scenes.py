"""Scenes and clear-depth classes for the tests of draws over a clear depth other than 0.0 (test_clear_depth_oracle.py on
the CPU, test_gpu_clear_depth.py on the GPU), and the input conditions both files assert on them.  No tests in here.

frr_clear's depth is the value every `rhw < depth` test of the frame starts from (phong.rs:317, renderer.rs:363).  In the
library it is the initial pixel key of a fused-clear draw, the start of the hierarchical-z tables, what both resolves write
where nobody won, and per-frame state that travels with frames in flight and with replays.  The scene below has what it
takes to tell a wrong bit in any of them: fragments of positive and of NEGATIVE rhw (the reference's clipper keeps the
original vertices, renderer.rs:171, so a triangle with negative w is rasterized), fans of NaN-depth fragments, and one tile
with more records than the tile kernel culls from registers.  The classes are computed from the oracle's frames, so they
follow the scene; everything that is counted is counted from the oracle alone.
"""
import numpy as np

from . import limit_scenes as ls

SIZES = ((200, 120), (203, 121))       # partial tiles right and bottom / odd stride: the depth-only resolve's scalar stores
RGBA = (9, 8, 7, 6)
DIRECT_MAX = 256                       # frr_raster.h: records of a tile that are culled straight from registers
HOT = (80.0, 48.0)                     # centre of tile (2, 1): where the cluster sits
CLASSES = ("mid", "neg_mid", "neg_zero", "neg_inf", "pos_inf", "flt_max", "neg_flt_max", "sub_pos", "sub_neg", "nan")
PATH_CLASSES = ("mid", "neg_mid", "pos_inf", "nan")      # the classes the alternative paths run
VARIANTS = ("depth", "color")          # VS_CLIP / PS_DEPTH (depth4 resolve, emission keys); VS_CLIP_COLOR / PS_COLOR (order keys)
NEG_WINDOW = (-60, 120, 0, 100)        # x0 < 0 on a 200 x 120 frame: stride 120 < width 180, rows share depth entries
SUB_WINDOW = (0, 160, 0, 100)          # x0 = y0 = 0, smaller than the frame

_FLT_MAX = np.float32(3.4028234663852886e38)
_cache = {}


# ---- the scene ------------------------------------------------------------------------------------------------------------

def scene(which=0):
    """VS_CLIP [n,3,4].  which = 0: the base scene; 1: a second one of the same make (frames in flight alternate the two).
    Positions are clip space, so one scene serves both frame sizes."""
    key = ("scene", which)
    if key not in _cache:
        from f_renderer_amd import scenes
        W, H = SIZES[0]
        tris = scenes.random_clip_triangles(1500, W, H, seed=11 + 12 * which, spread=1.05, w_jitter=0.1)
        tris[1::3] *= -1                      # the NDC position stays, rhw becomes negative, nothing is clipped away
        tris[::250, 1, 0] = 3e38              # screen positions that overflow: fans of NaN-depth fragments
        # a cluster of small triangles inside one tile: more than DIRECT_MAX records there.  Every triangle at a w of its
        # own in [1, 10) (the soup's range), every fourth one negative
        rng = np.random.default_rng(500 + which)
        n = 340
        c = np.asarray(HOT) + (2.0 * rng.random((n, 2)) - 1.0) * 3.0
        v = c[:, None, :] + (2.0 * rng.random((n, 3, 2)) - 1.0) * (3.0 + 6.0 * rng.random(n))[:, None, None]
        w = 1.0 + 9.0 * rng.random(n)
        w[::4] *= -1.0
        cl = ls.clip_from_pixels(v[..., 0], v[..., 1], W, H, w=np.repeat(w[:, None], 3, axis=1))
        out = np.concatenate([tris, cl], axis=0).astype(np.float32)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def scene_color(which=0):
    """The same positions as VS_CLIP_COLOR [n,3,7] (seeded colours)."""
    key = ("color", which)
    if key not in _cache:
        out = ls.with_colors(scene(which), 71 + which)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def scene_shifted(which=0):
    """The scene moved 60 pixels to the left (of a 200-pixel viewport): what NEG_WINDOW looks at."""
    t = np.array(scene(which))
    t[..., 0] -= np.float32(0.6) * t[..., 3]
    return t


def mesh(variant, which=0):
    return scene(which) if variant == "depth" else scene_color(which)


def shaders(mod, variant):
    """(vs, ps) ids of `variant` in `mod` (the oracle's binding or the library's package)."""
    return (mod.VS_CLIP, mod.PS_DEPTH) if variant == "depth" else (mod.VS_CLIP_COLOR, mod.PS_COLOR)


# ---- the oracle's frames ---------------------------------------------------------------------------------------------------

def bits(depth):
    return int(np.array([depth], np.float32).view(np.uint32)[0])


def oracle_frame(oracle, W, H, depth, variant="depth", which=0, window=None, tris=None, rgba=RGBA):
    """The C oracle's Frame of the scene drawn over clear(rgba, depth).  Cached (keyed by the clear depth's bits): treat it
    as read-only.  tris: another mesh of the variant's layout (not cached)."""
    key = ("frame", W, H, bits(depth), variant, which, window, tuple(rgba))
    if tris is None and key in _cache:
        return _cache[key]
    f = oracle.Frame(W, H)
    f.clear(rgba, depth)
    vs, ps = shaders(oracle, variant)
    f.draw(mesh(variant, which) if tris is None else tris, vs, ps, oracle.make_uniforms(), window=window)
    if tris is None:
        _cache[key] = f
    return f


def clear_depths(oracle, W, H):
    """name -> f32 clear depth of every class, for the W x H frame of the base scene."""
    key = ("classes", W, H)
    if key not in _cache:
        d0 = oracle_frame(oracle, W, H, 0.0).depth
        pos = np.sort(d0[np.isfinite(d0) & (d0 > 0)])
        dn = oracle_frame(oracle, W, H, -np.inf).depth
        with np.errstate(invalid="ignore"):
            neg = np.sort(dn[np.isfinite(dn) & (dn < 0)])
        assert pos.size and neg.size
        _cache[key] = {
            "mid": np.float32(pos[pos.size // 2]),            # an actual pixel's value, bit for bit: a fragment ties with it
            "neg_mid": np.float32(neg[neg.size // 2]),
            "neg_zero": np.float32(-0.0), "neg_inf": np.float32(-np.inf), "pos_inf": np.float32(np.inf),
            "flt_max": _FLT_MAX, "neg_flt_max": -_FLT_MAX,
            "sub_pos": np.float32(1e-40), "sub_neg": np.float32(-1e-40),
            "nan": np.float32(np.nan),
        }
    return _cache[key]


def hot_tile_records(oracle, W, H, which=0):
    """The largest (triangle, tile) record count of a tile, from the oracle's setup list."""
    spi = ls.setup_spi(oracle, W, H, scene(which))
    return int(ls.records_per_tile(spi, (0, W, 0, H)).max())


# ---- what the oracle's frames say about the classes ------------------------------------------------------------------------

NOBODY = 0xFFFFFFFF


def conditions(oracle, W, H):
    """The input conditions of every class, asserted from the C oracle alone; returns the figures (for messages)."""
    cd = clear_depths(oracle, W, H)
    fr = {k: oracle_frame(oracle, W, H, v) for k, v in cd.items()}
    f0 = oracle_frame(oracle, W, H, 0.0)
    won0 = f0.tri_id != NOBODY
    out = {"covered_at_0": int(won0.sum())}
    with np.errstate(invalid="ignore"):
        for k, f in fr.items():
            won = f.tri_id != NOBODY
            d = f.depth
            out[k] = dict(won=int(won.sum()), nan=int(np.isnan(d[won]).sum()), negative=int((d[won] < 0).sum()),
                          ties=int((won & (d.view(np.uint32) == bits(cd[k]))).sum()),
                          lost=int((won0 & ~won).sum()), kept=int((won0 & won).sum()), gained=int((won & ~won0).sum()))
            assert f.counters.frag_nan > 0, (k, out)
            # where nobody won the clear value stays, bit for bit (a NaN stays a NaN)
            rest = d[~won]
            assert rest.size, (k, out)
            assert np.isnan(rest).all() if k == "nan" else (rest.view(np.uint32) == bits(cd[k])).all(), (k, out)
    q = out["covered_at_0"] // 4
    m = out["mid"]
    assert m["ties"] >= 1 and m["lost"] >= q and m["kept"] >= q, out
    m = out["neg_mid"]
    assert m["ties"] >= 1 and m["gained"] > 0 and m["negative"] > 0, out
    # -inf rejects nothing, and neither does a NaN (`rhw < NaN` is false): every pixel a non-dropped fragment covers is won
    np.testing.assert_array_equal(fr["neg_inf"].tri_id != NOBODY, fr["nan"].tri_id != NOBODY)
    for k in ("neg_inf", "nan"):
        assert out[k]["won"] > out["covered_at_0"] and out[k]["negative"] > 0 and out[k]["lost"] == 0, out
    for k in ("pos_inf", "flt_max"):
        m = out[k]
        assert m["won"] > 0 and m["nan"] > 0 and m["won"] > m["nan"] and m["negative"] > 0, out
    assert np.signbit(fr["neg_zero"].depth[fr["neg_zero"].tri_id == NOBODY]).all(), out
    out["hot_tile_records"] = hot_tile_records(oracle, W, H)
    assert out["hot_tile_records"] > DIRECT_MAX, out
    return out
