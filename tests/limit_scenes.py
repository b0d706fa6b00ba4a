"""Scenes for the tests at the library's size and coordinate limits (test_limits_oracle.py on the CPU, test_gpu_limits.py
on the GPU), and the input conditions both files assert on them.  No tests in here.

Every generator is seeded (numpy default_rng) and places its triangles in SCREEN pixels: a vertex meant for pixel
(px, py) of a W x H viewport gets the clip position x = 2 px / W - 1, y = 1 - 2 py / H, z = 0.5, w = 1.  The reference's
clipper keeps the original vertices of a triangle that is not wholly inside the frustum (renderer.rs:171), so a triangle
placed thousands of pixels outside the viewport is set up and rasterized there: a raster window may lie anywhere in the
i16 range, far from a small FrameBuffer.  Where a vertex really lands is decided by the f32 rounding of
(x + 1) * W * 0.5 + 0.5, so everything that is counted -- boundary hits, boxes, records per tile -- is counted from the
ORACLE's setup list (`setup_spi`), never from the request.
"""
import numpy as np

TILE = 32
SPAN_SAFE = 8191                      # frr_raster.h: the span algebra is exact for coordinates within +-8191
BIN_LDS_MAX_TILES = 36864             # frr_kernels.h: owned tiles whose counters fit the LDS histogram
NEAR_8191 = (8190, 8191, 8192, 8193)
BOUNDARY_VALUES = NEAR_8191 + tuple(-v for v in NEAR_8191) + (32766, 32767, 32768, -32767, -32768, -32769)


# ---- generators ---------------------------------------------------------------------------------------------------

def clip_from_pixels(px, py, W, H, w=1.0, z=0.5):
    """[..., 4] f32 clip positions of screen pixels (px, py) for a W x H viewport."""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    w = np.broadcast_to(np.asarray(w, np.float64), px.shape)
    x = 2.0 * px / float(W) - 1.0
    y = 1.0 - 2.0 * py / float(H)
    return np.stack([x * w, y * w, z * w, w], axis=-1).astype(np.float32)


def pixel_soup(n, W, H, centre, extent, size, seed):
    """n triangles [n,3,4] (VS_CLIP, w = 1): centres uniform in centre +- extent, each vertex within +- s of its centre,
    s octave-uniform in [size[0], size[1])."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float64) + (2.0 * rng.random((n, 2)) - 1.0) * np.asarray(extent, np.float64)
    lo, hi = float(size[0]), float(size[1])
    s = lo * (hi / lo) ** rng.random(n)
    v = c[:, None, :] + (2.0 * rng.random((n, 3, 2)) - 1.0) * s[:, None, None]
    return clip_from_pixels(v[..., 0], v[..., 1], W, H)


def tile_grid(W, H, window, seed):
    """One triangle of ~180 px per 32 x 32 tile of `window` = (x0, x1, y0, y1), jittered about the tile's centre."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = window
    tx, ty = np.meshgrid(np.arange((x1 - x0 + TILE - 1) // TILE), np.arange((y1 - y0 + TILE - 1) // TILE), indexing="xy")
    cx = np.minimum(x0 + tx.ravel() * TILE + 16.0, x1 - 1.0)
    cy = np.minimum(y0 + ty.ravel() * TILE + 16.0, y1 - 1.0)
    c = np.stack([cx, cy], axis=1) + (2.0 * rng.random((cx.size, 2)) - 1.0) * 3.0
    shape = np.array([[-10.0, -8.0], [10.0, -6.0], [0.0, 11.0]])
    v = c[:, None, :] + shape[None] + (2.0 * rng.random((cx.size, 3, 2)) - 1.0) * 3.0
    return clip_from_pixels(v[..., 0], v[..., 1], W, H)


def cluster(n, W, H, centre, seed, radius=12.0):
    """n small triangles on one spot: one tile with far more records than its near-first slot."""
    return pixel_soup(n, W, H, centre, (radius * 0.25, radius * 0.25), (3.0, radius * 0.75), seed)


def jitter_w(tris, seed, lo=0.5, hi=2.0, cross_fraction=0.3):
    """The clipped-fan variant of a w = 1 soup: every vertex is scaled by a w of its own in [lo, hi) (the screen position
    stays, up to rounding; the depth now varies), and one vertex of `cross_fraction` of the triangles is pushed through a
    depth plane: half of them behind the near plane (z < 0), half beyond the far plane (z > w).  The reference's near-plane
    ratio is a_w / (a_w - b_w) (renderer.rs:60-73), which puts the new vertex at w ~ 0 where the epsilon test drops it, so
    it is the far-plane crossings that become fans here -- wherever on the screen the triangle lies."""
    rng = np.random.default_rng(seed)
    t = np.array(tris, np.float64)
    n = t.shape[0]
    t[..., :4] *= (lo + (hi - lo) * rng.random((n, 3)))[..., None]
    idx = np.nonzero(rng.random(n) < cross_fraction)[0]
    k = rng.integers(0, 3, n)[idx]
    amount = 0.25 * (0.2 + rng.random(idx.size))
    far = rng.random(idx.size) < 0.5
    t[idx, k, 2] = t[idx, k, 3] * np.where(far, 1.0 + amount, -amount)
    return t.astype(np.float32)


def with_colors(tris, seed):
    """VS_CLIP [n,3,4] -> VS_CLIP_COLOR [n,3,7]."""
    rng = np.random.default_rng(seed)
    return np.concatenate([tris, rng.random((tris.shape[0], 3, 3)).astype(np.float32)], axis=2)


def boundary_requests(W, H, values_x, values_y, centre, seed, n_each=32, size=(6.0, 48.0), reach=(0.0, 0.25)):
    """Triangles with ONE vertex asked onto a boundary value: for every v in values_x the vertex (v, ~centre y), for every
    v in values_y (~centre x, v), and for every pair of the two lists (vx, vy); `n_each` triangles each.  The other two
    vertices lie within `size` pixels of a point the fraction `reach` (uniform in that range) of the way towards `centre`:
    next to the boundary vertex by default, at the centre with reach = (1, 1) -- a sliver from a far boundary to there."""
    rng = np.random.default_rng(seed)
    cx, cy = float(centre[0]), float(centre[1])

    def ask(v):
        # spi = (spf + 0.5) as i32 truncates towards zero (renderer.rs:233-234): the middle of the interval that gives v
        return v + 0.25 if v >= 0 else v - 0.75

    first = []
    for v in values_x:
        first += [(ask(v), cy + d) for d in (2.0 * rng.random(n_each) - 1.0) * 60.0]
    for v in values_y:
        first += [(cx + d, ask(v)) for d in (2.0 * rng.random(n_each) - 1.0) * 60.0]
    for vx in values_x:
        for vy in values_y:
            first += [(ask(vx), ask(vy))] * n_each
    if not first:
        return np.zeros((0, 3, 4), np.float32)
    a = np.asarray(first, np.float64)
    n = a.shape[0]
    towards = a + (np.array([cx, cy]) - a) * (reach[0] + (reach[1] - reach[0]) * rng.random((n, 1)))
    lo, hi = size
    s = lo * (hi / lo) ** rng.random(n)
    others = towards[:, None, :] + (2.0 * rng.random((n, 2, 2)) - 1.0) * s[:, None, None]
    v = np.concatenate([a[:, None, :], others], axis=1)
    roll = rng.integers(0, 3, n)                       # the boundary vertex is not always vertex 0
    v = np.stack([np.roll(v[i], roll[i], axis=0) for i in range(n)]) if n else v
    return clip_from_pixels(v[..., 0], v[..., 1], W, H)


def setup_spi(oracle, W, H, tris, vs_id=None):
    """[n,3,2] i32: `spi` of the oracle's setup list for `tris` -- the list Frame.draw(..., keep_setup=True) returns
    (o_geometry_batch makes both), without rasterizing anything."""
    vs_id = oracle.VS_CLIP if vs_id is None else vs_id
    n = int(np.asarray(tris).shape[0])
    cap = n + n // 4 + 4096
    while True:
        try:
            return oracle.geometry_batch(W, H, tris, vs_id, oracle.make_uniforms(), cap=cap)["spi"].copy()
        except RuntimeError:                           # more fans than guessed
            cap *= 4


def boundary(oracle, W, H, values_x, values_y, centre, seed, n_each=32):
    """The boundary generator: (triangles, the oracle's setup spi for them)."""
    tris = boundary_requests(W, H, values_x, values_y, centre, seed, n_each)
    return tris, setup_spi(oracle, W, H, tris)


# ---- what the oracle's setup list says about a scene ---------------------------------------------------------------

def hits(spi, value, axis):
    """Setup triangles with a vertex whose `axis` (0 = x, 1 = y) component is exactly `value`."""
    return int((spi[:, :, axis] == value).any(axis=1).sum())


def clamped_boxes(spi, window):
    """(minx, maxx, miny, maxy, nonempty) per setup triangle: the i16-saturated box clamped to the window, as pack_pbox and
    tiles_of_pbox compute it (== renderer.rs:285-298 for windows within the i16 range)."""
    x0, x1, y0, y1 = window
    s = np.clip(spi.astype(np.int64), -32768, 32767)
    minx, maxx = np.clip(s[:, :, 0].min(1), x0, x1), np.clip(s[:, :, 0].max(1), x0, x1)
    miny, maxy = np.clip(s[:, :, 1].min(1), y0, y1), np.clip(s[:, :, 1].max(1), y0, y1)
    return minx, maxx, miny, maxy, (maxx > minx) & (maxy > miny)


def records_per_tile(spi, window):
    """[tiles_y, tiles_x] (triangle, tile) records of the window's 32 x 32 tiles, as tiles_of_pbox makes them."""
    x0, x1, y0, y1 = window
    tiles_x, tiles_y = (x1 - x0 + TILE - 1) // TILE, (y1 - y0 + TILE - 1) // TILE
    minx, maxx, miny, maxy, ok = clamped_boxes(spi, window)
    tx0, tx1 = (minx[ok] - x0) // TILE, (maxx[ok] - 1 - x0) // TILE + 1
    ty0, ty1 = (miny[ok] - y0) // TILE, (maxy[ok] - 1 - y0) // TILE + 1
    d = np.zeros((tiles_y + 1, tiles_x + 1), np.int64)
    np.add.at(d, (ty0, tx0), 1)
    np.add.at(d, (ty0, tx1), -1)
    np.add.at(d, (ty1, tx0), -1)
    np.add.at(d, (ty1, tx1), 1)
    return d.cumsum(0).cumsum(1)[:tiles_y, :tiles_x]


def sides_of_span_safe(spi, window):
    """(safe, unsafe): setup triangles with a non-empty clamped box in `window` whose coordinates all lie within
    +-SPAN_SAFE, and those with one beyond it (the span kernel sweeps these)."""
    ok = clamped_boxes(spi, window)[4]
    far = np.abs(spi.astype(np.int64)).max(axis=(1, 2)) > SPAN_SAFE
    return int((ok & ~far).sum()), int((ok & far).sum())


def drawn(tri_id, window, fb_width=None):
    """(drawn pixels, [tiles_y, tiles_x] bool: tiles with a drawn pixel) of a window, from an id buffer.  The window's
    pixel (cx, cy) is depth index (cy - y0) * x1 + (cx - x0) (renderer.rs:362)."""
    x0, x1, y0, y1 = window
    ww, wh = x1 - x0, y1 - y0
    tiles_x, tiles_y = (ww + TILE - 1) // TILE, (wh + TILE - 1) // TILE
    idx = (np.arange(wh, dtype=np.int64) * x1)[:, None] + np.arange(ww, dtype=np.int64)[None, :] if x0 or y0 or x1 != fb_width else None
    d = (tri_id.reshape(wh, ww) if idx is None else tri_id[idx]) != 0xFFFFFFFF
    pad = np.zeros((tiles_y * TILE, tiles_x * TILE), bool)
    pad[:wh, :ww] = d
    return int(d.sum()), pad.reshape(tiles_y, TILE, tiles_x, TILE).any(axis=(1, 3))


def window_depth_index(window):
    """[wh, ww] int64: the depth-buffer index of every pixel of the window."""
    x0, x1, y0, y1 = window
    return (np.arange(y1 - y0, dtype=np.int64) * x1)[:, None] + np.arange(x1 - x0, dtype=np.int64)[None, :]


# ---- section 3a: large grids -------------------------------------------------------------------------------------------

# name -> (W, H, expected binning path).  Owned tiles: A 36,864 (the LDS limit), B 37,056, C 65,280 (magic division at its
# upper edge, window within SPAN_SAFE), D 65,536 (plain division, win_safe == 0); F: tiles_x == 1 and 2, coordinates up to
# the i16 edge inside a full-frame window.  Case E is D on a 2-rank partition (32,768 owned tiles: segmented).
LARGE = {
    "A": (6144, 6144, "seg"),
    "B": (6176, 6144, "csr"),
    "C": (8160, 8191, "csr"),
    "D": (8192, 8192, "csr"),
    "F_32x32767": (32, 32767, "seg"),
    "F_33x32767": (33, 32767, "seg"),
    "F_32767x32": (32767, 32, "seg"),
}
CASE_A_TRIANGLES = 800_000


def reached(dim):
    """The boundary values a frame axis of `dim` pixels reaches: a triangle with a vertex there draws inside the frame."""
    return tuple(v for v in BOUNDARY_VALUES if 0 <= v <= dim + 2)


def large_scene(oracle, name, n_random=None):
    """(depth_tris VS_CLIP [n,3,4], color_tris VS_CLIP_COLOR [m,3,7], hot [(x, y), ...]: centres of the hot tiles) of a section-3a case: one triangle per
    tile, a soup of small and a few large triangles, bands of triangles across the frame's right and bottom edges and across
    8191, the boundary generator's triangles for every value the frame reaches, and a cluster on one tile.  Case A adds
    `n_random` (default CASE_A_TRIANGLES) of scenes.random_clip_triangles, which is what overflows the binning's staging
    area; the CPU test passes a smaller count.  The colour draw is a w-jittered soup with clipped fans."""
    from f_renderer_amd import scenes
    W, H, _ = LARGE[name]
    full = (0, W, 0, H)
    seed = 1000 + sorted(LARGE).index(name) * 100
    mid = (W / 2.0, H / 2.0)
    parts = [tile_grid(W, H, full, seed + 1),
             pixel_soup(20000, W, H, mid, (W / 2.0 + 40, H / 2.0 + 40), (3.0, 40.0), seed + 2),
             pixel_soup(60, W, H, mid, (W / 2.0, H / 2.0), (200.0, 1500.0), seed + 3),
             # across the right and the bottom edge of the frame
             pixel_soup(1500, W, H, (W, H / 2.0), (60.0, H / 2.0), (8.0, 90.0), seed + 4),
             pixel_soup(1500, W, H, (W / 2.0, H), (W / 2.0, 60.0), (8.0, 90.0), seed + 5)]
    if W > SPAN_SAFE - 200:
        parts.append(pixel_soup(1500, W, H, (SPAN_SAFE, H / 2.0), (80.0, H / 2.0), (8.0, 90.0), seed + 6))
    if H > SPAN_SAFE - 200:
        parts.append(pixel_soup(1500, W, H, (W / 2.0, SPAN_SAFE), (W / 2.0, 80.0), (8.0, 90.0), seed + 7))
    vx, vy = reached(W), reached(H)
    if vx or vy:
        # the boundary vertices' partners sit a little inside the frame, next to the boundary
        bc = (min(max(vx) if vx else mid[0], W) - 100.0 if vx else mid[0], min(max(vy) if vy else mid[1], H) - 100.0 if vy else mid[1])
        parts.append(boundary_requests(W, H, vx, vy, bc, seed + 8, n_each=40))
    hot = (min(W - 16.0, 1000.0), min(H - 16.0, 2000.0))
    hot = [(float(int(hot[0]) // TILE * TILE + 16), float(int(hot[1]) // TILE * TILE + 16))]
    if H >= 6144:
        hot.append((hot[0][0], 6000.0))      # tile row 187: the other rank's in both layouts of a 2-rank partition (case E)
    for k, h in enumerate(hot):
        parts.append(cluster(1500, W, H, h, seed + 20 + k))
    if name == "A":
        parts.append(scenes.random_clip_triangles(CASE_A_TRIANGLES if n_random is None else n_random, W, H, seed=seed + 10))
    if name.startswith("F"):
        # a frame of 1 M pixels has to be drawn nearly everywhere: a backdrop of two triangles per 512-pixel stretch, first
        long_x = W > H
        L = max(W, H)
        quads = []
        for a in range(0, L, 512):
            b = min(a + 512, L) + 1
            lo, hi = -2.0, (H if long_x else W) + 2.0
            q = [((a, lo), (b, lo), (b, hi)), ((a, lo), (b, hi), (a, hi))]
            quads += q if long_x else [tuple((y, x) for x, y in t) for t in q]
        v = np.asarray(quads, np.float64)
        parts.insert(0, clip_from_pixels(v[..., 0], v[..., 1], W, H, w=2.0))
    depth_tris = np.concatenate(parts, axis=0)
    col = np.concatenate([pixel_soup(12000, W, H, mid, (W / 2.0 + 40, H / 2.0 + 40), (4.0, 60.0), seed + 11),
                          ] + [cluster(600, W, H, h, seed + 30 + k) for k, h in enumerate(hot)], axis=0)
    color_tris = with_colors(jitter_w(col, seed + 13), seed + 14)
    return depth_tris, color_tris, hot


def slot_records(ntris_setup, window):
    """Records of a tile's near-first slot (frr_api.hip: max(256, 16 * ntris / ntiles), rounded up)."""
    x0, x1, y0, y1 = window
    ntiles = ((x1 - x0 + TILE - 1) // TILE) * ((y1 - y0 + TILE - 1) // TILE)
    return max(256, (ntris_setup * 16 + ntiles - 1) // ntiles)


def large_conditions(name, frame, spi_depth, spi_color, hot, a_full=True):
    """The input conditions of section 3a, from the oracle alone: `frame` is the oracle's Frame after both draws, spi_* the
    setup lists of the two draws, `hot` the hot tiles' centres.  Returns the figures it checked (for assertion messages).
    a_full=False: case A at a reduced triangle count (the CPU test), where the 1,000,000 records are not expected."""
    W, H, _ = LARGE[name]
    full = (0, W, 0, H)
    out = {}
    npix, tiles = drawn(frame.tri_id, full, W)
    out["drawn_pixels"], out["tiles_drawn"], out["tiles"] = npix, int(tiles.sum()), int(tiles.size)
    assert npix >= 1_000_000, out
    assert tiles.sum() >= 0.9 * tiles.size, out
    rec = records_per_tile(spi_depth, full)
    out["bin_entries_depth"] = int(rec.sum())
    out["max_tile_records"], out["slot"] = int(rec.max()), slot_records(spi_depth.shape[0], full)
    rec2 = records_per_tile(spi_color, full)
    out["max_tile_records_color"], out["slot_color"] = int(rec2.max()), slot_records(spi_color.shape[0], full)
    # the hot tiles: beyond the near-first slot on the segmented path, and where the CSR path's counters are largest (with
    # two of them each rank of case E's 2-rank partition owns one, in both layouts)
    for hx, hy in hot:
        tx, ty = int(hx) // TILE, int(hy) // TILE
        out[f"hot_{tx}_{ty}"] = (int(rec[ty, tx]), int(rec2[ty, tx]))
        assert rec[ty, tx] > out["slot"] and rec2[ty, tx] > out["slot_color"], out
    if name == "A" and a_full:
        assert out["bin_entries_depth"] >= 1_000_000, out
    if name[0] in "CDF":
        safe, unsafe = sides_of_span_safe(spi_depth, full)
        out["safe"], out["unsafe"] = safe, unsafe
        assert safe >= 200 and unsafe >= 200, out
        for axis, dim in ((0, W), (1, H)):
            for v in reached(dim):
                out[f"hits_{'xy'[axis]}_{v}"] = hits(spi_depth, v, axis)
                assert out[f"hits_{'xy'[axis]}_{v}"] >= 20, out
    return out


# ---- section 3b: far windows on small frames --------------------------------------------------------------------------

# name -> (W, H, (x0, x1, y0, y1)).  2048 x 1024 where the depth index (wh - 1) * x1 + ww needs the room.  A window that
# STARTS at x0 = -32768 has to end at x1 > 0 (raster_check), so it is wider than 32,768 pixels and fits no frame of these
# sizes: left out.
FAR_WINDOWS = {
    "x_end_8191": (2048, 1024, (7791, 8191, 100, 300)),
    "x_end_8192": (2048, 1024, (7792, 8192, 100, 300)),
    "x_start_8191": (2048, 1024, (8191, 8591, 0, 200)),
    "x_start_8192": (2048, 1024, (8192, 8592, 0, 200)),
    "x_straddle_8191": (2048, 1024, (7991, 8391, 0, 200)),
    "y_end_8191": (512, 512, (0, 512, 7791, 8191)),
    "y_end_8192": (512, 512, (0, 512, 7792, 8192)),
    "y_start_8191": (512, 512, (0, 512, 8191, 8591)),
    "y_start_8192": (512, 512, (0, 512, 8192, 8592)),
    "y_straddle_8191": (512, 512, (0, 512, 8000, 8400)),
    "y_straddle_minus_8191": (512, 512, (0, 512, -8400, -8000)),      # also: wholly at negative y
    "xy_straddle_8191": (2048, 1024, (8000, 8400, 8100, 8300)),
    "x_end_32767": (2048, 1024, (31767, 32767, 0, 60)),
    "y_end_32767": (512, 512, (0, 512, 32367, 32767)),
    "y_start_minus_32768": (512, 512, (0, 512, -32768, -32368)),
    "x_negative_to_positive": (512, 512, (-200, 300, 0, 400)),
    "y_negative_near": (512, 512, (16, 500, -450, -50)),
    "x_negative_deep": (512, 512, (-400, 100, 0, 300)),               # stride 100, width 500: five pixels per depth entry
}


def far_scene(oracle, name, n_soup=1500, fans=False):
    """VS_CLIP triangles of a far-window case: a soup over the window and its surroundings, the boundary generator's
    triangles for the values next to or inside the window (every one of them in x, in y and in both), and a few triangles
    reaching in from every other boundary value -- slivers tens of thousands of pixels long, whose i32 edge functions
    wrap.  fans: the w-jittered variant with near-plane-crossing triangles."""
    W, H, win = FAR_WINDOWS[name]
    x0, x1, y0, y1 = win
    seed = 5000 + sorted(FAR_WINDOWS).index(name) * 50
    c = ((x0 + x1) / 2.0, (y0 + y1) / 2.0)
    ext = ((x1 - x0) / 2.0 + 40.0, (y1 - y0) / 2.0 + 40.0)
    near_x = tuple(v for v in BOUNDARY_VALUES if x0 - 3 <= v <= x1 + 3)
    near_y = tuple(v for v in BOUNDARY_VALUES if y0 - 3 <= v <= y1 + 3)
    parts = [pixel_soup(n_soup, W, H, c, ext, (4.0, 70.0), seed + 1),
             boundary_requests(W, H, near_x, near_y, c, seed + 2, n_each=24),
             boundary_requests(W, H, BOUNDARY_VALUES, (), c, seed + 3, n_each=3, reach=(0.9, 1.0)),
             boundary_requests(W, H, (), BOUNDARY_VALUES, c, seed + 4, n_each=3, reach=(0.9, 1.0))]
    for axis, (lo, hi) in enumerate(((x0, x1), (y0, y1))):
        for b in (SPAN_SAFE, -SPAN_SAFE):
            if lo - 100 <= b <= hi + 100:                  # a band of triangles across +-8191 where the window is near it
                cc = (b, c[1]) if axis == 0 else (c[0], b)
                ee = (60.0, ext[1]) if axis == 0 else (ext[0], 60.0)
                parts.append(pixel_soup(400, W, H, cc, ee, (4.0, 50.0), seed + 5 + axis))
    tris = np.concatenate(parts, axis=0)
    return jitter_w(tris, seed + 9) if fans else tris


def far_conditions(name, frame, spi):
    """The input conditions of section 3b, from the oracle alone."""
    W, H, win = FAR_WINDOWS[name]
    x0, x1, y0, y1 = win
    # (depth indices, not pixels: with x1 < x1 - x0 the rows of a window overlap in the depth buffer, renderer.rs:362)
    out = {"drawn_pixels": int((frame.tri_id[np.unique(window_depth_index(win))] != 0xFFFFFFFF).sum())}
    assert out["drawn_pixels"] >= 5000, out
    assert int((frame.tri_id != 0xFFFFFFFF).sum()) == out["drawn_pixels"], "the oracle drew outside the window"
    out["safe"], out["unsafe"] = sides_of_span_safe(spi, win)
    contains = any(lo < b < hi for lo, hi in ((x0, x1), (y0, y1)) for b in (SPAN_SAFE, -SPAN_SAFE))
    if contains:
        assert out["safe"] >= 20 and out["unsafe"] >= 20, out
    return out


# ---- the oracle's frames of the scenes above (both test files render them the same way) ----------------------------------

FAR_VARIANTS = ("depth", "color", "fans")


def render_far(oracle, name, variant="depth", n_soup=1500):
    """dict(tris, vs, ps: names of the shader-table entries, frame: the oracle's Frame, spi: its setup list) of a
    far-window case.  depth: VS_CLIP / PS_DEPTH; color: the same soup with vertex colours, PS_COLOR; fans: the w-jittered
    soup with clipped fans, PS_DEPTH."""
    W, H, win = FAR_WINDOWS[name]
    tris = far_scene(oracle, name, n_soup, fans=variant == "fans")
    vs, ps = ("CLIP_COLOR", "COLOR") if variant == "color" else ("CLIP", "DEPTH")
    if variant == "color":
        tris = with_colors(tris, 77)
    f = oracle.Frame(W, H)
    f.clear()
    setup = f.draw(tris, getattr(oracle, "VS_" + vs), getattr(oracle, "PS_" + ps), oracle.make_uniforms(), window=win, keep_setup=True)
    return dict(tris=tris, vs=vs, ps=ps, frame=f, spi=setup["spi"].copy(), W=W, H=H, window=win)


def render_large(oracle, name, n_random=None):
    """dict(depth_tris, color_tris, hot, frame, spi_depth, spi_color) of a section-3a case: the depth-only draw, then the
    VS_CLIP_COLOR / PS_COLOR draw into the same frame."""
    W, H, _ = LARGE[name]
    depth_tris, color_tris, hot = large_scene(oracle, name, n_random)
    f = oracle.Frame(W, H)
    f.clear()
    u = oracle.make_uniforms()
    f.draw(depth_tris, oracle.VS_CLIP, oracle.PS_DEPTH, u)
    f.draw(color_tris, oracle.VS_CLIP_COLOR, oracle.PS_COLOR, u, tri_id_base=int(f.counters.tris_setup))
    return dict(depth_tris=depth_tris, color_tris=color_tris, hot=hot, frame=f, W=W, H=H,
                spi_depth=setup_spi(oracle, W, H, depth_tris), spi_color=setup_spi(oracle, W, H, color_tris, oracle.VS_CLIP_COLOR))
