"""Scenes that feed the SHADING arithmetic hostile attributes (test_shading_oracle.py on the CPU, test_gpu_shading_edges.py on
the GPU): zero / tiny / huge / non-finite normals, degenerate light and view geometry, uv outside [0, 1], odd texture sizes,
vertex colours outside [0, 1), subnormal 1/w, and all of these on triangles the clipper cuts.  No tests in here.

Everything is deterministic: NumPy and scenes.splitmix_u01 only.  Every frame is 96 x 64 (3 x 2 tiles).  The carrier of most
scenes is a grid of 16 x 16 pixel cells, two triangles each; in every cell one triangle is HOSTILE (it carries a sub-class of
the scene's attribute class) and the other ORDINARY (unit normals, uv in [0, 1], colours in [0, 1), w about 1), so that
hostile and ordinary pixels share tiles and waves.  The VS_PHONG / VS_GOURAUD scenes use identity matrices and w = 1
geometry: the attributes reach the shader as written.

A scene is the tuple (W, H, mesh, vs, ps, uniforms, texture, window) plus `sub` (the sub-class name of every input
triangle), `then` (None, or a second (mesh, sub) drawn over the first without a clear) and `family`.
"""
from collections import namedtuple

import numpy as np

from f_renderer_amd import scenes as _scenes

W, H, TILE, CELL = 96, 64, 32, 16
ORDINARY = "ordinary"
NEG_WINDOW = (-32, 64, 0, 64)           # x0 < 0: the pass goes through k_raster_entries (texels by IEEE division)

Scene = namedtuple("Scene", "W H mesh vs ps uniforms texture window sub then family")

DEFAULT_UNIFORMS = dict(model=np.eye(4, dtype=np.float32).reshape(-1), view=np.eye(4, dtype=np.float32).reshape(-1),
                        proj=np.eye(4, dtype=np.float32).reshape(-1), view_pos=(0.0, 0.0, 0.0), light_pos=(1.2, 1.0, 2.0),
                        light_color=(1.0, 1.0, 1.0), ambient=0.1, specular=0.5)


def _u(seed, *shape):
    return _scenes.splitmix_u01(0x5AD1E000 + seed, int(np.prod(shape))).reshape(shape)


# ---- carriers ---------------------------------------------------------------------------------------------------------

def grid_pixels(shift=(0.0, 0.0), cells=None):
    """([n,3,2] pixel corners, [n] bool hostile) of the cell grid: two triangles per cell, the hostile one alternating like a
    chess board.  shift moves the whole grid; cells keeps only the cells whose (cx + 2 cy) % 3 is in `cells`."""
    tris, hostile = [], []
    for cy in range(H // CELL):
        for cx in range(W // CELL):
            if cells is not None and (cx + 2 * cy) % 3 not in cells:
                continue
            x0, y0 = cx * CELL + shift[0], cy * CELL + shift[1]
            x1, y1 = x0 + CELL, y0 + CELL
            tris += [((x0, y0), (x1, y0), (x1, y1)), ((x0, y0), (x1, y1), (x0, y1))]
            first = (cx + cy) % 2 == 0
            hostile += [first, not first]
    return np.asarray(tris, np.float64), np.asarray(hostile, bool)


def ndc_of_pixels(px):
    return np.stack([2.0 * px[..., 0] / W - 1.0, 1.0 - 2.0 * px[..., 1] / H], axis=-1)


def ordinary_normals(seed, n):
    v = np.concatenate([0.6 * (_u(seed, n, 3, 2) - 0.5), np.ones((n, 3, 1))], axis=2)
    return v / np.sqrt((v * v).sum(axis=2, keepdims=True))


def phong_mesh(px, uv, normals, z=0.5):
    """[n,3,8] f32: pos3 (w = 1 under identity matrices), uv2, normal3."""
    n = px.shape[0]
    zz = np.broadcast_to(np.asarray(z, np.float64), (n, 3))[..., None]
    with np.errstate(all="ignore"):
        return np.concatenate([ndc_of_pixels(px), zz, uv, normals], axis=2).astype(np.float32)


def clip_mesh(px, w, extra=None, z=0.5):
    """[n,3,4(+3)] f32: clip position of pixel corners `px` at per-vertex `w` (+ a colour)."""
    ndc = ndc_of_pixels(px)
    w = np.asarray(w, np.float64)[..., None]
    pos = np.concatenate([ndc * w, z * w, w], axis=2)
    with np.errstate(all="ignore"):
        return (pos if extra is None else np.concatenate([pos, extra], axis=2)).astype(np.float32)


def assign(hostile, names):
    """[n] sub-class names: the hostile triangles take `names` in turn.  Also the index of each within its sub-class."""
    sub, variant, j = [], [], 0
    for h in hostile:
        if h:
            sub.append(names[j % len(names)])
            variant.append(j // len(names))
            j += 1
        else:
            sub.append(ORDINARY)
            variant.append(0)
    return np.asarray(sub), np.asarray(variant)


# ---- attribute sets: f(sub-class, variant, ordinary value [3, k]) -> [3, k] -------------------------------------------

NORMALS_SMALL = ("zero3", "zero1", "opposite", "negzero", "dot_subnormal", "dot_underflow")
NORMALS_BIG = ("dot_overflow", "inf", "nan")


def hostile_normal(name, v, base):
    """zero at three vertices / at one; opposite normals that interpolate through zero; -0.0 components; components about
    1e-20 (dot is subnormal); 1e-30 to 1e-38 (dot underflows to 0); 1e19 to 3e38 (dot overflows; 1e19 just does not);
    +-inf and NaN components."""
    n = np.array(base, np.float64)
    sign = np.where(_u(900 + v, 3, 3) < 0.5, -1.0, 1.0)
    if name == "zero3":
        n[:] = 0.0
    elif name == "zero1":
        n[v % 3] = 0.0
    elif name == "opposite":
        n[1] = -n[0]
        n[2] = n[0] if v % 2 else -n[0]
    elif name == "negzero":
        n[:] = [[-0.0, -0.0, 1.0], [-0.0, -0.0, -0.0], [0.0, -0.0, -1.0]][v % 3]
    elif name == "dot_subnormal":
        n = sign * 1e-20 * (0.5 + _u(910 + v, 3, 3))
    elif name == "dot_underflow":
        n = sign * np.array([1e-30, 1e-33, 1e-36, 1e-38])[(np.arange(9).reshape(3, 3) + v) % 4] * (0.5 + 0.5 * _u(920 + v, 3, 3))
    elif name == "dot_overflow":
        n = sign * np.array([1e19, 1e20, 1e30, 3e38])[(np.arange(9).reshape(3, 3) // 3 + v) % 4] * (0.9 + 0.1 * _u(930 + v, 3, 3))
    elif name == "inf":
        n[v % 3, v % 2] = np.inf
        n[(v + 1) % 3, 2] = -np.inf if v % 2 else n[(v + 1) % 3, 2]
        if v % 4 == 3:
            n[:] = np.inf
    elif name == "nan":
        n[v % 3, (v // 3) % 3] = np.nan
        if v % 4 == 3:
            n[:] = np.nan
    return n


UV_SUBS = ("unit_edges", "below_zero", "above_one", "huge", "inf", "nan", "subnormal")
ONE_BELOW = 1.0 - 2.0 ** -24


def hostile_uv(name, v, base):
    """exactly 0, 1 and 1 - 2^-24; just below 0 and -3; 5 and 1e9; 1e30 and 3e38; +-inf; NaN; subnormals.  Odd variants
    leave one vertex ordinary, so the interpolation mixes the two."""
    t = {"unit_edges": [[0.0, 0.0], [1.0, ONE_BELOW], [ONE_BELOW, 1.0]],
         "below_zero": [[-2.0 ** -24, 0.25], [-3.0, -2.0 ** -30], [0.5, -3.0]],
         "above_one": [[5.0, 0.5], [1e9, 5.0], [0.25, 1e9]],
         "huge": [[1e30, 0.5], [-1e30, 3e38], [3e38, 1e30]],
         "inf": [[np.inf, 0.5], [0.5, -np.inf], [np.inf, np.inf]],
         "nan": [[np.nan, 0.5], [0.25, np.nan], [np.nan, np.nan]],
         "subnormal": [[1e-40, -1e-40], [1.4e-45, 0.5], [-1.4e-45, 1e-39]]}[name]
    uv = np.roll(np.array(t, np.float64), v, axis=0)
    if v % 2 and name not in ("nan",):
        uv[v % 3] = base[v % 3]
    return uv


COLOR_SUBS = ("out_of_range", "huge", "inf", "nan", "tiny", "steps")
STEP_K = (1, 64, 128, 254, 255)


def hostile_color(name, v, base):
    """negative and > 1; 1e38; +-inf (mixed per vertex: the interpolation sees inf - inf and 0 * inf); NaN; subnormals and
    -0.0; a constant colour on both sides of a k/255 step (r: the f32 below k/255, g: k/255 itself, b: the f32 above)."""
    if name == "steps":
        s = np.float32(STEP_K[v % len(STEP_K)]) / np.float32(255.0)
        c = np.array([np.nextafter(s, np.float32(-1)), s, np.nextafter(s, np.float32(2))], np.float64)
        return np.tile(c, (3, 1))
    t = {"out_of_range": [[-0.5, 1.5, 0.5], [7.0, -3.0, 1.0], [1.0000001, -1e-7, 2.0]],
         "huge": [[1e38, 0.5, -1e38], [3e38, 3e38, 0.25], [-3e38, 1e38, 1e38]],
         "inf": [[np.inf, -np.inf, 0.5], [-np.inf, np.inf, np.inf], [0.0, 0.0, -np.inf]],
         "nan": [[np.nan, 0.5, 0.25], [0.5, np.nan, 0.25], [0.5, 0.25, np.nan]],
         "tiny": [[1e-40, -0.0, -1e-40], [1.4e-45, 1e-38, -0.0], [-0.0, -1.4e-45, 0.0039]]}[name]
    c = np.roll(np.array(t, np.float64), v, axis=0)
    if v % 2:
        c[v % 3] = base[v % 3]
    return c


def paste(sub, variant, ordinary, make):
    out = np.array(ordinary, np.float64)
    for i, (s, v) in enumerate(zip(sub, variant)):
        if s != ORDINARY:
            out[i] = make(s, int(v), ordinary[i])
    return out


# ---- textures ---------------------------------------------------------------------------------------------------------

def texture_all_bytes():
    """64 x 64: every byte value 0..255 in every channel (each channel a bijection of the texel index mod 256)."""
    i = np.arange(64 * 64, dtype=np.int64)
    t = np.stack([i % 256, (i * 7 + 13) % 256, 255 - (i // 16) % 256, (i * 3 + 101) % 256], axis=1)
    return np.ascontiguousarray(t.reshape(64, 64, 4).astype(np.uint8))


def texture_ge64():
    """32 x 32, every texel of every channel >= 64: a sampled colour is at least about 0.25."""
    y, x = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    t = np.stack([64 + (x * 5 + y * 3 + 17 * c) % 192 for c in range(4)], axis=2)
    return np.ascontiguousarray(t.astype(np.uint8))


def texture_small(w, h):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    t = np.stack([(x * 83 + y * 47 + 29 * c + 11) % 256 for c in range(4)], axis=2)
    return np.ascontiguousarray(t.astype(np.uint8))


TEXTURES = {"1x1": lambda: texture_small(1, 1), "3x3": lambda: texture_small(3, 3), "5x9": lambda: texture_small(5, 9),
            "all_bytes": texture_all_bytes, "ge64": texture_ge64}


# ---- light / view geometry ---------------------------------------------------------------------------------------------

S70 = 2.0 ** -70


def _diag(s):
    return np.diag([s, s, s, 1.0]).astype(np.float32).reshape(-1)


# name -> uniforms.  mirrored_far: light and eye 1.4e19 above and below the surface; the unit l and v are opposite up to
# 2 (x, y) / 1.4e19, so |l + v|^2 is about (x^2 + y^2) * 2e-38: subnormal in a disc around the centre of the frame.
# tiny_world: model = 2^-70, view = 2^70 (their product is exactly the identity), light and eye at that scale: every l.l
# and v.v is subnormal.
LIGHTS = {
    "light_eq_view": dict(light_pos=(0.3, 0.2, 2.0), view_pos=(0.3, 0.2, 2.0)),
    "mirrored_near": dict(light_pos=(0.010416667, 0.015625, 2.0), view_pos=(0.010416667, 0.015625, -1.0)),
    "mirrored_far": dict(light_pos=(0.0, 0.0, 1.4e19), view_pos=(0.0, 0.0, -1.4e19)),
    "light_huge": dict(light_pos=(1e30, 1e30, 1e30)),
    "light_inf": dict(light_pos=(np.inf, 1.0, 2.0)),
    "view_huge": dict(view_pos=(0.0, 0.0, -3e38)),
    "tiny_world": dict(model=_diag(S70), view=_diag(2.0 ** 70), light_pos=(1.2 * S70, S70, 2.0 * S70), view_pos=(0.0, 0.0, -S70)),
    "lc_zero_spec_neg": dict(light_color=(0.0, 0.0, 0.0), specular=-1.0),
    "lc_neg_spec_1e30": dict(light_color=(-1.0, 0.5, -0.25), specular=1e30),
    "lc_1e30_spec_inf": dict(light_color=(1e30, 1.0, 1e-30), specular=np.inf),
    "lc_inf_spec_zero": dict(light_color=(np.inf, -np.inf, 1.0), specular=0.0),
}


# ---- the scenes ---------------------------------------------------------------------------------------------------------

def _uniforms(**kw):
    return dict(DEFAULT_UNIFORMS, **kw)


def _phong_grid(seed, subs, normal_maker=None, uv_maker=None):
    px, hostile = grid_pixels()
    sub, variant = assign(hostile, subs)
    n = px.shape[0]
    normals = ordinary_normals(seed, n)
    uv = np.stack([px[..., 0] / W, px[..., 1] / H], axis=-1) * 0.999 + 0.0005 * _u(seed + 1, n, 3, 2)
    if normal_maker:
        normals = paste(sub, variant, normals, normal_maker)
    if uv_maker:
        uv = paste(sub, variant, uv, uv_maker)
    return phong_mesh(px, uv, normals), sub


def _rhw_layer(seed, shift, cells, subs, colors, ordinary=True):
    """A grid layer of the 1/w class: `subnormal*` triangles have every w in [2^126, 2^128), `mixed*` ones a single such
    vertex among w about 1, ordinary ones w in [0.5, 2) (ordinary=False: left out -- any of them beats every subnormal
    depth under it)."""
    px, hostile = grid_pixels(shift, cells)
    px = np.clip(px, 0.0, [W, H])             # (a shifted layer stays inside the frame: nothing of this class is clipped)
    if not ordinary:
        px, hostile = px[hostile], hostile[hostile]
    sub, _ = assign(hostile, subs)
    n = px.shape[0]
    w = 0.5 * 4.0 ** _u(seed, n, 3)
    big = 2.0 ** 126 * np.minimum(4.0 ** _u(seed + 1, n, 3) * (1.0 + 2.0 ** -20), 3.999)
    for i, s in enumerate(sub):
        if s.startswith("subnormal"):
            w[i] = big[i]
        elif s.startswith("mixed"):
            w[i, i % 3] = big[i, 0]
    extra = _u(seed + 2, n, 3, 3) if colors else None
    return clip_mesh(px, w, extra), sub


def _clip_carrier(seed, n=300):
    """scenes.random_clip_triangles with spread > 1 (side-plane crossings) and, on a vertex of every fifth triangle, z
    beyond the far plane or behind the near plane.  -> ([n,3,4] clip positions f64, [n] bool hostile)."""
    t = _scenes.random_clip_triangles(n, W, H, seed=0xC11F000 + seed, spread=1.25).astype(np.float64)
    k = np.arange(n)
    far, near = k % 5 == 1, k % 5 == 3
    t[far, k[far] % 3, 2] = 1.3 * t[far, k[far] % 3, 3]
    t[near, k[near] % 3, 2] = -0.2 * t[near, k[near] % 3, 3]
    return t, k % 2 == 0


def _clip_phong(seed, subs, normal_maker=None, uv_maker=None):
    t, hostile = _clip_carrier(seed)
    sub, variant = assign(hostile, subs)
    n = t.shape[0]
    ndc = t[..., :3] / t[..., 3:4]
    normals = ordinary_normals(seed + 3, n)
    uv = _u(seed + 4, n, 3, 2)
    if normal_maker:
        normals = paste(sub, variant, normals, normal_maker)
    if uv_maker:
        uv = paste(sub, variant, uv, uv_maker)
    with np.errstate(all="ignore"):
        return np.concatenate([ndc, uv, normals], axis=2).astype(np.float32), sub


def build():
    """name -> Scene, in a fixed order."""
    out = {}
    checker = _scenes.checker_texture(32, 4)

    def add(name, family, mesh, vs, ps, sub, uniforms=None, texture=None, then=None):
        out[name] = Scene(W, H, mesh, vs, ps, uniforms or _uniforms(), texture, None, sub, then, family)

    # normals: through the two Phong pixel shaders and through the Gouraud vertex shader
    small, small_sub = _phong_grid(10, NORMALS_SMALL, normal_maker=hostile_normal)
    big, big_sub = _phong_grid(20, NORMALS_BIG, normal_maker=hostile_normal)
    for tag, mesh, sub in (("small", small, small_sub), ("big", big, big_sub)):
        add(f"normals_{tag}/phong", "normals", mesh, "PHONG", "PHONG", sub, texture=checker)
        add(f"normals_{tag}/blinn", "normals", mesh, "PHONG", "BLINN", sub, texture=checker)
        add(f"normals_{tag}/gouraud", "normals", mesh, "GOURAUD", "COLOR", sub)
    # light / view geometry and light colours, over the small-normals mesh
    for lname, kw in LIGHTS.items():
        for ps in ("PHONG", "BLINN"):
            add(f"{lname}/{ps.lower()}", "light", small, "PHONG", ps, small_sub, uniforms=_uniforms(**kw), texture=checker)
    # uv, and the textures (each with the hostile uv mesh, but the >= 64 one)
    uvm, uv_sub = _phong_grid(30, UV_SUBS, uv_maker=hostile_uv)
    add("uv/phong", "uv", uvm, "PHONG", "PHONG", uv_sub, texture=checker)
    add("uv/blinn", "uv", uvm, "PHONG", "BLINN", uv_sub, texture=checker)
    for tname in ("1x1", "3x3", "5x9", "all_bytes"):
        add(f"tex_{tname}", "texture", uvm, "PHONG", "PHONG", uv_sub, texture=TEXTURES[tname]())

    def ge64_normal(name, v, base):
        return hostile_normal("zero3" if v % 2 else "zero1", v, base) if name == "normal_zero" else base

    def ge64_uv(name, v, base):
        return np.array([[np.nan, np.nan]] * 3) if name == "uv_nan" else base
    gm, g_sub = _phong_grid(40, ("normal_zero", "uv_nan"), normal_maker=ge64_normal, uv_maker=ge64_uv)
    add("tex_ge64", "texture", gm, "PHONG", "PHONG", g_sub, texture=TEXTURES["ge64"]())
    # vertex colours, at per-vertex w in [0.5, 2)
    px, hostile = grid_pixels()
    sub, variant = assign(hostile, COLOR_SUBS)
    col = paste(sub, variant, _u(51, px.shape[0], 3, 3), hostile_color)
    add("colors", "colors", clip_mesh(px, 0.5 * 4.0 ** _u(50, px.shape[0], 3), col), "CLIP_COLOR", "COLOR", sub)
    # subnormal 1/w: three overlapping layers, then two more drawn over them without a clear
    for tag, vs, ps, colors in (("depth", "CLIP", "DEPTH", False), ("color", "CLIP_COLOR", "COLOR", True)):
        layers = [_rhw_layer(60, (0.0, 0.0), None, ("subnormal",), colors),
                  _rhw_layer(63, (5.0, 3.0), (0, 1), ("subnormal_over", "mixed"), colors, False),
                  _rhw_layer(66, (-6.0, -5.0), (1,), ("subnormal_over",), colors, False)]
        second = [_rhw_layer(70, (-4.0, 6.0), (0, 2), ("subnormal_second", "mixed_second"), colors, False),
                  _rhw_layer(73, (9.0, -7.0), (2,), ("subnormal_second",), colors, False)]
        mesh, sub = (np.concatenate([x[i] for x in layers]) for i in (0, 1))
        then = tuple(np.concatenate([x[i] for x in second]) for i in (0, 1))
        add(f"rhw/{tag}", "rhw", mesh, vs, ps, sub, then=then)
    # through the clipper
    m, sub = _clip_phong(89, NORMALS_SMALL + NORMALS_BIG, normal_maker=hostile_normal)
    add("clip_normals", "clip", m, "PHONG", "PHONG", sub, texture=checker)
    add("clip_normals/gouraud", "clip", m, "GOURAUD", "COLOR", sub)
    m, sub = _clip_phong(81, UV_SUBS, uv_maker=hostile_uv)
    add("clip_uv", "clip", m, "PHONG", "BLINN", sub, texture=TEXTURES["all_bytes"]())
    t, hostile = _clip_carrier(82)
    sub, variant = assign(hostile, COLOR_SUBS)
    col = paste(sub, variant, _u(83, t.shape[0], 3, 3), hostile_color)
    with np.errstate(all="ignore"):
        add("clip_colors", "clip", np.concatenate([t, col], axis=2).astype(np.float32), "CLIP_COLOR", "COLOR", sub)
    t, hostile = _clip_carrier(84)
    sub, _ = assign(hostile, ("subnormal", "mixed"))
    ndc = t[..., :3] / t[..., 3:4]
    w = t[..., 3].copy()
    big = 2.0 ** 126 * (1.0 + _u(85, t.shape[0], 3) * (1.0 - 2.0 ** -20) + 2.0 ** -22)     # [2^126, 2^127): |x| w < 2^128
    for i, s in enumerate(sub):
        if s == "subnormal":
            w[i] = big[i]
        elif s == "mixed":
            w[i, i % 3] = big[i, 0]
    pos = np.concatenate([ndc * w[..., None], w[..., None]], axis=2)
    add("clip_rhw", "clip", np.concatenate([pos, _u(86, t.shape[0], 3, 3)], axis=2).astype(np.float32), "CLIP_COLOR", "COLOR", sub)
    return out


_cache = {}


def all_scenes():
    if "scenes" not in _cache:
        _cache["scenes"] = build()
    return _cache["scenes"]


def names(*families):
    return [n for n, s in all_scenes().items() if not families or s.family in families]


# ---- running a scene on the three implementations -----------------------------------------------------------------------

CLEAR = (30, 30, 30, 255)


def oracle_frame(oracle, scene, window=None):
    """The C oracle's frame of a scene: dict(frame, setup: [the setup list of every draw], bases: [tri_id_base of every
    draw]).  Raises if the reference would have panicked."""
    f = oracle.Frame(scene.W, scene.H)
    f.clear(CLEAR, 0.0)
    u = oracle.make_uniforms(tex=None if scene.texture is None else oracle.Texture(scene.texture), **scene.uniforms)
    setups, bases = [], []
    for mesh in [scene.mesh] + ([scene.then[0]] if scene.then else []):
        bases.append(int(f.counters.tris_setup))
        setups.append(f.draw(mesh, getattr(oracle, "VS_" + scene.vs), getattr(oracle, "PS_" + scene.ps), u, window=window or scene.window,
                             tri_id_base=bases[-1], keep_setup=True))
    return dict(frame=f, setup=setups, bases=bases)


def numpy_frame(scene, debug=None):
    """The NumPy restatement's frame: dict(color, depth, tri_id, setup: [list per draw], covered)."""
    from oracle import oracle_np as onp
    color = np.zeros((scene.H, scene.W, 4), np.uint8)
    color[...] = CLEAR
    depth, tid = np.zeros(scene.W * scene.H, np.float32), np.full(scene.W * scene.H, 0xFFFFFFFF, np.uint32)
    u = onp.Uniforms(tex=scene.texture, **scene.uniforms)
    setups, covered, base = [], 0, 0
    for mesh in [scene.mesh] + ([scene.then[0]] if scene.then else []):
        s, c = onp.draw(scene.W, scene.H, mesh, getattr(onp, "VS_" + scene.vs), getattr(onp, "PS_" + scene.ps), u, color, depth, tid,
                        window=scene.window, tri_id_base=base, debug=debug)
        setups.append(s)
        covered += c
        base += len(s)
    return dict(color=color, depth=depth, tri_id=tid, setup=setups, covered=covered)


def gpu_run(r, scene, window=None, shader=None):
    """Clear, draw and read a scene back on Renderer `r` (every uniform is set: a Renderer may be reused across scenes).
    shader: the id of a registered user shader that stands in for the scene's built-in pair.
    -> (color, depth, tri_id, stats)."""
    import f_renderer_amd as fr
    u = scene.uniforms
    if scene.texture is not None:
        r.set_texture(0, scene.texture)
    r.set_uniforms(model=u["model"], view=u["view"], proj=u["proj"], view_pos=u["view_pos"], light_pos=u["light_pos"],
                   light_color=u["light_color"], ambient_strength=u["ambient"], specular_strength=u["specular"], texture_slot=0)
    vs = getattr(fr, "VS_" + scene.vs) if shader is None else shader
    ps = getattr(fr, "PS_" + scene.ps) if shader is None else shader
    x0, x1, y0, y1 = window or scene.window or (0, scene.W, 0, scene.H)
    r.clear(CLEAR, 0.0)
    meshes = []
    try:
        for mesh in [scene.mesh] + ([scene.then[0]] if scene.then else []):
            meshes.append(r.upload_mesh(mesh, vs))
            r.draw(meshes[-1], ps, (x0, x1), (y0, y1))
        c, d, t = r.readback()
        return c, d, t, r.stats()
    finally:
        for m in meshes:
            m.free()


# ---- what the oracle's output says about a scene ------------------------------------------------------------------------

def owners(oracle, scene):
    """[setup triangles of all draws] -> the sub-class name of the input triangle each came from (a clipped triangle's fan
    inherits its name)."""
    u = oracle.make_uniforms(tex=None if scene.texture is None else oracle.Texture(scene.texture), **scene.uniforms)
    vs = getattr(oracle, "VS_" + scene.vs)
    out = []
    for mesh, sub in [(scene.mesh, scene.sub)] + ([scene.then] if scene.then else []):
        for tri, s in zip(mesh, sub):
            out += [s] * oracle.geometry_processing(scene.W, scene.H, tri, vs, u).shape[0]
    return np.asarray(out)


def pixels_per_sub(oracle, scene, tri_id):
    """sub-class name -> pixels of the final frame whose last passing fragment came from it."""
    own = owners(oracle, scene)
    won = tri_id[tri_id != 0xFFFFFFFF]
    names_, counts = np.unique(own[won], return_counts=True)
    return dict(zip(names_.tolist(), counts.tolist()))


def tiles_drawn(tri_id):
    d = (tri_id != 0xFFFFFFFF).reshape(H // TILE, TILE, W // TILE, TILE)
    return int(d.any(axis=(1, 3)).sum())
