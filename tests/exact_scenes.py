"""Scenes in which (nearly) every f32 operation of the reference is exact (TEST INFRASTRUCTURE ONLY; no tests in this file).

Positions are dyadic: pixel p of a width-W frame is x = 2p/W - 1, row p of a height-H frame y = 1 - 2p/H, both times the
vertex's w, which is a power of two.  A triangle's doubled area in pixels is a power of two wherever its pixels are meant to
be exact, so 1 / (a + b + c) does not round (renderer.rs:351-358).  Everything is a fractions.Fraction; the tests turn the
inputs into float32 (exactly: every input is an f32) for the oracles and the library, and hand the evaluator of
tests/exact_reference.py the same numbers.  Each generator asserts, with the evaluator, the property it is named for, and
every scene asserts the exact-share condition: at least three quarters of the covered pixels, and at least 64, are exact
through the last value the scene compares (`through`).
"""
import functools
from fractions import Fraction as Fr

from . import exact_reference as er

SHARE = Fr(3, 4)
MIN_EXACT = 64


class Scene:
    """One draw of `tris` (input triangles: three vertices of NF rationals each, the layout of the vertex shader `vs`)
    through pixel shader `ps` into a W x H frame cleared to depth 0, in `window` (x0, x1, y0, y1; None: the whole frame).
    through: the last value compared with equality as the assertion -- "depth", "input" (the pixel shader's input) or
    "color" (the RGBA8 bytes, and the input where it is exact)."""

    def __init__(self, name, W, H, vs, ps, tris, through, window=None, tex=None, uniforms=None, expect=None, translates=None):
        self.name, self.W, self.H, self.vs, self.ps, self.through = name, W, H, vs, ps, through
        self.translates = [(Fr(x), Fr(y)) for x, y in (translates or [(0, 0)])]   # one pass per entry: the model matrices of an instanced pass
        self.tris = [[[Fr(c) for c in v] for v in t] for t in tris]
        self.window, self.tex, self.uniforms = window, tex, dict(uniforms or {})
        self.expect = dict(expect or {})                 # what the coverage test looks for in the evaluator's output

    def vs_out(self, translate=(0, 0)):
        """The vertex shader's outputs (renderer.rs:116) of every input: (clip position, context).  CLIP_COLOR: position
        xyzw, colour rgb.  PHONG under identity view and projection and a model matrix that translates by `translate`
        (phong.rs:114-126): position xyz, uv, normal -> context uv, normal, world position; every sum of mvp * pos has at
        most two non-zero terms, both dyadic and small, so the vertex shader is exact in any association."""
        out = []
        tx, ty = Fr(translate[0]), Fr(translate[1])
        for t in self.tris:
            tri = []
            for v in t:
                if self.vs == "CLIP":
                    tri.append((v[:4], []))
                elif self.vs == "CLIP_COLOR":
                    tri.append((v[:4], v[4:7]))
                else:
                    world = [v[0] + tx, v[1] + ty, v[2]]
                    tri.append((world + [Fr(1)], v[3:5] + v[5:8] + world))
            out.append(tri)
        return out

    def er_uniforms(self):
        tex = er.Texture(self.tex) if self.tex is not None else None
        return er.Uniforms(tex=tex, **self.uniforms)

    def evaluate(self, perturb=(), translates=None):
        """The evaluator's frame of this scene (one pass per entry of `translates`)."""
        f = er.Frame(self.W, self.H)
        u = self.er_uniforms()
        for tr in (translates or self.translates):
            f.draw(self.vs_out(tr), self.ps, u, self.window, perturb)
        f.uniforms = u
        return f

    def models_f32(self):
        """The model matrices of the passes, column-major float32 [n, 16]."""
        import numpy as np
        m = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (len(self.translates), 1))
        for i, (tx, ty) in enumerate(self.translates):
            m[i, 12], m[i, 13] = float(tx), float(ty)
        return m

    def share(self, f=None):
        """(exact entries, owned entries) through self.through"""
        f = f or frame(self.name)
        return len(f.exact_entries(self.through)), len(f.owned_entries())


def px(p, W):
    return Fr(2 * Fr(p), W) - 1


def py(p, H):
    return 1 - Fr(2 * Fr(p), H)


def vert(W, H, p, w=1, z=Fr(1, 2), color=None):
    """A CLIP / CLIP_COLOR input at pixel position p = (x, y) with the given w; z is given in NDC."""
    w = Fr(w)
    v = [px(p[0], W) * w, py(p[1], H) * w, Fr(z) * w, w]
    return v + [Fr(c) for c in color] if color is not None else v


def tri(W, H, pts, ws=(1, 1, 1), colors=None, z=Fr(1, 2)):
    zs = z if isinstance(z, (list, tuple)) else (z, z, z)
    return [vert(W, H, p, w, zz, c) for p, w, zz, c in zip(pts, ws, zs, colors or (None, None, None))]


H2 = Fr(1, 2)
# doubled area 512, 512, 512; integer corners, half-integer corners, and both in one triangle; both orientations; each
# crosses the border between two 32-pixel tiles
SHAPES = [[(8, 8), (40, 8), (8, 24)],
          [(8 + H2, 30 + H2), (8 + H2, 46 + H2), (40 + H2, 30 + H2)],
          [(44, 8 + H2), (60, 8 + H2), (44, 40 + H2)]]
# k / 32: with weights that are multiples of 2^-11 the interpolated colour and its product with 255 fit 24 bits
COLORS = [[(Fr(8, 32), Fr(31, 32), Fr(1, 32)), (Fr(24, 32), Fr(3, 32), Fr(16, 32)), (Fr(1, 32), Fr(17, 32), Fr(30, 32))],
          [(Fr(32, 32), Fr(0, 32), Fr(5, 32)), (Fr(2, 32), Fr(28, 32), Fr(9, 32)), (Fr(12, 32), Fr(12, 32), Fr(32, 32))],
          [(Fr(7, 32), Fr(21, 32), Fr(11, 32)), (Fr(29, 32), Fr(4, 32), Fr(19, 32)), (Fr(15, 32), Fr(32, 32), Fr(0, 32))]]
W0 = H0 = 64


def flat_w():
    out = []
    for name, w in (("flat_w1", 1), ("flat_w2", 2), ("flat_whalf", Fr(1, 2))):
        tris = [tri(W0, H0, s, (w, w, w), c) for s, c in zip(SHAPES, COLORS)]
        out.append(Scene(name, W0, H0, "CLIP_COLOR", "color", tris, "color", expect={"snap": True}))
    return out


PERSP_W = [(1, 2, 4), (4, 1, 2), (2, 4, 1)]


def persp():
    tris = [tri(W0, H0, s, w, c) for s, w, c in zip(SHAPES, PERSP_W, COLORS)]
    return [Scene("persp_depth", W0, H0, "CLIP_COLOR", "depth", tris, "depth"),
            Scene("persp_color", W0, H0, "CLIP_COLOR", "color", tris, "depth")]


def _layer_tris():
    flat = lambda r, g, b: [(Fr(r, 32), Fr(g, 32), Fr(b, 32))] * 3
    far = tri(W0, H0, [(8, 8), (40, 8), (8, 40)], (4, 4, 4), flat(32, 0, 0))            # rhw 1/4, doubled area 1024
    mid = tri(W0, H0, [(8, 8), (24, 8), (8, 40)], (2, 2, 2), flat(0, 32, 0))            # rhw 1/2, 512
    near = tri(W0, H0, [(8, 8), (8, 24), (24, 8)], (1, 1, 1), flat(0, 0, 32))           # rhw 1, 256, the other orientation
    tie_a = tri(W0, H0, [(44, 8), (60, 8), (44, 24)], (2, 2, 2), flat(16, 16, 0))       # the same triangle twice: an exact tie,
    tie_b = tri(W0, H0, [(44, 8), (60, 8), (44, 24)], (2, 2, 2), flat(0, 16, 16))       # the later one wins (:363)
    edge_a = tri(W0, H0, [(8, 44), (24, 44), (24, 60)], (1, 1, 1), flat(8, 0, 24))      # a square split along its diagonal:
    edge_b = tri(W0, H0, [(8, 44), (24, 60), (8, 60)], (2, 2, 2), flat(24, 8, 0))       # every pixel covered exactly once
    return dict(far=far, mid=mid, near=near, tie_a=tie_a, tie_b=tie_b, edge_a=edge_a, edge_b=edge_b)


LAYER_ORDERS = {"layers_near_first": ("near", "mid", "far"), "layers_near_middle": ("far", "near", "mid"),
                "layers_near_last": ("far", "mid", "near")}


def layers():
    t = _layer_tris()
    out = []
    for name, order in LAYER_ORDERS.items():
        names = list(order) + ["tie_a", "tie_b", "edge_a", "edge_b"]
        sc = Scene(name, W0, H0, "CLIP_COLOR", "color", [t[n] for n in names], "color",
                   expect={"tie": (names.index("tie_a"), names.index("tie_b")), "edge_pair": (names.index("edge_a"), names.index("edge_b")),
                           "order": order})
        out.append(sc)
    return out


def clipped():
    """w = 1 unless said.  Pixel 96 of a 64-wide frame is x = 2: an edge from x = 0 (pixel 32) to there crosses X_RIGHT at
    ratio 1/2, one from pixel 48 to pixel 112 at 1/4.  The reference keeps the outside originals (:171), so spi leaves the
    frame and the fans hold zero-area triangles along the clipped edges."""
    C = COLORS
    out = []
    x_half = tri(W0, H0, [(32, 8), (32, 24), (96, 8)], colors=C[0])          # doubled area 1024; both crossing edges at 1/2
    x_quarter = tri(W0, H0, [(48, 34), (48, 50), (112, 34)], colors=C[1])    # both at 1/4
    out.append(Scene("clipped_x_right", W0, H0, "CLIP_COLOR", "color", [x_half, x_quarter], "color", expect={"planes": ["X_RIGHT"]}))
    y_half = tri(W0, H0, [(8, 32), (24, 32), (8, -32)], colors=C[2])         # pixel row -32 is y = 2: Y_UP at 1/2
    y_quarter = tri(W0, H0, [(34, 16), (50, 16), (34, -48)], colors=C[0])    # from row 16 (y = 1/2) to row -48 (y = 5/2): 1/4
    out.append(Scene("clipped_y_up", W0, H0, "CLIP_COLOR", "color", [y_half, y_quarter], "color", expect={"planes": ["Y_UP"]}))
    # Z_FAR: z / w from 1/2 to 3/2 (ratio 1/2) and from 3/4 to 7/4 (1/4) on the second vertex; the whole triangle stays on
    # the screen and is drawn as a fan about its first sorted vertex.  Which vertex is the far one decides whether the fan's
    # doubled areas are powers of two; these two are.
    z_half = tri(W0, H0, SHAPES[0], colors=C[1], z=(H2, Fr(3, 2), H2))
    z_quarter = tri(W0, H0, SHAPES[2], colors=C[2], z=(Fr(3, 4), Fr(7, 4), Fr(3, 4)))
    out.append(Scene("clipped_z_far", W0, H0, "CLIP_COLOR", "color", [z_half, z_quarter], "color", expect={"planes": ["Z_FAR"]}))
    # Z_NEAR: a_w / (a_w - b_w) (:70) is the crossing of w = 0, not of z = 0: the new vertex has w = a_w + t (b_w - a_w) = 0
    # whatever z is, :164 drops it, and the three originals are drawn unclipped.  A ratio of 1/2 or 1/4 would need a vertex
    # with negative w, which is outside X_LEFT or X_RIGHT as well; with w = 1 against 2 (ratio -1) and 2 against 1 (ratio 2) the
    # division, the product and the sum are as exact, and the near plane is the only one crossed.
    n_a = tri(W0, H0, SHAPES[0], (1, 2, 1), C[0], z=(H2, -H2, H2))
    n_b = tri(W0, H0, SHAPES[2], (2, 2, 1), C[2], z=(H2, H2, -H2))
    out.append(Scene("clipped_z_near", W0, H0, "CLIP_COLOR", "depth", [n_a, n_b], "depth", expect={"planes": ["Z_NEAR"], "dropped": True}))
    # two planes: X_RIGHT and Y_UP.  A (0, 0), B (2, 0), C (0, 4) in NDC: AB crosses X_RIGHT at 1/2, AC Y_UP at 1/4, BC
    # X_RIGHT at 1/2 and Y_UP at 1/4: four new vertices, a fan of five.
    two = [vert(W0, H0, (32, 32), color=C[0][0]), vert(W0, H0, (96, 32), color=C[0][1]), vert(W0, H0, (32, -96), color=C[0][2])]
    out.append(Scene("clipped_two_planes", W0, H0, "CLIP_COLOR", "color", [x_half, two, z_half], "color",
                     expect={"planes": ["X_RIGHT", "Y_UP"], "fan": 3}))
    return out


def windowed():
    out = []
    f = flat_w()[0]
    l = layers()[0]
    for base, tag in ((f, "flat_w1"), (l, "layers")):
        # a sub-window with x0 > 0 and y0 > 0 that cuts every triangle; depth entries have stride x1 = 52
        out.append(Scene(f"windowed_sub_{tag}", W0, H0, base.vs, base.ps, base.tris, base.through, window=(12, 52, 10, 50), expect=base.expect))
        # x0 < 0: the window is 64 wide, the depth stride 48, so the last 16 columns of a row share entries with the first 16
        # of the next (renderer.rs:362)
        out.append(Scene(f"windowed_neg_{tag}", W0, H0, base.vs, base.ps, base.tris, base.through, window=(-16, 48, 0, 64),
                         expect=dict(base.expect, shared=True)))
    return out


def _texture(w, h):
    """Bytes whose value / 255 * ambient * 255 stays clear of an integer for ambient 1/2 and 1/4 and every bilinear weight the
    scenes use: odd multiples that land on x.25 / x.5 / x.75 or on integers exactly."""
    vals = [255, 0, 51, 102, 153, 204, 85, 170, 17, 34, 119, 238, 221, 187, 68, 136]
    return [[(vals[(3 * x + 5 * y) % 16], vals[(x + 7 * y + 3) % 16], vals[(5 * x + y + 6) % 16], 255) for x in range(w)] for y in range(h)]


def textured():
    """VS_PHONG under identity matrices: w = 1, so a, b, c are the perspective weights.  The quad's uv runs over [0, 1] x [0, 1]
    over 32 pixels for 4 or 8 texels (pixel centres land on eighths and sixteenths of a texel, and on the borders),
    its normal points at +z and the light sits behind it at -z."""
    out = []
    for name, tw, th in (("textured_4x4", 4, 4), ("textured_4x8", 4, 8)):
        def v(p, uv):
            return [px(p[0], W0), py(p[1], H0), Fr(1, 2), Fr(uv[0]), Fr(uv[1]), 0, 0, 1]
        # corners on half-integer pixels: the pixel centres are uv = k / 32, so they reach the texel borders, u = 1 (column 40)
        # and, v running upwards, v = 0 (row 40)
        a, b = 8 + H2, 40 + H2
        quad = [[v((a, a), (0, 1)), v((b, a), (1, 1)), v((a, b), (0, 0))],
                [v((b, a), (1, 1)), v((b, b), (1, 0)), v((a, b), (0, 0))]]
        # a second, small quad whose uv stays just inside 0 and 1 and on the texel borders: 1/64 .. 63/64
        e, o = Fr(1, 64), Fr(63, 64)
        small = [[v((44, 8), (e, e)), v((60, 8), (o, e)), v((44, 24), (e, o))],
                 [v((60, 8), (o, e)), v((60, 24), (o, o)), v((44, 24), (e, o))]]
        out.append(Scene(name, W0, H0, "PHONG", "phong", quad + small, "color", tex=_texture(tw, th),
                         uniforms=dict(light_pos=(0, 0, -2), light_color=(1, Fr(1, 2), Fr(1, 4)), ambient=Fr(1, 2), specular=0),
                         expect={"texture": (tw, th)}))
    return out


def instanced():
    """flat_w's shapes as VS_PHONG inputs (w = 1 under identity view and projection) under three model matrices that translate
    by whole pixels, so each instance is as exact as the first; the instances overlap at equal depth, where the later one
    wins.  Shaded like `textured`."""
    uvs = [(0, 0), (1, 0), (0, 1)]
    tris = [[[px(p[0], W0), py(p[1], H0), Fr(1, 2), Fr(uv[0]), Fr(uv[1]), 0, 0, 1] for p, uv in zip(s, uvs)] for s in SHAPES]
    moves = [(0, 0), (Fr(2 * 3, W0), Fr(-2 * 2, H0)), (Fr(-2 * 6, W0), Fr(-2 * 5, H0))]      # (3, 2) and (-6, 5) pixels
    return [Scene("instanced_flat_w", W0, H0, "PHONG", "phong", tris, "color", tex=_texture(4, 4), translates=moves,
                  uniforms=dict(light_pos=(0, 0, -2), light_color=(1, Fr(1, 2), Fr(1, 4)), ambient=Fr(1, 2), specular=0))]


FAMILIES = {"instanced": instanced, "flat_w": flat_w, "persp": persp, "layers": layers, "clipped": clipped, "windowed": windowed, "textured": textured}


@functools.lru_cache(maxsize=None)
def all_scenes():
    out = {}
    for fam, gen in FAMILIES.items():
        for sc in gen():
            sc.family = fam
            assert sc.name not in out
            out[sc.name] = sc
    return out


def names(*families):
    return [n for n, s in all_scenes().items() if not families or s.family in families]


@functools.lru_cache(maxsize=None)
def frame(name):
    """The evaluator's frame of a scene, made once and left unchanged; the exact-share condition is asserted here."""
    sc = all_scenes()[name]
    f = sc.evaluate()
    exact, owned = sc.share(f)
    assert exact >= MIN_EXACT and exact >= SHARE * owned, f"{name}: {exact} of {owned} owned pixels are exact through {sc.through}"
    return f


# ---- the evaluator's output as arrays ------------------------------------------------------------------------------------
# Rationals that are f32 values convert to float32 exactly (through a double, which holds every f32).  A Fraction has no
# signed zero, so the comparisons below are by VALUE (numpy's assert_array_equal: -0.0 == 0.0); for every other finite
# value equal values are equal bits.

CLEAR_COLOR = (30, 30, 30, 255)
VS_K = {"CLIP": 0, "CLIP_COLOR": 3, "PHONG": 8}


def _f32(values):
    import numpy as np
    return np.array([float(v.v if isinstance(v, er.X) else v) for v in values], np.float32)


def inputs_f32(sc):
    """The scene's vertex-shader inputs as float32 [ntris, 3, NF]; asserts that nothing was lost."""
    import numpy as np
    a = np.array([[[float(c) for c in v] for v in t] for t in sc.tris], np.float32)
    assert all(Fr(float(a[i, j, k])) == c for i, t in enumerate(sc.tris) for j, v in enumerate(t) for k, c in enumerate(v))
    return a


def texture_u8(sc):
    import numpy as np
    return np.array(sc.tex, np.uint8)


class Expected:
    """What the evaluator says of a frame, as the arrays the oracles and the library deliver: depth [W*H] and ids [W*H] by
    depth entry, color [H, W, 4], the pixel shader's input [W*H, K] (NaN where no fragment owns the entry), the setup list
    (rhw [n,3], spf [n,3,2], spi [n,3,2], ctx [n,3,K]), tris_setup, frag_covered -- and, beside each, the mask of what is
    exact: *_exact are True where no rounding can have touched the value."""

    def __init__(self, f, K, ps):
        import numpy as np
        n = f.width * f.height
        self.W, self.H, self.K = f.width, f.height, K
        self.depth = _f32(f.depth)
        self.ids = np.array(f.ids, np.uint32)
        self.owned = np.zeros(n, bool)
        self.depth_exact = np.ones(n, bool)                 # (the cleared entries are exact)
        self.input = np.full((n, K), np.nan, np.float32)
        self.input_exact = np.zeros(n, bool)
        for i, fr_ in f.frag.items():
            self.owned[i] = True
            self.depth_exact[i] = fr_["depth_exact"]
            if fr_["input"] is not None:
                self.input[i] = _f32(fr_["input"])
                self.input_exact[i] = fr_["input_exact"]
        color = np.zeros((n, 4), np.uint8)
        color[:] = CLEAR_COLOR
        self.color_exact = np.ones(n, bool)
        for off, c in f.color.items():
            color[off] = c
            self.color_exact[off] = f.color_ok[off]
        self.color = color.reshape(f.height, f.width, 4)
        self.color_exact = self.color_exact.reshape(f.height, f.width)
        m = len(f.setup)
        self.rhw = np.array([[float(v.rhw.v) for v in t] for t in f.setup], np.float32).reshape(m, 3)
        self.spf = np.array([[[float(c.v) for c in v.spf] for v in t] for t in f.setup], np.float32).reshape(m, 3, 2)
        self.spi = np.array([[v.spi for v in t] for t in f.setup], np.int32).reshape(m, 3, 2)
        self.ctx = np.array([[[float(c.v) for c in v.ctx] for v in t] for t in f.setup], np.float32).reshape(m, 3, K)
        self.setup_exact = np.array([all(v.ex for v in t) for t in f.setup], bool)
        self.tris_setup, self.frag_covered = f.tris_setup, f.frag_covered


@functools.lru_cache(maxsize=None)
def expected(name):
    sc = all_scenes()[name]
    return Expected(frame(name), VS_K[sc.vs], sc.ps)


def assert_frame(want, sc, depth, ids, color, what, rows=None, inputs=None, setup=None):
    """depth / ids (by depth entry), color [H, W, 4] and, where given, the pixel shader's input [entries, K] and the setup list
    (a structured array with rhw, spf, spi, ctx) against the evaluator.  First the exact values, where equality is the
    assertion; then the rounded ones, where the evaluator follows the Rust text's association.  rows: a bool [H] of the pixel
    rows to compare (a rank's share).  The depth entries of a window are rows of its stride x1, so `rows` goes with whole-frame
    windows only."""
    import numpy as np
    depth, ids = np.asarray(depth, np.float32).ravel(), np.asarray(ids, np.uint32).ravel()
    sel = np.ones(want.W * want.H, bool) if rows is None else np.repeat(np.asarray(rows, bool), want.W)
    selc = sel.reshape(want.H, want.W)
    np.testing.assert_array_equal(ids[sel], want.ids[sel], err_msg=f"{what}: triangle ids")
    m = sel & want.depth_exact
    np.testing.assert_array_equal(depth[m], want.depth[m], err_msg=f"{what}: depth of the exact pixels")
    if sc.ps != "depth":
        m = selc & want.color_exact
        np.testing.assert_array_equal(color[m], want.color[m], err_msg=f"{what}: RGBA8 of the exact pixels")
    if inputs is not None:
        m = sel & want.input_exact
        np.testing.assert_array_equal(np.asarray(inputs)[m], want.input[m], err_msg=f"{what}: pixel-shader input of the exact pixels")
    if setup is not None:
        assert setup.shape[0] == want.tris_setup, f"{what}: {setup.shape[0]} setup triangles, evaluator {want.tris_setup}"
        np.testing.assert_array_equal(setup["spi"], want.spi, err_msg=f"{what}: spi")
        e = want.setup_exact
        np.testing.assert_array_equal(setup["spf"][e], want.spf[e], err_msg=f"{what}: spf of the exact setup triangles")
        np.testing.assert_array_equal(setup["rhw"][e], want.rhw[e], err_msg=f"{what}: rhw of the exact setup triangles")
        np.testing.assert_array_equal(setup["ctx"][e][..., :want.K], want.ctx[e], err_msg=f"{what}: varyings of the exact setup triangles")
    # the rounded class
    np.testing.assert_array_equal(depth[sel], want.depth[sel], err_msg=f"{what}: depth of the rounded pixels")
    if sc.ps != "depth":
        np.testing.assert_array_equal(color[selc], want.color[selc], err_msg=f"{what}: RGBA8 of the rounded pixels")
    if inputs is not None:
        m = sel & want.owned
        np.testing.assert_array_equal(np.asarray(inputs)[m], want.input[m], err_msg=f"{what}: pixel-shader input of the rounded pixels")
    if setup is not None:
        np.testing.assert_array_equal(setup["spf"], want.spf, err_msg=f"{what}: spf of the rounded setup triangles")
        np.testing.assert_array_equal(setup["rhw"], want.rhw, err_msg=f"{what}: rhw of the rounded setup triangles")
        np.testing.assert_array_equal(setup["ctx"][..., :want.K], want.ctx, err_msg=f"{what}: varyings of the rounded setup triangles")
