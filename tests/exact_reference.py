"""A rational evaluator of the reference's draw loop (TEST INFRASTRUCTURE ONLY; no tests in this file).

Third restatement of f_renderer/src/renderer.rs, written to stand apart from the other two: it imports nothing from oracle/
or f_renderer_amd/, uses no float type at all, and computes every value as a fractions.Fraction.  Every operation the
reference performs in f32 goes through ONE helper, rn32, which rounds the exact rational result to the nearest f32 (ties to
even) from the Fraction's integers and says whether it had to round.  A value (class X) carries `ex`: no operation on the way
to it rounded.  An exact operation does not round, so operand association, FMA contraction and glam's internals cannot change
its result: on values with ex == True any correct reading of the reference's formulas gives the same bits, and those bits are
what the scenes of tests/exact_scenes.py pin the two oracles and the library to.

Where a value has rounded, the evaluator follows the Rust text's association (left to right; glam's documented ones for
Vec * f32 and the sum of products), so it can still be compared, but there an equal result is evidence and not proof.

Two results that are exact although an operand is not are flagged exact, because no rounding can reach them:
  max(dot, 0) of a dot product that is negative by a wide margin (phong.rs:138), and the product of anything finite with an
  exact 0 (phong.rs:144 with specular_strength == 0).
`robust` on a colour says the bytes cannot depend on rounding although the channel values rounded (texel / 255): the unrounded
rational value of every channel times 255 stays at least BYTE_MARGIN away from an integer, far more than a handful of
half-ulp errors can move it.

perturb: a set of names that each misread one formula on purpose (tests/test_exact_cpu.py's sensitivity test):
  "swap_ab"    the weights a and b are paired with each other's vertex (renderer.rs:360, :370-371)
  "no_half"    px = (cx, cy) without the + 0.5 (renderer.rs:325)
  "near_plus"  the near plane's ratio is a_w / (a_w + b_w) (renderer.rs:70)
"""
import math
from fractions import Fraction as Fr

ZERO, ONE, HALF = Fr(0), Fr(1), Fr(1, 2)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
ANGLE_MARGIN = 1.0e-3            # rad: the closest two sort keys, or a key and the 0 / 2 pi cut, may come
DOT_MARGIN = Fr(1, 16)           # a cosine below -DOT_MARGIN is negative whatever normalize rounds to
BYTE_MARGIN = Fr(1, 64)          # distance of an unrounded channel * 255 from an integer that makes its byte robust
NO_ID = 0xFFFFFFFF


class Inexact(Exception):
    """The scene asks for something the evaluator refuses to decide (a sort too close to call, a value outside the normal
    f32 range, a shader term the scenes were not meant to reach)."""


# ---- the one rounding helper ---------------------------------------------------------------------------------------------

def rn32(x):
    """(nearest f32 to the rational x as a Fraction, ties to even; whether x was an f32 already).  Works on the integers of
    the Fraction: no float(), no double rounding.  Zero is exact; anything else outside the normal range raises."""
    x = Fr(x)
    if x == 0:
        return ZERO, True
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()                 # 2^e <= n/d < 2^(e+1), after the correction below
    if (n << -e if e < 0 else n) < (d << e if e > 0 else d):
        e -= 1
    if e < -126 or e > 127:
        raise Inexact(f"{x} is outside the normal f32 range")
    s = 23 - e                                          # q = n/d * 2^s lies in [2^23, 2^24)
    num, den = (n << s, d) if s >= 0 else (n, d << -s)
    q, r = divmod(num, den)
    exact = r == 0
    if 2 * r > den or (2 * r == den and q & 1):
        q += 1
    if q == 1 << 24 and e == 127:
        raise Inexact(f"{x} rounds past the largest f32")
    v = Fr(q << -s, 1) if s < 0 else Fr(q, 1 << s)
    return (-v if x < 0 else v), exact


def is_f32(x):
    return rn32(x)[1]


def f32_bits(x):
    """The 32-bit pattern of a rational that is an f32 (0 is +0.0)."""
    x = Fr(x)
    if x == 0:
        return 0
    v, exact = rn32(x)
    assert exact, x
    n, d = abs(v.numerator), v.denominator
    e = n.bit_length() - d.bit_length()
    if (n << -e if e < 0 else n) < (d << e if e > 0 else d):
        e -= 1
    m = abs(v) / (Fr(2) ** e)                           # in [1, 2)
    frac = (m - 1) * (1 << 23)
    assert frac.denominator == 1
    return (0x80000000 if x < 0 else 0) | ((e + 127) << 23) | int(frac)


class X:
    """An f32 value as a Fraction, with `ex`: nothing on the way to it rounded."""
    __slots__ = ("v", "ex")

    def __init__(self, v, ex=True):
        self.v, self.ex = v, ex

    @staticmethod
    def lit(v):
        """A literal or an input: has to be an f32 as it stands."""
        v = Fr(v)
        if not is_f32(v):
            raise Inexact(f"{v} is not an f32")
        return X(v, True)

    def _op(self, v, other):
        r, exact = rn32(v)
        return X(r, exact and self.ex and other.ex)

    def __add__(self, o):
        return self._op(self.v + o.v, o)

    def __sub__(self, o):
        return self._op(self.v - o.v, o)

    def __mul__(self, o):
        if (self.v == 0 and self.ex) or (o.v == 0 and o.ex):
            return X(ZERO, True)                        # an exact zero times anything finite: no rounding can reach it
        return self._op(self.v * o.v, o)

    def __truediv__(self, o):
        if o.v == 0:
            raise Inexact("division by zero")
        return self._op(self.v / o.v, o)

    def __neg__(self):
        return X(-self.v, self.ex)

    def __abs__(self):
        return X(abs(self.v), self.ex)

    def __repr__(self):
        return f"X({self.v}{'' if self.ex else ' ~'})"


def xs(values):
    return [v if isinstance(v, X) else X.lit(v) for v in values]


def all_exact(values):
    return all(v.ex for v in values)


def as_i32(x):
    """Rust's `as i32` of a finite f32: truncate toward zero, saturate (renderer.rs:233-234)."""
    t = int(x.v)                                        # int(Fraction) truncates toward zero
    return max(I32_MIN, min(I32_MAX, t))


C_HALF, C_ONE, C_255 = X(HALF), X(ONE), X(Fr(255))
EPSILON = X(rn32(Fr(1, 100000))[0])                     # renderer.rs:44: the literal 1.0e-5 as an f32


# ---- geometry: renderer.rs:96-267 ----------------------------------------------------------------------------------------

class Vtx:
    """renderer.rs:387-394"""
    __slots__ = ("pos", "ctx", "rhw", "spf", "spi", "new")

    def __init__(self, pos, ctx, new=False):
        self.pos, self.ctx, self.new = pos, ctx, new
        self.rhw, self.spf, self.spi = None, None, None

    @property
    def ex(self):
        return self.rhw.ex and all_exact(self.spf) and all_exact(self.ctx)


PLANES = ("X_LEFT", "X_RIGHT", "Y_UP", "Y_DOWN", "Z_NEAR", "Z_FAR")          # :123-131, the order of PLANE_LIST


def insides(plane, p):
    """renderer.rs:46-58"""
    x, y, z, w = (c.v for c in p)
    return {"X_LEFT": x >= -w, "X_RIGHT": x <= w, "Y_UP": y <= w, "Y_DOWN": y >= -w, "Z_FAR": z <= w, "Z_NEAR": z >= 0}[plane]


def intersect_ratio(plane, a, b, perturb=()):
    """renderer.rs:60-73, each sum taken left to right as written"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    if plane == "X_LEFT":
        return -(ax + aw) / (((bw + bx) - ax) - aw)
    if plane == "X_RIGHT":
        return (aw - ax) / (((aw - bw) - ax) + bx)
    if plane == "Y_UP":
        return (aw - ay) / (((aw - bw) - ay) + by)
    if plane == "Y_DOWN":
        return -(ay + aw) / (((bw + by) - aw) - ay)
    if plane == "Z_FAR":
        return (aw - az) / (((aw - bw) - az) + bz)
    if "near_plus" in perturb:
        return aw / (aw + bw)
    return aw / (aw - bw)                               # Z_NEAR, :70


def vertex_intersect(a, b, ratio):
    """renderer.rs:88-91: a.pos + ratio * (b.pos - a.pos); a.context + (b.context - a.context) * ratio"""
    pos = [pa + ratio * (pb - pa) for pa, pb in zip(a.pos, b.pos)]
    ctx = [ca + (cb - ca) * ratio for ca, cb in zip(a.ctx, b.ctx)]
    return Vtx(pos, ctx, new=True)


def sort_order(verts):
    """renderer.rs:180-218.  The order the angle sort gives, computed exactly: the centroid is rational, a vertex's place
    is its half plane about the centroid and then the sign of a cross product.  Refused (Inexact) where two angles come
    closer than ANGLE_MARGIN or an angle comes that close to the 0 / 2 pi cut: the f32 roundings of the centroid, of the
    differences and of atan2 are orders of magnitude smaller than that, so they cannot change this order."""
    n = len(verts)
    cx = sum(v.pos[0].v for v in verts) / n
    cy = sum(v.pos[1].v for v in verts) / n
    d = [(v.pos[0].v - cx, v.pos[1].v - cy) for v in verts]
    if any(x == 0 and y == 0 for x, y in d):
        raise Inexact("a vertex on the centroid has no angle")

    def half(p):                                         # 0: angle in [0, pi), 1: angle in [pi, 2 pi)
        return 0 if (p[1] > 0 or (p[1] == 0 and p[0] > 0)) else 1

    import functools

    def cmp(i, j):
        a, b = d[i], d[j]
        if half(a) != half(b):
            return half(a) - half(b)
        cr = a[0] * b[1] - a[1] * b[0]                   # > 0: b is counter-clockwise of a, so a's angle is smaller
        return -1 if cr > 0 else (1 if cr < 0 else 0)
    order = sorted(range(n), key=functools.cmp_to_key(cmp))
    ang = [math.atan2(float(d[i][1]), float(d[i][0])) % (2 * math.pi) for i in order]
    if ang[0] < ANGLE_MARGIN or 2 * math.pi - ang[-1] < ANGLE_MARGIN or any(b - a < ANGLE_MARGIN for a, b in zip(ang, ang[1:])):
        raise Inexact(f"sort keys too close to call: {ang}")
    return order


def geometry_processing(width, height, vs_out, perturb=()):
    """renderer.rs:96-267 for one input triangle.  vs_out: three (clip position [4], context [K]) pairs, the vertex shader's
    outputs (:116), as f32-exact rationals.  Returns the list of setup triangles ([Vtx; 3]) in emission order."""
    verts = [Vtx(xs(p), xs(c)) for p, c in vs_out]                        # :113-121
    if any(v.pos[3].v == 0 for v in verts):
        return []                                                         # :117-119
    inside = [[insides(pl, v.pos) for pl in PLANES] for v in verts]       # :138-148
    valid = []
    if not all(all(r) for r in inside):
        for i in range(3):                                                # :152-170
            for j in range(i + 1, 3):
                for k, pl in enumerate(PLANES):
                    if inside[i][k] != inside[j][k]:
                        t = intersect_ratio(pl, verts[i].pos, verts[j].pos, perturb)
                        nv = vertex_intersect(verts[i], verts[j], t)
                        if abs(nv.pos[3]).v > EPSILON.v:                  # :164
                            valid.append(nv)
    valid.extend(verts)                                                   # :171 (or :173)
    if len(valid) < 3:
        return []
    valid = [valid[i] for i in sort_order(valid)]                         # :180-218
    wf, hf = X.lit(width), X.lit(height)
    for v in valid:                                                       # :220-235
        v.rhw = C_ONE / v.pos[3]
        v.pos = [c * v.rhw for c in v.pos]
        v.spf = [((v.pos[0] + C_ONE) * wf) * C_HALF, ((C_ONE - v.pos[1]) * hf) * C_HALF]
        v.spi = [as_i32(v.spf[0] + C_HALF), as_i32(v.spf[1] + C_HALF)]
    if len(valid) == 3:
        return [valid]                                                    # :237-243
    tris = []
    last = len(valid) - 1
    while last > 3:                                                       # :249-254
        tris.append([valid[0], valid[last - 1], valid[last]])
        last -= 1
    tris.append([valid[0], valid[2], valid[3]])                           # :256-259
    tris.append([valid[0], valid[1], valid[2]])                           # :261-264
    return tris


# ---- shading: renderer.rs:6-14, :516-538, phong.rs:133-154 ----------------------------------------------------------------

def vec4_to_u8(rgba):
    """renderer.rs:6-14: (v * 255.0).clamp(0.0, 255.0) as u8 -> (bytes, every product exact)"""
    out, exact = [], True
    for c in rgba:
        v = c * C_255
        exact = exact and v.ex
        out.append(int(min(max(v.v, ZERO), Fr(255))))
    return out, exact


class Texture:
    """A FrameBuffer used as a texture (renderer.rs:411-416): rows of [r, g, b, a] bytes."""

    def __init__(self, rows):
        self.rows = [[tuple(int(b) for b in px) for px in row] for row in rows]
        self.height, self.width = len(self.rows), len(self.rows[0])
        self.reached = set()                                              # the (x, y) texels sample_2d has read

    def get_pixel(self, x, y):                                            # :506-514
        if not (0 <= x < self.width and 0 <= y < self.height):
            raise Inexact(f"texel ({x}, {y}) outside the texture: the reference would read another row or panic")
        self.reached.add((x, y))
        return self.rows[y][x]


def sample_2d(tex, uv):
    """renderer.rs:516-538 -> ([4] X, [4] unrounded rationals).  y1 and y2 are clamped by the WIDTH (:523, :525)."""
    x = uv[0] * X.lit(tex.width)
    y = uv[1] * X.lit(tex.height)
    if x.v < 0 or y.v < 0:
        raise Inexact("negative texture coordinate")
    a = X(x.v - int(x.v), x.ex)                                           # fract() never rounds
    b = X(y.v - int(y.v), y.ex)
    x1 = min(max(int(x.v), 0), tex.width - 1)
    y1 = min(max(int(y.v), 0), tex.width - 1)                             # sic
    x2 = min(x1 + 1, tex.width - 1)
    y2 = min(y1 + 1, tex.width - 1)                                       # sic
    oma, omb = C_ONE - a, C_ONE - b
    terms = [(tex.get_pixel(x1, y1), oma, omb), (tex.get_pixel(x1, y2), oma, b),
             (tex.get_pixel(x2, y1), a, omb), (tex.get_pixel(x2, y2), a, b)]
    out, ideal = [], []
    for ch in range(4):
        cs = [((X.lit(t[ch]) / C_255) * wa) * wb for t, wa, wb in terms]   # :19-22, :527-530
        out.append(((cs[0] + cs[1]) + cs[2]) + cs[3])                      # :533-536
        ideal.append(sum(Fr(t[ch], 255) * wa.v * wb.v for t, wa, wb in terms))
    return out, ideal


class Uniforms:
    """What the pixel shaders read.  light_pos, light_color, ambient and specular stand for phong.rs:128-132's constants."""

    def __init__(self, tex=None, light_pos=(0, 0, 0), light_color=(1, 1, 1), ambient=Fr(1, 2), specular=0):
        self.tex = tex
        self.light_pos, self.light_color = xs(light_pos), xs(light_color)
        self.ambient, self.specular = X.lit(ambient), X.lit(specular)


def pixel_shader(ps, u, ctx):
    """-> ([4] X, robust).  "color": the varyings as RGB, alpha 1.  "phong": phong.rs:133-154 as far as the scenes go -- the
    diffuse term has to be a robust zero and specular_strength an exact zero, anything else is refused."""
    if ps == "color":
        return [ctx[0], ctx[1], ctx[2], C_ONE], all_exact(ctx[:3])
    assert ps == "phong", ps
    uv, normal, wpos = ctx[0:2], ctx[2:5], ctx[5:8]
    ambient = [c * u.ambient for c in u.light_color]                      # :134
    # :136-138.  normalize() scales both vectors by positive numbers, so the sign of the dot product is that of the
    # unnormalised one; its cosine, computed in rationals, has to be far enough below zero that no rounding turns it.
    ld = [l.v - p.v for l, p in zip(u.light_pos, wpos)]
    nn, ll = sum(n.v * n.v for n in normal), sum(l * l for l in ld)
    dot = sum(n.v * l for n, l in zip(normal, ld))
    if nn == 0 or ll == 0 or dot >= 0 or dot * dot < DOT_MARGIN * DOT_MARGIN * nn * ll:
        raise Inexact("the scenes keep the light behind the surface: max(dot, 0) must be a robust zero")
    diff = X(ZERO, True)
    diffuse = [diff * c for c in u.light_color]                           # :139
    if u.specular.v != 0:
        raise Inexact("the scenes keep specular_strength at 0")
    specular = [X(ZERO, True) for _ in range(3)]                          # :143-144: 0 * spec * LIGHT_COLOR
    light = [(a + d) + s for a, d, s in zip(ambient, diffuse, specular)]  # :153
    tex, ideal = sample_2d(u.tex, uv)                                     # :146-151
    rgba = [tex[0] * light[0], tex[1] * light[1], tex[2] * light[2], tex[3] * C_ONE]
    ideal = [ideal[0] * light[0].v, ideal[1] * light[1].v, ideal[2] * light[2].v, ideal[3]]
    robust = all_exact(uv) and all_exact(light)
    for r, i in zip(rgba, ideal):
        q = i * 255
        lo = q - int(q)
        near = min(lo, 1 - lo) if 0 < q < 255 else (abs(q) if q <= 0 else q - 255)
        if not r.ex and (near < BYTE_MARGIN or int(min(max(q, ZERO), Fr(255))) != int(min(max((r * C_255).v, ZERO), Fr(255)))):
            robust = False
    return rgba, robust


# ---- raster: renderer.rs:269-384 -----------------------------------------------------------------------------------------

def is_top_left(a, b):
    """renderer.rs:26-29"""
    return (a[1] == b[1] and a[0] < b[0]) or a[1] > b[1]


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


class Frame:
    """The colour, depth and (auxiliary) triangle-id buffers of one frame (phong.rs:207-208), and what the evaluator knows
    about each entry: `frag`[index] of the fragment that owns a depth entry is a dict with the weights, the pixel shader's
    input, the colour and the exactness flags."""

    def __init__(self, width, height, clear_depth=0):
        self.width, self.height = width, height
        self.depth = [X.lit(clear_depth)] * (width * height)
        self.ids = [NO_ID] * (width * height)
        self.color = {}                                  # linear pixel offset (y * width + x) -> [r, g, b, a]
        self.color_ok = {}                               # ... -> the bytes cannot depend on a rounding
        self.frag = {}
        self.setup = []
        self.tris_setup = 0
        self.frag_covered = 0

    def rasterization(self, wr, hr, tri, ps, u, tri_id, perturb=()):
        """renderer.rs:285-381"""
        xs_, ys_ = [v.spi[0] for v in tri], [v.spi[1] for v in tri]
        min_x = max_x = _clamp(xs_[0], wr[0], wr[1])                      # :285-298
        min_y = max_y = _clamp(ys_[0], hr[0], hr[1])
        for k in (1, 2):
            min_x, max_x = _clamp(min(min_x, xs_[k]), *wr), _clamp(max(max_x, xs_[k]), *wr)
            min_y, max_y = _clamp(min(min_y, ys_[k]), *hr), _clamp(max(max_y, ys_[k]), *hr)
        v01 = [b - a for a, b in zip(tri[0].pos, tri[1].pos)]             # :300-305
        v02 = [b - a for a, b in zip(tri[0].pos, tri[2].pos)]
        nz = v01[0] * v02[1] - v02[0] * v01[1]
        vtx = [tri[0], tri[2], tri[1]] if nz.v > 0 else list(tri)         # :307-312
        p = [v.spi for v in vtx]
        bias = [0 if is_top_left(p[0], p[1]) else 1, 0 if is_top_left(p[1], p[2]) else 1, 0 if is_top_left(p[2], p[0]) else 1]
        setup_exact = all(v.ex for v in vtx)
        half = ZERO if "no_half" in perturb else HALF
        for cy in range(min_y, max_y):                                    # :322-381
            index_y = cy - hr[0]
            for cx in range(min_x, max_x):
                index_x = cx - wr[0]
                e01 = -(cx - p[0][0]) * (p[1][1] - p[0][1]) + (cy - p[0][1]) * (p[1][0] - p[0][0])
                e12 = -(cx - p[1][0]) * (p[2][1] - p[1][1]) + (cy - p[1][1]) * (p[2][0] - p[1][0])
                e20 = -(cx - p[2][0]) * (p[0][1] - p[2][1]) + (cy - p[2][1]) * (p[0][0] - p[2][0])
                if e01 < bias[0] or e12 < bias[1] or e20 < bias[2]:
                    continue
                self.frag_covered += 1
                px = [X.lit(cx) + X(half), X.lit(cy) + X(half)]           # :325
                s = [[v.spf[0] - px[0], v.spf[1] - px[1]] for v in vtx]   # :343-345

                def perp(m, n):                                           # glam: self.x * rhs.y - self.y * rhs.x
                    return abs(m[0] * n[1] - m[1] * n[0])
                a, b, c = perp(s[1], s[2]), perp(s[2], s[0]), perp(s[0], s[1])   # :347-349
                abc = (a, b, c)
                ssum = (a + b) + c                                        # :351
                if ssum.v == 0:
                    continue
                inv = C_ONE / ssum
                a, b, c = a * inv, b * inv, c * inv                       # :356-358
                wa, wb = (b, a) if "swap_ab" in perturb else (a, b)
                rhw = (vtx[0].rhw * wa + vtx[1].rhw * wb) + vtx[2].rhw * c   # :360
                index = index_y * wr[1] + index_x                         # :362
                if not 0 <= index < len(self.depth):
                    raise Inexact("depth index outside the buffer: the reference would panic")
                if rhw.v < self.depth[index].v:                           # :363
                    continue
                self.depth[index] = rhw                                   # :366
                self.ids[index] = tri_id
                f = dict(pixel=(cx, cy), tri=tri_id, vtx=vtx, abc=abc, s=ssum, weights=(a, b, c), rhw=rhw, depth_exact=rhw.ex,
                         setup_exact=setup_exact, input=None, rgba=None, color_exact=False, robust=False)
                self.frag[index] = f
                if ps == "depth":
                    continue
                w = C_ONE / (rhw if rhw.v != 0 else C_ONE)                # :368
                c0, c1, c2 = (vtx[0].rhw * wa) * w, (vtx[1].rhw * wb) * w, (vtx[2].rhw * c) * w   # :370-372
                inp = [(i0 * c0 + i1 * c1) + i2 * c2 for i0, i1, i2 in zip(vtx[0].ctx, vtx[1].ctx, vtx[2].ctx)]   # :378
                rgba, robust = pixel_shader(ps, u, inp)                   # :380
                off = index_y * self.width + index_x                      # :381, set_pixel's offset / 4 (:498)
                if not 0 <= off < self.width * self.height or index_x < 0 or index_y < 0:
                    raise Inexact("pixel outside the FrameBuffer: the reference would panic")
                byts, q_exact = vec4_to_u8(rgba)
                self.color[off] = byts
                self.color_ok[off] = q_exact or robust
                f.update(input=inp, rgba=byts, input_exact=all_exact(inp), color_exact=q_exact, robust=robust, offset=off)

    def draw(self, tris_vs_out, ps, u=None, window=None, perturb=()):
        """Loops A and B of phong.rs:319-381 over a list of input triangles (each three vertex-shader outputs)."""
        wr, hr = ((0, self.width), (0, self.height)) if window is None else (tuple(window[0:2]), tuple(window[2:4]))
        new = []
        for t in tris_vs_out:
            new.extend(geometry_processing(self.width, self.height, t, perturb))
        base = self.tris_setup
        for i, tri in enumerate(new):
            self.rasterization(wr, hr, tri, ps, u, base + i, perturb)
        self.setup.extend(new)
        self.tris_setup += len(new)
        return new

    # -- what the tests compare --
    def exact_entries(self, through):
        """The depth entries whose fragment is exact through `through`: "depth", "input" or "color" (robust bytes count)."""
        out = []
        for i, f in self.frag.items():
            if self.ids[i] != f["tri"]:
                continue
            ok = f["depth_exact"]
            if through == "input":
                ok = ok and f["input_exact"]
            elif through == "color":
                ok = ok and (f["color_exact"] or f["robust"])
            if ok:
                out.append(i)
        return sorted(out)

    def owned_entries(self):
        return sorted(i for i, f in self.frag.items())
