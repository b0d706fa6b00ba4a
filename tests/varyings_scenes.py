"""Scenes and expected values for the tests of frr_resolve_varyings / frr_readback_varyings (tests/test_varyings_cpu.py,
tests/test_gpu_varyings.py).

The expected value of every entry is the NumPy oracle's: oracle_np.draw(..., debug={}) leaves the interpolated `ctx`
(renderer.rs:368-378) of every z-passing fragment at its depth index, so after a frame debug["ctx"] holds the pixel
shader's input of each entry's final owner, NaN where nothing landed.  Nothing here is computed from the library.

Frames are small (96 x 70: 3 x 3 tiles, partial ones on the right and at the bottom) and computed once per process."""
import functools

import numpy as np

from oracle import oracle_np as onp
from f_renderer_amd import scenes

F = np.float32
W, H = 96, 70
BG = (30, 30, 30, 255)
SENTINEL_BITS = 0xDEADBEEF                                     # a finite float (-6.3e18): what un-owned entries must still hold
SENTINEL = float(np.array([SENTINEL_BITS], np.uint32).view(F)[0])


def clip_color_scene(seed=11, n=640, radius_px=(3.0, 8.0), near_every=53):
    """VS_CLIP_COLOR inputs [n, 3, 7]: small triangles all over the frame (n > 512: three geometry blocks), vertices with
    different w (so the perspective correction is not the identity), random vertex order (both windings), a colour per
    vertex.  The triangles near the frame's edges cross the frustum's side planes: their fans own pixels.  Every
    `near_every`-th triangle has one vertex behind the near plane (z < 0); the reference's near-plane ratio (renderer.rs:70,
    sic) puts that intersection at w = 0, where it is dropped (:164), so these stay single triangles that are not "all
    inside" -- the clipper's other way out."""
    u = scenes.splitmix_u01(0xA11CE000 + seed, 20 * n).reshape(n, 20)
    w_c = 1.0 + 2.0 * u[:, 0]
    cx, cy = 0.93 * (2.0 * u[:, 1] - 1.0), 0.93 * (2.0 * u[:, 2] - 1.0)
    r_ndc = 2.0 * (radius_px[0] + (radius_px[1] - radius_px[0]) * u[:, 3]) / float(W)
    out = np.empty((n, 3, 7), np.float64)
    for k in range(3):
        x = cx + r_ndc * (2.0 * u[:, 4 + 3 * k] - 1.0)
        y = cy + r_ndc * (2.0 * u[:, 5 + 3 * k] - 1.0) * (float(W) / float(H))
        w = w_c * (1.0 + 0.25 * (2.0 * u[:, 6 + 3 * k] - 1.0))
        out[:, k, 0], out[:, k, 1], out[:, k, 2], out[:, k, 3] = x * w, y * w, (0.2 + 0.6 * u[:, 13 + k]) * w, w
        out[:, k, 4:7] = u[:, 16:19] * (0.25 + 0.25 * k) + u[:, 19:20] * 0.2 * k
    near = np.arange(near_every // 2, n, near_every)
    out[near, 1, 2] = -0.4 * out[near, 1, 3]                    # (renderer.rs:123-131: z >= 0 is inside)
    return out.astype(F)


def phong_scene():
    """VS_PHONG inputs (K = 8) through model / view / proj: a coarse displaced sphere under the demo camera."""
    mesh = scenes.displaced_sphere(n=12)
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    model = np.array([1.1, 0, 0, 0, 0, 0.9, 0, 0, 0, 0, 1.0, 0, 0.1, -0.05, 0.0, 1], F)   # column-major: scale + translation
    return mesh, dict(model=model, view=onp.set_look_at(eye, at, up), proj=onp.set_perspective(fovy, aspect, zn, zf), view_pos=eye)


def gouraud_scene():
    mesh = scenes.torus(12, 10)
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    return mesh, dict(view=onp.set_look_at(eye, at, up), proj=onp.set_perspective(fovy, aspect, zn, zf), view_pos=eye)


def indexed_scene(seed=12, n=300):
    """(vertices [V, 7], indices [n, 3]) of a VS_CLIP_COLOR mesh whose corners are scattered over the vertex array."""
    tris = clip_color_scene(seed, n)
    perm = np.argsort(scenes.splitmix_u01(0x1D3000 + seed, 3 * n), kind="stable")
    verts = np.empty((3 * n, 7), F)
    verts[perm] = tris.reshape(-1, 7)
    return verts, perm.reshape(n, 3).astype(np.uint32)


def zero_ps(u, ctx):
    """a pixel shader for frames whose colour nobody looks at (the oracle's PS_PHONG would want a texture)"""
    return np.zeros((ctx.shape[0], 4), F)


class Expected:
    """One oracle frame: color [H, W, 4], depth / tri_id [W * H] by depth index, ctx [W * H, K] (NaN where nothing landed),
    n_emit: triangles each draw emitted."""

    def __init__(self, color, depth, tri_id, ctx, n_emit, window):
        self.color, self.depth, self.tri_id, self.ctx, self.n_emit, self.window = color, depth, tri_id, ctx, n_emit, window
        self.K = ctx.shape[1]
        x0, x1, y0, y1 = window
        self.entries = (y1 - y0) * x1

    def owned(self, first_draw=0):
        """bool [W * H]: entries owned by a triangle of draws first_draw .. last"""
        base = sum(self.n_emit[:first_draw])
        return (self.tri_id != 0xFFFFFFFF) & (self.tri_id >= base)

    def buffer(self, first_draw=0, start=None):
        """What a buffer that held `start` (default: the sentinel everywhere) holds after the resolves of draws
        first_draw .. last: [entries, K] float32."""
        out = np.full((self.entries, self.K), SENTINEL, F) if start is None else np.array(start, F).reshape(self.entries, self.K)
        o = self.owned(first_draw)[:self.entries]
        out[o] = self.ctx[:self.entries][o]
        return out


def render(draws, ps=onp.PS_COLOR, window=None, clear_depth=0.0):
    """draws: [(vs_inputs, vs_id, oracle_np.Uniforms)] of one frame, in order -> Expected"""
    color = np.zeros((H, W, 4), np.uint8)
    color[:] = BG
    depth = np.full(W * H, clear_depth, F)
    tri_id = np.full(W * H, 0xFFFFFFFF, np.uint32)
    debug, n_emit = {}, []
    for vin, vs, u in draws:
        setup, _ = onp.draw(W, H, vin, vs, ps, u, color, depth, tri_id, window=window, tri_id_base=sum(n_emit), debug=debug)
        n_emit.append(len(setup))
    K = onp.VS_K[draws[0][1]]
    ctx = debug.get("ctx", np.full((W * H, K), np.nan, F))
    return Expected(color, depth, tri_id, ctx, n_emit, window or (0, W, 0, H))


def emission_meta(vin, vs, u):
    """per emitted triangle of a draw: (input triangle, is a fan triangle, corners 1 / 2 swapped -- renderer.rs:300-312)"""
    vin = np.asarray(vin, F).reshape(-1, 3, onp.VS_NF[vs])
    inp, fan, swapped = [], [], []
    for t in range(vin.shape[0]):
        tris = onp.geometry_processing(W, H, vin[t], vs, u)
        for tri in tris:
            with np.errstate(all="ignore"):
                d1, d2 = tri[1]["ndc"] - tri[0]["ndc"], tri[2]["ndc"] - tri[0]["ndc"]
                nz = F(d1[0] * d2[1]) - F(d2[0] * d1[1])
            inp.append(t); fan.append(len(tris) > 1); swapped.append(bool(nz > 0.0))
    return np.array(inp), np.array(fan), np.array(swapped)


def check_scene(e, vin, vs, u):
    """The conditions a scene has to meet on the oracle's own output before a test may use it: a test that compares
    nothing cannot pass."""
    inp, fan, swapped = emission_meta(vin, vs, u)
    assert len(inp) == e.n_emit[0]
    own = e.owned()
    owners = np.unique(e.tri_id[own])
    assert len(owners) >= 60, len(owners)
    assert fan[owners].any(), "no fan triangle owns a pixel"
    nblocks = (np.asarray(vin).reshape(-1, 3, onp.VS_NF[vs]).shape[0] + 255) // 256
    assert nblocks >= 3 and set(inp[owners] // 256) == set(range(nblocks)), "a geometry block owns nothing"
    assert swapped[owners].any() and (~swapped[owners]).any(), "one winding only"
    unowned = 1.0 - own.mean()
    assert 0.05 <= unowned <= 0.60, unowned
    assert not np.isnan(e.ctx[own]).all(axis=1).any()           # every owned entry has its varyings
    return dict(owners=len(owners), fan_owners=int(fan[owners].sum()), unowned=float(unowned))


@functools.lru_cache(maxsize=None)
def basic():
    """the K = 3 scene every path test draws: (inputs, Expected of one PS_COLOR frame)"""
    tris = clip_color_scene()
    return tris, render([(tris, onp.VS_CLIP_COLOR, onp.Uniforms())])


@functools.lru_cache(maxsize=None)
def second():
    """a second K = 3 mesh (multi-draw, two frames in flight)"""
    return clip_color_scene(seed=23, n=520, radius_px=(4.0, 10.0), near_every=61)


@functools.lru_cache(maxsize=None)
def two_draws():
    a, b = basic()[0], second()
    return render([(a, onp.VS_CLIP_COLOR, onp.Uniforms()), (b, onp.VS_CLIP_COLOR, onp.Uniforms())])


@functools.lru_cache(maxsize=None)
def second_alone():
    return render([(second(), onp.VS_CLIP_COLOR, onp.Uniforms())])


SUB_WINDOW = (9, 83, 5, 61)                                      # x0 > 0, y0 > 0: depth stride x1 = 83, partial tiles on both sides


@functools.lru_cache(maxsize=None)
def sub_window():
    return render([(basic()[0], onp.VS_CLIP_COLOR, onp.Uniforms())], window=SUB_WINDOW)


@functools.lru_cache(maxsize=None)
def phong():
    mesh, kw = phong_scene()
    return mesh, kw, render([(mesh, onp.VS_PHONG, onp.Uniforms(**kw))], ps=zero_ps)


@functools.lru_cache(maxsize=None)
def gouraud():
    mesh, kw = gouraud_scene()
    return mesh, kw, render([(mesh, onp.VS_GOURAUD, onp.Uniforms(**kw))])


@functools.lru_cache(maxsize=None)
def indexed():
    verts, idx = indexed_scene()
    return verts, idx, render([(verts[idx], onp.VS_CLIP_COLOR, onp.Uniforms())])


# ---- user shaders (frr_shader_register) with K = 16 and K = 1 ----------------------------------------------------------
# Every varying is a signed copy of one of the three colour inputs.  The clipper (a + (b - a) * t, renderer.rs:88-91) and
# the interpolation (:374-378) treat each varying by itself, and IEEE negation commutes with +, -, *: varying k of the
# user shader is, bit for bit, SIGN[k] * varying SRC[k] of VS_CLIP_COLOR on the same inputs -- the oracle's value.
WIDE_SRC = (0, 1, 2, 2, 0, 1, 1, 2, 0, 2, 1, 0, 0, 0, 2, 1)
WIDE_SIGN = (1, 1, 1, -1, -1, -1, 1, -1, 1, 1, -1, 1, -1, 1, -1, 1)
NARROW_SRC, NARROW_SIGN = (1,), (-1,)


def _user_source(src, sign):
    body = " ".join(f"ctx[{k}] = {'-' if sg < 0 else ''}in[{4 + s}];" for k, (s, sg) in enumerate(zip(src, sign)))
    return ("__device__ void frr_user_vs(const frr::DevUniforms &u, const float *in, float pos[4], float *ctx)\n"
            "{ pos[0] = in[0]; pos[1] = in[1]; pos[2] = in[2]; pos[3] = in[3]; " + body + " }\n"
            "__device__ void frr_user_ps(const frr::DevUniforms &u, const float *ctx, float out[4], const float *u8lut)\n"
            "{ out[0] = ctx[0]; out[1] = 0.0f; out[2] = 0.0f; out[3] = 1.0f; }\n")


WIDE_SHADER = _user_source(WIDE_SRC, WIDE_SIGN)                 # K = 16: 64-byte entries, 16-byte stores
NARROW_SHADER = _user_source(NARROW_SRC, NARROW_SIGN)           # K = 1: the scalar-store path


def user_expected(e, src, sign):
    """the buffer a user shader above leaves on the frame `e` of the same inputs under VS_CLIP_COLOR"""
    b = e.buffer()
    out = np.full((e.entries, len(src)), SENTINEL, F)
    o = e.owned()[:e.entries]
    out[o] = b[o][:, list(src)] * np.array(sign, F)
    return out


def assert_bits_equal(got, want, err_msg=""):
    """float32 arrays as bit patterns; two NaNs are equal whatever their payload (which quiet NaN an operation gives is a
    property of the machine that ran it)"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (got.shape, want.shape)
    both = np.isnan(got) & np.isnan(want)
    np.testing.assert_array_equal(np.where(both, 0, got.view(np.uint32)), np.where(both, 0, want.view(np.uint32)), err_msg=err_msg)
