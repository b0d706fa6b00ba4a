"""Scenes and expected images for the tests of frr_shade_varyings / frr_shade_varyings_host (tests/test_shade_cpu.py,
tests/test_gpu_shade.py, built on tests/varyings_scenes.py).

Every expected value is the NumPy oracle's.  The expected colour of a frame: start from the frame the oracle leaves (the
background where nothing landed, whatever the test put there otherwise); for every entry the oracle's tri_id says is drawn
and in the range of ids, the pixel at window-local (i % x1, i // x1) becomes
oracle_np.quantize(oracle_np.pixel_shader(ps, u, ctx[i])), ctx being the oracle's interpolated varyings at that entry.
Nothing here is computed from the library.  Frames are 96 x 70 unless stated, and computed once per process."""
import functools

import numpy as np

from oracle import oracle_np as onp
from f_renderer_amd import scenes
from . import varyings_scenes as V

F = np.float32
W, H = V.W, V.H
EVERY = (0, 0xFFFFFFFF)
SNAN_BITS = 0x7FA0DEAD                                          # a signalling NaN: what entries of undrawn pixels hold in a caller-made buffer


# ---- textures (height >= width: frr_texture_upload) and lights ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def textures():
    a = scenes.checker_texture(64, 8)
    b = np.ascontiguousarray(np.roll(scenes.checker_texture(32, 4), 5, axis=1)[:, :, [2, 1, 0, 3]])
    u = scenes.splitmix_u01(0x7E87, 48 * 40 * 4).reshape(48, 40, 4)
    c = np.ascontiguousarray((u * 255.0).astype(np.uint8))       # 40 wide, 48 high: noise, alpha included
    return a, b, c


LIGHTS = (                                                       # test 2: three relights (the first is the frame's own)
    dict(),
    dict(light_pos=(-0.7, 1.9, 1.1), view_pos=(0.3, -0.4, 2.5), specular=0.9),
    dict(light_pos=(2.0, -1.0, 0.5), light_color=(0.9, 0.7, 1.0), ambient=0.25),
)


def oracle_uniforms(kw, tex=None, **light):
    """oracle_np.Uniforms of a scene's matrices (kw: model / view / proj / view_pos) with a texture and a light"""
    d = dict(kw)
    d.update(light)
    return onp.Uniforms(tex=tex, **d)


def gpu_uniforms(kw, **light):
    """the same as keyword arguments of Renderer.set_uniforms"""
    d = dict(kw)
    d.update(light)
    if "ambient" in d:
        d["ambient_strength"] = d.pop("ambient")
    if "specular" in d:
        d["specular_strength"] = d.pop("specular")
    return d


# ---- frames ---------------------------------------------------------------------------------------------------------------
def render(draws, ps=onp.PS_COLOR, window=None, size=(W, H), bg=V.BG):
    """varyings_scenes.render for any frame size: draws [(vs_inputs, vs_id, Uniforms)] of one frame, in order -> V.Expected"""
    w, h = size
    color = np.zeros((h, w, 4), np.uint8)
    color[:] = bg
    depth = np.zeros(w * h, F)
    tri_id = np.full(w * h, 0xFFFFFFFF, np.uint32)
    debug, n_emit = {}, []
    for vin, vs, u in draws:
        setup, _ = onp.draw(w, h, vin, vs, ps, u, color, depth, tri_id, window=window, tri_id_base=sum(n_emit), debug=debug)
        n_emit.append(len(setup))
    K = onp.VS_K[draws[0][1]]
    ctx = debug.get("ctx", np.full((w * h, K), np.nan, F))
    return V.Expected(color, depth, tri_id, ctx, n_emit, window or (0, w, 0, h))


def in_range(tri_id, ids):
    """bool per entry: drawn, and id - first < count (unsigned)"""
    first, count = ids
    return (tri_id != 0xFFFFFFFF) & (((tri_id.astype(np.int64) - int(first)) & 0xFFFFFFFF) < int(count))


def background(size=(W, H), bg=V.BG):
    w, h = size
    img = np.zeros((h, w, 4), np.uint8)
    img[:] = bg
    return img


def shaded(e, shades, start=None, ctx=None, rows=None):
    """The colour target [H, W, 4] after the shade calls `shades` = [(ps, Uniforms, (id_first, id_count))], in order, over
    the frame `e` on a target that held `start` (default: the background everywhere -- a cleared frame of depth-only
    draws).  ps: an oracle_np pixel shader id or a closure (u, ctx) -> rgba.  ctx: the buffer [entries, K] (default: the
    oracle's interpolated varyings).  rows: bool per window row, the rows a rank owns (default: all)."""
    x0, x1, y0, y1 = e.window
    img = background((e.color.shape[1], e.color.shape[0])) if start is None else np.array(start, np.uint8)
    ids = e.tri_id[:e.entries]
    ctx = e.ctx[:e.entries] if ctx is None else np.asarray(ctx, F).reshape(e.entries, -1)
    for ps, u, rng in shades:
        sel = in_range(ids, rng)
        i = np.nonzero(sel)[0]
        ly, lx = i // x1, i % x1
        assert (lx < x1 - x0).all()                              # (only pixels of the window carry an id)
        if rows is not None:
            keep = np.asarray(rows)[ly]
            i, ly, lx = i[keep], ly[keep], lx[keep]
        if i.size:
            img[ly, lx] = onp.quantize(onp.pixel_shader(ps, u, ctx[i]))
    return img


def range_pixels(e, ids):
    return int(in_range(e.tri_id[:e.entries], ids).sum())


def check_frame(e, ranges=(EVERY,)):
    """the conditions a frame has to meet on the oracle's output alone before a test may use it"""
    own = e.owned()[:e.entries]
    x0, x1, y0, y1 = e.window
    pix = (np.arange(e.entries) % x1) < (x1 - x0)                # entries that are pixels of the window
    unowned = 1.0 - own[pix].mean()
    assert 0.05 <= unowned <= 0.60, unowned
    for rng in ranges:
        assert range_pixels(e, rng) >= 50, (rng, range_pixels(e, rng))
    assert not np.isnan(e.ctx[:e.entries][own]).any()
    return float(unowned)


# ---- the frames of the tests ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def phong_forward():
    """the K = 8 scene drawn FORWARD by the oracle with PS_PHONG and texture 0: (mesh, kw, Expected)"""
    mesh, kw = V.phong_scene()
    # (a larger model than varyings_scenes.phong(): the sphere leaves 44 % of the frame undrawn, not 64 %)
    kw = dict(kw, model=np.array([1.3, 0, 0, 0, 0, 1.1, 0, 0, 0, 0, 1.3, 0, 0.1, -0.05, 0.0, 1], F))
    return mesh, kw, render([(mesh, onp.VS_PHONG, oracle_uniforms(kw, textures()[0]))], ps=onp.PS_PHONG)


@functools.lru_cache(maxsize=None)
def flat():
    """K = 0: VS_CLIP triangles, PS_FLAT"""
    tris = scenes.random_clip_triangles(260, W, H, seed=5, spread=0.85)
    u = onp.Uniforms(flat_color=FLAT_COLOR)
    return tris, render([(tris, onp.VS_CLIP, u)], ps=onp.PS_FLAT)


FLAT_COLOR = (0.25, 0.5, 0.75, 1.0)
WIDE_SIZE = (290, 34)                                            # a row spans two 256-pixel workgroups, the second partial; two tile rows


@functools.lru_cache(maxsize=None)
def wide():
    tris = V.basic()[0]
    return tris, render([(tris, onp.VS_CLIP_COLOR, onp.Uniforms())], size=WIDE_SIZE)


# ---- the boundary scene: two meshes, ranges cut at n_emit[0] + 1 (phong.rs:361-370: `i <= body_offset` is shaded BODY) ------
def boundary_mesh():
    """The second mesh of the boundary frame.  Input 0: an unclipped triangle in the middle of the frame, nearer (w = 0.5)
    than anything else in either mesh -- it keeps its pixels, and its emission index in the frame is n_emit[0], the `<=`
    boundary.  Input 1: a near triangle across the right edge of the frustum -- a fan, whose triangles own pixels in the
    second range.  Then the rest of varyings_scenes.second()."""
    b = V.second().copy()

    def tri(ndc, w, z=0.5):
        out = np.zeros((3, 7), np.float64)
        for k, (x, y) in enumerate(ndc):
            out[k, :4] = (x * w, y * w, z * w, w)
            out[k, 4:7] = (0.15 + 0.35 * k, 0.8 - 0.3 * k, 0.4 + 0.25 * k)
        return out.astype(F)
    b[0] = tri(((-0.15, -0.2), (0.17, -0.12), (0.02, 0.24)), 0.5)
    b[1] = tri(((0.55, -0.5), (1.6, 0.1), (0.6, 0.55)), 0.6)
    return b


@functools.lru_cache(maxsize=None)
def boundary():
    """(mesh a, mesh b, Expected of the frame of both, the two id ranges)"""
    a, b = V.basic()[0], boundary_mesh()
    e = render([(a, onp.VS_CLIP_COLOR, onp.Uniforms()), (b, onp.VS_CLIP_COLOR, onp.Uniforms())])
    cut = e.n_emit[0] + 1
    return a, b, e, ((0, cut), (cut, sum(e.n_emit) - cut))


def check_boundary():
    a, b, e, ranges = boundary()
    check_frame(e, ranges)
    ids = e.tri_id[:e.entries]
    assert (ids == e.n_emit[0]).sum() >= 1, "the boundary triangle owns nothing"
    owners = np.unique(ids[ids != 0xFFFFFFFF])
    fan = np.concatenate([V.emission_meta(m, onp.VS_CLIP_COLOR, onp.Uniforms())[1] for m in (a, b)])
    assert len(fan) == sum(e.n_emit)
    for first, count in ranges:
        mine = owners[(owners >= first) & (owners - first < count)]
        assert fan[mine].any(), f"no fan triangle owns a pixel in the range {(first, count)}"
    return int((ids == e.n_emit[0]).sum())


# ---- user pixel shaders -------------------------------------------------------------------------------------------------
# K = 3 over the varyings of VS_CLIP_COLOR (the user VS copies them, so the built-in VS hands over the same bits): the
# texture of the slot whose number is captured in u.user[3] at (ctx[0], ctx[1]) and slot 2 at (ctx[1], ctx[2]), both by number
# (frr::sample_2d_slot), blended with the captured weights u.user[0], u.user[1], plus u.user[2] on the red channel.  With
# (1, 0, 0, s) it is the texel of slot s: the `place` of phong.rs:34-38 as a captured value.
SLOTS_SHADER = r"""
__device__ void frr_user_vs(const frr::DevUniforms &u, const float *in, float pos[4], float *ctx)
{ pos[0] = in[0]; pos[1] = in[1]; pos[2] = in[2]; pos[3] = in[3]; ctx[0] = in[4]; ctx[1] = in[5]; ctx[2] = in[6]; }
__device__ void frr_user_ps(const frr::DevUniforms &u, const float *ctx, float out[4], const float *u8lut)
{
    float a[4], b[4];
    frr::sample_2d_slot(u, (int)u.user[3], ctx[0], ctx[1], a, u8lut);
    frr::sample_2d_slot(u, 2, ctx[1], ctx[2], b, u8lut);
    for (int k = 0; k < 4; ++k) out[k] = a[k] * u.user[0] + b[k] * u.user[1];
    out[0] = out[0] + u.user[2];
}
"""


def slots_ps(tex_sel, tex2, user):
    """SLOTS_SHADER's pixel shader on the oracle: tex_sel is the texture in slot user[3], tex2 the one in slot 2"""
    w0, w1, w2 = (F(x) for x in user[:3])

    def ps(u, ctx):
        a = onp.sample_2d(tex_sel, ctx[:, 0:2])
        b = onp.sample_2d(tex2, ctx[:, 1:3])
        out = (a * w0 + b * w1).astype(F)
        out[:, 0] = out[:, 0] + w2
        return out
    return ps


def first_varying_ps(u, ctx):
    """the pixel shader of varyings_scenes.WIDE_SHADER / NARROW_SHADER: (ctx[0], 0, 0, 1)"""
    n = ctx.shape[0]
    return np.stack([ctx[:, 0], np.zeros(n, F), np.zeros(n, F), np.ones(n, F)], axis=1).astype(F)


# ---- a buffer the caller made (test 5) ---------------------------------------------------------------------------------
def special_buffer(e):
    """[entries, 3] float32 for PS_COLOR over the frame e: the drawn entries cycle through values the quantisation has to
    get right, the others hold a signalling NaN"""
    specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 1.1754942e-38, -0.25, -1e30, 1.0, 1.0000001, 1.5, 3e38,
                         254.5 / 255.0, 254.0 / 255.0, 0.99999994, 0.5, 1.0 / 255.0, 0.9999 / 255.0, 0.003921569, 127.5 / 255.0], F)
    buf = np.full((e.entries, 3), 0, np.uint32)
    buf[:] = SNAN_BITS
    buf = buf.view(F)
    own = np.nonzero(e.owned()[:e.entries])[0]
    k = np.arange(own.size)
    for c in range(3):
        buf[own, c] = specials[(k * (c + 1) + 5 * c) % specials.size]
    return buf
