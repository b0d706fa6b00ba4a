"""frr_shade_varyings / frr_shade_varyings_host on the device: a pixel shader over a buffer of varyings into the colour target.
Every expected image is built from the NumPy oracle alone (tests/shade_scenes.py): the background, then
quantize(pixel_shader(uniforms, ctx)) on the entries the oracle's triangle ids say are drawn and in range.  The GPU's triangle
ids are held to the oracle's first; colours are compared as bytes."""
import functools

import numpy as np
import pytest

from oracle import oracle_np as onp
from . import lines_reference as R
from . import shade_scenes as S
from . import varyings_scenes as V
from .conftest import owned_pixel_rows

pytestmark = pytest.mark.gpu

W, H = V.W, V.H
FULL = W * H
UNTOUCHED_RANGE = (150, 300)                                     # (tests/test_shade_cpu.py: both sides of it own >= 50 pixels)


def _renderer(options=(), size=(W, H), stream=None):
    import f_renderer_amd as fr
    r = fr.Renderer(size[0], size[1], stream=stream)
    for k, v in options:
        r.set_option(k, v)
    return r


def _dev(arr):
    """a float32 array on the device, bit for bit (signalling NaNs included), ready before anything the library enqueues"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr, np.float32).view(np.int32).copy()).to("cuda").view(torch.float32)
    torch.cuda.synchronize()
    return t


def _sentinel(entries, K, n=1):
    import torch
    bufs = [torch.full((entries, max(K, 1)), V.SENTINEL, dtype=torch.float32, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    return bufs if n > 1 else bufs[0]


def _read(r, e):
    """(colour, depth, ids) of the current frame, the ids held to the oracle's (a synchronisation point)"""
    c, d, t = r.readback()
    np.testing.assert_array_equal(t, e.tri_id, err_msg="triangle ids differ from the oracle's")
    return c, d, t


@functools.lru_cache(maxsize=None)
def _sid(name):
    """user shaders are registered once per process (the registry is the process's; hiprtc takes seconds per program)"""
    import f_renderer_amd as fr
    source, nf, K = {"wide": (V.WIDE_SHADER, 7, 16), "narrow": (V.NARROW_SHADER, 7, 1), "slots": (S.SLOTS_SHADER, 7, 3)}[name]
    r = fr.Renderer(32, 32)
    sid = r.register_shader(source, nf, K)
    r.close()
    return sid


def _phong_renderer(options=(), stream=None):
    """a renderer with the K = 8 scene's mesh, matrices and the three textures in slots 0, 1, 2; texture_slot = 0"""
    import f_renderer_amd as fr
    mesh, kw, e = S.phong_forward()
    r = _renderer(options, stream=stream)
    for slot, tex in enumerate(S.textures()):
        r.set_texture(slot, tex)
    r.set_uniforms(texture_slot=0, **S.gpu_uniforms(kw))
    return r, r.upload_mesh(mesh, fr.VS_PHONG), kw, e


def _deferred_phong(r, m, buf, ps=None):
    """depth pre-pass, resolve, shade: the frame of test 1"""
    import f_renderer_amd as fr
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), FULL)
    r.shade_varyings(fr.PS_PHONG if ps is None else ps, buf.data_ptr(), FULL, 8)


def _phong_want(light=None, tex=0, ps=onp.PS_PHONG):
    mesh, kw, e = S.phong_forward()
    return S.shaded(e, [(ps, S.oracle_uniforms(kw, S.textures()[tex], **(light or {})), S.EVERY)])


# ---- 1. deferred == forward == the oracle ------------------------------------------------------------------------------------

def test_deferred_equals_forward_equals_the_oracle_k8():
    import f_renderer_amd as fr
    r, m, kw, e = _phong_renderer()
    for ps, ops in ((fr.PS_PHONG, onp.PS_PHONG), (fr.PS_BLINN, onp.PS_BLINN)):
        want = _phong_want(ps=ops)
        r.clear(V.BG, 0.0)
        r.draw(m, ps)
        ca, da, ta = _read(r, e)
        np.testing.assert_array_equal(ca, want, err_msg=f"forward frame, ps {ps}")
        buf = _sentinel(FULL, 8)
        _deferred_phong(r, m, buf, ps)
        cb, db, tb = _read(r, e)
        np.testing.assert_array_equal(cb, want, err_msg=f"deferred frame, ps {ps}")
        np.testing.assert_array_equal(db.view(np.uint32), da.view(np.uint32))
        np.testing.assert_array_equal(tb, ta)
    np.testing.assert_array_equal(_phong_want(), e.color)         # (the oracle's own forward frame: tests/test_shade_cpu.py)
    r.close()


def test_deferred_equals_forward_equals_the_oracle_k3_and_k0():
    import f_renderer_amd as fr
    tris, e = V.basic()
    want = S.shaded(e, [(onp.PS_COLOR, onp.Uniforms(), S.EVERY)])
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    ca, da, ta = _read(r, e)
    np.testing.assert_array_equal(ca, want)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    buf = _sentinel(FULL, 3)
    r.resolve_varyings(buf.data_ptr(), FULL)
    assert r.geometry_num_varyings() == 3
    r.shade_varyings(fr.PS_COLOR, buf.data_ptr())                # entries and K by default: the window's, the geometry pass's
    cb, db, tb = _read(r, e)
    np.testing.assert_array_equal(cb, want)
    np.testing.assert_array_equal(db.view(np.uint32), da.view(np.uint32))
    np.testing.assert_array_equal(tb, ta)
    # FRR_PS_FLAT takes a buffer of any K (and reads none of it)
    r.set_uniforms(flat_color=S.FLAT_COLOR)
    r.shade_varyings(fr.PS_FLAT, buf.data_ptr(), FULL, 3)
    np.testing.assert_array_equal(_read(r, e)[0], S.shaded(e, [(onp.PS_FLAT, onp.Uniforms(flat_color=S.FLAT_COLOR), S.EVERY)]))
    r.close()

    tris, e = S.flat()                                            # K = 0 and no buffer at all
    want = S.shaded(e, [(onp.PS_FLAT, onp.Uniforms(flat_color=S.FLAT_COLOR), S.EVERY)])
    r = _renderer()
    r.set_uniforms(flat_color=S.FLAT_COLOR)
    m = r.upload_mesh(tris, fr.VS_CLIP)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_FLAT)
    ca, da, ta = _read(r, e)
    np.testing.assert_array_equal(ca, want)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    r.shade_varyings(fr.PS_FLAT, 0, K=0)
    cb, db, tb = _read(r, e)
    np.testing.assert_array_equal(cb, want)
    np.testing.assert_array_equal(db.view(np.uint32), da.view(np.uint32))
    r.shade_varyings(fr.PS_FLAT, np.zeros((0, 0), np.float32), K=0)   # the host entry point with nothing to copy
    np.testing.assert_array_equal(_read(r, e)[0], want)
    r.close()


# ---- 2. relight ---------------------------------------------------------------------------------------------------------------

def test_relight_without_a_new_draw():
    import f_renderer_amd as fr
    r, m, kw, e = _phong_renderer()
    buf = _sentinel(FULL, 8)
    _deferred_phong(r, m, buf)
    c, d0, t0 = _read(r, e)
    np.testing.assert_array_equal(c, _phong_want())
    stats = r.stats()
    # (a) the light, the eye, the specular strength
    light = {}                                                    # (uniforms stay until they are set again)
    for change in S.LIGHTS[1:]:
        light.update(change)
        r.set_uniforms(**S.gpu_uniforms({}, **change))
        r.shade_varyings(fr.PS_PHONG, buf.data_ptr(), FULL, 8)
        want = _phong_want(light)
        assert (want != _phong_want()).any()
        np.testing.assert_array_equal(_read(r, e)[0], want, err_msg=f"relit with {light}")
    # (b) another texture slot
    r.set_uniforms(texture_slot=1)
    r.shade_varyings(fr.PS_PHONG, buf.data_ptr(), FULL, 8)
    np.testing.assert_array_equal(_read(r, e)[0], _phong_want(light, tex=1), err_msg="texture slot 1")
    # (c) a texture uploaded since the buffer was resolved
    r.set_texture(1, S.textures()[2])
    r.shade_varyings(fr.PS_BLINN, buf.data_ptr(), FULL, 8)
    c, d1, t1 = _read(r, e)
    np.testing.assert_array_equal(c, _phong_want(light, tex=2, ps=onp.PS_BLINN), err_msg="a texture uploaded since")
    assert r.stats() == stats, "a shade changed frr_stats"
    np.testing.assert_array_equal(d1.view(np.uint32), d0.view(np.uint32))
    np.testing.assert_array_equal(t1, t0)
    r.close()


# ---- 3. id ranges, the `<=` boundary -----------------------------------------------------------------------------------------

def test_id_ranges_and_the_place_rule():
    import f_renderer_amd as fr
    a, b, e, ranges = S.boundary()
    texs = S.textures()
    sid = _sid("slots")
    r = _renderer()
    for slot, tex in enumerate(texs):
        r.set_texture(slot, tex)
    ma, mb = r.upload_mesh(a, fr.VS_CLIP_COLOR), r.upload_mesh(b, fr.VS_CLIP_COLOR)
    buf = _sentinel(FULL, 3)
    r.clear(V.BG, 0.0)
    for m in (ma, mb):                                            # a resolve after each draw: the buffer composes
        r.draw(m, fr.PS_DEPTH)
        r.resolve_varyings(buf.data_ptr(), FULL)
    # an empty range writes nothing
    total = sum(e.n_emit)
    r.set_user_uniforms((1.0, 0.0, 0.0, 0))                      # slot 0
    r.shade_varyings(sid, buf.data_ptr(), FULL, 3, ids=(0, 0))
    r.shade_varyings(sid, buf.data_ptr(), FULL, 3, ids=(total, 1000))
    r.shade_varyings(sid, buf.data_ptr(), FULL, 3, ids=(0xFFFFFFFF, 1))      # (the range of 0xFFFFFFFF alone: "nothing drawn" is never in range)
    np.testing.assert_array_equal(_read(r, e)[0], S.background())
    r.shade_varyings(sid, buf.data_ptr(), FULL, 3, ids=ranges[0])
    r.set_user_uniforms((1.0, 0.0, 0.0, 1))                      # slot 1
    r.shade_varyings(sid, buf.data_ptr(), FULL, 3, ids=ranges[1])
    got = _read(r, e)[0]
    ps0, ps1 = S.slots_ps(texs[0], texs[2], (1.0, 0.0, 0.0, 0)), S.slots_ps(texs[1], texs[2], (1.0, 0.0, 0.0, 1))
    np.testing.assert_array_equal(got, S.shaded(e, [(ps0, None, ranges[0]), (ps1, None, ranges[1])]))
    # the boundary triangle (emission index n_emit[0], the first of the second mesh) carries slot 0's texels
    edge = np.nonzero(e.tri_id == e.n_emit[0])[0]
    q0, q1 = onp.quantize(ps0(None, e.ctx[edge])), onp.quantize(ps1(None, e.ctx[edge]))
    assert edge.size >= 1 and (q0 != q1).any()
    np.testing.assert_array_equal(got.reshape(-1, 4)[edge], q0)
    r.close()


# ---- 4. untouched means untouched --------------------------------------------------------------------------------------------

def test_untouched_means_untouched():
    import f_renderer_amd as fr
    tris, e = V.basic()
    before = (np.array([(0, 3, W - 1, 60), (5, 65, 90, 8), (48, 0, 48, H)], np.uint32), np.array([(255, 0, 0, 255), (0, 255, 0, 9), (1, 2, 3, 4)], np.uint8))
    after = (np.array([(0, 35, W - 1, 35), (10, 2, 80, 66)], np.uint32), np.array([(9, 9, 250, 255), (250, 250, 9, 77)], np.uint8))
    start = R.draw_lines(S.background(), *before)
    sel = S.in_range(e.tri_id, UNTOUCHED_RANGE).reshape(H, W)
    drawn = (e.tri_id != 0xFFFFFFFF).reshape(H, W)
    on_line = (start != S.background()).any(axis=2)
    assert (on_line & sel).any() and (on_line & drawn & ~sel).any() and (on_line & ~drawn).any()
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    Lb, La = r.upload_lines(*before), r.upload_lines(*after)
    buf = _sentinel(FULL, 3)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), FULL)
    r.draw_lines(Lb)
    c0, d0, t0 = _read(r, e)
    np.testing.assert_array_equal(c0, start)
    r.shade_varyings(fr.PS_COLOR, buf.data_ptr(), FULL, 3, ids=UNTOUCHED_RANGE)
    r.draw_lines(La)
    c1, d1, t1 = _read(r, e)
    want = S.shaded(e, [(onp.PS_COLOR, onp.Uniforms(), UNTOUCHED_RANGE)], start=start)
    assert (want[sel] != start[sel]).any() and (want[~sel] == start[~sel]).all()
    np.testing.assert_array_equal(c1, R.draw_lines(want, *after))
    np.testing.assert_array_equal(d1.view(np.uint32), d0.view(np.uint32))
    np.testing.assert_array_equal(t1, t0)
    r.close()


# ---- 5. a buffer the caller made ---------------------------------------------------------------------------------------------

def test_a_buffer_the_caller_made_device_and_host():
    import torch
    import f_renderer_amd as fr
    tris, e = V.basic()
    made = S.special_buffer(e)
    want = S.shaded(e, [(onp.PS_COLOR, onp.Uniforms(), S.EVERY)], ctx=made)
    assert (want[(e.tri_id == 0xFFFFFFFF).reshape(H, W)] == np.array(V.BG, np.uint8)).all()
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    # filled on a stream of the caller's own; frame_wait orders that write before the shade
    st = torch.cuda.Stream()
    src = _dev(made)
    with torch.cuda.stream(st):
        buf = src.clone()
    r.frame_wait(st.cuda_stream)
    r.shade_varyings(fr.PS_COLOR, buf.data_ptr(), FULL, 3)
    np.testing.assert_array_equal(_read(r, e)[0], want, err_msg="device buffer")
    # the same through the host entry point; the array is the caller's again as soon as the call returns
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    host = made.copy()
    r.shade_varyings(fr.PS_COLOR, host)
    host[...] = 0.5
    np.testing.assert_array_equal(_read(r, e)[0], want, err_msg="host array")
    r.close()


# ---- 6. user shaders -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wide", "narrow"])
def test_user_shaders_with_sixteen_varyings_and_with_one(name):
    import torch
    import f_renderer_amd as fr
    tris, e = V.basic()
    src, sign = {"wide": (V.WIDE_SRC, V.WIDE_SIGN), "narrow": (V.NARROW_SRC, V.NARROW_SIGN)}[name]
    K, sid = len(src), _sid(name)
    ctx = V.user_expected(e, src, sign)                         # the oracle's varyings of the user shader, the sentinel elsewhere
    want = S.shaded(e, [(S.first_varying_ps, None, S.EVERY)], ctx=ctx)
    # (K = 16: red is +colour 0, a gradient; K = 1: red is -colour 1, which quantises to 0 on every drawn pixel, not the background's 30)
    assert len(np.unique(want[..., 0])) > (50 if K == 16 else 1)
    r = _renderer()
    # a built-in vertex shader and the user pixel shader over a buffer of the user shader's K
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    made = _dev(ctx)
    r.shade_varyings(sid, made.data_ptr(), FULL, K)
    np.testing.assert_array_equal(_read(r, e)[0], want, err_msg="built-in VS + user PS")
    # the same user id for both: drawn forward, then depth pre-pass + resolve + shade
    mu = r.upload_mesh(tris, sid)
    r.clear(V.BG, 0.0)
    r.draw(mu, sid)
    np.testing.assert_array_equal(_read(r, e)[0], want, err_msg="forward, user VS + user PS")
    buf = _sentinel(FULL, K)
    r.clear(V.BG, 0.0)
    r.draw(mu, fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), FULL)
    r.shade_varyings(sid, buf.data_ptr())
    np.testing.assert_array_equal(_read(r, e)[0], want, err_msg="deferred, user VS + user PS")
    if K == 16:                                                   # ... and on a view offset by one float: the scalar loads
        assert buf.data_ptr() % 16 == 0
        raw = torch.full((FULL * 16 + 1,), V.SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.clear(V.BG, 0.0)
        r.draw(mu, fr.PS_DEPTH)
        r.resolve_varyings(raw.data_ptr() + 4, FULL)
        r.shade_varyings(sid, raw.data_ptr() + 4, FULL, 16)
        np.testing.assert_array_equal(_read(r, e)[0], want, err_msg="a buffer that is only 4-byte aligned")
    r.close()


@pytest.mark.parametrize("same_id", [False, True])
def test_user_shader_over_two_slots_relit_through_user_uniforms(same_id):
    import f_renderer_amd as fr
    tris, e = V.basic()
    texs = S.textures()
    sid = _sid("slots")
    r = _renderer()
    for slot, tex in enumerate(texs):
        r.set_texture(slot, tex)
    m = r.upload_mesh(tris, sid if same_id else fr.VS_CLIP_COLOR)
    buf = _sentinel(FULL, 3)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), FULL)
    seen = []
    for user in ((0.625, 0.3, 0.0, 1), (0.2, 0.75, 0.125, 0)):
        r.set_user_uniforms(user)
        r.shade_varyings(sid, buf.data_ptr(), FULL, 3)
        want = S.shaded(e, [(S.slots_ps(texs[user[3]], texs[2], user), None, S.EVERY)])
        np.testing.assert_array_equal(_read(r, e)[0], want, err_msg=f"user uniforms {user}")
        seen.append(want)
    assert (seen[0] != seen[1]).any() and len(np.unique(seen[0].reshape(-1, 4), axis=0)) > 50
    r.close()


# ---- 7. windows and shapes ---------------------------------------------------------------------------------------------------

def test_sub_window_with_depth_stride_x1():
    import f_renderer_amd as fr
    tris, e = V.basic()[0], V.sub_window()
    x0, x1, y0, y1 = V.SUB_WINDOW
    want = S.shaded(e, [(onp.PS_COLOR, onp.Uniforms(), S.EVERY)])
    np.testing.assert_array_equal(want, e.color)                  # (the oracle's forward frame of the window: window-local pixels, the frame's stride)
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.geometry_processing(m)
    r.rasterization((x0, x1), (y0, y1), fr.PS_DEPTH)
    buf = _sentinel(e.entries, 3)
    r.resolve_varyings(buf.data_ptr(), e.entries, (x0, x1), (y0, y1))
    r.shade_varyings(fr.PS_COLOR, buf.data_ptr(), width_range=(x0, x1), height_range=(y0, y1))
    np.testing.assert_array_equal(_read(r, e)[0], want)
    # ... and from the host
    r.clear(V.BG, 0.0)
    r.geometry_processing(m)
    r.rasterization((x0, x1), (y0, y1), fr.PS_DEPTH)
    r.shade_varyings(fr.PS_COLOR, r.readback_varyings((x0, x1), (y0, y1), fill=V.SENTINEL), width_range=(x0, x1), height_range=(y0, y1))
    np.testing.assert_array_equal(_read(r, e)[0], want)
    r.close()


def test_a_row_of_two_workgroups_over_two_tile_rows():
    import f_renderer_amd as fr
    tris, e = S.wide()
    w, h = S.WIDE_SIZE
    want = S.shaded(e, [(onp.PS_COLOR, onp.Uniforms(), S.EVERY)])
    np.testing.assert_array_equal(want, e.color)
    r = _renderer(size=S.WIDE_SIZE)
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    buf = _sentinel(w * h, 3)
    r.resolve_varyings(buf.data_ptr(), w * h)
    r.shade_varyings(fr.PS_COLOR, buf.data_ptr())
    np.testing.assert_array_equal(_read(r, e)[0], want)
    r.close()


# ---- 8. paths --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["raster_sweep", "bin_atomics", "clear_eager", "bound_targets"])
def test_paths(path):
    import torch
    r, m, kw, e = _phong_renderer(() if path == "bound_targets" else ((path, 1),))
    if path == "bound_targets":
        c_ = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_ = torch.zeros(FULL, dtype=torch.float32, device="cuda")
        t_ = torch.zeros(FULL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
    buf = _sentinel(FULL, 8)
    _deferred_phong(r, m, buf)
    if path == "bound_targets":
        r.sync()
        np.testing.assert_array_equal(t_.cpu().numpy().view(np.uint32), e.tri_id)
        got = c_.cpu().numpy().view(np.uint8).reshape(H, W, 4)
    else:
        got = _read(r, e)[0]
    np.testing.assert_array_equal(got, _phong_want(), err_msg=path)
    r.close()


class _Alias:
    """device memory at `ptr` as a torch tensor (no copy), through the CUDA array interface"""
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2}


@pytest.mark.parametrize("fif", [1, 2])
def test_two_frames_in_flight_shade_into_their_own_target_sets(fif):
    import torch
    import f_renderer_amd as fr
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    r, m, kw, e = _phong_renderer((("frames_in_flight", fif),), stream=st.cuda_stream)
    lights = (S.LIGHTS[0], S.LIGHTS[1])
    wants = [_phong_want(light) for light in lights]
    assert (wants[0] != wants[1]).any()
    r.clear(V.BG, 0.0)                                            # once by itself: the pass's need of the work lists is known
    r.draw(m, fr.PS_DEPTH)
    _read(r, e)
    taken = []
    bufs = _sentinel(FULL, 8, 4)
    for i in range(4):
        r.set_uniforms(**S.gpu_uniforms({"light_pos": (1.2, 1.0, 2.0), "view_pos": kw["view_pos"], "specular": 0.5}, **lights[i % 2]))
        _deferred_phong(r, m, bufs[i])
        r.frame_fence(st.cuda_stream)
        pc, pd, pt = r.target_ptrs()
        with torch.cuda.stream(st):
            taken.append((torch.as_tensor(_Alias(pc, (H, W), "<i4"), device="cuda").clone(), torch.as_tensor(_Alias(pt, (H * W,), "<i4"), device="cuda").clone()))
    torch.cuda.synchronize()
    for i, (c, t) in enumerate(taken):
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), e.tri_id, err_msg=f"frame {i}")
        np.testing.assert_array_equal(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), wants[i % 2], err_msg=f"frame {i}")
    assert r.stats()["replays"] == 0
    r.close()


def test_bound_targets_in_flight_behind_fences():
    import torch
    import f_renderer_amd as fr
    r, m, kw, e = _phong_renderer((("bound_targets_in_flight", 1),))
    lights = (S.LIGHTS[0], S.LIGHTS[1])
    wants = [_phong_want(light) for light in lights]
    sets = [tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32)) for _ in range(3)]
    bufs = _sentinel(FULL, 8, 6)
    st = torch.cuda.Stream()
    taken = []
    for i in range(6):
        c_, d_, t_ = sets[i % 3]
        r.frame_wait(st.cuda_stream)
        r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
        r.set_uniforms(**S.gpu_uniforms({"light_pos": (1.2, 1.0, 2.0), "view_pos": kw["view_pos"], "specular": 0.5}, **lights[i % 2]))
        _deferred_phong(r, m, bufs[i])
        r.frame_fence(st.cuda_stream)
        with torch.cuda.stream(st):
            taken.append((c_.clone(), t_.clone()))
    torch.cuda.synchronize()
    for i, (c, t) in enumerate(taken):
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32).ravel(), e.tri_id, err_msg=f"frame {i}")
        np.testing.assert_array_equal(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), wants[i % 2], err_msg=f"frame {i}")
    r.close()


# ---- 9. replay -----------------------------------------------------------------------------------------------------------------

def _clip_heavy(n=1200):
    """n VS_CLIP_COLOR triangles that all cross the right side plane of the frustum: at least 2 n fan triangles"""
    t = np.zeros((n, 3, 7), np.float32)
    y = np.linspace(-0.9, 0.8, n, dtype=np.float32)
    for k, (dx, dy) in enumerate(((0.7, 0.0), (1.5, 0.05), (0.75, 0.1))):
        t[:, k, 0], t[:, k, 1], t[:, k, 2], t[:, k, 3] = dx, y + dy, 0.5, 1.0
        t[:, k, 4:7] = 0.5
    return t


def test_a_replayed_shade_keeps_the_uniforms_of_its_call():
    """The geometry pass in front of the shade finds the fan space too small -- on the device, nobody has looked yet -- so the
    shade behind it is logged, cancelled and, at the synchronisation point, replayed in its place: with the uniforms of the
    original call, not the ones set since."""
    import f_renderer_amd as fr
    r, m, kw, e = _phong_renderer((("bin_capacity", 64), ("fan_capacity", 16)))
    heavy = r.upload_mesh(_clip_heavy(), fr.VS_CLIP_COLOR)
    buf = _sentinel(FULL, 8)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)                                        # (the (triangle, tile) lists are far too small: repaired inside the call)
    r.resolve_varyings(buf.data_ptr(), FULL)
    n1 = r.stats()["replays"]
    assert n1 > 0
    r.geometry_processing(heavy)                                  # overflows the fan space; frr_geometry does not wait to find out
    r.shade_varyings(fr.PS_PHONG, buf.data_ptr(), FULL, 8)
    r.set_uniforms(**S.gpu_uniforms({}, **S.LIGHTS[1]), texture_slot=1)   # ... something else, after the call and before the sync
    r.sync()
    assert r.stats()["replays"] > n1, "the geometry pass did not fail: nothing was replayed"
    np.testing.assert_array_equal(_read(r, e)[0], _phong_want())
    r.close()


# ---- 10. partition -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world,blocked", [(2, False), (2, True), (3, False), (3, True)])
def test_partitioned_ranks_shade_their_own_rows_and_stitch(world, blocked):
    """Caller-bound targets that hold the whole frame's depth and ids (the oracle's) and a pattern in colour; every rank
    draws (frr_draw: the filtered setup list) and shades from the oracle's buffer.  Every row carries ids in range, so a
    rank that shaded a row it does not own would show."""
    import torch
    import f_renderer_amd as fr
    tris, e = V.basic()
    pattern = np.full((H, W, 4), 0x0B, np.uint8)
    full = S.shaded(e, [(onp.PS_COLOR, onp.Uniforms(), S.EVERY)], start=pattern)
    stitched = np.zeros((H, W, 4), np.uint8)
    src = _dev(e.buffer())
    for rank in range(world):
        rows = owned_pixel_rows(H, rank, world, blocked)
        r = _renderer()
        r.set_partition(rank, world, blocked)
        c_ = torch.full((H, W), 0x0B0B0B0B, dtype=torch.int32, device="cuda")
        d_ = torch.from_numpy(e.depth.copy()).to("cuda")
        t_ = torch.from_numpy(e.tri_id.view(np.int32).copy()).to("cuda")
        torch.cuda.synchronize()
        r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
        m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
        r.draw(m, fr.PS_DEPTH)                                    # no clear: the rows of other ranks keep what the caller put there
        r.shade_varyings(fr.PS_COLOR, src.data_ptr(), FULL, 3)
        r.sync()
        np.testing.assert_array_equal(t_.cpu().numpy().view(np.uint32), e.tri_id, err_msg=f"rank {rank}")
        got = c_.cpu().numpy().view(np.uint8).reshape(H, W, 4)
        assert rows.any() and (got[~rows] == 0x0B).all(), "a rank wrote rows it does not own"
        np.testing.assert_array_equal(got, S.shaded(e, [(onp.PS_COLOR, onp.Uniforms(), S.EVERY)], start=pattern, rows=rows), err_msg=f"rank {rank}")
        stitched[rows] = got[rows]
        r.close()
    np.testing.assert_array_equal(stitched, full)


# ---- 11. errors ----------------------------------------------------------------------------------------------------------------

def test_errors():
    import f_renderer_amd as fr
    tris, e = V.basic()
    want = S.shaded(e, [(onp.PS_COLOR, onp.Uniforms(), S.EVERY)])
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    buf = _sentinel(FULL, 3)
    r.resolve_varyings(buf.data_ptr(), FULL)
    big = _sentinel(4 * FULL, 8)
    p, hostbuf = buf.data_ptr(), np.zeros((FULL, 8), np.float32)
    narrow = _sid("narrow")

    def refused(code, ps, b, *args, **kw):
        with pytest.raises(fr.FrrError) as err:
            r.shade_varyings(ps, b, *args, **kw)
        assert err.value.code == code, err.value
        assert len(str(err.value).split(": ", 1)[1]) > 8, "frr_last_error is empty"
        r.shade_varyings(fr.PS_COLOR, p, FULL, 3)               # a valid call still works

    for b in (p, hostbuf):
        refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, b, FULL - 1, 3)                             # in_entries < (y1 - y0) * x1
        refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, b, FULL, 3, (5, 5), (0, H))                 # x1 <= x0
        refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, b, FULL, 3, (0, W), (9, 3))                 # y1 <= y0
        refused(fr.FRR_ERR_UNSUPPORTED, fr.PS_COLOR, b, FULL, 3, (-1, W - 1), (0, H))        # x0 < 0
        refused(fr.FRR_ERR_INVALID, fr.PS_DEPTH, b, FULL, 3)                                 # nothing to shade
        refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, b, FULL, 8)                                 # K of the shader table
        refused(fr.FRR_ERR_INVALID, fr.PS_PHONG, b, FULL, 3)
        refused(fr.FRR_ERR_INVALID, narrow, b, FULL, 3)                                      # a user id with another K
    refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, big.data_ptr(), 4 * FULL, 3, (0, W + 1), (0, H))    # windows frr_raster would refuse
    refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, big.data_ptr(), 4 * FULL, 3, (0, W), (0, H + 1))
    refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, big.data_ptr(), 4 * FULL, 3, (50, 100), (0, H))     # the depth index 69 * 100 + 49 would leave the buffer
    refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, 0, FULL, 3)                                     # no buffer
    refused(fr.FRR_ERR_INVALID, fr.PS_COLOR, p + 2, FULL, 3)                                 # not 4-byte aligned
    refused(fr.FRR_ERR_INVALID, fr.PS_BLINN, big.data_ptr(), FULL, 8)                        # no texture in uniforms.texture_slot
    for ps in (-1, 5, 63, 9999):                                                             # no such shader
        refused(fr.FRR_ERR_INVALID, ps, p, FULL, 3)
    refused(fr.FRR_ERR_INVALID, fr.PS_FLAT, big.data_ptr(), FULL, 17)                   # FRR_MAX_VARYINGS + 1
    refused(fr.FRR_ERR_INVALID, fr.PS_FLAT, big.data_ptr(), FULL, -1)
    np.testing.assert_array_equal(_read(r, e)[0], want)
    r.close()
