"""frr_resolve_varyings / frr_readback_varyings on the device: the pixel shader's input (renderer.rs:368-378) as a buffer.
Every result is compared as bit patterns with the NumPy oracle's interpolated ctx (tests/varyings_scenes.py) on the entries
the oracle's triangle ids say are owned, and with a sentinel everywhere else; the GPU's triangle ids are held to the oracle's
first."""
import numpy as np
import pytest

from . import varyings_scenes as V
from .conftest import owned_pixel_rows

pytestmark = pytest.mark.gpu

W, H = V.W, V.H
FULL = W * H


def _renderer(options=()):
    import f_renderer_amd as fr
    r = fr.Renderer(W, H)
    for k, v in options:
        r.set_option(k, v)
    return r


def _buffers(entries, K, n=1):
    """n device buffers [entries, K] holding the sentinel, ready before anything the library enqueues"""
    import torch
    bufs = [torch.full((entries, K), V.SENTINEL, dtype=torch.float32, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    return bufs if n > 1 else bufs[0]


def _ids(r, e):
    """the GPU's triangle ids against the oracle's (a synchronisation point); returns the colour target"""
    c, _, t = r.readback()
    np.testing.assert_array_equal(t, e.tri_id, err_msg="triangle ids differ from the oracle's")
    return c


def _host(buf):
    return buf.cpu().numpy()


def test_basic_k3_device_and_host_after_colour_and_depth_draws():
    import f_renderer_amd as fr
    tris, e = V.basic()
    want = e.buffer()
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    for ps in (fr.PS_COLOR, fr.PS_DEPTH):
        r.clear(V.BG, 0.0)
        r.draw(m, ps)
        buf = _buffers(FULL, 3)
        r.resolve_varyings(buf.data_ptr(), FULL)
        host = r.readback_varyings(fill=V.SENTINEL)
        _ids(r, e)
        V.assert_bits_equal(_host(buf), want, f"device buffer, ps {ps}")
        V.assert_bits_equal(host, want, f"host buffer, ps {ps}")
    nan = r.readback_varyings()                                # default fill
    assert nan.shape == (FULL, 3) and np.isnan(nan[~e.owned()]).all()
    V.assert_bits_equal(nan[e.owned()], e.ctx[e.owned()])
    start = np.arange(FULL * 3, dtype=np.float32).reshape(FULL, 3)   # an array as fill: untouched entries keep their own values
    V.assert_bits_equal(r.readback_varyings(fill=start), e.buffer(start=start))
    r.close()


def test_shader_table_phong_gouraud_and_an_indexed_mesh():
    import f_renderer_amd as fr
    mesh, kw, e = V.phong()                                    # K = 8 through model / view / proj: 16-byte stores
    r = _renderer()
    r.set_uniforms(**kw)
    m = r.upload_mesh(mesh, fr.VS_PHONG)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_DEPTH)
    buf = _buffers(FULL, 8)
    r.resolve_varyings(buf.data_ptr(), FULL)
    host = r.readback_varyings(fill=V.SENTINEL)
    _ids(r, e)
    V.assert_bits_equal(_host(buf), e.buffer())
    V.assert_bits_equal(host, e.buffer())
    r.close()

    mesh, kw, e = V.gouraud()
    r = _renderer()
    r.set_uniforms(**kw)
    m = r.upload_mesh(mesh, fr.VS_GOURAUD)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    buf = _buffers(FULL, 3)
    r.resolve_varyings(buf.data_ptr(), FULL)
    np.testing.assert_array_equal(_ids(r, e), e.color)
    V.assert_bits_equal(_host(buf), e.buffer())
    r.close()

    verts, idx, e = V.indexed()
    r = _renderer()
    m = r.upload_mesh_indexed(verts, idx, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    buf = _buffers(FULL, 3)
    r.resolve_varyings(buf.data_ptr(), FULL)
    _ids(r, e)
    V.assert_bits_equal(_host(buf), e.buffer())
    r.close()


def test_user_shaders_with_sixteen_varyings_and_with_one():
    import f_renderer_amd as fr
    tris, e = V.basic()
    r = _renderer()
    sids = {}
    for source, src, sign in ((V.WIDE_SHADER, V.WIDE_SRC, V.WIDE_SIGN), (V.NARROW_SHADER, V.NARROW_SRC, V.NARROW_SIGN)):
        K = len(src)
        sid = sids[K] = r.register_shader(source, 7, K)
        m = r.upload_mesh(tris, sid)
        want = V.user_expected(e, src, sign)
        for ps in (sid, fr.PS_DEPTH):
            r.clear(V.BG, 0.0)
            r.draw(m, ps)
            buf = _buffers(FULL, K)
            r.resolve_varyings(buf.data_ptr(), FULL)
            host = r.readback_varyings(fill=V.SENTINEL)
            _ids(r, e)
            V.assert_bits_equal(_host(buf), want, f"K = {K}")
            V.assert_bits_equal(host, want, f"K = {K}, host")
    # K = 16 into a buffer that is only 4-byte aligned: the scalar stores
    import torch
    raw = torch.full((FULL * 16 + 1,), V.SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.clear(V.BG, 0.0)
    r.draw(r.upload_mesh(tris, sids[16]), fr.PS_DEPTH)
    r.resolve_varyings(raw.data_ptr() + 4, FULL)
    _ids(r, e)
    got = _host(raw)
    assert got.view(np.uint32)[0] == V.SENTINEL_BITS
    V.assert_bits_equal(got[1:].reshape(FULL, 16), V.user_expected(e, V.WIDE_SRC, V.WIDE_SIGN))
    r.close()


def test_two_draws_compose_and_a_late_buffer_keeps_the_sentinel():
    import f_renderer_amd as fr
    a, b, e = V.basic()[0], V.second(), V.two_draws()
    r = _renderer()
    ma, mb = r.upload_mesh(a, fr.VS_CLIP_COLOR), r.upload_mesh(b, fr.VS_CLIP_COLOR)
    every, late = _buffers(FULL, 3, 2)
    r.clear(V.BG, 0.0)
    r.draw(ma, fr.PS_COLOR)
    r.resolve_varyings(every.data_ptr(), FULL)
    r.draw(mb, fr.PS_DEPTH)
    r.resolve_varyings(every.data_ptr(), FULL)
    r.resolve_varyings(late.data_ptr(), FULL)
    _ids(r, e)
    V.assert_bits_equal(_host(every), e.buffer(0), "a resolve after each draw")
    V.assert_bits_equal(_host(late), e.buffer(1), "a resolve after the second draw only")
    kept = e.owned(0) & ~e.owned(1)
    assert kept.sum() > 500 and (_host(late).view(np.uint32)[kept] == V.SENTINEL_BITS).all()
    r.close()


def test_sub_window_with_depth_stride_x1():
    import f_renderer_amd as fr
    tris, e = V.basic()[0], V.sub_window()
    x0, x1, y0, y1 = V.SUB_WINDOW
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.geometry_processing(m)
    r.rasterization((x0, x1), (y0, y1), fr.PS_COLOR)
    buf = _buffers(e.entries, 3)
    r.resolve_varyings(buf.data_ptr(), e.entries, (x0, x1), (y0, y1))
    host = r.readback_varyings((x0, x1), (y0, y1), fill=V.SENTINEL)
    _ids(r, e)
    assert e.entries == (y1 - y0) * x1 and host.shape == (e.entries, 3)
    V.assert_bits_equal(_host(buf), e.buffer())
    V.assert_bits_equal(host, e.buffer())
    r.close()


def test_errors():
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    tris, e = V.basic()
    buf = _buffers(FULL, 3)
    r = _renderer()

    def refused(code, *args, **kw):
        with pytest.raises(fr.FrrError) as err:
            r.resolve_varyings(*args, **kw)
        assert err.value.code == code, err.value

    refused(fr.FRR_ERR_INVALID, buf.data_ptr(), FULL)                       # before any geometry pass
    with pytest.raises(fr.FrrError) as err:
        r.readback_varyings()
    assert err.value.code == fr.FRR_ERR_INVALID
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    refused(fr.FRR_ERR_UNSUPPORTED, buf.data_ptr(), FULL, (-1, W - 1), (0, H))
    refused(fr.FRR_ERR_INVALID, buf.data_ptr(), FULL - 1)                   # a short buffer
    refused(fr.FRR_ERR_INVALID, buf.data_ptr(), FULL, (5, 5), (0, H))       # x1 <= x0
    refused(fr.FRR_ERR_INVALID, buf.data_ptr(), FULL, (0, W), (9, 3))       # y1 <= y0
    refused(fr.FRR_ERR_INVALID, buf.data_ptr(), 4 * FULL, (0, W + 1), (0, H))   # beyond what frr_raster accepts
    refused(fr.FRR_ERR_INVALID, buf.data_ptr(), 4 * FULL, (0, W), (0, H + 1))
    refused(fr.FRR_ERR_INVALID, 0, FULL)                                    # no buffer
    refused(fr.FRR_ERR_INVALID, buf.data_ptr() + 2, FULL)                   # not 4-byte aligned
    r.resolve_varyings(buf.data_ptr(), FULL)                                # ... and none of them broke the ctx
    _ids(r, e)
    V.assert_bits_equal(_host(buf), e.buffer())
    # K == 0: valid, writes nothing
    buf = _buffers(FULL, 3)
    m0 = r.upload_mesh(scenes.random_clip_triangles(50, W, H, seed=5), fr.VS_CLIP)
    r.clear(V.BG, 0.0)
    r.draw(m0, fr.PS_FLAT)
    r.resolve_varyings(buf.data_ptr(), FULL)
    assert r.readback_varyings().shape == (FULL, 0)
    r.sync()
    assert (_host(buf).view(np.uint32) == V.SENTINEL_BITS).all()
    r.close()
    # the setup list of a partitioned frr_draw holds this rank's triangles only
    r = _renderer()
    r.set_partition(1, 2)
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    refused(fr.FRR_ERR_INVALID, buf.data_ptr(), FULL)
    with pytest.raises(fr.FrrError) as err:
        r.readback_varyings()
    assert err.value.code == fr.FRR_ERR_INVALID and "frr_geometry" in str(err.value)
    r.sync()
    assert (_host(buf).view(np.uint32) == V.SENTINEL_BITS).all()
    r.close()


@pytest.mark.parametrize("path", ["raster_sweep", "bin_atomics", "clip_queue", "clear_eager", "bound_targets"])
def test_paths(path):
    import torch
    import f_renderer_amd as fr
    tris, e = V.basic()
    r = _renderer(() if path == "bound_targets" else ((path, 1),))
    if path == "bound_targets":
        c_ = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        d_ = torch.zeros(FULL, dtype=torch.float32, device="cuda")
        t_ = torch.zeros(FULL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    buf = _buffers(FULL, 3)
    r.resolve_varyings(buf.data_ptr(), FULL)
    host = r.readback_varyings(fill=V.SENTINEL)
    if path == "bound_targets":
        r.sync()
        np.testing.assert_array_equal(t_.cpu().numpy().view(np.uint32), e.tri_id)
    else:
        _ids(r, e)
    V.assert_bits_equal(_host(buf), e.buffer(), path)
    V.assert_bits_equal(host, e.buffer(), path)
    r.close()


def test_replayed_draws_and_a_replayed_resolve():
    """Work lists far too small: the draw is repaired inside the call, and the resolve issued behind it -- before any
    synchronisation point -- is exact.  Then a resolve that is itself replayed: the geometry pass in front of it fails on the
    device (nobody has looked yet), the resolve is cancelled and runs again in its place when the raster pass repairs."""
    import f_renderer_amd as fr
    tris, e = V.basic()
    r = _renderer((("bin_capacity", 64), ("fan_capacity", 16)))
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    buf = _buffers(FULL, 3)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    r.resolve_varyings(buf.data_ptr(), FULL)
    assert r.stats()["replays"] > 0
    _ids(r, e)
    V.assert_bits_equal(_host(buf), e.buffer())
    r.close()

    r = _renderer((("fan_capacity", 16),))
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    early, buf = _buffers(FULL, 3, 2)
    r.clear(V.BG, 0.0)
    r.geometry_processing(m)                                    # the fan space overflows on the device
    r.resolve_varyings(early.data_ptr(), FULL)                  # nothing is drawn yet: whether cancelled or replayed, it writes nothing
    r.rasterization((0, W), (0, H), fr.PS_DEPTH)                # repairs: geometry, resolve and raster pass run again
    r.resolve_varyings(buf.data_ptr(), FULL)
    assert r.stats()["replays"] > 0
    _ids(r, e)
    V.assert_bits_equal(_host(buf), e.buffer())
    assert (_host(early).view(np.uint32) == V.SENTINEL_BITS).all()
    r.close()


@pytest.mark.parametrize("fif", [2, 1])
def test_two_frames_in_flight_resolve_into_their_own_buffers(fif):
    import torch
    import f_renderer_amd as fr
    a, ea = V.basic()
    b, eb = V.second(), V.second_alone()
    r = _renderer((("frames_in_flight", fif),))
    ma, mb = r.upload_mesh(a, fr.VS_CLIP_COLOR), r.upload_mesh(b, fr.VS_CLIP_COLOR)
    for m, e in ((ma, ea), (mb, eb)):                           # each frame once by itself: its ids, and its need of the work lists is known
        r.clear(V.BG, 0.0)
        r.draw(m, fr.PS_COLOR)
        _ids(r, e)
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    for _ in range(2):
        bufa, bufb = _buffers(FULL, 3, 2)
        r.clear(V.BG, 0.0)
        r.draw(ma, fr.PS_COLOR)
        r.resolve_varyings(bufa.data_ptr(), FULL)
        r.clear(V.BG, 0.0)
        r.draw(mb, fr.PS_DEPTH)
        r.resolve_varyings(bufb.data_ptr(), FULL)
        # one fence on a stream of the caller's own, then that stream's sync: the reads are ordered behind both frames.  (Not
        # torch's default stream: its handle is 0, which frame_fence takes for the renderer's own stream.)
        r.frame_fence(st.cuda_stream)
        with torch.cuda.stream(st):
            ga, gb = bufa.to("cpu", non_blocking=False), bufb.to("cpu", non_blocking=False)
        st.synchronize()
        V.assert_bits_equal(ga.numpy(), ea.buffer(), "first frame")
        V.assert_bits_equal(gb.numpy(), eb.buffer(), "second frame")
    _ids(r, eb)
    assert r.stats()["replays"] == 0
    r.close()


@pytest.mark.parametrize("world,blocked", [(2, False), (2, True), (3, False), (3, True)])
def test_partitioned_ranks_write_their_own_rows_and_stitch(world, blocked):
    import f_renderer_amd as fr
    tris, e = V.basic()
    want = e.buffer().reshape(H, W, 3)
    stitched = np.full((H, W, 3), np.nan, np.float32)
    ids = np.zeros((H, W), np.uint32)
    for rank in range(world):
        rows = owned_pixel_rows(H, rank, world, blocked)
        r = _renderer()
        r.set_partition(rank, world, blocked)
        m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
        r.clear(V.BG, 0.0)
        r.geometry_processing(m)                                # (unfiltered: frr_draw's list holds this rank's triangles only)
        r.rasterization((0, W), (0, H), fr.PS_COLOR)
        buf = _buffers(FULL, 3)
        r.resolve_varyings(buf.data_ptr(), FULL)
        host = r.readback_varyings(fill=V.SENTINEL)
        t = r.readback()[2].reshape(H, W)
        got = _host(buf).reshape(H, W, 3)
        assert rows.any() and (got[~rows].view(np.uint32) == V.SENTINEL_BITS).all(), "a rank wrote rows it does not own"
        V.assert_bits_equal(host, got.reshape(FULL, 3))
        stitched[rows], ids[rows] = got[rows], t[rows]
        r.close()
    np.testing.assert_array_equal(ids.reshape(-1), e.tri_id)
    V.assert_bits_equal(stitched, want)


def test_colour_target_is_the_quantised_resolve():
    """what FRR_PS_COLOR wrote is quantize() of what the resolve returns: the same value reached the pixel shader"""
    import f_renderer_amd as fr
    from oracle import oracle_np as onp
    tris, e = V.basic()
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(V.BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    got = r.readback_varyings()
    c = _ids(r, e).reshape(-1, 4)
    own = e.owned()
    assert (np.isnan(got).all(axis=1) == ~own).all()
    np.testing.assert_array_equal(c[own], onp.quantize(np.concatenate([got[own], np.ones((int(own.sum()), 1), np.float32)], axis=1)))
    np.testing.assert_array_equal(c[~own], np.tile(np.array(V.BG, np.uint8), (int((~own).sum()), 1)))
    r.close()
