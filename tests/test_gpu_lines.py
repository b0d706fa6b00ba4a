"""FrameBuffer::draw_line on the device (frr_draw_lines, frr_draw_wireframe): every image is compared byte for byte with
tests/lines_reference.py -- the reference's sequential walk, renderer.rs:540-588 -- applied to the image expected underneath.
The frame is 96 x 70: three tile rows, the last one 6 pixels high."""
import numpy as np
import pytest

from . import lines_reference as R

pytestmark = pytest.mark.gpu
W, H = 96, 70
BG = (30, 30, 30, 255)

HAND = [(0, 0, 3, 1), (0, 0, 2, 2), (2, 5, 6, 5), (4, 1, 4, 4), (1, 1, 4, 7)]


def _colors(n, seed=5):
    """n distinct opaque colours"""
    c = np.zeros((n, 4), np.uint8)
    k = np.arange(n, dtype=np.uint32) * 2654435761 + seed
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = 64 + (k & 127), (k >> 8) & 255, np.arange(n) & 255, 255 - (np.arange(n) >> 8)
    return c


def _segments(n, seed, reach=20):
    """n random segments inside the frame, up to `reach` pixels long per axis"""
    g = np.random.default_rng(seed)
    a = np.stack([g.integers(0, W, n), g.integers(0, H, n)], axis=1)
    b = a + g.integers(-reach, reach + 1, (n, 2))
    b[:, 0] = np.clip(b[:, 0], 0, W - 1)
    b[:, 1] = np.clip(b[:, 1], 0, H - 1)
    return np.concatenate([a, b], axis=1).astype(np.uint32)


def _blank():
    img = np.empty((H, W, 4), np.uint8)
    img[...] = BG
    return img


def _renderer(options=()):
    import f_renderer_amd as fr
    r = fr.Renderer(W, H)
    for k, v in options:
        r.set_option(k, v)
    return r


def _lines_on_clear(xyxy, rgba, options=()):
    r = _renderer(options)
    r.clear(BG, 0.0)
    L = r.upload_lines(xyxy, rgba)
    assert L.nlines == len(xyxy)
    r.draw_lines(L)
    c, d, t = r.readback()
    assert not d.any() and (t == 0xFFFFFFFF).all()          # colour only
    assert r.stats()["draws"] == 0 and r.stats()["tris_in"] == 0
    L.free()
    r.close()
    return c


# ---- list shapes -----------------------------------------------------------------------------------------------------

def test_hand_lists():
    got = _lines_on_clear(np.array(HAND, np.uint32), _colors(5))
    np.testing.assert_array_equal(got, R.draw_lines(_blank(), HAND, _colors(5)))
    for k, s in enumerate(HAND):   # each alone: exactly the listed pixels
        one = _lines_on_clear(np.array([s], np.uint32), _colors(1))
        want = _blank()
        for x, y in R.line_pixels(*s):
            want[y, x] = _colors(1)[0]
        np.testing.assert_array_equal(one, want, err_msg=str(s))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_around_the_wave(n):
    """a wave takes 64 segments: none, one, one short of a wave, a full one, one over, two and one"""
    xyxy, col = _segments(n, 100 + n), _colors(n)
    np.testing.assert_array_equal(_lines_on_clear(xyxy, col), R.draw_lines(_blank(), xyxy, col))


@pytest.mark.parametrize("chunk", [0, 7])
def test_long_line_among_points(chunk):
    """one 95-pixel line and 63 points in the same wave (chunk 7: the long line is walked in rounds of seven iterations)"""
    xyxy = _segments(64, 7, reach=0)
    xyxy[29] = (0, 3, 95, 66)
    col = _colors(64)
    got = _lines_on_clear(xyxy, col, options=(("lines_chunk", chunk),))
    np.testing.assert_array_equal(got, R.draw_lines(_blank(), xyxy, col))


def test_last_of_300_through_one_pixel_wins():
    # (the endpoints are sorted per axis: (40, 33) is on the drawn line when it is its lower or its upper corner, and the line
    # is neither vertical nor horizontal -- those exclude their upper end)
    g = np.random.default_rng(3)
    far = np.stack([g.integers(41, W, 300), g.integers(34, H, 300)], axis=1)
    far[::3] = np.stack([g.integers(0, 40, 100), g.integers(0, 33, 100)], axis=1)
    xyxy = np.concatenate([np.tile([40, 33], (300, 1)), far], axis=1).astype(np.uint32)
    xyxy[1::2] = xyxy[1::2][:, [2, 3, 0, 1]]
    col = _colors(300)
    for s in xyxy:
        assert (40, 33) in R.line_pixels(*map(int, s))
    got = _lines_on_clear(xyxy, col)
    assert got[33, 40].tolist() == col[299].tolist()
    np.testing.assert_array_equal(got, R.draw_lines(_blank(), xyxy, col))


def test_crossing_fans_in_both_orders():
    a = [(0, 0, x, H - 1) for x in range(5, W, 9)]
    b = [(W - 1, 0, x, H - 1) for x in range(0, W - 5, 9)]
    ca, cb = np.tile([250, 10, 10, 255], (len(a), 1)).astype(np.uint8), np.tile([10, 10, 250, 255], (len(b), 1)).astype(np.uint8)
    ab = _lines_on_clear(np.array(a + b, np.uint32), np.concatenate([ca, cb]))
    ba = _lines_on_clear(np.array(b + a, np.uint32), np.concatenate([cb, ca]))
    np.testing.assert_array_equal(ab, R.draw_lines(_blank(), a + b, np.concatenate([ca, cb])))
    np.testing.assert_array_equal(ba, R.draw_lines(_blank(), b + a, np.concatenate([cb, ca])))
    only_a, only_b = R.draw_lines(_blank(), a, ca), R.draw_lines(_blank(), b, cb)
    crossing = (only_a != _blank()).any(axis=2) & (only_b != _blank()).any(axis=2)
    assert crossing.sum() > 10
    np.testing.assert_array_equal((ab != ba).any(axis=2), crossing)


# ---- refused lists ---------------------------------------------------------------------------------------------------

def _list_with_bad_17():
    xyxy = _segments(40, 11)
    xyxy[17] = (W - 1, H - 2, W + 5, H - 1)      # ends at (W + 5, H - 1): index (H - 1) * W + W + 5 >= W * H
    assert R.panics(*map(int, xyxy[17]), W, H) and not any(R.panics(*map(int, s), W, H) for k, s in enumerate(xyxy) if k != 17)
    return xyxy


def test_refused_upload_names_the_segment():
    import f_renderer_amd as fr
    r = _renderer()
    r.clear(BG, 0.0)
    with pytest.raises(fr.FrrError) as e:
        r.upload_lines(_list_with_bad_17(), _colors(40))
    assert e.value.code == fr.FRR_ERR_INVALID and "segment 17 " in str(e.value)
    np.testing.assert_array_equal(r.readback()[0], _blank())
    r.close()


def test_refused_device_bind_names_the_segment():
    import torch
    import f_renderer_amd as fr
    r = _renderer()
    r.clear(BG, 0.0)
    xyxy = _list_with_bad_17()
    dx = torch.from_numpy(xyxy.view(np.int32)).cuda()
    dc = torch.from_numpy(_colors(40)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(fr.FrrError) as e:
        r.bind_lines_device(dx.data_ptr(), dc.data_ptr(), 40)
    assert e.value.code == fr.FRR_ERR_INVALID and "segment 17 " in str(e.value)
    np.testing.assert_array_equal(r.readback()[0], _blank())
    # the same list without its bad segment binds and draws
    good = np.delete(xyxy, 17, axis=0)
    dx = torch.from_numpy(np.ascontiguousarray(good).view(np.int32)).cuda()
    dc = torch.from_numpy(np.delete(_colors(40), 17, axis=0)).cuda()
    torch.cuda.synchronize()
    L = r.bind_lines_device(dx.data_ptr(), dc.data_ptr(), 39, keepalive=(dx, dc))
    r.draw_lines(L)
    np.testing.assert_array_equal(r.readback()[0], R.draw_lines(_blank(), good, np.delete(_colors(40), 17, axis=0)))
    L.free()
    r.close()


def test_wrapped_segment_lands_in_the_next_row():
    seg = (W - 3, 10, W + 4, 12)                    # x runs past the row: legal, its largest index is 12 * W + W + 4 < W * H
    got = _lines_on_clear(np.array([seg], np.uint32), _colors(1))
    want = R.draw_lines(_blank(), [seg], _colors(1))
    np.testing.assert_array_equal(got, want)
    assert (want[13, 4] == _colors(1)[0]).all() and (want[12, 4] == BG).all()    # (W + 4, 12) is pixel (4, 13)


# ---- ordering with draws and clears ------------------------------------------------------------------------------------

def _two_meshes():
    """near triangles (1 / w = 1) and far ones (1 / w = 0.5) that overlap them and the background: the far draw passes the
    depth test only off the near triangles"""
    from f_renderer_amd import scenes
    ndc = ([[(-0.9, -0.8), (0.2, -0.7), (-0.3, 0.9)], [(-0.1, -0.2), (0.6, 0.1), (0.1, 0.8)]],
           [[(-0.6, -0.9), (0.9, -0.5), (0.0, 0.6)], [(-0.8, 0.3), (0.8, 0.2), (0.3, 0.95)]])
    out = []
    for k, w in enumerate((1.0, 2.0)):
        big = np.array([[(x * w, y * w, 0.5 * w, w) for x, y in tri] for tri in ndc[k]], np.float64)
        small = scenes.random_clip_triangles(10, W, H, seed=40 + k, spread=0.9, w_jitter=0.0)
        clip = np.concatenate([big, small / small[..., 3:4] * w])
        col = scenes.splitmix_u01(60 + k, 12 * 9).reshape(12, 3, 3)
        out.append(np.concatenate([clip, col], axis=2).astype(np.float32))
    return out


def _oracle_sequence(oracle, steps):
    """steps: ("draw", tris) | ("geom", tris) | ("raster",) | ("lines", xyxy, rgba) on one oracle frame"""
    f = oracle.Frame(W, H)
    f.clear(BG, 0.0)
    last = None
    for s in steps:
        if s[0] == "geom":
            last = s[1]
        elif s[0] in ("draw", "raster"):
            last = s[1] if s[0] == "draw" else last
            f.draw(last, oracle.VS_CLIP_COLOR, oracle.PS_COLOR, oracle.make_uniforms(), tri_id_base=int(f.counters.tris_setup))
        else:
            R.draw_lines(f.color, s[1], s[2])
    return f


def _run_sequence(r, steps, meshes):
    import f_renderer_amd as fr
    r.clear(BG, 0.0)
    keep = []
    for s in steps:
        if s[0] == "draw":
            r.draw(meshes[id(s[1])], fr.PS_COLOR)
        elif s[0] == "geom":
            r.geometry_processing(meshes[id(s[1])])
        elif s[0] == "raster":
            r.rasterization((0, W), (0, H), fr.PS_COLOR)
        else:
            keep.append(r.upload_lines(s[1], s[2]))
            r.draw_lines(keep[-1])
    out = r.readback()
    for L in keep:
        L.free()
    return out


def _assert_targets(got, f):
    from .conftest import assert_depth_equal
    c, d, t = got
    np.testing.assert_array_equal(t, f.tri_id)
    assert_depth_equal(d, f.depth)
    np.testing.assert_array_equal(c, f.color)


@pytest.mark.parametrize("order", ["draw_lines", "lines_draw", "draw_lines_draw"])
def test_ordered_with_draws(oracle, order):
    import f_renderer_amd as fr
    near, far = _two_meshes()
    xyxy, col = _segments(90, 21, reach=60), _colors(90)
    steps = {"draw_lines": [("draw", near), ("lines", xyxy, col)],
             "lines_draw": [("lines", xyxy, col), ("draw", near)],
             "draw_lines_draw": [("draw", near), ("lines", xyxy, col), ("draw", far)]}[order]
    want = _oracle_sequence(oracle, steps)
    plain = _oracle_sequence(oracle, [s for s in steps if s[0] == "draw"])
    np.testing.assert_array_equal(want.depth.view(np.uint32), plain.depth.view(np.uint32))    # lines know no depth
    assert (want.color != plain.color).any()
    if order == "draw_lines_draw":   # the far draw covers line pixels off the near triangles, and only there
        after_lines = _oracle_sequence(oracle, steps[:2])
        lines_px = (after_lines.color != _oracle_sequence(oracle, steps[:1]).color).any(axis=2)
        kept = lines_px & (want.color == after_lines.color).all(axis=2)
        assert kept.any() and (lines_px & ~kept).any()
    r = _renderer()
    meshes = {id(m): r.upload_mesh(m, fr.VS_CLIP_COLOR) for m in (near, far)}
    _assert_targets(_run_sequence(r, steps, meshes), want)
    r.close()


@pytest.mark.parametrize("eager", [0, 1])
def test_clear_then_lines(eager):
    """frr_clear directly followed by frr_draw_lines: the deferred clear is settled first"""
    xyxy, col = _segments(70, 8, reach=40), _colors(70)
    r = _renderer((("clear_eager", eager),))
    r.clear((1, 2, 3, 4), 0.25)
    L = r.upload_lines(xyxy, col)
    r.draw_lines(L)
    c, d, t = r.readback()
    want = np.empty((H, W, 4), np.uint8)
    want[...] = (1, 2, 3, 4)
    np.testing.assert_array_equal(c, R.draw_lines(want, xyxy, col))
    assert (d == np.float32(0.25)).all() and (t == 0xFFFFFFFF).all()
    r.close()


@pytest.mark.parametrize("split", [False, True])
def test_replayed_frame_keeps_its_lines_in_place(oracle, split):
    """work lists far too small: the frame's commands are replayed inside the library, the line command between the draws.
    split: the first draw as geometry_processing, lines, rasterization -- the geometry pass's overflow is found by the
    raster pass only, so the replay starts in front of the line command"""
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    near, far = _two_meshes()
    # (something to overflow with: a mesh through the near plane, which needs fan slots)
    clip = scenes.random_clip_triangles(300, W, H, seed=9, spread=1.5, w_jitter=1.5)
    col3 = scenes.splitmix_u01(10, 300 * 9).reshape(300, 3, 3).astype(np.float32)
    big = np.concatenate([clip, col3], axis=2).astype(np.float32)
    xyxy, col = _segments(90, 21, reach=60), _colors(90)
    first = [("geom", big), ("lines", xyxy[40:], col[:50]), ("raster",)] if split else [("draw", big)]
    steps = first + [("lines", xyxy, col), ("draw", far), ("lines", xyxy[:30], col[30:60]), ("draw", near)]
    want = _oracle_sequence(oracle, steps)
    got = {}
    for tiny in (False, True):
        r = _renderer((("bin_capacity", 64), ("fan_capacity", 16)) if tiny else ())
        meshes = {id(m): r.upload_mesh(m, fr.VS_CLIP_COLOR) for m in (near, far, big)}
        got[tiny] = _run_sequence(r, steps, meshes)
        assert (r.stats()["replays"] > 0) == tiny
        r.close()
    _assert_targets(got[True], want)
    np.testing.assert_array_equal(got[True][0], got[False][0])


# ---- frames in flight, bound targets -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fif", [1, 2])
def test_frames_in_flight_alternate_two_lists(fif):
    lists = [(_segments(150, 31, reach=50), _colors(150, 1)), (_segments(80, 32, reach=70), _colors(80, 2))]
    r = _renderer((("frames_in_flight", fif),))
    Ls = [r.upload_lines(*l) for l in lists]
    for i in range(6):
        r.clear(BG, 0.0)
        r.draw_lines(Ls[i % 2])
        want = R.draw_lines(_blank(), *lists[i % 2])
        if i == 4:   # (two commands in one frame)
            r.draw_lines(Ls[1])
            R.draw_lines(want, *lists[1])
        np.testing.assert_array_equal(r.readback()[0], want, err_msg=f"frame {i}")
    r.close()


def test_bound_targets_in_flight_behind_fences():
    import torch
    lists = [(_segments(150, 31, reach=50), _colors(150, 1)), (_segments(80, 32, reach=70), _colors(80, 2))]
    r = _renderer((("bound_targets_in_flight", 1),))
    Ls = [r.upload_lines(*l) for l in lists]
    sets = [tuple(torch.zeros((H, W), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32)) for _ in range(3)]
    st = torch.cuda.Stream()
    taken = []
    for i in range(6):
        c_, d_, t_ = sets[i % 3]
        r.frame_wait(st.cuda_stream)
        r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
        r.clear(BG, 0.0)
        r.draw_lines(Ls[i % 2])
        r.frame_fence(st.cuda_stream)
        with torch.cuda.stream(st):
            taken.append(c_.clone())
    torch.cuda.synchronize()
    for i, c_ in enumerate(taken):
        np.testing.assert_array_equal(c_.cpu().numpy().view(np.uint8).reshape(H, W, 4), R.draw_lines(_blank(), *lists[i % 2]), err_msg=f"frame {i}")
    r.close()


# ---- partition -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("blocked", [False, True])
def test_partitioned_ranks_stitch(world, blocked):
    import torch
    from .conftest import owned_pixel_rows
    xyxy = np.concatenate([_segments(60, 51, reach=50), np.array([(3, 0, 90, H - 1), (50, 0, 50, H), (W - 2, 20, W + 30, 40)], np.uint32)])
    col = _colors(len(xyxy))
    want = R.draw_lines(_blank(), xyxy, col)
    for rank in range(world):
        rows = owned_pixel_rows(H, rank, world, blocked)
        r = _renderer()
        r.set_partition(rank, world, blocked)
        c_ = torch.full((H, W), 0x0B0B0B0B, dtype=torch.int32, device="cuda")
        d_, t_ = torch.zeros((H, W), dtype=torch.float32, device="cuda"), torch.zeros((H, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
        L = r.upload_lines(xyxy, col)
        r.draw_lines(L)                      # no clear: unowned rows must stay what they were
        r.sync()
        got = c_.cpu().numpy().view(np.uint8).reshape(H, W, 4)
        base = np.full((H, W, 4), 0x0B, np.uint8)
        mine = R.draw_lines(base.copy(), xyxy, col, row_filter=lambda y: rows[y])
        np.testing.assert_array_equal(got, mine, err_msg=f"rank {rank}")
        lines_px = (want != _blank()).any(axis=2)
        np.testing.assert_array_equal(got[rows][lines_px[rows]], want[rows][lines_px[rows]])
        np.testing.assert_array_equal(got[~rows], base[~rows])
        r.close()


# ---- wireframe -------------------------------------------------------------------------------------------------------

def _wire_scene():
    """one triangle through the near plane (a fan), one with a corner exactly on the right edge of the viewport (its spi is
    x = W: off the screen), and a few ordinary ones"""
    from f_renderer_amd import scenes
    clip = scenes.random_clip_triangles(9, W, H, seed=4, spread=0.8, w_jitter=0.0)
    clip = (clip / clip[..., 3:4]).astype(np.float32)
    clip[0] = [[-0.5, -0.5, 0.5, 1.0], [0.6, -0.4, 0.5, 1.0], [0.1, 0.7, -0.8, -0.5]]     # w < 0 at one corner
    clip[1] = [[1.0, 0.2, 0.5, 1.0], [0.2, 0.5, 0.5, 1.0], [0.3, -0.6, 0.5, 1.0]]
    col = scenes.splitmix_u01(5, 9 * 9).reshape(9, 3, 3).astype(np.float32)
    return np.concatenate([clip, col], axis=2).astype(np.float32)


def _wire_list(setup):
    """the list a host builds from frr_readback_setup: edges (v0,v1), (v1,v2), (v2,v0), skipped whole when an end is off screen"""
    segs, skipped = [], 0
    for tri in setup["spi"]:
        for e in range(3):
            (xa, ya), (xb, yb) = tri[e], tri[(e + 1) % 3]
            if 0 <= xa < W and 0 <= xb < W and 0 <= ya < H and 0 <= yb < H:
                segs.append((xa, ya, xb, yb))
            else:
                skipped += 1
    return np.array(segs, np.uint32).reshape(-1, 4), skipped


@pytest.mark.parametrize("after", ["geometry", "draw"])
def test_wireframe_is_draw_lines_of_the_setup_list(oracle, after):
    import f_renderer_amd as fr
    tris = _wire_scene()
    color = (255, 200, 0, 255)
    r = _renderer()
    m = r.upload_mesh(tris, fr.VS_CLIP_COLOR)
    r.clear(BG, 0.0)
    if after == "geometry":
        r.geometry_processing(m)
    else:
        r.draw(m, fr.PS_COLOR)
    r.draw_wireframe(color)
    c, d, t = r.readback()
    setup = r.setup_triangles()
    assert setup.shape[0] > tris.shape[0]              # a fan
    xyxy, skipped = _wire_list(setup)
    assert skipped > 0 and len(xyxy) > 0
    f = oracle.Frame(W, H)
    f.clear(BG, 0.0)
    if after == "draw":
        f.draw(tris, oracle.VS_CLIP_COLOR, oracle.PS_COLOR, oracle.make_uniforms())
    np.testing.assert_array_equal(d.view(np.uint32), f.depth.view(np.uint32))
    np.testing.assert_array_equal(t, f.tri_id)
    np.testing.assert_array_equal(c, R.draw_lines(f.color.copy(), xyxy, np.tile(np.array(color, np.uint8), (len(xyxy), 1))))
    # ... and frr_draw_lines of that list gives the same frame
    r.clear(BG, 0.0)
    if after == "draw":
        r.draw(m, fr.PS_COLOR)
    L = r.upload_lines(xyxy, color)
    r.draw_lines(L)
    np.testing.assert_array_equal(r.readback()[0], c)
    r.close()


def test_wireframe_of_a_replayed_geometry(oracle):
    """fan space too small: the geometry pass fails on the device, the wireframe behind it is cancelled and replayed with it"""
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    clip = scenes.random_clip_triangles(300, W, H, seed=9, spread=1.5, w_jitter=1.5)
    col3 = scenes.splitmix_u01(10, 300 * 9).reshape(300, 3, 3).astype(np.float32)
    big = np.concatenate([clip, col3], axis=2).astype(np.float32)
    got = {}
    for tiny in (False, True):
        r = _renderer((("fan_capacity", 16),) if tiny else ())
        m = r.upload_mesh(big, fr.VS_CLIP_COLOR)
        r.clear(BG, 0.0)
        r.geometry_processing(m)
        r.draw_wireframe((9, 250, 9, 255))
        got[tiny] = r.readback()[0]
        assert (r.stats()["replays"] > 0) == tiny
        xyxy, _ = _wire_list(r.setup_triangles())
        r.close()
    np.testing.assert_array_equal(got[False], R.draw_lines(_blank(), xyxy, np.tile(np.array((9, 250, 9, 255), np.uint8), (len(xyxy), 1))))
    np.testing.assert_array_equal(got[True], got[False])


def test_wireframe_refused_after_a_filtered_draw():
    import f_renderer_amd as fr
    r = _renderer()
    with pytest.raises(fr.FrrError) as e:
        r.draw_wireframe(BG)                           # no geometry yet
    assert e.value.code == fr.FRR_ERR_INVALID
    m = r.upload_mesh(_wire_scene(), fr.VS_CLIP_COLOR)
    r.set_partition(1, 2)
    r.clear(BG, 0.0)
    r.draw(m, fr.PS_COLOR)
    with pytest.raises(fr.FrrError) as e:
        r.draw_wireframe(BG)
    assert e.value.code == fr.FRR_ERR_INVALID
    with pytest.raises(fr.FrrError):
        r.setup_triangles()                            # (fails for the same reason)
    r.geometry_processing(m)                           # unfiltered: both work again
    r.draw_wireframe(BG)
    r.sync()
    r.close()


def test_cpp_example_wireframe_switch(tmp_path):
    """examples/phong_headless --wireframe (the C++ mirror's draw_wireframe after the shaded draw) == the same frame through
    the Python binding, whose wireframe the tests above hold to the reference"""
    import os
    import subprocess
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s", "phong_headless"])
    Wx, Hx = 160, 90
    mesh, tex = scenes.displaced_sphere(n=12), scenes.checker_texture(64, 8)
    mp, tp, op = (str(tmp_path / n) for n in ("mesh.f32", "tex.rgba", "out.rgba"))
    mesh.tofile(mp)
    tex.tofile(tp)
    frames = {}
    for wire in (False, True):
        cmd = [os.path.join(root, "examples", "phong_headless")] + (["--wireframe"] if wire else []) + [mp, str(mesh.shape[0]), tp, "64", str(Wx), str(Hx), op]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        frames[wire] = np.fromfile(op, np.uint8).reshape(Hx, Wx, 4)
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(Wx, Hx)
    r = fr.Renderer(Wx, Hx)
    r.set_texture(0, tex)
    r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
    r.clear()
    r.draw(r.upload_mesh(mesh, fr.VS_PHONG), fr.PS_PHONG)
    plain = r.readback()[0]
    r.draw_wireframe((255, 255, 255, 255))
    wired = r.readback()[0]
    r.close()
    np.testing.assert_array_equal(frames[False], plain)
    np.testing.assert_array_equal(frames[True], wired)
    assert (wired != plain).any()


# ---- housekeeping ----------------------------------------------------------------------------------------------------

def test_free_with_a_draw_in_flight_and_profile_counts():
    import f_renderer_amd as fr
    xyxy, col = _segments(200, 77, reach=80), _colors(200)
    r = _renderer()
    r.profile_enable(True, kernels=("k_lines_mark", "k_lines_paint"))
    assert fr.Renderer.KERNELS.index("k_lines_mark") == 8 and fr.Renderer.KERNELS.index("k_raster") == 6
    r.clear(BG, 0.0)
    for _ in range(3):
        L = r.upload_lines(xyxy, col)
        r.draw_lines(L)
        L.free()                                       # waits for the draw; the id is reused
    with pytest.raises(fr.FrrError):
        r.draw_lines(fr.Lines(r, 0, 200))              # freed
    np.testing.assert_array_equal(r.readback()[0], R.draw_lines(_blank(), xyxy, col))
    assert r.profile_get("k_lines_mark")[1] == 3 and r.profile_get("k_lines_paint")[1] == 3
    assert r.profile_get("k_lines_mark")[0] > 0.0
    r.close()
