"""Instanced passes (frr_geometry_instanced / frr_draw_instanced): one mesh under a table of model matrices in ONE geometry
pass.  By definition that is the reference's loop over objects (phong.rs:319-331), so every frame here is held, bit for bit,
to the oracle's loop of draws (tests/instanced_scenes.py) AND to the library's own loop of plain draws with
set_uniforms(model=models[i]) in between: triangle ids, depth, RGBA8, the setup list, tris_in / tris_setup / frag_covered."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle_np as onp

from . import instanced_scenes as S
from . import shade_scenes as SH
from . import user_shaders
from . import varyings_scenes as V
from .conftest import assert_depth_equal, owned_pixel_rows

pytestmark = pytest.mark.gpu
W, H = S.W, S.H


def _renderer(fr, sc, ps=None, options=(), stream=None):
    r = fr.Renderer(W, H, stream=stream)
    for k, v in options:
        r.set_option(k, v)
    r.set_texture(0, S.texture())
    if sc.lit:
        r.set_uniforms(texture_slot=0, **S.camera_kw(fr))
    return r


def _mesh(r, sc, vs_id, indexed=None):
    import f_renderer_amd as fr  # noqa: F401
    if indexed == "upload":
        return r.upload_mesh_indexed(sc.indexed[0], sc.indexed[1], vs_id)
    return r.upload_mesh(sc.tris, vs_id)


def _instanced(r, mesh, inst, ps_id, setup=True):
    r.clear(*S.CLEAR)
    r.draw_instanced(mesh, inst, ps_id)
    c, d, t = r.readback()
    return dict(c=c, d=d, t=t, st=r.stats(), setup=r.setup_triangles() if setup else None)


def _loop(r, mesh, models, ps_id):
    """the only way without instancing: one draw per matrix"""
    r.clear(*S.CLEAR)
    setups = []
    for m in models:
        r.set_uniforms(model=m)
        r.draw(mesh, ps_id)
        setups.append(r.setup_triangles())
    c, d, t = r.readback()
    return dict(c=c, d=d, t=t, st=r.stats(), setup=np.concatenate(setups) if setups else None)


def _assert_frame(got, f, rows=None):
    rows = slice(None) if rows is None else rows
    np.testing.assert_array_equal(got["t"].reshape(H, W)[rows], f.tri_id.reshape(H, W)[rows])
    assert_depth_equal(got["d"].reshape(H, W)[rows], f.depth.reshape(H, W)[rows])
    np.testing.assert_array_equal(got["c"][rows], f.color[rows])


def _assert_setup(g, want, K):
    assert g.shape[0] == want.shape[0]
    np.testing.assert_array_equal(g["spi"], want["spi"])
    for name in ("spf", "rhw"):
        np.testing.assert_array_equal(g[name].view(np.uint32), want[name].view(np.uint32))
    np.testing.assert_array_equal(g["ctx"][..., :K].view(np.uint32), want["ctx"][..., :K].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _phong_sid():
    """the user pair is registered once per process (the registry is the process's; hiprtc takes seconds per program)"""
    import f_renderer_amd as fr
    r = fr.Renderer(32, 32)
    sid = r.register_shader(user_shaders.PHONG, 8, 8)
    r.close()
    return sid


def _check(oracle, name, options=(), ps=None, vs_id=None, ps_id=None, user=False, indexed=None, loop=True):
    """the scene in one instanced pass == the oracle's loop of draws == the library's loop of plain draws"""
    import f_renderer_amd as fr
    sc = S.scene(name)
    of, osetup, per = S.oracle_frame(oracle, name, ps)
    r = _renderer(fr, sc, options=options)
    vs_id = getattr(fr, "VS_" + sc.vs) if vs_id is None else vs_id
    ps_id = getattr(fr, "PS_" + (ps or sc.ps)) if ps_id is None else ps_id
    if user:
        vs_id = _phong_sid() if vs_id == "user" else vs_id
        ps_id = _phong_sid() if ps_id == "user" else ps_id
    mesh = _mesh(r, sc, vs_id, indexed)
    inst = r.upload_instances(sc.models)
    assert inst.ninst == sc.ninst
    gi = _instanced(r, mesh, inst, ps_id)
    _assert_frame(gi, of)
    _assert_setup(gi["setup"], osetup, oracle.vs_num_varyings(getattr(oracle, "VS_" + sc.vs)))
    st = gi["st"]
    assert st["tris_in"] == sc.ntris * sc.ninst and st["draws"] == 1
    assert st["tris_setup"] == of.counters.tris_setup == sum(per) and st["frag_covered"] == of.counters.frag_covered
    assert st["frag_nan"] == of.counters.frag_nan
    if loop and sc.ninst:
        gl = _loop(r, mesh, sc.models, ps_id)
        for k in "tdc":
            np.testing.assert_array_equal(gi[k].view(np.uint32) if k == "d" else gi[k], gl[k].view(np.uint32) if k == "d" else gl[k])
        np.testing.assert_array_equal(gi["setup"], gl["setup"])
        for k in ("tris_in", "tris_setup", "frag_covered", "frag_nan"):
            assert st[k] == gl["st"][k], k
        assert gl["st"]["draws"] == sc.ninst
    inst.free()
    r.close()
    return st


@pytest.mark.parametrize("n,k", S.BOUNDARY)
def test_block_and_wave_boundaries(oracle, n, k):
    """the pass's inputs are the dense (instance, triangle) pairs: several instances inside one wave, blocks whose instance
    changes at lanes that are no wave starts, more than 128 instances in one block, a mesh over one, two and three blocks"""
    st = _check(oracle, "b%dx%d" % (n, k))
    assert st["frag_covered"] > 0 and st["replays"] == 0


def test_no_instances_draws_nothing(oracle):
    st = _check(oracle, "none")
    assert st["draws"] == 1 and st["tris_in"] == 0 and st["frag_covered"] == 0


def test_one_instance_is_the_plain_draw(oracle):
    assert _check(oracle, "one")["frag_covered"] > 0


def test_empty_mesh_under_four_instances(oracle):
    st = _check(oracle, "empty_mesh", loop=False)
    assert st["draws"] == 1 and st["tris_setup"] == 0


@pytest.mark.parametrize("name", ["tie_clip", "tie_phong"])
def test_the_later_instance_wins_a_depth_tie(oracle, name):
    """identical copies (a vertex shader that reads no matrix; duplicate matrices): every fragment ties with the other
    copies', and equal depth replaces (renderer.rs:363) -- every covered pixel belongs to the last instance"""
    import f_renderer_amd as fr
    _check(oracle, name)
    sc = S.scene(name)
    per = S.oracle_frame(oracle, name)[2]
    r = _renderer(fr, sc)
    g = _instanced(r, r.upload_mesh(sc.tris, getattr(fr, "VS_" + sc.vs)), r.upload_instances(sc.models), fr.PS_DEPTH, setup=False)
    ids = g["t"][g["t"] != 0xFFFFFFFF]
    assert ids.size > 50 and (ids >= per[0] + per[1]).all() and (ids < sum(per)).all()
    r.close()


@pytest.mark.parametrize("case", ["phong", "gouraud", "clip_color", "user", "user_vs_builtin_ps"])
def test_shaders(oracle, case):
    """the built-in pairs, and the run-time compiled build of the same kernels: a user pair whose vertex shader reads u.mvp
    AND u.model (the built-in Phong pair restated), and that vertex shader under the built-in pixel shader"""
    if case == "phong":
        st = _check(oracle, "clipped")
    elif case in ("gouraud", "clip_color"):
        st = _check(oracle, case)
    elif case == "user":
        st = _check(oracle, "clipped", vs_id="user", ps_id="user", user=True)
    else:
        st = _check(oracle, "clipped", vs_id="user", user=True)
    assert st["frag_covered"] > 0


def test_indexed_mesh_uploaded(oracle):
    sc = S.scene("indexed")
    assert sc.indexed[0].shape[0] == 289 and sc.indexed[1].shape[0] == 512
    assert _check(oracle, "indexed", indexed="upload")["frag_covered"] > 0


def test_indexed_mesh_device_bound(oracle):
    import torch
    import f_renderer_amd as fr
    sc = S.scene("indexed")
    of, osetup, per = S.oracle_frame(oracle, "indexed")
    v, f = sc.indexed
    dv, di = torch.from_numpy(v).to("cuda"), torch.from_numpy(f.view(np.int32)).to("cuda")
    torch.cuda.synchronize()
    r = _renderer(fr, sc)
    m = r.bind_mesh_device_indexed(dv.data_ptr(), v.shape[0], di.data_ptr(), f.shape[0], fr.VS_PHONG, keepalive=(dv, di))
    g = _instanced(r, m, r.upload_instances(sc.models), fr.PS_PHONG)
    _assert_frame(g, of)
    _assert_setup(g["setup"], osetup, 8)
    assert g["st"]["tris_setup"] == of.counters.tris_setup and g["st"]["tris_in"] == 512 * sc.ninst
    r.close()


@pytest.mark.parametrize("clip_queue", [0, 1])
def test_clipped_instances_become_fans(oracle, clip_queue):
    """instances through the near plane and the side planes: fans, expanded by the geometry blocks themselves or by the clip
    kernel (one wave per triangle: there the instance's matrices are wave-uniform)"""
    st = _check(oracle, "clipped", options=(("clip_queue", clip_queue),))
    assert st["tris_setup"] > st["tris_in"] and st["replays"] == 0


def test_clipped_pass_replayed_with_grown_work_lists(oracle):
    """fan space and (triangle, tile) lists far too small: the pass is replayed inside the library -- the table of matrices is
    filled again inside the replayed command -- and the frame is still exact"""
    st = _check(oracle, "clipped", options=(("fan_capacity", 16), ("bin_capacity", 64)))
    assert st["replays"] > 0


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("rank", [0, 1])
def test_partitioned(oracle, rank, blocked):
    """geometry filtered by tile-row ownership: the rank's rows are the oracle's and the triangle ids stay global"""
    import f_renderer_amd as fr
    sc = S.scene("clipped")
    of = S.oracle_frame(oracle, "clipped", "DEPTH")[0]
    r = _renderer(fr, sc)
    r.set_partition(rank, 2, blocked)
    g = _instanced(r, r.upload_mesh(sc.tris, fr.VS_PHONG), r.upload_instances(sc.models), fr.PS_DEPTH, setup=False)
    own = owned_pixel_rows(H, rank, 2, blocked)
    assert own.any() and (g["t"].reshape(H, W)[own] != 0xFFFFFFFF).any()
    _assert_frame(g, of, own)
    beyond = lambda ids: ((ids != 0xFFFFFFFF) & (ids >= sc.ntris * sc.ninst)).any()      # noqa: E731  (fans are counted globally)
    assert beyond(of.tri_id)
    assert beyond(g["t"].reshape(H, W)[own]) == beyond(of.tri_id.reshape(H, W)[own])
    if rank == 0:
        assert beyond(g["t"].reshape(H, W)[own])
    r.close()


@pytest.mark.parametrize("option", [("raster_sweep", 1), ("bin_atomics", 1), ("frames_in_flight", 1), ("overlap", 0), ("overlap", 1)])
def test_other_paths(oracle, option):
    _check(oracle, "clipped", options=(option,))


def test_plain_instanced_plain_in_one_frame(oracle):
    """the ids of a draw continue behind the whole instanced pass, and the pass's behind the draw before it"""
    import f_renderer_amd as fr
    sc, other = S.scene("clipped"), S.scene("b100x7")
    kw = S.camera_kw(oracle)
    kw["tex"] = oracle.Texture(S.texture())
    first = oracle.make_uniforms(model=other.models[0], **kw)
    last = oracle.make_uniforms(model=other.models[5], **kw)
    of = oracle.Frame(W, H)
    of.clear(*S.CLEAR)
    of.draw(other.tris, oracle.VS_PHONG, oracle.PS_PHONG, first)
    n_a = int(of.counters.tris_setup)
    S.oracle_loop(oracle, sc, frame=of, tri_id_base=n_a)
    n_b = int(of.counters.tris_setup)
    of.draw(other.tris, oracle.VS_PHONG, oracle.PS_PHONG, last, tri_id_base=n_b)
    ids = of.tri_id[of.tri_id != 0xFFFFFFFF]
    assert (ids < n_a).any() and ((ids >= n_a) & (ids < n_b)).any() and (ids >= n_b).any()
    r = _renderer(fr, sc)
    ma, mb = r.upload_mesh(other.tris, fr.VS_PHONG), r.upload_mesh(sc.tris, fr.VS_PHONG)
    inst = r.upload_instances(sc.models)
    r.clear(*S.CLEAR)
    r.set_uniforms(model=other.models[0])
    r.draw(ma, fr.PS_PHONG)
    r.draw_instanced(mb, inst, fr.PS_PHONG)
    r.set_uniforms(model=other.models[5])
    r.draw(ma, fr.PS_PHONG)
    c, d, t = r.readback()
    _assert_frame(dict(c=c, d=d, t=t), of)
    st = r.stats()
    assert st["tris_setup"] == of.counters.tris_setup and st["frag_covered"] == of.counters.frag_covered and st["draws"] == 3
    assert st["tris_in"] == 2 * other.ntris + sc.ntris * sc.ninst
    r.close()


def test_one_instanced_geometry_two_raster_windows(oracle):
    """renderer.rs:269-271: one setup list, several ranges"""
    import f_renderer_amd as fr
    sc = S.scene("clipped")
    wins = [(0, 64, 0, H), (0, W, 0, 40)]
    r = _renderer(fr, sc)
    mesh, inst = r.upload_mesh(sc.tris, fr.VS_PHONG), r.upload_instances(sc.models)
    for win in wins:
        # (a sub-window addresses colour and depth locally, renderer.rs:323-381: one frame per window)
        of = oracle.Frame(W, H)
        of.clear(*S.CLEAR)
        S.oracle_loop(oracle, sc, frame=of, window=win)
        r.clear(*S.CLEAR)
        n = r.geometry_processing_instanced(mesh, inst, count=True)
        assert n == of.counters.tris_setup
        r.rasterization(win[:2], win[2:], fr.PS_PHONG)
        c, d, t = r.readback()
        _assert_frame(dict(c=c, d=d, t=t), of)
    r.clear(*S.CLEAR)
    r.geometry_processing_instanced(mesh, inst)
    for win in wins:
        r.rasterization(win[:2], win[2:], fr.PS_PHONG)
    of = oracle.Frame(W, H)
    of.clear(*S.CLEAR)
    for k, win in enumerate(wins):
        S.oracle_loop(oracle, sc, frame=of, window=win)
    c, d, t = r.readback()
    _assert_frame(dict(c=c, d=d, t=t), of)
    r.close()


def test_wireframe_after_an_instanced_geometry(oracle):
    """draw_wireframe of the instanced setup list == draw_lines of the list a host builds from setup_triangles()"""
    import f_renderer_amd as fr
    from . import lines_reference as R
    sc = S.scene("clipped")
    of, osetup, _ = S.oracle_frame(oracle, "clipped")
    color = (255, 200, 0, 255)
    r = _renderer(fr, sc)
    mesh, inst = r.upload_mesh(sc.tris, fr.VS_PHONG), r.upload_instances(sc.models)
    r.clear(*S.CLEAR)
    r.draw_instanced(mesh, inst, fr.PS_PHONG)
    r.draw_wireframe(color)
    c, d, t = r.readback()
    setup = r.setup_triangles()
    np.testing.assert_array_equal(setup["spi"], osetup["spi"])
    segs, skipped = R.wireframe_segments(setup["spi"], W, H)
    xyxy = np.array(segs, np.uint32).reshape(-1, 4)
    assert skipped > 0 and len(xyxy) > 0
    np.testing.assert_array_equal(t, of.tri_id)
    assert_depth_equal(d, of.depth)
    np.testing.assert_array_equal(c, R.draw_lines(of.color.copy(), xyxy, np.tile(np.array(color, np.uint8), (len(xyxy), 1))))
    r.clear(*S.CLEAR)
    r.draw_instanced(mesh, inst, fr.PS_PHONG)
    r.draw_lines(r.upload_lines(xyxy, color))
    np.testing.assert_array_equal(r.readback()[0], c)
    r.close()


@functools.lru_cache(maxsize=None)
def _deferred_scene():
    """three instances of a small sheet, by the NumPy oracle (which keeps every pixel's interpolated varyings)"""
    tris = S.patch(60)
    models = S.clipped_models()[[0, 1, 5]]
    kw = S.camera_kw(onp)
    e = SH.render([(tris, onp.VS_PHONG, onp.Uniforms(model=m, **kw)) for m in models], ps=V.zero_ps, size=(W, H), bg=S.CLEAR[0])
    return tris, models, kw, e


def test_resolve_then_shade_one_instance(oracle):
    """resolve_varyings after an instanced PS_DEPTH draw, then shade_varyings over the id range of instance 1 alone: the ids
    of an instance are one contiguous range"""
    import torch
    import f_renderer_amd as fr
    tris, models, kw, e = _deferred_scene()
    rng = (e.n_emit[0], e.n_emit[1])
    assert SH.range_pixels(e, rng) >= 50 and SH.range_pixels(e, (0, e.n_emit[0])) >= 50
    sc = S.Scene(tris, "PHONG", "DEPTH", models)
    r = _renderer(fr, sc)
    buf = torch.full((W * H, 8), V.SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.clear(*S.CLEAR)
    r.draw_instanced(r.upload_mesh(tris, fr.VS_PHONG), r.upload_instances(models), fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), W * H)
    light = dict(light_pos=(-0.7, 1.9, 1.1), specular=0.9)
    r.set_uniforms(**SH.gpu_uniforms({}, **light))
    r.shade_varyings(fr.PS_PHONG, buf.data_ptr(), W * H, 8, ids=rng)
    c, d, t = r.readback()
    np.testing.assert_array_equal(t, e.tri_id)
    assert_depth_equal(d, e.depth)
    V.assert_bits_equal(buf.cpu().numpy(), e.buffer())
    want = SH.shaded(e, [(onp.PS_PHONG, SH.oracle_uniforms(kw, S.texture(), **light), rng)], start=SH.background((W, H), S.CLEAR[0]))
    np.testing.assert_array_equal(c, want)
    r.close()


def test_device_bound_table_rewritten_in_place(oracle):
    """the table is a torch tensor; after the first frame the caller rewrites it in place: frame_fence on its stream, rewrite,
    bind again -- no host wait of the caller's -- and both frames are the oracle's"""
    import torch
    import f_renderer_amd as fr
    sc = S.scene("clipped")
    m2 = np.ascontiguousarray(sc.models[[5, 0, 3, 1, 2, 4]])
    sc2 = S.Scene(sc.tris, "PHONG", "PHONG", m2)
    frames = [S.oracle_frame(oracle, "clipped")[0], S.oracle_loop(oracle, sc2)[0]]
    assert frames[0].tri_id.tobytes() != frames[1].tri_id.tobytes()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dm = torch.from_numpy(sc.models).to("cuda")
        nm = torch.from_numpy(m2).to("cuda")
    st.synchronize()
    r = _renderer(fr, sc, stream=st.cuda_stream)
    mesh = r.upload_mesh(sc.tris, fr.VS_PHONG)
    got = []
    inst = r.bind_instances_device(dm.data_ptr(), sc.ninst, keepalive=dm)
    r.clear(*S.CLEAR)
    r.draw_instanced(mesh, inst, fr.PS_PHONG)
    r.frame_fence(st.cuda_stream)                     # the rewrite follows every draw issued so far
    with torch.cuda.stream(st):
        dm.copy_(nm)
    inst2 = r.bind_instances_device(dm.data_ptr(), sc.ninst, keepalive=dm)
    got.append(r.readback())
    r.clear(*S.CLEAR)
    r.draw_instanced(mesh, inst2, fr.PS_PHONG)
    got.append(r.readback())
    for (c, d, t), of in zip(got, frames):
        _assert_frame(dict(c=c, d=d, t=t), of)
    assert r.stats()["tris_setup"] == frames[1].counters.tris_setup
    r.close()


def test_non_finite_matrices_are_not_refused():
    """an all-NaN and an all-zero matrix between finite ones: the reference would compute with them, and so does the pass --
    the frame of the library's own loop of plain draws (not held to the oracle)"""
    import f_renderer_amd as fr
    models = S.nonfinite_models()
    sc = S.Scene(S.patch(128), "PHONG", "DEPTH", models)
    r = _renderer(fr, sc)
    mesh = r.upload_mesh(sc.tris, fr.VS_PHONG)
    gi = _instanced(r, mesh, r.upload_instances(models), fr.PS_DEPTH, setup=False)
    gl = _loop(r, mesh, models, fr.PS_DEPTH)
    np.testing.assert_array_equal(gi["t"], gl["t"])
    assert_depth_equal(gi["d"], gl["d"])
    np.testing.assert_array_equal(gi["c"], gl["c"])
    for k in ("tris_in", "tris_setup", "frag_covered", "frag_nan"):
        assert gi["st"][k] == gl["st"][k], k
    assert (gi["t"] != 0xFFFFFFFF).sum() > 100
    r.close()


def test_errors_leave_the_ctx_drawing(oracle):
    import torch
    import f_renderer_amd as fr
    sc = S.scene("one")
    r = _renderer(fr, sc)
    L, ctx = r._lib, r._ctx
    iid = C.c_int(-7)
    assert L.frr_instances_upload(ctx, None, 3, C.byref(iid)) == fr.FRR_ERR_INVALID and iid.value == -7          # NULL, ninst > 0
    assert L.frr_instances_bind_device(ctx, None, 3, C.byref(iid)) == fr.FRR_ERR_INVALID and iid.value == -7
    dm = torch.zeros(16 * 4 + 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert L.frr_instances_bind_device(ctx, C.c_void_p(dm.data_ptr() + 4), 4, C.byref(iid)) == fr.FRR_ERR_INVALID   # misaligned
    assert iid.value == -7
    mesh = r.upload_mesh(sc.tris, fr.VS_PHONG)
    assert L.frr_draw_instanced(ctx, mesh.id, 99, fr.PS_PHONG, 0, W, 0, H) == fr.FRR_ERR_INVALID                # unknown id
    assert L.frr_geometry_instanced(ctx, mesh.id, -1, None) == fr.FRR_ERR_INVALID
    inst = r.upload_instances(sc.models)
    freed = inst.id
    inst.free()
    assert L.frr_draw_instanced(ctx, mesh.id, freed, fr.PS_PHONG, 0, W, 0, H) == fr.FRR_ERR_INVALID              # freed id
    assert L.frr_instances_free(ctx, freed) == fr.FRR_ERR_INVALID
    # the order-key limit on the product: 2^14 triangles x 2^13 instances == 2^27, refused at the draw before anything is allocated
    big = r.upload_mesh(np.zeros((1 << 14, 3, 4), np.float32), fr.VS_CLIP)
    table = r.upload_instances(np.zeros((1 << 13, 16), np.float32))
    with pytest.raises(fr.FrrError) as e:
        r.draw_instanced(big, table, fr.PS_DEPTH)
    assert e.value.code == fr.FRR_ERR_UNSUPPORTED
    assert L.frr_geometry_instanced(ctx, big.id, table.id, None) == fr.FRR_ERR_UNSUPPORTED
    of = S.oracle_frame(oracle, "one")[0]
    _assert_frame(_instanced(r, mesh, r.upload_instances(sc.models), fr.PS_PHONG, setup=False), of)
    r.close()


def test_cpp_host_draws_instances(oracle, tmp_path):
    """frr::Renderer::upload_instances + geometry_processing_instanced (frr_renderer.hpp; examples/phong_headless --instances):
    the compiled host's frame is the Python path's draw_instanced frame, byte for byte"""
    import os
    import subprocess
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    from f_renderer_amd.assets import Model, load_tga
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s", "phong_headless"])
    obj, tga = (os.path.join(root, "tests", "golden", n) for n in ("cube.obj", "checker24.tga"))
    cw, ch, n = 320, 180, 9
    op = str(tmp_path / "out.rgba")
    out = subprocess.run([os.path.join(root, "examples", "phong_headless"), "--assets", obj, tga, str(cw), str(ch), op, "--instances", str(n)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    vertices, faces = Model(obj).indexed_inputs()
    assert "instances: n=%d tris_in=%d" % (n, n * faces.shape[0]) in out.stdout
    F = np.float32
    cols = 3
    s = F(1.0) / F(cols)
    models = np.tile(np.eye(4, dtype=F).reshape(16), (n, 1))
    for i in range(n):
        models[i, [0, 5, 10]] = s
        models[i, 12] = ((F(i % cols) + F(0.5)) * s - F(0.5)) * F(3.0)
        models[i, 13] = ((F(i // cols) + F(0.5)) * s - F(0.5)) * F(2.0)
        models[i, 14] = F(-0.25) * F(i % 3)
    r = fr.Renderer(cw, ch)
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(cw, ch)
    r.set_texture(0, load_tga(tga))
    r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
    r.clear((30, 30, 30, 255), 0.0)
    r.draw_instanced(r.upload_mesh_indexed(vertices, faces, fr.VS_PHONG), r.upload_instances(models), fr.PS_PHONG)
    c, _, t = r.readback()
    assert (t != 0xFFFFFFFF).sum() > 1000 and np.unique(t[t != 0xFFFFFFFF] // faces.shape[0]).size == n
    np.testing.assert_array_equal(np.fromfile(op, np.uint8).reshape(ch, cw, 4), c)
    r.close()
