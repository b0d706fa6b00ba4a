"""Indexed meshes (frr_mesh_upload_indexed / frr_mesh_bind_device_indexed): a vertex array and three vertex numbers per
triangle instead of Vec<[VSInput;3]> (which the reference builds from an indexed Model on the CPU, phong.rs:187-205).  A
vertex shader is a pure function of one vertex, so the draw of (vertices, faces) must be the draw of vertices[faces] -- the
oracle's frame of the expanded mesh and the library's own frame of it through frr_mesh_upload -- bit for bit: depth, triangle
ids, RGBA8, the setup list, the statistics.  (The oracle has no binning, so bin_entries is held to the expanded draw.)"""
import ctypes as C

import numpy as np
import pytest

from . import indexed_scenes as S
from . import user_shaders

pytestmark = pytest.mark.gpu
W, H = S.W, S.H


def _renderer(fr, lit, ps, options=(), stream=None):
    r = fr.Renderer(W, H, stream=stream)
    for k, v in options:
        r.set_option(k, v)
    if ps == "PHONG":
        r.set_texture(0, S.texture())
    if lit:
        r.set_uniforms(texture_slot=0, **S.camera_kw(fr))
    return r


def _draw(r, mesh, ps, setup=True):
    r.clear(*S.CLEAR)
    r.draw(mesh, ps)
    c, d, t = r.readback()
    return dict(c=c, d=d, t=t, st=r.stats(), setup=r.setup_triangles() if setup else None)


def _assert_frame(got, f, rows=None):
    from .conftest import assert_depth_equal
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


def _check(oracle, name, options=(), vs_id=None, ps_id=None, user=None):
    """The scene drawn indexed == the oracle's frame of the expanded mesh == the library's frame of the expanded mesh."""
    import f_renderer_amd as fr
    v, f, vs, ps, lit = S.scene(name)
    of, osetup = S.oracle_frame(oracle, name)
    r = _renderer(fr, lit, ps, options)
    vs_id = getattr(fr, "VS_" + vs) if vs_id is None else vs_id
    ps_id = getattr(fr, "PS_" + ps) if ps_id is None else ps_id
    if user is not None:
        sid = r.register_shader(*user)
        vs_id = sid if vs_id == "user" else vs_id
        ps_id = sid if ps_id == "user" else ps_id
    mi = r.upload_mesh_indexed(v, f, vs_id)
    assert mi.ntris == f.shape[0]
    gi = _draw(r, mi, ps_id)
    ge = _draw(r, r.upload_mesh(S.expand(v, f), vs_id), ps_id)
    _assert_frame(gi, of)
    _assert_setup(gi["setup"], osetup, oracle.vs_num_varyings(getattr(oracle, "VS_" + vs)))
    assert gi["st"]["tris_in"] == f.shape[0]
    assert gi["st"]["tris_setup"] == of.counters.tris_setup and gi["st"]["frag_covered"] == of.counters.frag_covered
    for k in "tdc":
        np.testing.assert_array_equal(gi[k].view(np.uint32) if k == "d" else gi[k], ge[k].view(np.uint32) if k == "d" else ge[k])
    np.testing.assert_array_equal(gi["setup"], ge["setup"])
    assert gi["st"]["bin_entries"] == ge["st"]["bin_entries"]
    mi.free()
    st = gi["st"]
    r.close()
    return st


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_around_the_geometry_block(oracle, n):
    """GEOM_BLOCK = 256 input triangles per workgroup: the last block full, one short, one over; two blocks and one; none."""
    st = _check(oracle, "strip%d" % n)
    assert st["tris_in"] == n and (n == 0 or st["frag_covered"] > 0)


@pytest.mark.parametrize("name", ["grid", "fan", "degenerate", "one_vertex", "poisoned"])
def test_sharing_patterns(oracle, name):
    """17 x 17 vertices under 512 triangles (inner vertices used six times, the last vertex referenced); one vertex in every
    triangle; a triangle that is one vertex three times; a one-vertex array; unreferenced NaN / +-inf vertices around the
    referenced ones, which must change nothing."""
    v, f = S.scene(name)[:2]
    if name == "grid":
        assert v.shape[0] == 289 and f.shape[0] == 512 and f.max() == v.shape[0] - 1 and np.bincount(f.reshape(-1)).max() == 6
    if name == "fan":
        assert (f == 0).any(axis=1).all()
    if name == "degenerate":
        assert (f[60] == f[60, 0]).all()
    if name == "poisoned":
        assert not np.isfinite(v[-1]).any() and np.isfinite(v[np.unique(f)]).all()
        assert S.oracle_frame(oracle, "poisoned")[0].depth.tobytes() == S.oracle_frame(oracle, "grid")[0].depth.tobytes()
    st = _check(oracle, name)
    assert (st["frag_covered"] > 0) == (name != "one_vertex")


@pytest.mark.parametrize("case", ["clip_color", "phong", "gouraud", "user", "user_vs_builtin_ps"])
def test_shaders(oracle, case):
    """NF = 7 (vertex records that are no multiple of 16 bytes), the two 32-byte built-ins, and the run-time compiled build of
    the same kernels (a user pair; a user vertex shader under a built-in pixel shader)."""
    if case == "clip_color":
        st = _check(oracle, "color")
    elif case in ("phong", "gouraud"):
        st = _check(oracle, case)
    elif case == "user":
        st = _check(oracle, "color", vs_id="user", ps_id="user", user=(user_shaders.VERTEX_COLOR, 7, 3))
    else:
        st = _check(oracle, "color", vs_id="user", user=(user_shaders.VERTEX_COLOR, 7, 3))
    assert st["frag_covered"] > 0


@pytest.mark.parametrize("name", ["clipped", "color_clipped"])
@pytest.mark.parametrize("clip_queue", [0, 1])
def test_clipped_inputs_become_fans(oracle, name, clip_queue):
    """the grid through the near plane and the side planes: fans, expanded by the geometry blocks themselves or by the clip
    kernel (both fetch through the index list)"""
    of = S.oracle_frame(oracle, name)[0]
    assert of.counters.tris_setup > of.counters.tris_in
    st = _check(oracle, name, options=(("clip_queue", clip_queue),))
    assert st["replays"] == 0


@pytest.mark.parametrize("clip_queue", [0, 1])
def test_clipped_draw_replayed_with_grown_work_lists(oracle, clip_queue):
    """fan space and (triangle, tile) lists far too small: the draw is replayed inside the library -- through the same mesh
    record -- and the frame is still exact"""
    st = _check(oracle, "color_clipped", options=(("clip_queue", clip_queue), ("fan_capacity", 16), ("bin_capacity", 64)))
    assert st["replays"] > 0


@pytest.mark.parametrize("rank", [0, 1])
def test_partitioned(oracle, rank):
    """geometry filtered by tile-row ownership: the rank's rows are the oracle's and the triangle ids stay global"""
    import f_renderer_amd as fr
    from .conftest import owned_pixel_rows
    v, f, vs, ps, lit = S.scene("clipped")
    of = S.oracle_frame(oracle, "clipped")[0]
    r = _renderer(fr, lit, ps)
    r.set_partition(rank, 2)
    g = _draw(r, r.upload_mesh_indexed(v, f, fr.VS_CLIP), fr.PS_DEPTH, setup=False)
    own = owned_pixel_rows(H, rank, 2, False)
    assert own.any() and (g["t"].reshape(H, W)[own] != 0xFFFFFFFF).any()
    _assert_frame(g, of, own)
    ids = g["t"].reshape(H, W)[own]
    assert ((ids != 0xFFFFFFFF) & (ids >= f.shape[0])).any()      # ids beyond the input count: fans are counted globally
    r.close()


@pytest.mark.parametrize("option", ["raster_sweep", "bin_atomics", "frames_in_flight"])
def test_other_paths(oracle, option):
    _check(oracle, "color_clipped", options=((option, 1),))


@pytest.mark.parametrize("indexed_first", [True, False])
def test_indexed_and_expanded_mesh_in_one_frame(oracle, indexed_first):
    """the ids of the second mesh continue where the first one's end, whichever of the two is the indexed one"""
    import f_renderer_amd as fr
    va, fa = S.scene("clipped")[:2]
    vb, fb = S.scene("fan")[:2]
    of = oracle.Frame(W, H)
    of.clear(*S.CLEAR)
    of.draw(S.expand(va, fa), oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms())
    n_a = int(of.counters.tris_setup)
    of.draw(S.expand(vb, fb), oracle.VS_CLIP, oracle.PS_DEPTH, oracle.make_uniforms(), tri_id_base=n_a)
    assert n_a > fa.shape[0] and (of.tri_id[of.tri_id != 0xFFFFFFFF] >= n_a).any()
    r = fr.Renderer(W, H)
    ma = r.upload_mesh_indexed(va, fa, fr.VS_CLIP) if indexed_first else r.upload_mesh(S.expand(va, fa), fr.VS_CLIP)
    mb = r.upload_mesh(S.expand(vb, fb), fr.VS_CLIP) if indexed_first else r.upload_mesh_indexed(vb, fb, fr.VS_CLIP)
    r.clear(*S.CLEAR)
    r.draw(ma, fr.PS_DEPTH)
    r.draw(mb, fr.PS_DEPTH)
    c, d, t = r.readback()
    _assert_frame(dict(c=c, d=d, t=t), of)
    st = r.stats()
    assert st["tris_setup"] == of.counters.tris_setup and st["frag_covered"] == of.counters.frag_covered and st["draws"] == 2
    r.close()


def _two_oracle_frames(oracle, meshes):
    out = []
    for v, f in meshes:
        of = oracle.Frame(W, H)
        of.clear(*S.CLEAR)
        of.draw(S.expand(v, f), oracle.VS_CLIP_COLOR, oracle.PS_COLOR, oracle.make_uniforms())
        assert of.counters.frag_covered > 0
        out.append(of)
    assert out[0].color.tobytes() != out[1].color.tobytes()
    return out


@pytest.mark.parametrize("rewrite", ["vertices", "indices"])
def test_device_bound_mesh_rewritten_in_place(oracle, rewrite):
    """vertices and indices are torch tensors; after the first frame the caller moves the vertices (or permutes the index
    list) in place: frame_fence on its stream, rewrite, bind again -- no host wait of the caller's -- and both frames are
    the oracle's"""
    import torch
    import f_renderer_amd as fr
    v, f = S.scene("color_clipped")[:2]
    if rewrite == "vertices":
        v2 = v.copy()
        v2[:, 0] += np.float32(0.25) * v[:, 3]
        v2[:, 1] *= np.float32(0.75)
        f2 = f
    else:
        v2 = v
        f2 = np.ascontiguousarray(f[::-1, [1, 2, 0]])          # another submission order and other first corners
    frames = _two_oracle_frames(oracle, [(v, f), (v2, f2)])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dv = torch.from_numpy(v).to("cuda")
        di = torch.from_numpy(f.view(np.int32)).to("cuda")
        nv = torch.from_numpy(v2).to("cuda")
        ni = torch.from_numpy(f2.view(np.int32)).to("cuda")
    st.synchronize()
    r = fr.Renderer(W, H, stream=st.cuda_stream)
    got = []
    m = r.bind_mesh_device_indexed(dv.data_ptr(), v.shape[0], di.data_ptr(), f.shape[0], fr.VS_CLIP_COLOR, keepalive=(dv, di))
    r.clear(*S.CLEAR)
    r.draw(m, fr.PS_COLOR)
    r.frame_fence(st.cuda_stream)                     # the rewrite follows every draw issued so far
    with torch.cuda.stream(st):
        dv.copy_(nv)
        di.copy_(ni)
    m2 = r.bind_mesh_device_indexed(dv.data_ptr(), v.shape[0], di.data_ptr(), f.shape[0], fr.VS_CLIP_COLOR, keepalive=(dv, di))
    got.append(r.readback())
    r.clear(*S.CLEAR)
    r.draw(m2, fr.PS_COLOR)
    got.append(r.readback())
    for (c, d, t), of in zip(got, frames):
        _assert_frame(dict(c=c, d=d, t=t), of)
    assert r.stats()["tris_setup"] == frames[1].counters.tris_setup
    r.close()


def _raw(r, fn, vptr, nverts, iptr, ntris, vs):
    mid = C.c_int(-7)
    rc = getattr(r._lib, fn)(r._ctx, C.c_void_p(vptr), nverts, C.c_void_p(iptr), ntris, vs, C.byref(mid))
    return rc, mid.value, r._lib.frr_last_error(r._ctx).decode()


def _still_draws(oracle, r, fr):
    v, f = S.scene("fan")[:2]
    g = _draw(r, r.upload_mesh_indexed(v, f, fr.VS_CLIP), fr.PS_DEPTH)
    _assert_frame(g, S.oracle_frame(oracle, "fan")[0])


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_index_out_of_range_is_refused_at_registration(oracle, device, where):
    """index == nverts is the reference's out-of-bounds panic (model.vert(i, j)): FRR_ERR_INVALID, no mesh id, the first bad
    triangle named -- checked on the host for a host mesh, by a reduction kernel for a device-bound one"""
    import f_renderer_amd as fr
    v, f = S.scene("grid")[:2]
    t_bad = {"first": 0, "middle": 300, "last": f.shape[0] - 1}[where]
    bad = f.copy()
    bad[t_bad, 2] = v.shape[0]
    if where == "middle":
        bad[400, 0] = 0xFFFFFFFF                          # a later one too: the FIRST is reported
    r = fr.Renderer(W, H)
    if device:
        import torch
        dv, di = torch.from_numpy(v).to("cuda"), torch.from_numpy(bad.view(np.int32)).to("cuda")
        torch.cuda.synchronize()
        rc, mid, msg = _raw(r, "frr_mesh_bind_device_indexed", dv.data_ptr(), v.shape[0], di.data_ptr(), f.shape[0], fr.VS_CLIP)
    else:
        rc, mid, msg = _raw(r, "frr_mesh_upload_indexed", v.ctypes.data, v.shape[0], bad.ctypes.data, f.shape[0], fr.VS_CLIP)
    assert rc == fr.FRR_ERR_INVALID and mid == -7
    assert "triangle %d " % t_bad in msg
    _still_draws(oracle, r, fr)
    r.close()


def test_bad_arguments_are_refused(oracle):
    import torch
    import f_renderer_amd as fr
    v, f = S.scene("grid")[:2]
    r = fr.Renderer(W, H)
    dv = torch.zeros(v.size + 8, dtype=torch.float32, device="cuda")
    di = torch.from_numpy(f.view(np.int32)).to("cuda")
    torch.cuda.synchronize()
    nt = f.shape[0]
    for fn, args in (("frr_mesh_upload_indexed", (v.ctypes.data, 0, f.ctypes.data, nt)),             # triangles, no vertices
                     ("frr_mesh_bind_device_indexed", (dv.data_ptr(), 0, di.data_ptr(), nt)),
                     ("frr_mesh_upload_indexed", (v.ctypes.data, v.shape[0], 0, nt)),              # null index pointer
                     ("frr_mesh_bind_device_indexed", (dv.data_ptr(), v.shape[0], 0, nt)),
                     ("frr_mesh_bind_device_indexed", (dv.data_ptr() + 4, v.shape[0], di.data_ptr(), nt))):   # misaligned vertices
        rc, mid, msg = _raw(r, fn, *args, fr.VS_CLIP)
        assert rc == fr.FRR_ERR_INVALID and mid == -7, (fn, args, rc, msg)
    with pytest.raises(fr.FrrError) as e:
        r.upload_mesh_indexed(v, f + np.uint32(1), fr.VS_CLIP)
    assert e.value.code == fr.FRR_ERR_INVALID
    empty = r.upload_mesh_indexed(np.zeros((0, 4), np.float32), np.zeros((0, 3), np.uint32), fr.VS_CLIP)   # valid: nothing to draw
    r.clear(*S.CLEAR)
    r.draw(empty, fr.PS_DEPTH)
    assert r.stats()["tris_in"] == 0
    _still_draws(oracle, r, fr)
    r.close()


def test_debug_mvp_does_not_take_an_indexed_mesh():
    import f_renderer_amd as fr
    v, f = S.scene("phong")[:2]
    r = fr.Renderer(W, H)
    m = r.upload_mesh_indexed(v, f, fr.VS_PHONG)
    out = np.zeros(f.shape[0] * 12, np.float32)
    ms = C.c_float()
    assert r._lib.frr_debug_mvp(r._ctx, m.id, 0, out.ctypes.data, C.byref(ms)) == fr.FRR_ERR_UNSUPPORTED
    e = r.upload_mesh(S.expand(v, f), fr.VS_PHONG)
    assert r._lib.frr_debug_mvp(r._ctx, e.id, 0, out.ctypes.data, C.byref(ms)) == fr.FRR_OK
    r.close()


def test_cpp_host_draws_the_obj_through_the_indexed_upload(oracle, tmp_path):
    """frr::Model::indexed_inputs + Renderer::upload_mesh_indexed (frr_renderer.hpp; examples/phong_headless --assets): the
    compiled host's frame of cube.obj is the Python path's frame of Model.indexed_inputs(), byte for byte"""
    import os
    import subprocess
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    from f_renderer_amd.assets import Model, load_tga
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fr.build()
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s", "phong_headless"])
    obj, tga = (os.path.join(root, "tests", "golden", n) for n in ("cube.obj", "checker24.tga"))
    cw, ch = 320, 180
    op = str(tmp_path / "out.rgba")
    out = subprocess.run([os.path.join(root, "examples", "phong_headless"), "--assets", obj, tga, str(cw), str(ch), op], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    vertices, faces = Model(obj).indexed_inputs()
    assert "indexed: nverts=%d ntris=%d" % (vertices.shape[0], faces.shape[0]) in out.stdout
    r = fr.Renderer(cw, ch)
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(cw, ch)
    r.set_texture(0, load_tga(tga))
    r.set_uniforms(view=fr.set_look_at(eye, at, up), proj=fr.set_perspective(fovy, aspect, zn, zf), view_pos=eye, texture_slot=0)
    r.clear((30, 30, 30, 255), 0.0)
    r.draw(r.upload_mesh_indexed(vertices, faces, fr.VS_PHONG), fr.PS_PHONG)
    c, _, t = r.readback()
    assert (t != 0xFFFFFFFF).sum() > 3000
    np.testing.assert_array_equal(np.fromfile(op, np.uint8).reshape(ch, cw, 4), c)
    r.close()
