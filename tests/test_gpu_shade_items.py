"""frr_shade_items on the device: one shade of all the items of a pass, each under its own material.  Every case is byte-exact
against two expectations (tests/items_scenes.py) -- A, the definition: the loop of ranged shade_varyings calls under
set_uniforms / set_user_uniforms per item, on the same ctx; B, the oracle: the reference's loop with a ps_uniform per object
on the C oracle -- with depth, ids and stats() compared before and after the call.  Frames are 128 x 96."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle_np as onp
from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import items_scenes as IT
from . import shade_scenes as SH
from . import varyings_scenes as V
from .conftest import assert_depth_equal, owned_pixel_rows

pytestmark = pytest.mark.gpu
W, H = D.W, D.H
FULL = W * H
NONE = 0xFFFFFFFF
F = np.float32
CALL_USER = np.array([0.0] * 8 + [0.625, -3.0], F)               # u.user of the CALL: [0, 8) are the material's, [8] stays


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def _renderer(options=(), stream=None, textures=True):
    import f_renderer_amd as fr
    r = fr.Renderer(W, H, stream=stream)
    for k, v in options:
        r.set_option(k, v)
    if textures:
        for slot, tex in enumerate(D.place_textures()):
            r.set_texture(slot, tex)
    r.set_uniforms(texture_slot=0, **S.camera_kw(fr))
    r.set_user_uniforms(CALL_USER)
    return r


def _list(r, sc, kinds=None):
    """the scene's draw list on r; kinds[k]: "plain" (default), "indexed", "dev", "dev_indexed" per distinct mesh"""
    import torch
    import f_renderer_amd as fr
    meshes = []
    for k, m in enumerate(sc.meshes):
        kind = kinds[k] if kinds else "plain"
        if kind == "plain":
            meshes.append(r.upload_mesh(m.tris, fr.VS_PHONG))
        elif kind == "indexed":
            meshes.append(r.upload_mesh_indexed(m.indexed[0], m.indexed[1], fr.VS_PHONG))
        elif kind == "dev":
            dt = torch.from_numpy(m.tris).to("cuda")
            torch.cuda.synchronize()
            meshes.append(r.bind_mesh_device(dt.data_ptr(), m.ntris, fr.VS_PHONG, keepalive=dt))
        else:
            v, f = m.indexed
            dv, di = torch.from_numpy(v).to("cuda"), torch.from_numpy(f.view(np.int32)).to("cuda")
            torch.cuda.synchronize()
            meshes.append(r.bind_mesh_device_indexed(dv.data_ptr(), v.shape[0], di.data_ptr(), f.shape[0], fr.VS_PHONG, keepalive=(dv, di)))
    return r.upload_draw_list([meshes[w] for w in sc.which], sc.models), meshes


def _sentinel(entries=FULL, K=8):
    import torch
    buf = torch.full((entries, max(K, 1)), V.SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return buf


def _prepass(r, dl, buf, wr=(0, W), hr=(0, H)):
    """the list depth-only and one resolve: ids, depth and the varyings of every pixel, no colour"""
    import f_renderer_amd as fr
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_DEPTH, wr, hr)
    r.resolve_varyings(buf.data_ptr(), buf.shape[0], wr, hr)


def _snap(r):
    c, d, t = r.readback()
    return dict(c=c, d=d, t=t, st=r.stats())


def _unchanged(a, b):
    """depth, ids and every field of stats() of two snapshots"""
    np.testing.assert_array_equal(a["t"], b["t"])
    np.testing.assert_array_equal(a["d"].view(np.uint32), b["d"].view(np.uint32))
    assert a["st"] == b["st"], (a["st"], b["st"])


def _set_material(r, m):
    u = CALL_USER.copy()
    u[:8] = m["user"]
    r.set_uniforms(texture_slot=int(m["texture_slot"]), ambient_strength=m["ambient_strength"], specular_strength=m["specular_strength"], flat_color=m["flat_color"])
    r.set_user_uniforms(u)


def _loop_A(r, ps, buf, mats, entries=FULL, K=8, wr=None, hr=None):
    """the definition: one ranged shade_varyings per item of the latest pass under that item's material, then the call's
    uniforms again"""
    first, count = r.item_ranges()
    ptr = buf if isinstance(buf, (int, np.ndarray)) or buf is None else buf.data_ptr()
    for k in range(first.size):
        _set_material(r, mats[k])
        r.shade_varyings(ps, ptr, entries, K, wr, hr, ids=(int(first[k]), int(count[k])))
    r.set_uniforms(texture_slot=0, ambient_strength=F(0.1), specular_strength=0.5, flat_color=(1, 1, 1, 1))
    r.set_user_uniforms(CALL_USER)


def _items_frame(r, dl, ps, mats, K=8, buf=None, shade_buf=None, wr=(0, W), hr=(0, H)):
    """prepass, shade_items with depth / ids / stats compared around it; returns the snapshot after"""
    buf = _sentinel() if buf is None else buf
    _prepass(r, dl, buf, wr, hr)
    before = _snap(r)
    tab = r.upload_materials(mats)
    r.shade_items(ps, (buf if shade_buf is None else shade_buf).data_ptr() if K else None, tab, buf.shape[0], K, wr, hr)
    after = _snap(r)
    _unchanged(before, after)
    tab.free()
    return after


def _loop_frame(r, dl, ps, mats, K=8, buf=None, shade_buf=None, wr=(0, W), hr=(0, H)):
    buf = _sentinel() if buf is None else buf
    _prepass(r, dl, buf, wr, hr)
    _loop_A(r, ps, (buf if shade_buf is None else shade_buf) if K else None, mats, buf.shape[0], K, wr, hr)
    return _snap(r)


def _assert_B(g, fb):
    np.testing.assert_array_equal(g["t"], fb.tri_id, err_msg="triangle ids differ from the oracle's")
    assert_depth_equal(g["d"], fb.depth)
    np.testing.assert_array_equal(g["c"], fb.color)


# ---- 1. scenes, 3. PS_BLINN ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ps", [(n, "PHONG") for n in IT.SCENES] + [(n, "BLINN") for n in ("many", "clipped", "place")])
def test_scenes_equal_the_ranged_loop_and_the_oracle(oracle, name, ps):
    import f_renderer_amd as fr
    sc = D.scene(name)
    mats = IT.materials(sc.nitems)
    r = _renderer()
    dl, _ = _list(r, sc, ["plain", "indexed", "dev", "dev_indexed"] if name == "mix" else None)
    ps_id = getattr(fr, "PS_" + ps)
    g = _items_frame(r, dl, ps_id, mats)
    fb, per = IT.expected_B(name, ps)
    _assert_B(g, fb)                                              # B
    a = _loop_frame(r, dl, ps_id, mats)
    np.testing.assert_array_equal(g["c"], a["c"])                 # A
    np.testing.assert_array_equal(g["t"], a["t"])
    if name in ("none", "all_empty"):
        assert (g["c"] == np.array(D.CLEAR[0], np.uint8)).all()
    elif name != "one":
        assert len(np.unique(g["c"].reshape(-1, 4), axis=0)) > 3 * min(sc.nitems, 3)
    r.close()


# ---- 2. PS_FLAT: K = 0, no buffer, one colour per item ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["many", "empties", "clipped"])
def test_flat_is_one_colour_per_item(oracle, name):
    import f_renderer_amd as fr
    sc = D.scene(name)
    mats = IT.materials(sc.nitems)
    r = _renderer(textures=False)                                 # (an unlit shader asks for no texture)
    dl, _ = _list(r, sc)
    g = _items_frame(r, dl, fr.PS_FLAT, mats, K=0)
    # the direct expectation: from the read-back ids and item_ranges()
    first, count = r.item_ranges()
    item = IT.want_items(g["t"], (0, W), (0, H), np.concatenate([first, [first[-1] + count[-1]]]))
    want = np.zeros((FULL, 4), np.uint8)
    want[:] = D.CLEAR[0]
    hit = item != NONE
    want[hit] = onp.quantize(mats["flat_color"][item[hit]])
    np.testing.assert_array_equal(g["c"].reshape(-1, 4), want)
    assert len(np.unique(item[hit])) > 1
    _assert_B(g, IT.expected_B(name, "FLAT")[0])
    np.testing.assert_array_equal(g["c"], _loop_frame(r, dl, fr.PS_FLAT, mats, K=0)["c"])
    r.close()


# ---- 3. PS_COLOR reads nothing of a material: one unranged shade ------------------------------------------------------------------
def test_color_equals_one_unranged_shade():
    import f_renderer_amd as fr
    sc = D.scene("gouraud")
    r = _renderer(textures=False)
    meshes = [r.upload_mesh(m.tris, fr.VS_GOURAUD) for m in sc.meshes]
    dl = r.upload_draw_list([meshes[w] for w in sc.which], sc.models)
    buf = _sentinel(FULL, 3)
    g = _items_frame(r, dl, fr.PS_COLOR, IT.materials(sc.nitems), K=3, buf=buf)
    _prepass(r, dl, buf)
    r.shade_varyings(fr.PS_COLOR, buf.data_ptr(), FULL, 3)
    one = _snap(r)
    np.testing.assert_array_equal(g["c"], one["c"])
    assert (g["t"] != NONE).sum() > 200 and (g["c"] != np.array(D.CLEAR[0], np.uint8)).any()
    r.close()


# ---- 4. instanced passes: items = instances ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntris,ninst", [(1, 4100), (100, 7)])
def test_instanced_pass(oracle, ntris, ninst):
    """4,100 instances of one triangle: more items than any LDS copy of the boundaries would hold, and nearly every pixel of a
    span another item's; 7 instances of patch(100)"""
    import f_renderer_amd as fr
    tris, models, mats = S.patch(ntris), IT.dense_models(82, 50) if ninst == 4100 else S.grid_models(ninst), IT.materials(ninst)
    r = _renderer()
    mesh, inst = r.upload_mesh(tris, fr.VS_PHONG), r.upload_instances(models)
    tab = r.upload_materials(mats)

    def prepass(buf):
        r.clear(*D.CLEAR)
        r.draw_instanced(mesh, inst, fr.PS_DEPTH)
        r.resolve_varyings(buf.data_ptr(), FULL)
    buf = _sentinel()
    prepass(buf)
    before = _snap(r)
    r.shade_items(fr.PS_PHONG, buf.data_ptr(), tab)
    g = _snap(r)
    _unchanged(before, g)
    fb, per = IT.forward_B([(tris, models[i]) for i in range(ninst)], mats)
    _assert_B(g, fb)
    first, count = r.item_ranges()
    assert first.size == ninst and count.tolist() == per
    owners = np.unique(IT.want_items(g["t"], (0, W), (0, H), np.concatenate([first, [first[-1] + count[-1]]])))
    assert owners.size > (2000 if ninst == 4100 else 6)           # most items own a pixel
    prepass(buf)
    _loop_A(r, fr.PS_PHONG, buf, mats)
    np.testing.assert_array_equal(g["c"], _snap(r)["c"])
    r.close()


# ---- 5. a plain pass is one item ------------------------------------------------------------------------------------------------
def test_plain_pass_is_one_item_under_the_first_material(oracle):
    import f_renderer_amd as fr
    sc = D.scene("one")
    mats = IT.materials(3, seed=1)                                # (more entries than items: the rest is ignored)
    r = _renderer()
    mesh = r.upload_mesh(sc.item_tris(0), fr.VS_PHONG)
    tab = r.upload_materials(mats)
    buf = _sentinel()

    def prepass():
        r.clear(*D.CLEAR)
        r.set_uniforms(model=sc.models[0])
        r.draw(mesh, fr.PS_DEPTH)
        r.resolve_varyings(buf.data_ptr(), FULL)
    prepass()
    r.shade_items(fr.PS_PHONG, buf.data_ptr(), tab)
    g = _snap(r)
    _assert_B(g, IT.forward_B([(sc.item_tris(0), sc.models[0])], mats)[0])
    prepass()
    first, count = r.item_ranges()
    assert first.size == 1
    _set_material(r, mats[0])
    r.shade_varyings(fr.PS_PHONG, buf.data_ptr(), FULL, 8, ids=(int(first[0]), int(count[0])))
    np.testing.assert_array_equal(g["c"], _snap(r)["c"])
    r.close()


# ---- 6. two passes in a frame ---------------------------------------------------------------------------------------------------
def test_pixels_of_an_earlier_pass_keep_their_forward_colour(oracle):
    import f_renderer_amd as fr
    sc = D.scene("sizes")
    mats = IT.materials(sc.nitems, seed=2)
    front = S.patch(90)
    fmodel = S.clipped_models()[1]
    # the oracle: the earlier pass forward under texture 0, then the items behind its ids
    fb, _ = IT.forward_B([(front, fmodel)], IT.materials(1))
    n_front = int(fb.counters.tris_setup)
    fb, per = IT.forward_B(IT.scene_items(sc), mats, frame=fb)
    kept = (fb.tri_id != NONE) & (fb.tri_id < n_front)
    assert kept.sum() > 100 and ((fb.tri_id != NONE) & (fb.tri_id >= n_front)).sum() > 100
    r = _renderer()
    dl, _ = _list(r, sc)
    fmesh = r.upload_mesh(front, fr.VS_PHONG)
    tab = r.upload_materials(mats)
    buf = _sentinel()
    for use_items in (True, False):
        r.clear(*D.CLEAR)
        _set_material(r, IT.materials(1)[0])
        r.set_uniforms(model=fmodel)
        r.draw(fmesh, fr.PS_PHONG)
        r.set_uniforms(texture_slot=0, ambient_strength=F(0.1), specular_strength=0.5, flat_color=(1, 1, 1, 1))
        r.set_user_uniforms(CALL_USER)
        r.draw_list(dl, fr.PS_DEPTH)
        r.resolve_varyings(buf.data_ptr(), FULL)
        if use_items:
            r.shade_items(fr.PS_PHONG, buf.data_ptr(), tab)
            g = _snap(r)
            _assert_B(g, fb)
            assert r.item_ranges()[0][0] == n_front
        else:
            _loop_A(r, fr.PS_PHONG, buf, mats)
            np.testing.assert_array_equal(g["c"], _snap(r)["c"])
    r.close()


# ---- 7. sub-windows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0", [0, 17])
@pytest.mark.parametrize("width", [1, 63, 64, 65, 100])
def test_sub_windows(oracle, x0, width):
    """the pass, the resolve and the shade over one window (row stride x1, a row sub-range): the last span of a row shorter than
    a wave, one span, a span and a lane; entries and pixels outside are untouched"""
    import f_renderer_amd as fr
    sc = D.scene("many")
    mats = IT.materials(sc.nitems)
    wr, hr = (x0, x0 + width), (5, 77)
    entries = (hr[1] - hr[0]) * wr[1]
    fb, per = IT.expected_B("many", "PHONG", (wr[0], wr[1], hr[0], hr[1]))
    r = _renderer()
    dl, _ = _list(r, sc)
    buf = _sentinel(entries)
    g = _items_frame(r, dl, fr.PS_PHONG, mats, buf=buf, wr=wr, hr=hr)
    _assert_B(g, fb)
    if width > 1:
        assert (g["t"] != NONE).any()
    outside = np.ones((H, W), bool)
    outside[:hr[1] - hr[0], :width] = False                       # (colour lands at (cx - x0, cy - y0))
    assert (g["c"][outside] == np.array(D.CLEAR[0], np.uint8)).all()
    np.testing.assert_array_equal(g["c"], _loop_frame(r, dl, fr.PS_PHONG, mats, buf=buf, wr=wr, hr=hr)["c"])
    r.close()


# ---- 8. user shaders --------------------------------------------------------------------------------------------------------------
# reads u.user[0 .. 8) (the material's) AND u.user[8] (the call's), samples the material's slot (frr::sample_2d) and slot 2 by
# number; FRR_USER_K is the K it is registered with (16: 16-byte loads; 1: scalar ones)
USER_SHADER = r"""
__device__ void frr_user_vs(const frr::DevUniforms &u, const float *in, float pos[4], float *ctx)
{ pos[0] = in[0]; pos[1] = in[1]; pos[2] = in[2]; pos[3] = 1.0f; for (int k = 0; k < FRR_USER_K; ++k) ctx[k] = in[k % 8]; }
__device__ void frr_user_ps(const frr::DevUniforms &u, const float *ctx, float out[4], const float *u8lut)
{
    float a[4], b[4];
    frr::sample_2d(u, ctx[0], ctx[1 % FRR_USER_K], a, u8lut);
    frr::sample_2d_slot(u, 2, ctx[1 % FRR_USER_K], ctx[2 % FRR_USER_K], b, u8lut);
    for (int k = 0; k < 4; ++k) out[k] = a[k] * u.user[k] + b[k] * u.user[4 + k];
    out[0] = out[0] + u.user[8] * ctx[FRR_USER_K - 1];
}
"""


@functools.lru_cache(maxsize=None)
def _sid(K):
    import f_renderer_amd as fr
    r = fr.Renderer(32, 32)
    sid = r.register_shader(USER_SHADER, 8, K)
    r.close()
    return sid


def _user_ps(K, tex, tex2, mat):
    w = mat["user"].astype(F)

    def ps(u, ctx):
        a = onp.sample_2d(tex, ctx[:, [0, 1 % K]])
        b = onp.sample_2d(tex2, ctx[:, [1 % K, 2 % K]])
        out = (a * w[None, :4] + b * w[None, 4:8]).astype(F)
        out[:, 0] = out[:, 0] + CALL_USER[8] * ctx[:, K - 1]
        return out
    return ps


@pytest.mark.parametrize("K,misalign", [(16, False), (1, False), (16, True)])
def test_user_shader_reads_the_material_and_the_call(oracle, K, misalign):
    """the buffer is the caller's ([entries][K] in [0, 1), nothing to do with the pass's varyings); the expectation is the
    NumPy closure per item over the oracle's ids, and the ranged loop on the same ctx"""
    import torch
    sc, kw, e = IT.depth_only("clipped")
    mats = IT.materials(sc.nitems)
    texs = D.place_textures()
    rng = np.random.default_rng(8 + K)
    host = rng.random((FULL, K), dtype=F)
    flat = torch.zeros(FULL * K + 4, dtype=torch.float32, device="cuda")
    off = 1 if misalign else 0
    flat[off:off + FULL * K] = torch.from_numpy(host.reshape(-1)).to("cuda")
    torch.cuda.synchronize()
    ptr = flat.data_ptr() + 4 * off
    assert (ptr % 16 == 0) == (not misalign)
    want = SH.shaded(e, [(_user_ps(K, texs[int(mats[k]["texture_slot"])], texs[2], mats[k]), None, rg) for k, rg in enumerate(IT.item_ranges(e.n_emit))],
                     start=SH.background((W, H), IT.BG), ctx=host)
    r = _renderer()
    dl, _ = _list(r, sc)
    tab = r.upload_materials(mats)
    scratch = _sentinel()
    _prepass(r, dl, scratch)
    before = _snap(r)
    r.shade_items(_sid(K), ptr, tab, FULL, K)
    g = _snap(r)
    _unchanged(before, g)
    np.testing.assert_array_equal(g["t"], e.tri_id)
    np.testing.assert_array_equal(g["c"], want)
    _prepass(r, dl, scratch)
    _loop_A(r, _sid(K), ptr, mats, FULL, K)
    np.testing.assert_array_equal(g["c"], _snap(r)["c"])
    # ... and from host memory
    _prepass(r, dl, scratch)
    r.shade_items(_sid(K), host, tab)
    np.testing.assert_array_equal(g["c"], _snap(r)["c"])
    r.close()


def test_user_shader_samples_an_empty_slot_as_zero(oracle):
    """Slot 2 holds no texture.  A material that names it is valid under a user pixel shader, and both ways of sampling it give
    zeros: frr::sample_2d_slot(u, 2, ...) by its own test, frr::sample_2d(u, ...) because such a material is given a 1 x 1 texture
    of zeros.  The expectation is the NumPy closure alone: the ranged loop under uniforms.texture_slot = 2 is the one thing
    frr_shade_varyings leaves undefined, so it is not run."""
    K = 16
    sc, kw, e = IT.depth_only("clipped")
    mats = IT.materials(sc.nitems)
    assert (mats["texture_slot"] == 2).sum() >= 2
    none = np.zeros((1, 1, 4), np.uint8)
    texs = D.place_textures()[:2] + [none]
    host = np.random.default_rng(31).random((FULL, K), dtype=F)
    want = SH.shaded(e, [(_user_ps(K, texs[int(mats[k]["texture_slot"])], none, mats[k]), None, rg) for k, rg in enumerate(IT.item_ranges(e.n_emit))],
                     start=SH.background((W, H), IT.BG), ctx=host)
    r = _renderer(textures=False)
    for slot in (0, 1):
        r.set_texture(slot, texs[slot])
    dl, _ = _list(r, sc)
    tab = r.upload_materials(mats)
    scratch = _sentinel()
    _prepass(r, dl, scratch)
    before = _snap(r)
    r.shade_items(_sid(K), host, tab)
    g = _snap(r)
    _unchanged(before, g)
    np.testing.assert_array_equal(g["t"], e.tri_id)
    np.testing.assert_array_equal(g["c"], want)
    # the items of slot 2 are shaded (user[8] * ctx[15] on the red channel), not skipped, and hold nothing of a texture
    first, count = r.item_ranges()
    item = IT.want_items(g["t"], (0, W), (0, H), np.concatenate([first, [first[-1] + count[-1]]]))
    dark = np.isin(item, np.nonzero(mats["texture_slot"] == 2)[0])
    assert dark.sum() > 50 and (g["c"].reshape(-1, 4)[dark][:, 1:] == 0).all() and (g["c"].reshape(-1, 4)[dark][:, 0] > 0).any()
    r.close()


# ---- 9. replay ------------------------------------------------------------------------------------------------------------------
def _clip_heavy(n=1200):
    """n VS_CLIP_COLOR triangles that all cross the right side plane of the frustum: at least 2 n fan triangles"""
    t = np.zeros((n, 3, 7), np.float32)
    y = np.linspace(-0.9, 0.8, n, dtype=np.float32)
    for k, (dx, dy) in enumerate(((0.7, 0.0), (1.5, 0.05), (0.75, 0.1))):
        t[:, k, 0], t[:, k, 1], t[:, k, 2], t[:, k, 3] = dx, y + dy, 0.5, 1.0
        t[:, k, 4:7] = 0.5
    return t


def test_a_replayed_shade_keeps_its_uniforms_and_reads_the_table_again(oracle):
    """Tiny work lists.  Frame 1: the list pass finds them too small and is repaired inside its call.  Frame 2: a geometry
    pass that overflows the fan space -- on the device, nobody has looked yet: frr_geometry does not wait -- sits in front of
    the list pass, the resolve and the shade, which are cancelled behind it and, at the synchronisation point, replayed in
    their places: the shade with the uniforms of its call, not the ones set since.  The overflowing pass is never rastered, so
    it only moves the items' ids up by what it emitted."""
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    mats = IT.materials(sc.nitems)
    fb, per = IT.expected_B("clipped")
    r = _renderer((("bin_capacity", 64), ("fan_capacity", 16)))
    dl, _ = _list(r, sc)
    heavy = r.upload_mesh(_clip_heavy(), fr.VS_CLIP_COLOR)
    tab = r.upload_materials(mats)
    buf = _sentinel()
    _prepass(r, dl, buf)
    r.shade_items(fr.PS_PHONG, buf.data_ptr(), tab)
    g = _snap(r)
    assert g["st"]["replays"] > 0, "the work lists were large enough: nothing was replayed"
    _assert_B(g, fb)
    r.clear(*D.CLEAR)
    r.geometry_processing(heavy)
    r.draw_list(dl, fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), FULL)
    r.shade_items(fr.PS_PHONG, buf.data_ptr(), tab)
    r.set_uniforms(light_pos=(9, 9, 9), view_pos=(1, 1, 1), texture_slot=2)   # ... something else, after the call and before the sync
    r.set_user_uniforms(np.ones(10, F))
    g = _snap(r)
    assert g["st"]["replays"] > 0, "the geometry pass did not fail: nothing was replayed"
    base = int(r.item_ranges()[0][0])
    assert base >= 2400
    drawn = fb.tri_id != NONE
    np.testing.assert_array_equal(g["t"][drawn], fb.tri_id[drawn] + np.uint32(base))
    assert (g["t"][~drawn] == NONE).all()
    np.testing.assert_array_equal(g["c"], fb.color)
    # ... and it is still A: the same frame again (the lists fit now), shaded by the ranged loop
    r.set_uniforms(texture_slot=0, light_pos=(F(1.2), 1.0, 2.0), **S.camera_kw(fr))
    r.set_user_uniforms(CALL_USER)
    r.clear(*D.CLEAR)
    r.geometry_processing(heavy)
    r.draw_list(dl, fr.PS_DEPTH)
    r.resolve_varyings(buf.data_ptr(), FULL)
    _loop_A(r, fr.PS_PHONG, buf, mats)
    a = _snap(r)
    np.testing.assert_array_equal(g["c"], a["c"])
    np.testing.assert_array_equal(g["t"], a["t"])
    r.close()


# ---- 10. target sets and partition ----------------------------------------------------------------------------------------------
class _Alias:
    """device memory at `ptr` as a torch tensor (no copy), through the CUDA array interface"""
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2}


@pytest.mark.parametrize("fif", [1, 2])
def test_frames_in_flight_shade_into_their_own_target_sets(oracle, fif):
    import torch
    import f_renderer_amd as fr
    st = torch.cuda.Stream()
    sc = D.scene("sizes")
    tables = [IT.materials(sc.nitems), IT.materials(sc.nitems, seed=1)]
    wants = [IT.forward_B(IT.scene_items(sc), m)[0] for m in tables]
    assert (wants[0].color != wants[1].color).any()
    r = _renderer((("frames_in_flight", fif),), stream=st.cuda_stream)
    dl, _ = _list(r, sc)
    tabs = [r.upload_materials(m) for m in tables]
    bufs = [_sentinel() for _ in range(4)]
    _prepass(r, dl, bufs[0])                                      # once by itself: the pass's need of the work lists is known
    r.sync()
    taken = []
    for i in range(4):
        _prepass(r, dl, bufs[i])
        r.shade_items(fr.PS_PHONG, bufs[i].data_ptr(), tabs[i % 2])
        r.frame_fence(st.cuda_stream)
        pc, pd, pt = r.target_ptrs()
        with torch.cuda.stream(st):
            taken.append((torch.as_tensor(_Alias(pc, (H, W), "<i4"), device="cuda").clone(), torch.as_tensor(_Alias(pt, (H * W,), "<i4"), device="cuda").clone()))
    torch.cuda.synchronize()
    for i, (c, t) in enumerate(taken):
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), wants[i % 2].tri_id, err_msg=f"frame {i}")
        np.testing.assert_array_equal(c.cpu().numpy().view(np.uint8).reshape(H, W, 4), wants[i % 2].color, err_msg=f"frame {i}")
    assert r.stats()["replays"] == 0
    r.close()


def test_caller_bound_targets(oracle):
    import torch
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    mats = IT.materials(sc.nitems)
    fb, _ = IT.expected_B("clipped")
    r = _renderer()
    c_ = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    d_ = torch.zeros(FULL, dtype=torch.float32, device="cuda")
    t_ = torch.zeros(FULL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.bind_targets(c_.data_ptr(), d_.data_ptr(), t_.data_ptr())
    dl, _ = _list(r, sc)
    buf = _sentinel()
    _prepass(r, dl, buf)
    r.shade_items(fr.PS_PHONG, buf.data_ptr(), r.upload_materials(mats))
    r.sync()
    np.testing.assert_array_equal(t_.cpu().numpy().view(np.uint32), fb.tri_id)
    np.testing.assert_array_equal(c_.cpu().numpy().view(np.uint8).reshape(H, W, 4), fb.color)
    r.close()


@pytest.mark.parametrize("blocked", [False, True])
def test_partitioned_ranks_stitch_to_the_unpartitioned_frame(oracle, blocked):
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    mats = IT.materials(sc.nitems)
    fb, _ = IT.expected_B("clipped")
    stitched = np.zeros((H, W, 4), np.uint8)
    for rank in (0, 1):
        rows = owned_pixel_rows(H, rank, 2, blocked)
        r = _renderer()
        r.set_partition(rank, 2, blocked)
        dl, _ = _list(r, sc)
        buf = _sentinel()
        r.clear(*D.CLEAR)
        r.geometry_list(dl)                                       # (unfiltered: a draw_list would keep this rank's triangles only)
        r.rasterization((0, W), (0, H), fr.PS_DEPTH)
        r.resolve_varyings(buf.data_ptr(), FULL)
        r.shade_items(fr.PS_PHONG, buf.data_ptr(), r.upload_materials(mats))
        g = _snap(r)
        assert rows.any() and (g["t"].reshape(H, W)[rows] != NONE).any()
        np.testing.assert_array_equal(g["c"][rows], fb.color[rows], err_msg=f"rank {rank}")
        stitched[rows] = g["c"][rows]
        r.close()
    np.testing.assert_array_equal(stitched, fb.color)


# ---- 11. stream order -----------------------------------------------------------------------------------------------------------
def test_later_commands_win_where_they_write(oracle):
    import f_renderer_amd as fr
    sc = D.scene("sizes")
    mats = IT.materials(sc.nitems)
    over, omodel = S.patch(90), S.clipped_models()[0]
    fb, _ = IT.forward_B(IT.scene_items(sc), mats)
    before_over = fb.color.copy()
    fb, _ = IT.forward_B([(over, omodel)], IT.materials(1), frame=fb)
    assert (fb.color != before_over).any()
    xyxy = np.array([[3, 4, 120, 90], [10, 80, 100, 80]], np.uint32)
    want = fr.FrameBuffer(W, H, fb.color.copy())
    for seg in xyxy:
        want.draw_line(*seg, (255, 0, 255, 255))
    r = _renderer()
    dl, _ = _list(r, sc)
    omesh = r.upload_mesh(over, fr.VS_PHONG)
    lines = r.upload_lines(xyxy, (255, 0, 255, 255))
    buf = _sentinel()
    _prepass(r, dl, buf)
    r.shade_items(fr.PS_PHONG, buf.data_ptr(), r.upload_materials(mats))
    _set_material(r, IT.materials(1)[0])
    r.set_uniforms(model=omodel)
    r.draw(omesh, fr.PS_PHONG)
    r.draw_lines(lines)
    g = _snap(r)
    np.testing.assert_array_equal(g["t"], fb.tri_id)
    np.testing.assert_array_equal(g["c"], want.buffer)
    r.close()


# ---- 12. a device-bound table, 13. free ----------------------------------------------------------------------------------------
def test_device_bound_table_rewritten_behind_a_fence_and_freed_in_flight(oracle):
    import torch
    import f_renderer_amd as fr
    sc = D.scene("sizes")
    tables = [IT.materials(sc.nitems), IT.materials(sc.nitems, seed=1)]
    wants = [IT.forward_B(IT.scene_items(sc), m)[0].color for m in tables]
    st = torch.cuda.Stream()
    r = _renderer(stream=st.cuda_stream)
    dl, _ = _list(r, sc)
    buf = _sentinel()
    with torch.cuda.stream(st):
        dev = torch.from_numpy(tables[0].view(np.uint8).copy()).to("cuda")
    assert dev.data_ptr() % 16 == 0
    tab = r.bind_materials_device(dev.data_ptr(), sc.nitems, keepalive=dev)
    _prepass(r, dl, buf)
    r.shade_items(fr.PS_PHONG, buf.data_ptr(), tab)
    r.frame_fence(st.cuda_stream)                                 # the rewrite follows the shade that still reads the table
    with torch.cuda.stream(st):
        pc = r.target_ptrs()[0]
        first = torch.as_tensor(_Alias(pc, (H, W), "<i4"), device="cuda").clone()
        dev.copy_(torch.from_numpy(tables[1].view(np.uint8).copy()).to("cuda"))
    tab2 = r.bind_materials_device(dev.data_ptr(), sc.nitems, keepalive=dev)   # (validates again, behind the rewrite)
    _prepass(r, dl, buf)
    r.shade_items(fr.PS_PHONG, buf.data_ptr(), tab2)
    tab2.free()                                                   # 13: directly after the call -- it finishes first
    tab.free()
    r.sync()
    np.testing.assert_array_equal(first.cpu().numpy().view(np.uint8).reshape(H, W, 4), wants[0])
    np.testing.assert_array_equal(_snap(r)["c"], wants[1])
    assert (wants[0] != wants[1]).any()
    r.close()


# ---- 14. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_ctx_drawing(oracle):
    import torch
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    mats = IT.materials(sc.nitems)
    fb, _ = IT.expected_B("clipped")
    r = _renderer(textures=False)
    for slot in (0, 1):                                           # slot 2 stays empty
        r.set_texture(slot, D.place_textures()[slot])
    dl, _ = _list(r, sc)
    buf = _sentinel()
    p = buf.data_ptr()
    ok2 = mats.copy()
    ok2["texture_slot"] %= 2
    tab, tab01 = r.upload_materials(mats), r.upload_materials(ok2)

    def refused(code, fn, *args, has=None, **kw):
        with pytest.raises(fr.FrrError) as err:
            fn(*args, **kw)
        assert err.value.code == code, err.value
        text = str(err.value).split(": ", 1)[1]
        assert len(text) > 8 and (has is None or has in text), text

    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p, tab01, FULL, 8, has="before any geometry pass")
    # table contents, at upload and at bind
    bad = mats.copy()
    bad["texture_slot"][3] = 4
    refused(fr.FRR_ERR_INVALID, r.upload_materials, bad, has="entry 3")
    bad = mats.copy()
    bad["texture_slot"][2] = -1
    bad["reserved"][5] = 1
    refused(fr.FRR_ERR_INVALID, r.upload_materials, bad, has="entry 2")
    bad = mats.copy()
    bad["reserved"][4] = 1
    dev = torch.from_numpy(bad.view(np.uint8).copy()).to("cuda")
    torch.cuda.synchronize()
    refused(fr.FRR_ERR_INVALID, r.bind_materials_device, dev.data_ptr(), sc.nitems, has="entry 4")
    refused(fr.FRR_ERR_INVALID, r.bind_materials_device, dev.data_ptr() + 8, 2, has="16-byte")
    refused(fr.FRR_ERR_INVALID, r.bind_materials_device, 0, 2)
    assert r.bind_materials_device(dev.data_ptr(), 4).n == 4      # the first four entries are fine
    empty = r.upload_materials(np.zeros(0, fr.MATERIAL_DTYPE))    # n == 0 is a table
    nan = mats.copy()
    nan["ambient_strength"][0], nan["flat_color"][1] = np.nan, np.inf
    r.upload_materials(nan).free()                                # NaN / inf are not refused
    _prepass(r, dl, buf)
    # the rules of shade_varyings, in its order
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p, tab01, FULL, 8, (5, 5), (0, H))
    refused(fr.FRR_ERR_UNSUPPORTED, r.shade_items, fr.PS_PHONG, p, tab01, FULL, 8, (-1, W - 1), (0, H))
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_DEPTH, p, tab01, FULL, 8)
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p, tab01, FULL, 3)
    refused(fr.FRR_ERR_INVALID, r.shade_items, 9999, p, tab01, FULL, 8)
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p, tab01, FULL - 1, 8)
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, 0, tab01, FULL, 8)
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p + 2, tab01, FULL, 8)
    # table ids and sizes
    freed = r.upload_materials(mats)
    freed.free()
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p, freed, has="table id")
    assert r._lib.frr_shade_items(r._ctx, fr.PS_PHONG, 0, W, 0, H, C.c_void_p(p), FULL, 8, 99) == fr.FRR_ERR_INVALID
    assert r._lib.frr_materials_free(r._ctx, 99) == fr.FRR_ERR_INVALID
    short = r.upload_materials(ok2[:-1])
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p, short, has="fewer entries")
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_FLAT, None, empty, FULL, 0, has="fewer entries")
    # a lit shader with an unfilled slot; PS_FLAT does not care
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p, tab, has="slot 2")
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_BLINN, p, tab, has="slot 2")
    r.shade_items(fr.PS_FLAT, None, tab, FULL, 0)
    # after a filtered draw on a partitioned ctx
    r.set_partition(0, 2)
    r.clear(*D.CLEAR)
    r.draw_list(dl, fr.PS_DEPTH)
    refused(fr.FRR_ERR_INVALID, r.shade_items, fr.PS_PHONG, p, tab01, has="unfiltered")
    r.set_partition(0, 1)
    # after a clear since the pass: FRR_OK, nothing written
    _prepass(r, dl, buf)
    r.clear((1, 2, 3, 4), 0.0)
    r.shade_items(fr.PS_PHONG, p, tab01)
    assert (_snap(r)["c"] == np.array((1, 2, 3, 4), np.uint8)).all()
    # ... and the ctx still draws: the whole frame under three textures
    r.set_texture(2, D.place_textures()[2])
    _prepass(r, dl, buf)
    r.shade_items(fr.PS_PHONG, p, tab)
    _assert_B(_snap(r), fb)
    r.close()


# ---- 15. a host-form shade refused on the host after its array was staged -------------------------------------------------------
def test_host_form_refused_after_staging_leaves_the_next_shade_alone(oracle):
    """The pass's draw list is freed behind the pre-pass, so the argument rules still pass, the host form stages the caller's
    array on the device, and the executor then refuses the command: nothing is logged, nothing is written, and the staged copy
    goes with the call.  Behind a sync the same shade from host memory, over a pass of a list that exists, is the oracle's
    frame (B) -- with a logged host-form shade_varyings, whose copy stays, on either side of the refused call."""
    import f_renderer_amd as fr
    sc = D.scene("clipped")
    mats = IT.materials(sc.nitems)
    fb, _ = IT.expected_B("clipped")
    r = _renderer()
    tab = r.upload_materials(mats)
    dl, _ = _list(r, sc)
    buf = _sentinel()
    _prepass(r, dl, buf)
    host = buf.cpu().numpy()
    dl.free()                                                     # (finishes first: the pass and its resolve are done)
    r.shade_varyings(fr.PS_PHONG, host)                           # logged; reads its own staged copy
    with pytest.raises(fr.FrrError) as err:
        r.shade_items(fr.PS_PHONG, host, tab)
    assert err.value.code == fr.FRR_ERR_INVALID and "freed" in str(err.value), err.value
    r.shade_varyings(fr.PS_PHONG, host)
    r.sync()
    before = _snap(r)
    assert (before["c"] != np.array(D.CLEAR[0], np.uint8)).any()
    with pytest.raises(fr.FrrError):
        r.shade_items(fr.PS_PHONG, host, tab)
    _unchanged(before, _snap(r))
    np.testing.assert_array_equal(before["c"], _snap(r)["c"])
    dl2, _ = _list(r, sc)
    _prepass(r, dl2, buf)
    r.shade_items(fr.PS_PHONG, buf.cpu().numpy(), tab)
    _assert_B(_snap(r), fb)
    r.close()
