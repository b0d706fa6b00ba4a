"""Lifetimes of the host layer's device memory and events (f_renderer_amd/csrc/frr_own.h): slots of freed meshes and line
lists taken again, a texture replaced in its slot, workspace buffers that grow between the passes of one frame, and two
contexts one after the other in one process.  Every frame is 64 x 64 (2 x 2 tiles) and is compared bit for bit with the
oracle's: the C oracle's frame for colour, depth and triangle ids, tests/lines_reference.py for the lines on top, the NumPy
oracle's interpolated ctx (as tests/varyings_scenes.py takes it) for the varyings buffers.  The oracle frames are computed
once per process and never modified."""
import functools

import numpy as np
import pytest

from oracle import oracle_np as onp
from f_renderer_amd import scenes
from . import indexed_scenes as S
from . import lines_reference as R
from . import varyings_scenes as V
from .conftest import assert_depth_equal

pytestmark = pytest.mark.gpu
W, H = 64, 64
BG = (30, 30, 30, 255)
NONE = 0xFFFFFFFF


def _texture(w, h, seed):
    t = (scenes.splitmix_u01(0x7E70000 + seed, w * h * 4) * 256.0).astype(np.uint8).reshape(h, w, 4)
    t[..., 3] = 255
    return t


def _camera(mod):
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    return dict(view=mod.set_look_at(eye, at, up), proj=mod.set_perspective(fovy, aspect, zn, zf), view_pos=eye)


def _segments(n, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, W, (n, 4)).astype(np.uint32), g.integers(1, 255, (n, 4)).astype(np.uint8)


OLD_TEX, NEW_TEX = _texture(4, 4, 1), _texture(8, 16, 2)        # (height >= width: sample_2d clamps y with the width)
OLD_LINES, NEW_LINES = _segments(70, 1), _segments(90, 2)


@functools.lru_cache(maxsize=None)
def _new_mesh():
    return scenes.displaced_sphere(n=12)                        # VS_PHONG inputs [288, 3, 8]: two geometry blocks


_FINAL = {}


def _final_oracle(oracle):
    """the frame of the new data alone: the new mesh with Phong under the 8 x 16 texture, then the new lines"""
    if not _FINAL:
        f = oracle.Frame(W, H)
        f.clear(BG, 0.0)
        f.draw(_new_mesh(), oracle.VS_PHONG, oracle.PS_PHONG, oracle.make_uniforms(tex=oracle.Texture(NEW_TEX), **_camera(oracle)))
        under = f.color.copy()
        R.draw_lines(f.color, NEW_LINES[0].tolist(), NEW_LINES[1])
        assert (f.tri_id != NONE).sum() > 500 and (f.color != under).any(axis=2).sum() > 200   # a mesh and lines to compare
        # ... and the texture matters: the same draw under the old one gives another image
        g = oracle.Frame(W, H)
        g.clear(BG, 0.0)
        g.draw(_new_mesh(), oracle.VS_PHONG, oracle.PS_PHONG, oracle.make_uniforms(tex=oracle.Texture(OLD_TEX), **_camera(oracle)))
        assert (g.color != under).any(axis=2).sum() > 200
        _FINAL["f"] = f
    return _FINAL["f"]


def _draw_final(r, mesh, lines):
    import f_renderer_amd as fr
    r.set_uniforms(texture_slot=0, **_camera(fr))
    r.clear(BG, 0.0)
    r.draw(mesh, fr.PS_PHONG)
    r.draw_lines(lines)
    return r.readback()


def _assert_frame(got, f):
    c, d, t = got
    np.testing.assert_array_equal(t, f.tri_id, err_msg="triangle ids")
    assert_depth_equal(d, f.depth)
    np.testing.assert_array_equal(c, f.color, err_msg="colour")


def test_freed_slots_are_taken_again_and_a_texture_is_replaced(oracle):
    import f_renderer_amd as fr
    want = _final_oracle(oracle)
    r = fr.Renderer(W, H)
    keep = r.upload_mesh(scenes.torus(8, 6), fr.VS_GOURAUD)                  # an expanded mesh that stays
    v, f = S.grid_clip(8, 8)
    old_mesh = r.upload_mesh_indexed(v, f, fr.VS_CLIP)                       # an indexed one and a line list that go
    old_lines = r.upload_lines(*OLD_LINES)
    r.set_texture(0, OLD_TEX)
    r.clear(BG, 0.0)                                                         # (all of them used once: the frees come behind work)
    r.draw(keep, fr.PS_DEPTH)
    r.draw(old_mesh, fr.PS_DEPTH)
    r.draw_lines(old_lines)
    ids = (old_mesh.id, old_lines.id)
    old_mesh.free()
    old_lines.free()
    assert r._lib.frr_mesh_free(r._ctx, ids[0]) == fr.FRR_ERR_INVALID and r._lib.frr_lines_free(r._ctx, ids[1]) == fr.FRR_ERR_INVALID   # (free once)
    mesh = r.upload_mesh(_new_mesh(), fr.VS_PHONG)                           # expanded, in the slot of an indexed one
    lines = r.upload_lines(*NEW_LINES)
    assert (mesh.id, lines.id) == ids and keep.id != mesh.id
    r.set_texture(0, NEW_TEX)                                                # 4 x 4 -> 8 x 16 in the same slot
    _assert_frame(_draw_final(r, mesh, lines), want)
    mesh.free(); lines.free(); keep.free()
    r.close()


@functools.lru_cache(maxsize=None)
def _growth_scene():
    """Three K = 3 draws into one frame without a clear between them: small, large, the small one again.  Per draw: the oracle's
    targets and the varyings buffer a resolve behind that draw leaves (the sentinel where no triangle of THAT draw owns the
    entry)."""
    small = V.clip_color_scene(seed=31, n=200, radius_px=(4.0, 9.0))
    large = V.clip_color_scene(seed=32, n=4096, radius_px=(1.0, 2.5))
    color = np.zeros((H, W, 4), np.uint8)
    color[:] = BG
    depth, tri_id = np.zeros(W * H, np.float32), np.full(W * H, NONE, np.uint32)
    debug, base, steps = {}, 0, []
    for mesh in (small, large, small):
        setup, _ = onp.draw(W, H, mesh, onp.VS_CLIP_COLOR, onp.PS_COLOR, onp.Uniforms(), color, depth, tri_id, tri_id_base=base, debug=debug)
        owned = (tri_id != NONE) & (tri_id >= base)
        buf = np.full((W * H, 3), V.SENTINEL, np.float32)
        buf[owned] = debug["ctx"][owned]
        assert owned.sum() > 300 and not np.isnan(buf[owned]).any()
        steps.append(dict(buf=buf, earlier=int(((tri_id != NONE) & (tri_id < base)).sum())))
        base += len(setup)
    assert steps[1]["earlier"] > 100 and steps[2]["earlier"] > 100   # (entries of earlier draws survive: a resolve must leave them alone)
    return small, large, steps, (color, depth, tri_id)


@pytest.mark.parametrize("fan_capacity", [0, 64])
def test_workspace_grows_between_the_passes_of_one_frame(fan_capacity):
    """exec_geometry sizes the fan space by region: FRR_MAX_OUT_TRIS (19) * GEOM_BLOCK (256) slots for every block that allocates
    in a region, blocks taking the FAN_REGIONS = 8 regions in turn.  200 triangles are one block: 19 * 256 = 4,864 slots per
    region (less than the 2^20 / 8 a small mesh may have outright), 200 + 8 * 4,864 = 39,112 setup slots.  4,096 triangles are
    sixteen blocks, two per region: 9,728 per region, 4,096 + 77,824 = 81,920 setup slots, seventeen block sums instead of
    two.  So the second geometry pass finds every buffer of its workspace set too small (block sums and prefix, tinfo, fanbase,
    fan keys, records, boxes, bin counts, varyings) and replaces each, behind a drain, while the first pass's commands are in
    the log; consecutive passes alternate between the two slot tables of the set, so the third pass resolves with the table
    the first one sized for 39,112 slots under a set of 81,920 and replaces that too.  (By default -- frames in flight on the
    ctx's own targets -- all passes of a frame use one workspace set; with option frames_in_flight 1 passes with varyings
    alternate between the two sets instead and nothing grows: the results are the same.)  The case depends on FRR_MAX_OUT_TRIS,
    GEOM_BLOCK, FAN_REGIONS, the 2^20-slot allowance of small meshes and the choice of set (`fif2 ? f.tset`) in exec_geometry:
    the results say nothing about whether a buffer was replaced, so a change to any of them means choosing the meshes anew.
    fan_capacity 64 (8 slots per region) takes the other way to the same growth: every pass overflows its fan space on the
    device, and the replay inside the library replaces the fan-sized buffers with the failed pass still in the log."""
    import torch
    import f_renderer_amd as fr
    small, large, steps, (color, depth, tri_id) = _growth_scene()
    r = fr.Renderer(W, H)
    r.set_option("fan_capacity", fan_capacity)
    meshes = [r.upload_mesh(small, fr.VS_CLIP_COLOR), r.upload_mesh(large, fr.VS_CLIP_COLOR)]
    bufs = [torch.full((W * H, 3), V.SENTINEL, dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    r.clear(BG, 0.0)
    for k, m in enumerate((meshes[0], meshes[1], meshes[0])):
        r.geometry_processing(m)
        r.rasterization((0, W), (0, H), fr.PS_COLOR)
        r.resolve_varyings(bufs[k].data_ptr(), W * H)
    c, d, t = r.readback()                                      # (the synchronisation point: the buffers are final too)
    np.testing.assert_array_equal(t, tri_id, err_msg="triangle ids")
    assert_depth_equal(d, depth)
    np.testing.assert_array_equal(c, color, err_msg="colour")
    for k in range(3):
        V.assert_bits_equal(bufs[k].cpu().numpy(), steps[k]["buf"], f"varyings buffer of pass {k}")
    st = r.stats()
    assert st["draws"] == 3 and (not fan_capacity or st["replays"] > 0), st   # (the small fan space was in fact outgrown)
    r.close()


def test_two_contexts_one_after_the_other(oracle):
    """the second context takes the first one's streams out of the pool, after the first one's buffers and events went with it"""
    import f_renderer_amd as fr
    want = _final_oracle(oracle)
    frames = []
    for _ in range(2):
        r = fr.Renderer(W, H)
        r.set_texture(0, NEW_TEX)
        frames.append(_draw_final(r, r.upload_mesh(_new_mesh(), fr.VS_PHONG), r.upload_lines(*NEW_LINES)))
        r.close()
    for got in frames:
        _assert_frame(got, want)
    for a, b in zip(*frames):
        assert a.tobytes() == b.tobytes()
