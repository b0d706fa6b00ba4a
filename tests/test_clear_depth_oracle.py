"""The scenes of the clear-depth tests (tests/clear_depth_scenes.py) on the CPU: the two oracles agree bit for bit on a frame
that starts from every class of clear depth, and every class meets its input conditions for the C oracle alone -- which is
what makes test_gpu_clear_depth.py test what it says."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from . import clear_depth_scenes as cs
from .conftest import assert_depth_equal

_setup = {}


def _np_setup(W, H):
    """oracle_np's setup list of the coloured base scene (its geometry stage is a Python loop: once per frame size)."""
    if (W, H) not in _setup:
        u, out = onp.Uniforms(), []
        with np.errstate(over="ignore"):                     # (the 3e38 vertices overflow the fan centre's sum, as in the reference)
            for t in cs.scene_color():
                out.extend(onp.geometry_processing(W, H, t, onp.VS_CLIP_COLOR, u))
        _setup[(W, H)] = out
    return _setup[(W, H)]


@pytest.mark.parametrize("cls", cs.CLASSES)
@pytest.mark.parametrize("size", cs.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_c_and_numpy_oracles_agree_over_every_clear_depth(oracle, size, cls):
    """C oracle == NumPy oracle on ids, depth bits (a NaN only has to be a NaN) and RGBA8, VS_CLIP_COLOR / PS_COLOR; the
    depth-only frame of the C oracle has the same ids and depths (the pixel shader does not take part in the z rule)."""
    W, H = size
    clear = cs.clear_depths(oracle, W, H)[cls]
    f = cs.oracle_frame(oracle, W, H, clear, "color")
    color = np.zeros((H, W, 4), np.uint8)
    color[...] = cs.RGBA
    depth, tid = np.full(W * H, clear, np.float32), np.full(W * H, cs.NOBODY, np.uint32)
    setup, u, cov = _np_setup(W, H), onp.Uniforms(), 0
    for i, tri in enumerate(setup):
        cov += onp.rasterization((0, W), (0, H), tri, onp.PS_COLOR, u, color, depth, tid, i, W)
    assert len(setup) == f.counters.tris_setup and cov == f.counters.frag_covered
    np.testing.assert_array_equal(tid, f.tri_id)
    assert_depth_equal(depth, f.depth)
    np.testing.assert_array_equal(color, f.color)
    fd = cs.oracle_frame(oracle, W, H, clear, "depth")
    np.testing.assert_array_equal(fd.tri_id, f.tri_id)
    assert_depth_equal(fd.depth, f.depth)
    assert (fd.color.reshape(-1, 4) == np.array(cs.RGBA, np.uint8)).all()


@pytest.mark.parametrize("size", cs.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_class_meets_its_conditions(oracle, size):
    """From the C oracle alone: `mid` and `neg_mid` have a fragment that ties with the clear and passes, `mid` loses and
    keeps at least a quarter of the pixels covered at 0.0 each, `neg_mid` wins pixels that 0.0 does not, -inf and NaN win
    every pixel a non-dropped fragment covers (the same set, larger than at 0.0) with negative depths among them, +inf and
    FLT_MAX still have winners -- NaN ones, and non-NaN ones behind them, some negative --, pixels nobody won keep the clear's
    bits (a NaN stays a NaN), every frame has NaN fragments and one tile holds more than DIRECT_MAX records."""
    W, H = size
    got = cs.conditions(oracle, W, H)
    print(got)
    cd = cs.clear_depths(oracle, W, H)
    assert cd["mid"] > 0 and np.isfinite(cd["mid"]) and cd["neg_mid"] < 0 and np.isfinite(cd["neg_mid"])
    assert cs.hot_tile_records(oracle, W, H, which=1) > cs.DIRECT_MAX     # the second scene of the frames-in-flight test


@pytest.mark.parametrize("cls", ["mid", "nan"])
def test_negative_x0_window_scene(oracle, cls):
    """The x0 < 0 case of the GPU file: both oracles agree on it (rows share depth entries, renderer.rs:362), it has NaN
    fragments, winners left of x = 0 of the window, and at `mid` it loses pixels that a clear to 0.0 keeps."""
    W, H = cs.SIZES[0]
    x0, x1, y0, y1 = win = cs.NEG_WINDOW
    assert x1 > 0 and (y1 - y0 - 1) * x1 + (x1 - x0) <= W * H and x1 - x0 <= W and y1 - y0 <= H and x1 < x1 - x0
    clear = cs.clear_depths(oracle, W, H)[cls]
    tris = cs.scene_shifted()
    f = cs.oracle_frame(oracle, W, H, clear, "depth", window=win, tris=tris)
    f0 = cs.oracle_frame(oracle, W, H, 0.0, "depth", window=win, tris=tris)
    won, won0 = f.tri_id != cs.NOBODY, f0.tri_id != cs.NOBODY
    assert f.counters.frag_nan > 0 and won.sum() > 1000
    if cls == "mid":
        assert (won0 & ~won).sum() > 1000 and (won0 & won).sum() > 1000
    else:
        assert (won & ~won0).sum() > 0
    color = np.zeros((H, W, 4), np.uint8)
    color[...] = cs.RGBA
    depth, tid = np.full(W * H, clear, np.float32), np.full(W * H, cs.NOBODY, np.uint32)
    with np.errstate(over="ignore"):
        _, cov = onp.draw(W, H, tris, onp.VS_CLIP, onp.PS_DEPTH, onp.Uniforms(), color, depth, tid, window=win)
    assert cov == f.counters.frag_covered
    np.testing.assert_array_equal(tid, f.tri_id)
    assert_depth_equal(depth, f.depth)
