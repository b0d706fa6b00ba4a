"""The shading arithmetic on hostile attributes against the C oracle (scenes: tests/shading_scenes.py; their input
conditions and the agreement of the two CPU restatements on them are checked without a GPU by tests/test_shading_oracle.py).
The bar is test_gpu_parity's: ids, depth bits (a NaN only has to be a NaN), RGBA8 byte for byte and tris_setup / frag_covered /
frag_nan equal the oracle's, no tolerance.  What the scenes reach inside the kernels:

  normalize3 -> rsqrt_exact with lanes of one wave in and out of its fast range (zero, subnormal, overflowing and non-finite
  dot products next to ordinary ones); f32_max as v_max_f32 on a NaN operand; sample_2d_of's saturating conversions on uv
  that are negative, huge, infinite or NaN, through the LDS table (tile kernel) and through the IEEE division (windows with
  x0 < 0); quantize_u8 on colours outside [0, 1); the perspective divide of the varyings at subnormal 1/w, where the depth
  products, recip_exact's slow path, the depth keys and the hi-z bound all work on denormals; vertex_intersect on all of these;
  and the run-time build of the same Phong shader as a user shader.

Every frame is 96 x 64: a case is milliseconds of GPU time.
"""
import numpy as np
import pytest

from . import shading_scenes as ss
from . import user_shaders
from .conftest import assert_depth_equal, owned_pixel_rows

pytestmark = pytest.mark.gpu

# (raster_nw = 16 and 3: the tile kernel's 16-wave shape and its light-tile shape by name, whichever the default picks for 6 tiles)
PATHS = {"default": {}, "sweep": {"raster_sweep": 1}, "nw16": {"raster_nw": 16}, "nw3": {"raster_nw": 3}}
SCENES = ss.names()
_oracle_cache = {}


def _want(oracle, name, window=None):
    if (name, window) not in _oracle_cache:
        _oracle_cache[(name, window)] = ss.oracle_frame(oracle, ss.all_scenes()[name], window)["frame"]
    return _oracle_cache[(name, window)]


@pytest.fixture(scope="module")
def renderers():
    """One Renderer per path for the whole module (every frame has the same size), and one with the user shader."""
    import f_renderer_amd as fr
    made = {}

    def get(path):
        if path not in made:
            r = fr.Renderer(ss.W, ss.H)
            for k, v in PATHS.get(path, {}).items():
                r.set_option(k, v)
            made[path] = r
        return made[path]
    yield get
    for r in made.values():
        r.close()


@pytest.fixture(scope="module")
def user_phong(renderers):
    """(Renderer, shader id): tests/user_shaders.PHONG registered once -- the hiprtc build, a compile of its own."""
    r = renderers("user")
    return r, r.register_shader(user_shaders.PHONG, 8, 8)


def _assert_equal(got, f, note, stats=True):
    c, d, t, st = got
    first = np.flatnonzero((c.reshape(-1, 4) != f.color.reshape(-1, 4)).any(axis=1))
    where = "" if not first.size else (f": {first.size} pixels, first (x, y) = ({first[0] % f.width}, {first[0] // f.width}), "
                                       f"got {c.reshape(-1, 4)[first[0]].tolist()}, oracle {f.color.reshape(-1, 4)[first[0]].tolist()}")
    np.testing.assert_array_equal(t, f.tri_id, err_msg=f"{note}: triangle ids differ")
    assert_depth_equal(d, f.depth, err_msg=f"{note}: depth bits differ")
    assert not first.size, f"{note}: RGBA8 differs{where}"
    if stats:
        oc = f.counters.as_dict()
        for k in ("tris_in", "tris_setup", "frag_covered", "frag_nan"):
            assert st[k] == oc[k], (note, k, st, oc)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", SCENES)
def test_scene_equals_oracle(oracle, renderers, name, path):
    """Every scene on the span kernel with LUT texels (default, nw16, nw3) and on the sweep."""
    _assert_equal(ss.gpu_run(renderers(path), ss.all_scenes()[name]), _want(oracle, name), f"{name} on {path}")


@pytest.mark.parametrize("name", SCENES)
def test_scene_in_a_window_with_negative_x0_equals_oracle(oracle, renderers, name):
    """Window (-32, 64) x (0, 64): k_raster_entries shades the pass, texels by the IEEE division instead of the LDS table."""
    got = ss.gpu_run(renderers("default"), ss.all_scenes()[name], window=ss.NEG_WINDOW)
    _assert_equal(got, _want(oracle, name, ss.NEG_WINDOW), f"{name} in window {ss.NEG_WINDOW}")


def test_lut_texels_equal_division_texels_on_every_byte_value(oracle, renderers):
    """The 64 x 64 texture with every byte value in every channel: the full-frame pass (u8lut table) and the x0 < 0 pass
    (division) give the same RGBA8 where both draw -- screen columns 0..63, which the window stores at local columns
    32..95 (every depth of this scene is 1.0, so no fragment is rejected in either)."""
    sc = ss.all_scenes()["tex_all_bytes"]
    lut = ss.gpu_run(renderers("default"), sc)
    div = ss.gpu_run(renderers("default"), sc, window=ss.NEG_WINDOW)
    drawn = lut[2].reshape(ss.H, ss.W)[:, :64] != 0xFFFFFFFF
    assert drawn.all()
    np.testing.assert_array_equal(div[0][:, 32:96], lut[0][:, :64])
    np.testing.assert_array_equal(lut[0], _want(oracle, "tex_all_bytes").color)


@pytest.mark.parametrize("name", ss.names("normals", "rhw"))
def test_two_rank_partition_stitches_to_the_oracle(oracle, name):
    import f_renderer_amd as fr
    sc, f = ss.all_scenes()[name], _want(oracle, name)
    oc = f.counters.as_dict()
    acc_c = np.zeros((ss.H, ss.W, 4), np.uint8)
    acc_d, acc_t = np.zeros((ss.H, ss.W), np.float32), np.zeros((ss.H, ss.W), np.uint32)
    covered = 0
    for rank in range(2):
        r = fr.Renderer(ss.W, ss.H)
        try:
            r.set_partition(rank, 2, blocked=bool(rank))
            c, d, t, st = ss.gpu_run(r, sc)
        finally:
            r.close()
        assert st["tris_setup"] == oc["tris_setup"] and st["frag_nan"] <= oc["frag_nan"], (st, oc)
        covered += st["frag_covered"]
        own = owned_pixel_rows(ss.H, rank, 2, False)       # (two tile rows, two ranks: both layouts give rank r row r)
        acc_c[own], acc_d[own], acc_t[own] = c[own], d.reshape(ss.H, ss.W)[own], t.reshape(ss.H, ss.W)[own]
    _assert_equal((acc_c, acc_d.ravel(), acc_t.ravel(), None), f, f"{name} stitched", stats=False)
    assert covered == oc["frag_covered"]


def test_clipped_hostile_fans_are_replayed_with_tiny_capacities(oracle):
    """bin_capacity and fan_capacity far too small: the geometry and binning of the clipped hostile fans run again inside the
    library, with the same result."""
    import f_renderer_amd as fr
    r = fr.Renderer(ss.W, ss.H)
    try:
        r.set_option("bin_capacity", 64)
        r.set_option("fan_capacity", 8)
        got = ss.gpu_run(r, ss.all_scenes()["clip_normals"])
    finally:
        r.close()
    assert got[3]["replays"] > 0, got[3]
    _assert_equal(got, _want(oracle, "clip_normals"), "clip_normals with tiny capacities")


USER_SCENES = [n for n in ss.names("normals", "uv", "texture") if ss.all_scenes()[n].ps == "PHONG"]


@pytest.mark.parametrize("name", USER_SCENES)
def test_user_shader_phong_equals_the_builtin_and_the_oracle(oracle, user_phong, name):
    """tests/user_shaders.PHONG through hiprtc (its own compile, its own flags) on the normals, uv and texture scenes."""
    r, sid = user_phong
    sc = ss.all_scenes()[name]
    builtin = ss.gpu_run(r, sc)
    user = ss.gpu_run(r, sc, shader=sid)
    for k, what in enumerate(("RGBA8", "depth", "ids")):
        a, b = (x[k].view(np.uint32) if k == 1 else x[k] for x in (user, builtin))
        np.testing.assert_array_equal(a, b, err_msg=f"{name}: the user shader's {what} differ from the built-in's")
    _assert_equal(user, _want(oracle, name), f"{name} with the user shader")


USER_PATH_SCENE = "normals_small/phong"


def test_user_shader_on_the_entries_and_sweep_kernels_equals_the_builtin_and_the_oracle(oracle, user_phong):
    """The user-shader builds of k_raster_entries (a window with x0 < 0) and of k_raster (option raster_sweep): the two tile
    kernels of a user module that the test above does not launch.  No compile beyond the fixture's."""
    r, sid = user_phong
    sc = ss.all_scenes()[USER_PATH_SCENE]

    def check(window, note):
        f = _want(oracle, USER_PATH_SCENE, window)
        drawn = f.tri_id.ravel() != 0xFFFFFFFF
        shaded = drawn & (f.color.reshape(-1, 4) != np.array(ss.CLEAR, np.uint8)).any(axis=1)
        assert shaded.any(), f"{note}: the oracle shades no pixel away from the clear colour"
        builtin = ss.gpu_run(r, sc, window=window)
        user = ss.gpu_run(r, sc, window=window, shader=sid)
        _assert_equal(user, f, f"{USER_PATH_SCENE} with the user shader, {note}")
        _assert_equal(builtin, f, f"{USER_PATH_SCENE} with the built-in pair, {note}")
        for k, what in enumerate(("RGBA8", "depth", "ids")):
            a, b = (x[k].view(np.uint32) if k == 1 else x[k] for x in (user, builtin))
            np.testing.assert_array_equal(a, b, err_msg=f"{note}: the user shader's {what} differ from the built-in's")

    check(ss.NEG_WINDOW, f"window {ss.NEG_WINDOW} (entries kernel)")
    r.set_option("raster_sweep", 1)
    try:
        check(None, "raster_sweep (sweep kernel)")
    finally:
        r.set_option("raster_sweep", 0)
