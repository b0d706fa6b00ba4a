"""The clipping path of the geometry pass against the C oracle (scenes: tests/clip_scenes.py; what they reach, and the
agreement of the two CPU restatements on them, is checked without a GPU by tests/test_clip_oracle.py).  The bar is
test_gpu_parity's, no tolerance: the setup records (spi, spf, rhw, ctx[:K]) bit for bit, tris_in / tris_setup / frag_covered /
frag_nan, triangle ids, depth bits and RGBA8 byte for byte.  In the setup records a NaN is compared by its bits too (sign and
payload are the reference machine's: frr_exact.h, x86_nan); only a NaN DEPTH has to be just a NaN (conftest.assert_depth_equal).

The device counts the kept intersections of an input twice: classify (per thread: the block scan, the fan slots, tinfo, the
emission offsets and every later triangle id rest on it) and clip_triangle_wave (one lane per candidate vertex, kept by a
ballot, popcount - 2 records into the slots the first count reserved).  A disagreement between them writes fan slots nobody
reserved, so what is compared first is always the setup list and its length.  What the scenes reach: all 54 inside classes at
every vertex (fans of 1 .. 11), vertices and edges exactly on the planes and equal sort keys (only the stable rank
`ok == key && k < li` orders them), the |w| > 1e-5 keep rule on both sides with kept vertices whose screen coordinates
saturate, NaN / inf / FLT_MAX / subnormal / signed-zero components, and geometry blocks in which all 256 inputs become large
fans (block sums, s_cl / s_ce, the fan-region cursors, the clip queue hand-off, the 13-bit emission offset of the records).

Every frame is 96 x 64: a case is milliseconds of GPU time, but for the full cube (157,464 inputs, 1.3 M records over six tiles).
"""
import numpy as np
import pytest

from . import clip_scenes as cs
from .conftest import assert_depth_equal, owned_pixel_rows

pytestmark = pytest.mark.gpu

SCENES = cs.names()
VARIANT_SCENES = cs.names("patterns", "epsilon", "dense")
PARTITION_SCENES = cs.names("patterns", "epsilon")
# option sets; count: fragment counting (off: early-z runs, and frag_covered / frag_nan are not kept)
VARIANTS = {"clip_queue_auto": dict(options={"clip_queue": -1}), "clip_queue_off": dict(options={"clip_queue": 0}),
            "clip_queue_on": dict(options={"clip_queue": 1}), "sweep": dict(options={"raster_sweep": 1}),
            "nw16": dict(options={"raster_nw": 16}), "early_z": dict(count=False),
            "replayed": dict(options={"fan_capacity": 16, "bin_capacity": 64}, replays=True),
            "replayed_clip_queue_on": dict(options={"fan_capacity": 16, "bin_capacity": 64, "clip_queue": 1}, replays=True)}
_oracle_cache = {}


def _want(oracle, name):
    """The C oracle's frame and setup list of a scene, once per module."""
    if name not in _oracle_cache:
        _oracle_cache[name] = cs.oracle_frame(oracle, cs.all_scenes()[name])
    return _oracle_cache[name]


@pytest.fixture(scope="module")
def renderers():
    """One Renderer per option set for the whole module (every frame has the same size)."""
    import f_renderer_amd as fr
    made = {}

    def get(variant="default"):
        if variant not in made:
            r = fr.Renderer(cs.W, cs.H)
            v = VARIANTS.get(variant, {})
            for k, val in v.get("options", {}).items():
                r.set_option(k, val)
            r.set_count_fragments(v.get("count", True))
            made[variant] = r
        return made[variant]
    yield get
    for r in made.values():
        r.close()


def _same_bits(got, want, what):
    """The raw words, NaNs included (test_gpu_parity._assert_setup_equal's rule)."""
    got, want = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(want, np.float32).ravel()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def _assert_setup(g, want, K, note):
    assert g.shape[0] == want.shape[0], f"{note}: {g.shape[0]} setup triangles, oracle {want.shape[0]}"
    np.testing.assert_array_equal(g["spi"], want["spi"], err_msg=f"{note}: spi")
    _same_bits(g["spf"], want["spf"], f"{note}: spf")
    _same_bits(g["rhw"], want["rhw"], f"{note}: rhw")
    if K:
        _same_bits(g["ctx"][..., :K], want["ctx"][..., :K], f"{note}: ctx")


def _assert_frame(got, f, note, rows=None):
    c, d, t = got[:3]
    rows = slice(None) if rows is None else rows
    np.testing.assert_array_equal(t.reshape(cs.H, cs.W)[rows], f.tri_id.reshape(cs.H, cs.W)[rows], err_msg=f"{note}: triangle ids differ")
    assert_depth_equal(d.reshape(cs.H, cs.W)[rows], f.depth.reshape(cs.H, cs.W)[rows], err_msg=f"{note}: depth bits differ")
    np.testing.assert_array_equal(c[rows], f.color[rows], err_msg=f"{note}: RGBA8 differs")


def _assert_stats(st, f, note, count=True):
    oc = f.counters.as_dict()
    for k in ("tris_in", "tris_setup") + (("frag_covered", "frag_nan") if count else ()):
        assert st[k] == oc[k], (note, k, st, oc)


def _K(oracle, sc):
    return oracle.vs_num_varyings(getattr(oracle, "VS_" + sc.vs))


def _check(oracle, r, name, note, count=True, **kw):
    sc, want = cs.all_scenes()[name], _want(oracle, name)
    got = cs.gpu_run(r, sc, setup=True, **kw)
    _assert_setup(got[4], want["setup"], _K(oracle, sc), note)
    _assert_stats(got[3], want["frame"], note, count)
    _assert_frame(got, want["frame"], note)
    return got


# ---- every family, both layouts ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_scene_equals_oracle(oracle, renderers, name):
    st = _check(oracle, renderers(), name, name)[3]
    assert st["replays"] == 0, st


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", VARIANT_SCENES)
def test_variant_equals_oracle(oracle, renderers, name, variant):
    """The clip queue forced off and on and left to itself (k_geom_clip expands what the blocks hand over), fan and bin space
    so small that the pass is replayed, the sweep kernel, the 16-wave tile kernel, and early-z (fragment counting off)."""
    import f_renderer_amd as fr
    v = VARIANTS[variant]
    if v.get("replays"):               # (a Renderer of its own: the work lists stay grown after a replay)
        r = fr.Renderer(cs.W, cs.H)
        try:
            for k, val in v["options"].items():
                r.set_option(k, val)
            st = _check(oracle, r, name, f"{name}, {variant}")[3]
        finally:
            r.close()
        assert st["replays"] > 0, st
        return
    r = renderers(variant)
    _check(oracle, r, name, f"{name}, {variant}", count=v.get("count", True))
    if "clip_queue" in variant:        # twice: the automatic mode decides from the counters the first frame read back
        _check(oracle, r, name, f"{name}, {variant}, second frame")


_repeated_cache = {}


def _nonfinite_repeated(oracle, layout):
    """(scene, oracle frame and setup list) of the nonfinite family eight times over, once per module and layout."""
    if layout not in _repeated_cache:
        sc = cs.all_scenes()[f"nonfinite/{layout}"]
        sc = sc._replace(mesh=np.ascontiguousarray(np.tile(sc.mesh, (8, 1, 1))))
        _repeated_cache[layout] = (sc, cs.oracle_frame(oracle, sc))
    return _repeated_cache[layout]


@pytest.mark.parametrize("variant", ["default", "early_z", "nw16"])
@pytest.mark.parametrize("layout", list(cs.LAYOUTS))
def test_nan_fragments_of_many_cull_steps_are_all_resolved(oracle, renderers, layout, variant):
    """The nonfinite family eight times over (7,680 inputs, 36,256 bin entries over six tiles: many cull steps per tile).  A
    fragment whose rhw is NaN passes every z-test (renderer.rs:363), so the LAST copy's NaN fragments own their pixels,
    although those pixels hold the highest depth key by then and although most of these triangles have finite rhw at all
    three vertices (the NaN comes from a screen position).  Their depth bound must be 'never culled' (cull_zub; DESIGN.md
    section 3 has the figures of the bound that looked at the vertex rhw alone): frag_nan counts every one of them."""
    sc, want = _nonfinite_repeated(oracle, layout)
    last = want["frame"].tri_id[np.isnan(want["frame"].depth)]
    assert last.size >= 2000 and (last >= want["setup"].shape[0] * 7 // 8).all()       # NaN pixels, all owned by the last copy
    count = VARIANTS.get(variant, {}).get("count", True)
    note = f"nonfinite/{layout} x 8, {variant}"
    got = cs.gpu_run(renderers(variant), sc, setup=True)
    _assert_setup(got[4], want["setup"], _K(oracle, sc), note)
    _assert_stats(got[3], want["frame"], note, count)
    _assert_frame(got, want["frame"], note)


# ---- the full cube -------------------------------------------------------------------------------------------------------

def test_full_cube_setup_list_and_frame(oracle, renderers):
    """All 54^3 inputs in one draw (PS_DEPTH): 1,285,956 setup records, compared in full, the statistics, and the frame (ids, depth, RGBA8) --
    the hot-tile case, every one of the six tiles culls the whole list.  The oracle's frame is drawn in row bands on host
    threads (cref.draw_banded: the reference's own sub-window feature), its setup list in one batch."""
    import f_renderer_amd as fr
    sc = cs.cube_scene("clip")
    u = oracle.make_uniforms()
    want = oracle.geometry_batch(cs.W, cs.H, sc.mesh, oracle.VS_CLIP, u)
    color, depth, tri_id, covered, _ = oracle.draw_banded(cs.W, cs.H, sc.mesh, oracle.VS_CLIP, oracle.PS_DEPTH, u, rgba=cs.CLEAR, threads=8)
    r = renderers()
    m = r.upload_mesh(sc.mesh, fr.VS_CLIP)
    try:
        r.clear(cs.CLEAR, 0.0)
        r.draw(m, fr.PS_DEPTH)
        c, d, t = r.readback()
        st = r.stats()
        g = r.setup_triangles()
    finally:
        m.free()
    assert want.shape[0] == 1285956
    _assert_setup(g, want, 0, "full cube")
    assert st["tris_in"] == cs.CUBE_N and st["tris_setup"] == want.shape[0] and st["frag_covered"] == covered and st["frag_nan"] == 0, st
    np.testing.assert_array_equal(t, tri_id, err_msg="full cube: triangle ids differ")
    assert_depth_equal(d, depth, err_msg="full cube: depth bits differ")
    np.testing.assert_array_equal(c, color, err_msg="full cube: RGBA8 differs")     # (PS_DEPTH writes no colour: the clear colour on both sides)


# ---- partition -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("world", [3, 5])
@pytest.mark.parametrize("name", PARTITION_SCENES)
def test_partition_ranks_stitch_to_the_oracle(oracle, name, world, blocked):
    """Every rank of worlds 3 and 5 (two tile rows: most ranks own none): the owned rows are the oracle's, the others keep the
    clear values, tris_setup is the oracle's on every rank (k_geom_single skips the fan of a clipped input whose rows the
    rank does not own -- only with all w > 0 and nothing behind the near plane -- but keeps its count), and the ranks' covered
    fragments add up."""
    import f_renderer_amd as fr
    sc, f = cs.all_scenes()[name], _want(oracle, name)["frame"]
    oc = f.counters.as_dict()
    acc_c = np.zeros((cs.H, cs.W, 4), np.uint8)
    acc_d, acc_t = np.zeros((cs.H, cs.W), np.float32), np.zeros((cs.H, cs.W), np.uint32)
    covered, seen = 0, np.zeros(cs.H, bool)
    r = fr.Renderer(cs.W, cs.H)
    try:
        for rank in range(world):
            r.set_partition(rank, world, blocked=blocked)
            c, d, t, st = cs.gpu_run(r, sc)
            own = owned_pixel_rows(cs.H, rank, world, blocked)
            note = f"{name}, rank {rank} of {world}, {'blocked' if blocked else 'interleaved'}"
            assert st["tris_setup"] == oc["tris_setup"] and st["tris_in"] == oc["tris_in"], (note, st, oc)
            _assert_frame((c, d, t), f, note, rows=own)
            assert (c[~own] == np.array(cs.CLEAR, np.uint8)).all(), note + ": a row the rank does not own was written"
            assert (d.reshape(cs.H, cs.W)[~own].view(np.uint32) == 0).all() and (t.reshape(cs.H, cs.W)[~own] == 0xFFFFFFFF).all(), note
            assert not (seen & own).any()
            seen |= own
            covered += st["frag_covered"]
            acc_c[own], acc_d[own], acc_t[own] = c[own], d.reshape(cs.H, cs.W)[own], t.reshape(cs.H, cs.W)[own]
    finally:
        r.close()
    assert seen.all()
    _assert_frame((acc_c, acc_d, acc_t), f, f"{name} stitched")
    assert covered == oc["frag_covered"]


# ---- the other forms of k_geom_single / k_geom_clip, on the dense family ----------------------------------------------------

@pytest.mark.parametrize("clip_queue", [0, 1])
@pytest.mark.parametrize("layout", list(cs.LAYOUTS))
def test_dense_indexed_mesh_equals_oracle(oracle, renderers, layout, clip_queue):
    """upload_mesh_indexed of the same triangles (one vertex record per corner, named in order)."""
    import f_renderer_amd as fr
    name = f"dense/{layout}"
    sc = cs.all_scenes()[name]
    nf = sc.mesh.shape[2]
    r = renderers("clip_queue_on" if clip_queue else "clip_queue_off")
    m = r.upload_mesh_indexed(sc.mesh.reshape(-1, nf), np.arange(3 * sc.mesh.shape[0], dtype=np.uint32).reshape(-1, 3), getattr(fr, "VS_" + sc.vs))
    try:
        _check(oracle, r, name, f"{name} indexed, clip_queue {clip_queue}", mesh=m)
    finally:
        m.free()


@pytest.mark.parametrize("clip_queue", [0, 1])
@pytest.mark.parametrize("layout", list(cs.LAYOUTS))
def test_dense_instanced_equals_the_oracles_loop(oracle, renderers, layout, clip_queue):
    """Two instances in one pass against the oracle's two draws.  The vertex shaders of these layouts read no matrix (like
    the tie_clip and clip_color scenes of the instanced tests), so the second copy ties with the first on every fragment and
    wins it (renderer.rs:363): every drawn id belongs to the second instance."""
    import f_renderer_amd as fr
    name = f"dense/{layout}"
    sc = cs.all_scenes()[name]
    vs, ps, u = getattr(oracle, "VS_" + sc.vs), getattr(oracle, "PS_" + sc.ps), oracle.make_uniforms()
    f = oracle.Frame(cs.W, cs.H)
    f.clear(cs.CLEAR, 0.0)
    setups = []
    for _ in range(2):
        setups.append(f.draw(sc.mesh, vs, ps, u, tri_id_base=int(f.counters.tris_setup), keep_setup=True))
    r = renderers("clip_queue_on" if clip_queue else "clip_queue_off")
    m = r.upload_mesh(sc.mesh, getattr(fr, "VS_" + sc.vs))
    inst = r.upload_instances(np.stack([np.eye(4, dtype=np.float32).reshape(-1)] * 2))
    try:
        r.clear(cs.CLEAR, 0.0)
        r.draw_instanced(m, inst, getattr(fr, "PS_" + sc.ps))
        c, d, t = r.readback()
        st, g = r.stats(), r.setup_triangles()
    finally:
        inst.free()
        m.free()
    note = f"{name} instanced, clip_queue {clip_queue}"
    _assert_setup(g, np.concatenate(setups), _K(oracle, sc), note)
    _assert_stats(st, f, note)
    _assert_frame((c, d, t), f, note)
    drawn = t[t != 0xFFFFFFFF]
    assert drawn.size > 1000 and (drawn >= setups[0].shape[0]).all()


@pytest.mark.parametrize("clip_queue", [0, 1])
@pytest.mark.parametrize("layout", list(cs.LAYOUTS))
def test_dense_draw_list_of_three_items_equals_oracle(oracle, renderers, layout, clip_queue):
    """The mesh cut into three items (at inputs that are no block or wave starts, inside the run of large fans) under
    identity matrices: one list pass is the plain draw."""
    import f_renderer_amd as fr
    name = f"dense/{layout}"
    sc, want = cs.all_scenes()[name], _want(oracle, name)
    r = renderers("clip_queue_on" if clip_queue else "clip_queue_off")
    cuts = (0, 301, 650, sc.mesh.shape[0])
    meshes = [r.upload_mesh(sc.mesh[a:b], getattr(fr, "VS_" + sc.vs)) for a, b in zip(cuts[:-1], cuts[1:])]
    dl = r.upload_draw_list(meshes, np.stack([np.eye(4, dtype=np.float32).reshape(-1)] * 3))
    try:
        r.clear(cs.CLEAR, 0.0)
        r.draw_list(dl, getattr(fr, "PS_" + sc.ps))
        c, d, t = r.readback()
        st, g = r.stats(), r.setup_triangles()
    finally:
        r.free_draw_list(dl)
        for m in meshes:
            m.free()
    note = f"{name} as a draw list, clip_queue {clip_queue}"
    _assert_setup(g, want["setup"], _K(oracle, sc), note)
    _assert_stats(st, want["frame"], note)
    _assert_frame((c, d, t), want["frame"], note)
