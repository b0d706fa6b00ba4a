"""The library against answers derived in exact arithmetic, not against the oracle.

tests/exact_scenes.py holds scenes in which (nearly) every f32 operation of the reference is exact, and tests/exact_reference.py
evaluates them in rationals straight from the reference's text (tests/test_exact_cpu.py holds the two CPU oracles, the
evaluator's rounding and a set of hand-worked pixels to it without a GPU).  Here frr_readback, frr_readback_setup,
frr_get_stats and the varyings of frr_resolve_varyings are compared with the evaluator directly, on every raster path that
tests/test_gpu_paths.py selects: on the exact values equality is the assertion -- a weight paired with the wrong vertex, an
off-by-half in px or the wrong operand in a plane's ratio cannot hide behind an oracle that shares the misreading -- and the
rounded remainder is compared too, where the evaluator follows the Rust text's association.

Every frame is 64 x 64 and a few triangles: a case is milliseconds of GPU time."""
import numpy as np
import pytest

from . import exact_scenes as es
from .conftest import owned_pixel_rows

pytestmark = pytest.mark.gpu

SCENES = es.names()
# option sets; count: fragment counting (off: early-z runs, and frag_covered is not kept); frames: frames drawn back to back
# before the read-back; replays: work lists of one record, so every scene overflows them and the pass runs again
VARIANTS = {"default": {}, "sweep": dict(options={"raster_sweep": 1}), "atomic_binning": dict(options={"bin_atomics": 1}),
            "early_z": dict(count=False), "two_frames_in_flight": dict(options={"frames_in_flight": 2}, frames=2),
            "tiny_work_lists": dict(options={"fan_capacity": 1, "bin_capacity": 1}, replays=True)}
for _nw, _occ in ((3, 6), (4, 6), (4, 8), (6, 6), (8, 6), (16, 4)):            # the tile kernel's shapes, as test_gpu_paths forces them
    VARIANTS[f"nw{_nw}_occ{_occ}"] = dict(options={"raster_nw": _nw, "raster_occ": _occ})


def _make(variant):
    import f_renderer_amd as fr
    v = VARIANTS[variant]
    r = fr.Renderer(es.W0, es.H0)
    for k, val in v.get("options", {}).items():
        r.set_option(k, val)
    r.set_count_fragments(v.get("count", True))
    return r


@pytest.fixture(scope="module")
def renderers():
    """One Renderer per option set for the whole module (every frame has the same size)."""
    made = {}

    def get(variant="default"):
        if variant not in made:
            made[variant] = _make(variant)
        return made[variant]
    yield get
    for r in made.values():
        r.close()


def _prepare(r, sc):
    """Every uniform is set: a Renderer is reused across scenes."""
    import f_renderer_amd as fr
    u = sc.uniforms
    if sc.tex is not None:
        r.set_texture(0, es.texture_u8(sc))
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    r.set_uniforms(model=eye, view=eye, proj=eye, view_pos=(0, 0, 0),
                   light_pos=[float(x) for x in u.get("light_pos", (0, 0, 0))], light_color=[float(x) for x in u.get("light_color", (1, 1, 1))],
                   ambient_strength=float(u.get("ambient", 0)), specular_strength=float(u.get("specular", 0)), texture_slot=0)
    return getattr(fr, "VS_" + sc.vs), getattr(fr, "PS_" + sc.ps.upper())


def _windows(sc):
    x0, x1, y0, y1 = sc.window or (0, sc.W, 0, sc.H)
    return (x0, x1), (y0, y1)


def _run(r, sc, how="draw", frames=1):
    """Clear, draw and read a scene back.  how: "draw" (one frr_draw per model matrix of the scene, the matrix in the
    uniforms), "instanced" or "list" (one pass over all of them).  -> dict of color, depth, ids, stats, setup (the latest
    pass's list), inputs (the pixel shader's input by depth entry, NaN where nobody owns it; None where not asked for)."""
    vs, ps = _prepare(r, sc)
    wr, hr = _windows(sc)
    models = sc.models_f32()
    mesh = r.upload_mesh(es.inputs_f32(sc), vs)
    table = None
    try:
        if how == "instanced":
            table = r.upload_instances(models)
        elif how == "list":
            table = r.upload_draw_list([mesh] * len(models), models)
        for _ in range(frames):
            r.clear(es.CLEAR_COLOR, 0.0)
            if how == "instanced":
                r.draw_instanced(mesh, table, ps, wr, hr)
            elif how == "list":
                r.draw_list(table, ps, wr, hr)
            else:
                for m in models:
                    r.set_uniforms(model=m)
                    r.draw(mesh, ps, wr, hr)
        buf = None
        if sc.ps != "depth" and wr[0] >= 0 and (how != "draw" or len(models) == 1):
            import torch
            entries = (hr[1] - hr[0]) * wr[1]
            buf = torch.full((entries, r.geometry_num_varyings()), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()                               # (ready before anything the library enqueues)
            r.resolve_varyings(buf.data_ptr(), entries, wr, hr)    # frr_resolve_varyings; the read-back below is the wait
        c, d, t = r.readback()
        out = dict(color=c, depth=d, ids=t, stats=r.stats(), setup=r.setup_triangles(), inputs=None)
        if buf is not None:
            got = buf.cpu().numpy()
            full = np.full((sc.W * sc.H, got.shape[1]), np.nan, np.float32)
            full[:got.shape[0]] = got
            out["inputs"] = full
        return out
    finally:
        if table is not None:
            table.free()
        mesh.free()


def _check(got, sc, what, count=True, setup=True):
    want = es.expected(sc.name)
    st = got["stats"]
    assert st["tris_setup"] == want.tris_setup, (what, st)
    if count:
        assert st["frag_covered"] == want.frag_covered, (what, st)
    if got["inputs"] is not None:
        inp = got["inputs"]
        assert not np.isnan(inp[want.owned]).any() and np.isnan(inp[~want.owned]).all(), f"{what}: the entries that have an input"
    es.assert_frame(want, sc, got["depth"], got["ids"], got["color"], what, inputs=got["inputs"], setup=got["setup"] if setup else None)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", SCENES)
def test_scene_equals_evaluator(renderers, name, variant):
    """Every scene on every raster path: the default, the sweep kernel, each shape of the tile kernel, atomic binning, early-z
    (fragment counting off), work lists so small that the pass is replayed, and two frames in flight.  The scenes in a window
    with x0 < 0 run k_raster_entries whatever the options say."""
    sc, v = es.all_scenes()[name], VARIANTS[variant]
    many = len(sc.translates) > 1                                  # (several frr_draw: the setup list read back is the last pass's)
    if v.get("replays"):                                           # (a Renderer of its own: the work lists stay grown after a replay)
        r = _make(variant)
        try:
            got = _run(r, sc, "instanced" if many else "draw")
        finally:
            r.close()
        assert got["stats"]["replays"] > 0, got["stats"]
    else:
        got = _run(renderers(variant), sc, "instanced" if many else "draw", frames=v.get("frames", 1))
    _check(got, sc, f"{name}, {variant}", count=v.get("count", True))


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("name", es.names("layers"))
def test_layers_split_over_three_ranks(name, blocked):
    """A world of 3 over the frame's two tile rows (one rank owns nothing): the owned rows stitched together are the
    evaluator's frame, every rank reports the whole setup list's length, and the ranks' fragments add up."""
    import f_renderer_amd as fr
    sc, want = es.all_scenes()[name], es.expected(name)
    depth, ids = np.zeros(sc.W * sc.H, np.float32), np.full(sc.W * sc.H, 0xFFFFFFFF, np.uint32)
    color = np.zeros((sc.H, sc.W, 4), np.uint8)
    covered, seen = 0, np.zeros(sc.H, bool)
    for rank in range(3):
        r = fr.Renderer(sc.W, sc.H)
        try:
            r.set_partition(rank, 3, blocked=blocked)
            vs, ps = _prepare(r, sc)
            r.clear(es.CLEAR_COLOR, 0.0)
            r.draw(r.upload_mesh(es.inputs_f32(sc), vs), ps)
            c, d, t = r.readback()
            st = r.stats()
        finally:
            r.close()
        assert st["tris_setup"] == want.tris_setup, (rank, st)
        covered += st["frag_covered"]
        rows = owned_pixel_rows(sc.H, rank, 3, blocked)
        assert not (rows & seen).any()
        seen |= rows
        own = np.repeat(rows, sc.W)
        depth[own], ids[own], color[rows] = d[own], t[own], c[rows]
        es.assert_frame(want, sc, d, t, c, f"{name}, rank {rank} of 3, blocked={blocked}", rows=rows)
    assert seen.all() and covered == want.frag_covered
    es.assert_frame(want, sc, depth, ids, color, f"{name}, three ranks stitched, blocked={blocked}")


@pytest.mark.parametrize("how", ["draw", "instanced", "list"])
def test_flat_w_under_translation_matrices(renderers, how):
    """flat_w's shapes under three model matrices that translate by whole pixels, as one frr_draw per matrix, as an instanced
    pass and as a draw list, against the evaluator run once per instance; the one-pass forms deliver the whole setup list in
    (instance, triangle) order and every entry's input."""
    sc = es.all_scenes()["instanced_flat_w"]
    got = _run(renderers(), sc, how)
    if how == "draw":                                              # (statistics and setup list are per pass there)
        want = es.expected(sc.name)
        es.assert_frame(want, sc, got["depth"], got["ids"], got["color"], f"{sc.name}, {how}")
        n = want.tris_setup // len(sc.translates)
        last = got["setup"]
        assert last.shape[0] == n
        np.testing.assert_array_equal(last["spi"], want.spi[-n:])
        np.testing.assert_array_equal(last["spf"], want.spf[-n:])
    else:
        _check(got, sc, f"{sc.name}, {how}")
