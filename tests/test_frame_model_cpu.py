"""The generator and the CPU model of tests/frame_model.py, on the seeds tests/test_gpu_frame_model.py runs: the sequences are
deterministic and legal, every step that writes is felt in a compared output, the seed set covers what it is there to cover
(computed from the step records alone), every rung clears the work lists' growth rule by its margin, and the model agrees
with the expectations the per-feature GPU tests already use."""
import collections

import numpy as np
import pytest

from . import frame_model as M
from . import predicate_scenes as P
from . import varyings_scenes as V
from oracle import oracle_np as onp


@pytest.fixture(scope="module")
def generated(oracle):
    return {seed: M.generate(seed, oracle) for seed in M.SEEDS}


@pytest.fixture(scope="module")
def expected(oracle, generated):
    """the model's run of every seed (where it resolves varyings it runs both oracles and asserts that they agree bit for bit)"""
    return {seed: M.run_model(oracle, frames) for seed, frames in generated.items()}


def _strip(frames):
    return [[{k: v for k, v in s.items()} for s in steps] for steps in frames]


def test_generate_is_deterministic(oracle, generated):
    for seed in (0, 7, 22):
        M._GENERATED.pop(seed)
        again = M.generate(seed, oracle)
        assert _strip(again) == _strip(generated[seed]), seed
    assert len({repr(_strip(f)) for f in generated.values()}) == len(generated)


def test_shape_of_the_sequences(generated):
    for seed, frames in generated.items():
        assert len(frames) == M.FRAMES
        windows = [tuple(steps[0]["window"]) for steps in frames]
        assert sorted(windows) == sorted([M.FULL, M.FULL, M.SUB]) and M.SUB[0] > 0, (seed, windows)
        for fi, steps in enumerate(frames):
            assert steps[0]["op"] == "clear" and steps[-1]["op"] in ("readback", "fenced") and len(steps) - 1 <= M.MAX_STEPS, (seed, fi)
            open_pass, passes = None, 0
            for s in steps[1:-1]:
                assert s["op"] not in ("clear", "readback", "fenced")
                if s["op"] == "geom":
                    assert open_pass is None, "every geometry pass is rastered exactly once"
                    open_pass, between = s, 0
                elif s["op"] == "raster":
                    assert open_pass is not None and s["ps"] in M.VS_PS[open_pass["vs"]] and between <= 4
                    open_pass = None
                elif open_pass is not None:
                    between += 1
                    assert s["op"] != "set_cull"    # (and a set_uniforms there changes nothing the vertex shader reads: the model refuses it)
                if s["op"] in ("geom", "draw"):
                    passes += 1
                    assert s["kind"] in M.KINDS and all(m in M.MESHES for m, _ in s["items"])
                    if s["kind"] == "instanced":
                        assert 2 <= len(s["items"]) <= 5 and len({m for m, _ in s["items"]}) == 1 and any(mi == M.M_MIRROR for _, mi in s["items"])
                    if s["kind"] in ("list", "list_if") and not s["rung"] and s["items"]:
                        assert 3 <= len(s["items"]) <= 7
                if s["op"] in ("wireframe", "item_ranges", "setup_triangles") or (s["op"] == "count" and s["unit"] == "triangle"):
                    assert passes > 0, f"seed {seed} frame {fi}: {s['op']} before the frame's first geometry pass"
                if s["op"] in ("resolve", "count"):
                    assert s["buf"][0] == "AB"[fi % 2], "caller buffers come from two pools that alternate by frame"
            assert open_pass is None


def test_model_runs_and_the_two_oracles_agree(expected):
    """run_model over every seed; Model._np_ctx asserts depth, ids and colour of the NumPy oracle equal to the C oracle's
    wherever a resolve uses both"""
    resolves = 0
    for seed, out in expected.items():
        assert len(out) == M.FRAMES
        resolves += sum(1 for s in M.steps_of(M.generate(seed)) if s["op"] == "resolve" and not s.get("noop"))
    assert resolves >= len(expected) // 2 and len(M._NP_CTX) > 0


def test_every_kept_step_is_felt(oracle, generated):
    for seed, frames in generated.items():
        bad = M.insensitive_steps(oracle, frames)
        assert not bad, f"seed {seed}: removing {[(fi, M.describe(s)) for fi, s in bad]} changes no compared output"
        flat = M.steps_of(frames)
        noops = [s for s in flat if s.get("noop")]
        assert len(noops) <= M.NOOP_SHARE * len(flat), (seed, len(noops), len(flat))


def _command_kind(s):
    return {"lines": "lines", "wireframe": "wireframe", "resolve": "resolve", "shade": "shade"}.get(s["op"]) or \
        ("count_" + s["unit"] if s["op"] == "count" else None)


def test_coverage_of_the_seed_set(generated):
    kinds = collections.defaultdict(set)           # (pass kind, fused) -> seeds
    inside, behind = collections.defaultdict(set), collections.defaultdict(set)
    # ... and the same for the passes over r1 and r2 alone (a small first pass is a fan rung too, while the list holds 16
    # slots), and for those of them in frames 1 and 2: the replays that are neither at the first draw nor in the first frame
    inside_r, inside_late, behind_r = collections.defaultdict(set), collections.defaultdict(set), collections.defaultdict(set)
    fed, with_cull, with_window = set(), set(), set()
    for seed, frames in generated.items():
        cull = 0
        for fi, steps in enumerate(frames):
            window = "full" if tuple(steps[0]["window"]) == M.FULL else "sub"
            in_rung = after_rung = in_r = after_r = False
            for s in steps:
                if s["op"] == "set_cull":
                    cull = s["mode"]
                if s["op"] in ("geom", "draw"):
                    kinds[s["kind"], s["op"] == "draw"].add(seed)
                    with_cull.add((s["kind"], cull))
                    with_window.add((s["kind"], window))
                    if s["kind"] == "list_if" and s["fed"]:
                        fed.add(seed)
                    in_rung = s["op"] == "geom" and s["fan_rung"]
                    after_rung |= s["op"] == "draw" and s["fan_rung"]
                    in_r = s["op"] == "geom" and s["rung"] > 0
                    after_r |= s["op"] == "draw" and s["rung"] > 0
                elif s["op"] == "raster":
                    after_rung |= in_rung
                    after_r |= in_r
                    in_rung = in_r = False
                elif _command_kind(s):
                    if in_rung:
                        inside[_command_kind(s)].add(seed)
                    elif after_rung:
                        behind[_command_kind(s)].add(seed)
                    if in_r:
                        inside_r[_command_kind(s)].add(seed)
                        if fi > 0:
                            inside_late[_command_kind(s)].add(seed)
                    elif after_r:
                        behind_r[_command_kind(s)].add(seed)
    for kind in M.KINDS:
        for fused in (True, False):
            assert len(kinds[kind, fused]) >= 3, f"{kind} {'fused' if fused else 'split'}: seeds {sorted(kinds[kind, fused])}"
        for cull in (0, 1, 2):
            assert (kind, cull) in with_cull, f"{kind} under cull mode {cull}"
        for window in ("full", "sub"):
            assert (kind, window) in with_window, f"{kind} in a {window} window"
    for c in M.COMMANDS:
        assert len(inside[c]) >= 3, f"{c} inside a fan rung's split pass: seeds {sorted(inside[c])}"
        assert len(behind[c]) >= 3, f"{c} behind a rung pass in its frame: seeds {sorted(behind[c])}"
        assert len(inside_r[c]) >= 3, f"{c} inside the split pass of r1 or r2: seeds {sorted(inside_r[c])}"
        assert len(inside_late[c]) >= 1, f"{c} inside the split pass of r1 or r2 in frame 1 or 2: seeds {sorted(inside_late[c])}"
        assert len(behind_r[c]) >= 2, f"{c} behind the pass of r1 or r2 in its frame: seeds {sorted(behind_r[c])}"
    assert len(fed) >= 4, f"a predicated pass fed by a count buffer: seeds {sorted(fed)}"


def test_rung_margins(generated):
    """every pass over a rung mesh needs at least MARGIN times the fan slots the growth rule can have left behind by then (the
    test's own walk over the step records), the rungs are met in increasing order, and the model says so frame by frame.
    The bin records: r2 clears their growth rule by the same margin in every seed; r1 is a rung of the fan slots alone -- its
    5,700 to 6,300 records are 3.1 to 5 times what an ordinary pass of up to 640 records can have left (640 + 160 + 1024), so
    the margin holds in some seeds only, and they are counted."""
    r1_bin_rungs = 0
    for seed, frames in generated.items():
        cap, bins, met = M.TINY["fan_capacity"], M.TINY["bin_capacity"], []
        for fi, steps in enumerate(frames):
            for s in steps:
                if s["op"] not in ("geom", "draw"):
                    continue
                if s["rung"]:
                    assert s["fan_need"] >= M.MARGIN * cap, f"seed {seed} frame {fi}: rung {s['rung']} needs {s['fan_need']}, the list may hold {cap}"
                    assert s["fan_rung"]
                    assert s["bin_rung"] == (s["bin_need"] >= M.MARGIN * bins), (seed, fi, s["bin_need"], bins)
                    if s["rung"] == 2:
                        assert s["bin_need"] >= M.MARGIN * bins, f"seed {seed} frame {fi}: rung 2 needs {s['bin_need']} records, the list may hold {bins}"
                    else:
                        r1_bin_rungs += s["bin_rung"]
                    met.append((s["rung"], fi))
                else:
                    assert s["fan_need"] <= M.ORDINARY_FAN_NEED
                if s["fan_need"] > M.TINY["fan_capacity"]:
                    cap = max(cap, M.growth(s["fan_need"], 8))
                if s["bin_need"] > M.TINY["bin_capacity"]:
                    bins = max(bins, M.growth(s["bin_need"], 4))
        assert [r for r, _ in met] == [1, 2] and met[0][1] < met[1][1], (seed, met)
    assert r1_bin_rungs >= len(generated) // 2, r1_bin_rungs


def test_an_empty_list_takes_any_pixel_shader(oracle):
    """frr_drawlist_upload takes the list's vertex shader from its first item; a list without items has none.  frr_draw_list of
    it skips the rasterization, so any pixel shader goes; frr_geometry_list + frr_raster of it used to refuse FRR_PS_COLOR,
    FRR_PS_PHONG and FRR_PS_BLINN against a placeholder K of 0 (seed 5 of the GPU runs met it: a split, predicated, empty list
    rastered with FRR_PS_BLINN).  The pass has K = 0 all the same: a resolve into a K = 8 buffer is not defined."""
    empty = dict(op="geom", kind="list", vs="PHONG", items=[], rung=0)
    for ps in ("BLINN", "PHONG", "COLOR", "DEPTH", "FLAT"):
        m = M.Model(oracle)
        m.apply(dict(op="clear", window=M.FULL))
        m.apply(empty)
        assert m.last.K == 0 and m.stats()["draws"] == 1
        m.apply(dict(op="raster", ps=ps))
        assert not m.changed and m.stats() == dict(tris_in=0, tris_setup=0, draws=1, frag_covered=0, frag_nan=0)
    with pytest.raises(M.Undefined):
        m.apply(dict(op="resolve", buf="A.v8a"))
    split_empty = [s for seed in M.SEEDS for steps in M.generate(seed, oracle) for s in steps if s["op"] == "geom" and not s["items"]]
    assert split_empty, "no seed rasters an empty list behind its geometry pass any more"


def test_cull_mode_travels_with_the_geometry_command(oracle):
    """frame_model.cull_inside_split: each set_cull between a geometry* and its rasterization leaves that pass alone and
    holds for the next one -- moving it in front of the geometry call changes what the frame leaves, and so does removing it;
    the first pass is a rung of the tiny lists, so the GPU run replays it"""
    frames = M.cull_inside_split()
    want, = M.run_model(oracle, frames)
    assert want["crossed"] and want["stats"]["draws"] == 3 and 0 < want["stats"]["tris_setup"]
    steps = frames[0]
    inner = [k for k, s in enumerate(steps) if s["op"] == "set_cull" and steps[k - 1]["op"] == "geom"]
    assert len(inner) == 2
    for k in inner:
        moved = steps[:k - 1] + [steps[k], steps[k - 1]] + steps[k + 1:]
        assert not M.same_outputs(M.run_model(oracle, [moved])[0], want), f"set_cull at step {k} moved before its geometry call"
        assert not M.same_outputs(M.run_model(oracle, [steps[:k] + steps[k + 1:]])[0], want), f"set_cull at step {k} removed"
    assert not M.insensitive_steps(oracle, frames)


def test_growth_rule_is_the_host_layers():
    """the two constants of finish() the rungs are sized against, read from the source"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "f_renderer_amd", "csrc", "frr_api.hip")).read()
    assert re.search(r"worst \+ worst / 4 \+ 1024", src) and re.search(r"nf \+ nf / 8 \+ 1024", src)
    assert M.growth(4000, 4) == 4000 + 1000 + 1024 and M.growth(4000, 8) == 4000 + 500 + 1024


def test_fast_line_painting_is_the_reference_walk():
    from . import lines_reference as R
    for xyxy, rgba in M.LINES:
        img = np.full((M.H, M.W, 4), 7, np.uint8)
        idx, col = M.painted(xyxy, rgba)
        fast = img.copy()
        fast.reshape(-1, 4)[idx] = col
        np.testing.assert_array_equal(fast, R.draw_lines(img.copy(), xyxy, rgba))


# ---- the model pinned to the expectations the per-feature tests use -----------------------------------------------------------

def test_pinned_to_the_lines_sequence(oracle):
    """tests/test_gpu_lines.py: draw, lines, draw on its 96 x 70 frame"""
    from . import test_gpu_lines as L
    near, far = L._two_meshes()
    xyxy, col = L._segments(90, 21, reach=60), L._colors(90)
    want = L._oracle_sequence(oracle, [("draw", near), ("lines", xyxy, col), ("draw", far)])
    M.MESHES.update(pin_near=near, pin_far=far)
    M.LINES.append((xyxy, col))
    try:
        steps = [dict(op="clear", window=(0, L.W, 0, L.H)),
                 dict(op="draw", kind="plain", vs="CLIP_COLOR", items=[("pin_near", M.M_IDENT)], ps="COLOR", rung=0),
                 dict(op="lines", list=len(M.LINES) - 1),
                 dict(op="geom", kind="plain", vs="CLIP_COLOR", items=[("pin_far", M.M_IDENT)], rung=0), dict(op="raster", ps="COLOR"),
                 dict(op="readback")]
        got, = M.run_model(oracle, [steps], size=(L.W, L.H), clear=(L.BG, 0.0))
    finally:
        M.LINES.pop()
        for k in ("pin_near", "pin_far"):
            M.MESHES.pop(k)
    np.testing.assert_array_equal(got["color"], want.color)
    np.testing.assert_array_equal(got["tri_id"], want.tri_id)
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want.depth.view(np.uint32))
    assert got["stats"]["tris_setup"] == int(want.counters.tris_setup) and got["stats"]["frag_covered"] == int(want.counters.frag_covered)


def test_pinned_to_the_predicate_expectation(oracle):
    """tests/predicate_scenes.py: the list `clipped` under a mask, through a mask buffer the model reads at the geometry call"""
    sc = P.scene("clipped")
    kept = P.clipped_masks()["drop_near"]
    frame, setup, per = P.expected(oracle, "clipped", kept)
    cm = M.MODELS[:6]
    models = [int(np.flatnonzero((cm == m).all(axis=1))[0]) for m in sc.models]
    names = [f"pin_{w}" for w in sc.which]
    M.MESHES.update({f"pin_{k}": m.tris for k, m in enumerate(sc.meshes)})
    M.MASKS["pin_mask"] = kept.astype(np.uint32)
    try:
        steps = [dict(op="clear", window=M.FULL),
                 dict(op="draw", kind="list_if", vs="PHONG", items=list(zip(names, models)), keep="pin_mask", keep_entries=sc.nitems, min=1, ps="PHONG", rung=0),
                 dict(op="item_ranges"), dict(op="setup_triangles"), dict(op="readback")]
        got, = M.run_model(oracle, [steps])
    finally:
        M.MASKS.pop("pin_mask")
        for k in range(len(sc.meshes)):
            M.MESHES.pop(f"pin_{k}")
    np.testing.assert_array_equal(got["color"], frame.color)
    np.testing.assert_array_equal(got["tri_id"], frame.tri_id)
    np.testing.assert_array_equal(got["depth"].view(np.uint32), frame.depth.view(np.uint32))
    (_, ranges), (_, tris) = got["answers"]
    assert list(ranges["count"]) == per and per[P.CLIPPED_NEAR] == 0
    np.testing.assert_array_equal(tris["spi"], setup["spi"])
    assert got["stats"]["tris_in"] == sum(sc.ntris) and got["stats"]["tris_setup"] == sum(per)


def test_pinned_to_the_two_pass_resolve(oracle):
    """tests/varyings_scenes.py: two_draws() on its 96 x 70 frame, a resolve behind each draw into one buffer"""
    e = V.two_draws()
    a, b = V.basic()[0], V.second()
    M.MESHES.update(pin_a=a, pin_b=b)
    try:
        steps = [dict(op="clear", window=(0, V.W, 0, V.H)),
                 dict(op="draw", kind="plain", vs="CLIP_COLOR", items=[("pin_a", M.M_IDENT)], ps="COLOR", rung=0), dict(op="resolve", buf="A.v3a"),
                 dict(op="geom", kind="plain", vs="CLIP_COLOR", items=[("pin_b", M.M_IDENT)], rung=0), dict(op="resolve", buf="A.v3b"),
                 dict(op="raster", ps="COLOR"), dict(op="resolve", buf="A.v3a"), dict(op="readback")]
        got, = M.run_model(oracle, [steps], size=(V.W, V.H), clear=(V.BG, 0.0))
    finally:
        for k in ("pin_a", "pin_b"):
            M.MESHES.pop(k)
    np.testing.assert_array_equal(got["color"], e.color)
    np.testing.assert_array_equal(got["tri_id"], e.tri_id)
    np.testing.assert_array_equal(got["depth"].view(np.uint32), e.depth.view(np.uint32))
    V.assert_bits_equal(got["bufs"]["A.v3a"][:e.entries].view(np.float32), e.buffer())
    assert (got["bufs"]["A.v3b"] == M.SENTINEL_BITS).all(), "a resolve between geometry and rasterization owns no pixel yet"
    assert onp.VS_K[onp.VS_CLIP_COLOR] == 3
