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


# ---- the extended sequences: shade_items, passes rastered again, abandoned passes; legal on a partitioned context ---------------

# sha256 over repr(frame_model.steps_of(frame_model.generate(seed))) of the seeds 0 .. 23 in order, computed at the commit before
# the generator learnt the extended steps: what it yields for SEEDS without `extended` is what it yielded then
DIGEST_OF_SEEDS = "2e727c2bf165b3032769c590bd70ddf1b5778159580c95327e6cea3ed450d0e2"


def test_the_sequences_of_the_first_seed_set_are_unchanged(generated):
    import hashlib
    h = hashlib.sha256()
    for seed in M.SEEDS:
        h.update(repr(M.steps_of(generated[seed])).encode())
    assert h.hexdigest() == DIGEST_OF_SEEDS


@pytest.fixture(scope="module")
def extended(oracle):
    return {seed: M.generate(seed, oracle, extended=True) for seed in M.XSEEDS}


def test_extended_sequences_are_deterministic_and_legal(oracle, extended):
    assert len(M.XSEEDS) == 12
    seed = M.XSEEDS[3]
    M._GENERATED.pop((seed, "extended"))
    assert _strip(M.generate(seed, oracle, extended=True)) == _strip(extended[seed])
    for seed, frames in extended.items():
        assert len(frames) == M.FRAMES
        out = M.run_model(oracle, frames, partitioned=True)          # (raises where a step is refused on a partitioned context)
        plain = M.run_model(oracle, frames)
        assert all(M.same_outputs(a, b) for a, b in zip(out, plain)), "the partitioned mode only refuses: it computes nothing else"
        for fi, steps in enumerate(frames):
            assert steps[0]["op"] == "clear" and steps[-1]["op"] in ("readback", "fenced") and len(steps) - 1 <= M.MAX_STEPS, (seed, fi)
            assert tuple(steps[0]["window"]) in (M.FULL, M.SUB)
            latest = None                      # the latest pass: (its step, rastered how often)
            for s in steps[1:-1]:
                if s["op"] in ("geom", "draw"):
                    latest = [s, int(s["op"] == "draw")]
                elif s["op"] == "raster":
                    assert latest is not None and latest[0]["op"] == "geom" and not latest[0].get("abandoned")
                    assert bool(s.get("again")) == (latest[1] > 0), "`again` marks the rasters behind a pass's first"
                    latest[1] += 1
                elif s["op"] in ("wireframe", "resolve", "count", "item_ranges", "setup_triangles", "shade_items") and latest is not None:
                    assert latest[0]["op"] == "geom", f"seed {seed} frame {fi}: {s['op']} behind a fused pass"
                if s["op"] == "shade_items":
                    assert s["table"] in M.MATERIALS and s["ps"] in M.K_PS[M.buffer_k(s["buf"])]


def _extended_coverage(extended):
    n = collections.Counter()
    for seed, frames in extended.items():
        tiny = seed % 2 == 1                   # tests/test_gpu_frame_model.py: the odd seeds run with the tiny work lists
        for steps in frames:
            latest, rastered = None, 0
            for s in steps:
                if s["op"] in ("geom", "draw"):
                    latest, rastered = s, int(s["op"] == "draw")
                    n["abandoned"] += bool(s.get("abandoned"))
                    n["abandoned rung, tiny lists"] += bool(s.get("abandoned") and s["rung"] and s["fan_rung"] and tiny)
                elif s["op"] == "raster":
                    rastered += 1
                    n["second raster"] += bool(s.get("again"))
                    n["depth pre-pass pair"] += bool(s.get("again") and s["ps"] != "DEPTH" and first_ps == "DEPTH")
                    if rastered == 1:
                        first_ps = s["ps"]
                elif s["op"] == "shade_items":
                    n["shade_items"] += 1
                    if latest is not None and rastered and not s.get("noop"):
                        kind = {"list_if": "list", "indexed": "plain"}.get(latest["kind"], latest["kind"])
                        n["shade_items behind " + ("an " if kind == "instanced" else "a ") + kind + " pass"] += 1
                        n["shade_items under a lit shader"] += s["ps"] in ("PHONG", "BLINN")
                    if latest is not None and latest["op"] == "geom" and not rastered:
                        n["shade_items inside a split pass"] += 1
                        n["shade_items inside a split pass, tiny lists"] += tiny
                        n["shade_items inside a fan rung's split pass, tiny lists"] += bool(tiny and latest["fan_rung"])
    return n


def test_coverage_of_the_extended_seed_set(extended):
    n = _extended_coverage(extended)
    print(dict(n))
    for kind in ("shade_items", "second raster", "abandoned", "depth pre-pass pair"):
        assert n[kind] >= 6, (kind, dict(n))
    for place in ("behind a list pass", "behind an instanced pass", "behind a plain pass", "inside a split pass, tiny lists"):
        assert n["shade_items " + place] >= 3, (place, dict(n))
    assert n["shade_items under a lit shader"] >= 3, dict(n)
    assert n["shade_items inside a fan rung's split pass, tiny lists"] >= 1, dict(n)
    assert n["abandoned rung, tiny lists"] >= 1, dict(n)


def test_every_kept_step_of_the_extended_sequences_is_felt(oracle, extended):
    for seed, frames in extended.items():
        bad = M.insensitive_steps(oracle, frames, partitioned=True)
        assert not bad, f"seed {seed}: removing {[(fi, M.describe(s)) for fi, s in bad]} changes no compared output"
        flat = M.steps_of(frames)
        assert len([s for s in flat if s.get("noop")]) <= M.NOOP_SHARE * len(flat), seed


def _one_frame(oracle, steps, **kw):
    m = M.Model(oracle, **kw)
    return m, M.run_frames(m, [steps])[0]


def test_shade_items_is_the_materials_rule_and_the_forward_loop(oracle):
    """The model's shade_items held to the two things the per-feature tests hold frr_shade_items to: the tables pass the rule
    the host and the device share (tests/materials_rule.py), and a depth-only list pass, a resolve and one shade_items leave
    the frame of items_scenes' construction B -- the reference's loop with one ps_uniform per object on the C oracle."""
    from . import drawlist_scenes as D
    from . import items_scenes as IT
    from . import materials_rule as MR
    for name, t in M.MATERIALS.items():
        assert len(t) == 8 and set(t["texture_slot"]) == {0, 1} and not t["user"].any() and not t["reserved"].any()
        assert [g[0] for g in MR.ask([MR.ok(int(e["texture_slot"]), int(e["reserved"])) for e in t])] == [1] * 8
        for k in range(7):
            assert t["texture_slot"][k] != t["texture_slot"][k + 1] or k == 3
            assert t["ambient_strength"][k] != t["ambient_strength"][k + 1] and t["specular_strength"][k] != t["specular_strength"][k + 1]
            assert (t["flat_color"][k] != t["flat_color"][k + 1]).any()
        for items in (0, 1, 7, 8):
            code, text = MR.ask([MR.table(MR.SHADE, 4096, len(t), items, True, 0b0011, 0b0011)])[0]
            assert code == MR.OK and text.split("|")[0] == ""
    assert len({t.tobytes() for t in M.MATERIALS.values()}) == 3 and M.DEVICE_BOUND_TABLE in M.MATERIALS
    sc = D.scene("clipped")
    fb, per = IT.expected_B("clipped", "PHONG")
    models = [int(np.flatnonzero((M.MODELS[:6] == m).all(axis=1))[0]) for m in sc.models]
    names = [f"pin_{w}" for w in sc.which]
    M.MESHES.update({f"pin_{k}": m.tris for k, m in enumerate(sc.meshes)})
    M.MATERIALS["pin"] = IT.materials(sc.nitems)
    ntex = len(M.TEXTURES)
    M.TEXTURES.extend(D.place_textures())
    try:
        steps = [dict(op="clear", window=M.FULL),
                 dict(op="geom", kind="list", vs="PHONG", items=list(zip(names, models)), rung=0), dict(op="shade_items", ps="PHONG", buf="A.v8a", table="pin"),
                 dict(op="raster", ps="DEPTH"), dict(op="resolve", buf="A.v8a"), dict(op="shade_items", ps="PHONG", buf="A.v8a", table="pin"),
                 dict(op="readback")]
        m = M.Model(oracle)
        m.tex = [ntex, ntex + 1, ntex + 2]
        for s in steps[:3]:
            m.apply(s)
        assert not m.changed, "a pass that is not rastered yet has no id in the target: nothing is shaded"
        got = M.run_frames(m, [steps[3:]])[0]
    finally:
        del M.TEXTURES[ntex:]
        M.MATERIALS.pop("pin")
        for k in range(len(sc.meshes)):
            M.MESHES.pop(f"pin_{k}")
    assert len(set(M.MATERIALS)) == 3
    np.testing.assert_array_equal(got["tri_id"], fb.tri_id)
    np.testing.assert_array_equal(got["depth"].view(np.uint32), fb.depth.view(np.uint32))
    np.testing.assert_array_equal(got["color"], fb.color)
    assert got["stats"]["tris_setup"] == sum(per) and (fb.tri_id != M.NONE).sum() > 500


def test_shade_items_where_it_is_undefined_and_where_it_writes_nothing(oracle):
    inst = [("torus", int(M.M_CLIPPED[0])), ("torus", M.M_MIRROR), ("torus", int(M.M_GRID[0]))]
    geom = dict(op="geom", kind="instanced", vs="PHONG", items=inst, rung=0)
    items = dict(op="shade_items", ps="PHONG", buf="A.v8a", table="mat0")
    clear = dict(op="clear", window=M.FULL)
    m = M.Model(oracle)
    m.apply(clear)
    with pytest.raises(M.Undefined):           # before any geometry pass
        m.apply(items)
    for s in (geom, dict(op="raster", ps="DEPTH"), dict(op="resolve", buf="A.v8a")):
        m.apply(s)
    for bad in (dict(items, ps="COLOR"), dict(items, buf="A.v3a", ps="PHONG")):       # a buffer whose K the shader refuses
        with pytest.raises(M.Undefined):
            m.copy().apply(bad)
    a = m.copy()
    a.apply(items)
    assert a.changed and (a.frame.tri_id == m.frame.tri_id).all() and a.stats() == m.stats()
    # every item under ITS material: item k's pixels under FLAT hold the quantised flat colour of entry k
    b = m.copy()
    b.apply(dict(items, ps="FLAT", table="mat1"))
    first = M.VIS.bounds_of(m.last.per_item, m.last.base).astype(np.int64)
    seen = 0
    for k in range(3):
        px = (m.frame.tri_id >= first[k]) & (m.frame.tri_id < first[k + 1])
        seen += bool(px.any())
        assert (b.frame.color.reshape(-1, 4)[px] == onp.quantize(M.MATERIALS["mat1"]["flat_color"][k:k + 1])).all(), k
    assert seen >= 2
    # ... after a clear since the pass, and for a pass that emitted nothing: FRR_OK, nothing written
    c = m.copy()
    c.apply(clear)
    c.apply(items)
    assert not c.changed
    c.apply(dict(op="geom", kind="list", vs="PHONG", items=[("empty", int(M.M_GRID[0]))], rung=0))
    c.apply(dict(op="raster", ps="PHONG"))
    c.apply(items)
    assert not c.changed
    # on a partitioned context: refused behind a fused pass, like everything that reads the pass's tables
    p = M.Model(oracle, partitioned=True)
    p.apply(clear)
    p.apply(dict(geom, op="draw", ps="DEPTH"))
    for s in (items, dict(op="wireframe", color=0), dict(op="resolve", buf="A.v8a"), dict(op="item_ranges"), dict(op="setup_triangles"),
              dict(op="count", unit="item", buf="A.c0", entries=3), dict(op="count", unit="triangle", buf="A.c0", entries=30), dict(op="raster", ps="PHONG")):
        with pytest.raises(M.Undefined):
            p.copy().apply(s)
    p.apply(dict(op="shade", buf="A.v8a", ps="FLAT", ids=(0, M.NONE)))                 # a ranged shade reads no pass


def test_a_pass_rastered_again_and_an_abandoned_pass(oracle):
    """the depth pre-pass pair leaves the frame of the one shading raster and counts its fragments twice; draws, tris_in and
    tris_setup count at the geometry call; an abandoned pass owns no pixel and the next pass's ids start behind it"""
    lst = [("p100", int(M.M_CLIPPED[0])), ("torus", int(M.M_GRID[1])), ("spiky", int(M.M_CLIPPED[3]))]
    clear, geom = dict(op="clear", window=M.SUB), dict(op="geom", kind="list", vs="PHONG", items=lst, rung=0)
    _, once = _one_frame(oracle, [clear, geom, dict(op="raster", ps="PHONG"), dict(op="readback")])
    _, pair = _one_frame(oracle, [clear, geom, dict(op="raster", ps="DEPTH"), dict(op="raster", ps="PHONG", again=True), dict(op="readback")])
    for k in ("color", "depth", "tri_id"):
        assert once[k].tobytes() == pair[k].tobytes(), k
    assert once["stats"]["frag_covered"] > 0 and pair["stats"]["frag_covered"] == 2 * once["stats"]["frag_covered"]
    assert {k: pair["stats"][k] for k in ("draws", "tris_in", "tris_setup")} == {k: once["stats"][k] for k in ("draws", "tris_in", "tris_setup")}
    plain = dict(op="geom", kind="plain", vs="GOURAUD", items=[("p40", M.M_IDENT)], rung=0)
    m, left = _one_frame(oracle, [clear, geom, plain, dict(op="raster", ps="COLOR"), dict(op="item_ranges"), dict(op="readback")])
    n = once["stats"]["tris_setup"]
    assert left["answers"][0][1]["first"][0] == n > 0 and left["stats"]["draws"] == 2 and left["stats"]["tris_setup"] > n
    ids = left["tri_id"][left["tri_id"] != M.NONE]
    assert ids.size and ids.min() >= n, "the abandoned pass owns no pixel"
    assert left["stats"]["tris_in"] == once["stats"]["tris_in"] + M.MESHES["p40"].shape[0]
    # ... and the fixed sequence of the GPU runs: one block abandoned, then a pass of several
    frames = M.abandoned_then_larger()
    want, = M.run_model(oracle, frames)
    assert M.MESHES["grid"].shape[0] <= M.GEOM_BLOCK < sum(M.MESHES[m].shape[0] for m, _ in frames[0][3]["items"]) - M.GEOM_BLOCK
    first = want["answers"][0][1]["first"][0]
    assert first >= 128 and want["tri_id"][want["tri_id"] != M.NONE].min() >= first and not M.insensitive_steps(oracle, frames)


def test_the_fixed_sequences_of_the_partitioned_runs(oracle):
    frames = M.refused_behind_fused()
    want, = M.run_model(oracle, frames, partitioned=True)
    refused = [s for s in frames[0] if s.get("refused")]
    assert {s["op"] for s in refused} == {"wireframe", "setup_triangles", "item_ranges", "resolve", "count", "shade_items", "query", "query_host"}
    assert {s["unit"] for s in refused if s["op"] == "count"} == {"item", "triangle"}
    with pytest.raises(AssertionError, match="marked as refused"):
        M.run_model(oracle, frames)            # (without a partition nothing filters the setup list: every one is taken)
    assert (want["bufs"]["A.v8b"] != M.SENTINEL_BITS).any() and [op for op, _ in want["answers"]] == ["item_ranges", "stats"]
    kept = [[s for s in frames[0] if not s.get("refused")]]
    assert not M.insensitive_steps(oracle, kept, partitioned=True)


def test_lines_and_draws_own_different_rows_in_a_short_window_of_the_blocked_layout(oracle):
    """frr_draw_lines takes its owner from the context's tile rows, draws, resolves, shades and counts from the window's.
    Interleaved (ty % world) the two agree on every row whatever the counts are; blocked they agree only where the window has
    as many tile rows as the context.  On the 96-row frame a window of 40 rows has two: with two ranks the draws give plane
    rows 32 .. 39 to rank 1 and the lines give them to rank 0, so a line over a triangle there is complete on no rank."""
    from f_renderer_amd.multigpu import tile_row_owner
    for world in (2, 3, 4, 8):
        for ctx_rows in range(1, 12):
            for win_rows in range(1, ctx_rows + 1):
                assert tile_row_owner(win_rows, world, False) == tile_row_owner(ctx_rows, world, False)[:win_rows]
    assert tile_row_owner(2, 2, True) == [0, 1] and tile_row_owner(3, 2, True) == [0, 0, 1]
    x0, x1, y0, y1 = M.LINE_WINDOW
    assert (y1 - y0 + 31) // 32 == 2 and (M.H + 31) // 32 == 3
    draws0, lines0 = (M.command_rows(op, M.LINE_WINDOW, M.H, 0, 2, True) for op in ("shade", "lines"))
    draws1, lines1 = (M.command_rows(op, M.LINE_WINDOW, M.H, 1, 2, True) for op in ("shade", "lines"))
    assert draws1[32:40].all() and lines0[32:40].all() and not draws0[32:40].any() and not lines1[32:40].any()
    steps = M.line_ownership()[0]
    want, = M.run_model(oracle, [steps])
    assert not M.insensitive_steps(oracle, [steps])
    # the frame has what the question is about: line pixels over the pass's pixels in plane rows 32 .. 39, some shaded after
    idx, _ = M.painted(*M.LINES[0])
    on_pass = idx[(want["tri_id"][idx] != M.NONE) & (idx // M.W >= 32) & (idx // M.W < 40)]
    assert on_pass.size >= 4 and (want["tri_id"][on_pass] < 20).any() and (want["tri_id"][on_pass] >= 20).any()
    for world in (2, 3):
        for blocked in (False, True):
            ranks = [M.run_rank(oracle, steps, rank, world, blocked)["color"] for rank in range(world)]
            by_lines = np.stack([M.command_rows("lines", M.LINE_WINDOW, M.H, rank, world, blocked) for rank in range(world)])
            by_draws = np.stack([M.command_rows("shade", M.LINE_WINDOW, M.H, rank, world, blocked) for rank in range(world)])
            stitched = np.zeros_like(want["color"])
            for rank in range(world):
                stitched[by_lines[rank]] = ranks[rank][by_lines[rank]]
            if not blocked:
                assert (by_lines[:, :y1 - y0] == by_draws[:, :y1 - y0]).all()
                np.testing.assert_array_equal(stitched, want["color"])
            elif world == 2:
                for rule in (by_lines, by_draws):
                    stitched = np.zeros_like(want["color"])
                    for rank in range(world):
                        stitched[rule[rank]] = ranks[rank][rule[rank]]
                    assert (stitched[32:40] != want["color"][32:40]).any(), "rows 32 .. 39 are complete on no rank"
                    assert (stitched[:32] == want["color"][:32]).all()


# ---- the query sequences: occlusion queries, box queries, their host forms, and the passes they decide ------------------------

# sha256 over repr(frame_model.steps_of(frame_model.generate(seed, extended=True))) of the seeds 100 .. 111 in order, computed
# at the commit before the generator learnt the query steps
DIGEST_OF_XSEEDS = "41783c2fe72959ea4139486565e198a2b2acb51e18ad56376e6602d18f6aa8f2"


def test_the_sequences_of_the_extended_seed_set_are_unchanged(extended):
    import hashlib
    h = hashlib.sha256()
    for seed in M.XSEEDS:
        h.update(repr(M.steps_of(extended[seed])).encode())
    assert h.hexdigest() == DIGEST_OF_XSEEDS
    assert not any(s["op"] in ("query", "boxes", "query_host", "boxes_host", "bounds") or "cover" in repr(s.get("items")) for f in extended.values()
                   for s in M.steps_of(f))


@pytest.fixture(scope="module")
def queried(oracle):
    return {seed: M.generate(seed, oracle, queries=True) for seed in M.QSEEDS}


def _key(s):
    return s["vs"], tuple(tuple(i) for i in s["items"])


def _walk(oracle, frames):
    """the model over a sequence, step by step: yields (frame number, index in the frame, step, the model BEFORE the step, the
    step's answer), applying the step when the consumer comes back"""
    m = M.Model(oracle, partitioned=True)
    for fi, steps in enumerate(frames):
        for k, s in enumerate(steps):
            before = m.copy()
            a = m.apply(s)
            yield fi, k, s, before, m, a


def test_query_sequences_are_deterministic_and_legal(oracle, queried):
    assert len(M.QSEEDS) == 16
    seed = M.QSEEDS[5]
    M._GENERATED.pop((seed, "queries"))
    assert _strip(M.generate(seed, oracle, queries=True)) == _strip(queried[seed])
    assert len({repr(_strip(f)) for f in queried.values()}) == len(queried)
    for seed, frames in queried.items():
        assert len(frames) == M.FRAMES
        out = M.run_model(oracle, frames, partitioned=True)          # (raises where a step is refused on a partitioned context)
        plain = M.run_model(oracle, frames)
        assert all(M.same_outputs(a, b) for a, b in zip(out, plain)), "the partitioned mode only refuses: it computes nothing else"
        windows = [tuple(steps[0]["window"]) for steps in frames]
        assert sorted(windows) == sorted([M.FULL, M.FULL, M.SUB]), (seed, windows)
        for fi, steps in enumerate(frames):
            assert steps[0]["op"] == "clear" and steps[-1]["op"] in ("readback", "fenced") and len(steps) - 1 <= M.MAX_STEPS, (seed, fi)
            latest = None                      # the latest pass: (its step, rastered how often)
            for s in steps[1:-1]:
                if s["op"] in ("geom", "draw"):
                    latest = [s, int(s["op"] == "draw")]
                    if s["kind"] in ("list", "list_if") and not s["rung"] and s["items"]:
                        assert 3 <= len(s["items"]) <= 7
                elif s["op"] == "raster":
                    assert latest is not None and latest[0]["op"] == "geom" and not latest[0].get("abandoned")
                    assert bool(s.get("again")) == (latest[1] > 0), "`again` marks the rasters behind a pass's first"
                    latest[1] += 1
                elif s["op"] in ("wireframe", "resolve", "count", "item_ranges", "setup_triangles", "shade_items", "query", "query_host") and latest is not None:
                    assert latest[0]["op"] == "geom", f"seed {seed} frame {fi}: {s['op']} behind a fused pass"
                if s["op"] in ("count", "query", "boxes", "resolve"):
                    assert s["buf"][0] == "AB"[fi % 2], "caller buffers come from two pools that alternate by frame"
                if s["op"] in ("boxes", "boxes_host", "bounds"):
                    assert s["vs"] in M.VS_PS and 3 <= len(s["items"]) <= 7 and all(m in M.MESHES and m not in M.RUNGS.values() for m, _ in s["items"])
        # every fed pass names a buffer whose provenance matches its list; a buffer of box answers is read under min_value 1 only
        for fi, k, s, m, _, _ in _walk(oracle, frames):
            if s["op"] in ("geom", "draw") and s["kind"] == "list_if" and s["keep"] in m.bufs:
                pr = m.prov.get(s["keep"])
                if s["fed"]:
                    assert pr is not None and pr["unit"] == "item" and [tuple(i) for i in pr["items"]] == [tuple(i) for i in s["items"]], (seed, fi, k)
                    assert pr["entries"] == s["keep_entries"] >= len(s["items"]) and pr["frame"] >= m.fno - 1 and pr["source"] == s["source"]
                    assert pr["source"] != "boxes" or pr["vs"] == s["vs"], "a box answer feeds the list that was queried"
                assert pr is None or pr["source"] != "boxes" or s["min"] == 1, (seed, fi, k)


def test_every_kept_step_of_the_query_sequences_is_felt(oracle, queried):
    for seed, frames in queried.items():
        bad = M.insensitive_steps(oracle, frames, partitioned=True)
        assert not bad, f"seed {seed}: removing {[(fi, M.describe(s)) for fi, s in bad]} changes no compared output"
        flat = M.steps_of(frames)
        assert len([s for s in flat if s.get("noop")]) <= M.NOOP_SHARE * len(flat), seed


def _query_coverage(oracle, queried):
    from . import box_reference as BX
    n, status = collections.Counter(), collections.Counter()
    for seed, frames in queried.items():
        tiny = seed % 2 == 1                   # the seeds that run with the tiny lists on a partition too
        cam_of = {}                            # list -> the camera of its last use
        for fi, k, s, m, after, a in _walk(oracle, frames):
            op = s["op"]
            if op == "clear":
                latest, rastered, abandoned, draws, asked = None, 0, False, 0, {}
                sub = tuple(s["window"]) == M.SUB
                steps = frames[fi]
            elif op in ("geom", "draw"):
                latest, rastered = s, int(op == "draw")
                abandoned |= bool(s.get("abandoned"))
                draws += op == "draw"
                if s["kind"] in ("list", "list_if"):
                    cam_of[_key(s)] = m.cam
                if s["kind"] == "list_if" and s.get("fed") and s.get("source") in ("query", "boxes"):
                    src, pr = s["source"], m.prov[s["keep"]]
                    kept = P.kept_of(m.bufs[s["keep"]][:len(s["items"])], s["min"])
                    n["fed by " + src] += 1
                    n["fed by " + src + ", some dropped and some kept"] += bool(kept.any() and not kept.all())
                    n["fed by " + src + " within one frame"] += pr["frame"] == m.fno
                    n["fed by " + src + " across a frame boundary"] += pr["frame"] == m.fno - 1
            elif op == "raster":
                rastered += 1
                draws += 1
            elif op in ("query", "query_host"):
                n["host form"] += op == "query_host"
                if op == "query_host":
                    continue
                p = m.last
                inside = latest is not None and latest["op"] == "geom" and not rastered and not p.cleared
                units = len(p.items) if s["unit"] == "item" else p.base + p.emit
                n["query"] += 1
                n["query per triangle"] += s["unit"] == "triangle"
                n["query with entries below n"] += s["entries"] < units
                n["query with entries above n"] += s["entries"] > units
                n["query inside a split pass, tiny lists"] += inside and tiny
                n["query inside a bin rung's split pass, tiny lists"] += bool(inside and tiny and latest["bin_rung"])
                n["query in a sub-window frame"] += sub
                n["query behind an abandoned pass"] += abandoned
                n["query after a clear since the pass"] += bool(p.cleared)
                n["query of a list_if pass with a dropped item"] += bool(not p.cleared and p.kind == "list_if" and not p.kept.all())
                n["query under a cull mode"] += bool(not p.cleared and p.cull != 0)
            elif op in ("boxes", "boxes_host", "bounds"):
                n["host form"] += op != "boxes"
                if op == "bounds":
                    continue
                if op == "boxes":
                    log = after.box_log[-1]
                    nitems = len(s["items"])
                    n["boxes"] += 1
                    n["boxes first behind the clear"] += k == 1
                    n["boxes behind a changed camera"] += _key(s) in cam_of and cam_of[_key(s)] != m.cam and \
                        any(x["op"] == "set_uniforms" for f in frames[:fi + 1] for x in f)
                    status.update(int(v) for v in log["srl"][:, 0])
                    if _key(s) in asked and draws > asked[_key(s)][1] and (asked[_key(s)][0] != log["srl"][:, 0]).any():
                        n["two boxes of one list around a draw that differ"] += 1
                    asked[_key(s)] = (log["srl"][:, 0].copy(), draws)
                cam_of[_key(s)] = m.cam
    names = {BX.NONE: "NONE", BX.OUTSIDE: "OUTSIDE", BX.HIDDEN: "HIDDEN", BX.KEPT: "KEPT", BX.UNBOUNDED: "UNBOUNDED"}
    return n, {names[k]: v for k, v in status.items()}


def test_coverage_of_the_query_seed_set(oracle, queried):
    n, status = _query_coverage(oracle, queried)
    print(dict(n), status)
    for what in ("query", "boxes", "host form"):
        assert n[what] >= 6, (what, dict(n))
    for what in ("query per triangle", "query with entries below n", "query with entries above n", "query inside a split pass, tiny lists",
                 "query in a sub-window frame", "boxes first behind the clear", "boxes behind a changed camera",
                 "two boxes of one list around a draw that differ", "fed by query", "fed by boxes"):
        assert n[what] >= 3, (what, dict(n))
    for what in ("query inside a bin rung's split pass, tiny lists", "query behind an abandoned pass", "query after a clear since the pass",
                 "query of a list_if pass with a dropped item", "query under a cull mode"):
        assert n[what] >= 1, (what, dict(n))
    for what in ("HIDDEN", "KEPT", "UNBOUNDED"):
        assert status.get(what, 0) >= 3, (what, status)
    for what in ("OUTSIDE", "NONE"):
        assert status.get(what, 0) >= 1, (what, status)
    for src in ("query", "boxes"):
        assert n["fed by " + src + ", some dropped and some kept"] >= 2, (src, dict(n))
        assert n["fed by " + src + " within one frame"] >= 2, (src, dict(n))
    assert n["fed by query across a frame boundary"] + n["fed by boxes across a frame boundary"] >= 1, dict(n)


def _pin_scene(prefix, sc):
    """a drawlist_scenes list as items of the model: its meshes under names of their own, its matrices behind MODELS"""
    base = len(M.MODELS)
    M.MESHES.update({f"{prefix}_{k}": m.tris for k, m in enumerate(sc.meshes)})
    M.MODELS = np.concatenate([M.MODELS, np.asarray(sc.models, np.float32).reshape(-1, 16)])
    return [(f"{prefix}_{w}", base + i) for i, w in enumerate(sc.which)]


def test_pinned_to_the_query_pairs(oracle):
    """tests/query_reference.py: the per-item answers of the pair (`clipped` as the occluders, `sizes` as the probe) and of
    `sizes` against the cleared depth, as the device form writes them and as the host form returns them"""
    from . import drawlist_scenes as D
    from . import query_reference as QR
    models, names = M.MODELS, set(M.MESHES)
    try:
        occ, probe = _pin_scene("qpin_occ", D.scene("clipped")), _pin_scene("qpin_probe", D.scene("sizes"))
        n = len(probe)
        steps = [dict(op="clear", window=M.FULL),
                 dict(op="geom", kind="list", vs="PHONG", items=probe, rung=0), dict(op="query", unit="item", buf="A.c0", entries=n),
                 dict(op="draw", kind="list", vs="PHONG", items=occ, ps="DEPTH", rung=0),
                 dict(op="geom", kind="list", vs="PHONG", items=probe, rung=0), dict(op="query", unit="item", buf="A.c1", entries=n + 2),
                 dict(op="query_host", unit="item", entries=n - 1), dict(op="query_host", unit="triangle", entries=M.COUNT_CAP), dict(op="stats"),
                 dict(op="readback")]
        got, = M.run_model(oracle, [steps])
    finally:
        M.MODELS = models
        for k in set(M.MESHES) - names:
            M.MESHES.pop(k)
    pair = QR.PAIRS["clipped", "sizes"]
    assert list(got["bufs"]["A.c0"][:n]) == QR.CLEARED["sizes"] and list(got["bufs"]["A.c1"][:n]) == pair
    assert list(got["bufs"]["A.c1"][n:n + 2]) == [0, 0] and got["bufs"]["A.c1"][n + 2] == M.SENTINEL_BITS and got["bufs"]["A.c0"][n] == M.SENTINEL_BITS
    (_, a), (_, t), (_, st) = got["answers"]
    assert list(a["out"]) == pair[:n - 1]
    d0, setup, per, per_tri, per_item = QR.pair(oracle, "clipped", "sizes")
    first = st["tris_setup"] - len(setup)          # the second probe pass's first id: behind the first probe pass and the occluders
    assert first > len(setup) and not t["out"][:first].any() and list(t["out"][first:first + len(setup)]) == list(per_tri) and not t["out"][first + len(setup):].any()
    frame = D.oracle_frame(oracle, "clipped", "DEPTH")[0]
    np.testing.assert_array_equal(got["depth"].view(np.uint32), frame.depth.view(np.uint32), err_msg="a query draws nothing")
    assert st["draws"] == 3 and st["frag_covered"] == int(frame.counters.frag_covered), "a query counts no fragment"


def _box_steps(oracle, frames):
    """(frame, index, step, the recorded inputs, out, status) of every box query of a sequence, the host forms included"""
    for fi, k, s, _, after, a in _walk(oracle, frames):
        if s["op"] == "boxes":
            log = after.box_log[-1]
            yield fi, k, s, log["args"], log["out"], log["srl"]
        elif s["op"] == "boxes_host":
            yield fi, k, s, a["args"], a["out"], a["srl"]


def test_box_answers_are_the_host_builds(oracle, queried):
    """every box query of the query seeds: the model's answer (tests/box_reference.py over the model's depth) equals
    frr_host_query_boxes, the host build of the header the kernels compile, value for value -- and so do a rank's own"""
    import f_renderer_amd as fr
    seen = 0
    for seed, frames in queried.items():
        for fi, k, s, args, out, srl in _box_steps(oracle, frames):
            for rows in (None, M.rank_tile_rows(args["window"], 1, 2, False), M.rank_tile_rows(args["window"], 0, 3, True)):
                want, want_srl = M.box_answer(args, rows)
                host, host_srl = fr.host_query_boxes(args["mvps"], args["lo_hi"], args["flags"], args["size"], args["window"], args["depth"],
                                                     row_owned=None if rows is None else rows.astype(np.uint8), entries=args["entries"])
                np.testing.assert_array_equal(host, want, err_msg=f"seed {seed} frame {fi} step {k}")
                np.testing.assert_array_equal(host_srl, want_srl, err_msg=f"seed {seed} frame {fi} step {k}")
            np.testing.assert_array_equal(M.box_answer(args)[0], out)
            seen += 1
    assert seen >= 6


def test_the_ranks_box_answers_are_zero_together_where_the_whole_answer_is(oracle, queried):
    """The partition rule for box answers: a rank's answer is its own and the ranks' answers do not add up to the unpartitioned
    one, but their sum is zero exactly where the unpartitioned answer is zero -- which is all frr_draw_list_if reads under
    min_value 1.  For every box query of the query seeds, on every world and layout of the partitioned GPU runs."""
    differ = checked = 0
    for seed, frames in queried.items():
        for fi, k, s, args, out, srl in _box_steps(oracle, frames):
            for world in (2, 3, 4):
                for blocked in (False, True):
                    total = sum(M.box_answer(args, M.rank_tile_rows(args["window"], rank, world, blocked))[0].astype(np.int64) for rank in range(world))
                    np.testing.assert_array_equal(total == 0, out == 0, err_msg=f"seed {seed} frame {fi} step {k}, world {world}, blocked {blocked}")
                    differ += int((total != out).sum())
                    checked += out.size
    assert checked > 1000 and differ > 0, (checked, differ)


def test_a_pass_decided_by_a_box_query_is_the_whole_pass(oracle, queried):
    """include/frr.h: `out[i] == 0 implies that drawing item i now changes no entry`.  Every predicated pass of the query seeds
    that a box query of the same list decides under min_value 1, with nothing written to a target and no uniform changed
    between the two, against the same sequence with the unpredicated list pass in its place: colour and depth after the pass
    are equal, and every item the query dropped owns no pixel of the whole pass (the ids differ: the survivors' are dense)."""
    checked = dropped = 0
    for seed, frames in queried.items():
        for fi, k, s, m, _, _ in _walk(oracle, frames):
            if not (s["op"] == "draw" and s["kind"] == "list_if" and s.get("fed") and s.get("source") == "boxes" and s["min"] == 1):
                continue
            steps = frames[fi]
            at = max((j for j in range(k) if steps[j]["op"] == "boxes" and steps[j]["buf"] == s["keep"]), default=None)
            if at is None or _key(steps[at]) != _key(s) or \
                    any(x["op"] in ("draw", "raster", "lines", "wireframe", "shade", "shade_items", "set_uniforms", "set_cull", "clear") for x in steps[at + 1:k]):
                continue
            a, b = m.copy(), m.copy()
            a.apply(s)
            b.apply(dict(s, kind="list"))
            what = f"seed {seed} frame {fi} step {k}"
            np.testing.assert_array_equal(a.frame.color, b.frame.color, err_msg=what)
            np.testing.assert_array_equal(a.frame.depth.view(np.uint32), b.frame.depth.view(np.uint32), err_msg=what)
            first = M.VIS.bounds_of(b.last.per_item, b.last.base).astype(np.int64)
            ids = b.frame.tri_id.astype(np.int64)
            for i, kept in enumerate(a.last.kept):
                if not kept:
                    assert not ((ids >= first[i]) & (ids < first[i + 1]) & (b.frame.tri_id != M.NONE)).any(), f"{what}: dropped item {i} owns a pixel"
                    dropped += 1
            checked += 1
    assert checked >= 3 and dropped >= 3, (checked, dropped)


def test_the_fixed_query_sequences(oracle):
    """frame_model.query_overflows_a_rung and boxes_around_a_draw, which tests/test_gpu_frame_model.py runs: legal on a
    partition, every step felt, and they hold what they are there for"""
    from . import box_reference as BX
    frames = M.query_overflows_a_rung()
    want, = M.run_model(oracle, frames, partitioned=True)
    m = M.Model(oracle, partitioned=True)
    for s in frames[0][:3]:
        m.apply(s)
    assert m.last.fan_rung and m.last.bin_rung and want["crossed"] and want["crossed_fan"]
    n = len(M.LOOP_LIST)
    c0, c2 = want["bufs"]["A.c0"][:3], want["bufs"]["A.c2"][:n + 3]
    assert c0[0] > 0 and (c2[:n] == 0).any() and (c2[:n] > 0).any() and not c2[n:].any(), (c0, c2)
    assert (want["bufs"]["A.c1"][:3] == 0).all(), "a count in front of the pass's raster finds none of its ids"
    assert not M.insensitive_steps(oracle, frames, partitioned=True)
    frames = M.boxes_around_a_draw()
    want = M.run_model(oracle, frames, partitioned=True)
    n = len(M.LOOP_LIST)
    b0, b1, b2 = (want[0]["bufs"][f"A.c{k}"][:n] for k in range(3))
    assert (b0 != b1).any() and (b1 != b2).any() and (b0 != b2).any() and (b2 == 0).any() and (b2 > 0).any()
    st = {int(v) for log in want[0]["boxes"] + want[1]["boxes"] for v in log["srl"][:, 0]}
    assert st >= {BX.NONE, BX.HIDDEN, BX.KEPT, BX.UNBOUNDED}, st
    (_, bounds), (_, host) = want[0]["answers"]
    assert bounds["flags"][3] == 2 and list(host["out"]) == list(b2[:n - 2])
    assert (want[1]["bufs"]["B.c0"][:n] != want[1]["bufs"]["B.c1"][:n]).any(), "the split pass's raster lies between the two"
    assert not M.insensitive_steps(oracle, frames, partitioned=True)


def test_queries_where_they_are_undefined_and_where_they_answer_zeros(oracle):
    lst = [("p100", int(M.M_CLIPPED[0])), ("torus", int(M.M_GRID[1])), ("spiky", int(M.M_CLIPPED[3])), ("empty", int(M.M_GRID[2]))]
    clear, geom = dict(op="clear", window=M.SUB), dict(op="geom", kind="list", vs="PHONG", items=lst, rung=0)
    query = dict(op="query", unit="item", buf="A.c0", entries=6)
    m = M.Model(oracle, partitioned=True)
    m.apply(clear)
    with pytest.raises(M.Undefined):           # before any geometry pass
        m.apply(query)
    m.apply(dict(op="boxes", vs="PHONG", items=lst, buf="A.c1", entries=4))            # a box query needs no pass
    with pytest.raises(M.Undefined):
        m.copy().apply(dict(op="boxes", vs="CLIP_COLOR", items=lst, buf="A.c1", entries=4))
    m.apply(geom)
    before = (m.frame.color.copy(), m.frame.depth.copy(), m.frame.tri_id.copy(), m.stats(), m.last)
    m.apply(query)
    got = m.bufs["A.c0"][:7]
    assert got[0] > 0 and got[3] == 0 and got[4] == got[5] == 0 and got[6] == M.SENTINEL_BITS, got
    assert m.stats() == before[3] and m.last is before[4] and all((a == b).all() for a, b in zip(before[:3], (m.frame.color, m.frame.depth, m.frame.tri_id)))
    # a pass that is not rastered yet counts like any other: the raster changes exactly the entries the triangles' queries
    # count together, at most their sum
    m.apply(dict(op="raster", ps="DEPTH"))
    assert 0 < (m.frame.tri_id != M.NONE).sum() <= int(got[:4].sum())
    again = m.copy()
    again.apply(dict(query, buf="A.c2"))
    assert (again.bufs["A.c2"][:4] <= got[:4]).all() and again.bufs["A.c2"][0] > 0, "rhw == depth passes: the pass's own fragments still count"
    # per triangle: indices below the pass's first id get 0; a dropped item of a predicated pass counts 0
    m.apply(dict(geom, kind="list_if", keep="mask0", keep_entries=8, min=1))
    n = m.last.base + m.last.emit
    m.apply(dict(op="query", unit="triangle", buf="A.c1", entries=n + 3))
    m.apply(dict(query, buf="A.c2"))
    assert not m.bufs["A.c1"][:m.last.base].any() and m.bufs["A.c1"][m.last.base:n].any() and not m.bufs["A.c1"][n:n + 3].any()
    assert m.last.base > 0 and m.bufs["A.c2"][1] == 0 and not m.last.kept[1] and m.bufs["A.c2"][0] > 0
    # after a clear since the pass: zeros per item, and the model leaves the per-triangle form undefined there
    m.apply(clear)
    m.apply(query)
    assert not m.bufs["A.c0"][:6].any()
    with pytest.raises(M.Undefined):
        m.copy().apply(dict(op="query", unit="triangle", buf="A.c1", entries=9))
    # on a partitioned context behind a fused pass: refused, where the count is refused; the box query is not
    m.apply(dict(geom, op="draw", ps="DEPTH"))
    for s in (query, dict(op="query_host", unit="item", entries=4), dict(op="count", unit="item", buf="A.c0", entries=4)):
        with pytest.raises(M.Undefined):
            m.copy().apply(s)
    m.apply(dict(op="boxes", vs="PHONG", items=lst, buf="A.c1", entries=4))
    assert m.box_log[-1]["srl"][3, 0] == 0 and m.prov["A.c1"]["source"] == "boxes"
