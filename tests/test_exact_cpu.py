"""The two CPU oracles against answers derived in exact arithmetic (no GPU).

oracle/frr_oracle.c and oracle/oracle_np.py are this project's restatements of the reference; tests/exact_reference.py is a
third one that computes in rationals and knows where nothing rounded.  On those values any correct reading of the reference
gives the same bits, so equality there is the assertion (tests/exact_scenes.py: the scenes and the comparison).  The
evaluator itself is held to pixels worked out by hand (tests/golden/kat_exact.json), its rounding helper to numpy's float32,
and the scenes to reaching what they are named for and to seeing three deliberate misreadings of the formulas."""
import json
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

from oracle import oracle_np as onp

from . import exact_reference as er
from . import exact_scenes as es

SCENES = es.names()
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- rn32 ----------------------------------------------------------------------------------------------------------------

def _f32_fraction(bits):
    return Fr(float(np.array([bits], np.uint32).view(np.float32)[0]))


def test_rn32_against_float32():
    """Operands on which a double holds the exact result (sums and products of two f32 of nearby exponents; quotients are
    left out), so np.float32(double) rounds once: ties, one step either side of a tie, exact values, both signs, the edges of
    the normal range."""
    rng = np.random.default_rng(5)
    cases = []
    for bits in (0x3F800000, 0x3F800001, 0x3FFFFFFF, 0x40490FDB, 0x00800000, 0x7F7FFFFF, 0x4B7FFFFF, 0x33800000):
        x = _f32_fraction(bits)
        nxt = _f32_fraction(bits + 1) if bits != 0x7F7FFFFF else None
        cases.append(x)
        if nxt is not None:
            tie = (x + nxt) / 2
            step = (nxt - x) / 4
            cases += [tie, tie - step, tie + step, tie - step / 1024, tie + step / 1024]
    a = rng.integers(0x3D000000, 0x42000000, 400, dtype=np.uint32).view(np.float32)
    b = rng.integers(0x3D000000, 0x42000000, 400, dtype=np.uint32).view(np.float32)
    for x, y in zip(a.tolist(), b.tolist()):
        cases += [Fr(x) * Fr(y), Fr(x) + Fr(y), Fr(x) - Fr(y)]       # 48-bit products, sums within 2^10 of each other: exact in a double
    n_inexact = n_tie = 0
    for c in cases:
        if c == 0:
            continue
        for v in (c, -c):
            assert Fr(float(v)) == v, "the case itself does not fit a double"
            got, exact = er.rn32(v)
            want = Fr(float(np.float32(float(v))))
            assert got == want, (v, got, want)
            assert exact == (got == v)
            n_inexact += not exact
    for bits in (0x3F800000, 0x3F800001):                            # ties to even, said outright: 1 + 2^-24 -> 1, 1 + 3 * 2^-24 -> 1 + 2^-22
        x, nxt = _f32_fraction(bits), _f32_fraction(bits + 1)
        got, exact = er.rn32((x + nxt) / 2)
        assert not exact and got == (x if bits % 2 == 0 else nxt)
        n_tie += 1
    assert n_inexact > 500 and n_tie == 2
    assert er.rn32(0) == (0, True)
    for bad in (Fr(1, 2 ** 127), Fr(2 ** 128), _f32_fraction(0x7F7FFFFF) + Fr(2 ** 103)):
        with pytest.raises(er.Inexact):
            er.rn32(bad)
    assert er.f32_bits(Fr(-3, 2)) == 0xBFC00000 and er.f32_bits(_f32_fraction(0x40490FDB)) == 0x40490FDB


# ---- the hand-checked anchors --------------------------------------------------------------------------------------------

with open(os.path.join(HERE, "golden", "kat_exact.json")) as _fh:
    ANCHORS = json.load(_fh)["anchors"]


@pytest.mark.parametrize("name", list(ANCHORS))
def test_evaluator_reproduces_hand_checked_anchor(name):
    k = ANCHORS[name]
    sc = es.all_scenes()[k["scene"]]
    f = es.frame(k["scene"])
    cx, cy = k["pixel"]
    index = cy * sc.W + cx
    fr_ = f.frag[index]
    assert fr_["pixel"] == (cx, cy) and fr_["tri"] == k["tri"] == f.ids[index]
    assert [[c.v for c in v.spf] for v in fr_["vtx"]] == [[Fr(c) for c in p] for p in k["spf"]]
    assert [list(v.spi) for v in fr_["vtx"]] == k["spi"]
    assert [v.rhw.v for v in fr_["vtx"]] == [Fr(r) for r in k["vtx_rhw"]]
    assert [x.v for x in fr_["abc"]] == [Fr(k["a"]), Fr(k["b"]), Fr(k["c"])]
    assert fr_["s"].v == Fr(k["s"])
    assert [x.v for x in fr_["weights"]] == [Fr(w) for w in k["weights"]]
    assert fr_["rhw"].v == Fr(k["rhw"]) == f.depth[index].v
    assert fr_["depth_exact"] and fr_["setup_exact"]
    if k["rgba"] is not None:
        assert fr_["rgba"] == k["rgba"] == f.color[index] and fr_["color_exact"]


# ---- the oracles against the evaluator -----------------------------------------------------------------------------------

def _oracle_uniforms(oracle, sc, model=None):
    kw = {} if model is None else {"model": model}
    if sc.uniforms:
        u = sc.uniforms
        kw = dict(kw, light_pos=[float(Fr(x)) for x in u["light_pos"]], light_color=[float(Fr(x)) for x in u["light_color"]],
                  ambient=float(Fr(u["ambient"])), specular=float(Fr(u["specular"])))
    c = oracle.make_uniforms(tex=oracle.Texture(es.texture_u8(sc)) if sc.tex is not None else None, **kw)
    n = onp.Uniforms(tex=es.texture_u8(sc) if sc.tex is not None else None, **kw)
    return c, n


def _ids(mod, sc):
    return getattr(mod, "VS_" + sc.vs), getattr(mod, "PS_" + sc.ps.upper())


def _np_setup(setup_np, K):
    dt = np.dtype([("ctx", "<f4", (max(K, 1),)), ("rhw", "<f4"), ("spf", "<f4", (2,)), ("spi", "<i4", (2,))])
    out = np.zeros((len(setup_np), 3), dt)
    for i, tri in enumerate(setup_np):
        for k in range(3):
            out[i, k]["rhw"], out[i, k]["spf"], out[i, k]["spi"] = tri[k]["rhw"], tri[k]["spf"], tri[k]["spi"]
            out[i, k]["ctx"][:K] = tri[k]["ctx"]
    return out


@pytest.mark.parametrize("name", SCENES)
def test_c_oracle_equals_evaluator(oracle, name):
    sc, want = es.all_scenes()[name], es.expected(name)
    vs, ps = _ids(oracle, sc)
    f = oracle.Frame(sc.W, sc.H)
    f.clear()
    setup = np.concatenate([f.draw(es.inputs_f32(sc), vs, ps, _oracle_uniforms(oracle, sc, m)[0], window=sc.window, keep_setup=True,
                                   tri_id_base=int(f.counters.tris_setup)) for m in sc.models_f32()])
    assert f.counters.tris_setup == want.tris_setup and f.counters.frag_covered == want.frag_covered and f.counters.frag_nan == 0
    es.assert_frame(want, sc, f.depth, f.tri_id, f.color, f"{name}, C oracle", setup=setup)


@pytest.mark.parametrize("name", SCENES)
def test_numpy_oracle_equals_evaluator(oracle, name):
    sc, want = es.all_scenes()[name], es.expected(name)
    vs, ps = _ids(onp, sc)
    color = np.zeros((sc.H, sc.W, 4), np.uint8)
    color[...] = es.CLEAR_COLOR
    depth, tid = np.zeros(sc.W * sc.H, np.float32), np.full(sc.W * sc.H, 0xFFFFFFFF, np.uint32)
    shared = sc.window is not None and sc.window[0] < 0          # (rows share depth entries: an entry has no single input)
    debug = None if sc.ps == "depth" or shared else {}
    setup, cov = [], 0
    for m in sc.models_f32():
        s_, c_ = onp.draw(sc.W, sc.H, es.inputs_f32(sc), vs, ps, _oracle_uniforms(oracle, sc, m)[1], color, depth, tid, window=sc.window,
                          tri_id_base=len(setup), debug=debug)
        setup, cov = setup + s_, cov + c_
    assert len(setup) == want.tris_setup and cov == want.frag_covered
    inputs = None
    if debug is not None:
        inputs = debug["ctx"]
        assert not np.isnan(inputs[want.owned]).any() and np.isnan(inputs[~want.owned]).all()
    es.assert_frame(want, sc, depth, tid, color, f"{name}, NumPy oracle", inputs=inputs, setup=_np_setup(setup, want.K))


# ---- what the scenes reach -----------------------------------------------------------------------------------------------

def test_exact_share_of_every_scene():
    """At least three quarters of the owned pixels, and at least 64, are exact through the last value the scene compares (the
    generators assert it too; here the shares are printed)."""
    for name in SCENES:
        sc = es.all_scenes()[name]
        exact, owned = sc.share()
        print(f"{name}: {exact} of {owned} exact through {sc.through} ({100.0 * exact / owned:.1f} %)")
        assert exact >= es.MIN_EXACT and exact * 4 >= owned * 3, name


def test_flat_w_reaches_both_snap_cases_and_tile_borders():
    for name in es.names("flat_w"):
        f = es.frame(name)
        fracs = {c.v % 1 for t in f.setup for v in t for c in v.spf}
        assert fracs == {Fr(0), Fr(1, 2)}, fracs
        for t in f.setup:
            for v in t:                                           # the snap itself: trunc(spf + 0.5)
                assert v.spi == [int(v.spf[0].v + Fr(1, 2)), int(v.spf[1].v + Fr(1, 2))]
        assert any(v.spi[0] != v.spf[0].v for t in f.setup for v in t)
        tiles = {(fr_["tri"], fr_["pixel"][0] // 32, fr_["pixel"][1] // 32) for fr_ in f.frag.values()}
        assert all(len({t[1:] for t in tiles if t[0] == i}) >= 2 for i in range(3))
        assert {v.rhw.v for t in f.setup for v in t} == {{"flat_w1": Fr(1), "flat_w2": Fr(1, 2), "flat_whalf": Fr(2)}[name]}
        assert all(fr_["color_exact"] for fr_ in f.frag.values() if fr_["depth_exact"])


def test_persp_depth_is_exact_where_colour_is_not():
    f = es.frame("persp_color")
    assert {v.rhw.v for t in f.setup for v in t} == {Fr(1), Fr(1, 2), Fr(1, 4)}
    exact_depth = [fr_ for fr_ in f.frag.values() if fr_["depth_exact"]]
    assert len(exact_depth) >= 64 and sum(not fr_["input_exact"] for fr_ in exact_depth) >= 64      # 1 / rhw rounds
    assert len({fr_["rhw"].v for fr_ in exact_depth}) >= 64      # the depth varies from pixel to pixel


def test_layers_reach_a_tie_a_shared_edge_and_every_order():
    for name in es.names("layers"):
        sc, f = es.all_scenes()[name], es.frame(name)
        ta, tb = sc.expect["tie"]
        owners = set(f.ids)
        assert tb in owners and ta not in owners                   # an exact tie: the later triangle owns every pixel (:363)
        tied = [fr_ for fr_ in f.frag.values() if fr_["tri"] == tb]
        assert len(tied) >= 64 and all(fr_["depth_exact"] and fr_["rhw"].v == Fr(1, 2) for fr_ in tied)
        ea, eb = sc.expect["edge_pair"]
        px = sorted(fr_["pixel"] for fr_ in f.frag.values() if fr_["tri"] in (ea, eb))
        assert px == sorted((x, y) for x in range(8, 24) for y in range(44, 60))      # every pixel of the square, once
        assert any(fr_["tri"] == ea for fr_ in f.frag.values()) and any(fr_["tri"] == eb for fr_ in f.frag.values())
        pair = es.Scene("pair", sc.W, sc.H, sc.vs, sc.ps, [sc.tris[ea], sc.tris[eb]], "color").evaluate()
        assert pair.frag_covered == 256                            # covered exactly once: no fragment of one under the other
        near, mid, far = (sc.expect["order"].index(n) for n in ("near", "mid", "far"))
        at = lambda x, y: f.ids[y * sc.W + x]
        assert at(10, 10) == near and at(12, 30) == mid and at(30, 12) == far      # decided by rhw, not by submission order
        assert all(f.frag[y * sc.W + x]["depth_exact"] for x, y in ((10, 10), (12, 30), (30, 12)))
    assert [es.all_scenes()[n].expect["order"].index("near") for n in es.names("layers")] == [0, 1, 2]


def test_clipped_reaches_each_plane_and_a_fan():
    crossed = set()
    for name in es.names("clipped"):
        sc, f = es.all_scenes()[name], es.frame(name)
        for t in sc.vs_out():
            pos = [er.xs(p) for p, _ in t]
            ins = [[er.insides(pl, p) for pl in er.PLANES] for p in pos]
            here = {pl for k, pl in enumerate(er.PLANES) if len({ins[i][k] for i in range(3)}) == 2}
            crossed |= here
            for i in range(3):
                for j in range(i + 1, 3):
                    for k, pl in enumerate(er.PLANES):
                        if ins[i][k] != ins[j][k]:
                            r = er.intersect_ratio(pl, pos[i], pos[j])
                            assert r.ex, (name, pl)                  # the ratio, and so the new vertex, is exact
                            if pl != "Z_NEAR":                       # (1/4 from the inside vertex is 3/4 from the outside one)
                                assert min(r.v, 1 - r.v) in (Fr(1, 2), Fr(1, 4)), (name, pl, r)
        assert set(sc.expect["planes"]) <= {pl for t in sc.vs_out() for k, pl in enumerate(er.PLANES)
                                            if len({er.insides(pl, er.xs(p)) for p, _ in t}) == 2}
        assert f.tris_setup > len(sc.tris) or sc.expect.get("dropped")
        assert all(v.ex for t in f.setup for v in t)
    assert crossed == {"X_RIGHT", "Y_UP", "Z_FAR", "Z_NEAR"}
    f = es.frame("clipped_z_near")
    assert f.tris_setup == 2                                       # :70 puts the new vertex at w = 0 and :164 drops it
    sc, f = es.all_scenes()["clipped_two_planes"], es.frame("clipped_two_planes")
    assert f.tris_setup == 3 + 5 + 3                               # four new vertices: a fan of five between two fans of three
    owners = {fr_["tri"] for fr_ in f.frag.values()}
    assert len(owners & set(range(3, 8))) >= 2, owners             # (the others have no area or lie off the screen)
    assert any(not (0 <= v.spi[0] <= sc.W and 0 <= v.spi[1] <= sc.H) for t in f.setup for v in t)   # spi outside the frame


def test_windowed_reaches_sub_windows_and_shared_entries():
    for name in es.names("windowed"):
        sc, f = es.all_scenes()[name], es.frame(name)
        x0, x1, y0, y1 = sc.window
        assert all(x0 <= fr_["pixel"][0] < x1 and y0 <= fr_["pixel"][1] < y1 for fr_ in f.frag.values())
        if x0 > 0:
            assert y0 > 0
            full = es.frame({"windowed_sub_flat_w1": "flat_w1", "windowed_sub_layers": "layers_near_first"}[name])
            assert 0 < len(f.frag) < len(full.frag)                 # the window cuts the triangles
            for i, fr_ in f.frag.items():                           # entry (cy - y0) * x1 + (cx - x0) holds the whole frame's pixel
                cx, cy = fr_["pixel"]
                assert i == (cy - y0) * x1 + (cx - x0) and full.frag[cy * sc.W + cx]["rhw"].v == fr_["rhw"].v
        else:
            # an entry reached from two rows: index_x = cx - x0 goes up to 63, the stride is 48
            reach = {}
            for cy in range(y0, y1):
                for cx in range(x0, x1):
                    reach.setdefault((cy - y0) * x1 + (cx - x0), set()).add(cy)
            shared = [i for i in f.frag if len(reach[i]) == 2]
            assert shared, name
            # the owner of a shared entry is the fragment the raster order and the depth rule leave there; at least one such
            # entry lies off its owner's own row start, i.e. was written through index_x >= x1
            assert any(f.frag[i]["pixel"][0] - x0 >= x1 for i in shared), name


def test_textured_reaches_the_clamped_row_and_the_borders():
    for name, (tw, th) in (("textured_4x4", (4, 4)), ("textured_4x8", (4, 8))):
        sc, f = es.all_scenes()[name], es.frame(name)
        tex = f.uniforms.tex
        assert (tex.width, tex.height) == (tw, th)
        ys = {y for _, y in tex.reached}
        assert max(ys) == tw - 1                                    # y1, y2 are clamped by the WIDTH (:523, :525)
        if th > tw:
            assert all(y < tw for y in ys) and any(fr_["input"][1].v * th >= tw for fr_ in f.frag.values())
        assert {x for x, _ in tex.reached} == set(range(tw))
        us = {fr_["input"][0].v for fr_ in f.frag.values()} | {fr_["input"][1].v for fr_ in f.frag.values()}
        assert Fr(0) in us and Fr(1) in us and Fr(1, 64) < min(us - {Fr(0)}) < Fr(1, 16) and Fr(15, 16) < max(us - {Fr(1)}) < 1   # 0, 1, and just inside
        assert any((u * tw) % 1 == 0 for u in us)                   # on a texel border
        robust = [fr_ for fr_ in f.frag.values() if fr_["robust"] and not fr_["color_exact"]]
        assert len(robust) >= 64                                    # bytes that rounded on the way and cannot depend on it
        assert all(fr_["input_exact"] for fr_ in f.frag.values() if fr_["depth_exact"])      # w = 1: exact weights, exact input


# ---- the scenes can see a misread formula --------------------------------------------------------------------------------

def _changed_exact_pixels(name, perturb):
    """How many exact pixels of the scene change their id, depth or bytes under the perturbed evaluator."""
    sc, f = es.all_scenes()[name], es.frame(name)
    g = sc.evaluate(perturb={perturb})
    n = 0
    for i in f.exact_entries(sc.through):
        a, b = f.frag[i], g.frag.get(i)
        n += b is None or f.ids[i] != g.ids[i] or a["rhw"].v != b["rhw"].v or (sc.through == "color" and a["rgba"] != b["rgba"])
    return n


@pytest.mark.parametrize("perturb,scenes", [("swap_ab", ["persp_depth", "flat_w1"]), ("no_half", ["persp_depth", "flat_w1"]),
                                            ("near_plus", ["clipped_z_near"])])
def test_scenes_see_a_misread_formula(perturb, scenes):
    changed = {name: _changed_exact_pixels(name, perturb) for name in scenes}
    print(perturb, changed)
    assert all(n > 0 for n in changed.values()), changed
