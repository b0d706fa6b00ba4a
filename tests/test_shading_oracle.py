"""The hostile-attribute scenes of tests/shading_scenes.py without a GPU: the two CPU restatements (C: oracle/frr_oracle.c,
NumPy: oracle/oracle_np.py) agree on every one of them bit for bit, and every scene meets its input conditions -- asserted
from oracle output, so that a class cannot go dead unnoticed.  tests/test_gpu_shading_edges.py runs the same scenes on the
GPU against the C oracle.

Before oracle_np had its f32_max (Rust's f32::max: a NaN operand yields the other one, phong.rs:138,143) the cross-check
failed on the normals classes: np.maximum kept the NaN that normalize() makes of a zero or underflowing normal.
"""
import numpy as np
import pytest

from . import shading_scenes as ss
from .conftest import assert_depth_equal

SCENES = ss.names()
NAN_RHW = ("clip_rhw",)                 # the only scene whose 1/w interpolates to NaN: the clipper's ratios overflow at w ~ 2^126
MIN_NORMAL = np.float32(2.0 ** -126)
_c, _np = {}, {}


def _c_frame(oracle, name):
    if name not in _c:
        _c[name] = ss.oracle_frame(oracle, ss.all_scenes()[name])      # raises if the reference would have panicked
    return _c[name]


def _np_frame(name):
    if name not in _np:
        debug = {}
        with np.errstate(all="ignore"):
            _np[name] = dict(ss.numpy_frame(ss.all_scenes()[name], debug), debug=debug)
    return _np[name]


def _same_bits(a, b, what):
    """Bit for bit, except that a NaN only has to be a NaN (conftest.assert_depth_equal's rule)."""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    an, bn = np.isnan(a), np.isnan(b)
    np.testing.assert_array_equal(an, bn, err_msg=what + " (NaN positions)")
    np.testing.assert_array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn], err_msg=what)


def _owner_of_pixels(oracle, name, tri_id):
    own = ss.owners(oracle, ss.all_scenes()[name])
    out = np.full(tri_id.shape, "", dtype=own.dtype)
    drawn = tri_id != 0xFFFFFFFF
    out[drawn] = own[tri_id[drawn]]
    return out


def _not_unit(v):
    """Per pixel: the vector has a NaN or its squared length is not 1 within 1e-5 (a normalised f32 vector is within 4e-7)."""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        return ~(np.abs((v * v).sum(axis=1) - 1.0) < 1e-5)


def _dot_f32(v):
    with np.errstate(all="ignore"):
        return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


# ---- the two restatements agree ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_c_and_numpy_oracles_agree(oracle, name):
    sc = ss.all_scenes()[name]
    c, n = _c_frame(oracle, name), _np_frame(name)
    f = c["frame"]
    K = oracle.vs_num_varyings(getattr(oracle, "VS_" + sc.vs))
    for setup_c, setup_np in zip(c["setup"], n["setup"]):
        assert len(setup_np) == setup_c.shape[0]
        if not len(setup_np):
            continue
        np.testing.assert_array_equal(np.array([[v["spi"] for v in tri] for tri in setup_np], np.int32), setup_c["spi"])
        _same_bits(np.array([[v["spf"] for v in tri] for tri in setup_np]), setup_c["spf"], "spf")
        _same_bits(np.array([[v["rhw"] for v in tri] for tri in setup_np]), setup_c["rhw"], "rhw")
        if K:
            _same_bits(np.array([[v["ctx"] for v in tri] for tri in setup_np]), setup_c["ctx"][..., :K], "ctx")
    assert n["covered"] == f.counters.frag_covered
    np.testing.assert_array_equal(n["tri_id"], f.tri_id, err_msg="triangle ids differ")
    assert_depth_equal(n["depth"], f.depth)
    bad = np.flatnonzero((n["color"].reshape(-1, 4) != f.color.reshape(-1, 4)).any(axis=1))
    if bad.size:
        per_sub = dict(zip(*np.unique(_owner_of_pixels(oracle, name, f.tri_id)[bad], return_counts=True)))
        pytest.fail(f"{name}: RGBA8 of the two oracles differs on {bad.size} pixels, by sub-class {per_sub}")


# ---- every scene meets its conditions ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_scene_conditions(oracle, name):
    sc = ss.all_scenes()[name]
    f = _c_frame(oracle, name)["frame"]
    oc = f.counters.as_dict()
    if name in NAN_RHW:
        assert oc["frag_nan"] > 0, oc
    else:
        assert oc["frag_nan"] == 0, oc
    assert int((f.tri_id != 0xFFFFFFFF).sum()) >= 500
    assert ss.tiles_drawn(f.tri_id) >= 4
    per_sub = ss.pixels_per_sub(oracle, sc, f.tri_id)
    for s in set(sc.sub.tolist()) | set(sc.then[1].tolist() if sc.then else ()):
        assert per_sub.get(s, 0) >= 100, (s, per_sub)
    if sc.family == "clip":
        assert oc["tris_setup"] >= oc["tris_in"] + 100, oc          # the clipper made fans


def test_subnormal_depths_decide_z_tests(oracle):
    """>= 300 pixels end on a positive subnormal depth, and the z-test decided between two subnormal fragments both ways.
    Every triangle is redrawn alone (nothing of this class is clipped: one setup triangle each); replaying `rhw < depth`
    (renderer.rs:363) over those fragments in submission order must give the frame and its frag_zpass."""
    sc = ss.all_scenes()["rhw/depth"]
    f = _c_frame(oracle, "rhw/depth")["frame"]
    final_subnormal = (f.depth > 0) & (f.depth < MIN_NORMAL)
    assert int(final_subnormal.sum()) >= 300
    cur = np.zeros(sc.W * sc.H, np.float32)
    zpass = won = lost = 0
    u = oracle.make_uniforms()
    for tri in np.concatenate([sc.mesh, sc.then[0]]):
        one = oracle.Frame(sc.W, sc.H)
        one.clear(ss.CLEAR, 0.0)
        one.draw(tri[None], oracle.VS_CLIP, oracle.PS_DEPTH, u)
        assert one.counters.tris_setup == 1
        m, d = one.tri_id != 0xFFFFFFFF, one.depth
        both = m & (cur > 0) & (cur < MIN_NORMAL) & (d > 0) & (d < MIN_NORMAL)
        passed = m & ~(d < cur)
        won += int((both & (d > cur)).sum())
        lost += int((both & (d < cur)).sum())
        zpass += int(passed.sum())
        cur[passed] = d[passed]
    np.testing.assert_array_equal(cur.view(np.uint32), f.depth.view(np.uint32))
    assert zpass == f.counters.frag_zpass and zpass < f.counters.frag_covered
    assert won >= 1 and lost >= 1, (won, lost)


def _lighting(oracle, name):
    n = _np_frame(name)
    own = _owner_of_pixels(oracle, name, n["tri_id"])
    return n["debug"], own, own == ss.ORDINARY


@pytest.mark.parametrize("ps", ["phong", "blinn"])
def test_normals_classes_reach_the_degenerate_normalisations(oracle, ps):
    """normalize() of a zero normal, of one whose dot underflows to 0, overflows, or holds inf / NaN is not a unit vector on
    ANY pixel of those sub-classes; the ordinary pixels beside them are all unit."""
    for scene, subs in ((f"normals_small/{ps}", ("zero3", "dot_underflow")), (f"normals_big/{ps}", ss.NORMALS_BIG)):
        dbg, own, ordinary = _lighting(oracle, scene)
        bad = _not_unit(dbg["normal"])
        assert not bad[ordinary].any()
        for s in subs:
            assert (own == s).sum() >= 100 and bad[own == s].all(), (scene, s, int(bad[own == s].sum()), int((own == s).sum()))
        if "small" in scene:
            d = _dot_f32(dbg["ctx"][:, 2:5])[own == "dot_subnormal"]
            assert ((d > 0) & (d < MIN_NORMAL)).sum() >= 100       # the dot product itself is a subnormal


@pytest.mark.parametrize("ps", ["phong", "blinn"])
def test_light_classes_reach_the_degenerate_vectors(oracle, ps):
    """Counted on the ORDINARY pixels (unit normals): which of l, v and the reflection / half vector each uniform set breaks,
    from the NumPy restatement's intermediates."""
    def counts(name):
        dbg, _, o = _lighting(oracle, f"{name}/{ps}")
        return dbg, o, int(o.sum()), {k: int(_not_unit(dbg[k])[o].sum()) for k in ("normal", "light_dir", "view_dir", "spec_dir")}

    dbg, o, n, c = counts("light_eq_view")
    assert n >= 2000 and c == dict(normal=0, light_dir=0, view_dir=0, spec_dir=0), c
    dbg, o, n, c = counts("light_huge")                 # |l|^2 overflows: 1 / sqrt(inf) = 0, l = 0
    assert c["light_dir"] == n and c["view_dir"] == 0, c
    dbg, o, n, c = counts("light_inf")                  # inf * 0 = NaN
    assert c["light_dir"] == n and c["spec_dir"] == n and np.isnan(dbg["light_dir"][o]).any(axis=1).all(), c
    dbg, o, n, c = counts("view_huge")
    assert c["view_dir"] == n and c["light_dir"] == 0, c
    dbg, o, n, c = counts("tiny_world")                 # l.l and v.v are subnormals with a handful of bits
    wpos = dbg["ctx"][:, 5:8]
    u = ss.all_scenes()[f"tiny_world/{ps}"].uniforms
    for key, vec in (("light_dir", np.asarray(u["light_pos"], np.float32) - wpos), ("view_dir", np.asarray(u["view_pos"], np.float32) - wpos)):
        d = _dot_f32(vec)[o]
        assert ((d > 0) & (d < MIN_NORMAL)).all() and c[key] >= 1000, (key, c)
    if ps == "blinn":
        # l + v: exactly zero-length under the light on one pixel (mirrored_near), subnormal-length in a disc of
        # x^2 + y^2 < 0.58 NDC units, 45 % of the frame (mirrored_far)
        dbg, o, n, c = counts("mirrored_near")
        assert (_dot_f32(dbg["spec_vec"])[o] < MIN_NORMAL).sum() >= 1 and c["spec_dir"] >= 1, c
        dbg, o, n, c = counts("mirrored_far")
        assert (_dot_f32(dbg["spec_vec"])[o] < MIN_NORMAL).sum() >= 1000, c
    # light colours and specular strengths: where the lighting sum is NaN or not positive
    def sums(name):
        dbg, _, o = _lighting(oracle, f"{name}/{ps}")
        black = (_np_frame(f"{name}/{ps}")["color"].reshape(-1, 4)[:, :3] == 0).all(axis=1)
        return dbg, int(o.sum()), np.isnan(dbg["light"]).any(axis=1)[o], (dbg["light"] <= 0).any(axis=1)[o], black[o], o
    dbg, n, nan, nonpos, black, o = sums("lc_zero_spec_neg")          # every term is 0 * x or -1 * s * 0
    assert nonpos.all() and black.all() and not nan.any()
    dbg, n, nan, nonpos, black, o = sums("lc_neg_spec_1e30")          # r and b are negative on every pixel, g is not
    assert nonpos.all() and not black.any()
    dbg, n, nan, nonpos, black, o = sums("lc_1e30_spec_inf")          # inf * s^32 is NaN exactly where s^32 == 0
    s32 = dbg["spec"][o]
    with np.errstate(all="ignore"):
        for _ in range(5):
            s32 = s32 * s32
    assert nan.sum() >= 100 and np.array_equal(nan, s32 == 0) and np.array_equal(black, nan)
    dbg, n, nan, nonpos, black, o = sums("lc_inf_spec_zero")          # 0 * s * inf
    assert nan.all()


def test_texels_of_at_least_64_go_black_only_through_nan(oracle):
    """Every texel >= 64 and ambient 0.1: a covered pixel with RGB (0, 0, 0) needs a NaN (or a non-positive lighting sum,
    which the default light cannot give).  Exactly the uv_nan pixels are black; the zero-normal pixels are NOT -- f32::max
    turns their NaN dot products into 0.0 and the ambient term remains (phong.rs:138,143,153)."""
    f = _c_frame(oracle, "tex_ge64")["frame"]
    own = _owner_of_pixels(oracle, "tex_ge64", f.tri_id)
    black = (f.color.reshape(-1, 4)[:, :3] == 0).all(axis=1)
    assert (own == "uv_nan").sum() >= 1000 and (own == "normal_zero").sum() >= 1000
    np.testing.assert_array_equal(black, own == "uv_nan")
    dbg = _np_frame("tex_ge64")["debug"]
    with np.errstate(invalid="ignore"):
        dead = np.isnan(dbg["tex"][:, :3]).any(axis=1) | np.isnan(dbg["light"]).any(axis=1) | (dbg["light"] <= 0).any(axis=1)
    assert int(dead.sum()) == int(black.sum())
    assert np.isnan(dbg["normal"][own == "normal_zero"]).any(axis=1).sum() >= 500


def test_every_byte_value_is_sampled_in_every_channel(oracle):
    """tex_all_bytes: the texels the ordinary pixels touch (renderer.rs:519-525) hold all 256 byte values in all 4 channels."""
    sc = ss.all_scenes()["tex_all_bytes"]
    dbg, _, o = _lighting(oracle, "tex_all_bytes")
    uv = dbg["ctx"][o, 0:2]
    assert ((uv >= 0) & (uv < 1)).all()
    x1, y1 = (uv[:, 0] * np.float32(64)).astype(np.int64), (uv[:, 1] * np.float32(64)).astype(np.int64)
    x2, y2 = np.minimum(x1 + 1, 63), np.minimum(y1 + 1, 63)
    used = np.concatenate([sc.texture[y, x] for x in (x1, x2) for y in (y1, y2)])
    for ch in range(4):
        assert np.unique(used[:, ch]).size == 256
