"""The clipper scenes of tests/clip_scenes.py without a GPU: the two CPU restatements (C: oracle/frr_oracle.c, NumPy:
oracle/oracle_np.py) agree on them bit for bit -- setup lists and frames -- and every family reaches what it was built for,
asserted from oracle output so that a later edit of a builder cannot hollow the suite out.  tests/test_gpu_clip_edges.py runs
the same scenes on the GPU against the C oracle.

The NumPy restatement takes about 0.7 ms per input, so it sees the `patterns` subset and a fixed stride of the full cube; the C
oracle sets up the whole cube (1.4 s) and counts its fans.  The subset's frame is compared in full in the colour layout; in the
clip layout (the same positions, no varyings) its setup list in full and the PS_DEPTH frame of every fourth input.
"""
import numpy as np
import pytest

from . import clip_scenes as cs
from .conftest import assert_depth_equal

SCENES = cs.names()
NP_FRAMES = [n for n in SCENES if n != "patterns/clip"]
# the fan sizes of the 54^3 cube, as the C oracle counts them (DESIGN.md records the same table)
CUBE_FANS = {1: 354, 2: 192, 3: 3420, 4: 1536, 5: 14928, 6: 6336, 7: 34728, 8: 13056, 9: 44784, 10: 13872, 11: 24258}
_c, _np, _fans = {}, {}, {}


def _c_frame(oracle, name):
    if name not in _c:
        _c[name] = cs.oracle_frame(oracle, cs.all_scenes()[name])          # raises if the reference would have panicked
    return _c[name]


def _np_frame(name):
    if name not in _np:
        _np[name] = cs.numpy_frame(cs.all_scenes()[name])
    return _np[name]


def _fans_of(oracle, family):
    if family not in _fans:
        _fans[family] = cs.oracle_fans(oracle, cs.all_scenes()[family + "/clip"])
    return _fans[family]


def _same_bits(a, b, what):
    """Bit for bit, NaNs included: both restatements run on the same machine."""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=what)


def _assert_setup_agrees(setup_np, setup_c, K, note):
    assert len(setup_np) == setup_c.shape[0], note
    if not len(setup_np):
        return
    np.testing.assert_array_equal(np.array([[v["spi"] for v in tri] for tri in setup_np], np.int32), setup_c["spi"], err_msg=note)
    _same_bits(np.array([[v["spf"] for v in tri] for tri in setup_np]), setup_c["spf"], note + ": spf")
    _same_bits(np.array([[v["rhw"] for v in tri] for tri in setup_np]), setup_c["rhw"], note + ": rhw")
    if K:
        _same_bits(np.array([[v["ctx"] for v in tri] for tri in setup_np]), setup_c["ctx"][..., :K], note + ": ctx")


# ---- the two restatements agree ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NP_FRAMES)
def test_c_and_numpy_oracles_agree(oracle, name):
    """Setup lists (spi, spf, rhw, ctx[:K]) and frames (covered fragments, ids, depth bits, RGBA8)."""
    sc = cs.all_scenes()[name]
    c, n = _c_frame(oracle, name), _np_frame(name)
    f = c["frame"]
    _assert_setup_agrees(n["setup"], c["setup"], oracle.vs_num_varyings(getattr(oracle, "VS_" + sc.vs)), name)
    assert n["covered"] == f.counters.frag_covered
    np.testing.assert_array_equal(n["tri_id"], f.tri_id, err_msg="triangle ids differ")
    assert_depth_equal(n["depth"], f.depth)
    np.testing.assert_array_equal(n["color"], f.color, err_msg="RGBA8 differs")


def test_c_and_numpy_oracles_agree_on_a_depth_frame_of_the_subset(oracle):
    """`patterns/clip` thinned to every fourth input (968 inputs, all fan sizes): the PS_DEPTH frame and its setup list."""
    sc = cs.all_scenes()["patterns/clip"]
    sc = sc._replace(mesh=np.ascontiguousarray(sc.mesh[::4]))
    c, n = cs.oracle_frame(oracle, sc), cs.numpy_frame(sc)
    f = c["frame"]
    assert set(np.unique(cs.kept_counts(sc.mesh)).tolist()) == set(CUBE_FANS)
    _assert_setup_agrees(n["setup"], c["setup"], 0, "patterns/clip[::4]")
    assert n["covered"] == f.counters.frag_covered
    np.testing.assert_array_equal(n["tri_id"], f.tri_id, err_msg="triangle ids differ")
    assert_depth_equal(n["depth"], f.depth)
    np.testing.assert_array_equal(n["color"], f.color, err_msg="RGBA8 differs")


@pytest.mark.parametrize("layout", list(cs.LAYOUTS))
def test_c_and_numpy_setup_lists_agree_on_a_stride_of_the_cube(oracle, layout):
    """Every 157th input of the full cube (1,003 inputs; `patterns/clip`, which has no NumPy frame, in full as well)."""
    from oracle import oracle_np as onp
    full = cs.cube_scene(layout)
    parts = [full.mesh[cs.CUBE_NP_STRIDE]] + ([cs.all_scenes()["patterns/clip"].mesh] if layout == "clip" else [])
    vs_c, vs_n, u_c, u_n = getattr(oracle, "VS_" + full.vs), getattr(onp, "VS_" + full.vs), oracle.make_uniforms(), onp.Uniforms()
    for mesh in parts:
        want = oracle.geometry_batch(cs.W, cs.H, mesh, vs_c, u_c)
        got = []
        with np.errstate(all="ignore"):
            for tri in mesh:
                got.extend(onp.geometry_processing(cs.W, cs.H, tri, vs_n, u_n))
        _assert_setup_agrees(got, want, oracle.vs_num_varyings(vs_c), f"cube stride, {layout}")


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_kept_counts_is_the_oracles_fan_count(oracle, family):
    """clip_scenes.kept_counts (what the builders choose inputs by) is the C oracle's triangle count on every input."""
    sc = cs.all_scenes()[family + "/clip"]
    np.testing.assert_array_equal(cs.kept_counts(sc.mesh), _fans_of(oracle, family))
    assert _fans_of(oracle, family).sum() == _c_frame(oracle, family + "/clip")["frame"].counters.tris_setup


# ---- every family reaches what it was built for ------------------------------------------------------------------------

def test_patterns_cube_reaches_fans_of_1_to_11(oracle):
    """The C oracle's fan size of all 54^3 inputs (from its batch setup list via per-input counts on the subset, and
    kept_counts == those counts): sizes 1 .. 11 and no other, 11 the maximum, with the histogram recorded above."""
    pos = cs.cube()
    total = oracle.geometry_batch(cs.W, cs.H, pos, oracle.VS_CLIP, oracle.make_uniforms()).shape[0]
    n = cs.kept_counts(pos)
    assert total == int(n.sum()) == sum(k * v for k, v in CUBE_FANS.items())
    # per-input counts straight from the oracle on a stride that is coprime to 54 and reaches every size
    idx = np.arange(5, cs.CUBE_N, 23)
    u = oracle.make_uniforms()
    direct = np.array([oracle.geometry_processing(cs.W, cs.H, t, oracle.VS_CLIP, u).shape[0] for t in pos[idx]])
    np.testing.assert_array_equal(direct, n[idx])
    assert set(np.unique(direct).tolist()) == set(range(1, 12)) and direct.max() == 11
    assert dict(zip(*(x.tolist() for x in np.unique(n, return_counts=True)))) == CUBE_FANS


def test_patterns_classes_are_the_54_inside_patterns():
    """Per vertex slot the class table has 27 different inside-bit patterns with w > 0 (no axis with neither of its bits)
    and 27 with w < 0 (no axis with both); eight patterns occur on both sides, so a class is (sign of w, pattern)."""
    for slot in range(3):
        tab = cs.slot_table(slot).astype(np.float32)
        bits = cs.inside_bits(np.repeat(tab[:, None, :], 3, axis=1))[:, 0]
        pos, neg = bits[tab[:, 3] > 0], bits[tab[:, 3] < 0]
        assert np.unique(pos).size == 27 and np.unique(neg).size == 27 and np.unique(bits).size == 46
        assert not any(((pos >> s) & 3 == 0).any() or ((neg >> s) & 3 == 3).any() for s in (0, 2, 4))


def test_patterns_subset_has_every_fan_size_and_every_class_in_every_slot(oracle):
    sc = cs.all_scenes()["patterns/clip"]
    assert sc.mesh.shape[0] <= 4000
    assert set(np.unique(_fans_of(oracle, "patterns")).tolist()) == set(CUBE_FANS)
    cl = cs.cube_classes(sc.meta["cube_index"])
    for slot in range(3):
        assert np.unique(cl[:, slot]).size == 54
        assert np.unique(cs.inside_bits(sc.mesh)[:, slot] + 64 * (sc.mesh[:, slot, 3] < 0)).size == 54


def test_ties_have_equal_sort_keys():
    """From the NumPy restatement's own keys: inputs whose vertex list holds two equal sort keys (only the stable order
    decides between them), among them an intersection that coincides with an original vertex."""
    from oracle import oracle_np as onp
    sc = cs.all_scenes()["ties/clip"]
    equal, dup_of_original = [], 0
    with np.errstate(all="ignore"):
        for i, tri in enumerate(sc.mesh):
            dbg = {}
            onp.geometry_processing(cs.W, cs.H, tri, onp.VS_CLIP, onp.Uniforms(), debug=dbg)
            keys = dbg.get("keys", [])
            if len(set(keys)) < len(keys):
                equal.append(i)
                dup_of_original += bool(set(keys[:dbg["kept"]]) & set(keys[dbg["kept"]:]))
    assert len(equal) >= 1
    assert dup_of_original >= 20, dup_of_original
    kinds = {str(sc.meta["names"][i]).split("_p")[0].split("_w")[0] for i in equal}
    assert {"edge_out", "coincide_inside", "ray"} <= kinds, kinds


def test_epsilon_near_crossings_are_kept_and_dropped_from_2_to_the_7(oracle):
    """(a): every input crosses the near plane and no other, with one vertex behind it or two.  Either way two of its edges
    cross (the edge between two vertices behind does not), so there are 2 intersections and fan - 1 of them were kept.  None
    is kept for k <= 6; for k >= 7 kept AND dropped ones occur."""
    sc = cs.all_scenes()["epsilon/clip"]
    at, k = sc.meta["near"], sc.meta["near_k"]
    bits = cs.inside_bits(sc.mesh[at])
    assert ((bits | 16) == 63).all() and (((bits >> 4) & 1).sum(axis=1) % 3 != 0).all()     # only the near bit, on 1 or 2 vertices
    kept = _fans_of(oracle, "epsilon")[at] - 1
    assert kept.max() <= 2
    assert (kept[k <= 6] == 0).all()
    assert (kept[k >= 7] > 0).sum() >= 10 and (kept[k >= 7] < 2).sum() >= 10
    assert np.unique(k[kept > 0]).size >= 8, np.unique(k[kept > 0])                        # in many octaves, not one


def test_epsilon_mixed_sign_neighbours_differ_in_fan_count(oracle):
    """(b): the two inputs of every committed pair differ in ONE component by one f32 step, and in their fan count."""
    sc = cs.all_scenes()["epsilon/clip"]
    pairs = sc.meta["pairs"]
    assert pairs.shape[0] >= 60
    fans = _fans_of(oracle, "epsilon")
    assert (fans[pairs[:, 0]] != fans[pairs[:, 1]]).all()
    a, b = sc.mesh[pairs[:, 0]].reshape(-1, 12), sc.mesh[pairs[:, 1]].reshape(-1, 12)
    d = a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)
    assert ((d != 0).sum(axis=1) == 1).all() and (np.abs(d).max(axis=1) == 1).all()
    w = sc.mesh[pairs[:, 0]][..., 3]
    assert ((w > 0).any(axis=1) & (w < 0).any(axis=1)).all()


def test_ordinary_inputs_share_the_blocks_of_the_hostile_ones(oracle):
    for family, key in (("epsilon", None), ("nonfinite", "hostile")):
        sc = cs.all_scenes()[family + "/clip"]
        special = np.concatenate([sc.meta["near"], sc.meta["pairs"].ravel()]) if key is None else sc.meta[key]
        assert (special % 2 == 0).all() and special.size * 2 == sc.mesh.shape[0]
        ordinary = np.setdiff1d(np.arange(sc.mesh.shape[0]), special)
        assert (_fans_of(oracle, family)[ordinary] == 1).all() and (cs.inside_bits(sc.mesh[ordinary]) == 63).all()


def test_nonfinite_inputs_are_dropped_kept_and_clipped(oracle):
    sc = cs.all_scenes()["nonfinite/clip"]
    fans = _fans_of(oracle, "nonfinite")[sc.meta["hostile"]]
    assert (fans == 0).sum() >= 1 and (fans == 1).sum() >= 1 and (fans > 1).sum() >= 1
    names = sc.meta["names"]
    zero_w = np.array([("_+0_w_" in n or "_-0_w_" in n) for n in names])
    assert zero_w.sum() == 24 and (fans[zero_w] == 0).all() and (fans[~zero_w] > 0).all()  # renderer.rs:117-119, nothing else
    m = sc.mesh[sc.meta["hostile"]]
    for what in (np.isnan(m), np.isinf(m), np.abs(m) == np.float32(3.4028234663852886e38),
                 (m != 0) & (np.abs(m) < np.float32(2.0 ** -126)), (m == 0) & np.signbit(m)):
        assert what.any(axis=0).all()                        # in every component of every vertex slot
    assert _c_frame(oracle, "nonfinite/clip")["frame"].counters.frag_nan > 0


def test_dense_blocks_hold_nothing_but_large_fans(oracle):
    sc = cs.all_scenes()["dense/clip"]
    fans = _fans_of(oracle, "dense")
    n = fans.size
    assert n >= 3 * cs.GEOM_BLOCK and n % cs.GEOM_BLOCK != 0
    per_block = [int(fans[b:b + cs.GEOM_BLOCK].sum()) for b in range(0, n, cs.GEOM_BLOCK)]
    full = [b for b in range(0, n - cs.GEOM_BLOCK + 1, cs.GEOM_BLOCK) if (fans[b:b + cs.GEOM_BLOCK] >= 10).all()]
    assert len(full) >= 2 and max(per_block) >= 2560, per_block
    assert (fans[:cs.DENSE_BEFORE] == 1).all() and (fans[-cs.DENSE_AFTER:] == 1).all() and fans.max() == 11
