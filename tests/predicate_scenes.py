"""Predicated list passes (frr_geometry_list_if / frr_draw_list_if) for tests/test_predicate_cpu.py and
tests/test_gpu_predicate.py: the keep masks, the keep rule on the host, and the expected frames.  A predicated pass is by
definition the list pass with the mesh of every dropped item replaced by an empty mesh, so the expected frame is
drawlist_scenes.oracle_list_loop(..., keep=[all or none of item i's inputs]) -- the oracle's loop over the kept items, the
dropped ones still counted as items.  Each expected frame is computed once per process and shared (never modified).

One scene of its own, `hidden`: a large patch in front and, behind it, items it covers completely, beside items that stay
visible -- the scene of the loop draw, count, draw again."""
import numpy as np

from . import drawlist_scenes as D
from . import instanced_scenes as S

W, H, CLEAR = D.W, D.H, D.CLEAR
NONE = 0xFFFFFFFF
THRESHOLD_VALUES = [0, 1, 5, 6, 7, 0x80000000, 0xFFFFFFFF]
THRESHOLD_MINS = [6, 0, 0x80000001]

_HIDDEN = None


def _along_view(s):
    """the point s object units behind the origin as the demo camera (eye (0, 1, 3), looking at the origin) sees it"""
    d = np.array([0.0, -1.0, -3.0]) / np.sqrt(10.0)
    return tuple(d * s)


def _facing():
    """a patch turned to face the demo camera"""
    return S.rot_x(-np.arctan2(1.0, 3.0))


def scene(name):
    """drawlist_scenes.scene, and `hidden`: items 0 and 3 beside the cover, item 2 the cover, items 1, 4 and 5 behind it -- one
    before and two after it in list order, so that one loses its pixels to a later item and two never get any"""
    global _HIDDEN
    if name != "hidden":
        return D.scene(name)
    if _HIDDEN is None:
        col = S._col_major
        models = np.stack([
            col(S.translate(-1.15, 0.0, 0.0) @ S.rot_y(0.3) @ S.scale(0.8)),
            col(S.translate(*_along_view(0.5)) @ _facing() @ S.scale(0.8)),
            col(S.translate(*_along_view(-0.6)) @ _facing() @ S.scale(2.2)),           # the cover, in front
            col(S.translate(1.15, 0.1, 0.0) @ S.rot_y(-0.3) @ S.scale(0.8)),
            col(S.translate(*_along_view(1.0)) @ _facing() @ S.rot_y(0.4) @ S.scale(0.6)),
            col(S.translate(*_along_view(0.25)) @ _facing() @ S.scale(0.5)),
        ])
        meshes = [D.Mesh(S.patch(60)), D.Mesh(S.patch(200)), D.Mesh(S.patch(70))]
        _HIDDEN = D.Scene(meshes, [0, 2, 1, 0, 2, 0], models, "PHONG", "PHONG")
    return _HIDDEN


def kept_of(values, min_value):
    """the keep rule on the host: NumPy's unsigned >= (frr_rules.h: item_kept)"""
    return np.asarray(values, np.uint32) >= np.uint32(min_value)


def oracle_keep(sc, kept):
    """drawlist_scenes.oracle_list_loop's `keep`: all of a kept item's inputs, none of a dropped item's"""
    kept = np.asarray(kept, bool)
    assert kept.shape == (sc.nitems,)
    return [np.full(n, bool(k), bool) for n, k in zip(sc.ntris, kept)]


def masks(n, seed=20261020):
    """the named masks over n items: all, none, first, last, alternating, a seeded random one"""
    idx = np.arange(n)
    rnd = np.random.default_rng(seed + n).integers(0, 2, n).astype(bool)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": idx == 0, "last": idx == n - 1,
            "alternating": idx % 2 == 0, "random": rnd}


def sizes_masks():
    """on `sizes` (5, 100, 255, 256, 257, 513, 1): the 256-triangle item alone dropped; 255 and 257 dropped around a kept 256"""
    s = np.array(D.SIZES)
    return {"drop256": s != 256, "drop255_257": (s != 255) & (s != 257)}


CLIPPED_SPIKY, CLIPPED_NEAR = 5, 2       # items of drawlist_scenes' `clipped`: first and last input clipped; through the near plane


def clipped_masks():
    idx = np.arange(scene("clipped").nitems)
    return {"drop_spiky": idx != CLIPPED_SPIKY, "only_spiky": idx == CLIPPED_SPIKY, "drop_near": idx != CLIPPED_NEAR}


def gpu_cases():
    """every (scene, label, kept mask) tests/test_gpu_predicate.py holds against expected(): tests/test_predicate_cpu.py
    holds expected() itself to the definition on the same cases"""
    out = []
    for name in D.BOUNDARY:
        out += [(name, k, m) for k, m in masks(scene(name).nitems).items()]
    out += [("sizes", k, m) for k, m in sizes_masks().items()]
    out += [("sizes", "min%x" % mv, kept_of(THRESHOLD_VALUES, mv)) for mv in THRESHOLD_MINS]
    out += [("clipped", k, m) for k, m in clipped_masks().items()]
    out += [("mix", "drop%d" % i, np.arange(scene("mix").nitems) != i) for i in range(scene("mix").nitems)]
    return out


_EXPECTED = {}


def expected(oracle, name, kept, ps=None):
    """(Frame, setup list, triangles emitted per item -- 0 for a dropped one) of the named list under the mask"""
    key = (name, tuple(bool(k) for k in kept), ps)
    if key not in _EXPECTED:
        sc = scene(name)
        _EXPECTED[key] = D.oracle_list_loop(oracle, sc, ps, keep=oracle_keep(sc, kept))
    return _EXPECTED[key]


def item_counts(tri_id, per):
    """pixels per item of a frame's triangle ids: np.bincount over the items' id ranges"""
    ids = np.asarray(tri_id).ravel()
    ids = ids[ids != NONE].astype(np.int64)
    bounds = np.cumsum([0] + list(per))
    assert ids.size == 0 or ids.max() < bounds[-1]
    item = np.searchsorted(bounds, ids, side="right") - 1
    return np.bincount(item, minlength=len(per)).astype(np.uint32)


def hidden_counts(oracle):
    """The per-item pixel counts of `hidden` drawn whole, by the CPU oracle -- and the scene's condition, asserted here and
    nowhere softened: at least one item without a pixel, at least two with some."""
    f, _, per = expected(oracle, "hidden", np.ones(scene("hidden").nitems, bool))
    counts = item_counts(f.tri_id, per)
    assert (counts == 0).sum() >= 1 and (counts > 0).sum() >= 2, counts
    return counts


def kept_scene(sc, kept):
    """the list of the kept items alone: what a caller uploads today instead"""
    idx = [i for i in range(sc.nitems) if kept[i]]
    return D.Scene(sc.meshes, [sc.which[i] for i in idx], sc.models[idx], sc.vs, sc.ps, nf=sc.nf)
