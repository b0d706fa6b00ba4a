"""Scenes of the box query (frr_drawlist_bounds / frr_query_boxes) for tests/test_boxes_cpu.py and tests/test_gpu_boxes.py:
draw lists in the 128 x 96 frame of tests/drawlist_scenes.py under the demo camera, the depth they are tested against (the
cover of predicate_scenes' `hidden` drawn alone, unless a case brings its own), and the windows and ownership masks.  Every
oracle result is computed once per process and shared (never modified)."""
import numpy as np

from . import box_reference as R
from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import predicate_scenes as P

W, H = D.W, D.H
FULL = (0, W, 0, H)
# sub-windows with x0, y0 > 0 and sizes that are no multiples of 4 or 32; one pixel; one row; one column
WINDOWS = [FULL, (3, 125, 5, 91), (17, 82, 33, 70), (40, 41, 50, 51), (0, W, 47, 48), (64, 65, 0, H), (1, 36, 2, 35)]
# world 2 over the frame's three tile rows: (rank, blocked) -> one byte per tile row
ROW_MASKS = {(0, False): [1, 0, 1], (1, False): [0, 1, 0], (0, True): [1, 1, 0], (1, True): [0, 0, 1]}


def camera():
    """(proj, view) of the demo camera, float32 [16] column-major, by the library's own host helpers"""
    import f_renderer_amd as fr
    kw = S.camera_kw(fr)
    return np.asarray(kw["proj"], np.float32).reshape(16), np.asarray(kw["view"], np.float32).reshape(16)


_SCENES = {}


def scene(name):
    """prototype: the 6 items of `hidden`, a 6 x 4 grid of small patches on a plane behind the cover, and a patch under the six
    clipped_models() -- 36 items: some behind the cover, some beside it, one through the near plane, one off-screen.
    clipped / nonfinite: patch(100) under instanced_scenes' matrices.  sizes: patches of growing scale facing the camera
    (rectangles of every pyramid level)."""
    if name in _SCENES:
        return _SCENES[name]
    col = S._col_major
    if name == "prototype":
        h = P.scene("hidden")
        meshes = list(h.meshes) + [D.Mesh(S.patch(100))]
        which, models = list(h.which), [m for m in h.models]
        base = np.array(P._along_view(0.9))
        for gy in range(4):
            for gx in range(6):
                t = base + np.array([0.55 * (gx - 2.5), 0.5 * (gy - 1.5), 0.0])
                which.append(0)
                models.append(col(S.translate(*t) @ P._facing() @ S.scale(0.45)))
        for m in S.clipped_models():
            which.append(3)
            models.append(m)
        sc = D.Scene(meshes, which, np.stack(models), "PHONG", "PHONG")
    elif name == "clipped":
        sc = D.Scene([D.Mesh(S.patch(100))], [0] * 6, S.clipped_models(), "PHONG", "PHONG")
    elif name == "nonfinite":
        sc = D.Scene([D.Mesh(S.patch(100))], [0] * 4, S.nonfinite_models(), "PHONG", "PHONG")
    elif name == "sizes":
        scales = [0.02, 0.1, 0.2, 0.4, 0.8, 1.5, 3.0, 6.0]
        models = [col(S.translate(*P._along_view(-0.2 + 0.05 * k)) @ P._facing() @ S.scale(s)) for k, s in enumerate(scales)]
        sc = D.Scene([D.Mesh(S.patch(60))], [0] * len(scales), np.stack(models), "PHONG", "PHONG")
    else:
        raise KeyError(name)
    _SCENES[name] = sc
    return sc


NAMES = ["prototype", "clipped", "nonfinite", "sizes"]


def bounds(sc):
    """(lo_hi [n, 6], flags [n]) of the list's items by NumPy"""
    per_mesh = [R.bounds_of(m.tris) for m in sc.meshes]
    lo_hi = np.stack([per_mesh[w][0] for w in sc.which]) if sc.nitems else np.zeros((0, 6), np.float32)
    return lo_hi.astype(np.float32), np.array([per_mesh[w][1] for w in sc.which], np.uint32)


def mvps(sc):
    proj, view = camera()
    return R.mvps_of(proj, view, sc.models)


_COVER = {}


def cover_scene():
    h = P.scene("hidden")
    return P.kept_scene(h, [i == 2 for i in range(h.nitems)])


def cover_depth(oracle):
    """the depth of the cover of `hidden` drawn alone into a cleared frame (float32 [W * H])"""
    if "d" not in _COVER:
        _COVER["d"] = np.array(D.oracle_list_loop(oracle, cover_scene(), "DEPTH")[0].depth, np.float32)
    return _COVER["d"]


def far_scene():
    """(scene, proj, view, view_pos): the unit patch a million units along x, seen by the demo camera moved as far: the item's
    mvp = (proj * view) * model is composed under cancellation (w is the difference of two products near 1e6), so the error
    bound E decides what the test can say"""
    import f_renderer_amd as fr
    from f_renderer_amd import scenes
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    off = np.array([1.0e6, 0.0, 0.0])
    eye2 = tuple(np.array(eye) + off)
    view = np.asarray(fr.set_look_at(eye2, tuple(np.array(at) + off), up), np.float32).reshape(16)
    proj = np.asarray(fr.set_perspective(fovy, aspect, zn, zf), np.float32).reshape(16)
    models = np.stack([S._col_major(S.translate(*off)), S._col_major(S.translate(*(off + np.array(P._along_view(1.0)))) @ S.scale(0.3))])
    return D.Scene([D.Mesh(S.patch(60))], [0, 0], models, "PHONG", "PHONG"), proj, view, eye2


def far_translation():
    """(mvps [2, 16], lo_hi, flags) of far_scene()"""
    sc, proj, view, _ = far_scene()
    lo_hi, flags = bounds(sc)
    return R.mvps_of(proj, view, sc.models), lo_hi, flags


def special_depths(oracle):
    """name -> depth array: the cover's depth with NaN, -0.0 and +-inf entries"""
    d0 = cover_depth(oracle)
    out = {}
    for name, v in (("nan", np.nan), ("neg0", -0.0), ("inf", np.inf), ("ninf", -np.inf)):
        d = d0.copy()
        d[(np.arange(d.size) * 7919) % 13 == 0] = np.float32(v)
        out[name] = d
    out["all_inf"] = np.full(d0.size, np.inf, np.float32)
    out["all_nan"] = np.full(d0.size, np.nan, np.float32)
    return out
