"""Small draw lists -- (mesh, model matrix) items -- for tests/test_drawlist_cpu.py and tests/test_gpu_drawlist.py, and their
frames on the CPU oracle.  frr_draw_list(list) is by definition the reference's setup loop over objects that do not share a
mesh (phong.rs:319-359): one draw of mesh_i under `vs_uniform.model = model_i` per item, triangle ids running on; that loop,
through oracle.Frame.draw(..., tri_id_base=running, keep_setup=True), is the expected frame.  Each oracle frame is computed
once per process and shared (never modified).

The frame is that of tests/instanced_scenes.py, 128 x 96: three tile rows, so both ranks of a world-2 partition own rows."""
import numpy as np

from . import cull_scenes as CS
from . import indexed_scenes as I
from . import instanced_scenes as S

W, H, CLEAR = S.W, S.H, S.CLEAR
SIZES = [5, 100, 255, 256, 257, 513, 1]      # item sizes around the 256-input geometry block and the 64-lane wave
EMPTIES = [0, 7, 0, 0, 300, 0]               # empty items first, in a row and last


class Mesh:
    """tris: the expanded mesh [n, 3, NF]; indexed: (vertices, faces) of the same mesh, or None"""

    def __init__(self, tris, indexed=None):
        self.tris, self.indexed = np.ascontiguousarray(tris, np.float32), indexed
        self.ntris = self.tris.shape[0]


class Scene:
    """meshes: the distinct meshes; items: one (index into meshes, model [16]) per item, in list order"""

    def __init__(self, meshes, which, models, vs, ps, nf=8):
        self.meshes, self.which, self.vs, self.ps = meshes, [int(w) for w in which], vs, ps
        self.models = np.ascontiguousarray(models, np.float32).reshape(-1, 16)
        assert len(self.which) == self.models.shape[0]
        self.lit = vs in ("PHONG", "GOURAUD")
        self.nitems = len(self.which)
        self.ntris = [meshes[w].ntris for w in self.which]
        self.nf = nf

    def item_tris(self, i):
        return self.meshes[self.which[i]].tris


def spiky(n):
    """patch(n) with a corner of its first and of its last triangle pulled far outside the side planes: the first and the last
    input of the item are clipped into fans"""
    t = S.patch(n).copy()
    t[0, 0, 0] += 9.0
    t[-1, 2, 0] -= 9.0
    return t


def empty(nf=8):
    return Mesh(np.zeros((0, 3, nf), np.float32))


def _sized(sizes):
    meshes = [Mesh(S.patch(n)) if n else empty() for n in sizes]
    return Scene(meshes, range(len(sizes)), S.grid_models(len(sizes)), "PHONG", "PHONG")


def place_textures():
    """three textures that differ everywhere (slots 0..2: BODY, FACE, HAIR of phong.rs:41-47)"""
    from f_renderer_amd import scenes
    a = scenes.checker_texture(64, 8)
    b, c = a.copy(), a.copy()
    b[..., 0], c[..., 1] = 255 - a[..., 0], 255 - a[..., 1]
    return [a, np.ascontiguousarray(b), np.ascontiguousarray(c)]


BOUNDARY = ["sizes", "sizes_rev", "many", "empties"]
NAMES = BOUNDARY + ["one", "none", "all_empty", "clipped", "mix", "same_mesh", "tie", "clip_vs", "clip_color", "gouraud", "mirrored", "place"]
_SCENES = {}


def scene(name):
    if name in _SCENES:
        return _SCENES[name]
    from f_renderer_amd import scenes
    if name == "sizes":
        sc = _sized(SIZES)
    elif name == "sizes_rev":
        sc = _sized(SIZES[::-1])
    elif name == "many":
        # 300 items of 1..3 triangles from three meshes: the item changes inside every wave
        rng = np.random.default_rng(20260712)
        sc = Scene([Mesh(S.patch(1)), Mesh(S.patch(2)), Mesh(S.patch(3))], rng.integers(0, 3, 300), S.grid_models(300), "PHONG", "PHONG")
    elif name == "empties":
        sc = _sized(EMPTIES)
    elif name == "one":
        sc = Scene([Mesh(S.patch(40))], [0], S.clipped_models()[1:2], "PHONG", "PHONG")
    elif name == "none":
        sc = Scene([], [], np.zeros((0, 16), np.float32), "PHONG", "PHONG")
    elif name == "all_empty":
        sc = Scene([empty()], [0, 0, 0], S.grid_models(3), "PHONG", "PHONG")
    elif name == "clipped":
        # through the near plane, through a side plane, wholly off-screen, in view; and an item whose first and last inputs
        # are clipped (spiky), in front
        cm = S.clipped_models()
        sc = Scene([Mesh(S.patch(128)), Mesh(S.patch(70)), Mesh(spiky(30))], [0, 1, 0, 1, 0, 2, 1], np.concatenate([cm, cm[:1]])[[0, 1, 2, 3, 4, 6, 5]],
                   "PHONG", "PHONG")
    elif name == "mix":
        # plain + indexed + (on the GPU) a device-bound mesh + a device-bound indexed mesh: four distinct meshes
        v, f = S.patch_grid(8, 8)
        v2, f2 = S.patch_grid(5, 9)
        cm = S.clipped_models()
        sc = Scene([Mesh(S.patch(100)), Mesh(v[f.astype(np.int64)], (v, f)), Mesh(S.patch(77)), Mesh(v2[f2.astype(np.int64)], (v2, f2))],
                   [0, 1, 2, 3, 1], cm[[0, 1, 5, 3, 2]], "PHONG", "PHONG")
    elif name == "same_mesh":
        sc = Scene([Mesh(S.patch(100))], [0] * 7, S.grid_models(7), "PHONG", "PHONG")
    elif name == "tie":
        m = S.grid_models(1)[0]
        sc = Scene([Mesh(S.patch(60))], [0, 0], np.stack([m, m]), "PHONG", "DEPTH")
    elif name == "clip_vs":
        # a vertex shader that reads no matrix; two different meshes, the second clipped
        v, f = I.grid_clip(8, 8)
        v2, f2 = I.grid_clip(6, 6, clipped=True)
        sc = Scene([Mesh(I.expand(v, f)), Mesh(I.expand(v2, f2), (v2, f2))], [0, 1, 0], S.grid_models(3), "CLIP", "DEPTH", nf=4)
    elif name == "clip_color":
        v, f = I.grid_clip(6, 6, clipped=True)
        v2, f2 = I.grid_clip(9, 4)
        sc = Scene([Mesh(I.expand(I.with_colors(v), f)), Mesh(I.expand(I.with_colors(v2, 11), f2))], [1, 0], S.grid_models(2), "CLIP_COLOR", "COLOR", nf=7)
    elif name == "gouraud":
        sc = Scene([Mesh(scenes.torus(10, 6, R=0.3, r=0.12)), Mesh(scenes.torus(7, 5, R=0.25, r=0.1))], [0, 1, 1, 0], S.grid_models(4), "GOURAUD", "COLOR")
    elif name == "mirrored":
        # a closed mesh twice: as it is on the left, mirrored (a model matrix of negative determinant) on the right
        t = scenes.torus(10, 6, R=0.3, r=0.12)
        sc = Scene([Mesh(t), Mesh(scenes.torus(8, 6, R=0.4, r=0.2))], [0, 1, 0], np.stack([CS.left_model(), S.grid_models(1)[0], CS.mirrored_model()]), "GOURAUD", "COLOR")
    elif name == "place":
        # three meshes (body, face, hair of phong.rs:321-359); the first input of item 1 is clipped into a fan and its first
        # fan triangle -- emission index first[1], which the reference's `<=` shades with item 0's texture -- owns pixels
        cm = S.clipped_models()
        sc = Scene([Mesh(S.patch(60)), Mesh(spiky(40)), Mesh(S.patch(50))], [0, 1, 2], cm[[0, 1, 5]], "PHONG", "DEPTH")
    else:
        raise KeyError(name)
    _SCENES[name] = sc
    return sc


def uniform_kw(oracle, sc, ps):
    kw = S.camera_kw(oracle) if sc.lit else {}
    if ps in ("PHONG", "BLINN"):
        kw["tex"] = oracle.Texture(S.texture())
    return kw


def oracle_list_loop(oracle, sc, ps=None, frame=None, window=None, keep=None, tri_id_base=None, kw=None):
    """The loop over items on the oracle: one draw of mesh_i under model_i per item into `frame` (default: a cleared one), ids
    running on from tri_id_base (default: behind what the frame holds).  keep: per item a bool mask of the inputs that are drawn (a culled pass), or None.
    kw: the uniform keywords of the pass other than `model` (default: the demo camera and the scenes' texture).
    Returns (frame, setup list, triangles emitted per item)."""
    ps = ps or sc.ps
    kw = uniform_kw(oracle, sc, ps) if kw is None else kw
    if frame is None:
        frame = oracle.Frame(W, H)
        frame.clear(*CLEAR)
    setups, per_item = [], []
    base = int(frame.counters.tris_setup) if tri_id_base is None else tri_id_base
    for i in range(sc.nitems):
        before = int(frame.counters.tris_setup)
        tris = sc.item_tris(i)
        if keep is not None:
            tris = np.ascontiguousarray(tris[keep[i]])
        if tris.shape[0]:
            setups.append(frame.draw(tris, getattr(oracle, "VS_" + sc.vs), getattr(oracle, "PS_" + ps),
                                     oracle.make_uniforms(model=sc.models[i], **kw), window=window,
                                     tri_id_base=base + sum(per_item), keep_setup=True))
        per_item.append(int(frame.counters.tris_setup) - before)
    setup = np.concatenate(setups) if setups else np.zeros((0, 3), oracle.VERTEX_DTYPE)
    return frame, setup, per_item


_FRAMES = {}


def oracle_frame(oracle, name, ps=None):
    """(Frame, setup list, triangles emitted per item) of the named list drawn into a cleared frame"""
    key = (name, ps)
    if key not in _FRAMES:
        _FRAMES[key] = oracle_list_loop(oracle, scene(name), ps)
    return _FRAMES[key]


def cull_keep(sc, mode):
    """per item: the inputs the cull mode keeps under that item's matrices (tests/cull_scenes.py: the f32 determinant)"""
    out = []
    for i in range(sc.nitems):
        c = CS.Scene(sc.item_tris(i), sc.vs, sc.ps, sc.models[i])
        out.append(CS.keep_mask(c, mode) if c.ntris else np.zeros(0, bool))
    return out
