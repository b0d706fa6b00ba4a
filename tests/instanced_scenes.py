"""Small instanced scenes -- one mesh, a table of model matrices -- for tests/test_instanced_cpu.py and
tests/test_gpu_instanced.py, and their frames on the CPU oracle.  frr_draw_instanced(mesh, models) is by definition the
reference's loop over objects (phong.rs:319-331): one draw of the mesh per matrix, `vs_uniform.model = models[i]`, triangle
ids running on; that loop, through oracle.Frame.draw(..., tri_id_base=...), is the expected frame.  Each oracle frame is
computed once per process and shared (never modified).

The frame is 128 x 96: three tile rows, so both ranks of a world-2 partition own rows."""
import math

import numpy as np

W, H = 128, 96
CLEAR = ((30, 30, 30, 255), 0.0)
# (triangles of the mesh, instances): around the 256-triangle geometry block and the 64-lane wave -- several instances inside
# one wave, blocks whose instance changes at lanes that are no wave starts, a block with more than 128 instances, a mesh over
# one, two and three blocks
BOUNDARY = [(5, 3), (100, 7), (255, 2), (256, 2), (257, 2), (513, 2), (1, 300), (12, 64)]


# ---- matrices (column-major [16], like frr_uniforms.model) -------------------------------------------------------------

def _col_major(m):
    return np.ascontiguousarray(np.asarray(m, np.float64).T.reshape(16).astype(np.float32))


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1.0]])


def scale(s):
    return np.diag([s, s, s, 1.0])


def grid_models(k):
    """k translations on a grid across the view, each with its own rotation and a scale that keeps the copies apart"""
    cols = max(1, int(math.ceil(math.sqrt(k * 4.0 / 3.0))))
    rows = (k + cols - 1) // cols
    s = min(1.0, 2.4 / cols)
    out = []
    for i in range(k):
        gx, gy = i % cols, i // cols
        t = translate((gx + 0.5) / cols * 3.0 - 1.5, (gy + 0.5) / rows * 2.0 - 1.0, -0.3 * (i % 3))
        out.append(_col_major(t @ rot_y(0.2 * i) @ rot_x(0.1 * (i % 5)) @ scale(s)))
    return np.stack(out) if out else np.zeros((0, 16), np.float32)


def clipped_models():
    """Around the demo camera (eye (0, 1, 3) looking at the origin): two copies in view, a small one edge on through the near
    plane, one through a side plane, one wholly off-screen (the reference still sets its triangles up), one rotated and
    scaled behind the others."""
    return np.stack([
        _col_major(translate(-0.6, 0.1, 0.0) @ rot_y(0.3)),
        _col_major(translate(0.5, -0.2, -0.4) @ rot_x(-0.4) @ scale(1.3)),
        _col_major(translate(0.1, 0.99, 2.86) @ rot_x(-1.3) @ scale(0.2)),   # 0.14 in front of the eye, edge on: straddles z_near = 0.1
        _col_major(translate(1.7, 0.0, 0.2) @ scale(1.5)),             # through a side plane
        _col_major(translate(60.0, 0.0, 0.0)),                         # wholly off-screen
        _col_major(translate(-0.2, 0.3, -0.8) @ rot_y(-0.7) @ scale(2.0)),
    ])


# ---- meshes ------------------------------------------------------------------------------------------------------------

def patch_grid(nx, ny):
    """A bumped sheet of 0.7 x 0.6 object units (pos3, uv2, normal3 per vertex: the VS_PHONG / VS_GOURAUD layout) as
    (vertices [(nx+1)(ny+1), 8], faces [2 nx ny, 3])"""
    from .indexed_scenes import grid_faces
    s, t = np.meshgrid(np.arange(nx + 1) / nx, np.arange(ny + 1) / ny, indexing="ij")
    x, y = 0.7 * (s - 0.5), 0.6 * (t - 0.5)
    z = 0.12 * np.sin(5.0 * x) * np.cos(4.0 * y)
    dzdx = 0.6 * np.cos(5.0 * x) * np.cos(4.0 * y)
    dzdy = -0.48 * np.sin(5.0 * x) * np.sin(4.0 * y)
    n = np.stack([-dzdx, -dzdy, np.ones_like(x)], axis=2)
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    v = np.concatenate([np.stack([x, y, z], 2), np.stack([s, t], 2), n], axis=2).reshape(-1, 8)
    return v.astype(np.float32), grid_faces(nx, ny)


def patch(n):
    """the first n triangles of such a sheet, expanded: [n, 3, 8]"""
    cells = max(1, (n + 1) // 2)
    nx = min(cells, 16)
    ny = (cells + nx - 1) // nx
    v, f = patch_grid(nx, ny)
    return np.ascontiguousarray(v[f.astype(np.int64)][:n])


def texture():
    from f_renderer_amd import scenes
    return scenes.checker_texture(64, 8)


def camera_kw(mod):
    """uniform keywords of the demo camera for `mod` = f_renderer_amd or the oracle binding"""
    from f_renderer_amd import scenes
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    return dict(view=mod.set_look_at(eye, at, up), proj=mod.set_perspective(fovy, aspect, zn, zf), view_pos=eye)


# ---- scenes ------------------------------------------------------------------------------------------------------------

class Scene:
    """tris: the expanded mesh [n, 3, NF]; indexed: (vertices, faces) of the same mesh, or None; models [ninst, 16]"""

    def __init__(self, tris, vs, ps, models, indexed=None):
        self.tris, self.vs, self.ps, self.models, self.indexed = np.ascontiguousarray(tris, np.float32), vs, ps, np.ascontiguousarray(models, np.float32).reshape(-1, 16), indexed
        self.lit = vs in ("PHONG", "GOURAUD")
        self.ntris, self.ninst = self.tris.shape[0], self.models.shape[0]


NAMES = ["b%dx%d" % p for p in BOUNDARY] + ["clipped", "tie_clip", "tie_phong", "gouraud", "clip_color", "indexed",
                                            "none", "one", "empty_mesh"]
_SCENES = {}


def scene(name):
    if name in _SCENES:
        return _SCENES[name]
    from f_renderer_amd import scenes
    from . import indexed_scenes as I
    if name[0] == "b" and "x" in name:
        n, k = (int(x) for x in name[1:].split("x"))
        sc = Scene(patch(n), "PHONG", "PHONG", grid_models(k))
    elif name == "clipped":
        sc = Scene(patch(128), "PHONG", "PHONG", clipped_models())
    elif name == "tie_clip":
        # a vertex shader that reads no matrix: three identical copies, every fragment of a copy ties with the others'
        v, f = I.grid_clip(8, 8)
        sc = Scene(I.expand(v, f), "CLIP", "DEPTH", grid_models(3))
    elif name == "tie_phong":
        sc = Scene(patch(60), "PHONG", "DEPTH", np.stack([grid_models(1)[0]] * 3))
    elif name == "gouraud":
        sc = Scene(scenes.torus(10, 6, R=0.3, r=0.12), "GOURAUD", "COLOR", grid_models(4))
    elif name == "clip_color":
        v, f = I.grid_clip(6, 6, clipped=True)
        sc = Scene(I.expand(I.with_colors(v), f), "CLIP_COLOR", "COLOR", grid_models(3))
    elif name == "indexed":
        v, f = patch_grid(16, 16)                      # 17 x 17 vertices under 512 triangles
        sc = Scene(v[f.astype(np.int64)], "PHONG", "PHONG", clipped_models()[[0, 2, 5]], indexed=(v, f))
    elif name == "none":
        sc = Scene(patch(40), "PHONG", "PHONG", np.zeros((0, 16), np.float32))
    elif name == "one":
        sc = Scene(patch(40), "PHONG", "PHONG", clipped_models()[1:2])
    elif name == "empty_mesh":
        sc = Scene(np.zeros((0, 3, 8), np.float32), "PHONG", "PHONG", grid_models(4))
    else:
        raise KeyError(name)
    _SCENES[name] = sc
    return sc


def nonfinite_models():
    """one all-NaN and one all-zero matrix between finite ones"""
    m = clipped_models()[[0, 1, 5, 3]].copy()
    m[1] = np.nan
    m[2] = 0.0
    return m


_FRAMES = {}


def oracle_loop(oracle, sc, ps=None, frame=None, tri_id_base=0, window=None):
    """The loop over objects (phong.rs:319-331) on the oracle: one draw per matrix into `frame` (default: a cleared one),
    ids running on from tri_id_base.  Returns (frame, setup list, triangles emitted per instance)."""
    ps = ps or sc.ps
    kw = camera_kw(oracle) if sc.lit else {}
    if ps in ("PHONG", "BLINN"):
        kw["tex"] = oracle.Texture(texture())
    if frame is None:
        frame = oracle.Frame(W, H)
        frame.clear(*CLEAR)
    setups, per_inst = [], []
    for i in range(sc.ninst):
        before = int(frame.counters.tris_setup)
        if sc.ntris:
            setups.append(frame.draw(sc.tris, getattr(oracle, "VS_" + sc.vs), getattr(oracle, "PS_" + ps),
                                     oracle.make_uniforms(model=sc.models[i], **kw), window=window,
                                     tri_id_base=tri_id_base + sum(per_inst), keep_setup=True))
        per_inst.append(int(frame.counters.tris_setup) - before)
    setup = np.concatenate(setups) if setups else np.zeros((0, 3), oracle.VERTEX_DTYPE)
    return frame, setup, per_inst


def oracle_frame(oracle, name, ps=None):
    """(Frame, setup list, triangles emitted per instance) of the named scene drawn into a cleared frame"""
    key = (name, ps)
    if key not in _FRAMES:
        _FRAMES[key] = oracle_loop(oracle, scene(name), ps)
    return _FRAMES[key]
