"""Small indexed meshes (vertices [V, NF] f32, faces [F, 3] u32) for tests/test_gpu_indexed.py, and their frames on the CPU
oracle.  An indexed draw is the draw of `vertices[faces]`, which the oracle renders as it renders every expanded mesh; each
oracle frame is computed once per process and shared (never modified)."""
import math

import numpy as np

W, H = 256, 192
CLEAR = ((30, 30, 30, 255), 0.0)


def grid_faces(nx, ny):
    """two triangles per cell of an (nx+1) x (ny+1) vertex grid, row-major vertex numbers"""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).reshape(-1)
    b, c, d = a + (ny + 1), a + (ny + 1) + 1, a + 1
    return np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.uint32)


def grid_clip(nx=16, ny=16, clipped=False):
    """A folded sheet in clip space (VS_CLIP): the two halves overlap on screen at different w, so the depth test decides.
    clipped: 1.5 x larger than the screen and dipping behind the near plane along one edge -- inputs straddle the side planes
    and the near plane and become fans."""
    s, t = np.meshgrid(np.arange(nx + 1) / nx, np.arange(ny + 1) / ny, indexing="ij")
    x = 0.9 * (1.0 - 2.0 * np.abs(2.0 * s - 1.0))
    y = -0.85 + 1.6 * t + 0.1 * s
    w = 1.0 + 2.0 * s + 0.5 * t
    z = 0.5 * np.ones_like(s)
    if clipped:
        x, y = 1.5 * x, 1.5 * y
        z = t - 0.15
    v = np.stack([x * w, y * w, z * w, w], axis=2).reshape(-1, 4)
    return v.astype(np.float32), grid_faces(nx, ny)


def strip(n):
    """the first n triangles of a 32-wide grid (n = 1, 255, 256, 257, 513: around the 256-triangle geometry block)"""
    ny = max(1, (n + 63) // 64)
    v, f = grid_clip(32, ny)
    return v, np.ascontiguousarray(f[:n])


def fan(n=40):
    """one vertex in every triangle"""
    ang = [2.0 * math.pi * k / n for k in range(n + 1)]
    ring = [[0.8 * math.cos(a), 0.8 * math.sin(a), 0.5, 1.0] for a in ang]
    wv = np.array([1.0] + [1.0 + 0.5 * (k % 5) for k in range(n + 1)])
    v = np.array([[0.05, -0.1, 0.5, 1.0]] + ring) * wv[:, None]
    f = np.array([[0, k + 1, k + 2] for k in range(n)], np.uint32)
    return v.astype(np.float32), f


def degenerate():
    """a grid with one triangle whose three corners are the same vertex, in the middle of the list"""
    v, f = grid_clip(8, 8)
    return v, np.ascontiguousarray(np.insert(f, 60, [40, 40, 40], axis=0).astype(np.uint32))


def one_vertex():
    return np.array([[0.1, 0.2, 0.5, 1.0]], np.float32), np.zeros((3, 3), np.uint32)


def poisoned(v, f):
    """the same mesh with unreferenced vertices of NaN and +-inf in front of, inside and behind the vertex array"""
    nf = v.shape[1]
    bad = np.array([[np.nan] * nf, [np.inf] * nf, [-np.inf] * nf], np.float32)
    mid = v.shape[0] // 2
    vv = np.concatenate([bad, v[:mid], bad[::-1], v[mid:], bad[[1, 0, 2]]]).astype(np.float32)
    ff = np.where(f < mid, f + 3, f + 6).astype(np.uint32)
    return vv, ff


def index_mesh(tris):
    """an expanded mesh [n, 3, NF] as (vertices, faces): one record per distinct vertex bit pattern"""
    nf = tris.shape[2]
    flat = np.ascontiguousarray(tris, np.float32).reshape(-1, nf).view(np.uint32)
    u, inv = np.unique(flat, axis=0, return_inverse=True)
    return np.ascontiguousarray(u).view(np.float32), np.ascontiguousarray(inv.reshape(-1, 3).astype(np.uint32))


def with_colors(v, seed=7):
    from f_renderer_amd import scenes
    col = scenes.splitmix_u01(seed, v.shape[0] * 3).reshape(-1, 3).astype(np.float32)
    return np.concatenate([v, col], axis=1).astype(np.float32)


def expand(v, f):
    return np.ascontiguousarray(v[f.astype(np.int64)])          # [F, 3, NF]


def camera_kw(mod):
    """uniform keywords of the demo camera for `mod` = f_renderer_amd or the oracle binding"""
    from f_renderer_amd import scenes
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    return dict(view=mod.set_look_at(eye, at, up), proj=mod.set_perspective(fovy, aspect, zn, zf), view_pos=eye)


def texture():
    from f_renderer_amd import scenes
    return scenes.checker_texture(64, 8)


_SCENES = {}


def scene(name):
    """(vertices, faces, vs name, ps name, lit) of the named scene"""
    if name in _SCENES:
        return _SCENES[name]
    from f_renderer_amd import scenes
    if name.startswith("strip"):
        v, f = strip(int(name[5:]))
        sc = (v, f, "CLIP", "DEPTH", False)
    elif name == "grid":
        sc = grid_clip() + ("CLIP", "DEPTH", False)
    elif name == "fan":
        sc = fan() + ("CLIP", "DEPTH", False)
    elif name == "degenerate":
        sc = degenerate() + ("CLIP", "DEPTH", False)
    elif name == "one_vertex":
        sc = one_vertex() + ("CLIP", "DEPTH", False)
    elif name == "poisoned":
        sc = poisoned(*grid_clip()) + ("CLIP", "DEPTH", False)
    elif name == "clipped":
        sc = grid_clip(clipped=True) + ("CLIP", "DEPTH", False)
    elif name in ("color", "color_clipped"):
        v, f = grid_clip(clipped=name == "color_clipped")
        sc = (with_colors(v), f, "CLIP_COLOR", "COLOR", False)
    elif name == "phong":
        sc = index_mesh(scenes.displaced_sphere(n=24)) + ("PHONG", "PHONG", True)
    elif name == "gouraud":
        sc = index_mesh(scenes.torus(20, 14)) + ("GOURAUD", "COLOR", True)
    else:
        raise KeyError(name)
    _SCENES[name] = sc
    return sc


_FRAMES = {}


def oracle_frame(oracle, name, window=None):
    """(Frame, setup list) of ONE draw of the scene's expanded mesh into a cleared frame"""
    key = (name, window)
    if key not in _FRAMES:
        v, f, vs, ps, lit = scene(name)
        kw = camera_kw(oracle) if lit else {}
        if ps == "PHONG":
            kw["tex"] = oracle.Texture(texture())
        fr = oracle.Frame(W, H)
        fr.clear(*CLEAR)
        setup = fr.draw(expand(v, f), getattr(oracle, "VS_" + vs), getattr(oracle, "PS_" + ps), oracle.make_uniforms(**kw),
                        window=window, keep_setup=True) if f.shape[0] else np.zeros((0, 3), oracle.VERTEX_DTYPE)
        _FRAMES[key] = (fr, setup)
    return _FRAMES[key]
