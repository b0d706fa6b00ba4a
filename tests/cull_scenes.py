"""Scenes for the face-culling tests (tests/test_cull_cpu.py, tests/test_gpu_cull.py) and their NumPy side.

A geometry pass under a cull mode (frr_set_cull) is BY DEFINITION the plain pass over the sub-mesh of the inputs the mode
keeps, in their original order.  So the expected frame of a culled draw is the oracle's frame of `mesh[keep]`, where `keep`
comes from the sign of the determinant of the three clip positions the vertex shader returns -- oracle_np.vertex_shader
for the positions, and det_f32 below for the determinant: a NumPy float32 restatement of the formula of include/frr.h,
written independently of the C source.  Each oracle frame is computed once per process and shared (never modified).

The frame is 96 x 70: three tile rows and three tile columns."""
import numpy as np

from oracle import oracle_np as onp

W, H = 96, 70
CLEAR = ((30, 30, 30, 255), 0.0)
NONE, NEG, POS = 0, 1, 2
F = np.float32


# ---- the rule ----------------------------------------------------------------------------------------------------------

def det_f32(clip):
    """d = (x0*(y1*w2 - y2*w1) - x1*(y0*w2 - y2*w0)) + x2*(y0*w1 - y1*w0) in float32, one rounding per operation, for clip
    positions [..., 3, 4] (x, y, z, w)"""
    c = np.asarray(clip, F)
    x0, y0, w0 = c[..., 0, 0], c[..., 0, 1], c[..., 0, 3]
    x1, y1, w1 = c[..., 1, 0], c[..., 1, 1], c[..., 1, 3]
    x2, y2, w2 = c[..., 2, 0], c[..., 2, 1], c[..., 2, 3]
    with np.errstate(all="ignore"):
        a = (x0 * ((y1 * w2).astype(F) - (y2 * w1).astype(F)).astype(F)).astype(F)
        b = (x1 * ((y0 * w2).astype(F) - (y2 * w0).astype(F)).astype(F)).astype(F)
        e = (x2 * ((y0 * w1).astype(F) - (y1 * w0).astype(F)).astype(F)).astype(F)
        return ((a - b).astype(F) + e).astype(F)


def keeps(d, mode):
    """which inputs with determinants d a mode keeps: d == 0 and NaN are never dropped"""
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore"):
        if mode == NEG:
            return ~(d < 0)
        if mode == POS:
            return ~(d > 0)
    return np.ones(d.shape, bool)


def exact_sign(clip):
    """the sign of the same determinant over the rationals, for ONE triple [3, 4] of finite floats"""
    from fractions import Fraction
    (x0, y0, _, w0), (x1, y1, _, w1), (x2, y2, _, w2) = [[Fraction(float(v)) for v in p] for p in np.asarray(clip, F)]
    d = x0 * (y1 * w2 - y2 * w1) - x1 * (y0 * w2 - y2 * w0) + x2 * (y0 * w1 - y1 * w0)
    return (d > 0) - (d < 0)


def near_collinear(n=4096, seed=20260611):
    """n triples whose third point lies within float32 rounding of the line through the other two:
    p2 = p0 + s (p1 - p0) + N(0, 3e-8) in NDC, w in [0.5, 2], as clip positions [n, 3, 4] (z = w / 2: inside the frustum)"""
    rng = np.random.default_rng(seed)
    p0, p1 = rng.uniform(-0.9, 0.9, (n, 2)), rng.uniform(-0.9, 0.9, (n, 2))
    s = rng.uniform(0.05, 0.95, (n, 1))
    p2 = p0 + s * (p1 - p0) + rng.normal(0.0, 3e-8, (n, 2))
    w = rng.uniform(0.5, 2.0, (n, 3))
    out = np.empty((n, 3, 4), np.float64)
    for k, p in enumerate((p0, p1, p2)):
        out[:, k, 0], out[:, k, 1], out[:, k, 2], out[:, k, 3] = p[:, 0] * w[:, k], p[:, 1] * w[:, k], 0.5 * w[:, k], w[:, k]
    return np.ascontiguousarray(out.astype(F))


HAND_CASES = {
    "ccw": [[0, 0, 0.5, 1], [1, 0, 0.5, 1], [0, 1, 0.5, 1]],
    "cw": [[0, 0, 0.5, 1], [0, 1, 0.5, 1], [1, 0, 0.5, 1]],
    "ccw_one_w_negative": [[0.25, 0.5, 0.5, 1], [1, 0.125, 0.5, -1], [0.5, 1, 0.5, 1]],
    "cw_one_w_negative": [[0.25, 0.5, 0.5, 1], [0.5, 1, 0.5, 1], [1, 0.125, 0.5, -1]],
    "repeated_vertex": [[0.3, 0.7, 0.5, 1.5], [0.3, 0.7, 0.5, 1.5], [-0.2, 0.1, 0.5, 1]],
    "nan": [[0, 0, 0.5, 1], [np.nan, 0, 0.5, 1], [0, 1, 0.5, 1]],
    "inf_minus_inf": [[3e38, 3e38, 0.5, 3e38], [3e38, 2e38, 0.5, 3e38], [2e38, 3e38, 0.5, 2e38]],
}


# ---- scenes ------------------------------------------------------------------------------------------------------------

def camera_kw(mod):
    """uniform keywords of the demo camera for `mod` = f_renderer_amd or an oracle binding"""
    from f_renderer_amd import scenes
    eye, at, up, fovy, aspect, zn, zf = scenes.demo_camera(W, H)
    return dict(view=mod.set_look_at(eye, at, up), proj=mod.set_perspective(fovy, aspect, zn, zf), view_pos=eye)


def texture():
    from f_renderer_amd import scenes
    return scenes.checker_texture(64, 8)


class Scene:
    """tris: the expanded mesh [n, 3, NF]; vs / ps: shader names; model: the model matrix ([16], column-major) or None"""

    def __init__(self, tris, vs, ps, model=None):
        self.tris, self.vs, self.ps = np.ascontiguousarray(tris, F), vs, ps
        self.model = None if model is None else np.ascontiguousarray(model, F).reshape(16)
        self.lit = vs in ("PHONG", "GOURAUD")
        self.ntris = self.tris.shape[0]
        self._det = None

    def with_model(self, model):
        return Scene(self.tris, self.vs, self.ps, model)

    def clip(self):
        """[n, 3, 4]: what the vertex shader returns for every corner"""
        u = onp.Uniforms(model=self.model, **(camera_kw(onp) if self.lit else {}))
        vs = getattr(onp, "VS_" + self.vs)
        return np.array([[onp.vertex_shader(vs, u, v)[0] for v in tri] for tri in self.tris], F).reshape(-1, 3, 4)

    def det(self):
        if self._det is None:
            self._det = det_f32(self.clip())
        return self._det


def keep_mask(sc, mode):
    return keeps(sc.det(), mode)


def flipped(tris, cull):
    """`tris` (a VS_CLIP / VS_CLIP_COLOR mesh) with two vertices swapped wherever needed so that exactly the inputs of the
    bool pattern `cull` have d < 0 (those FRR_CULL_NEG drops) and the others d > 0"""
    t = np.array(tris, F)
    swap = (det_f32(t[..., :4]) < 0) != np.asarray(cull, bool)
    t[swap] = t[swap][:, [0, 2, 1]]
    d = det_f32(t[..., :4])
    assert ((d < 0) == cull).all() and (d != 0).all()
    return t


SIZES = [255, 256, 257, 513]      # around the 256-input geometry block, and a third block
PATTERNS = ["alternate", "lanes_0_63", "wave", "block", "last_kept", "all"]


def pattern(name, n):
    """bool[n]: the inputs the pattern culls"""
    i = np.arange(n)
    if name == "alternate":
        return i % 2 == 1
    if name == "lanes_0_63":
        return (i % 64 == 0) | (i % 64 == 63)
    if name == "wave":
        return (i >= 64) & (i < 128) if n < 513 else (i >= 320) & (i < 384)
    if name == "block":                        # a whole 256-input block: its block sum is 0 (n <= 256: that is everything)
        return (i >= 256) & (i < 512) if n >= 513 else i < 256
    if name == "last_kept":
        return i < n - 1
    if name == "all":
        return np.ones(n, bool)
    raise KeyError(name)


def pattern_cases():
    return [(p, n) for p in PATTERNS for n in SIZES if not (p == "block" and n <= 256)]


def left_model():
    """column-major [16]: the mesh moved to the left half of the view"""
    m = np.eye(4)
    m[:3, 3] = (-0.8, 0.1, 0.0)
    return np.ascontiguousarray(m.T.reshape(16).astype(F))


def mirrored_model():
    """a model matrix of negative determinant: the mesh mirrored in x, in the right half of the view"""
    m = np.diag([-1.0, 1.0, 1.0, 1.0])
    m[:3, 3] = (0.8, -0.1, 0.2)
    return np.ascontiguousarray(m.T.reshape(16).astype(F))


MAIN = ["torus", "sphere"]
ADMITTED = ["torus", "sphere", "clipped", "small_torus_left", "small_torus_mirrored"]   # (scene, NEG) and (scene, POS) are both used
_SCENES = {}


def scene(name):
    if name in _SCENES:
        return _SCENES[name]
    from f_renderer_amd import scenes
    from . import indexed_scenes as I
    if name == "torus":
        sc = Scene(scenes.torus(12, 10), "GOURAUD", "COLOR")
    elif name == "sphere":
        sc = Scene(scenes.displaced_sphere(16), "PHONG", "PHONG")
    elif name == "small_torus":
        sc = Scene(scenes.torus(10, 6, R=0.55, r=0.22), "GOURAUD", "COLOR")
    elif name == "small_torus_left":
        sc = scene("small_torus").with_model(left_model())
    elif name == "small_torus_mirrored":
        sc = scene("small_torus").with_model(mirrored_model())
    elif name == "clipped":
        # a sheet larger than the screen that dips behind the near plane: inputs through the side planes and the near
        # plane become fans.  Culled and kept inputs interleave in runs of three.
        v, f = I.grid_clip(16, 16, clipped=True)
        t = I.expand(I.with_colors(v), f)
        sc = Scene(flipped(t, (np.arange(t.shape[0]) // 3) % 2 == 0), "CLIP_COLOR", "COLOR")
    elif name.startswith("pat_"):
        p, n = name[4:name.rindex("_")], int(name[name.rindex("_") + 1:])      # "pat_<pattern>_<inputs>"
        v, f = I.strip(n)
        sc = Scene(flipped(I.expand(I.with_colors(v), f), pattern(p, n)), "CLIP_COLOR", "COLOR")
    elif name == "collinear":
        sc = Scene(near_collinear(), "CLIP", "DEPTH")
    else:
        raise KeyError(name)
    _SCENES[name] = sc
    return sc


# ---- the oracle's side -------------------------------------------------------------------------------------------------

def uniforms(oracle, sc, ps=None):
    kw = camera_kw(oracle) if sc.lit else {}
    if (ps or sc.ps) in ("PHONG", "BLINN"):
        kw["tex"] = oracle.Texture(texture())
    return oracle.make_uniforms(model=sc.model, **kw)


def oracle_draw(oracle, frame, sc, mode, ps=None, window=None):
    """one culled draw of the scene into `frame`, ids running on behind what the frame holds: cref.Frame.draw of mesh[keep].
    Returns the setup list."""
    sub = np.ascontiguousarray(sc.tris[keep_mask(sc, mode)])
    if not sub.shape[0]:
        return np.zeros((0, 3), oracle.VERTEX_DTYPE)
    return frame.draw(sub, getattr(oracle, "VS_" + sc.vs), getattr(oracle, "PS_" + (ps or sc.ps)), uniforms(oracle, sc, ps),
                      window=window, tri_id_base=int(frame.counters.tris_setup), keep_setup=True)


_FRAMES = {}


def oracle_frame(oracle, name, mode, ps=None):
    """(Frame, setup list) of ONE culled draw of the named scene into a cleared frame"""
    key = (name, mode, ps)
    if key not in _FRAMES:
        f = oracle.Frame(W, H)
        f.clear(*CLEAR)
        _FRAMES[key] = (f, oracle_draw(oracle, f, scene(name), mode, ps))
    return _FRAMES[key]
