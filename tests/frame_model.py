"""Random whole-frame command sequences and their CPU model, for tests/test_frame_model_cpu.py and
tests/test_gpu_frame_model.py.

generate(seed) yields three frames of commands the way a caller composes them: state setters (cull mode, uniforms, textures),
geometry passes of five kinds (plain, indexed, instanced, list, predicated list), each fused (draw*) or split into geometry*
... rasterization with up to three other commands in between, lines, wireframes, resolves, shades, per-item and per-triangle
counts, host queries, and a frame end that is a read-back or a fenced copy.  Model applies one step at a time to the two CPU
oracles and to NumPy copies of the caller's buffers; run_model(oracle, frames) returns what every frame must leave behind.
Nothing here is computed from the library.

What a step means is what include/frr.h says, built from the pieces the per-feature tests already hold the library to:
  a pass        drawlist_scenes.oracle_list_loop (an instanced pass is a list of one mesh, a plain pass a list of one item);
                per item the inputs the cull mode keeps (cull_scenes.det_f32 / keeps under the pass's matrices), none of a
                predicate-dropped item (predicate_scenes.kept_of over the keep buffer's contents AT THE GEOMETRY CALL)
  a split pass  recorded at geometry* (setup list, item ranges, tris_in / tris_setup / draws), drawn at rasterization: the
                commands in between see the frame without it and its setup list with it
  lines         lines_reference.draw_lines; a wireframe: the same over lines_reference.wireframe_segments of the setup spi
  counts        visible_scenes.want_counts over the frame's ids
  varyings      oracle_np.draw(..., debug=) of the pass over the frame as it was before the pass; its depth, ids and colour
                are asserted equal to the C oracle's every time
  shade         the C oracle's pixel shader and quantisation over the buffer's entries (oracle.cref.shade_pixels)

Work lists.  The tiny-list runs start with 64 bin records and 16 fan slots; finish() (f_renderer_amd/csrc/frr_api.hip) grows
a list that was too small to need + need / 4 + 1024 records, need + need / 8 + 1024 fan slots (need: eight times the fullest
of the eight regions the 256-input geometry blocks allocate in).  The model computes every pass's need (fan triangles per
block; setup triangles times 32-pixel tiles under their bounding boxes) and keeps an UPPER bound of what the growth rule can
have left behind.  A pass whose need is at least MARGIN times that bound is a rung: it must overflow, whatever rounding
exec_geometry applies.  Two meshes are made for that, r1 and r2; each seed meets r1 in an earlier frame than r2.

The extended sequences.  generate(seed, extended=True) for seed in XSEEDS adds three things, and leaves what generate(seed)
yields for SEEDS exactly as it was (tests/test_frame_model_cpu.py pins a digest):
  shade_items   {ps, buf, table}: frr_shade_items by its definition -- per item k of the latest pass the `shade` above over
                (id_first[k], id_count[k]) under the call's uniforms with MATERIALS[table][k]'s texture slot (the slot's texture
                as of the call), strengths and flat colour.  Undefined before any geometry pass and for a buffer whose K the
                shader refuses; nothing is written after a clear since the pass, for a pass that emitted nothing and for one
                that is not rastered yet, whose ids are not in the target
  a raster of a pass that is rastered already ("again"), in the frame's one window and with a shader of the same K:
                oracle_list_loop runs again over the frame as it is, with the same ids.  frag_covered and frag_nan add up
                again; draws, tris_in and tris_setup counted at the geometry call.  The pass's `before`, `after` and `ps` are
                those of the LATEST raster: a resolve sees the ownership the last raster left
  an abandoned pass ("abandoned"): a geometry* that no raster follows.  tris_in, draws and the emitted triangles advance, it
                owns no pixel, the next pass's ids start behind it, and with the tiny lists a rung still overflows
They are generated against Model(partitioned=True): on a partitioned context a fused draw* filters the setup list, and
frr_draw_wireframe, frr_readback_setup, frr_geometry_item_ranges, frr_resolve_varyings, frr_visible_pixels, frr_shade_items and
a further frr_raster behind it are Undefined (FRR_ERR_INVALID) until the next geometry*; ranged shades stay allowed.  The
partitioned mode refuses, it computes nothing else: the model is the UNPARTITIONED frame, which the ranks' parts must stitch to.
run_rank() is one rank's part of a frame, for the fixed sequence line_ownership().

The query sequences.  generate(seed, queries=True) for seed in QSEEDS yields the extended sequences plus (the sequences of
SEEDS and XSEEDS stay as they were: two digests are pinned):
  query         {unit, buf, entries}: frr_query_pixels over the latest pass in the frame's window -- per setup triangle the
                entries rasterization(t) ALONE changes on a copy of the frame's depth at this step (query_reference.counts_c; the
                NumPy oracle's counts asserted equal where the pass is no rung), summed per item or offset by the pass's first
                id, by frr_visible_pixels' every-entry-is-written rule.  A pass that is not rastered counts like any other; zeros
                per item after a clear since the pass; Undefined before any pass and, partitioned, behind a fused draw*.  Targets
                and statistics stay; it bins like frr_raster of the pass, so in front of a rung's raster it is what overflows
  boxes         {vs, items, buf, entries}: frr_query_boxes of a draw list (any list) under the uniforms of the step:
                box_reference.query over the frame's depth, bounds from box_reference.bounds_of of the items' meshes
  query_host, boxes_host, bounds: the host forms and frr_drawlist_bounds, as host queries (QUERIES)
  feeding       m.prov records what wrote a count buffer (count, query or boxes), for which list; a list_if pass may name any of
                them, a box answer only for the list that was asked and under min_value 1.  _Gen.loop is the loop the queries are
                for: the `cover` mesh as occluder, the query, the pass it decides, on one stream
On a partition a rank's box answer is its own (box_answer(args, row_owned)); the ranks' answers sum to zero exactly where the
unpartitioned answer is zero, which is what the partitioned runner's all-reduce relies on.

Left out: user shaders, x0 < 0, a second raster of one geometry pass in another window (the model has one window per
frame), state setters that change the vertex shader's uniforms between a geometry* and its rasterization, resolves behind
the rasterization of a rung mesh (the NumPy oracle's cost).  The generator issues set_cull between passes only;
cull_inside_split() is the fixed sequence with one inside split passes."""
import ctypes
import hashlib

import numpy as np

from f_renderer_amd import scenes
from oracle import oracle_np as onp

from . import box_reference as BX
from . import cull_scenes as CS
from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import lines_reference as R
from . import predicate_scenes as P
from . import query_reference as QR
from . import varyings_scenes as V
from . import visible_scenes as VIS

F = np.float32
W, H = S.W, S.H
CLEAR = S.CLEAR
FULL = (0, W, 0, H)
SUB = (24, 120, 8, 88)                         # x0 > 0, y0 > 0, x1 < W: depth stride 120, partial tiles on every side
NONE = 0xFFFFFFFF
SENTINEL_BITS = V.SENTINEL_BITS
ENTRIES = W * H                                # entries of every varyings buffer
COUNT_CAP = 16384                              # entries of every count buffer
SEEDS = range(24)
FRAMES, MAX_STEPS = 3, 10
MARGIN = 4
TINY = {"bin_capacity": 64, "fan_capacity": 16}
GEOM_BLOCK, FAN_REGIONS = 256, 8
NOOP_SHARE = 0.2
ORDINARY_FAN_NEED = 700                        # the most fan slots a pass that is no rung may need

VS_PS = {"PHONG": ("DEPTH", "FLAT", "PHONG", "BLINN"), "GOURAUD": ("DEPTH", "FLAT", "COLOR")}
VS_K = {"PHONG": 8, "GOURAUD": 3}
PIN_VS = {"CLIP_COLOR": (3, ("DEPTH", "FLAT", "COLOR"))}   # what the generator never draws: the pinning sequences of the CPU tests
K_PS = {8: ("FLAT", "PHONG", "BLINN"), 3: ("FLAT", "COLOR")}
KINDS = ("plain", "indexed", "instanced", "list", "list_if")
COMMANDS = ("lines", "wireframe", "resolve", "shade", "count_item", "count_triangle")
HOST_QUERIES = ("item_ranges", "setup_triangles", "stats", "sync")      # what the first two generators draw from
QUERIES = HOST_QUERIES + ("query_host", "boxes_host", "bounds")
WRITERS = ("geom", "draw", "lines", "wireframe", "resolve", "shade", "count", "set_cull", "set_uniforms", "set_texture", "shade_items",
           "query", "boxes")
COMMANDS_X = COMMANDS + ("shade_items",)       # the extended generator's
COMMANDS_Q = COMMANDS_X + ("query_item", "query_triangle")   # the query generator's
XSEEDS = range(100, 112)                       # the extended seeds: tests/test_gpu_frame_model.py runs them on partitioned contexts
QSEEDS = range(200, 216)                       # the query seeds: run on single contexts with both list sizes AND on partitioned ones

UP, FOVY, ZN, ZF = (0.0, 1.0, 0.0), scenes.demo_camera(W, H)[3], 0.1, 100.0
CAMERAS = [((0.0, 1.0, 3.0), (0.0, 0.0, 0.0)), ((0.9, 0.6, 2.6), (0.0, 0.05, 0.0))]
LIGHTS = [(1.2, 1.0, 2.0), (-1.5, 2.0, 1.0)]
FLATS = [(1.0, 1.0, 1.0, 1.0), (1.0, 0.5, 0.25, 1.0), (0.1, 0.7, 0.9, 0.5)]
WIRE_COLORS = [(255, 200, 0, 255), (0, 255, 120, 255)]
MIN_VALUES = (1, 150)
MASKS = {"mask0": np.array([1, 0, 1, 1, 0, 1, 0, 1], np.uint32), "mask1": np.array([0, 7, 300, 0, 149, 150, 0, 2], np.uint32),
         "mask2": np.zeros(8, np.uint32)}


def _materials(seed):
    """a table of 8 materials (f_renderer_amd.MATERIAL_DTYPE; 8: the most items a generated pass has): slots in {0, 1}, and no
    two neighbours share a slot, a strength or a flat colour; user[...] stays zero (the model has no user shaders)"""
    from f_renderer_amd import MATERIAL_DTYPE
    m = np.zeros(8, MATERIAL_DTYPE)
    k = np.arange(8) + seed
    m["texture_slot"] = k % 2
    m["ambient_strength"] = (0.05 + 0.1 * (k % 5)).astype(F)
    m["specular_strength"] = (0.2 + 0.15 * (k % 4)).astype(F)
    m["flat_color"] = np.stack([((k * 37 + 11 * seed) % 256) / 255.0, ((k * 91 + 40) % 256) / 255.0, ((k * 13 + 200) % 256) / 255.0,
                                1.0 - 0.25 * (k % 3)], axis=1).astype(F)
    return m


MATERIALS = {"mat0": _materials(0), "mat1": _materials(3), "mat2": _materials(5)}
DEVICE_BOUND_TABLE = "mat2"                    # the GPU runner uploads the others with frr_materials_upload


class Undefined(Exception):
    """the step is refused, or its result is not defined, at this place of the sequence"""


# ---- the fixed material: meshes, matrices, textures, line lists ------------------------------------------------------------

def _big(n, seed, radius=3.0):
    """n triangles of `radius` object units around points in front of both cameras: every one crosses several frustum planes and
    is clipped into a fan (7 to 9 fan triangles on average)"""
    rs = np.random.RandomState(seed)
    t = np.zeros((n, 3, 8), F)
    c = np.stack([rs.uniform(-0.8, 0.8, n), rs.uniform(-0.5, 0.5, n), rs.uniform(-1.0, 0.5, n)], 1)
    th0 = rs.uniform(0, 2 * np.pi, n)
    for k in range(3):
        th = th0 + k * 2 * np.pi / 3 + rs.uniform(-0.4, 0.4, n)
        t[:, k, 0], t[:, k, 1] = c[:, 0] + radius * np.cos(th), c[:, 1] + radius * np.sin(th)
        t[:, k, 2] = c[:, 2] + rs.uniform(-0.3, 0.3, n)
        t[:, k, 3], t[:, k, 4] = 0.5 + 0.5 * np.cos(th), 0.5 + 0.5 * np.sin(th)
        t[:, k, 5:8] = (0.0, 0.0, 1.0)
    return t


def _rung2():
    """17 geometry blocks: blocks 0, 8 and 16 -- the three that allocate in fan region 0 -- hold 256 such triangles each, the
    others small triangles in view"""
    rs = np.random.RandomState(103)
    n = 17 * GEOM_BLOCK
    t = np.zeros((n, 3, 8), F)
    c = np.stack([rs.uniform(-1.0, 1.0, n), rs.uniform(-0.7, 0.7, n), rs.uniform(-0.8, 0.4, n)], 1)
    for k in range(3):
        t[:, k, :3] = c + rs.uniform(-0.04, 0.04, (n, 3))
        t[:, k, 3:5] = rs.uniform(0, 1, (n, 2))
        t[:, k, 5:8] = (0.0, 0.0, 1.0)
    for b in (0, 8, 16):
        t[b * GEOM_BLOCK:(b + 1) * GEOM_BLOCK] = _big(GEOM_BLOCK, 104 + b)
    return t


def _cover():
    """the occluder of the query sequences: two large triangles in the plane z = 1 between both cameras and the origin, over
    the left half of the view and a little more -- under the identity the boxes of the small meshes behind it are hidden, those
    beside it are kept.  It is clipped into a dozen setup triangles and is no rung."""
    x0, x1, y0, y1, z = -1.1, 0.3, -0.8, 1.0, 1.0
    c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    t = np.zeros((2, 3, 8), F)
    for k, corners in enumerate(((0, 1, 2), (0, 2, 3))):
        for j, i in enumerate(corners):
            t[k, j, :3] = (c[i][0], c[i][1], z)
            t[k, j, 3:5] = ((c[i][0] - x0) / (x1 - x0), (c[i][1] - y0) / (y1 - y0))
            t[k, j, 5:8] = (0.0, 0.0, 1.0)
    return t


_GRID = S.patch_grid(8, 8)                     # the indexed mesh: 81 vertices under 128 triangles
MESHES = {
    "p40": S.patch(40), "p100": S.patch(100), "p257": S.patch(257), "spiky": D.spiky(30),
    "torus": scenes.torus(10, 6, R=0.3, r=0.12), "grid": np.ascontiguousarray(_GRID[0][_GRID[1].astype(np.int64)]),
    "empty": np.zeros((0, 3, 8), F), "r1": _big(128, 101), "r2": _rung2(),
    "cover": _cover(),                         # (the query sequences alone draw it)
}
INDEXED = {"grid": _GRID}
RUNGS = {1: "r1", 2: "r2"}
SMALL = ("p40", "p100", "spiky", "torus", "grid")
_IDENT = np.eye(4, dtype=F).reshape(16)
MODELS = np.concatenate([S.clipped_models(), S.grid_models(7), CS.mirrored_model()[None], CS.left_model()[None], _IDENT[None]]).astype(F)
M_CLIPPED, M_GRID, M_MIRROR, M_LEFT, M_IDENT = range(0, 6), range(6, 13), 13, 14, 15
TEXTURES = [S.texture(), D.place_textures()[1]]


def _line_list(seed, n=14):
    rs = np.random.RandomState(seed)
    xy = np.stack([rs.randint(0, W, n), rs.randint(0, H, n), rs.randint(0, W, n), rs.randint(0, H, n)], 1).astype(np.uint32)
    xy[0, 2] = xy[0, 0]                        # a vertical, a horizontal and a single-pixel segment
    xy[1, 3] = xy[1, 1]
    xy[2, 2:] = xy[2, :2]
    return xy, rs.randint(0, 256, (n, 4)).astype(np.uint8)


LINES = [_line_list(7), _line_list(8, 9)]


def buffer_names():
    """the caller's device buffers: two pools (frames alternate), each with two varyings buffers per K and three count buffers"""
    return [f"{p}.{b}" for p in "AB" for b in ("v8a", "v8b", "v3a", "v3b", "c0", "c1", "c2")]


def buffer_k(name):
    return {"v8": 8, "v3": 3}.get(name.split(".")[1][:2], 0)


def new_buffers():
    out = {}
    for name in buffer_names():
        k = buffer_k(name)
        out[name] = np.full((ENTRIES, k) if k else COUNT_CAP, SENTINEL_BITS, np.uint32)
    return out


def uniform_kw(mod, cam, light, flat):
    """the uniform keywords of a state for `mod` = the C oracle's binding or f_renderer_amd (set_look_at / set_perspective)"""
    eye, at = CAMERAS[cam]
    return dict(view=mod.set_look_at(eye, at, UP), proj=mod.set_perspective(FOVY, float(W) / float(H), ZN, ZF), view_pos=eye,
                light_pos=LIGHTS[light], flat_color=FLATS[flat])


# ---- geometry of one (mesh, matrix) under one camera, computed once ----------------------------------------------------------

_GEOM, _DET, _NP_CTX = {}, {}, {}


class _Memo(dict):
    """results of the oracles by a digest of everything they depend on (the sensitivity runs repeat most steps unchanged);
    the oldest entries leave when it is full"""

    def __init__(self, size):
        super().__init__()
        self.size = size

    def put(self, key, value):
        if len(self) >= self.size:
            for k in list(self)[:self.size // 4]:
                del self[k]
        self[key] = value
        return value


_RASTER, _SHADE, _PAINT = _Memo(400), _Memo(400), _Memo(200)
_QUERY, _BOXES = _Memo(400), _Memo(2000)


def _digest(*parts):
    h = hashlib.sha1()
    for x in parts:
        h.update(x if isinstance(x, (bytes, bytearray, memoryview)) else x.tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
    return h.digest()


def painted(xyxy, rgba, W=W, H=H):
    """lines_reference.draw_lines of a list as (pixel indices, colours), each pixel once with the colour of its last write"""
    key = _digest(np.ascontiguousarray(xyxy), np.ascontiguousarray(rgba), (W, H))
    if key not in _PAINT:
        last = {}
        for (x1, y1, x2, y2), c in zip(np.asarray(xyxy).tolist(), np.asarray(rgba, np.uint8)):
            if R.panics(x1, y1, x2, y2, W, H):
                raise IndexError("draw_line leaves the buffer")
            for i in R.line_indices(x1, y1, x2, y2, W):
                last[i] = c
        idx = np.fromiter(last.keys(), np.int64, len(last))
        _PAINT.put(key, (idx, np.array(list(last.values()), np.uint8).reshape(-1, 4)))
    return _PAINT[key]


def _item_geometry(oracle, mesh, mi, cam, light, vs, W=W, H=H):
    """(setup list of every input concatenated, triangles each input emits)"""
    key = (mesh, mi, cam, light, vs, W, H)
    if key not in _GEOM:
        kw = uniform_kw(oracle, cam, light, 0)
        u = oracle.make_uniforms(model=MODELS[mi], **kw)
        vs_id = getattr(oracle, "VS_" + vs)
        parts = [oracle.geometry_processing(W, H, t, vs_id, u) for t in MESHES[mesh]]
        counts = np.array([len(p) for p in parts], np.int64)
        setup = np.concatenate(parts) if parts else np.zeros((0, 3), oracle.VERTEX_DTYPE)
        _GEOM[key] = (setup, counts)
    return _GEOM[key]


def _det(mesh, mi, cam, vs):
    """the facing determinant of every input (cull_scenes.det_f32 of oracle_np.vertex_shader's clip positions)"""
    key = (mesh, mi, cam)
    if key not in _DET:
        eye, at = CAMERAS[cam]
        u = onp.Uniforms(model=MODELS[mi], view=onp.set_look_at(eye, at, UP), proj=onp.set_perspective(FOVY, float(W) / float(H), ZN, ZF))
        vs_id = getattr(onp, "VS_" + vs)
        clip = np.array([[onp.vertex_shader(vs_id, u, v)[0] for v in t] for t in MESHES[mesh]], F).reshape(-1, 3, 4)
        _DET[key] = CS.det_f32(clip)
    return _DET[key]


def growth(need, extra):
    """what finish() grows a list to after a pass that needed `need`: need + need / extra + 1024"""
    return need + need // extra + 1024


def pass_needs(setup, fans):
    """(fan slots, bin records) a pass needs, as finish() counts them: eight times the fullest region's fan triangles (block b
    of 256 inputs allocates in region b % 8; `fans`: fan triangles per submitted input, 0 for one that is not clipped or emits
    nothing); setup triangles times the 32-pixel tiles under their bounding boxes"""
    region = np.zeros(FAN_REGIONS, np.int64)
    for b in range(0, len(fans), GEOM_BLOCK):
        region[(b // GEOM_BLOCK) % FAN_REGIONS] += int(fans[b:b + GEOM_BLOCK].sum())
    spi = setup["spi"].astype(np.int64)
    if spi.shape[0]:
        lo = np.clip(spi.min(axis=1), 0, [W, H])
        hi = np.clip(spi.max(axis=1), 0, [W, H])
        tiles = np.maximum((hi + 31) // 32 - lo // 32, 0)
        bins = int((tiles[:, 0] * tiles[:, 1] * ((hi > lo).all(axis=1))).sum())
    else:
        bins = 0
    return int(region.max()) * FAN_REGIONS, bins


class _Pass:
    pass


def _vs_k(vs):
    return VS_K[vs] if vs in VS_K else PIN_VS[vs][0]


def _vs_ps(vs):
    return VS_PS[vs] if vs in VS_PS else PIN_VS[vs][1]


# ---- the model ---------------------------------------------------------------------------------------------------------------

class Model:
    """The state a sequence of steps leaves behind: the frame on the C oracle, the caller's buffers, the state that travels
    with commands, the latest geometry pass, the host's statistics, and the upper bounds of the work lists."""

    def __init__(self, oracle, size=(W, H), clear=CLEAR, partitioned=False):
        self.o, (self.W, self.H), self.clear = oracle, size, clear
        self.part = partitioned                # the sequence has to be legal on a partitioned context (frr_set_partition, world > 1)
        self.cull, self.cam, self.light, self.flat, self.slot, self.tex = 0, 0, 0, 0, 0, [0, 1]
        self.frame = oracle.Frame(*size)
        self.window, self.fno = FULL, -1
        self.tris_in = self.draws = self.emitted = 0
        self.last = None
        self.bufs = new_buffers()
        self.prov = {}                         # count buffer -> what the latest count, query or box query into it was
        self.box_log = []                      # this frame's box queries into buffers: what a rank's own answer is computed from
        self.wrote = {}                        # varyings buffer -> the entries this frame's resolves wrote (bool[ENTRIES])
        self.buf_win = {}                      # varyings buffer -> the (x1, rows) of the windows its resolves ran in, ever
        self.fan_cap, self.bin_cap = TINY["fan_capacity"], TINY["bin_capacity"]
        self.crossed = False                   # a rung was crossed in this frame
        self.crossed_fan = False               # ... a rung of the fan slots, by a pass no partition filters: the same on every rank
        self.changed = False                   # the latest step changed a target or a buffer

    def copy(self):
        m = Model.__new__(Model)
        m.__dict__.update(self.__dict__)
        m.tex = list(self.tex)
        m.frame = self.o.Frame(self.W, self.H)
        m.frame.color[...] = self.frame.color
        m.frame.depth[...] = self.frame.depth
        m.frame.tri_id[...] = self.frame.tri_id
        ctypes.memmove(ctypes.byref(m.frame.counters), ctypes.byref(self.frame.counters), ctypes.sizeof(self.frame.counters))
        m.bufs = {k: v.copy() for k, v in self.bufs.items()}
        m.prov = dict(self.prov)
        m.box_log = list(self.box_log)
        m.wrote = {k: v.copy() for k, v in self.wrote.items()}
        m.buf_win = {k: set(v) for k, v in self.buf_win.items()}
        return m

    # -- uniforms of the moment --
    def _uniforms(self):
        return uniform_kw(self.o, self.cam, self.light, self.flat), self.tex[self.slot]

    def _window_entries(self):
        x0, x1, y0, y1 = self.window
        return (y1 - y0) * x1

    def _window_index(self):
        x0, x1, y0, y1 = self.window
        cy, cx = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
        return (cy - y0) * x1 + (cx - x0), cy - y0, cx - x0

    def _latest(self, cleared_ok=False, filtered_ok=False):
        if self.last is None or (self.last.cleared and not cleared_ok):
            raise Undefined("no geometry pass in this frame yet")
        if self.part and self.last.filtered and not filtered_ok:
            raise Undefined("on a partitioned context a fused draw* filters the setup list: FRR_ERR_INVALID")
        return self.last

    # -- steps --
    def apply(self, s):
        """apply one step; returns the host's answer of a query, or None"""
        self.changed = False
        return getattr(self, "_" + s["op"])(s)

    def _clear(self, s):
        self.frame.clear(*self.clear)
        self.frame.counters = type(self.frame.counters)()
        self.window, self.fno = tuple(s["window"]), self.fno + 1
        self.tris_in = self.draws = self.emitted = 0
        self.crossed = self.crossed_fan = False
        self.wrote = {}
        self.box_log = []
        if self.last is not None:
            self.last = self._copy_pass(self.last)
            self.last.cleared = True

    @staticmethod
    def _copy_pass(p):
        q = _Pass()
        q.__dict__.update(p.__dict__)
        return q

    def _set_cull(self, s):
        self.cull = s["mode"]

    def _set_uniforms(self, s):
        if self.last is not None and not self.last.cleared and not self.last.rastered and (s["cam"], s["light"]) != (self.cam, self.light):
            raise Undefined("the model does not change the vertex shader's uniforms inside a split pass")
        self.cam, self.light, self.flat, self.slot = s["cam"], s["light"], s["flat"], s["slot"]

    def _set_texture(self, s):
        self.tex[s["slot"]] = s["image"]

    def _geom(self, s, fused=False):
        # (behind a pass that was never rastered -- an abandoned one -- too: it counted its tris_in, draws and triangles at its
        # geometry call, owns no pixel, and this pass's ids start behind it)
        items, vs = [tuple(i) for i in s["items"]], s["vs"]
        if s["kind"] == "list_if":
            kept = P.kept_of(self.bufs[s["keep"]].reshape(-1)[:len(items)], s["min"]) if s["keep"] in self.bufs else \
                P.kept_of(MASKS[s["keep"]][:len(items)], s["min"])
        else:
            kept = np.ones(len(items), bool)
        p = _Pass()
        # (a list without items names no vertex shader: its K is 0, and any pixel shader goes with nothing)
        p.items, p.vs, p.K, p.kind, p.cam, p.light = items, vs, _vs_k(vs) if items else 0, s["kind"], self.cam, self.light
        p.kept, p.cull = kept, self.cull        # (which items the predicate kept; the cull mode of the geometry call)
        p.keep, p.per_item, setups, fans = [], [], [], []
        for i, (mesh, mi) in enumerate(items):
            setup, counts = _item_geometry(self.o, mesh, mi, self.cam, self.light, vs, self.W, self.H)
            k = np.full(counts.size, bool(kept[i]), bool)
            if self.cull != CS.NONE and counts.size:
                k &= CS.keeps(_det(mesh, mi, self.cam, vs), self.cull)
            emit = np.where(k, counts, 0)
            p.keep.append(k)
            p.per_item.append(int(emit.sum()))
            fans.append(np.where(emit > 1, emit, 0))
            setups.append(setup[np.repeat(k, counts)])
        p.setup = np.concatenate(setups) if setups else np.zeros((0, 3), self.o.VERTEX_DTYPE)
        p.base, p.emit, p.rastered, p.cleared, p.filtered = self.emitted, sum(p.per_item), False, False, False
        p.fan_need, p.bin_need = pass_needs(p.setup, np.concatenate(fans) if fans else np.zeros(0, np.int64))
        p.fan_rung, p.bin_rung = p.fan_need >= MARGIN * self.fan_cap, p.bin_need >= MARGIN * self.bin_cap
        self.crossed |= p.fan_rung or p.bin_rung
        # (a fused draw* on a partitioned context filters its inputs by the rank's rows: what a rank needs there is a fraction
        # the model does not compute -- nothing at all on a rank that owns nothing)
        self.crossed_fan |= p.fan_rung and not (fused and self.part)
        if p.fan_need > TINY["fan_capacity"]:     # the pass may have overflowed: what the growth rule can have left
            self.fan_cap = max(self.fan_cap, growth(p.fan_need, 8))
        if p.bin_need > TINY["bin_capacity"]:
            self.bin_cap = max(self.bin_cap, growth(p.bin_need, 4))
        self.tris_in += sum(MESHES[m].shape[0] for m, _ in items)
        self.draws += 1
        self.emitted += p.emit
        self.last = p

    def _raster(self, s, fused=False):
        # (a pass that is rastered already is rastered again, in the frame's one window: the loop over its setup list runs again
        # over the frame as it is now, with the same ids -- `rhw < depth` rejects, equal depth replaces, so after a depth-only
        # raster a shading one gives every pixel of the pass its colour.  frag_covered and frag_nan add up again; draws,
        # tris_in and tris_setup counted at the geometry call.  before / after / ps are those of the LATEST raster: a resolve
        # sees the ownership that the last raster left.)
        p = self._latest(filtered_ok=fused)
        if p.items and s["ps"] not in _vs_ps(p.vs):
            raise Undefined("a pixel shader for another K")
        if (p.cam, p.light) != (self.cam, self.light):
            raise Undefined("the model does not change the vertex shader's uniforms inside a split pass")
        p = self.last = self._copy_pass(p)
        f = self.frame
        p.before = (f.color.copy(), f.depth.copy(), f.tri_id.copy())
        sc = D.Scene([D.Mesh(MESHES[m]) for m, _ in p.items], range(len(p.items)), MODELS[[mi for _, mi in p.items]].reshape(-1, 16), p.vs, s["ps"])
        kw, image = self._uniforms()
        kw["tex"] = self.o.Texture(TEXTURES[image])
        key = _digest(*p.before, (p.items, p.vs, s["ps"], p.cam, p.light, self.flat, image, self.window, p.base), *p.keep,
                      bytes(f.counters))
        if key in _RASTER:
            p.after, counters = _RASTER[key]
            f.color[...], f.depth[...], f.tri_id[...] = p.after
            ctypes.memmove(ctypes.byref(f.counters), counters, len(counters))
        else:
            _, setup, per = D.oracle_list_loop(self.o, sc, s["ps"], frame=f, window=self.window, keep=p.keep, tri_id_base=p.base, kw=kw)
            assert per == p.per_item and setup.tobytes() == p.setup.tobytes(), "the split pass's geometry is the fused pass's"
            p.after = (f.color.copy(), f.depth.copy(), f.tri_id.copy())
            _RASTER.put(key, (p.after, bytes(f.counters)))
        p.rastered, p.ps, p.state = True, s["ps"], (self.flat, image)
        self.changed = any((a != b).any() for a, b in zip(p.before[1:], p.after[1:])) or (p.before[0] != p.after[0]).any() or p.emit > 0

    def _draw(self, s):
        self._geom(s, fused=True)
        self.last.filtered = True              # (what a partitioned context does to the setup list of a fused pass)
        self._raster(s, fused=True)

    def _lines(self, s):
        self._paint(*LINES[s["list"]])

    def _paint(self, xyxy, rgba):
        idx, col = painted(xyxy, rgba, self.W, self.H)
        flat = self.frame.color.reshape(-1, 4)
        self.changed = bool((flat[idx] != col).any())
        flat[idx] = col

    def _wireframe(self, s):
        p = self._latest()
        if not hasattr(p, "segs"):
            p.segs = R.wireframe_segments(p.setup["spi"], self.W, self.H)[0]       # (of the pass: whoever holds it later finds it there)
        segs = p.segs
        if segs:
            self._paint(np.array(segs, np.uint32), np.tile(np.array(WIRE_COLORS[s["color"]], np.uint8), (len(segs), 1)))

    def _owned(self, p):
        t = self.frame.tri_id
        return (t != NONE) & (t >= p.base) & (t < p.base + p.emit)

    def _resolve(self, s):
        p = self._latest()
        buf = self.bufs[s["buf"]]
        if buffer_k(s["buf"]) != p.K:
            raise Undefined("a buffer of another K")
        if not p.rastered or not p.emit:
            return
        n = self._window_entries()
        own = self._owned(p)[:n]
        ctx = self._np_ctx(p)[:n]
        assert not np.isnan(ctx[own]).all(axis=1).any(), "an owned entry without varyings"
        before = buf[:n][own].copy()
        buf[:n][own] = ctx[own].view(np.uint32)
        self.wrote.setdefault(s["buf"], np.zeros(buf.shape[0], bool))[:n] |= own
        if own.any():
            self.buf_win.setdefault(s["buf"], set()).add((self.window[1], self.window[3] - self.window[2]))
        self.changed = (before != buf[:n][own]).any()

    def _np_ctx(self, p):
        """the interpolated varyings of every fragment of the latest pass that passed the depth test, by depth index: the NumPy
        oracle's draw of the pass over the frame as it was before, held to the C oracle's frame after it"""
        color, depth, tri = (a.copy() for a in p.before)
        key = hashlib.sha1(repr((p.items, p.vs, p.ps, p.cam, p.light, p.state, self.window, p.base, self.W, self.H, [k.tobytes() for k in p.keep])).encode()
                           + depth.tobytes() + tri.tobytes()).hexdigest()
        if key in _NP_CTX:
            return _NP_CTX[key]
        eye, at = CAMERAS[p.cam]
        flat, image = p.state
        ps = V.zero_ps if p.ps == "DEPTH" else getattr(onp, "PS_" + p.ps)
        debug, base = {}, p.base
        for (mesh, mi), keep, emit in zip(p.items, p.keep, p.per_item):
            tris = MESHES[mesh][keep]
            if tris.shape[0]:
                u = onp.Uniforms(model=MODELS[mi], view=onp.set_look_at(eye, at, UP), proj=onp.set_perspective(FOVY, float(W) / float(H), ZN, ZF),
                                 view_pos=eye, flat_color=FLATS[flat], tex=TEXTURES[image], light_pos=LIGHTS[p.light])
                setup, _ = onp.draw(self.W, self.H, tris, getattr(onp, "VS_" + p.vs), ps, u, color, depth, tri, window=self.window, tri_id_base=base, debug=debug)
                assert len(setup) == emit
            base += emit
        np.testing.assert_array_equal(tri, p.after[2], err_msg="the NumPy oracle's ids differ from the C oracle's")
        np.testing.assert_array_equal(depth.view(np.uint32), p.after[1].view(np.uint32), err_msg="the NumPy oracle's depth differs from the C oracle's")
        if p.ps != "DEPTH":
            np.testing.assert_array_equal(color, p.after[0], err_msg="the NumPy oracle's colour differs from the C oracle's")
        _NP_CTX[key] = debug.get("ctx", np.full((self.W * self.H, p.K), np.nan, F))
        return _NP_CTX[key]

    def _rank_holds(self, name):
        """On a partitioned context a resolve writes the entries of the rank's rows only, and nothing carries them to the other
        ranks: a shade reads what the ranks' resolves left where every one of them ran in a window with this one's depth
        stride and rows (entry i is then the same rank's, i // x1 being its row) -- or nothing was resolved at all."""
        if self.part and self.buf_win.get(name, set()) - {(self.window[1], self.window[3] - self.window[2])}:
            raise Undefined("a varyings buffer resolved in a window that divides its entries among the ranks in another way")

    def _shade(self, s):
        self._rank_holds(s["buf"])
        buf, K = self.bufs[s["buf"]], buffer_k(s["buf"])
        if s["ps"] not in K_PS[K]:
            raise Undefined("a pixel shader for another K")
        self._shade_range(s["ps"], buf, *s["ids"])

    def _shade_range(self, ps, buf, first, count, material=None):
        """frr_shade_varyings of one id range under the uniforms of the moment -- with `material` (one record of MATERIALS) its
        texture slot, strengths and flat colour in place of theirs"""
        idx, ry, rx = self._window_index()
        ids = self.frame.tri_id[idx].astype(np.int64)
        sel = (ids != NONE) & (((ids - first) & 0xFFFFFFFF) < count)
        if not sel.any():
            return
        kw, image = self._uniforms()
        what = (ps, self.cam, self.light, self.flat, image)
        if material is not None:
            image = self.tex[int(material["texture_slot"])]     # (the slot's texture as of the call)
            kw.update(ambient=material["ambient_strength"], specular=material["specular_strength"], flat_color=material["flat_color"])
            what = (ps, self.cam, self.light, image, material.tobytes())
        kw["tex"] = self.o.Texture(TEXTURES[image])
        ctx = np.ascontiguousarray(buf[idx[sel]])
        key = _digest(what, ctx)
        rgba = _SHADE[key] if key in _SHADE else \
            _SHADE.put(key, self.o.shade_pixels(getattr(self.o, "PS_" + ps), self.o.make_uniforms(**kw), ctx.view(F)))
        before = self.frame.color[ry[sel], rx[sel]].copy()
        self.frame.color[ry[sel], rx[sel]] = rgba
        self.changed |= bool((before != rgba).any())

    def _shade_items(self, s):
        """frr_shade_items by its definition in include/frr.h: for every item k of the latest pass one ranged shade over
        (id_first[k], id_count[k]) under the call's uniforms with materials[k]'s texture slot, strengths and flat colour.
        After a clear since the pass, for a pass that emitted nothing and for one that is not rastered yet (its ids are not in
        the target) that writes nothing."""
        if self.last is None:
            raise Undefined("before any geometry pass")
        p = self._latest(cleared_ok=True)
        self._rank_holds(s["buf"])
        buf, K = self.bufs[s["buf"]], buffer_k(s["buf"])
        if s["ps"] not in K_PS[K]:
            raise Undefined("a pixel shader for another K")
        table = MATERIALS[s["table"]]
        if len(table) < len(p.items):
            raise Undefined("a table with fewer entries than the pass has items")
        if p.cleared:
            return
        first = VIS.bounds_of(p.per_item, p.base)
        for k, n in enumerate(p.per_item):
            self._shade_range(s["ps"], buf, int(first[k]), int(n), table[k])

    def _count(self, s):
        buf, e = self.bufs[s["buf"]], int(s["entries"])
        if not 0 < e <= COUNT_CAP:
            raise Undefined("out_entries")
        x0, x1, y0, y1 = self.window
        if s["unit"] == "item":
            p = self._latest(cleared_ok=True)
            n = len(p.items)
            out = np.zeros(e, np.uint32) if p.cleared else \
                VIS.want_counts(self.frame.tri_id, (x0, x1), (y0, y1), bounds=VIS.bounds_of(p.per_item, p.base), entries=e)
        else:
            p = self._latest()
            n = p.base + p.emit
            out = VIS.want_counts(self.frame.tri_id, (x0, x1), (y0, y1), units=n, entries=e)
        self.changed = (buf[:e] != out).any()
        buf[:e] = out
        self.prov[s["buf"]] = dict(frame=self.fno, unit=s["unit"], n=n, entries=e, items=p.items, kind=p.kind, source="count", vs=p.vs)

    # -- occlusion queries (include/frr.h, "occlusion queries") --
    def _query_counts(self, p):
        """per setup triangle of pass p the entries rasterization(t) ALONE changes on a copy of the frame's depth as it is now
        (query_reference.counts_c); where the pass is no rung the same on the NumPy oracle, asserted equal"""
        assert (self.W, self.H) == (QR.W, QR.H), "query_reference is written for the 128 x 96 frame"
        depth = np.array(self.frame.depth, F)
        key = _digest(b"query", depth, p.setup, self.window)
        if key not in _QUERY:
            per_tri = QR.counts_c(self.o, depth, p.setup, self.window)
            if not any(mesh in RUNGS.values() for mesh, _ in p.items):
                np.testing.assert_array_equal(QR.counts_np(depth, p.setup, self.window), per_tri, err_msg="the NumPy oracle's query counts differ from the C oracle's")
            _QUERY.put(key, per_tri)
        return _QUERY[key]

    def _query_answer(self, s):
        """(out uint32 [entries], n, the pass) of frr_query_pixels at this place.  The units, n and the every-entry-is-written
        rule are frr_visible_pixels': after a clear since the pass the per-item answer is zeros (the per-triangle one the model
        leaves undefined, as it leaves that count); a dropped item and a culled input have no setup triangle and count 0"""
        e = int(s["entries"])
        if not 0 < e <= COUNT_CAP:
            raise Undefined("out_entries")
        if self.last is None:
            raise Undefined("before any geometry pass")
        p = self._latest(cleared_ok=s["unit"] == "item")
        out = np.zeros(e, np.uint32)
        if s["unit"] == "item":
            n = len(p.items)
            vals = np.zeros(n, np.uint32) if p.cleared else QR.per_item_sums(self._query_counts(p), p.per_item)
        else:
            n = p.base + p.emit
            vals = np.concatenate([np.zeros(p.base, np.uint32), self._query_counts(p)])
        out[:min(n, e)] = vals[:min(n, e)]
        return out, n, p

    def _query(self, s):
        buf = self.bufs[s["buf"]]
        out, n, p = self._query_answer(s)
        e = out.size
        # (the query bins like frr_raster of the same pass: in front of the raster of a bin rung it is the command that overflows)
        if not p.cleared:
            self.crossed |= p.fan_rung or p.bin_rung
        self.changed = bool((buf[:e] != out).any())
        buf[:e] = out
        self.prov[s["buf"]] = dict(frame=self.fno, unit=s["unit"], n=n, entries=e, items=p.items, kind=p.kind, source="query", vs=p.vs)

    def _query_host(self, s):
        return dict(out=self._query_answer(s)[0])

    # -- box queries (include/frr.h, "box queries") --
    def _bounds_of(self, items):
        per = [BX.bounds_of(MESHES[mesh]) for mesh, _ in items]      # (the expanded `grid`: the corners its triangles name)
        lo_hi = np.stack([b for b, _ in per]).astype(F) if per else np.zeros((0, 6), F)
        return lo_hi, np.array([f for _, f in per], np.uint32)

    def _box_args(self, s):
        """what frr_query_boxes of the step's list reads at this place: the matrices under the uniforms of the moment, the
        bounds table, the viewport, the frame's window and the depth as it is now (a pending clear is settled: the model's
        clear is never pending)"""
        if s["vs"] not in VS_PS:
            raise Undefined("a list whose vertex shader has no object space")
        e = int(s["entries"])
        if not 0 < e <= COUNT_CAP:
            raise Undefined("out_entries")
        items = [tuple(i) for i in s["items"]]
        kw, _ = self._uniforms()
        proj, view = (np.asarray(kw[k], F).reshape(16) for k in ("proj", "view"))
        lo_hi, flags = self._bounds_of(items)
        return dict(mvps=BX.mvps_of(proj, view, MODELS[[mi for _, mi in items]].reshape(-1, 16)), lo_hi=lo_hi, flags=flags, size=(self.W, self.H),
                    window=self.window, depth=np.array(self.frame.depth, F), entries=e)

    def _boxes(self, s):
        buf, args = self.bufs[s["buf"]], self._box_args(s)
        out, srl = box_answer(args)
        e = out.size
        self.changed = bool((buf[:e] != out).any())
        buf[:e] = out
        items = [tuple(i) for i in s["items"]]
        self.box_log = self.box_log + [dict(buf=s["buf"], args=args, out=out, srl=srl)]
        self.prov[s["buf"]] = dict(frame=self.fno, unit="item", n=len(items), entries=e, items=items, kind="list", source="boxes", vs=s["vs"])

    def _boxes_host(self, s):
        args = self._box_args(s)
        out, srl = box_answer(args)
        return dict(out=out, args=args, srl=srl)

    def _bounds(self, s):
        lo_hi, flags = self._bounds_of([tuple(i) for i in s["items"]])
        return dict(lo_hi=lo_hi, flags=flags)

    def _item_ranges(self, s):
        p = self._latest()
        return dict(first=VIS.bounds_of(p.per_item, p.base)[:-1], count=np.array(p.per_item, np.uint32))

    def _setup_triangles(self, s):
        p = self._latest()
        return dict(spi=p.setup["spi"].copy(), spf=p.setup["spf"].copy(), rhw=p.setup["rhw"].copy())

    def stats(self):
        c = self.frame.counters
        return dict(tris_in=self.tris_in, tris_setup=self.emitted, draws=self.draws, frag_covered=int(c.frag_covered), frag_nan=int(c.frag_nan))

    def _stats(self, s):
        return self.stats()

    def _sync(self, s):
        return None

    def _readback(self, s):
        return None

    _fenced = _readback

    def outputs(self):
        """what a frame end is compared with"""
        f = self.frame
        return dict(color=f.color.copy(), depth=f.depth.copy(), tri_id=f.tri_id.copy(), stats=self.stats(),
                    bufs={k: v.copy() for k, v in self.bufs.items()}, crossed=self.crossed, crossed_fan=self.crossed_fan, boxes=list(self.box_log),
                    wrote={k: v.copy() for k, v in self.wrote.items()})


def box_answer(args, row_owned=None):
    """(out, status_rect_level) of a box query whose inputs Model._box_args recorded -- with row_owned (bool per window-local
    tile row) the answer of the rank of a partition that owns those rows"""
    key = _digest(b"boxes", args["mvps"], args["lo_hi"], args["flags"], (args["size"], args["window"], args["entries"]), args["depth"],
                  None if row_owned is None else np.asarray(row_owned, bool))
    if key not in _BOXES:
        _BOXES.put(key, BX.query(args["mvps"], args["lo_hi"], args["flags"], args["size"], args["window"], args["depth"], row_owned=row_owned,
                                 entries=args["entries"]))
    return _BOXES[key]


def rank_tile_rows(window, rank, world, blocked):
    """bool per window-local tile row: the rows rank `rank` owns in the window (what a draw, a count and a query go by)"""
    from f_renderer_amd.multigpu import tile_row_owner
    return np.asarray(tile_row_owner((window[3] - window[2] + 31) // 32, world, blocked)) == rank


def run_frames(model, frames, skip=None):
    """apply frames (lists of steps) to `model`; skip: a set of id(step) left out.  Returns per frame the model's outputs at the
    frame end with the queries' answers, in order, under "answers"."""
    out = []
    for steps in frames:
        answers = []
        for s in steps:
            if skip and id(s) in skip:
                continue
            if s.get("refused"):               # (a fixed sequence's step that the library has to refuse at this place)
                try:
                    model.copy().apply(s)
                except Undefined:
                    continue
                raise AssertionError("the model takes a step marked as refused: " + describe(s))
            a = model.apply(s)
            if s["op"] in QUERIES:
                answers.append((s["op"], a))
        o = model.outputs()
        o["answers"] = answers
        out.append(o)
    return out


def run_model(oracle, frames, **kw):
    """what every frame of a sequence must leave behind: per frame the colour, depth and triangle ids, the statistics, every
    caller buffer, the host queries' answers in order, and whether the model says a rung is crossed in it"""
    return run_frames(Model(oracle, **kw), frames)


def command_rows(op, window, height, rank, world, blocked):
    """bool[height]: the plane rows of the colour target (= window-local rows) in which rank `rank` performs a command.  Draws,
    resolves, shades and counts take their owner from the WINDOW's tile rows, frr_draw_lines and frr_draw_wireframe from the
    CONTEXT's (frr_api.hip: row_owner(f, tiles_y) with each command's own tiles_y)."""
    from f_renderer_amd.multigpu import tile_row_owner
    x0, x1, y0, y1 = window
    rows = height if op in ("lines", "wireframe") else y1 - y0
    own = np.zeros(height, bool)
    own[:rows] = np.asarray(tile_row_owner((rows + 31) // 32, world, blocked))[np.arange(rows) // 32] == rank
    return own


def run_rank(oracle, steps, rank, world, blocked, **kw):
    """One frame as ONE rank of a partition leaves it: every step is applied to the rank's own frame and undone in the rows and
    entries its command does not own there (each command's result at a pixel depends on that pixel and its entry alone).
    For frames without counts and predicated passes, whose geometry depends on what the other ranks counted."""
    m = Model(oracle, **kw)
    for s in steps:
        assert s["op"] != "count" and s.get("kind") != "list_if"
        if s["op"] == "clear":
            m.apply(s)
            continue
        own = command_rows(s["op"], m.window, m.H, rank, world, blocked)
        row = np.arange(m.W * m.H) // m.window[1]
        mine = np.zeros(m.W * m.H, bool)
        mine[row < m.H] = own[row[row < m.H]]
        f = m.frame
        before = (f.color.copy(), f.depth.copy(), f.tri_id.copy(), {k: v.copy() for k, v in m.bufs.items() if buffer_k(k)})
        m.apply(s)
        f.color[~own] = before[0][~own]
        f.depth[~mine], f.tri_id[~mine] = before[1][~mine], before[2][~mine]
        for k, v in before[3].items():
            m.bufs[k][:mine.size][~mine] = v[:mine.size][~mine]
    return m.outputs()


def same_outputs(a, b):
    """do two frame outputs agree in everything that is compared?"""
    if a["stats"] != b["stats"] or len(a["answers"]) != len(b["answers"]):
        return False
    for k in ("color", "depth", "tri_id"):
        if a[k].tobytes() != b[k].tobytes():
            return False
    if any(a["bufs"][k].tobytes() != b["bufs"][k].tobytes() for k in a["bufs"]):
        return False
    for (na, xa), (nb, xb) in zip(a["answers"], b["answers"]):
        if na != nb or (xa is None) != (xb is None):
            return False
        if isinstance(xa, dict) and any(np.asarray(xa[k]).tobytes() != np.asarray(xb[k]).tobytes() for k in xa if not isinstance(xa[k], dict)):
            return False
    return True


def pass_partners(steps, s):
    """the rasterizations that belong to the geometry step s of a split pass: those up to the next geometry pass (one, in the
    sequences of SEEDS; none for an abandoned pass, several for one that is rastered again)"""
    i = next(k for k, x in enumerate(steps) if x is s)
    out = []
    for x in steps[i + 1:]:
        if x["op"] in ("geom", "draw"):
            break
        if x["op"] == "raster":
            out.append(x)
    return out


def _drop_of(steps, s):
    return {id(s)} | ({id(x) for x in pass_partners(steps, s)} if s["op"] == "geom" else set())


def insensitive_steps(oracle, frames, **model_kw):
    """The writing steps, not marked as no-ops, whose removal changes no compared output (a split pass is removed as a whole,
    the commands inside it stay; a rasterization of a pass that is rastered already is removed by itself too).  A removal
    after which a later step is refused or undefined counts as a change."""
    starts, m = [], Model(oracle, **model_kw)
    want = []
    for steps in frames:
        starts.append(m.copy())
        want += run_frames(m, [steps])
    bad = []
    for fi, steps in enumerate(frames):
        for s in steps:
            again = s["op"] == "raster" and s.get("again")
            if (s["op"] not in WRITERS and not again) or s.get("noop"):
                continue
            skip = _drop_of(steps, s)
            try:
                m = starts[fi].copy()
                same = all(same_outputs(run_frames(m, [frames[k]], skip)[0], want[k]) for k in range(fi, len(frames)))
            except (Undefined, RuntimeError):
                same = False
            if same:
                bad.append((fi, s))
    return bad


# ---- the generator -----------------------------------------------------------------------------------------------------------

class _Gen:
    """Draws steps with np.random.RandomState(seed) and consults the model for each: a step that is refused or undefined at its
    place is drawn again, a step that writes is kept only if it changes a target or a buffer (or is a no-op on purpose, while
    the seed's share of those allows one more), a state setter only in front of a command that comes out differently under it."""

    def __init__(self, oracle, seed, extended=False, queries=False):
        extended = extended or queries
        self.o, self.seed, self.rng, self.m = oracle, seed, np.random.RandomState(seed), Model(oracle, partitioned=extended)
        self.ext = extended                    # shade_items, second rasters and abandoned passes; legal on a partitioned context
        self.q = queries                       # ... and occlusion queries, box queries, their host forms and the passes they decide
        self.commands = COMMANDS_Q if queries else COMMANDS_X if extended else COMMANDS
        self.box_lists = []                    # (vs, items) of the lists a box query has been asked of
        self.list_cam = {}                     # (vs, items) -> the camera of the list's last use (a pass over it or a box query)
        self.last_resolve = None               # the varyings buffer the latest resolve wrote into
        self.frames, self.steps, self.reserve = [], None, 0
        self.noops = self.total = 0
        self.ranges = []                       # (first, count) of the items of this frame's rastered passes
        self.resolved = []                     # varyings buffers a resolve has written into
        self.geom_step = None

    def pick(self, seq, p=None):
        return seq[self.rng.choice(len(seq), p=p)]

    def room(self):
        """steps this frame can still take before its end (the clear does not count, the frame end does)"""
        return MAX_STEPS - 1 - (len(self.steps) - 1) - self.reserve

    def noop_allowed(self):
        return self.noops + 1 <= NOOP_SHARE * (self.total + 1)

    def probe(self, steps):
        """(a digest of the targets and the setup list after `steps` on a copy of the model, did the last one change
        anything), or (None, False) where a step is refused or undefined"""
        trial = self.m.copy()
        try:
            for s in steps:
                trial.apply(s)
        except (Undefined, RuntimeError):
            return None, False
        f, p = trial.frame, trial.last
        self.probed = trial
        return (f.color.tobytes(), f.depth.tobytes(), f.tri_id.tobytes(), p.setup.tobytes() if p is not None else b"", trial.emitted), trial.changed

    def add(self, s, noop_ok=False, force=False):
        if self.room() < (2 if s["op"] == "geom" else 1) and not force:
            return False
        trial = self.m.copy()
        try:
            trial.apply(s)
        except (Undefined, RuntimeError):
            return False
        if s["op"] in ("lines", "wireframe", "resolve", "shade", "shade_items", "count", "draw", "raster", "query", "boxes") and not trial.changed:
            if not force and not (noop_ok and self.noop_allowed()):
                return False
            (self.geom_step if s["op"] == "raster" else s)["noop"] = True
            self.noops += 1
        self.m = trial
        self.steps.append(s)
        self.total += 1
        if self.q and s["op"] in ("geom", "draw", "boxes", "boxes_host") and (s["op"] in ("boxes", "boxes_host") or s["kind"] in ("list", "list_if")):
            self.list_cam[s["vs"], tuple(tuple(i) for i in s["items"])] = trial.cam
        if s["op"] == "geom":
            self.geom_step = s
            if self.ext:                       # (an abandoned pass meets no raster that would record them)
                p = trial.last
                s.update(fan_need=p.fan_need, bin_need=p.bin_need, fan_rung=bool(p.fan_rung), bin_rung=bool(p.bin_rung))
        if s["op"] in ("draw", "raster"):
            p = trial.last
            first = VIS.bounds_of(p.per_item, p.base)
            self.ranges += [(int(first[i]), int(c)) for i, c in enumerate(p.per_item)]
            (self.geom_step if s["op"] == "raster" else s).update(fan_need=p.fan_need, bin_need=p.bin_need, fan_rung=bool(p.fan_rung),
                                                                   bin_rung=bool(p.bin_rung))
        return True

    # -- candidates --
    def setter(self, inside):
        """inside a split pass only what the pixel shader reads changes (the model's restriction)"""
        rng, m = self.rng, self.m
        kind = self.pick(("cull", "uniforms", "texture"), p=(0.0, 0.6, 0.4) if inside else (0.35, 0.45, 0.2))
        if kind == "cull":
            return dict(op="set_cull", mode=int(self.pick([x for x in (0, 1, 2) if x != m.cull])))
        if kind == "texture":
            slot = m.slot if rng.rand() < 0.8 else 1 - m.slot      # (mostly the slot the pixel shaders sample)
            return dict(op="set_texture", slot=slot, image=1 - m.tex[slot])
        s = dict(op="set_uniforms", cam=m.cam, light=m.light, flat=m.flat, slot=m.slot)
        what = self.pick(("flat", "slot")) if inside else self.pick(("cam", "light", "flat", "slot"), p=(0.4, 0.2, 0.2, 0.2))
        s[what] = int(self.pick([x for x in range(3 if what == "flat" else 2) if x != s[what]]))
        return s

    def new_pass(self, rung):
        rng, m = self.rng, self.m
        s = dict(vs=self.pick(("PHONG", "GOURAUD")))
        if rung:
            kind = self.pick(("plain", "list", "list_if"), p=(0.5, 0.3, 0.2))
            items = [(RUNGS[rung], M_IDENT)]
            if kind != "plain":
                items += [(self.pick(("p40", "empty", "torus")), int(M_GRID[i])) for i in range(int(rng.randint(2, 4)))]
        else:
            kind = self.pick(KINDS)
            if self.ext and rng.rand() < 0.5:  # (every kind of pass in front of a shade_items in several seeds)
                kind = ("list", "instanced", "plain")[(self.seed + self.m.fno + len(self.steps)) % 3]
            fed = [(b, pr) for b, pr in sorted(m.prov.items()) if pr["unit"] == "item" and pr["frame"] >= m.fno - 1 and pr["kind"] in ("list", "list_if")
                   and pr["entries"] >= pr["n"] >= 3 and all(mesh not in RUNGS.values() for mesh, _ in pr["items"])
                   and (self.q or pr["source"] == "count")]
            if fed and rng.rand() < 0.4:
                kind = "list_if"               # the counts of an earlier pass are there to be fed back
            if kind == "plain":
                items = [(self.pick(("p40", "p100", "p257", "spiky", "torus")), int(self.pick(list(M_CLIPPED) + [M_MIRROR, M_LEFT, M_IDENT])))]
            elif kind == "indexed":
                items = [("grid", int(self.pick(list(M_CLIPPED)[:4] + [M_IDENT])))]
            elif kind == "instanced":
                n = int(rng.randint(2, 6))
                ms = [int(x) for x in rng.choice(list(M_GRID) + list(M_CLIPPED), n, replace=False)]
                ms[int(rng.randint(n))] = M_MIRROR
                mesh = self.pick(("p40", "p100", "torus", "spiky"))
                items = [(mesh, mi) for mi in ms]
            else:
                if kind == "list_if" and fed and rng.rand() < 0.8:
                    b, pr = fed[int(rng.randint(len(fed)))]
                    items = list(pr["items"])
                    s.update(keep=b, keep_entries=pr["entries"], min=int(self.pick(MIN_VALUES)), fed=True)
                    if self.q:
                        s["source"] = pr["source"]
                        if pr["source"] == "boxes":      # the list that was queried; on a partition only `min 1` reads the ranks' sum as one answer
                            s.update(vs=pr["vs"], min=1)
                else:
                    n = int(rng.randint(3, 8)) if rng.rand() < 0.93 else 0
                    ms = [int(x) for x in rng.choice(list(M_GRID) + list(M_CLIPPED), n, replace=False)]
                    items = [(self.pick(SMALL + ("empty", "empty")), mi) for mi in ms]
        if kind == "list_if" and "keep" not in s:
            mask = "mask0" if rung else self.pick(sorted(MASKS), p=(0.45, 0.45, 0.1))
            s.update(keep=mask, keep_entries=8, min=int(self.pick(MIN_VALUES)) if mask == "mask1" else 1, fed=False)
        s.update(kind=kind, items=[tuple(i) for i in items], rung=rung)
        return s

    def command(self, kind, inside):
        """one target or buffer command of the given kind at this place, or None"""
        rng, m, pool = self.rng, self.m, "AB"[self.m.fno % 2]
        p = m.last if m.last is not None and not m.last.cleared else None
        if kind == "lines":
            return dict(op="lines", list=int(rng.randint(2)))
        if kind == "wireframe":
            return dict(op="wireframe", color=int(rng.randint(2))) if p else None
        if kind == "resolve":
            if not p or not p.K or (p.rastered and any(mesh in RUNGS.values() for mesh, _ in p.items)):
                return None                    # (the NumPy oracle is not run over a rung's thousands of triangles)
            return dict(op="resolve", buf=f"{pool}.v{p.K}{self.pick('ab')}")
        if kind == "shade":
            if not self.resolved:
                return None
            K = buffer_k(self.pick(self.resolved))
            written = [b for b in self.resolved if buffer_k(b) == K]
            ids = (0, NONE) if inside or not self.ranges or rng.rand() < 0.5 else self.ranges[int(rng.randint(len(self.ranges)))]
            return dict(op="shade", buf=self.pick(written), ps=self.pick(K_PS[K]), ids=tuple(int(x) for x in ids))
        if kind == "shade_items":
            # behind a raster of the pass: over the buffer the latest resolve wrote; before it (a no-op, replayed with the pass
            # where the tiny lists overflow): over any buffer of the pass's K
            if not p or not p.K or (self.m.part and p.filtered):
                return None
            bufs = [b for b in self.resolved if buffer_k(b) == p.K]
            if p.rastered and not bufs:
                return None
            buf = self.last_resolve if p.rastered and self.last_resolve in bufs and rng.rand() < 0.8 else \
                self.pick(bufs) if p.rastered else f"{pool}.v{p.K}{self.pick('ab')}"
            ps = self.pick(("PHONG", "BLINN")) if p.K == 8 and rng.rand() < 0.6 else self.pick(K_PS[p.K])
            return dict(op="shade_items", ps=ps, buf=buf, table=self.pick(sorted(MATERIALS)))
        unit = kind.split("_")[1]
        if kind.startswith("query") and (m.last is None or (m.part and m.last.filtered)):
            return None
        if unit == "item":
            if m.last is None:
                return None
            n = len(m.last.items)
        else:
            if p is None:
                return None
            n = p.base + p.emit
        e = n + int(self.pick((0, -1, 3)))
        return dict(op=kind.split("_")[0], unit=unit, buf=f"{pool}.c{int(rng.randint(3))}", entries=e) if e > 0 else None

    def place(self, kind, inside):
        """one command of the kind; a shade half the time behind a state setter it comes out differently under"""
        c = self.command(kind, inside)
        if c and c["op"] == "shade" and self.room() > (2 if inside else 1) and self.rng.rand() < 0.6:
            t = self.setter(inside)
            if t["op"] != "set_cull":
                a, b = self.probe([t, c])[0], self.probe([c])[0]
                if a is not None and b is not None and a != b:
                    self.add(t)
        return self.add_command(c)

    def kind_of_command(self):
        """shades and resolves come up more often where they can do something"""
        p = self.m.last
        commands = self.commands
        w = {k: 1.0 for k in commands}
        w["shade"] = 2.5 if self.resolved else 0.0
        w["resolve"] = 2.0 if p is not None and p.rastered and not p.cleared else 0.5
        w["shade_items"] = 2.5 if self.resolved and p is not None and p.rastered and not p.cleared else 0.0
        ws = np.array([w[k] for k in commands])
        return self.pick(commands, p=ws / ws.sum())

    def add_command(self, c):
        ok = bool(c) and self.add(c, noop_ok=c["op"] in ("resolve", "count", "query") or (c["op"] == "shade" and c["ids"][1] == 0) or
                                  (c["op"] == "shade_items" and not self.m.last.rastered))
        if ok and c["op"] == "resolve" and not c.get("noop"):
            self.last_resolve = c["buf"]
            if c["buf"] not in self.resolved:
                self.resolved.append(c["buf"])
        return ok

    # -- one pass, fused or split --
    def one_pass(self, rung):
        rng = self.rng
        for _ in range(16):
            s = self.new_pass(rung)
            # (a rung covers the screen: behind a depth-only rasterization the lines and shades inside its pass stay visible)
            ps = "DEPTH" if rung and rng.rand() < 0.6 else self.pick(("DEPTH", "FLAT") if rung == 2 else VS_PS[s["vs"]])
            draw = dict(s, op="draw", ps=ps, fused=True)
            if rung and self.m.cull != 0:
                self.add(dict(op="set_cull", mode=0), force=True)      # a rung is sized for the whole mesh
            elif not rung and self.room() >= 3 and rng.rand() < 0.6:
                t = self.setter(False)
                a, b = self.probe([t, draw])[0], self.probe([draw])[0]
                if a is not None and b is not None and a != b:
                    self.add(t)
            digest, changed = self.probe([draw])
            if digest is None or (not changed and not self.noop_allowed()):
                continue
            if not rung and self.probed.last.fan_need > ORDINARY_FAN_NEED:
                continue                       # (the rungs are sized against what an ordinary pass can need)
            if self.room() < 3 or rng.rand() < (0.2 if rung else 0.5):
                if self.add(draw, noop_ok=True):
                    return
                continue
            added = self.add(dict(s, op="geom", fused=False))
            assert added
            want = int(rng.randint(1, 4)) if rung else int(rng.randint(0, 4))
            kinds = [str(k) for k in rng.permutation(COMMANDS)]
            if rung:                            # every kind of command is the first one tried inside the rungs of some seeds
                first = COMMANDS[(self.seed + 3 * rung) % len(COMMANDS)]
                kinds.remove(first)
                kinds.append(first)
            elif self.resolved and rng.rand() < 0.6:
                kinds.remove("shade")
                kinds.append("shade")
            n = 0
            for _ in range(12):
                if n >= want or self.room() <= 1 or not kinds:
                    break
                r = rng.rand()
                if r < 0.15:
                    n += self.add(self.host_query())
                else:
                    n += self.place(kinds.pop(), True)
            added = self.add(dict(op="raster", ps=ps), force=True)
            assert added, "a geometry pass whose rasterization is refused"
            return
        raise AssertionError("no pass could be placed")

    def one_pass_x(self, rung):
        """one_pass of the extended generator.  A split pass may be abandoned (no raster: the next pass, or the frame's end,
        follows its geometry call and the commands inside it), and may be rastered twice, mostly as the pair a caller of the
        split form uses: depth only, then the same list under a shader that writes colour.  Split passes are the usual case: on
        a partitioned context everything that reads the setup list or the pass's tables needs one."""
        rng = self.rng
        for _ in range(16):
            s = self.new_pass(rung)
            ps = "DEPTH" if rung and rng.rand() < 0.5 else self.pick(("DEPTH", "FLAT") if rung == 2 else VS_PS[s["vs"]])
            draw = dict(s, op="draw", ps=ps, fused=True)
            if rung and self.m.cull != 0:
                self.add(dict(op="set_cull", mode=0), force=True)
            elif not rung and self.room() >= 3 and rng.rand() < 0.5:
                t = self.setter(False)
                a, b = self.probe([t, draw])[0], self.probe([draw])[0]
                if a is not None and b is not None and a != b:
                    self.add(t)
            digest, changed = self.probe([draw])
            if digest is None or (not changed and not self.noop_allowed()):
                continue
            if not rung and self.probed.last.fan_need > ORDINARY_FAN_NEED:
                continue
            if self.room() < 3 or rng.rand() < 0.15:
                if self.add(draw, noop_ok=True):
                    return
                continue
            added = self.add(dict(s, op="geom", fused=False))
            assert added
            # (a rung is abandoned in the seeds of one residue: with the tiny lists it overflows all the same)
            abandon = rng.rand() < (1.0 if rung == 1 and self.seed % 4 == 1 else 0.12)
            pair = not abandon and self.room() >= 4 and rng.rand() < 0.5
            want = int(rng.randint(1, 3)) if rung else int(rng.randint(0, 2))
            kinds = [str(k) for k in rng.permutation(self.commands)]
            if rng.rand() < (0.35 if self.seed % 2 else 0.0):     # (the seeds that run with the tiny lists)
                kinds.remove("shade_items")
                kinds.append("shade_items")
            if self.q and (rng.rand() < 0.6 or (rung and self.seed % 2)):
                # a query is the first command tried inside the pass: in front of a rung's raster it is what overflows the lists
                first = "query_item" if rng.rand() < 0.6 else "query_triangle"
                kinds.remove(first)
                kinds.append(first)
                want = max(want, 1)
            n = 0
            for _ in range(12):
                if n >= want or self.room() <= (3 if pair else 2) or not kinds:
                    break
                if rng.rand() < 0.15:
                    n += self.add(self.host_query())
                else:
                    n += self.place(kinds.pop(), True)
            if abandon:
                self.geom_step["abandoned"] = True
                return
            colours = [x for x in VS_PS[s["vs"]] if x != "DEPTH"] if s["items"] else ["FLAT"]
            added = self.add(dict(op="raster", ps="DEPTH" if pair else ps), force=True)
            assert added, "a geometry pass whose rasterization is refused"
            if pair or (self.room() >= 2 and rng.rand() < 0.2):
                first = "DEPTH" if pair else ps
                ps2 = ps if pair and ps != "DEPTH" else self.pick([x for x in colours + ["DEPTH"] if x != first])
                for kind in rng.permutation(("resolve", "count_item", "count_triangle", "lines"))[:int(rng.randint(0, 2))]:
                    if self.room() >= 2:
                        self.place(str(kind), True)
                self.add(dict(op="raster", ps=ps2, again=True))
            return
        raise AssertionError("no pass could be placed")

    def items_behind(self):
        """behind a pass: a resolve of it, and one shade of all its items under a table"""
        p = self.m.last
        if p.rastered and not (self.m.part and p.filtered) and p.K and p.emit and self.room() >= 2 and self.rng.rand() < (0.4 if self.q else 0.95) and \
                not any(mesh in RUNGS.values() for mesh, _ in p.items):
            self.add_command(self.command("resolve", False))
            if self.last_resolve and buffer_k(self.last_resolve) == p.K:
                self.place("shade_items", False)

    # -- the query generator's own patterns --
    def host_query(self):
        """a host query at this place; the query generator draws the host forms of the two queries and frr_drawlist_bounds too"""
        if not self.q:
            return dict(op=self.pick(HOST_QUERIES))
        op = self.pick(QUERIES, p=(0.1, 0.1, 0.15, 0.1, 0.25, 0.2, 0.1))
        if op == "query_host":
            c = self.command(self.pick(("query_item", "query_triangle")), False)
            return dict(op="query_host", unit=c["unit"], entries=c["entries"]) if c else dict(op="stats")
        if op in ("boxes_host", "bounds"):
            vs, items = self.a_list()
            s = dict(op=op, vs=vs, items=list(items))
            if op == "boxes_host":
                s["entries"] = len(items) + int(self.pick((0, -1, 3)))
                self.note_list(vs, items)
            return s
        return dict(op=op)

    def note_list(self, vs, items):
        if (vs, items) not in self.box_lists:
            self.box_lists.append((vs, items))

    def a_list(self, known=0.4):
        """(vs, items) of a list for a box query: one that was asked before, or 4 to 7 small meshes, the empty one among them,
        under any of the matrices -- behind the cover, beside it, through the near plane, off the screen"""
        rng = self.rng
        if self.box_lists and rng.rand() < known:
            return self.box_lists[int(rng.randint(len(self.box_lists)))]
        n = int(rng.randint(4, 8))
        ms = [int(x) for x in rng.choice(len(MODELS), n, replace=False)]
        items = tuple((self.pick(("p40", "p40", "torus", "grid", "p100", "spiky", "empty")), mi) for mi in ms)
        return self.pick(("PHONG", "GOURAUD")), items

    def cover_draw(self):
        vs = self.pick(("PHONG", "GOURAUD"))
        return dict(op="draw", kind="plain", vs=vs, items=[("cover", M_IDENT)], ps="DEPTH" if self.rng.rand() < 0.5 else self.pick(VS_PS[vs]), rung=0, fused=True)

    def fed_draw(self, vs, items, buf, entries, source):
        """frr_draw_list_if of the list under the keep buffer a query or a box query wrote (min_value 1)"""
        return dict(op="draw", kind="list_if", vs=vs, items=[tuple(i) for i in items], keep=buf, keep_entries=entries, min=1, fed=True, source=source,
                    ps=self.pick(VS_PS[vs]), rung=0, fused=True)

    def fits(self, vs, items):
        """the list as a pass is no rung by accident"""
        digest, _ = self.probe([dict(op="geom", kind="list", vs=vs, items=list(items), rung=0, fused=False)])
        return digest is not None and self.probed.last.fan_need <= ORDINARY_FAN_NEED

    def start_q(self, fno):
        """behind the clear: a pass decided by what the previous frame's query or box query left in its buffer; a box query as the
        first command behind the clear; a per-item query of the previous frame's pass (zeros)"""
        rng, m, pool = self.rng, self.m, "AB"[fno % 2]
        self.reserve = 4
        prev = [(b, pr) for b, pr in sorted(m.prov.items()) if pr["source"] in ("query", "boxes") and pr["frame"] == m.fno - 1 and pr["unit"] == "item"
                and pr["kind"] in ("list", "list_if") and pr["entries"] >= pr["n"] >= 3 and all(mesh not in RUNGS.values() for mesh, _ in pr["items"])]
        h = (self.seed + fno) % 4
        if h in (0, 2):
            vs, items = self.a_list()
            if self.add(dict(op="boxes", vs=vs, items=list(items), buf=f"{pool}.c{int(rng.randint(3))}", entries=len(items) + int(self.pick((0, 3)))),
                        noop_ok=True):
                self.note_list(vs, items)
        elif h == 1 and fno > 0:
            self.add_command(self.command("query_item", False))
        if prev and rng.rand() < 0.8:
            b, pr = prev[int(rng.randint(len(prev)))]
            vs = pr["vs"] if pr["source"] == "boxes" else self.pick(("PHONG", "GOURAUD"))
            if self.fits(vs, pr["items"]):
                self.add(self.fed_draw(vs, pr["items"], b, pr["entries"], pr["source"]), noop_ok=True)
        self.reserve = 0

    def loop(self, fno):
        """the loop the two queries are there for, all on one stream: occluders, the query, the pass it decides.
        boxes:      draw cover; [set_uniforms: the other camera]; boxes(list) -> buf; draw list_if(list, keep = buf)
        two boxes:  boxes(list) -> buf'; draw cover; boxes(list) -> buf; draw list_if(list, keep = buf)
        query:      draw cover; geom list; query item -> buf; [raster]; draw list_if(list, keep = buf): the list's own geometry is
                    the proxy, and the pass that asked is abandoned or rastered depth-only"""
        rng, m, pool = self.rng, self.m, "AB"[fno % 2]
        kind = ("boxes", "query", "two_boxes")[(self.seed + fno) % 3]
        if self.room() < 4:
            return
        for _ in range(6):
            vs, items = self.a_list(0.6 if kind == "boxes" and self.seed % 2 else 0.3)
            if self.fits(vs, items):
                break
        else:
            return
        n, bufs = len(items), [f"{pool}.c{int(k)}" for k in rng.permutation(3)]
        e = n + int(self.pick((0, 3)))
        if kind == "two_boxes" and self.room() >= 5:
            if self.add(dict(op="boxes", vs=vs, items=list(items), buf=bufs[1], entries=n), noop_ok=True):
                self.note_list(vs, items)
        self.add(self.cover_draw(), noop_ok=True)
        if kind == "query":
            if not self.add(dict(op="geom", kind="list", vs=vs, items=list(items), rung=0, fused=False)):
                return
            g = self.geom_step
            self.add(dict(op="query", unit="item", buf=bufs[0], entries=e), noop_ok=True)
            if not (self.room() >= 3 and rng.rand() < 0.5 and self.add(dict(op="raster", ps="DEPTH"), force=True)):
                g["abandoned"] = True
            self.add(self.fed_draw(vs, items, bufs[0], e, "query"), noop_ok=True)
            return
        cam = self.list_cam.get((vs, items))
        if kind == "boxes" and cam is not None and cam == m.cam and self.room() >= 3:
            self.add(dict(op="set_uniforms", cam=1 - m.cam, light=m.light, flat=m.flat, slot=m.slot))
        if self.add(dict(op="boxes", vs=vs, items=list(items), buf=bufs[0], entries=e), noop_ok=True):
            self.note_list(vs, items)
            self.add(self.fed_draw(vs, items, bufs[0], e, "boxes"), noop_ok=True)

    # -- one frame --
    def frame(self, fno, window, rung, end):
        rng = self.rng
        self.steps, self.ranges, self.reserve = [dict(op="clear", window=tuple(window))], [], 0
        self.m.apply(self.steps[0])
        npass = int(rng.randint(2, 5))
        at = int(rng.randint(npass)) if rung else -1
        if self.q:
            self.start_q(fno)
        if fno > 0 and rng.rand() < 0.3:       # a per-item count of the previous frame's pass right after the clear: zeros
            self.reserve = 3
            self.add_command(self.command("count_item", False))
        for k in range(npass):
            r = rung if k == at else 0
            self.reserve = 3 if rung and k <= at else 0
            if self.q and k == (self.seed + fno) % npass:
                self.loop(fno)
            self.reserve = 3 if rung and k < at else 0        # (room for the rung's pass behind this one)
            if not r and self.room() < 2:
                continue
            if self.ext:
                self.one_pass_x(r)
                if not r:
                    self.items_behind()
            else:
                self.one_pass(r)
            p = self.m.last
            if not r and p.kind in ("list", "list_if") and len(p.items) >= 3 and self.room() >= 1 and rng.rand() < 0.6:
                n = len(p.items)
                self.add_command(dict(op="count", unit="item", buf=f"{'AB'[fno % 2]}.c{int(rng.randint(3))}", entries=n + int(self.pick((0, 3)))))
            if not r and not self.resolved and self.room() >= 1 and rng.rand() < 0.7:
                self.add_command(self.command("resolve", False))
            for _ in range(int(rng.randint(1, 4))):
                if self.room() < 1:
                    break
                if rng.rand() < 0.2:
                    self.add(self.host_query())
                else:
                    self.place(self.kind_of_command(), False)
        self.reserve = 0
        self.steps.append(dict(op=end))
        self.m.apply(self.steps[-1])
        self.total += 1
        self.frames.append(self.steps)


_GENERATED = {}


def steps_of(frames):
    return [s for steps in frames for s in steps if s["op"] != "clear"]


def generate(seed, oracle=None, extended=False, queries=False):
    """The frames of a seed: a list of FRAMES lists of steps (dicts: "op" and its arguments; "noop" on a step that writes
    nothing on purpose; "rung" on a pass over a rung mesh; "fan_rung", "bin_rung", "fan_need", "bin_need" on every pass, from
    the model).  Every frame starts with its "clear" and ends with "readback" or "fenced"; the steps after the clear are at most
    MAX_STEPS.  A pure function of the seed: np.random.RandomState(seed) is the only source of randomness, and the model the
    generator consults is deterministic."""
    key = (seed, "queries") if queries else (seed, "extended") if extended else seed
    if key in _GENERATED:
        return _GENERATED[key]
    if oracle is None:
        from oracle import cref as oracle
    model_kw = dict(partitioned=True) if extended or queries else {}
    g = _Gen(oracle, seed, extended, queries)
    rng = g.rng
    f1 = int(rng.randint(0, 2))
    f2 = int(rng.randint(f1 + 1, FRAMES))
    sub = int(rng.randint(FRAMES))
    for fno in range(FRAMES):
        g.frame(fno, SUB if fno == sub else FULL, 1 if fno == f1 else 2 if fno == f2 else 0, g.pick(("readback", "fenced")))
    frames = g.frames
    # what a later step overwrote: a step whose removal changes no compared output any more leaves the sequence
    for _ in range(24):
        bad = insensitive_steps(oracle, frames, **model_kw)
        if not bad:
            break
        fi, s = bad[0]
        drop = _drop_of(frames[fi], s)
        frames = [[x for x in steps if id(x) not in drop] for steps in frames]
    # ... and the share of no-ops on purpose holds for what is left
    while True:
        flat = steps_of(frames)
        noops = [s for s in flat if s.get("noop")]
        if len(noops) <= NOOP_SHARE * len(flat):
            break
        for s in sorted(noops, key=lambda x: x["op"] in ("geom", "draw")):       # (a command before a pass)
            fi = next(k for k, steps in enumerate(frames) if any(x is s for x in steps))
            drop = _drop_of(frames[fi], s)
            fewer = [[x for x in steps if id(x) not in drop] for steps in frames]
            try:
                run_model(oracle, fewer, **model_kw)
            except (Undefined, RuntimeError):
                continue
            frames = fewer
            break
        else:
            raise AssertionError("the share of no-ops cannot be met")
    if queries:
        _settle_feeds(oracle, frames)
    _GENERATED[key] = frames
    return frames


def fed_by(oracle, frames):
    """{id(step): the model's provenance of the keep buffer at that step} for every predicated pass of `frames` that names a
    caller buffer"""
    m, out = Model(oracle, partitioned=True), {}
    for steps in frames:
        for s in steps:
            if s["op"] in ("geom", "draw") and s["kind"] == "list_if" and s["keep"] in m.bufs:
                out[id(s)] = m.prov.get(s["keep"])
            m.apply(s)
    return out


def _settle_feeds(oracle, frames):
    """after the pruning: a predicated pass whose feeding command left the sequence reads whatever the buffer holds -- it is
    marked as not fed -- and every pass that is fed says by what"""
    prov = fed_by(oracle, frames)
    for s in steps_of(frames):
        if id(s) in prov:
            pr = prov[id(s)]
            ok = pr is not None and pr["unit"] == "item" and [tuple(i) for i in pr["items"]] == [tuple(i) for i in s["items"]] and \
                pr["entries"] == s["keep_entries"] and (pr["source"] != "boxes" or pr["vs"] == s["vs"])
            s["fed"], s["source"] = bool(ok), pr["source"] if ok else None


def cull_inside_split():
    """A fixed frame for what the generator never draws: frr_set_cull between a geometry* and its rasterization.  The mode
    travels with the geometry command -- the pass that is open keeps the mode of its geometry call, through a replay too,
    and the next pass takes the new one.  With the tiny lists the first pass overflows, so its geometry is cancelled and
    replayed with the later set_cull already issued."""
    inst = [("torus", mi) for mi in (int(M_CLIPPED[0]), M_MIRROR, int(M_CLIPPED[2]), int(M_GRID[0]), int(M_CLIPPED[4]))]
    return [[dict(op="clear", window=FULL),
             dict(op="set_cull", mode=CS.NEG),
             dict(op="geom", kind="instanced", vs="PHONG", items=inst, rung=0, fused=False),
             dict(op="set_cull", mode=CS.POS),
             dict(op="count", unit="item", buf="A.c0", entries=5),
             dict(op="raster", ps="PHONG"),
             dict(op="item_ranges"),
             dict(op="geom", kind="plain", vs="GOURAUD", items=[("spiky", int(M_CLIPPED[1]))], rung=0, fused=False),
             dict(op="set_cull", mode=CS.NONE),
             dict(op="raster", ps="COLOR"),
             dict(op="stats"),
             dict(op="draw", kind="plain", vs="PHONG", items=[("torus", M_LEFT)], ps="BLINN", rung=0, fused=True),
             dict(op="readback")]]


def refused_behind_fused():
    """A fixed frame for a partitioned context: behind a fused draw*, which filtered the setup list there, every command that
    reads the setup list or the pass's tables is refused (FRR_ERR_INVALID; "refused" marks the steps) and leaves the context
    drawing; ranged shades stay allowed; behind a split pass the same commands are taken."""
    lst = [("p100", int(M_CLIPPED[0])), ("torus", int(M_GRID[1])), ("spiky", int(M_CLIPPED[3])), ("p40", int(M_GRID[4]))]
    inst = [("torus", mi) for mi in (int(M_CLIPPED[1]), M_MIRROR, int(M_GRID[2]))]
    no = dict(refused=True)
    return [[dict(op="clear", window=FULL),
             dict(op="geom", kind="instanced", vs="PHONG", items=inst, rung=0, fused=False),
             dict(op="raster", ps="DEPTH"),
             dict(op="resolve", buf="A.v8a"),
             dict(op="draw", kind="list", vs="PHONG", items=lst, ps="PHONG", rung=0, fused=True),
             dict(no, op="wireframe", color=0),
             dict(no, op="setup_triangles"),
             dict(no, op="item_ranges"),
             dict(no, op="resolve", buf="A.v8b"),
             dict(no, op="count", unit="item", buf="A.c0", entries=4),
             dict(no, op="count", unit="triangle", buf="A.c1", entries=64),
             dict(no, op="query", unit="item", buf="A.c0", entries=4),
             dict(no, op="query_host", unit="triangle", entries=64),
             dict(no, op="shade_items", ps="PHONG", buf="A.v8a", table="mat0"),
             dict(op="lines", list=0),
             dict(op="shade", buf="A.v8a", ps="BLINN", ids=(0, NONE)),
             dict(op="geom", kind="list", vs="PHONG", items=lst, rung=0, fused=False),
             dict(op="raster", ps="DEPTH"),
             dict(op="resolve", buf="A.v8b"),
             dict(op="shade_items", ps="PHONG", buf="A.v8b", table="mat1"),
             dict(op="count", unit="item", buf="A.c0", entries=4),
             dict(op="item_ranges"),
             dict(op="stats"),
             dict(op="readback")]]


def abandoned_then_larger():
    """A fixed frame: a geometry pass of one 256-input block that nothing rasters, then a pass of several blocks.  The second
    pass's ids start behind what the first emitted -- a count the library takes from the first pass's block sums, which it has
    to scan before the second pass sizes the tables (both passes use one workspace set with two frames in flight and with
    option overlap 0; seed 100 of the partitioned runs met a scan of the reallocated sums)."""
    lst = [("p257", int(M_CLIPPED[0])), ("spiky", int(M_GRID[3])), ("p257", int(M_GRID[4])), ("p100", int(M_CLIPPED[2]))]
    return [[dict(op="clear", window=FULL),
             dict(op="geom", kind="indexed", vs="GOURAUD", items=[("grid", int(M_CLIPPED[0]))], rung=0, fused=False, abandoned=True),
             dict(op="lines", list=1),
             dict(op="geom", kind="list", vs="PHONG", items=lst, rung=0, fused=False),
             dict(op="raster", ps="PHONG"),
             dict(op="item_ranges"),
             dict(op="stats"),
             dict(op="readback")]]


LOOP_LIST = [("p40", 0), ("torus", 6), ("spiky", 2), ("empty", 4), ("p40", 12), ("grid", 10), ("p100", 3)]


def query_overflows_a_rung():
    """A fixed frame: the loop of an occlusion query with the query as the command that meets the tiny lists.  The cover, the
    geometry of a list over r1 (a rung of the fan slots and of the bin records), a per-item query of it between a line list and
    a count -- the first command that bins the pass, verified inside the call --, its depth-only raster, then the geometry of
    the small list, its query, and the pass the query decides while the small list's own pass stays abandoned."""
    big = [("r1", M_IDENT), ("p40", int(M_GRID[0])), ("torus", int(M_GRID[1]))]
    return [[dict(op="clear", window=FULL),
             dict(op="draw", kind="plain", vs="PHONG", items=[("cover", M_IDENT)], ps="FLAT", rung=0, fused=True),
             dict(op="geom", kind="list", vs="PHONG", items=big, rung=1, fused=False),
             dict(op="lines", list=0),
             dict(op="query", unit="item", buf="A.c0", entries=3),
             dict(op="count", unit="item", buf="A.c1", entries=3),
             dict(op="raster", ps="DEPTH"),
             dict(op="geom", kind="list", vs="GOURAUD", items=LOOP_LIST, rung=0, fused=False, abandoned=True),
             dict(op="query", unit="item", buf="A.c2", entries=len(LOOP_LIST) + 3),
             dict(op="query_host", unit="triangle", entries=40),
             dict(op="draw", kind="list_if", vs="GOURAUD", items=LOOP_LIST, keep="A.c2", keep_entries=len(LOOP_LIST) + 3, min=1, fed=True, source="query",
                  ps="COLOR", rung=0, fused=True),
             dict(op="stats"),
             dict(op="fenced")]]


def boxes_around_a_draw():
    """Two fixed frames in the two windows: a box query as the first command behind the clear (it settles the clear, eager or
    not), the cover, the same query under the other camera, again under the first one -- the answers differ around the draw
    and around the camera --, the pass the last one decides; in the next frame, in the sub-window, the buffer decides a pass
    again before a box query of this frame replaces it, inside a split pass."""
    n = len(LOOP_LIST)
    boxes = dict(op="boxes", vs="PHONG", items=LOOP_LIST, entries=n)
    fed = dict(op="draw", kind="list_if", vs="PHONG", items=LOOP_LIST, keep_entries=n, min=1, fed=True, source="boxes", rung=0, fused=True)
    return [[dict(op="clear", window=FULL),
             dict(boxes, buf="A.c0"),
             dict(op="bounds", vs="PHONG", items=LOOP_LIST),
             dict(op="draw", kind="plain", vs="GOURAUD", items=[("cover", M_IDENT)], ps="DEPTH", rung=0, fused=True),
             dict(op="set_uniforms", cam=1, light=0, flat=0, slot=0),
             dict(boxes, buf="A.c1"),
             dict(op="set_uniforms", cam=0, light=0, flat=1, slot=0),
             dict(boxes, buf="A.c2", entries=n + 2),
             dict(op="boxes_host", vs="PHONG", items=LOOP_LIST, entries=n - 2),
             dict(fed, keep="A.c2", keep_entries=n + 2, ps="BLINN"),
             dict(op="fenced")],
            [dict(op="clear", window=SUB),
             dict(fed, keep="A.c2", keep_entries=n + 2, ps="FLAT"),
             dict(op="geom", kind="plain", vs="PHONG", items=[("cover", M_IDENT)], rung=0, fused=False),
             dict(boxes, buf="B.c0"),
             dict(op="raster", ps="PHONG"),
             dict(boxes, buf="B.c1"),
             dict(fed, keep="B.c1", ps="PHONG"),
             dict(op="readback")]]


LINE_WINDOW = (0, W, 0, 40)                    # two tile rows of the window, three of the context (line_ownership)


def line_ownership():
    """A fixed frame in a window of 40 rows: a pass, a line list over it, one shade of the pass's pixels.  The draw, the resolve
    and the shade take their owner from the window's two tile rows, the lines from the context's three."""
    return [[dict(op="clear", window=LINE_WINDOW),
             dict(op="geom", kind="plain", vs="PHONG", items=[("spiky", int(M_CLIPPED[5]))], rung=0, fused=False),
             dict(op="raster", ps="PHONG"),
             dict(op="resolve", buf="A.v8a"),
             dict(op="lines", list=0),
             dict(op="shade", buf="A.v8a", ps="FLAT", ids=(0, 20)),
             dict(op="readback")]]


def describe(s):
    """one step as a line of a failure report"""
    return s["op"] + "(" + ", ".join(f"{k}={v}" for k, v in s.items() if k not in ("op", "fan_need", "bin_need")) + ")"
