"""Host-side mirror of the reference's rasterization interface over the C ABI (include/frr.h).

Reference surface (Rust, /root/reference/f_renderer/src/renderer.rs):
  Renderer::geometry_processing(width, height, vs_inputs, vertex_shader, vs_uniform)   :96-112
  Renderer::rasterization(width_range, height_range, triangle, pixel_shader, ps_uniform,
                          frame_buffer, depth_buffer)                                  :269-284
  FrameBuffer::{new, fill, clear, get_size, get_data, set_pixel, get_pixel}            :418-514
  FrameBuffer::draw_line                                                               :540-588
and the matrix/camera helpers matrix_util.rs:3-35, camera.rs:4-26.

The per-triangle, closure-taking calls become batched calls with table-selected shaders: same
names, same argument meaning (width_range/height_range tuples, clear colours, uniforms), same
error behaviour (what panics in the reference raises FrrError(FRR_ERR_INVALID) here).
This module is plumbing only: all arithmetic of the path runs in libfrr_hip.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _native as N
from ._native import (CULL_NEG, CULL_NONE, CULL_POS, FrrError, PS_BLINN, PS_COLOR, PS_DEPTH, PS_FLAT, PS_PHONG,  # noqa: F401
                      VS_CLIP, VS_CLIP_COLOR, VS_GOURAUD, VS_PHONG)

SETUP_DTYPE = np.dtype([("spf", "<f4", (2,)), ("spi", "<i4", (2,)), ("rhw", "<f4"), ("ctx", "<f4", (N.MAX_VARYINGS,))])
assert SETUP_DTYPE.itemsize == C.sizeof(N.SetupVertex)
# frr_material as a NumPy record: a table is an array of these (Renderer.upload_materials)
MATERIAL_DTYPE = np.dtype([("texture_slot", "<i4"), ("ambient_strength", "<f4"), ("specular_strength", "<f4"), ("reserved", "<i4"),
                           ("flat_color", "<f4", (4,)), ("user", "<f4", (N.MATERIAL_USER,))])
assert MATERIAL_DTYPE.itemsize == C.sizeof(N.Material) == 64

_f32p = C.POINTER(C.c_float)


def _fp(a):
    return a.ctypes.data_as(_f32p)


# ---- matrix_util.rs / camera.rs -------------------------------------------------------------

def set_identity():
    """matrix_util.rs:3-8"""
    m = np.zeros(16, np.float32)
    N.lib().frr_set_identity(_fp(m))
    return m


def set_look_at(eye, at, up):
    """matrix_util.rs:10-22 (left-handed look-at, column-major)"""
    m = np.zeros(16, np.float32)
    e, a, u = (np.ascontiguousarray(x, np.float32) for x in (eye, at, up))
    N.lib().frr_set_look_at(_fp(e), _fp(a), _fp(u), _fp(m))
    return m


def set_perspective(fovy, aspect, zn, zf):
    """matrix_util.rs:24-35 (LH, depth 0..1, w_clip = z_view)"""
    m = np.zeros(16, np.float32)
    N.lib().frr_set_perspective(np.float32(fovy), np.float32(aspect), np.float32(zn), np.float32(zf), _fp(m))
    return m


class Camera:
    """camera.rs:4-26"""

    def __init__(self, eye, at, up):
        self.eye, self.at, self.up = (np.asarray(x, np.float32) for x in (eye, at, up))
        self.mat_look_at = set_look_at(self.eye, self.at, self.up)

    def cal_look_at(self):
        self.mat_look_at = set_look_at(self.eye, self.at, self.up)
        return self.mat_look_at


# ---- FrameBuffer ------------------------------------------------------------------------------

class FrameBuffer:
    """Host image with the reference's FrameBuffer surface (renderer.rs:411-514): RGBA8 row-major,
    offset (y*width + x)*4.  Used for textures and for what Renderer.frame_buffer() reads back."""

    def __init__(self, width, height, data=None):
        self.width, self.height = int(width), int(height)
        self.buffer = np.zeros((self.height, self.width, 4), np.uint8) if data is None else \
            np.ascontiguousarray(data, np.uint8).reshape(self.height, self.width, 4)

    @staticmethod
    def new(width, height):
        return FrameBuffer(width, height)

    def get_data(self):
        return self.buffer.reshape(-1)

    def get_size(self):
        return self.width * self.height * 4

    def clear(self):
        self.buffer[...] = 0

    def fill(self, color):
        self.buffer[...] = np.asarray(color, np.uint8)

    def set_pixel(self, x, y, color):
        self.buffer[y, x] = np.asarray(color, np.uint8)

    def get_pixel(self, x, y):
        return self.buffer[y, x].copy()

    def _set_linear(self, x, y, color):
        # set_pixel as draw_line reaches it (renderer.rs:497-503): offset (y*width + x)*4 with no test of x, so x >= width
        # lands in a later row; past the buffer the reference panics
        p = y * self.width + x
        if p >= self.width * self.height:
            raise IndexError(f"draw_line: pixel ({x}, {y}) is past the {self.width} x {self.height} buffer")
        self.buffer.reshape(-1, 4)[p] = color

    def draw_line(self, x1, y1, x2, y2, color):
        """renderer.rs:540-588, statement by statement.  The endpoints are sorted per axis, independently (a falling line
        is drawn as the rising one); vertical and horizontal lines exclude their upper end."""
        color = np.asarray(color, np.uint8)
        x1, y1, x2, y2 = int(x1), int(y1), int(x2), int(y2)
        x1, x2 = (x1, x2) if x1 < x2 else (x2, x1)
        y1, y2 = (y1, y2) if y1 < y2 else (y2, y1)
        if x1 == x2 and y1 == y2:
            self._set_linear(x1, y1, color)
        elif x1 == x2:
            for y in range(y1, y2):
                self._set_linear(x1, y, color)
        elif y1 == y2:
            for x in range(x1, x2):
                self._set_linear(x, y1, color)
        else:
            dx, dy, rem = x2 - x1, y2 - y1, 0
            if dx > dy:
                y = y1
                for x in range(x1, x2):
                    self._set_linear(x, y, color)
                    rem += dy
                    if rem >= dx:
                        y += 1
                        rem -= dx
                        self._set_linear(x, y, color)
            else:
                x = x1
                for y in range(y1, y2):
                    self._set_linear(x, y, color)
                    rem += dx
                    if rem >= dy:
                        x += 1
                        rem -= dy
                        self._set_linear(x, y, color)
            self._set_linear(x2, y2, color)


class Mesh:
    def __init__(self, renderer, mesh_id, ntris, vs_id, keepalive=None):
        self.renderer, self.id, self.ntris, self.vs_id, self._keep = renderer, mesh_id, ntris, vs_id, keepalive

    def free(self):
        if self.id is not None:
            self.renderer._check(N.lib().frr_mesh_free(self.renderer._ctx, self.id))
            self.id = None


class Lines:
    """A list of draw_line calls on the device (Renderer.upload_lines / bind_lines_device)."""

    def __init__(self, renderer, lines_id, nlines, keepalive=None):
        self.renderer, self.id, self.nlines, self._keep = renderer, lines_id, nlines, keepalive

    def free(self):
        if self.id is not None:
            self.renderer._check(N.lib().frr_lines_free(self.renderer._ctx, self.id))
            self.id = None


class Instances:
    """A table of model matrices on the device (Renderer.upload_instances / bind_instances_device): one per instance of an
    instanced pass."""

    def __init__(self, renderer, inst_id, ninst, keepalive=None):
        self.renderer, self.id, self.ninst, self._keep = renderer, inst_id, ninst, keepalive

    def free(self):
        if self.id is not None:
            self.renderer._check(N.lib().frr_instances_free(self.renderer._ctx, self.id))
            self.id = None


class Materials:
    """A table of frr_material on the device (Renderer.upload_materials / bind_materials_device): the pixel uniforms of each
    item of a pass, for Renderer.shade_items."""

    def __init__(self, renderer, mat_id, n, keepalive=None):
        self.renderer, self.id, self.n, self._keep = renderer, mat_id, n, keepalive

    def free(self):
        if self.id is not None:
            self.renderer._check(N.lib().frr_materials_free(self.renderer._ctx, self.id))
            self.id = None


class DrawList:
    """A list of (mesh, model matrix) items on the device (Renderer.upload_draw_list): a snapshot of the meshes it names."""

    def __init__(self, renderer, list_id, nitems, ntris, keepalive=None):
        self.renderer, self.id, self.nitems, self.ntris, self._keep = renderer, list_id, nitems, ntris, keepalive

    def free(self):
        if self.id is not None:
            self.renderer._check(N.lib().frr_drawlist_free(self.renderer._ctx, self.id))
            self.id = None


def host_list_item(first, ntris, t):
    """The item of a list pass that owns input t as the geometry kernels find it (frr_host_list_item): the i with
    first[i] <= t < first[i] + ntris[i], or -1."""
    f, n = np.ascontiguousarray(first, np.uint32), np.ascontiguousarray(ntris, np.uint32)
    if f.shape != n.shape or f.ndim != 1:
        raise FrrError(N.FRR_ERR_INVALID, "host_list_item: first and ntris must be 1-D and of one length")
    return int(N.lib().frr_host_list_item(f.ctypes.data, n.ctypes.data, f.size, int(t)))


def host_visible_counts(ids, width_range, height_range, bounds=None, units=None, entries=None):
    """The counts of frr_visible_pixels over a host id array, by the host build of the kernel's span logic
    (frr_host_visible_counts): `ids` uint32, entry (cy - y0) * x1 + (cx - x0).  bounds: the nitems + 1 item boundaries
    (first ids, then the end of the last) for per-item counts; None: per triangle over the ids 0 .. units.  Returns
    (counts uint32 [entries, default: the number of units], adds: the run heads that counted)."""
    a = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    b = None if bounds is None else np.ascontiguousarray(bounds, np.uint32).reshape(-1)
    if b is not None and b.size < 1:
        raise FrrError(N.FRR_ERR_INVALID, "host_visible_counts: nitems + 1 boundaries")
    n = b.size - 1 if b is not None else int(units)
    out = np.empty(n if entries is None else int(entries), np.uint32)
    adds = N.lib().frr_host_visible_counts(a.ctypes.data, a.size, int(width_range[0]), int(width_range[1]), int(height_range[0]), int(height_range[1]),
                                           None if b is None else b.ctypes.data, n, out.ctypes.data if out.size else None, out.size)
    if adds < 0:
        raise FrrError(N.FRR_ERR_INVALID, "host_visible_counts: bad window, array or boundaries")
    return out, int(adds)


def host_entry_items(ids, width_range, height_range, bounds):
    """The item of every entry of a host id array as frr_shade_items' kernel finds it (frr_host_entry_items): `ids` uint32,
    entry (cy - y0) * x1 + (cx - x0); bounds: the nitems + 1 item boundaries.  Returns (items uint32, shaped like ids.reshape(-1):
    the item, 0xFFFFFFFF where the id is not one of the pass's or the entry lies outside the window; rounds: the number of
    (64-entry span, distinct item) pairs, what the kernel's loop over a span's items runs)."""
    a = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    b = np.ascontiguousarray(bounds, np.uint32).reshape(-1)
    if b.size < 1:
        raise FrrError(N.FRR_ERR_INVALID, "host_entry_items: nitems + 1 boundaries")
    out = np.full(a.size, 0xFFFFFFFF, np.uint32)
    rounds = N.lib().frr_host_entry_items(a.ctypes.data, a.size, int(width_range[0]), int(width_range[1]), int(height_range[0]), int(height_range[1]),
                                          b.ctypes.data, b.size - 1, out.ctypes.data if out.size else None)
    if rounds < 0:
        raise FrrError(N.FRR_ERR_INVALID, "host_entry_items: bad window, array or boundaries")
    return out, int(rounds)


BOX_NONE, BOX_OUTSIDE, BOX_HIDDEN, BOX_KEPT, BOX_UNBOUNDED = 0, 1, 2, 3, 4   # status of frr_host_query_boxes (frr_boxes.h: BoxStatus)


def host_query_boxes(mvps, lo_hi, flags, size, window, depth, row_owned=None, entries=None):
    """The whole rule of frr_query_boxes over host arrays, by the host build of the header the kernels compile
    (frr_host_query_boxes): mvps float32 [n, 16], lo_hi float32 [n, 6], flags uint32 [n]; size = (W, H), the viewport;
    window = (x0, x1, y0, y1); depth float32, entry (cy - y0) * x1 + (cx - x0); row_owned: None, or one byte per
    window-local tile row.  Returns (out uint32 [entries, default n], status_rect_level int32 [n, 6])."""
    m = np.ascontiguousarray(mvps, np.float32).reshape(-1, 16)
    b = np.ascontiguousarray(lo_hi, np.float32).reshape(-1, 6)
    f = np.ascontiguousarray(flags, np.uint32).reshape(-1)
    d = np.ascontiguousarray(depth, np.float32).reshape(-1)
    n = f.size
    if m.shape[0] != n or b.shape[0] != n:
        raise FrrError(N.FRR_ERR_INVALID, "host_query_boxes: one matrix, one box and one flag word per item")
    ro = None if row_owned is None else np.ascontiguousarray(row_owned, np.uint8).reshape(-1)
    x0, x1, y0, y1 = (int(v) for v in window)
    if ro is not None and ro.size < (max(y1 - y0, 0) + 31) // 32:
        raise FrrError(N.FRR_ERR_INVALID, "host_query_boxes: one row_owned byte per tile row of the window")
    out = np.full(n if entries is None else int(entries), 0xDEADBEEF, np.uint32)
    srl = np.zeros((n, 6), np.int32)
    rc = N.lib().frr_host_query_boxes(m.ctypes.data if n else None, b.ctypes.data if n else None, f.ctypes.data if n else None, n, int(size[0]), int(size[1]),
                                      x0, x1, y0, y1, d.ctypes.data, d.size, None if ro is None else ro.ctypes.data,
                                      out.ctypes.data if out.size else None, out.size, srl.ctypes.data if n else None)
    if rc < 0:
        raise FrrError(N.FRR_ERR_INVALID, "host_query_boxes: bad window or arrays")
    return out, srl


def host_instance_mvp(proj, view, model):
    """(proj * view) * model as the device computes it per instance (frr_host_instance_mvp): float32 [16], column-major."""
    p, v, m = (np.ascontiguousarray(x, np.float32).reshape(16) for x in (proj, view, model))
    out = np.zeros(16, np.float32)
    N.lib().frr_host_instance_mvp(_fp(p), _fp(v), _fp(m), _fp(out))
    return out


def host_cull_det(clip):
    """The facing determinant of three clip positions (float32 [3][4]: x, y, z, w) as the geometry kernels compute it
    (frr_host_cull_det): CULL_NEG drops an input whose value is < 0, CULL_POS one whose value is > 0."""
    p = np.ascontiguousarray(clip, np.float32).reshape(12)
    return np.float32(N.lib().frr_host_cull_det(_fp(p)))


def _options_from_env():
    """The test-suite and the tools select code paths with FRR_* environment variables; the library reads none, so they
    are translated into frr_set_option calls here (every new Renderer)."""
    import os
    e, o = os.environ, {}
    if e.get("FRR_RASTER") == "sweep":
        o["raster_sweep"] = 1
    for var, name in (("FRR_RASTER_NW", "raster_nw"), ("FRR_RASTER_OCC", "raster_occ"), ("FRR_BIN_G", "bin_chunks"),
                      ("FRR_ENT_SLOT", "tile_slot_records"), ("FRR_BIN_CAP", "bin_capacity"), ("FRR_FAN_CAP", "fan_capacity"),
                      ("FRR_CLIP_QUEUE", "clip_queue"), ("FRR_OVERLAP", "overlap"), ("FRR_FRAMES_IN_FLIGHT", "frames_in_flight"),
                      ("FRR_BOUND_IN_FLIGHT", "bound_targets_in_flight"), ("FRR_TILE_ORDER", "tile_order")):
        if e.get(var):
            o[name] = int(e[var])
    if e.get("FRR_CLEAR") == "eager":
        o["clear_eager"] = 1
    if e.get("FRR_BIN") == "atomics":
        o["bin_atomics"] = 1
    return o


class Renderer:
    """Device-resident FrameBuffer (width x height RGBA8) + f32 depth buffer + u32 triangle-id
    buffer, and the two halves of the reference's draw loop (phong.rs:319-381) as batched calls."""

    def __init__(self, width, height, device=0, stream=None):
        self._lib = N.lib()
        self.width, self.height = int(width), int(height)
        ctx = C.c_void_p()
        rc = self._lib.frr_create(int(device), self.width, self.height, C.c_void_p(stream or 0), C.byref(ctx))
        if rc != N.FRR_OK:
            raise FrrError(rc, "frr_create failed (no gfx950 device, bad size, or out of memory); "
                               "there is no CPU fallback")
        self._ctx = ctx
        self.uniforms = N.Uniforms()
        ident = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
        self.uniforms.model[:] = ident
        self.uniforms.view[:] = ident
        self.uniforms.proj[:] = ident
        self.uniforms.light_pos[:] = [float(np.float32(1.2)), 1.0, 2.0]
        self.uniforms.light_color[:] = [1.0, 1.0, 1.0]
        self.uniforms.ambient_strength = float(np.float32(0.1))
        self.uniforms.specular_strength = 0.5
        self.uniforms.flat_color[:] = [1.0, 1.0, 1.0, 1.0]
        self._keep = []
        self.last_warning = None
        for name, value in _options_from_env().items():
            self.set_option(name, value)

    def tile_order_passes(self):
        """Raster passes so far whose tile kernel took a built tile order (option tile_order; tests)."""
        n = C.c_uint64()
        self._check(self._lib.frr_tile_order_passes(self._ctx, C.byref(n)))
        return int(n.value)

    def set_option(self, name, value):
        """Development / test switches of the library (include/frr.h: frr_set_option); none changes a result."""
        self._check(self._lib.frr_set_option(self._ctx, name.encode(), int(value)))

    # -- lifetime / errors --
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.frr_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        """Negative status: raise.  Positive status (a warning; none is defined at present): the call delivered its results; remembered in
        `last_warning` (None when the latest checked call had nothing to report)."""
        if rc < N.FRR_OK:
            raise FrrError(rc, self._lib.frr_last_error(self._ctx).decode())
        self.last_warning = rc if rc > N.FRR_OK else None

    # -- scene --
    def upload_mesh(self, vs_inputs, vs_id):
        """Vec<[VSInput;3]> (phong.rs:187-205) -> device.  vs_inputs: float32 [ntris,3,NF]."""
        nf = self._lib.frr_vs_input_floats(vs_id)
        if nf < 0:
            raise FrrError(N.FRR_ERR_INVALID, "unknown vertex shader id")
        a = np.ascontiguousarray(vs_inputs, np.float32)
        if a.size % (3 * nf):
            raise FrrError(N.FRR_ERR_INVALID, "vs_inputs size is not a multiple of 3*floats_per_vertex")
        ntris = a.size // (3 * nf)
        mid = C.c_int()
        self._check(self._lib.frr_mesh_upload(self._ctx, a.ctypes.data, ntris, vs_id, C.byref(mid)))
        return Mesh(self, mid.value, ntris, vs_id)

    def bind_mesh_device(self, dev_ptr, ntris, vs_id, keepalive=None):
        """Same, for data already in HBM (e.g. a torch tensor's data_ptr())."""
        mid = C.c_int()
        self._check(self._lib.frr_mesh_bind_device(self._ctx, C.c_void_p(dev_ptr), ntris, vs_id, C.byref(mid)))
        return Mesh(self, mid.value, ntris, vs_id, keepalive)

    def upload_mesh_indexed(self, vertices, indices, vs_id):
        """The Model itself instead of its expansion (phong.rs:187-205): vertices float32 [V,NF], indices uint32 [F,3];
        corner j of triangle t is vertices[indices[t, j]].  Draws exactly as upload_mesh(vertices[indices]) does.
        An index >= V (the reference's out-of-bounds panic) raises FrrError(FRR_ERR_INVALID)."""
        nf = self._lib.frr_vs_input_floats(vs_id)
        if nf < 0:
            raise FrrError(N.FRR_ERR_INVALID, "unknown vertex shader id")
        v = np.ascontiguousarray(vertices, np.float32)
        i = np.ascontiguousarray(indices, np.uint32)
        if v.size % nf or i.size % 3:
            raise FrrError(N.FRR_ERR_INVALID, "vertices / indices size is not a multiple of floats_per_vertex / 3")
        ntris = i.size // 3
        mid = C.c_int()
        self._check(self._lib.frr_mesh_upload_indexed(self._ctx, v.ctypes.data, v.size // nf, i.ctypes.data, ntris, vs_id, C.byref(mid)))
        return Mesh(self, mid.value, ntris, vs_id)

    def bind_mesh_device_indexed(self, vert_ptr, nverts, idx_ptr, ntris, vs_id, keepalive=None):
        """Same, for a vertex array (float32 [nverts,NF]) and an index list (uint32 [ntris,3]) already in HBM, e.g. two
        torch tensors' data_ptr().  The indices are validated on the device inside this call (a host wait).  After an
        in-place rewrite of either buffer: frame_fence, rewrite, bind again (which validates again)."""
        mid = C.c_int()
        self._check(self._lib.frr_mesh_bind_device_indexed(self._ctx, C.c_void_p(vert_ptr), nverts, C.c_void_p(idx_ptr), ntris, vs_id, C.byref(mid)))
        return Mesh(self, mid.value, ntris, vs_id, keepalive)

    def upload_instances(self, models):
        """The model matrices of the objects that share a mesh (phong.rs:319-331: vs_uniform.model per object) -> device.
        models: float32 [ninst, 16] (or [ninst, 4, 4] in memory order), column-major like uniforms.model."""
        a = np.ascontiguousarray(models, np.float32)
        if a.size % 16:
            raise FrrError(N.FRR_ERR_INVALID, "models size is not a multiple of 16")
        iid = C.c_int()
        self._check(self._lib.frr_instances_upload(self._ctx, a.ctypes.data if a.size else None, a.size // 16, C.byref(iid)))
        return Instances(self, iid.value, a.size // 16)

    def bind_instances_device(self, ptr, ninst, keepalive=None):
        """Same, for a table already in HBM (float32 [ninst,16], 16-byte aligned, e.g. a torch tensor's data_ptr()).  After an
        in-place rewrite: frame_fence, rewrite, bind again."""
        iid = C.c_int()
        self._check(self._lib.frr_instances_bind_device(self._ctx, C.c_void_p(ptr), ninst, C.byref(iid)))
        return Instances(self, iid.value, ninst, keepalive)

    def upload_materials(self, materials):
        """One frr_material per item of a pass -> device (frr_materials_upload).  materials: an array of MATERIAL_DTYPE, or a
        sequence of dicts with any of texture_slot, ambient_strength, specular_strength, flat_color, user (up to
        MATERIAL_USER floats), reserved; what a dict leaves out is 0 (flat_color: 1, 1, 1, 1)."""
        if isinstance(materials, np.ndarray) and materials.dtype == MATERIAL_DTYPE:
            a = np.ascontiguousarray(materials).reshape(-1)
        else:
            a = np.zeros(len(materials), MATERIAL_DTYPE)
            a["flat_color"] = 1.0
            for i, m in enumerate(materials):
                for k, v in m.items():
                    if k == "user":
                        v = np.asarray(v, np.float32).reshape(-1)
                        if v.size > N.MATERIAL_USER:
                            raise FrrError(N.FRR_ERR_INVALID, "a material takes at most MATERIAL_USER user floats")
                        a["user"][i, :v.size] = v
                    else:
                        a[k][i] = v
        mid = C.c_int()
        self._check(self._lib.frr_materials_upload(self._ctx, a.ctypes.data if a.size else None, a.size, C.byref(mid)))
        return Materials(self, mid.value, int(a.size))

    def bind_materials_device(self, ptr, n, keepalive=None):
        """Same, for a table already in HBM (n records of MATERIAL_DTYPE, 16-byte aligned, e.g. a torch tensor's data_ptr());
        checked on the device inside this call (a host wait).  After an in-place rewrite: frame_fence, rewrite, bind again."""
        mid = C.c_int()
        self._check(self._lib.frr_materials_bind_device(self._ctx, C.c_void_p(ptr), int(n), C.byref(mid)))
        return Materials(self, mid.value, int(n), keepalive)

    def upload_lines(self, xyxy, rgba):
        """A list of FrameBuffer::draw_line calls (renderer.rs:540-588) -> device.  xyxy: uint32 [n,4] = x1, y1, x2, y2;
        rgba: uint8 [n,4], or one colour for all.  A segment that would panic in the reference (its walk leaves the
        buffer) raises FrrError(FRR_ERR_INVALID) naming it, and nothing is uploaded."""
        a = np.ascontiguousarray(xyxy, np.uint32).reshape(-1, 4)
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(rgba, np.uint8).reshape(-1, 4), (a.shape[0], 4)))
        lid = C.c_int()
        self._check(self._lib.frr_lines_upload(self._ctx, a.ctypes.data, c.ctypes.data, a.shape[0], C.byref(lid)))
        return Lines(self, lid.value, a.shape[0])

    def bind_lines_device(self, xyxy_ptr, rgba_ptr, nlines, keepalive=None):
        """Same, for a list already in HBM (uint32 [n,4] and uint8 [n,4], e.g. two torch tensors' data_ptr()); validated on
        the device inside this call (a host wait).  After an in-place rewrite: frame_fence, rewrite, bind again."""
        lid = C.c_int()
        self._check(self._lib.frr_lines_bind_device(self._ctx, C.c_void_p(xyxy_ptr), C.c_void_p(rgba_ptr), nlines, C.byref(lid)))
        return Lines(self, lid.value, nlines, keepalive)

    def set_texture(self, slot, image):
        """PSUniform.sample_2d_* (phong.rs:43-45): FrameBuffer or uint8 [h,w,4]."""
        buf = image.buffer if isinstance(image, FrameBuffer) else np.ascontiguousarray(image, np.uint8)
        h, w = buf.shape[0], buf.shape[1]
        self._check(self._lib.frr_texture_upload(self._ctx, slot, buf.ctypes.data, w, h))

    def set_uniforms(self, model=None, view=None, proj=None, view_pos=None, light_pos=None, light_color=None,
                     ambient_strength=None, specular_strength=None, flat_color=None, texture_slot=None):
        u = self.uniforms
        for name, v in (("model", model), ("view", view), ("proj", proj), ("view_pos", view_pos),
                        ("light_pos", light_pos), ("light_color", light_color), ("flat_color", flat_color)):
            if v is not None:
                getattr(u, name)[:] = [float(x) for x in np.asarray(v, np.float32).reshape(-1)]
        if ambient_strength is not None:
            u.ambient_strength = float(np.float32(ambient_strength))
        if specular_strength is not None:
            u.specular_strength = float(np.float32(specular_strength))
        if texture_slot is not None:
            u.texture_slot = int(texture_slot)
        self._check(self._lib.frr_set_uniforms(self._ctx, C.byref(u)))

    def register_shader(self, hip_source, vs_input_floats, num_varyings):
        """The reference's closure API (renderer.rs:105,283) as text: HIP source defining frr_user_vs / frr_user_ps
        (include/frr.h: user shaders), compiled at run time into the library's kernels.  Returns the shader id to pass as
        vs_id to upload_mesh and as pixel_shader to rasterization / draw."""
        sid = C.c_int()
        self._check(self._lib.frr_shader_register(self._ctx, hip_source.encode(), int(vs_input_floats), int(num_varyings), C.byref(sid)))
        return sid.value

    def set_user_uniforms(self, values):
        """u.user[...] of the user shaders: what the reference's closures would have captured."""
        v = np.ascontiguousarray(values, np.float32).reshape(-1)
        self._check(self._lib.frr_set_user_uniforms(self._ctx, _fp(v), v.size))

    def set_cull(self, mode):
        """Face culling of the geometry passes issued from now on (frr_set_cull): CULL_NONE, CULL_NEG (drop inputs whose
        clip-space determinant is < 0) or CULL_POS (> 0).  A culled pass is the plain pass over the inputs it keeps."""
        self._check(self._lib.frr_set_cull(self._ctx, int(mode)))

    def set_partition(self, rank, world, blocked=False):
        """Tile-row ownership of a multi-GPU rank: interleaved rows (ty % world == rank) or, blocked=True,
        a contiguous run of tile_rows // world rows (the first tile_rows % world ranks one more)."""
        self._check(self._lib.frr_set_partition(self._ctx, rank, world))
        self._check(self._lib.frr_set_partition_layout(self._ctx, 1 if blocked else 0))

    def owned_rows(self, height_range=None):
        """Bands [row0, row1) of window-local pixel rows this rank owns (frr_owned_rows): what the final-image
        gather of a multi-GPU run sends."""
        y0, y1 = height_range or (0, self.height)
        n = self._lib.frr_owned_band_count(self._ctx, y0, y1)
        if n < 0:
            raise FrrError(n, "frr_owned_band_count")
        out = []
        for b in range(n):
            a, e = C.c_int32(), C.c_int32()
            self._check(self._lib.frr_owned_rows(self._ctx, y0, y1, b, C.byref(a), C.byref(e)))
            out.append((a.value, e.value))
        return out

    def set_count_fragments(self, enable):
        self._check(self._lib.frr_set_count_fragments(self._ctx, 1 if enable else 0))

    def bind_targets(self, color_ptr=None, depth_ptr=None, tri_id_ptr=None):
        self._check(self._lib.frr_bind_targets(self._ctx, C.c_void_p(color_ptr or 0), C.c_void_p(depth_ptr or 0),
                                               C.c_void_p(tri_id_ptr or 0)))

    def target_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._lib.frr_target_ptrs(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # -- frame --
    def clear(self, color=(30, 30, 30, 255), depth=0.0):
        """frame_buffer.fill(color); depth_buffer.fill(depth)  (phong.rs:316-317)"""
        c = np.asarray(color, np.uint8)
        self._check(self._lib.frr_clear(self._ctx, c.ctypes.data, np.float32(depth)))

    def geometry_processing(self, mesh, count=False):
        """Loop A (phong.rs:321-331): Renderer::geometry_processing over all triangles of mesh."""
        n = C.c_uint64()
        self._check(self._lib.frr_geometry(self._ctx, mesh.id, C.byref(n) if count else None))
        return int(n.value) if count else None

    def rasterization(self, width_range, height_range, pixel_shader):
        """Loop B (phong.rs:361-381): Renderer::rasterization of the last geometry_processing."""
        self._check(self._lib.frr_raster(self._ctx, pixel_shader, int(width_range[0]), int(width_range[1]),
                                         int(height_range[0]), int(height_range[1])))

    def draw(self, mesh, pixel_shader, width_range=None, height_range=None):
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        self._check(self._lib.frr_draw(self._ctx, mesh.id, pixel_shader, wr[0], wr[1], hr[0], hr[1]))

    def geometry_processing_instanced(self, mesh, instances, count=False):
        """Loop A under every matrix of the table in turn (phong.rs:319-331: the loop over objects around it), into ONE setup
        list in (instance, triangle) order (frr_geometry_instanced)."""
        n = C.c_uint64()
        self._check(self._lib.frr_geometry_instanced(self._ctx, mesh.id, instances.id, C.byref(n) if count else None))
        return int(n.value) if count else None

    def draw_instanced(self, mesh, instances, pixel_shader, width_range=None, height_range=None):
        """geometry_processing_instanced + rasterization: what one draw(mesh) per matrix with set_uniforms(model=...) in
        between gives, bit for bit, in one pass (frr_draw_instanced)."""
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        self._check(self._lib.frr_draw_instanced(self._ctx, mesh.id, instances.id, pixel_shader, wr[0], wr[1], hr[0], hr[1]))

    def upload_draw_list(self, meshes, models, reserved=0):
        """(mesh, model matrix) items -> device (frr_drawlist_upload): meshes, a sequence of Mesh; models, float32
        [nitems, 16] (or [nitems, 4, 4] in memory order), column-major like uniforms.model.  The list is a snapshot: freeing
        a mesh it names kills it."""
        a = np.ascontiguousarray(models, np.float32).reshape(-1)
        if a.size != 16 * len(meshes):
            raise FrrError(N.FRR_ERR_INVALID, "one 4x4 model matrix per mesh")
        items = (N.DrawItem * max(len(meshes), 1))()
        for i, m in enumerate(meshes):
            items[i].mesh, items[i].reserved = -1 if m.id is None else m.id, reserved
            items[i].model[:] = a[16 * i:16 * i + 16].tolist()
        lid = C.c_int()
        self._check(self._lib.frr_drawlist_upload(self._ctx, C.cast(items, C.c_void_p) if meshes else None, len(meshes), C.byref(lid)))
        return DrawList(self, lid.value, len(meshes), sum(m.ntris for m in meshes), keepalive=list(meshes))

    def free_draw_list(self, draw_list):
        draw_list.free()

    def geometry_list(self, draw_list, count=False):
        """Loop A over every item's mesh under that item's model matrix, into ONE setup list in (item, triangle) order: the
        whole setup loop of phong.rs:319-359 (frr_geometry_list)."""
        n = C.c_uint64()
        self._check(self._lib.frr_geometry_list(self._ctx, draw_list.id, C.byref(n) if count else None))
        return int(n.value) if count else None

    def draw_list(self, draw_list, pixel_shader, width_range=None, height_range=None):
        """geometry_list + rasterization: what one set_uniforms(model=...) + draw(mesh) per item gives, bit for bit, in one
        pass (frr_draw_list)."""
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        self._check(self._lib.frr_draw_list(self._ctx, draw_list.id, pixel_shader, wr[0], wr[1], hr[0], hr[1]))

    def geometry_list_if(self, draw_list, keep_ptr, entries, min_value=1, count=False):
        """geometry_list with every item i whose keep[i] < min_value (unsigned) replaced by an empty mesh
        (frr_geometry_list_if).  keep_ptr: device memory, one uint32 per item, `entries` of them -- what
        visible_pixels("item", out_ptr=...) wrote, or a 0/1 mask of a 32-bit integer torch tensor.  The buffer is read on the
        library's streams behind every earlier command of this renderer and behind pending frame_wait streams; it has to
        stay as it is until the next sync() or clear()."""
        n = C.c_uint64()
        self._check(self._lib.frr_geometry_list_if(self._ctx, draw_list.id, keep_ptr, entries, min_value, C.byref(n) if count else None))
        return int(n.value) if count else None

    def draw_list_if(self, draw_list, keep_ptr, entries, pixel_shader, min_value=1, width_range=None, height_range=None):
        """geometry_list_if + rasterization: draw_list of the same list without the dropped items, bit for bit; the items keep
        their numbers (item_ranges, visible_pixels("item")), a dropped one with nothing in it (frr_draw_list_if)."""
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        self._check(self._lib.frr_draw_list_if(self._ctx, draw_list.id, keep_ptr, entries, min_value, pixel_shader, wr[0], wr[1], hr[0], hr[1]))

    def list_bounds(self, draw_list):
        """(lo_hi float32 [nitems, 6], flags uint32 [nitems]): per item of the list the object-space box of the positions
        its mesh's triangles name -- lo xyz, hi xyz -- and flags, bit 0: a position is NaN or infinite, bit 1: the mesh has no
        triangles (frr_drawlist_bounds; computed on the device, a synchronisation point).  The table stays with the list:
        query_boxes needs it."""
        n = C.c_uint64()
        lo_hi, flags = np.zeros((draw_list.nitems, 6), np.float32), np.zeros(draw_list.nitems, np.uint32)
        self._check(self._lib.frr_drawlist_bounds(self._ctx, -1 if draw_list.id is None else draw_list.id, lo_hi.ctypes.data if lo_hi.size else None,
                                                  flags.ctypes.data if flags.size else None, draw_list.nitems, C.byref(n)))
        return lo_hi, flags

    def query_boxes(self, draw_list, out_ptr=None, entries=None, window=None):
        """The box query (frr_query_boxes): per item of the list 0 where the item's box, under the item's matrix and the
        current view and projection, lies behind the depth target as it stands or outside window = (x0, x1, y0, y1)
        (default: the frame) -- drawing the item now would change nothing -- else an upper bound of the pixels it can own.
        Conservative, not exact; needs list_bounds(draw_list) first.  With `out_ptr` (device memory of `entries` uint32) it
        is a command on the frame's stream with no host wait and returns nothing: the buffer is a keep buffer for
        draw_list_if as it is.  Without `out_ptr` it is the host form (a synchronisation point) and returns a uint32 array
        of the list's items, or of `entries` of them."""
        win = tuple(int(v) for v in (window or (0, self.width, 0, self.height)))
        lid = -1 if draw_list.id is None else draw_list.id
        if out_ptr is not None:
            if entries is None:
                raise FrrError(N.FRR_ERR_INVALID, "query_boxes: the device form needs the buffer's entries")
            self._check(self._lib.frr_query_boxes(self._ctx, lid, *win, C.c_void_p(out_ptr), int(entries)))
            return None
        out = np.zeros(draw_list.nitems if entries is None else int(entries), np.uint32)
        n = C.c_uint64()
        self._check(self._lib.frr_query_boxes_host(self._ctx, lid, *win, out.ctypes.data if out.size else None, out.size, C.byref(n)))
        return out

    def item_ranges(self, cap=None):
        """(first, count), uint32 arrays: per item of the latest geometry pass -- the items of a list pass, the instances of
        an instanced pass, one item for a plain pass -- the triangle id of its first setup triangle and how many it emitted
        (frr_geometry_item_ranges; a synchronisation point).  cap: at most that many entries."""
        n = C.c_uint64()
        self._check(self._lib.frr_geometry_item_ranges(self._ctx, None, None, 0, C.byref(n)))
        w = int(n.value) if cap is None else min(int(cap), int(n.value))
        first, count = np.zeros(w, np.uint32), np.zeros(w, np.uint32)
        if w:
            self._check(self._lib.frr_geometry_item_ranges(self._ctx, first.ctypes.data, count.ctypes.data, w, C.byref(n)))
        return first, count

    def draw_lines(self, lines):
        """for each segment of the list, in order: frame_buffer.draw_line(x1, y1, x2, y2, color) on the colour target (depth
        and triangle ids untouched), ordered with the draws around it like any of them."""
        self._check(self._lib.frr_draw_lines(self._ctx, lines.id))

    def draw_wireframe(self, color):
        """The three edges of every triangle of the last geometry_processing (between their spi), one colour; an edge with
        an endpoint off the screen is skipped whole.  No read-back, no host wait."""
        c = np.ascontiguousarray(color, np.uint8).reshape(4)
        self._check(self._lib.frr_draw_wireframe(self._ctx, c.ctypes.data))

    def resolve_varyings(self, out_ptr, entries, width_range=None, height_range=None):
        """The pixel shader's input (renderer.rs:368-378) of every pixel of the window that a triangle of the last
        geometry_processing owns, into device memory: float32 [entries][K] at `out_ptr` (e.g. a torch tensor's data_ptr()),
        entry (cy - y0) * x1 + (cx - x0); every other entry is left untouched.  No host wait: order the reads with
        frame_fence(stream) or sync() (frr_resolve_varyings).  `stream` has to be a created stream (torch.cuda.Stream()):
        handle 0 -- torch's default stream -- means the renderer's own stream to frame_fence and fences nothing for the caller."""
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        self._check(self._lib.frr_resolve_varyings(self._ctx, int(wr[0]), int(wr[1]), int(hr[0]), int(hr[1]), C.c_void_p(out_ptr or 0), int(entries)))

    def readback_varyings(self, width_range=None, height_range=None, fill=np.nan):
        """The same on the host: float32 [(y1 - y0) * x1, K], `fill` (a scalar, or an array of that shape) where no triangle
        of the last geometry_processing owns the entry (frr_readback_varyings)."""
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        k = self._lib.frr_geometry_num_varyings(self._ctx)   # the library's own K: the copy-back can never pass the array
        if k < 0:
            raise FrrError(N.FRR_ERR_INVALID, "readback_varyings before geometry_processing")
        entries = max(int(hr[1]) - int(hr[0]), 0) * max(int(wr[1]), 0)
        out = np.empty((entries, k), np.float32)
        out[...] = fill
        buf = out if out.size else np.zeros(1, np.float32)   # (nothing to write: the call still checks its arguments)
        self._check(self._lib.frr_readback_varyings(self._ctx, int(wr[0]), int(wr[1]), int(hr[0]), int(hr[1]), buf.ctypes.data, entries))
        return out

    def geometry_num_varyings(self):
        """K of the last geometry_processing / draw: what sizes the buffers of resolve_varyings and shade_varyings."""
        k = self._lib.frr_geometry_num_varyings(self._ctx)
        if k < 0:
            raise FrrError(N.FRR_ERR_INVALID, "geometry_num_varyings before geometry_processing")
        return k

    def _varyings_in(self, who, buf, entries, K, wr, hr):
        """The buffer argument of shade_varyings / shade_items: (host array?, pointer, entries, K, what keeps the pointer alive).
        A NumPy array goes to the host entry point; entries defaults to (y1 - y0) * x1 (or the array's rows), K to the array's
        columns, else to geometry_num_varyings()."""
        window = max(int(hr[1]) - int(hr[0]), 0) * max(int(wr[1]), 0)
        if isinstance(buf, np.ndarray):
            a = np.ascontiguousarray(buf, np.float32)
            if K is None:
                K = a.shape[-1] if a.ndim >= 2 else self.geometry_num_varyings()
            if entries is None:
                entries = a.size // K if K else window
            if a.size < min(int(entries) * int(K), window * int(K)):
                raise FrrError(N.FRR_ERR_INVALID, who + ": the array is smaller than entries * K")
            return True, (a.ctypes.data if a.size else 0), entries, K, a
        if K is None:
            K = self.geometry_num_varyings()
        return False, int(buf or 0), window if entries is None else entries, K, None

    def shade_varyings(self, pixel_shader, buf, entries=None, K=None, width_range=None, height_range=None, ids=(0, 0xFFFFFFFF)):
        """pixel_shader over a buffer of varyings into the colour target (frr_shade_varyings): every pixel of the window whose
        triangle id lies in ids = (first, count) -- id != 0xFFFFFFFF and id - first < count -- becomes
        vec4_to_u8_array(pixel_shader(uniforms, buf[i])), i = (cy - y0) * x1 + (cx - x0); every other pixel, depth, ids and
        stats() are untouched.  `buf`: a device pointer to float32 [entries][K] (e.g. a torch tensor's data_ptr(); it stays
        allocated and unchanged until sync() or the next clear(); no host wait), or a NumPy array [entries, K], which is
        copied to the device inside the call (frr_shade_varyings_host).  entries defaults to (y1 - y0) * x1 (or the
        array's rows), K to the array's columns, else to geometry_num_varyings().  The uniforms are those of the call."""
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        host, ptr, entries, K, _keep = self._varyings_in("shade_varyings", buf, entries, K, wr, hr)
        fn = self._lib.frr_shade_varyings_host if host else self._lib.frr_shade_varyings
        self._check(fn(self._ctx, int(pixel_shader), int(wr[0]), int(wr[1]), int(hr[0]), int(hr[1]), C.c_void_p(ptr), int(entries), int(K),
                       int(ids[0]) & 0xFFFFFFFF, int(ids[1]) & 0xFFFFFFFF))

    def shade_items(self, pixel_shader, buf, materials, entries=None, K=None, width_range=None, height_range=None):
        """shade_varyings for all items of the latest geometry pass at once, each under its own material (frr_shade_items):
        what `for k: set the uniforms' texture_slot / strengths / flat_color / user[:8] from materials[k];
        shade_varyings(..., ids=(first[k], count[k]))` over item_ranges() leaves, byte for byte, in one pass over the window.
        `buf`, entries and K as for shade_varyings; everything else in the uniforms is the call's."""
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        host, ptr, entries, K, _keep = self._varyings_in("shade_items", buf, entries, K, wr, hr)
        fn = self._lib.frr_shade_items_host if host else self._lib.frr_shade_items
        self._check(fn(self._ctx, int(pixel_shader), int(wr[0]), int(wr[1]), int(hr[0]), int(hr[1]), C.c_void_p(ptr), int(entries), int(K),
                       -1 if materials.id is None else int(materials.id)))

    def visible_pixels(self, unit="item", out_ptr=None, entries=None, width_range=None, height_range=None):
        """How many entries of the window each unit owns in the triangle-id target (frr_visible_pixels): unit="item", the
        items of the latest geometry pass as item_ranges() reports them, or "triangle", the triangle ids of the frame so far.
        With `out_ptr` -- device memory of `entries` uint32, e.g. a torch int32 / uint32 tensor's data_ptr() -- it is a
        command on the frame's stream with no host wait and returns nothing: every entry is written, units at and beyond
        `entries` are counted nowhere; order the reads with frame_fence(a created stream) or sync(), and keep the buffer
        until then.  Without `out_ptr` it is the host form (a synchronisation point) and returns a uint32 array of the n
        counts, or of `entries` of them."""
        wr = width_range or (0, self.width)
        hr = height_range or (0, self.height)
        return self._count_pixels("visible_pixels", unit, (wr[0], wr[1], hr[0], hr[1]), out_ptr, entries)

    def query_pixels(self, unit="item", window=None, out_ptr=None, entries=None):
        """The occlusion query (frr_query_pixels): how many fragments of each unit of the latest geometry pass -- unit="item"
        or "triangle", as for visible_pixels -- would pass the depth test against the depth target as it stands, in
        window = (x0, x1, y0, y1) (default: the frame).  Nothing is drawn.  With `out_ptr` (device memory of `entries`
        uint32) it is a command on the frame's stream with no host wait and returns nothing: the buffer can be the keep
        buffer of a later draw_list_if as it is.  Without `out_ptr` it is the host form (a synchronisation point) and
        returns a uint32 array of the n counts, or of `entries` of them."""
        return self._count_pixels("query_pixels", unit, window or (0, self.width, 0, self.height), out_ptr, entries)

    def _count_pixels(self, who, unit, window, out_ptr, entries):
        """visible_pixels / query_pixels (`who`): frr_<who> over the caller's device buffer, or frr_<who>_host"""
        u = {"item": N.PER_ITEM, "triangle": N.PER_TRIANGLE}.get(unit, unit)
        win = tuple(int(v) for v in window)
        if out_ptr is not None:
            if entries is None:
                raise FrrError(N.FRR_ERR_INVALID, who + ": the device form needs the buffer's entries")
            self._check(getattr(self._lib, "frr_" + who)(self._ctx, int(u), *win, C.c_void_p(out_ptr), int(entries)))
            return None
        host = getattr(self._lib, "frr_" + who + "_host")
        n = C.c_uint64()
        if entries is None:   # n first (one entry is enough to ask), then the counts
            probe = np.zeros(1, np.uint32)
            self._check(host(self._ctx, int(u), *win, probe.ctypes.data, 1, C.byref(n)))
            entries = int(n.value)
            if entries <= 1:
                return probe[:entries]
        out = np.zeros(int(entries), np.uint32)
        if out.size:
            self._check(host(self._ctx, int(u), *win, out.ctypes.data, out.size, C.byref(n)))
        return out

    def frame_fence(self, stream=None):
        """`stream` (a hipStream_t handle, e.g. torch's stream.cuda_stream; None = the ctx's stream) waits for every frame
        issued so far -- no host wait (frr_frame_fence; option bound_targets_in_flight)."""
        self._check(self._lib.frr_frame_fence(self._ctx, C.c_void_p(stream or 0)))

    def frame_wait(self, stream=None):
        """The next kernel that writes the frame targets waits for what `stream` (default: the ctx's) holds now
        (frr_frame_wait): e.g. an exchange that still reads a target set about to be bound for a new frame."""
        self._check(self._lib.frr_frame_wait(self._ctx, C.c_void_p(stream or 0)))

    def sync(self):
        self._check(self._lib.frr_sync(self._ctx))

    # -- results --
    def readback(self, color=True, depth=True, tri_id=True):
        n = self.width * self.height
        c = np.empty((self.height, self.width, 4), np.uint8) if color else None
        d = np.empty(n, np.float32) if depth else None
        t = np.empty(n, np.uint32) if tri_id else None
        self._check(self._lib.frr_readback(self._ctx, c.ctypes.data if color else None, d.ctypes.data if depth else None,
                                           t.ctypes.data if tri_id else None))
        return c, d, t

    def frame_buffer(self):
        """FrameBuffer with get_data() as phong.rs:386 reads it."""
        c, _, _ = self.readback(True, False, False)
        return FrameBuffer(self.width, self.height, c)

    def setup_triangles(self):
        """Vec<[Vertex;3]> of the last geometry_processing (emission order), for parity tests."""
        n = C.c_uint64()
        self._check(self._lib.frr_readback_setup(self._ctx, None, 0, C.byref(n)))
        out = np.zeros((int(n.value), 3), SETUP_DTYPE)
        if n.value:
            self._check(self._lib.frr_readback_setup(self._ctx, out.ctypes.data, n.value, C.byref(n)))
        return out

    def stats(self):
        s = N.Stats()
        self._check(self._lib.frr_get_stats(self._ctx, C.byref(s)))
        return s.as_dict()

    # -- timing --
    def event_record(self, slot):
        self._check(self._lib.frr_event_record(self._ctx, slot))

    def event_elapsed_ms(self, a, b):
        ms = C.c_float()
        self._check(self._lib.frr_event_elapsed_ms(self._ctx, a, b, C.byref(ms)))
        return float(ms.value)

    KERNELS = ("k_clear", "k_geom", "k_geom_scan", "k_bin_count",
               "k_tile_scan", "k_bin_fill", "k_raster", "k_bin_seg", "k_lines_mark", "k_lines_paint")

    # the order of the profile's mask bits: KERNELS, the kernels of a frame, then what was appended since
    PROFILE_ORDER = KERNELS + ("k_visible",)
    # ... and the bits behind those (frr_profile_get's list goes on: the bits above keep their meaning)
    PROFILE_APPENDED = ("k_boxes",)

    def profile_enable(self, on=True, kernels=None, period=1):
        """Bracket launches with HIP events: all kernels (on=True), none (False) or the named ones; only every
        `period`-th launch of each (an event pair costs the stream ~4 us)."""
        mask = (-1 if on else 0) if kernels is None else sum(1 << (self.PROFILE_ORDER + self.PROFILE_APPENDED).index(k) for k in kernels)
        self._check(self._lib.frr_profile_set_period(self._ctx, period))
        self._check(self._lib.frr_profile_enable(self._ctx, mask))

    def profile_reset(self):
        self._check(self._lib.frr_profile_reset(self._ctx))

    def profile_get(self, kernel):
        ms, n = C.c_float(), C.c_uint32()
        self._check(self._lib.frr_profile_get(self._ctx, kernel.encode(), C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def debug_rcp_check(self, lo_bits, hi_bits):
        """(mismatches, first offending bit pattern) of recip_exact vs the IEEE division on [lo_bits, hi_bits)."""
        n, first = C.c_uint64(0), C.c_uint32(0)
        self._check(self._lib.frr_debug_rcp_check(self._ctx, lo_bits, hi_bits, C.byref(n), C.byref(first)))
        return int(n.value), int(first.value)

    def debug_scan64(self, values):
        v = np.ascontiguousarray(values, np.uint32)
        assert v.size == 64
        out = np.empty(64, np.uint32)
        self._check(self._lib.frr_debug_scan64(self._ctx, v.ctypes.data, out.ctypes.data))
        return out

    def debug_atan2f(self, y, x):
        y = np.ascontiguousarray(y, np.float32)
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(y)
        self._check(self._lib.frr_debug_atan2f(self._ctx, y.ctypes.data, x.ctypes.data, out.ctypes.data, y.size))
        return out
