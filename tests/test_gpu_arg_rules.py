"""The status code of every entry point that takes a window, a pixel shader or a buffer, for arguments that break its rules
one at a time and two at a time, before any geometry pass and after a frr_draw that filtered the setup list on a 2-rank
partition.  A statement about behaviour: which rule answers, with which code, and which answers first when two are broken.
One 64 x 48 ctx, a one-triangle VS_CLIP_COLOR mesh (K = 3), a one-instance table, a one-item draw list; a one-triangle
VS_PHONG mesh (K = 8) serves the texture rule alone.  No refused call leaves anything behind: the frame drawn after the
table is the oracle's."""
import ctypes as C

import numpy as np
import pytest

from f_renderer_amd import scenes

pytestmark = pytest.mark.gpu
W, H = 64, 48
FULL = (0, W, 0, H)
OK, INVALID, UNSUPPORTED = 0, -1, -4
UNKNOWN_USER = 64 + 100000      # FRR_SHADER_USER_BASE + an index nobody registered

# (window, code) of the raster window rule: frr_raster and, behind their geometry pass, frr_draw / _instanced / _list
RASTER_WINDOWS = [
    (FULL, OK),
    ((5, 5, 0, H), OK), ((0, W, 7, 7), OK),                    # empty: valid, draws nothing
    ((-4, 60, 0, H), OK),                                      # x0 < 0 with the last depth index inside the buffer
    ((10, 5, 0, H), INVALID), ((0, W, 9, 2), INVALID),         # min > max
    ((0, W + 1, 0, H), INVALID), ((0, W, 0, H + 1), INVALID),  # larger than the FrameBuffer
    ((-32769, -32760, 0, H), UNSUPPORTED), ((0, W, -32769, -32760), UNSUPPORTED),      # outside i16
    ((32760, 32768, 0, H), UNSUPPORTED), ((0, W, 32760, 32768), UNSUPPORTED),
    ((-5, 0, 0, H), INVALID),                                  # x1 <= 0
    ((W, 2 * W, 0, H), INVALID),                               # the depth index leaves the buffer
    # two rules, different codes: the one applied first answers
    ((-32769, -32769 + W + 1, 0, H), INVALID),                 # larger than the FrameBuffer, before i16
    ((32710, 32768, 0, H), UNSUPPORTED),                       # i16, before the depth index
    ((32768, 32760, 0, H), INVALID),                           # min > max, before i16
]
# ... of the entry-addressed window rule: frr_resolve_varyings, frr_readback_varyings, frr_visible_pixels*, frr_shade_varyings*
ENTRY_WINDOWS = [
    (FULL, OK), ((3, 40, 5, 30), OK),
    ((5, 5, 0, H), INVALID), ((0, W, 7, 7), INVALID), ((10, 5, 0, H), INVALID), ((0, W, 9, 2), INVALID),   # empty, inverted
    ((-4, 60, 0, H), UNSUPPORTED),                             # x0 < 0
    ((0, W + 1, 0, H), INVALID), ((0, W, 0, H + 1), INVALID),  # larger than the FrameBuffer
    ((0, W, -32769, -32760), INVALID), ((32760, 32768, 0, H), INVALID), ((0, W, 32760, 32768), INVALID),   # outside i16
    ((W, 2 * W, 0, H), INVALID),                               # the depth index leaves the buffer
    # two rules, different codes
    ((-1, W, 0, H), UNSUPPORTED),                              # x0 < 0, before larger than the FrameBuffer
    ((-5, -5, 0, H), INVALID),                                 # empty, before x0 < 0
    ((-32769, -32760, 0, H), UNSUPPORTED),                     # x0 < 0: the i16 rule never sees x0
]


def _phong_triangle(L, fr):
    nf = L.frr_vs_input_floats(fr.VS_PHONG)
    a = np.zeros((1, 3, nf), np.float32)
    a[0, :, :2] = [[-0.5, -0.5], [0.5, -0.5], [0.0, 0.5]]
    return a


def test_status_codes_of_every_argument_rule():
    import torch
    import f_renderer_amd as fr
    from oracle import cref

    tri = scenes.single_triangle_rgb()
    r = fr.Renderer(W, H)
    L, ctx = r._lib, r._ctx
    mesh = r.upload_mesh(tri, fr.VS_CLIP_COLOR)
    mesh8 = r.upload_mesh(_phong_triangle(L, fr), fr.VS_PHONG)
    inst = r.upload_instances(np.eye(4, dtype=np.float32).reshape(1, 16))
    dl = r.upload_draw_list([mesh], np.eye(4, dtype=np.float32).reshape(1, 16))
    K, E = 3, W * H
    vbuf = torch.zeros(E * 8, dtype=torch.float32, device="cuda")      # [E][K] for K up to 8
    cbuf = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp, cp = vbuf.data_ptr(), cbuf.data_ptr()
    hv = np.zeros(E * 8, np.float32)
    hc = np.zeros(16, np.uint32)
    rgba = (C.c_uint8 * 4)(255, 0, 0, 255)
    n64 = C.c_uint64()
    P = C.c_void_p

    raster = lambda ps, w: L.frr_raster(ctx, ps, *w)
    draws = {
        "frr_draw": lambda ps, w: L.frr_draw(ctx, mesh.id, ps, *w),
        "frr_draw_instanced": lambda ps, w: L.frr_draw_instanced(ctx, mesh.id, inst.id, ps, *w),
        "frr_draw_list": lambda ps, w: L.frr_draw_list(ctx, dl.id, ps, *w),
    }
    resolve = lambda w, p=vp, e=E: L.frr_resolve_varyings(ctx, *w, P(p), e)
    rb_vary = lambda w, p=hv.ctypes.data, e=E: L.frr_readback_varyings(ctx, *w, P(p), e)
    visible = lambda w, unit=0, p=cp, e=16: L.frr_visible_pixels(ctx, unit, *w, P(p), e)
    visible_h = lambda w, unit=0, p=hc.ctypes.data, e=16: L.frr_visible_pixels_host(ctx, unit, *w, P(p), e, C.byref(n64))
    shade = lambda w, ps=fr.PS_COLOR, p=vp, e=E, k=K, count=0xFFFFFFFF: L.frr_shade_varyings(ctx, ps, *w, P(p), e, k, 0, count)
    shade_h = lambda w, ps=fr.PS_COLOR, p=hv.ctypes.data, e=E, k=K, count=0xFFFFFFFF: L.frr_shade_varyings_host(ctx, ps, *w, P(p), e, k, 0, count)
    wire = lambda: L.frr_draw_wireframe(ctx, rgba)
    rb_setup = lambda: L.frr_readback_setup(ctx, None, 0, C.byref(n64))
    ranges = lambda: L.frr_geometry_item_ranges(ctx, None, None, 0, C.byref(n64))
    entry_fns = {"frr_resolve_varyings": resolve, "frr_readback_varyings": rb_vary, "frr_visible_pixels": visible,
                 "frr_visible_pixels_host": visible_h, "frr_shade_varyings": shade, "frr_shade_varyings_host": shade_h}
    need_list = {"frr_draw_wireframe": wire, "frr_readback_setup": rb_setup, "frr_geometry_item_ranges": ranges}

    table = []     # (what, got, want)

    def row(what, got, want):
        table.append((what, got, want))

    r.clear()
    # ---- before any geometry pass -----------------------------------------------------------------------------------
    row("frr_raster before geometry", raster(fr.PS_COLOR, FULL), INVALID)
    row("frr_raster before geometry, i16", raster(fr.PS_COLOR, (32760, 32768, 0, H)), INVALID)       # the pass is asked for first
    for name, fn in entry_fns.items():
        shades = "shade" in name                                                                     # reads no geometry pass
        row(name + " before geometry", fn(FULL), OK if shades else INVALID)
        row(name + " before geometry, x0 < 0", fn((-4, 60, 0, H)), UNSUPPORTED if shades else INVALID)
    row("frr_visible_pixels before geometry, unknown unit", visible(FULL, unit=2), INVALID)
    for name, fn in need_list.items():
        row(name + " before geometry", fn(), INVALID)
    row("frr_readback_setup before geometry, ntris NULL", L.frr_readback_setup(ctx, None, 0, None), INVALID)

    # ---- behind an unfiltered geometry pass: every rule alone, and pairs ---------------------------------------------
    assert L.frr_geometry(ctx, mesh.id, None) == OK
    for w, want in RASTER_WINDOWS:
        row(f"frr_raster {w}", raster(fr.PS_COLOR, w), want)
        for name, fn in draws.items():
            row(f"{name} {w}", fn(fr.PS_COLOR, w), want)
    for ps, want in ((fr.PS_DEPTH, OK), (fr.PS_FLAT, OK), (fr.PS_COLOR, OK), (fr.PS_PHONG, INVALID), (fr.PS_BLINN, INVALID),
                     (-1, INVALID), (fr.PS_BLINN + 1, INVALID), (UNKNOWN_USER, INVALID)):
        row(f"frr_raster ps {ps}", raster(ps, FULL), want)
        for name, fn in draws.items():
            row(f"{name} ps {ps}", fn(ps, FULL), want)
    for name, fn in [("frr_raster", raster)] + list(draws.items()):
        row(name + " bad ps, i16 window", fn(fr.PS_PHONG, (32760, 32768, 0, H)), UNSUPPORTED)        # the window is asked for first
        row(name + " bad ps, empty window", fn(fr.PS_PHONG, (5, 5, 0, H)), INVALID)                  # ... and an empty one is still checked on
    assert L.frr_geometry(ctx, mesh8.id, None) == OK                                                 # K = 8, no texture bound
    row("frr_raster PS_PHONG, no texture", raster(fr.PS_PHONG, FULL), INVALID)
    row("frr_raster PS_BLINN, no texture", raster(fr.PS_BLINN, FULL), INVALID)
    row("frr_raster PS_COLOR on K = 8", raster(fr.PS_COLOR, FULL), INVALID)
    row("frr_draw PS_PHONG, no texture", L.frr_draw(ctx, mesh8.id, fr.PS_PHONG, *FULL), INVALID)
    row("frr_raster PS_FLAT on K = 8", raster(fr.PS_FLAT, FULL), OK)

    assert L.frr_geometry(ctx, mesh.id, None) == OK and raster(fr.PS_COLOR, FULL) == OK
    for w, want in ENTRY_WINDOWS:
        for name, fn in entry_fns.items():
            row(f"{name} {w}", fn(w), want)
    # buffers
    for name, fn in (("frr_resolve_varyings", resolve), ("frr_readback_varyings", rb_vary)):
        row(name + " NULL", fn(FULL, p=0), INVALID)
        row(name + " misaligned", fn(FULL, p=(vp if "resolve" in name else hv.ctypes.data) + 2), INVALID)
        row(name + " too few entries", fn(FULL, e=E - 1), INVALID)
        row(name + " entries of a sub-window", fn((3, 40, 5, 30), e=25 * 40), OK)
        row(name + " one entry short of a sub-window", fn((3, 40, 5, 30), e=25 * 40 - 1), INVALID)
        row(name + " NULL, x0 < 0", fn((-4, 60, 0, H), p=0), UNSUPPORTED)                            # the window is asked for first
    for name, fn in (("frr_visible_pixels", visible), ("frr_visible_pixels_host", visible_h)):
        row(name + " NULL", fn(FULL, p=0), INVALID)
        row(name + " misaligned", fn(FULL, p=(cp if name.endswith("pixels") else hc.ctypes.data) + 2), INVALID)
        row(name + " no entries, NULL", fn(FULL, p=0, e=0), OK)
        row(name + " per triangle", fn(FULL, unit=1), OK)
        for unit in (-1, 2):
            row(f"{name} unit {unit}", fn(FULL, unit=unit), INVALID)
            row(f"{name} unit {unit}, x0 < 0", fn((-4, 60, 0, H), unit=unit), INVALID)               # the unit is asked for first
            row(f"{name} unit {unit}, no entries", fn(FULL, unit=unit, p=0, e=0), INVALID)
        row(name + " NULL, x0 < 0", fn((-4, 60, 0, H), p=0), UNSUPPORTED)
    for name, fn in (("frr_shade_varyings", shade), ("frr_shade_varyings_host", shade_h)):
        base = vp if name.endswith("varyings") else hv.ctypes.data
        row(name + " NULL", fn(FULL, p=0), INVALID)
        row(name + " misaligned", fn(FULL, p=base + 2), INVALID)
        row(name + " too few entries", fn(FULL, e=E - 1), INVALID)
        row(name + " PS_FLAT, K = 0, NULL", fn(FULL, ps=fr.PS_FLAT, p=0, k=0), OK)
        row(name + " PS_FLAT, K = 0, misaligned", fn(FULL, ps=fr.PS_FLAT, p=base + 2, k=0), INVALID)
        row(name + " PS_FLAT, K = 8", fn(FULL, ps=fr.PS_FLAT, k=8), OK)
        row(name + " PS_FLAT, K = 16", fn(FULL, ps=fr.PS_FLAT, k=16, e=E, p=0), INVALID)             # (NULL: the K rule passes, the buffer rule answers)
        for k in (-1, 17):
            row(f"{name} PS_FLAT, K = {k}", fn(FULL, ps=fr.PS_FLAT, k=k), INVALID)
        row(name + " PS_DEPTH", fn(FULL, ps=fr.PS_DEPTH), INVALID)
        row(name + " PS_COLOR, K = 8", fn(FULL, ps=fr.PS_COLOR, k=8), INVALID)
        for ps in (fr.PS_PHONG, fr.PS_BLINN):
            row(f"{name} ps {ps}, K = 3", fn(FULL, ps=ps), INVALID)
            row(f"{name} ps {ps}, K = 8, no texture", fn(FULL, ps=ps, k=8), INVALID)
        for ps in (-1, fr.PS_BLINN + 1, UNKNOWN_USER):
            row(f"{name} ps {ps}", fn(FULL, ps=ps), INVALID)
        row(name + " PS_DEPTH, x0 < 0", fn((-4, 60, 0, H), ps=fr.PS_DEPTH), UNSUPPORTED)             # the window is asked for first
        row(name + " PS_DEPTH, NULL", fn(FULL, ps=fr.PS_DEPTH, p=0), INVALID)
        row(name + " no ids", fn(FULL, count=0), OK)
        row(name + " no ids, PS_DEPTH", fn(FULL, ps=fr.PS_DEPTH, count=0), INVALID)                  # (the other checks still apply)
    for name, fn in need_list.items():
        row(name + " behind an unfiltered pass", fn(), OK)
    row("frr_readback_setup ntris NULL", L.frr_readback_setup(ctx, None, 0, None), INVALID)
    row("frr_geometry_item_ranges nitems NULL", L.frr_geometry_item_ranges(ctx, None, None, 0, None), INVALID)
    row("frr_draw_wireframe colour NULL", L.frr_draw_wireframe(ctx, None), INVALID)

    # ---- behind a frr_draw that filtered the setup list (2-rank partition) -------------------------------------------
    for name, fn in draws.items():
        r.set_partition(0, 2)
        row(name + " on a partition", fn(fr.PS_COLOR, FULL), OK)
        row(f"frr_raster behind a filtered {name}, its window", raster(fr.PS_COLOR, FULL), OK)
        row(f"frr_raster behind a filtered {name}, another window", raster(fr.PS_COLOR, (0, W, 0, H - 1)), INVALID)
        row(f"frr_raster behind a filtered {name}, another window outside i16", raster(fr.PS_COLOR, (0, W, 32760, 32768)), UNSUPPORTED)
        for ename, efn in entry_fns.items():
            shades = "shade" in ename
            row(f"{ename} behind a filtered {name}", efn(FULL), OK if shades else INVALID)
            row(f"{ename} behind a filtered {name}, x0 < 0", efn((-4, 60, 0, H)), UNSUPPORTED)       # the window is asked for first
            if not shades:
                row(f"{ename} behind a filtered {name}, NULL", efn(FULL, p=0), INVALID)
        row(f"frr_visible_pixels behind a filtered {name}, no entries", visible(FULL, p=0, e=0), INVALID)
        for lname, lfn in need_list.items():
            row(f"{lname} behind a filtered {name}", lfn(), INVALID)
        r.set_partition(0, 1)
        row(f"frr_raster behind a filtered {name}, another partition", raster(fr.PS_COLOR, FULL), INVALID)
        row(f"frr_resolve_varyings behind a filtered {name}, another partition", resolve(FULL), INVALID)
        row(name + " again, no partition", fn(fr.PS_COLOR, FULL), OK)
        row(f"frr_resolve_varyings behind an unfiltered {name}", resolve(FULL), OK)
        row(f"frr_draw_wireframe behind an unfiltered {name}", wire(), OK)
    r.set_partition(0, 2)
    row("frr_draw on a partition, inverted rows", L.frr_draw(ctx, mesh.id, fr.PS_COLOR, 0, W, 9, 2), INVALID)
    row("frr_readback_setup behind it: the list was not filtered", rb_setup(), OK)
    r.set_partition(0, 1)

    bad = [t for t in table if t[1] != t[2]]
    assert not bad, f"{len(bad)} of {len(table)} status codes differ (what, got, want): {bad}"
    assert len(table) > 350

    # a rule's text names what the reference would have done
    assert raster(fr.PS_COLOR, (10, 5, 0, H)) == INVALID and b"renderer.rs:285" in L.frr_last_error(ctx)
    assert raster(fr.PS_COLOR, (W, 2 * W, 0, H)) == INVALID and b"renderer.rs:362" in L.frr_last_error(ctx)
    assert resolve((W, 2 * W, 0, H)) == INVALID and b"renderer.rs:362" in L.frr_last_error(ctx)

    # ---- a refused call leaves the ctx drawing ----------------------------------------------------------------------
    r.clear()
    r.draw(mesh, fr.PS_COLOR)
    c, d, t = r.readback()
    f = cref.Frame(W, H)
    f.clear()
    f.draw(tri, cref.VS_CLIP_COLOR, cref.PS_COLOR, cref.make_uniforms())
    assert f.counters.frag_covered > 100
    np.testing.assert_array_equal(t, f.tri_id)
    np.testing.assert_array_equal(d.view(np.uint32), f.depth.view(np.uint32))
    np.testing.assert_array_equal(c, f.color)
    r.close()
