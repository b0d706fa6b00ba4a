"""What tests/test_shade_items_cpu.py and tests/test_gpu_shade_items.py share: the materials of a scene's items, and the
expected colour of frr_shade_items by two independent constructions, neither computed from the library.

  A  the definition, restated on the NumPy oracle: the depth-only frame of the list (ids, interpolated varyings), then one
     shade_scenes.shaded step per item over that item's id range under the call's uniforms with the item's material;
  B  the reference's loop with a ps_uniform per object, on the C oracle: one FORWARD frame.draw per item under that item's
     texture, strengths and flat colour (phong.rs:34-47, 361-370 without the `<=` quirk); its final RGBA is the expectation.

Also the per-entry item lookup restated with np.searchsorted (want_items) and the count of (span, distinct item) rounds.
Frames are the 128 x 96 of tests/drawlist_scenes.py; every oracle frame is computed once per process and never modified."""
import functools

import numpy as np

from oracle import oracle_np as onp
from . import drawlist_scenes as D
from . import instanced_scenes as S
from . import shade_scenes as SH
from . import varyings_scenes as V

F = np.float32
W, H = D.W, D.H
NONE = 0xFFFFFFFF
SCENES = ["sizes", "sizes_rev", "many", "empties", "clipped", "mix", "place", "one", "none", "all_empty"]
BG = D.CLEAR[0]


def materials(n, seed=0):
    """n materials (f_renderer_amd.MATERIAL_DTYPE): slots cycle 0..2 (drawlist_scenes.place_textures), and no two
    neighbours share a strength, a flat colour or a user value"""
    from f_renderer_amd import MATERIAL_DTYPE
    m = np.zeros(n, MATERIAL_DTYPE)
    k = np.arange(n) + seed
    m["texture_slot"] = k % 3
    m["ambient_strength"] = (0.05 + 0.1 * (k % 5)).astype(F)
    m["specular_strength"] = (0.2 + 0.15 * (k % 4)).astype(F)
    m["flat_color"] = np.stack([((k * 37) % 256) / 255.0, ((k * 91 + 40) % 256) / 255.0, ((k * 13 + 200) % 256) / 255.0, np.ones(n)], axis=1).astype(F)
    m["user"] = ((k[:, None] * 8 + np.arange(8)[None, :]) % 23 / 22.0).astype(F)
    return m


def _np_uniforms(kw, mat, texs):
    return onp.Uniforms(tex=texs[int(mat["texture_slot"])], ambient=F(mat["ambient_strength"]), specular=F(mat["specular_strength"]),
                        flat_color=tuple(F(x) for x in mat["flat_color"]), **kw)


@functools.lru_cache(maxsize=None)
def depth_only(name):
    """the list drawn depth-only by the NumPy oracle, which keeps every pixel's varyings: (scene, camera keywords, Expected)"""
    sc = D.scene(name)
    kw = S.camera_kw(onp)
    full = [i for i in range(sc.nitems) if sc.ntris[i]]           # (an empty item is no draw at all, as in drawlist_scenes.oracle_list_loop)
    draws = [(sc.item_tris(i), onp.VS_PHONG, onp.Uniforms(model=sc.models[i], **kw)) for i in full]
    if not draws:
        e = V.Expected(SH.background((W, H), BG), np.zeros(W * H, F), np.full(W * H, NONE, np.uint32), np.full((W * H, 8), np.nan, F), [], (0, W, 0, H))
    else:
        e = SH.render(draws, ps=V.zero_ps, size=(W, H), bg=BG)
    per = [0] * sc.nitems
    for i, n in zip(full, e.n_emit):
        per[i] = n
    e.n_emit = per                                                # per ITEM from here on
    return sc, kw, e


def item_ranges(per, base=0):
    """[(first id, count)] per item"""
    b = base + np.cumsum([0] + list(per))
    return [(int(b[k]), int(per[k])) for k in range(len(per))]


def expected_A(name, ps=onp.PS_PHONG, mats=None, start=None):
    """construction A: [H, W, 4]"""
    sc, kw, e = depth_only(name)
    mats = materials(sc.nitems) if mats is None else mats
    texs = D.place_textures()
    shades = [(ps, _np_uniforms(kw, mats[k], texs), rg) for k, rg in enumerate(item_ranges(e.n_emit))]
    return SH.shaded(e, shades, start=SH.background((W, H), BG) if start is None else start)


def forward_B(items, mats, ps="PHONG", frame=None, window=None):
    """construction B over any items [(tris [n, 3, 8], model [16])]: one forward draw per item on the C oracle under that item's
    material, into `frame` (default: a cleared one), ids running on behind what the frame holds.  Returns (Frame, triangles
    emitted per item)."""
    from oracle import cref as oracle
    texs = [oracle.Texture(t) for t in D.place_textures()]
    if frame is None:
        frame = oracle.Frame(W, H)
        frame.clear(*D.CLEAR)
    kw = S.camera_kw(oracle)
    base = int(frame.counters.tris_setup)
    per = []
    for i, (tris, model) in enumerate(items):
        before = int(frame.counters.tris_setup)
        if tris.shape[0]:
            m = mats[i]
            u = oracle.make_uniforms(model=model, tex=texs[int(m["texture_slot"])], ambient=m["ambient_strength"], specular=m["specular_strength"],
                                     flat_color=m["flat_color"], **kw)
            frame.draw(tris, oracle.VS_PHONG, getattr(oracle, "PS_" + ps), u, window=window, tri_id_base=base + sum(per))
        per.append(int(frame.counters.tris_setup) - before)
    return frame, per


def dense_models(cols, rows, s=0.12):
    """cols * rows model matrices on a grid that fills the view, each with its own rotation: with instanced_scenes.patch(1)
    a few pixels per instance, most instances visible, a neighbour in nearly every pixel's span"""
    out = []
    for i in range(cols * rows):
        gx, gy = i % cols, i // cols
        t = S.translate((gx + 0.5) / cols * 3.4 - 1.7, (gy + 0.5) / rows * 2.6 - 1.3, -0.2 * (i % 3))
        out.append(S._col_major(t @ S.rot_y(0.2 * i) @ S.rot_x(0.1 * (i % 5)) @ S.scale(s)))
    return np.stack(out)


def scene_items(sc):
    return [(sc.item_tris(i), sc.models[i]) for i in range(sc.nitems)]


@functools.lru_cache(maxsize=None)
def _expected_B(name, ps, window=None):
    sc = D.scene(name)
    return forward_B(scene_items(sc), materials(sc.nitems), ps, window=window)


def expected_B(name, ps="PHONG", window=None):
    """construction B of a scene: (the C oracle's Frame -- color [H, W, 4], depth, tri_id --, triangles emitted per item);
    window: (x0, x1, y0, y1) of every draw"""
    return _expected_B(name, ps, window)


def want_items(ids, wr, hr, bounds):
    """every entry's item by np.searchsorted over the boundaries, NONE where the id is not one of the pass's or the entry is
    not one of the window's: uint32, shaped like ids.reshape(-1)"""
    (x0, x1), (y0, y1) = wr, hr
    a = np.asarray(ids, np.uint32).reshape(-1)
    b = np.asarray(bounds, np.int64)
    out = np.full(a.size, NONE, np.uint32)
    i = (np.arange(y1 - y0)[:, None] * x1 + np.arange(x1 - x0)[None, :]).reshape(-1)
    v = a[i].astype(np.int64)
    ok = (v != NONE) & (v >= b[0]) & (v < b[-1])
    out[i[ok]] = np.searchsorted(b[1:], v[ok], side="right")
    return out


def want_rounds(items, wr, hr):
    """(span, distinct item) pairs: per window row and 64 entries of it, the distinct items its entries hold; also the
    histogram {distinct items in a span: spans}"""
    (x0, x1), (y0, y1) = wr, hr
    it = np.asarray(items, np.uint32).reshape(-1)
    rounds, hist = 0, {}
    for ry in range(y1 - y0):
        for c0 in range(0, x1 - x0, 64):
            s = it[ry * x1 + c0: ry * x1 + min(c0 + 64, x1 - x0)]
            n = np.unique(s[s != NONE]).size
            rounds += n
            hist[n] = hist.get(n, 0) + 1
    return rounds, hist
