"""Expected counts of frr_query_pixels on the CPU oracles, for tests/test_query_cpu.py and tests/test_gpu_query.py.

The count of setup triangle t is the number of entries that rasterization(t) ALONE changes on a copy of the depth buffer:
the depth D0 goes into a scratch Frame whose ids are reset, Frame.rasterization(..., PS_DEPTH, tri_id=marker) runs, and the
entries that hold the marker are counted -- per triangle, and summed per item.  The same through oracle_np.rasterization is
the cross-check.  Both oracles take the depth array as an argument.  Results are computed once per process and shared (never
modified)."""
import numpy as np

from . import drawlist_scenes as D

W, H = D.W, D.H
FULL = (0, W, 0, H)
MARK = 0x00ABCDEF
NONE = 0xFFFFFFFF

# (occluder list whose DEPTH frame is the depth, probe list): the pairs of the query tests, with the per-item counts the C
# oracle gave when they were chosen (None: pinned by sums, below)
PAIRS = {
    ("same_mesh", "clipped"): [576, 561, 1880, 667, 0, 3204, 456],
    ("clipped", "sizes"): [121, 104, 0, 94, 165, 128, 34],
    ("sizes", "sizes"): [121, 104, 112, 115, 165, 128, 34],
    ("tie", "tie"): [477, 477],
    ("clipped", "many"): None,        # sum 531 with 137 items at 0
    ("many", "empties"): [0, 203, 0, 0, 240, 0],
}
# the same probe lists against a cleared depth
CLEARED = {
    "clipped": [576, 561, 1880, 667, 0, 3215, 542],
    "sizes": [121, 104, 112, 117, 165, 128, 34],
}


def per_item_sums(per_tri, per_item):
    """per-triangle counts -> per-item sums, items of per_item[k] consecutive triangles"""
    b = np.concatenate([[0], np.cumsum(per_item)]).astype(np.int64)
    return np.array([int(per_tri[b[k]:b[k + 1]].sum()) for k in range(len(per_item))], np.uint32)


def counts_c(oracle, depth, setup, window=FULL, row_mask=None):
    """Per setup triangle, on the C oracle.  depth: the depth array (not modified).  row_mask: bool per window row, the rows
    that count (a partitioned rank's), or None."""
    x0, x1, y0, y1 = window
    fr = oracle.Frame(W, H)
    fr.depth[:] = depth
    u = oracle.make_uniforms()
    out = np.zeros(len(setup), np.uint32)
    for t in range(len(setup)):
        fr.rasterization((x0, x1), (y0, y1), setup[t], oracle.PS_DEPTH, 0, u, tri_id=MARK)
        idx = np.nonzero(fr.tri_id == MARK)[0]
        out[t] = idx.size if row_mask is None else int(row_mask[idx // x1].sum())
        fr.depth[idx] = depth[idx]
        fr.tri_id[idx] = NONE
    return out


def np_triangle(tri):
    """a setup triangle of the C oracle as oracle_np's rasterization takes it (`pos` holds the divided position)"""
    return [{"spi": (np.int32(v["spi"][0]), np.int32(v["spi"][1])), "spf": (np.float32(v["spf"][0]), np.float32(v["spf"][1])),
             "rhw": np.float32(v["rhw"]), "ctx": np.zeros(0, np.float32), "ndc": np.array(v["pos"], np.float32)} for v in tri]


def counts_np(depth, setup, window=FULL):
    """Per setup triangle, on the NumPy oracle"""
    from oracle import oracle_np as onp
    x0, x1, y0, y1 = window
    out = np.zeros(len(setup), np.uint32)
    color = np.zeros((H, W, 4), np.uint8)
    for t in range(len(setup)):
        d = np.array(depth, np.float32)
        ids = np.full(d.size, NONE, np.uint32)
        onp.rasterization((x0, x1), (y0, y1), np_triangle(setup[t]), onp.PS_DEPTH, None, color, d, ids, MARK, W)   # (a depth-only pass reads no uniform)
        out[t] = int((ids == MARK).sum())
    return out


_PAIR = {}


def pair(oracle, occ, probe):
    """(depth D0 of the occluder list's DEPTH frame, or the cleared depth for occ None; the probe's setup list; triangles per
    item; per-triangle counts; per-item counts) on the C oracle, full frame"""
    key = (occ, probe)
    if key not in _PAIR:
        if occ is None:
            d0 = np.full(W * H, D.CLEAR[1], np.float32)
        else:
            d0 = D.oracle_frame(oracle, occ, "DEPTH")[0].depth
        _, setup, per = D.oracle_frame(oracle, probe, "DEPTH")
        pt = counts_c(oracle, d0, setup)
        _PAIR[key] = (d0, setup, per, pt, per_item_sums(pt, per))
    return _PAIR[key]


BOX_INFLATE = 0.02      # about a pixel's worth at the demo camera's distance in the 128 x 96 frame


def box_scenes():
    """The box-proxy case of the end-to-end test, on predicate_scenes' `hidden` (a cover, items beside it and items behind
    it): (the occluder list: the cover alone; the probe list: all of `hidden`; the proxy list: the probe list with every mesh
    replaced by its inflated box, scenes.box_proxy, under the same matrices)"""
    from f_renderer_amd import scenes
    from . import predicate_scenes as P
    sc = P.scene("hidden")
    cover = P.kept_scene(sc, [i == 2 for i in range(sc.nitems)])
    boxes = D.Scene([D.Mesh(scenes.box_proxy(m.tris, BOX_INFLATE)) for m in sc.meshes], sc.which, sc.models, "PHONG", "DEPTH")
    return cover, sc, boxes
