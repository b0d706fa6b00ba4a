"""What tests/test_visible_cpu.py and tests/test_gpu_visible.py share: the definition of frr_visible_pixels restated in NumPy
-- np.bincount of np.searchsorted over the item boundaries per item, np.bincount of the ids per triangle."""
import numpy as np

NONE = 0xFFFFFFFF


def want_counts(ids, wr, hr, bounds=None, units=None, entries=None):
    """the definition in NumPy over the window's entries i = (cy - y0) * x1 + (cx - x0)"""
    (x0, x1), (y0, y1) = wr, hr
    i = (np.arange(y1 - y0)[:, None] * x1 + np.arange(x1 - x0)[None, :]).reshape(-1)
    v = np.asarray(ids, np.uint32).reshape(-1)[i].astype(np.int64)
    v = v[v != NONE]
    if bounds is None:
        n = int(units)
        c = np.bincount(v[v < n], minlength=n)
    else:
        b = np.asarray(bounds, np.int64)
        n = b.size - 1
        v = v[(v >= b[0]) & (v < b[-1])]
        c = np.bincount(np.searchsorted(b[1:], v, side="right"), minlength=n)[:n] if n else np.zeros(0, np.int64)
    e = n if entries is None else entries
    out = np.zeros(e, np.uint32)
    out[:min(n, e)] = c[:min(n, e)]
    return out


def bounds_of(per, base=0):
    return (base + np.cumsum([0] + list(per))).astype(np.uint32)
