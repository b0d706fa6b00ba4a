"""The rule of frr_query_boxes (include/frr.h, "box queries") restated in NumPy float32, operation by operation in the written
association, for tests/test_boxes_cpu.py and tests/test_gpu_boxes.py.  It shares no code with the header the library
compiles: every np.float32 operation below rounds once, as the C expression does.  Also the bounds of a mesh as
frr_drawlist_bounds defines them."""
import numpy as np

F = np.float32
NONE, OUTSIDE, HIDDEN, KEPT, UNBOUNDED = 0, 1, 2, 3, 4
U21 = F(2.0 ** -21)
ZUB_FACTOR = F(1.000003814697265625)
GUARD_LIMIT = F(32767.0)
ALL_ONES = 0xFFFFFFFF


def mat_mul(a, b):
    """glam Mat4 * Mat4, column-major [16]: column c of the product = ((a0*b0 + a1*b1) + a2*b2) + a3*b3"""
    a, b = np.asarray(a, F).reshape(16), np.asarray(b, F).reshape(16)
    out = np.zeros(16, F)
    with np.errstate(all="ignore"):
        for c in range(4):
            for r in range(4):
                out[4 * c + r] = ((a[r] * b[4 * c] + a[4 + r] * b[4 * c + 1]) + a[8 + r] * b[4 * c + 2]) + a[12 + r] * b[4 * c + 3]
    return out


def mvps_of(proj, view, models):
    """(proj * view) * model per item: [n, 16]"""
    pv = mat_mul(proj, view)
    m = np.asarray(models, F).reshape(-1, 16)
    return np.stack([mat_mul(pv, x) for x in m]) if len(m) else np.zeros((0, 16), F)


def bounds_of(tris):
    """(lo_hi [6], flags) of an expanded mesh [n, 3, NF]: frr_drawlist_bounds' definition (-0.0 reported as +0.0)"""
    t = np.asarray(tris, F)
    if t.shape[0] == 0:
        return np.zeros(6, F), 2
    p = t[:, :, :3].reshape(-1, 3)
    if not np.isfinite(p).all():
        return np.zeros(6, F), 1
    return np.concatenate([p.min(axis=0), p.max(axis=0)]).astype(F) + F(0.0), 0


def zkey(f):
    u = int((F(f) + F(0.0)).view(np.uint32))
    return u ^ (ALL_ONES if u >> 31 else 0x80000000)


def zkey_depth(d):
    """keys of an array of depths: a NaN below everything"""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        u = (d + F(0.0)).view(np.uint32)
    k = np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(d)] = 0
    return k


def as_i32(f):
    """Rust's `f32 as i32`"""
    if np.isnan(f):
        return 0
    if f >= F(2147483648.0):
        return 2 ** 31 - 1
    if f <= F(-2147483648.0):
        return -2 ** 31
    return int(np.trunc(f))


def owned_rows(ry0, ry1, row_owned):
    """owned pixel rows among the window-local rows ry0 .. ry1"""
    rows = np.arange(ry0, ry1 + 1)
    return int(rows.size if row_owned is None else np.asarray(row_owned, bool)[rows >> 5].sum())


def item(mvp, lo_hi, flags, size, window, keys, row_owned):
    """(out, status, rx0, ry0, rx1, ry1, level) of one item; keys: zkey_depth of the depth array"""
    W, H = size
    x0, x1, y0, y1 = window
    ww, wh = x1 - x0, y1 - y0
    if flags & 2:
        return 0, NONE, 0, 0, 0, 0, 0
    unbounded = (min(owned_rows(0, wh - 1, row_owned) * ww, ALL_ONES), UNBOUNDED, 0, 0, 0, 0, 0)
    m, b = np.asarray(mvp, F), np.asarray(lo_hi, F)
    with np.errstate(all="ignore"):
        a = np.maximum(np.abs(b[:3]), np.abs(b[3:]))
        am = np.abs(m)
        E = [(((am[r] * a[0] + am[4 + r] * a[1]) + am[8 + r] * a[2]) + am[12 + r] * F(1.0)) * U21 for r in range(4)]
        if (flags & 1) or not all(np.isfinite(e) for e in E):
            return unbounded
        clips, ndcs, spis = [], [], []
        for j in range(8):
            c = [b[3 + k] if (j >> k) & 1 else b[k] for k in range(3)]
            clip = [((m[r] * c[0] + m[4 + r] * c[1]) + m[8 + r] * c[2]) + m[12 + r] * F(1.0) for r in range(4)]
            rhw = F(1.0) / clip[3]
            ndc = (clip[0] * rhw, clip[1] * rhw)
            spf = ((ndc[0] + F(1.0)) * F(W) * F(0.5), (F(1.0) - ndc[1]) * F(H) * F(0.5))
            clips.append(clip)
            ndcs.append(ndc)
            spis.append((as_i32(spf[0] + F(0.5)), as_i32(spf[1] + F(0.5))))
        for clip, ndc in zip(clips, ndcs):
            if not all(np.isfinite(v) for v in clip) or not all(np.isfinite(v) for v in ndc):
                return unbounded
            if not (clip[2] - E[2] >= F(0.0)) or not (clip[3] - E[3] > F(0.0)):
                return unbounded
        wmin = min(c[3] for c in clips)
        wm = wmin - E[3]
        den = wm - E[3]
        if not den > F(0.0):
            return unbounded
        G = []
        for axis, D in ((0, F(W)), (1, F(H))):
            n = max(abs(v[axis]) for v in ndcs)
            eps = (E[axis] + n * E[3]) / den + n * U21
            d = eps * D + (n + F(1.0)) * D * U21
            if not d < GUARD_LIMIT:
                return unbounded
            G.append(1 + int(d))
        zub = (F(1.0) / wm) * ZUB_FACTOR
    lx = max(min(s[0] for s in spis) - G[0], x0)
    hx = min(max(s[0] for s in spis) + G[0], x1)
    ly = max(min(s[1] for s in spis) - G[1], y0)
    hy = min(max(s[1] for s in spis) + G[1], y1)
    if lx >= hx or ly >= hy:
        return 0, OUTSIDE, 0, 0, 0, 0, 0
    rx0, rx1, ry0, ry1 = lx - x0, hx - 1 - x0, ly - y0, hy - 1 - y0
    rows = owned_rows(ry0, ry1, row_owned)
    if rows == 0:
        return 0, OUTSIDE, 0, 0, 0, 0, 0
    count = rows * (rx1 - rx0 + 1)
    s = 2
    while (rx1 >> s) - (rx0 >> s) > 3 or (ry1 >> s) - (ry0 >> s) > 3:
        s += 1
    px = np.arange((rx0 >> s) << s, min(((rx1 >> s) + 1) << s, ww))
    py = np.arange((ry0 >> s) << s, min(((ry1 >> s) + 1) << s, wh))
    if row_owned is not None:
        py = py[np.asarray(row_owned, bool)[py >> 5]]
    region = keys[(py[:, None].astype(np.int64) * x1 + px[None, :]).reshape(-1)]    # renderer.rs:362
    dmin = int(region.min()) if region.size else ALL_ONES
    if zkey(zub) < dmin:
        return 0, HIDDEN, rx0, ry0, rx1, ry1, s
    return count, KEPT, rx0, ry0, rx1, ry1, s


def query(mvps, lo_hi, flags, size, window, depth, row_owned=None, entries=None):
    """(out uint32 [entries, default n], status_rect_level int32 [n, 6]) as frr_host_query_boxes returns them"""
    mvps, lo_hi = np.asarray(mvps, F).reshape(-1, 16), np.asarray(lo_hi, F).reshape(-1, 6)
    n = len(mvps)
    keys = zkey_depth(np.asarray(depth, F).reshape(-1))
    out = np.zeros(n if entries is None else int(entries), np.uint32)
    srl = np.zeros((n, 6), np.int32)
    for i in range(n):
        r = item(mvps[i], lo_hi[i], int(flags[i]), size, window, keys, row_owned)
        if i < out.size:
            out[i] = r[0]
        srl[i] = r[1:]
    return out, srl
