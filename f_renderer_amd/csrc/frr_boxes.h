// frr_boxes.h -- frr_drawlist_bounds and frr_query_boxes: the cheap occlusion test.  Per item of a draw list the object-space
// box of its mesh, projected under the item's own matrix, against the farthest depth stored under its screen rectangle -- no
// geometry pass, no binning, no work list.  The test is CONSERVATIVE: an item it calls hidden changes no entry of colour,
// depth or ids when drawn now, and the value it writes is an upper bound of the pixels the item can own (DESIGN section 5,
// "Box queries", proves the three margins used below: E, the guard G, and the depth bound zub).
//
// The rule (box_corner .. box_rect, box_host_query) is plain C++: it compiles for the device, for the host side of the library
// (frr_host_query_boxes) and with no HIP at all (tests/boxes_host.cpp).  Host and device run the same functions per corner and
// per item; what differs is only how the eight corners are reduced (a loop / 16 lanes) and where the smallest depth key of
// the region comes from (a walk over the pixels / the pyramid) -- minima and maxima, which do not depend on the order.
//
//   k_box_bounds        per distinct mesh of a list: min / max of the positions its triangles name, as order-preserving keys:
//                       per wave with shuffles, across waves through LDS, one integer atomic per workgroup and component
//   k_box_bounds_finish per item: the keys of its mesh decoded into lo, hi and the flags
//   k_box_base          (a) one workgroup per 32 x 32 tile of the window: the depth keys' minima over 4 x 4, 8 x 8, 16 x 16
//                       and 32 x 32 pixels (levels 2 .. 5); pixels outside the window or in rows of another rank are all-ones
//   k_box_top           (b) levels 6 and up from level 5, one wave per cell
//   k_box_test          (c) 16 lanes per item: a corner per lane, reductions inside the group, the at most 4 x 4 cells
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include "frr_kernels.h"
#define FRR_BOX_HD FRR_HD
#else
#define FRR_BOX_HD inline
#endif

namespace frr {

enum BoxStatus { BOX_NONE = 0, BOX_OUTSIDE = 1, BOX_HIDDEN = 2, BOX_KEPT = 3, BOX_UNBOUNDED = 4 };
constexpr uint32_t BOX_FLAG_NONFINITE = 1u;   // some referenced position component is NaN or +-inf (lo / hi unspecified)
constexpr uint32_t BOX_FLAG_EMPTY = 2u;       // the mesh has no triangles
constexpr int BOX_LEVEL_MIN = 2, BOX_LEVEL_TILE = 5, BOX_LEVEL_MAX = 13;   // 32,767 >> 13 == 3: four cells span any window
constexpr float BOX_GUARD_LIMIT = 32767.0f;   // a guard of 2^15 pixels or more: the item is UNBOUNDED

// ---- bits ---------------------------------------------------------------------------------------------------------------
// (restated from frr_exact.h -- zkey, zkey_depth, f32_as_i32_ref -- so that this part needs no HIP header)
FRR_BOX_HD uint32_t box_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
FRR_BOX_HD float box_float(uint32_t u) { return __builtin_bit_cast(float, u); }
FRR_BOX_HD bool box_finite(float f) { return (box_bits(f) & 0x7F800000u) != 0x7F800000u; }
FRR_BOX_HD float box_abs(float f) { return box_float(box_bits(f) & 0x7FFFFFFFu); }
FRR_BOX_HD uint32_t box_zkey(float f)
{
    const uint32_t u = box_bits(f + 0.0f);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
FRR_BOX_HD uint32_t box_zkey_depth(float d) { return d == d ? box_zkey(d) : 0u; }
FRR_BOX_HD float box_zkey_decode(uint32_t k) { return box_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
FRR_BOX_HD int32_t box_as_i32(float f)
{
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int32_t)f;
}

// ---- the rule -----------------------------------------------------------------------------------------------------------
// mvp = pv * model, column by column with the association of mat4_mul_vec4 (k_instance_mvp, frr_host_instance_mvp): the bits
// the list pass transforms the item's vertices with.
FRR_BOX_HD void box_mvp(const float *pv, const float *model, float *mvp)
{
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r)
            mvp[4 * c + r] = ((pv[r] * model[4 * c] + pv[4 + r] * model[4 * c + 1]) + pv[8 + r] * model[4 * c + 2]) + pv[12 + r] * model[4 * c + 3];
}

// Corner j of the box (bit k of j picks hi[k]) as the geometry pass would see a vertex there: clip position, then rhw, ndc,
// spf and spi by renderer.rs:223-234.
struct BoxCorner { float x, y, z, w, ndcx, ndcy; int32_t spix, spiy; };
FRR_BOX_HD BoxCorner box_corner(const float *m, const float *lo_hi, int j, uint32_t W, uint32_t H)
{
    const float cx = lo_hi[(j & 1) ? 3 : 0], cy = lo_hi[(j & 2) ? 4 : 1], cz = lo_hi[(j & 4) ? 5 : 2];
    BoxCorner c;
    c.x = ((m[0] * cx + m[4] * cy) + m[8] * cz) + m[12] * 1.0f;
    c.y = ((m[1] * cx + m[5] * cy) + m[9] * cz) + m[13] * 1.0f;
    c.z = ((m[2] * cx + m[6] * cy) + m[10] * cz) + m[14] * 1.0f;
    c.w = ((m[3] * cx + m[7] * cy) + m[11] * cz) + m[15] * 1.0f;
    const float rhw = 1.0f / c.w;                              // :223
    c.ndcx = c.x * rhw; c.ndcy = c.y * rhw;                    // :226
    const float spfx = (c.ndcx + 1.0f) * (float)W * 0.5f;      // :229
    const float spfy = (1.0f - c.ndcy) * (float)H * 0.5f;      // :230
    c.spix = box_as_i32(spfx + 0.5f); c.spiy = box_as_i32(spfy + 0.5f);   // :233-234
    return c;
}
// E = |mvp| * (a, 1) * 2^-21 with a = max(|lo|, |hi|) per axis: every mesh vertex p has |p_k| <= a_k, so each of its computed
// clip components lies within E / 2 of the exact affine image of p, and so does each corner's.
FRR_BOX_HD void box_error(const float *m, const float *lo_hi, float E[4])
{
    float a[3];
    for (int k = 0; k < 3; ++k) { const float l = box_abs(lo_hi[k]), h = box_abs(lo_hi[3 + k]); a[k] = l > h ? l : h; }
    for (int r = 0; r < 4; ++r)
        E[r] = (((box_abs(m[r]) * a[0] + box_abs(m[4 + r]) * a[1]) + box_abs(m[8 + r]) * a[2]) + box_abs(m[12 + r]) * 1.0f) * 4.76837158203125e-07f;
}
// What the eight corners reduce to.  bad: some corner has a clip component or an ndc that is not finite, z - E_z < 0 (it may
// lie in front of the near plane: the reference's Z_NEAR ratio, renderer.rs:70, puts intersection vertices outside the
// triangle's own segment) or w - E_w <= 0.
struct BoxReduce { uint32_t bad; float wmin, nx, ny; int32_t sxmin, sxmax, symin, symax; };
FRR_BOX_HD BoxReduce box_reduce_one(const BoxCorner &c, const float E[4])
{
    BoxReduce r;
    const bool fin = box_finite(c.x) && box_finite(c.y) && box_finite(c.z) && box_finite(c.w) && box_finite(c.ndcx) && box_finite(c.ndcy);
    const bool front = (c.z - E[2] >= 0.0f) && (c.w - E[3] > 0.0f);   // (false where a NaN is involved)
    r.bad = fin && front ? 0u : 1u;
    r.wmin = c.w; r.nx = box_abs(c.ndcx); r.ny = box_abs(c.ndcy);
    r.sxmin = r.sxmax = c.spix; r.symin = r.symax = c.spiy;
    return r;
}
FRR_BOX_HD BoxReduce box_reduce_join(const BoxReduce &a, const BoxReduce &b)
{
    BoxReduce r;
    r.bad = a.bad | b.bad;
    r.wmin = b.wmin < a.wmin ? b.wmin : a.wmin;   // (NaNs make the item `bad`: what these hold then is never read)
    r.nx = b.nx > a.nx ? b.nx : a.nx; r.ny = b.ny > a.ny ? b.ny : a.ny;
    r.sxmin = b.sxmin < a.sxmin ? b.sxmin : a.sxmin; r.sxmax = b.sxmax > a.sxmax ? b.sxmax : a.sxmax;
    r.symin = b.symin < a.symin ? b.symin : a.symin; r.symax = b.symax > a.symax ? b.symax : a.symax;
    return r;
}

// The window of the command and who owns its tile rows.  Own: `bool operator()(int ty) const`, does this rank own window-local
// tile row ty (32 pixel rows)?
struct BoxWindow { uint32_t W, H; int32_t x0, x1, y0, y1; };
template <class Own> FRR_BOX_HD uint32_t box_owned_rows(int32_t ry0, int32_t ry1, const Own &own)   // owned pixel rows in [ry0, ry1], window-local
{
    uint32_t n = 0u;
    for (int32_t t = ry0 >> 5; t <= (ry1 >> 5); ++t) {
        if (!own(t)) continue;
        const int32_t a = t * 32 > ry0 ? t * 32 : ry0, b = t * 32 + 31 < ry1 ? t * 32 + 31 : ry1;
        n += (uint32_t)(b - a + 1);
    }
    return n;
}
// The verdict of one item up to the depth comparison.
//   status   NONE, OUTSIDE, UNBOUNDED: final.  KEPT: the item is HIDDEN instead iff zkey < the smallest depth key of the region.
//   rx0..ry1 the rectangle clamped to the window, window-local, inclusive; level: the pyramid level of the region -- the cells
//            (rx0 >> level .. rx1 >> level) x (ry0 >> level .. ry1 >> level), at most 4 x 4, cut to the window
//   count    the value written unless hidden: the owned pixels of the rectangle (UNBOUNDED: of the window; else 0)
// The guard, per axis (x: n = nx, D = W; y: n = ny, D = H), with den = (wmin - E_w) - E_w, which has to be positive:
//   eps = (E_axis + n * E_w) / den + n * 2^-21        how far a vertex's computed ndc can lie outside the corners' computed ndc
//   d   = eps * D + (n + 1) * D * 2^-21               ... and its spf outside theirs, in pixels
//   G   = 1 + (int)d                                  d has to stay below BOX_GUARD_LIMIT
struct BoxRect { int32_t status, rx0, ry0, rx1, ry1, level; uint32_t zkey, count; };
template <class Own>
FRR_BOX_HD BoxRect box_rect(uint32_t flags, const float E[4], const BoxReduce &red, const BoxWindow &w, const Own &own, uint32_t window_owned_rows)
{
    BoxRect o;
    o.status = BOX_NONE; o.rx0 = o.ry0 = o.rx1 = o.ry1 = o.level = 0; o.zkey = 0u; o.count = 0u;
    if (flags & BOX_FLAG_EMPTY) return o;
    const unsigned long long wpx = (unsigned long long)window_owned_rows * (unsigned long long)(w.x1 - w.x0);
    const uint32_t unbounded = wpx > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)wpx;
    o.status = BOX_UNBOUNDED; o.count = unbounded;
    if ((flags & BOX_FLAG_NONFINITE) || red.bad || !box_finite(E[0]) || !box_finite(E[1]) || !box_finite(E[2]) || !box_finite(E[3])) return o;
    const float wm = red.wmin - E[3], den = wm - E[3];
    if (!(den > 0.0f)) return o;
    const float ex = (E[0] + red.nx * E[3]) / den + red.nx * 4.76837158203125e-07f;
    const float ey = (E[1] + red.ny * E[3]) / den + red.ny * 4.76837158203125e-07f;
    const float dx = ex * (float)w.W + (red.nx + 1.0f) * (float)w.W * 4.76837158203125e-07f;
    const float dy = ey * (float)w.H + (red.ny + 1.0f) * (float)w.H * 4.76837158203125e-07f;
    if (!(dx < BOX_GUARD_LIMIT) || !(dy < BOX_GUARD_LIMIT)) return o;   // (not finite: the comparison is false)
    const long long gx = 1 + (long long)(int32_t)dx, gy = 1 + (long long)(int32_t)dy;
    // a triangle's fragments lie in min spi <= c < max spi, clamped to the window (renderer.rs:285-298, :322-324)
    long long lx = (long long)red.sxmin - gx, hx = (long long)red.sxmax + gx, ly = (long long)red.symin - gy, hy = (long long)red.symax + gy;
    lx = lx < w.x0 ? w.x0 : lx; hx = hx > w.x1 ? w.x1 : hx; ly = ly < w.y0 ? w.y0 : ly; hy = hy > w.y1 ? w.y1 : hy;
    o.status = BOX_OUTSIDE; o.count = 0u;
    if (lx >= hx || ly >= hy) return o;
    o.rx0 = (int32_t)(lx - w.x0); o.rx1 = (int32_t)(hx - 1 - w.x0); o.ry0 = (int32_t)(ly - w.y0); o.ry1 = (int32_t)(hy - 1 - w.y0);
    const uint32_t rows = box_owned_rows(o.ry0, o.ry1, own);
    if (rows == 0u) { o.rx0 = o.ry0 = o.rx1 = o.ry1 = 0; return o; }
    o.count = rows * (uint32_t)(o.rx1 - o.rx0 + 1);   // (below 2^30: window coordinates are i16)
    int s = BOX_LEVEL_MIN;
    while ((o.rx1 >> s) - (o.rx0 >> s) > 3 || (o.ry1 >> s) - (o.ry0 >> s) > 3) ++s;
    o.level = s;
    // every vertex's w is at least wmin - E_w, so (f32 division is monotone) its rhw is at most 1 / (wmin - E_w); a fragment's
    // is a convex combination of three up to the factor cull_zub proves
    o.zkey = box_zkey((1.0f / wm) * 1.000003814697265625f);
    o.status = BOX_KEPT;
    return o;
}

// ---- the host build of the whole rule ---------------------------------------------------------------------------------------
struct BoxOwnMask {
    const uint8_t *m;   // [tile rows of the window] or null: all
    bool operator()(int ty) const { return !m || m[ty] != 0; }
};
// out[i], i < min(nitems, out_entries), = the item's value; entries at and beyond nitems = 0.  The region's minimum is a plain
// walk over its pixels.  status_rect_level: [nitems][6] = status, rx0, ry0, rx1, ry1, level, or null.  Returns nitems.
inline int64_t box_host_query(const float *mvps, const float *lo_hi, const uint32_t *flags, uint64_t nitems, const BoxWindow &w,
                              const float *depth, const uint8_t *row_owned, uint32_t *out, uint64_t out_entries, int32_t *srl)
{
    const BoxOwnMask own = {row_owned};
    const int32_t ww = w.x1 - w.x0, wh = w.y1 - w.y0;
    const uint32_t wrows = box_owned_rows(0, wh - 1, own);
    for (uint64_t i = 0; i < nitems; ++i) {
        const float *m = mvps + 16 * i, *b = lo_hi + 6 * i;
        float E[4];
        box_error(m, b, E);
        BoxReduce red = box_reduce_one(box_corner(m, b, 0, w.W, w.H), E);
        for (int j = 1; j < 8; ++j) red = box_reduce_join(red, box_reduce_one(box_corner(m, b, j, w.W, w.H), E));
        BoxRect r = box_rect(flags[i], E, red, w, own, wrows);
        if (r.status == BOX_KEPT) {
            const int s = r.level;
            uint32_t dmin = 0xFFFFFFFFu;
            const int32_t px0 = (r.rx0 >> s) << s, py0 = (r.ry0 >> s) << s;
            int32_t px1 = ((r.rx1 >> s) + 1) << s, py1 = ((r.ry1 >> s) + 1) << s;
            px1 = px1 > ww ? ww : px1; py1 = py1 > wh ? wh : py1;
            for (int32_t py = py0; py < py1; ++py) {
                if (!own(py >> 5)) continue;
                for (int32_t px = px0; px < px1; ++px) {
                    const uint32_t k = box_zkey_depth(depth[(size_t)py * (size_t)w.x1 + (size_t)px]);   // renderer.rs:362
                    dmin = k < dmin ? k : dmin;
                }
            }
            if (r.zkey < dmin) { r.status = BOX_HIDDEN; r.count = 0u; }   // strictly: a tie keeps, as fragment_passes lets ties pass
        }
        if (i < out_entries) out[i] = r.count;
        if (srl) { int32_t *q = srl + 6 * i; q[0] = r.status; q[1] = r.rx0; q[2] = r.ry0; q[3] = r.rx1; q[4] = r.ry1; q[5] = r.level; }
    }
    for (uint64_t i = nitems; i < out_entries; ++i) out[i] = 0u;
    return (int64_t)nitems;
}

#if defined(__HIPCC__)
// ---- bounds -------------------------------------------------------------------------------------------------------------
constexpr int BOX_WG = 256;
constexpr uint32_t BOX_WG_TRIS = 1024;   // triangles per workgroup and step of k_box_bounds: 3,072 corners, 12 per thread
struct BoundsJob {
    const float *verts;     // [ntris][3][nf], or with idx: [nverts][nf]
    const uint32_t *idx;    // [ntris][3] or null
    uint32_t nverts, ntris, nf, pad;
};
// keys: [njobs][8] = min x y z, max x y z, non-finite flag, pad; on entry 0xFFFFFFFF x 3, 0 x 5.  grid = (chunks, njobs).
__global__ __launch_bounds__(BOX_WG) void k_box_bounds(const BoundsJob *__restrict__ jobs, uint32_t *__restrict__ keys)
{
    __shared__ uint32_t s_red[BOX_WG / 64][8];
    const BoundsJob j = jobs[blockIdx.y];
    const unsigned long long ncorn = 3ull * j.ntris;
    if ((unsigned long long)blockIdx.x * (3ull * BOX_WG_TRIS) >= ncorn) return;   // (block-uniform)
    const bool vec = ((uintptr_t)j.verts & 15u) == 0u && (j.nf & 3u) == 0u;
    const uint32_t last = j.nverts ? j.nverts - 1u : 0u;
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u}, bad = 0u;
    for (unsigned long long base = (unsigned long long)blockIdx.x * (3ull * BOX_WG_TRIS); base < ncorn; base += (unsigned long long)gridDim.x * (3ull * BOX_WG_TRIS)) {
        const unsigned long long end = base + 3ull * BOX_WG_TRIS < ncorn ? base + 3ull * BOX_WG_TRIS : ncorn;
        for (unsigned long long q = base + threadIdx.x; q < end; q += BOX_WG) {
            const size_t rec = j.idx ? (size_t)min(j.idx[q], last) : (size_t)q;   // (the clamp of the geometry kernels: tri_inputs)
            const float *p = j.verts + rec * j.nf;
            float v[3];
            if (vec) { const float4 f = *reinterpret_cast<const float4 *>(p); v[0] = f.x; v[1] = f.y; v[2] = f.z; }
            else { v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (!box_finite(v[k])) { bad = 1u; continue; }
                const uint32_t key = box_zkey(v[k]);
                mn[k] = min(mn[k], key); mx[k] = max(mx[k], key);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = min(mn[k], (uint32_t)__shfl_xor(mn[k], o)); mx[k] = max(mx[k], (uint32_t)__shfl_xor(mx[k], o)); }
        bad |= (uint32_t)__shfl_xor(bad, o);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_red[wv][k] = mn[k]; s_red[wv][3 + k] = mx[k]; }
        s_red[wv][6] = bad; s_red[wv][7] = 0u;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int k = threadIdx.x;
        uint32_t v = s_red[0][k];
        for (int x = 1; x < BOX_WG / 64; ++x) v = k < 3 ? min(v, s_red[x][k]) : k < 6 ? max(v, s_red[x][k]) : (v | s_red[x][k]);
        uint32_t *dst = keys + (size_t)blockIdx.y * 8 + k;
        if (k < 3) atomicMin(dst, v); else if (k < 6) atomicMax(dst, v); else if (v) atomicOr(dst, v);
    }
}
__global__ __launch_bounds__(BOX_WG) void k_box_bounds_finish(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ item_job, const BoundsJob *__restrict__ jobs,
                                                              uint32_t nitems, float *__restrict__ lo_hi, uint32_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * BOX_WG + threadIdx.x;
    if (i >= nitems) return;
    const uint32_t jb = item_job[i];
    const uint32_t *k = keys + (size_t)jb * 8;
    const bool empty = jobs[jb].ntris == 0u;
    for (int c = 0; c < 6; ++c) lo_hi[(size_t)i * 6 + c] = empty ? 0.0f : box_zkey_decode(k[c]);
    flags[i] = (k[6] ? BOX_FLAG_NONFINITE : 0u) | (empty ? BOX_FLAG_EMPTY : 0u);
}

// ---- the pyramid --------------------------------------------------------------------------------------------------------
// Level s (2 .. top) holds the minima of the depth keys over cells of 2^s x 2^s window pixels, row-major, lw[s] cells to a row.
// Levels up to 5 are padded to whole tiles (lw = tiles_x << (5 - s)), so a tile's workgroup writes its cells unconditionally.
struct BoxPyramid {
    uint32_t *cells;
    uint32_t off[BOX_LEVEL_MAX + 1], lw[BOX_LEVEL_MAX + 1], lh[BOX_LEVEL_MAX + 1];
    int32_t top;            // the last level: the first at which four cells span the window in both directions
    uint32_t top_cells;     // cells of the levels 6 .. top together
};
struct BoxOwnRows {
    RowOwner o;
    __device__ __forceinline__ bool operator()(int ty) const { return owns_tile_row(ty, o); }
};
struct BoxArgs {
    BoxWindow w;
    int32_t tiles_x, tiles_y;
    RowOwner own;
    uint32_t window_owned_rows;
    const float *depth;               // the frame's depth target: entry (ry, rx) of the window at ry * x1 + rx
    int32_t depth_vec;                // the pointer is 16-byte aligned
    BoxPyramid pyr;
    Mat4Arg pv;                       // proj * view of the call
    const float *models;              // [nitems][16] the list's matrices
    const float *lo_hi;               // [nitems][6] frr_drawlist_bounds
    const uint32_t *flags;            // [nitems]
    uint32_t nitems;
    uint32_t *out; unsigned long long out_entries;
    uint32_t seq, epoch; const Counters *cnt;
};

__global__ __launch_bounds__(256) void k_box_base(BoxArgs a)
{
    __shared__ uint32_t s3[4][4];
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;
    const int tx = (int)(blockIdx.x % (uint32_t)a.tiles_x), ty = (int)(blockIdx.x / (uint32_t)a.tiles_x);
    const int i = threadIdx.x, lane = i & 63, wv = i >> 6;
    const int y = i >> 3, xq = (i & 7) * 4;
    const int ww = a.w.x1 - a.w.x0, wh = a.w.y1 - a.w.y0;
    const int rx = tx * TILE + xq, ry = ty * TILE + y;
    uint32_t m = 0xFFFFFFFFu;
    if (owns_tile_row(ty, a.own) && ry < wh && rx < ww) {
        const size_t e = (size_t)ry * (size_t)a.w.x1 + (size_t)rx;
        if (a.depth_vec && (e & 3u) == 0u && rx + 3 < ww) {
            const float4 d = *reinterpret_cast<const float4 *>(a.depth + e);
            m = min(min(box_zkey_depth(d.x), box_zkey_depth(d.y)), min(box_zkey_depth(d.z), box_zkey_depth(d.w)));
        } else {
            for (int k = 0; k < 4 && rx + k < ww; ++k) m = min(m, box_zkey_depth(a.depth[e + k]));
        }
    }
    // a wave holds eight rows of the tile: lane = (y & 7) * 8 + x cell
    m = min(m, (uint32_t)__shfl_xor(m, 8)); m = min(m, (uint32_t)__shfl_xor(m, 16));     // 4 x 4 pixels
    const BoxPyramid &p = a.pyr;
    if ((lane & 24) == 0) p.cells[p.off[2] + (size_t)(ty * 8 + (y >> 2)) * p.lw[2] + (tx * 8 + (i & 7))] = m;
    m = min(m, (uint32_t)__shfl_xor(m, 1)); m = min(m, (uint32_t)__shfl_xor(m, 32));     // 8 x 8
    if ((lane & 57) == 0) {
        const int cx = (lane >> 1) & 3;
        p.cells[p.off[3] + (size_t)(ty * 4 + wv) * p.lw[3] + (tx * 4 + cx)] = m;
        s3[wv][cx] = m;
    }
    __syncthreads();
    if (i < 4) {
        const int cx = i & 1, cy = i >> 1;
        const uint32_t v = min(min(s3[2 * cy][2 * cx], s3[2 * cy][2 * cx + 1]), min(s3[2 * cy + 1][2 * cx], s3[2 * cy + 1][2 * cx + 1]));
        p.cells[p.off[4] + (size_t)(ty * 2 + cy) * p.lw[4] + (tx * 2 + cx)] = v;
        uint32_t t = min(v, (uint32_t)__shfl_xor(v, 1));
        t = min(t, (uint32_t)__shfl_xor(t, 2));
        if (i == 0) p.cells[p.off[5] + (size_t)ty * p.lw[5] + tx] = t;
    }
}
// one wave per cell of the levels 6 .. top: the minimum of the level-5 cells under it
__global__ __launch_bounds__(256) void k_box_top(BoxArgs a)
{
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;
    const BoxPyramid &p = a.pyr;
    const int lane = threadIdx.x & 63;
    uint32_t cell = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (cell >= p.top_cells) return;   // (wave-uniform)
    int s = BOX_LEVEL_TILE + 1;
    while (s < p.top && cell >= p.lw[s] * p.lh[s]) { cell -= p.lw[s] * p.lh[s]; ++s; }
    const int k = s - BOX_LEVEL_TILE;
    const uint32_t cx = cell % p.lw[s], cy = cell / p.lw[s];
    const uint32_t bx0 = cx << k, by0 = cy << k;
    const uint32_t bw = min((uint32_t)a.tiles_x - bx0, 1u << k), bh = min((uint32_t)a.tiles_y - by0, 1u << k);
    uint32_t m = 0xFFFFFFFFu;
    for (uint32_t e = (uint32_t)lane; e < bw * bh; e += 64u) m = min(m, p.cells[p.off[5] + (size_t)(by0 + e / bw) * p.lw[5] + (bx0 + e % bw)]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor(m, o));
    if (lane == 0) p.cells[p.off[s] + (size_t)cy * p.lw[s] + cx] = m;
}

// ---- the test -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ BoxReduce box_group_reduce(BoxReduce r)
{
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        BoxReduce b;
        b.bad = (uint32_t)__shfl_xor(r.bad, o); b.wmin = __shfl_xor(r.wmin, o); b.nx = __shfl_xor(r.nx, o); b.ny = __shfl_xor(r.ny, o);
        b.sxmin = __shfl_xor(r.sxmin, o); b.sxmax = __shfl_xor(r.sxmax, o); b.symin = __shfl_xor(r.symin, o); b.symax = __shfl_xor(r.symax, o);
        r = box_reduce_join(r, b);
    }
    return r;
}
// 16 lanes per unit: unit u < nitems is item u, the units behind them only zero their entry (every entry is written).
__global__ __launch_bounds__(256) void k_box_test(BoxArgs a)
{
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;
    const int sub = threadIdx.x & 15;
    const unsigned long long units = a.out_entries > a.nitems ? a.out_entries : (unsigned long long)a.nitems;
    const BoxOwnRows own = {a.own};
    // (the trip count is the same for the 16 lanes of a group, and for a whole wave where it matters: the shuffles below stay
    // inside a group, whose lanes are all in the loop together)
    for (unsigned long long u = (unsigned long long)blockIdx.x * 16u + (threadIdx.x >> 4); u < units; u += (unsigned long long)gridDim.x * 16u) {
        if (u >= a.nitems) { if (sub == 0 && u < a.out_entries) a.out[u] = 0u; continue; }
        float model[16], mvp[16], b[6], E[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 f = reinterpret_cast<const float4 *>(a.models + (size_t)u * 16)[k];
            model[4 * k] = f.x; model[4 * k + 1] = f.y; model[4 * k + 2] = f.z; model[4 * k + 3] = f.w;
        }
        box_mvp(a.pv.m, model, mvp);
#pragma unroll
        for (int k = 0; k < 6; ++k) b[k] = a.lo_hi[(size_t)u * 6 + k];
        box_error(mvp, b, E);
        const BoxReduce red = box_group_reduce(box_reduce_one(box_corner(mvp, b, sub & 7, a.w.W, a.w.H), E));
        BoxRect r = box_rect(a.flags[u], E, red, a.w, own, a.window_owned_rows);
        uint32_t dmin = 0xFFFFFFFFu;
        if (r.status == BOX_KEPT) {
            const int s = r.level;
            const uint32_t cx = (uint32_t)(r.rx0 >> s) + (uint32_t)(sub & 3), cy = (uint32_t)(r.ry0 >> s) + (uint32_t)(sub >> 2);
            if (cx <= (uint32_t)(r.rx1 >> s) && cy <= (uint32_t)(r.ry1 >> s) && cx < a.pyr.lw[s] && cy < a.pyr.lh[s])
                dmin = a.pyr.cells[a.pyr.off[s] + (size_t)cy * a.pyr.lw[s] + cx];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) dmin = min(dmin, (uint32_t)__shfl_xor(dmin, o));
        if (r.status == BOX_KEPT && r.zkey < dmin) r.count = 0u;   // HIDDEN
        if (sub == 0 && u < a.out_entries) a.out[u] = r.count;
    }
}
#endif // __HIPCC__

} // namespace frr
