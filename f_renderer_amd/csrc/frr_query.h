// frr_query.h -- frr_query_pixels: the occlusion query.  Loop B (renderer.rs:269-384) over the triangles of the latest geometry
// pass with every store taken out: per item of the pass, or per triangle of the frame, the number of fragments for which
// `rhw < depth[i]` (:363) is false against the depth target AS IT STANDS -- nothing is written, so every fragment meets the
// same stored value.
//
// The command is a raster command (exec_raster: binning, verification, replay, the partition's grid) with k_query in the tile
// kernel's place: one workgroup per owned tile, in a shape of kSpanShapes.
//   depth      the tile's 32 x 32 depths in LDS as f32, one coalesced load; pixels of a partial tile outside the window are
//              never addressed (every box is clamped to the window)
//   records    through TileSource, segmented or CSR, CULL per wave step; nothing is sorted and nothing copied to bins2
//   skip       a record whose depth bound (cull_zub) lies strictly below the smallest depth key of the tile has no fragment
//              that passes: skipped whole.  Exact: ties do not skip, a NaN depth has the lowest key and disables it,
//              all-ones bounds are never below anything.  The same bound against the minima of the row's 4-pixel cells
//              shrinks a span (span_row_window); the depth never changes here, so the cells are built once.
//   coverage   exact row spans from the integer edge functions (SpanTri, span_edge_bound), fragments packed 64 to a step across
//              rows and across the triangles of a step, as k_raster_span packs them; windows and records outside SPAN_SAFE
//              (and FRR_RASTER=sweep) take the brute-force sweep, exact under wrapping arithmetic
//   counting   per step the ballot of fragment_passes; the fragments of one triangle are consecutive, so the first lane of
//              each run adds the run's share to the triangle's staging slot.  After the step a triangle with a non-zero count
//              finds its unit -- per item with the boundary search of frr_visible.h over the table k_visible_prep built --
//              and adds once: into the LDS histogram (flushed with one global add per non-zero bin) or to global memory.
// Integer adds only: the bytes do not depend on the order in which they arrive.
#pragma once
#include "frr_raster.h"
#include "frr_visible.h"
#include "frr_rules.h"

namespace frr {

struct QueryArgs {
    int32_t unit;                     // frr_visible_unit
    uint32_t nitems;                  // FRR_PER_ITEM: the items of the pass
    const uint32_t *bounds;           // [nitems + 1] k_visible_prep's table: the ids of item k are [bounds[k], bounds[k + 1])
    uint32_t *out;                    // [out_entries], zeroed by k_visible_prep
    unsigned long long out_entries;
    int32_t sweep_all;                // every record takes the brute-force sweep (option raster_sweep)
};

template <int NW, int B, bool HIST> struct QueryLds {
    static constexpr int WAVES = NW, BATCH = B;
    static constexpr int DEPTH = 0;                        // float[TILE_PX]
    static constexpr int TRI = DEPTH + TILE_PX * 4;        // SpanTri[NW][B] (pad: rhw of the third vertex)
    static constexpr int FA = TRI + NW * B * 48;           // float4[NW][B]  s0x s0y s1x s1y
    static constexpr int FB = FA + NW * B * 16;            // float4[NW][B]  s2x s2y rhw0 rhw1
    static constexpr int CNT = FB + NW * B * 16;           // u32[NW][B]     passing fragments of the staged triangle
    static constexpr int HROW = CNT + NW * B * 4;          // u64[NW][B/2]
    static constexpr int HFRAG = HROW + NW * (B / 2) * 8;  // u64[NW][32]
    static constexpr int Q = HFRAG + NW * 32 * 8;          // u32[NW][64]
    static constexpr int SEGPRE = Q + NW * 64 * 4;         // u32[BIN_MAX_G + 1]
    static constexpr int SEGSRC = SEGPRE + ((BIN_MAX_G + 1 + 3) & ~3) * 4; // u32[BIN_MAX_G]
    static constexpr int HZ = SEGSRC + BIN_MAX_G * 4;      // u32[HZ_SIZE]: only the cells [HZ_C4 ..) are used
    static constexpr int SCAL = HZ + ((HZ_SIZE + 3) & ~3) * 4; // u32[4]: next, tmin
    static constexpr int HISTO = SCAL + 4 * 4;             // u32[VIS_LDS_BINS]
    static constexpr int BYTES = HISTO + (HIST ? (int)VIS_LDS_BINS * 4 : 0);
    static_assert(B <= 32 && BYTES <= 64 * 1024 && HZ % 16 == 0, "staging slots are five bits of a span descriptor; static LDS");
    template <class T> static __device__ __forceinline__ T *at(unsigned char *lds, int off) { return reinterpret_cast<T *>(lds + off); }
    static __device__ __forceinline__ float *depth(unsigned char *lds) { return at<float>(lds, DEPTH); }
    static __device__ __forceinline__ auto tri(unsigned char *lds) { return at<SpanTri[B]>(lds, TRI); }
    static __device__ __forceinline__ auto fa(unsigned char *lds) { return at<float4[B]>(lds, FA); }
    static __device__ __forceinline__ auto fb(unsigned char *lds) { return at<float4[B]>(lds, FB); }
    static __device__ __forceinline__ auto cnt(unsigned char *lds) { return at<uint32_t[B]>(lds, CNT); }
    static __device__ __forceinline__ auto hrow(unsigned char *lds) { return at<unsigned long long[B / 2]>(lds, HROW); }
    static __device__ __forceinline__ auto hfrag(unsigned char *lds) { return at<unsigned long long[32]>(lds, HFRAG); }
    static __device__ __forceinline__ auto q(unsigned char *lds) { return at<uint32_t[64]>(lds, Q); }
    static __device__ __forceinline__ uint32_t *segpre(unsigned char *lds) { return at<uint32_t>(lds, SEGPRE); }
    static __device__ __forceinline__ uint32_t *segsrc(unsigned char *lds) { return at<uint32_t>(lds, SEGSRC); }
    static __device__ __forceinline__ uint32_t *hz(unsigned char *lds) { return at<uint32_t>(lds, HZ); }
    static __device__ __forceinline__ uint32_t &next(unsigned char *lds) { return *at<uint32_t>(lds, SCAL); }
    static __device__ __forceinline__ uint32_t &tmin(unsigned char *lds) { return *at<uint32_t>(lds, SCAL + 4); }
    static __device__ __forceinline__ uint32_t *hist(unsigned char *lds) { return at<uint32_t>(lds, HISTO); }
};

// Brute-force sweep of ONE triangle (wave-uniform index t) by the whole wave, as sweep_triangle walks it: the number of its
// fragments in this tile that pass (wave-uniform).
__device__ __forceinline__ uint32_t query_sweep(const RasterArgs &a, const TileCtx &c, uint32_t t, int lane, const float *s_depth)
{
    const RasterRec *__restrict__ r = a.recs + t;
    const float s0x = r->s[0], s0y = r->s[1], s1x = r->s[2], s1y = r->s[3], s2x = r->s[4], s2y = r->s[5];
    const SweepSetup t3 = sweep_setup(r, a);
    const int bx0 = max(t3.bx0, c.ax0), bx1 = min(t3.bx1, c.ax0 + c.tw);
    const int by0 = max(t3.by0, c.ay0), by1 = min(t3.by1, c.ay0 + c.th);
    const int bw = bx1 - bx0, bh = by1 - by0;
    if (bw <= 0 || bh <= 0) return 0u;
    const int npx = bw * bh;
    const uint32_t A01 = t3.A(0), B01 = t3.B(0), A12 = t3.A(1), B12 = t3.B(1), A20 = t3.A(2), B20 = t3.B(2);
    const uint32_t E01o = t3.E(0, bx0, by0), E12o = t3.E(1, bx0, by0), E20o = t3.E(2, bx0, by0);
    const int thr01 = t3.thr(0), thr12 = t3.thr(1), thr20 = t3.thr(2);
    const float r0 = r->rhw[0], r1 = r->rhw[1], r2 = r->rhw[2];
    const float inv_bw = __builtin_amdgcn_rcpf((float)bw);   // (sweep_triangle: exact for p < 1024, bw <= 32)
    uint32_t n = 0u;
    for (int p0 = 0; p0 < npx; p0 += 64) {
        const int p = p0 + lane;
        bool pass = false;
        if (p < npx) {
            const int dy = (int)(((float)p + 0.5f) * inv_bw);
            const int dx = p - __mul24(dy, bw);
            const int E01 = (int)(E01o + A01 * (uint32_t)dx + B01 * (uint32_t)dy);
            const int E12 = (int)(E12o + A12 * (uint32_t)dx + B12 * (uint32_t)dy);
            const int E20 = (int)(E20o + A20 * (uint32_t)dx + B20 * (uint32_t)dy);
            if ((E01 > thr01) & (E12 > thr12) & (E20 > thr20)) {
                const int cx = bx0 + dx, cy = by0 + dy;
                const Frag f = frag_eval(s0x, s0y, s1x, s1y, s2x, s2y, r0, r1, r2, cx, cy);
                pass = f.valid && fragment_passes(f.rhw, s_depth[(cy - c.ay0) * TILE + (cx - c.ax0)]);
            }
        }
        n += (uint32_t)__popcll(__ballot(pass));
    }
    return n;
}

// The lanes with `has` add n to the unit of the triangle with frame-global emission index e.  Called by the whole wave.
template <bool ITEM, bool HIST, class L>
__device__ __forceinline__ void query_add(const QueryArgs &qa, unsigned char *lds, uint32_t limit, bool has, uint32_t e, uint32_t n)
{
    uint32_t unit;
    if constexpr (ITEM) {
        const uint32_t mn = vis_wave_min(has ? e : VIS_NONE), mx = vis_wave_max(has ? e : 0u);
        if (mn == VIS_NONE) return;   // (wave-uniform)
        const VisRange r = vis_span_range(qa.bounds, qa.nitems, mn, mx);
        unit = vis_item_unit(qa.bounds, r, e, has, limit);
    } else {
        unit = has ? vis_tri_unit(e, limit) : VIS_NONE;
    }
    if (unit == VIS_NONE) return;
    if constexpr (HIST) atomicAdd(&L::hist(lds)[unit], n);
    else atomicAdd(&qa.out[unit], n);
}

// ITEM: per item (else per triangle).  HIST: the units fit the LDS histogram (the host decides; per item only).
template <bool ITEM, bool HIST, int NW>
__global__ __launch_bounds__(NW * 64) void k_query(RasterArgs a, QueryArgs qa, int win_safe)
{
    constexpr int B = NW >= 16 ? 16 : SPAN_BATCH;
    constexpr int CULL = SPAN_CULL < B ? SPAN_CULL : B;
    constexpr int NT = NW * 64;
    using L = QueryLds<NW, B, HIST>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[L::BYTES];
    // this or an earlier command failed: nothing is counted, the host replays (the zeros are k_visible_prep's, cancelled alike)
    if (seq_cancelled(a.cnt, a.seq, a.epoch, true)) return;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    TileCtx c = tile_ctx(a);
    const bool segmented = a.nseg != 0;
    if (segmented) {
        // column c.ltile of the segment table -> where each chunk's records of this tile start, and how many lie before them
        for (uint32_t g = threadIdx.x; g < (uint32_t)BIN_MAX_G; g += NT) {
            uint32_t s0 = 0u, cn = 0u;
            if (g < a.nseg) {
                const uint32_t *r = a.seg + (size_t)g * ((size_t)gridDim.x + 1) + c.ltile;   // (grid = the rank's tiles)
                s0 = r[0];
                cn = r[1] - s0;
            }
            L::segsrc(lds)[g] = s0;
            L::segpre(lds)[g] = cn;
        }
        __syncthreads();
        if (w == 0) {
            static_assert(BIN_MAX_G == 256, "four segments per lane of one wave");
            uint32_t v[4], sum = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = L::segpre(lds)[lane * 4 + j]; sum += v[j]; }
            uint32_t run = wave_incl_scan_dpp(sum) - sum;
#pragma unroll
            for (int j = 0; j < 4; ++j) { L::segpre(lds)[lane * 4 + j] = run; run += v[j]; }
            if (lane == 63) L::segpre(lds)[BIN_MAX_G] = run;
        }
        __syncthreads();
        c.beg = 0u;
        c.end = __builtin_amdgcn_readfirstlane(L::segpre(lds)[BIN_MAX_G]);
    }
    if (c.beg >= c.end) return;   // nothing binned here
    const uint32_t nent = c.end - c.beg;
    // ---- the tile's depth, the minima of its 4-pixel cells (as keys >> 1: span_row_window) and of the whole tile ----
    if (threadIdx.x == 0) { L::next(lds) = 0u; L::tmin(lds) = 0xFFFFFFFFu; }
    for (int i = threadIdx.x; i < TILE_PX; i += NT) {
        const int x = i & (TILE - 1), y = i >> 5;
        L::depth(lds)[i] = x < c.tw && y < c.th ? a.depth[(size_t)(c.ly0 + y) * a.dstride + (c.lx0 + x)] : 0.0f;
    }
    const uint32_t tri_base = gtab_of(a)->tri_base;
    uint32_t limit;
    if constexpr (ITEM) limit = (uint32_t)min((unsigned long long)qa.nitems, qa.out_entries);
    else limit = (uint32_t)min(min((unsigned long long)tri_base + gtab_of(a)->n_emit, qa.out_entries), 0xFFFFFFFFull);
    if constexpr (HIST) {
        limit = min(limit, VIS_LDS_BINS);   // (a guard for the machine: the host takes this path only where the units fit)
        for (uint32_t b = threadIdx.x; b < limit; b += NT) L::hist(lds)[b] = 0u;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TILE_PX / 4; i += NT) {
        const int y = i >> 3, x = (i & 7) * 4;
        const float4 d = reinterpret_cast<const float4 *>(L::depth(lds))[i];
        const float dv[4] = {d.x, d.y, d.z, d.w};
        uint32_t m = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (x + k < c.tw && y < c.th) m = min(m, zkey_depth(dv[k]));
        L::hz(lds)[HZ_C4 + i] = m >> 1;
        atomicMin(&L::tmin(lds), m);
    }
    __syncthreads();
    const uint32_t tmin = __builtin_amdgcn_readfirstlane(L::tmin(lds));
    const TileSource source = {a, c, segmented, L::segpre(lds), L::segsrc(lds)};
    const bool sweep_all = qa.sweep_all != 0 || !win_safe;
    const uint32_t le_lo = lane < 32 ? (2u << lane) - 1u : 0xFFFFFFFFu;
    const uint32_t le_hi = lane < 32 ? 0u : (2u << (lane - 32)) - 1u;
    SpanDbg dbg;
    uint32_t n_cov = 0u;   // (span_row_window's, not counted: COUNT = false)
    for (;;) {
        // ---- lane = record, CULL per step ----
        uint32_t b = 0u;
        if (lane == 0) b = atomicAdd(&L::next(lds), 1u);
        b = __builtin_amdgcn_readfirstlane(b);
        const uint32_t e0 = b * (uint32_t)CULL;
        if (e0 >= nent) break;
        const bool valid = lane < (int)min((uint32_t)CULL, nent - e0);
        const uint4 en = valid ? source(e0 + (uint32_t)lane) : make_uint4(0, 0, 0, 0);
        const int mnx = (int)(short)(en.z & 0xFFFFu), mny = (int)(short)(en.z >> 16);
        const int mxx = (int)(short)(en.w & 0xFFFFu), mxy = (int)(short)(en.w >> 16);
        // the clamped box (renderer.rs:285-298) in this tile, as span_cull forms it
        const int bx0 = max(clampi(mnx, a.x0, a.x1), c.ax0), bx1 = min(clampi(mxx, a.x0, a.x1), c.ax0 + c.tw);
        const int by0 = max(clampi(mny, a.y0, a.y1), c.ay0), by1 = min(clampi(mxy, a.y0, a.y1), c.ay0 + c.th);
        // en.y < tmin: every fragment's rhw lies below every depth of the tile -- none passes
        const bool live = valid && bx1 > bx0 && by1 > by0 && !(en.y < tmin);
        const int amax = max(max(abs(mnx), abs(mxx)), max(abs(mny), abs(mxy)));
        const bool alive = live && !sweep_all && amax <= SPAN_SAFE;
        unsigned long long um = __ballot(live && !alive);
        while (um) {
            const int src = __builtin_ctzll(um);
            um &= um - 1;
            const uint32_t tu = (uint32_t)__builtin_amdgcn_readlane((int)en.x, src);
            const uint32_t n = query_sweep(a, c, tu, lane, L::depth(lds));
            if (n) query_add<ITEM, HIST, L>(qa, lds, limit, lane == 0, tri_base + emission_id(a, tu) - 1u, n);   // (n is wave-uniform)
        }
        const unsigned long long am = __ballot(alive);
        if (am == 0ull) continue;
        // ---- a survivor stages its edge data at its rank among the survivors (k_raster_span, step 1b) ----
        const int trank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));
        const uint32_t rows = alive ? (uint32_t)(by1 - by0) : 0u;
        const uint32_t rincl = wave_incl_scan_dpp(rows);
        uint32_t emis = 0u;
        if (alive) {
            const uint4 *rp = reinterpret_cast<const uint4 *>(a.recs + en.x);
            const uint4 q0 = rp[0], q1 = rp[1], q2 = rp[2], q3 = rp[3];
            auto m_of = [&](uint32_t kd, uint32_t cc) { return (int)cc + __mul24((int)(kd << 16) >> 16, by0) - __mul24((int)(kd >> 16), bx0); };
            auto r_of = [&](uint32_t kd) { return fminf(__builtin_amdgcn_rcpf((float)(kd >> 16)), 64.0f); };
            SpanTri t;
            t.m01 = m_of(q0.x, q0.y); t.m12 = m_of(q0.z, q0.w); t.m20 = m_of(q1.x, q1.y);
            t.zub = en.y;
            t.kd01 = q0.x; t.kd12 = q0.z; t.kd20 = q1.x;
            t.misc = (uint32_t)(bx0 - c.ax0) | ((uint32_t)(by0 - c.ay0) << 5) | ((uint32_t)(bx1 - bx0) << 10) |
                     (((q3.w >> REC_POS_SHIFT) & 7u) << 16) | ((rincl - rows) << 19);
            t.r01 = r_of(q0.x); t.r12 = r_of(q0.z); t.r20 = r_of(q1.x);
            t.pad = u2f(q3.z);                   // rhw of the third vertex
            L::tri(lds)[w][trank] = t;
            L::fa(lds)[w][trank] = make_float4(u2f(q1.z), u2f(q1.w), u2f(q2.x), u2f(q2.y));
            L::fb(lds)[w][trank] = make_float4(u2f(q2.z), u2f(q2.w), u2f(q3.x), u2f(q3.y));
            L::cnt(lds)[w][trank] = 0u;
            emis = tri_base + emission_id_rec(a, en.x, q3.w) - 1u;
        }
        const int R = (int)__builtin_amdgcn_readlane((int)rincl, 63);
        if (lane < B / 2) L::hrow(lds)[w][lane] = 0ull;
        wave_lds_fence();
        if (rows) {
            const uint32_t st = rincl - rows;
            atomicOr(reinterpret_cast<uint32_t *>(&L::hrow(lds)[w][0]) + (st >> 5), 1u << (st & 31));
        }
        wave_lds_fence();
        const unsigned long long hrow_mine = L::hrow(lds)[w][lane & (B / 2 - 1)];
        wave_lds_fence();
        int jbase = 0;
        for (int r0 = 0; r0 < R; r0 += 64) {
            const RowWindow rw = span_row_window<false, L>(lds, R, hrow_mine, r0, lane, w, le_lo, le_hi, jbase, n_cov, dbg);
            if (!rw.any) continue;
            int qbase = 0;
            // ---- lane = fragment: rhw with the tile kernel's arithmetic, the depth test, the count ----
            for (int f0 = 0; f0 < rw.F; f0 += 64) {
                const uint32_t g_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)rw.hfrag_mine, f0 >> 6);
                const uint32_t g_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(rw.hfrag_mine >> 32), f0 >> 6);
                const bool in_f = f0 + lane < rw.F;
                bool pass = false;
                uint32_t sj = 64u;   // (no staging slot: a lane behind the last fragment is a run of its own)
                if (in_f) {
                    const uint32_t d = L::q(lds)[w][seg_rank(g_lo, g_hi, le_lo, le_hi, qbase - 1)];
                    sj = d & 31u;
                    const int y = (int)((d >> 5) & 31u), x = (int)(d >> 10) + (f0 - 2048) + lane;
                    const float4 fa = L::fa(lds)[w][sj], fb = L::fb(lds)[w][sj];
                    const float r2 = L::tri(lds)[w][sj].pad;
                    const Frag f = frag_eval(fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w, r2, c.ax0 + x, c.ay0 + y);
                    pass = f.valid && fragment_passes(f.rhw, L::depth(lds)[y * TILE + x]);
                }
                const unsigned long long pm = __ballot(pass);
                if (pm != 0ull) {   // (wave-uniform)
                    // the fragments of a triangle are consecutive: the first lane of each run adds the run's passing fragments
                    const uint32_t left = (uint32_t)__shfl_up(sj, 1);
                    const bool head = vis_is_head(sj, left, lane);
                    const unsigned long long heads = __ballot(head);
                    if (head && in_f) {
                        const uint32_t len = vis_run_len(heads, lane);
                        const unsigned long long run = (len >= 64u ? ~0ull : (1ull << len) - 1ull) << lane;
                        const uint32_t n = (uint32_t)__popcll(pm & run);
                        if (n) atomicAdd(&L::cnt(lds)[w][sj], n);
                    }
                }
                qbase += __popc(g_lo) + __popc(g_hi);
            }
            wave_lds_fence(); // the span queue and the fragment heads are rewritten by the next row window
        }
        wave_lds_fence();
        // ---- one add per triangle of the step with a non-zero count ----
        const uint32_t n = alive ? L::cnt(lds)[w][trank] : 0u;
        query_add<ITEM, HIST, L>(qa, lds, limit, n != 0u, emis, n);
        wave_lds_fence(); // staging is rewritten by the next step
    }
    if constexpr (HIST) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < limit; b += NT) {
            const uint32_t v = L::hist(lds)[b];
            if (v) atomicAdd(&qa.out[b], v);
        }
    }
}

} // namespace frr
