// frr_varyings.h -- the ShaderContext the reference hands to the pixel shader (`input`, renderer.rs:368-378) as a device
// buffer: frr_resolve_varyings writes, for every pixel of a window whose triangle-id entry names a triangle of the latest
// geometry pass, the perspective-correct interpolation of that triangle's varyings at that pixel -- the value shade_pixel (frr_raster.h)
// feeds to run_ps: the same fragment and weights (rec_frag, frag_weights: frr_device.h), the sums in the same association (vary_sums).
//
// The triangle-id target holds emission indices; the records and varyings live at SLOTS (frr_device.h: slots and order
// keys).  slot_of_emission finds a slot with two binary searches of dependent loads, which is wrong once per pixel, so
// the command is two launches:
//   k_vary_slots     one thread per used setup slot: table[emission index within the draw] = slot
//   k_vary_resolve   one thread per window pixel: id -> range test -> table -> record, varyings -> K sums -> store
// No LDS, no atomics.  Included by frr_api.hip only (not part of the text embedded for user shaders).
#pragma once
#include "frr_kernels.h"

namespace frr {

struct VaryArgs {
    int32_t x0, x1, y0, y1;           // the window of the raster passes (depth index (cy - y0) * x1 + (cx - x0), renderer.rs:362; x0 >= 0)
    int32_t K;                        // varyings per vertex of the geometry pass
    const RasterRec *recs;            // [setup_cap] the pass's setup list ...
    const float *vary;                // [setup_cap][3][K]
    const uint32_t *tinfo, *fan_okey, *block_prefix;   // ... and its id tables (GeomArgs)
    uint32_t *table;                  // [setup_cap] emission index within the draw -> slot
    uint32_t setup_cap, fan_cap;
    uint32_t ntris;                   // input triangles of the pass as the host knows them (the tables are sized by it)
    int32_t gpar, lane;               // whose Counters::gtab holds the pass's tri_base, n_emit, input count and fan cursors
    RowOwner own;                     // tile-row ownership over the window's tile rows
    uint32_t seq, epoch;              // the command's sequence number (Counters::first_bad)
    const Counters *cnt;
    const uint32_t *tri_id;           // the frame's triangle-id target
    float *out;                       // [entries][K], pixel-major
};

constexpr int VARY_WG = 256;

// One thread per used setup slot: the inputs that emit exactly one triangle (they live at their own slot) and the used
// part of every fan region (FanMap, as lines_walk<true> walks them).  The emission index comes from the record's flags
// word, as in emission_id_rec (frr_raster.h).
__global__ __launch_bounds__(VARY_WG) void k_vary_slots(VaryArgs a)
{
    // a failed earlier command cancels this one (the host replays both): the tables it would read are not there
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;
    const FanMap fm = fan_map(&a.cnt->lane[a.lane].gtab[a.gpar], a.fan_cap);
    const uint32_t total = fan_map_total(fm);
    if (fm.ntris == 0u || fm.ntris != a.ntris) return;   // (the second: a guard for the machine -- the tables are the pass's own)
    for (uint64_t v0 = (uint64_t)blockIdx.x * VARY_WG + threadIdx.x; v0 < total; v0 += (uint64_t)gridDim.x * VARY_WG) {
        const uint32_t v = (uint32_t)v0;
        const bool fan = v >= fm.ntris;
        if (!fan && (a.tinfo[v] & ((1u << FAN_BITS) - 1u)) != 1u) continue;
        const uint32_t slot = fan ? fan_map_slot(fm, v) : v;
        if (slot >= a.setup_cap) continue;                  // (guards for the machine: a consistent pass never takes them)
        const uint32_t t = fan ? min(a.fan_okey[slot - fm.ntris] >> FAN_BITS, fm.ntris - 1u) : slot;
        const uint32_t e = a.block_prefix[t / GEOM_BLOCK] + ((a.recs[slot].flags >> REC_EOFF_SHIFT) & REC_EOFF_MASK);
        if (e < a.setup_cap) a.table[e] = slot;
    }
}

// N consecutive varyings of one pixel: out[k] = i0[k] * c0 + i1[k] * c1 + i2[k] * c2 (renderer.rs:374-378), k < N.  Every load
// is issued before the first store (the compiler cannot know that the caller's buffer overlaps nothing it reads).
// VEC (N a multiple of 4): v + j * K and o are 16-byte aligned.
template <int N, bool VEC> __device__ __forceinline__ void vary_sums(const float *v, int K, float c0, float c1, float c2, float *o)
{
    float p[3][N], s[N];
    if constexpr (VEC) {
        for (int j = 0; j < 3; ++j)
            for (int q = 0; q < N / 4; ++q) {
                const float4 x = *reinterpret_cast<const float4 *>(v + j * K + 4 * q);
                p[j][4 * q] = x.x; p[j][4 * q + 1] = x.y; p[j][4 * q + 2] = x.z; p[j][4 * q + 3] = x.w;
            }
    } else {
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < N; ++k) p[j][k] = v[j * K + k];
    }
    for (int k = 0; k < N; ++k) s[k] = p[0][k] * c0 + p[1][k] * c1 + p[2][k] * c2;
    if constexpr (VEC) {
        for (int q = 0; q < N / 4; ++q) *reinterpret_cast<float4 *>(o + 4 * q) = make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
    } else {
        for (int k = 0; k < N; ++k) o[k] = s[k];
    }
}

// One thread per window pixel, a workgroup per run of VARY_WG pixels of one row: the id loads and the K * 4-byte stores of
// a wavefront are contiguous.  KT: K at compile time (the shader table's 3 and 8), or 0: a.K (user shaders).  VEC: K is a
// multiple of 4 and the caller's buffer is 16-byte aligned, so every pixel's entry is (the varyings of a slot start at a
// multiple of 48 bytes then): 16-byte loads and stores; else scalar ones.  The host decides: it is the same for all pixels.
template <int KT, bool VEC> __global__ __launch_bounds__(VARY_WG) void k_vary_resolve(VaryArgs a)
{
    const int K = KT > 0 ? KT : a.K;
    const int cx = a.x0 + (int)(blockIdx.x * VARY_WG + threadIdx.x), ry = (int)blockIdx.y, cy = a.y0 + ry;
    if (cx >= a.x1) return;
    if (a.own.world > 1 && !owns_tile_row(ry / TILE, a.own)) return;
    // behind a failed command the ids are stale (the cancelled draw never wrote its own): nothing is written, and the
    // replay runs this command again in its place
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;
    const GeomTab *gt = &a.cnt->lane[a.lane].gtab[a.gpar];
    const size_t i = (size_t)ry * (size_t)a.x1 + (size_t)(cx - a.x0);          // :362
    const uint32_t e = a.tri_id[i] - gt->tri_base;
    if (e >= gt->n_emit || e >= a.setup_cap) return;                           // not a triangle of this pass (or nothing drawn: ~0)
    const uint32_t t = min(a.table[e], a.setup_cap - 1u);                      // (a guard for the machine)
    const RecFrag rf = rec_frag(a.recs + t, cx, cy);                           // :343-360
    const float3 cw = frag_weights(rf.f, rf.r0, rf.r1, rf.r2);                 // :368-372
    const float *v = a.vary + (size_t)t * (size_t)(3 * K);
    float *o = a.out + i * (size_t)K;
    if constexpr (KT > 0) {
        vary_sums<KT, VEC>(v, K, cw.x, cw.y, cw.z, o);
    } else {
        int k = 0;
        for (; k + 4 <= K; k += 4) vary_sums<4, VEC>(v + k, K, cw.x, cw.y, cw.z, o + k);
        for (; k < K; ++k) vary_sums<1, false>(v + k, K, cw.x, cw.y, cw.z, o + k);
    }
}

} // namespace frr
