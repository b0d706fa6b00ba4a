// frr_visible.h -- frr_visible_pixels: how many entries of a window each item of the latest geometry pass (or each triangle
// of the frame) owns in the triangle-id target.  A histogram of the ids -- per triangle of the ids themselves, per item of
// the item whose id range [bounds[k], bounds[k + 1]) holds the id -- in integer adds only, so the bytes do not depend on
// the order in which the adds arrive.
//
// Ids come in runs along a row, so nothing is added per pixel.  A wavefront takes a SPAN, 64 consecutive entries of one
// row, finds each lane's unit, and only the first lane of every run of equal units (a run HEAD) adds the run's length:
//   unit       per triangle the id; per item a binary search of the nitems + 1 boundaries, narrowed to the items of the
//              span's smallest and largest id (ids are not monotonic along a row, the boundaries are: every id between
//              the two lies in an item between theirs) -- one item for most spans, and then no lane searches at all
//   run heads  lane 0, and every lane whose unit differs from its left neighbour's (one cross-lane compare)
//   run length the distance to the next head in the ballot of the heads
// Two launches make the command:
//   k_visible_prep   out[0 .. out_entries) = 0, and per item bounds[i] = tri_base + what k_item_firsts computes
//   k_visible        a workgroup walks `rows` window rows; where the units fit VIS_LDS_BINS the heads add into an LDS
//                    histogram that is flushed with one global add per non-zero bin, else they add to global memory; the
//                    boundaries of a pass of at most VIS_LDS_BINS items are searched in an LDS copy
// The span logic (vis_*) also compiles for the host with no HIP at all: frr_host_visible_counts and tests/visible_host.cpp
// run visible_counts_host, which walks the spans as the kernel does, lane by lane.
// The search functions (vis_item_search .. vis_item_unit, vis_wave_min / vis_wave_max) are also what frr_shade_items finds a
// pixel's item with (frr_shade.h: k_shade_items), so this file is part of the text embedded for user shaders: under hiprtc
// only those functions remain, the kernels and the host walks of this command are left out.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#include "frr_kernels.h"
#define FRR_VIS_HD FRR_HD
#else
#define FRR_VIS_HD inline
#endif

namespace frr {

constexpr uint32_t VIS_NONE = 0xFFFFFFFFu;   // a lane that counts for nobody (nothing drawn, another pass's id, a unit >= out_entries, past the row's end)
constexpr int VIS_SPAN = 64;                 // entries per span: one per lane
constexpr uint32_t VIS_LDS_BINS = 4096;      // units the LDS histogram takes: 16 KiB, and as much again for the boundaries per item

// The item k in [lo, hi] with bounds[k] <= id < bounds[k + 1], given bounds[lo] <= id < bounds[hi + 1]: the LAST k whose
// boundary is not behind id.  An item that emitted nothing has bounds[k] == bounds[k + 1] and is never the answer.
FRR_VIS_HD uint32_t vis_item_search(const uint32_t *bounds, uint32_t lo, uint32_t hi, uint32_t id)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (bounds[mid] <= id) lo = mid; else hi = mid - 1u;
    }
    return lo;
}
// is id one of the pass's, whose ids are [b0, bn)?  (0xFFFFFFFF, nothing drawn, never is: bn - b0 <= 0xFFFFFFFF - b0)
FRR_VIS_HD bool vis_in_pass(uint32_t id, uint32_t b0, uint32_t bn) { return id != VIS_NONE && id - b0 < bn - b0; }
// The items a span can meet: those of its smallest and its largest in-pass id (mn <= mx, both in the pass; nitems >= 1).
struct VisRange { uint32_t lo, hi; };
FRR_VIS_HD VisRange vis_span_range(const uint32_t *bounds, uint32_t nitems, uint32_t mn, uint32_t mx)
{
    VisRange r;
    r.lo = vis_item_search(bounds, 0u, nitems - 1u, mn);
    r.hi = mx < bounds[r.lo + 1u] ? r.lo : vis_item_search(bounds, r.lo, nitems - 1u, mx);
    return r;
}
// a lane's unit per item (in_pass: vis_in_pass of its id) and per triangle; units >= limit are counted nowhere
FRR_VIS_HD uint32_t vis_item_unit(const uint32_t *bounds, VisRange r, uint32_t id, bool in_pass, uint32_t limit)
{
    if (!in_pass) return VIS_NONE;
    const uint32_t k = r.lo == r.hi ? r.lo : vis_item_search(bounds, r.lo, r.hi, id);
    return k < limit ? k : VIS_NONE;
}
FRR_VIS_HD uint32_t vis_tri_unit(uint32_t id, uint32_t limit) { return id < limit ? id : VIS_NONE; }
// is `lane` the head of a run?  (left: the unit of lane - 1)
FRR_VIS_HD bool vis_is_head(uint32_t unit, uint32_t left, int lane) { return lane == 0 || unit != left; }
// the length of the run that starts at head `lane`: up to the next head, or to the span's end
FRR_VIS_HD uint32_t vis_run_len(unsigned long long heads, int lane)
{
    const unsigned long long above = lane >= VIS_SPAN - 1 ? 0ull : heads >> (lane + 1);
    return above ? (uint32_t)__builtin_ctzll(above) + 1u : (uint32_t)(VIS_SPAN - lane);
}

#ifndef __HIPCC_RTC__
// The counts of a window of an id array on the host, span by span and lane by lane as k_visible takes them.  bounds: the
// nunits + 1 item boundaries, or null: per triangle, the units are the ids 0 .. nunits.  Every entry of out is written.
// Returns the number of adds (run heads that count for a unit).  The caller has checked the window against the array.
inline uint64_t visible_counts_host(const uint32_t *ids, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                                    const uint32_t *bounds, uint64_t nunits, uint32_t *out, uint64_t out_entries)
{
    for (uint64_t k = 0; k < out_entries; ++k) out[k] = 0u;
    const uint32_t limit = (uint32_t)(nunits < out_entries ? nunits : out_entries);
    if (limit == 0u) return 0;
    const uint32_t nitems = (uint32_t)nunits;
    const uint32_t b0 = bounds ? bounds[0] : 0u, bn = bounds ? bounds[nitems] : 0u;
    const int64_t ww = (int64_t)x1 - x0, wh = (int64_t)y1 - y0;
    uint64_t adds = 0;
    for (int64_t ry = 0; ry < wh; ++ry) {
        for (int64_t c0 = 0; c0 < ww; c0 += VIS_SPAN) {
            uint32_t id[VIS_SPAN], unit[VIS_SPAN];
            uint32_t mn = VIS_NONE, mx = 0u;
            bool any = false;
            for (int l = 0; l < VIS_SPAN; ++l) {
                id[l] = c0 + l < ww ? ids[(uint64_t)ry * (uint64_t)x1 + (uint64_t)(c0 + l)] : VIS_NONE;
                if (bounds && vis_in_pass(id[l], b0, bn)) { any = true; mn = id[l] < mn ? id[l] : mn; mx = id[l] > mx ? id[l] : mx; }
            }
            if (bounds && !any) continue;
            VisRange r = {0u, 0u};
            if (bounds) r = vis_span_range(bounds, nitems, mn, mx);
            for (int l = 0; l < VIS_SPAN; ++l)
                unit[l] = bounds ? vis_item_unit(bounds, r, id[l], vis_in_pass(id[l], b0, bn), limit) : vis_tri_unit(id[l], limit);
            unsigned long long heads = 0ull;
            for (int l = 0; l < VIS_SPAN; ++l) if (vis_is_head(unit[l], l ? unit[l - 1] : VIS_NONE, l)) heads |= 1ull << l;
            for (int l = 0; l < VIS_SPAN; ++l)
                if (((heads >> l) & 1ull) && unit[l] != VIS_NONE) { out[unit[l]] += vis_run_len(heads, l); ++adds; }
        }
    }
    return adds;
}

// The item of every entry of a window of an id array on the host, as k_shade_items (frr_shade.h) finds it: span by span the
// smallest and largest in-pass id, the narrowed range, each lane's search -- and then the rounds of the span, one per
// DISTINCT item its lanes hold, in the order the kernel takes them (the first remaining lane's item).  item_out[i] is written
// for every entry i of the window: the item, or VIS_NONE (nothing drawn, another pass's id).  Returns the number of rounds.
// bounds: the nitems + 1 boundaries, nitems >= 1.  The caller has checked the window against the arrays.
inline uint64_t entry_items_host(const uint32_t *ids, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                                 const uint32_t *bounds, uint32_t nitems, uint32_t *item_out)
{
    const uint32_t b0 = bounds[0], bn = bounds[nitems];
    const int64_t ww = (int64_t)x1 - x0, wh = (int64_t)y1 - y0;
    uint64_t rounds = 0;
    for (int64_t ry = 0; ry < wh; ++ry) {
        for (int64_t c0 = 0; c0 < ww; c0 += VIS_SPAN) {
            uint32_t id[VIS_SPAN], item[VIS_SPAN];
            uint32_t mn = VIS_NONE, mx = 0u;
            for (int l = 0; l < VIS_SPAN; ++l) {
                id[l] = c0 + l < ww ? ids[(uint64_t)ry * (uint64_t)x1 + (uint64_t)(c0 + l)] : VIS_NONE;
                if (vis_in_pass(id[l], b0, bn)) { mn = id[l] < mn ? id[l] : mn; mx = id[l] > mx ? id[l] : mx; }
            }
            VisRange r = {0u, 0u};
            if (mn != VIS_NONE) r = vis_span_range(bounds, nitems, mn, mx);
            for (int l = 0; l < VIS_SPAN; ++l) {
                item[l] = mn == VIS_NONE ? VIS_NONE : vis_item_unit(bounds, r, id[l], vis_in_pass(id[l], b0, bn), nitems);
                if (c0 + l < ww) item_out[(uint64_t)ry * (uint64_t)x1 + (uint64_t)(c0 + l)] = item[l];
            }
            unsigned long long left = 0ull;   // the lanes that still wait for their round
            for (int l = 0; l < VIS_SPAN; ++l) if (item[l] != VIS_NONE) left |= 1ull << l;
            while (left) {
                const uint32_t k = item[__builtin_ctzll(left)];   // (readfirstlane of the remaining lanes)
                for (int l = 0; l < VIS_SPAN; ++l) if (item[l] == k) left &= ~(1ull << l);
                ++rounds;
            }
        }
    }
    return rounds;
}
#endif // !__HIPCC_RTC__

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)

#ifndef __HIPCC_RTC__
struct VisibleArgs {
    int32_t x0, x1, y0, y1;           // the window (depth index (cy - y0) * x1 + (cx - x0), renderer.rs:362; x0 >= 0)
    int32_t unit;                     // frr_visible_unit
    uint32_t nitems;                  // FRR_PER_ITEM: the items of the pass
    const uint32_t *item_first;       // ... of a list pass: their first inputs; else null: `stride` inputs each (k_item_firsts)
    uint32_t stride, ntris;           // ntris: input triangles of the pass as the host knows them (the tables are sized by it)
    const uint32_t *tinfo, *block_prefix;   // the pass's id tables (GeomArgs)
    uint32_t *bounds;                 // [nitems + 1] k_visible_prep -> k_visible: the ids of item k are [bounds[k], bounds[k + 1])
    int32_t gpar, lane;               // whose Counters::gtab holds the pass's tri_base and n_emit
    RowOwner own;                     // tile-row ownership over the window's tile rows
    uint32_t seq, epoch;              // the command's sequence number (Counters::first_bad)
    const Counters *cnt;
    const uint32_t *tri_id;           // the frame's triangle-id target
    uint32_t *out;                    // [out_entries]
    unsigned long long out_entries;
    uint32_t rows;                    // window rows per workgroup of k_visible
};

constexpr int VIS_WG = 256;

// The zeroing, and the item boundaries: both belong to the command, so both obey seq_cancelled -- behind a failed command
// the caller's buffer keeps what it held, and the replay runs this again in its place.
__global__ __launch_bounds__(VIS_WG) void k_visible_prep(VisibleArgs a)
{
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;
    const GeomTab *gt = &a.cnt->lane[a.lane].gtab[a.gpar];
    const uint32_t n_emit = a.ntris ? gt->n_emit : 0u, tri_base = gt->tri_base;
    const unsigned long long nb = a.unit == FRR_PER_ITEM && a.bounds ? (unsigned long long)a.nitems + 1ull : 0ull;
    const unsigned long long total = a.out_entries > nb ? a.out_entries : nb;
    for (unsigned long long i = (unsigned long long)blockIdx.x * VIS_WG + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * VIS_WG) {
        if (i < a.out_entries) a.out[i] = 0u;
        if (i < nb) a.bounds[i] = tri_base + item_first_emission(a.item_first, a.stride, a.nitems, a.ntris, a.tinfo, a.block_prefix, n_emit, (uint32_t)i);
    }
}
#endif // !__HIPCC_RTC__

__device__ __forceinline__ uint32_t vis_wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint32_t vis_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
    return v;
}

#ifndef __HIPCC_RTC__
// ITEM: per item (else per triangle).  LDS: the units fit VIS_LDS_BINS (the host decides: it is the same for all spans).
// BLDS (ITEM only): the pass has at most VIS_LDS_BINS items, and the workgroup searches a copy of the boundaries in LDS -- a
// search is a chain of dependent loads, a dozen for 4,096 items, and from global memory that chain is what a span costs.
// Workgroup b walks the window rows [b * rows, b * rows + rows); its four waves take the spans of those rows in turn.
template <bool ITEM, bool LDS, bool BLDS> __global__ __launch_bounds__(VIS_WG) void k_visible(VisibleArgs a)
{
    __shared__ uint32_t s_hist[LDS ? VIS_LDS_BINS : 1];
    __shared__ uint32_t s_bounds[BLDS ? VIS_LDS_BINS + 1 : 1];
    // behind a failed command the ids are stale (the cancelled draw never wrote its own): nothing is counted
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;
    const GeomTab *gt = &a.cnt->lane[a.lane].gtab[a.gpar];
    uint32_t b0 = 0u, bn = 0u;
    unsigned long long units;
    if constexpr (ITEM) { units = a.nitems; b0 = a.bounds[0]; bn = a.bounds[a.nitems]; }
    else units = (unsigned long long)gt->tri_base + (a.ntris ? gt->n_emit : 0u);
    uint32_t limit = (uint32_t)min(min(units, a.out_entries), 0xFFFFFFFFull);
    if constexpr (LDS) {
        limit = min(limit, VIS_LDS_BINS);   // (a guard for the machine: the host takes this path only where the units fit)
        for (uint32_t b = threadIdx.x; b < limit; b += VIS_WG) s_hist[b] = 0u;
    }
    const uint32_t *bounds = a.bounds;
    if constexpr (BLDS) {
        for (uint32_t b = threadIdx.x; b <= min(a.nitems, VIS_LDS_BINS); b += VIS_WG) s_bounds[b] = a.bounds[b];
        bounds = s_bounds;
    }
    if constexpr (LDS || BLDS) __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t ww = (uint32_t)(a.x1 - a.x0), wh = (uint32_t)(a.y1 - a.y0);
    const uint32_t spr = (ww + VIS_SPAN - 1u) / VIS_SPAN;   // spans per row
    const uint32_t r0 = blockIdx.x * a.rows, r1 = min(r0 + a.rows, wh);
    const uint32_t nspans = r1 > r0 ? (r1 - r0) * spr : 0u;
    for (uint32_t s = (uint32_t)w; s < nspans && limit > 0u; s += VIS_WG / 64) {
        const uint32_t ry = r0 + s / spr, c = (s % spr) * VIS_SPAN + (uint32_t)lane;
        if (a.own.world > 1 && !owns_tile_row((int)ry / TILE, a.own)) continue;
        const uint32_t id = c < ww ? a.tri_id[(size_t)ry * (size_t)a.x1 + c] : VIS_NONE;   // :362
        uint32_t unit;
        if constexpr (ITEM) {
            const bool in = vis_in_pass(id, b0, bn);
            const uint32_t mn = vis_wave_min(in ? id : VIS_NONE), mx = vis_wave_max(in ? id : 0u);
            if (mn == VIS_NONE) continue;   // no lane holds an id of the pass (wave-uniform)
            const VisRange r = vis_span_range(bounds, a.nitems, mn, mx);
            unit = vis_item_unit(bounds, r, id, in, limit);
        } else {
            unit = vis_tri_unit(id, limit);
        }
        const uint32_t left = (uint32_t)__shfl_up(unit, 1);
        const bool head = vis_is_head(unit, left, lane);
        const unsigned long long heads = __ballot(head);
        if (head && unit != VIS_NONE) {
            const uint32_t len = vis_run_len(heads, lane);
            if constexpr (LDS) atomicAdd(&s_hist[unit], len);
            else atomicAdd(&a.out[unit], len);
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < limit; b += VIS_WG) {
            const uint32_t v = s_hist[b];
            if (v) atomicAdd(&a.out[b], v);
        }
    }
}
#endif // !__HIPCC_RTC__

#endif // __HIPCC__

} // namespace frr
