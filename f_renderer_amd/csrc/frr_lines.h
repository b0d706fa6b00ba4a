// frr_lines.h -- FrameBuffer::draw_line (f_renderer/src/renderer.rs:540-588) on the device: lists of
// segments (frr_draw_lines) and the edges of the latest setup list (frr_draw_wireframe).
//
// The reference walks a segment with a running remainder.  The walk has a closed form -- iteration i of `major` paints
// the minor coordinate m0 + floor(i * minor / major), and m0 + floor((i + 1) * minor / major) as well when that is larger;
// one last pixel (x2, y2) follows -- so every iteration stands alone (line_iter below, compiled for the host too:
// frr_host_line_pixels).  set_pixel (:497-503) addresses linearly, (y * width + x) * 4 with no test of x: a pixel is its
// linear index here, and x >= width lands in a later row as it does there.
//
// Calls are sequential in the reference: where segments cross, the later call's colour stays.  That order is resolved
// per pixel by two launches over the same iterations: k_lines_mark raises owner[p] to (segment number + 1) with
// atomicMax, k_lines_paint stores the colour where owner[p] names its own segment and puts the 0 back -- the plane is
// all-zero between commands.  A segment never paints a pixel twice (its linear indices rise strictly along the walk), so
// exactly one thread finds its number.
//
// Included by frr_api.hip only (not part of the text embedded for user shaders).
#pragma once
#include "frr_kernels.h"

namespace frr {

// a draw_line call after the per-axis sort of its endpoints (:541-542): the corner (x1, y1) and the extents
struct LineSeg { uint32_t x1, y1, dx, dy; };

FRR_HD LineSeg line_setup(uint32_t xa, uint32_t ya, uint32_t xb, uint32_t yb)
{
    LineSeg s;
    s.x1 = xa < xb ? xa : xb; s.dx = (xa < xb ? xb : xa) - s.x1;
    s.y1 = ya < yb ? ya : yb; s.dy = (ya < yb ? yb : ya) - s.y1;
    return s;
}
// iterations of the walk: a point 1 (:545), a vertical dy (:548), a horizontal dx (:553), else the major extent and the
// last pixel (:563-572, :575-584)
FRR_HD uint64_t line_iters(const LineSeg &s)
{
    if (s.dx == 0u) return s.dy == 0u ? 1ull : (uint64_t)s.dy;
    if (s.dy == 0u) return (uint64_t)s.dx;
    return (uint64_t)(s.dx > s.dy ? s.dx : s.dy) + 1ull;
}
// the largest linear pixel index the walk writes: where the reference's buffer index panics first
FRR_HD uint64_t line_max_index(const LineSeg &s, uint64_t W)
{
    const uint64_t x1 = s.x1, y1 = s.y1, x2 = x1 + s.dx, y2 = y1 + s.dy;
    if (s.dx == 0u) return s.dy == 0u ? y1 * W + x1 : (y2 - 1ull) * W + x1;
    if (s.dy == 0u) return y1 * W + x2 - 1ull;
    return y2 * W + x2;
}
// iteration i (< line_iters) of the walk: the one or two linear pixel indices it writes, in write order
FRR_HD int line_iter(const LineSeg &s, uint32_t i, uint64_t W, uint64_t p[2])
{
    if (s.dx == 0u || s.dy == 0u) {   // point, vertical, horizontal
        const uint64_t x = (uint64_t)s.x1 + (s.dy == 0u ? i : 0u), y = (uint64_t)s.y1 + (s.dy == 0u ? 0u : i);
        p[0] = y * W + x;
        return 1;
    }
    const bool xmajor = s.dx > s.dy;   // (dx == dy walks y: :561)
    const uint32_t major = xmajor ? s.dx : s.dy, minor = xmajor ? s.dy : s.dx;
    if (i >= major) { p[0] = ((uint64_t)s.y1 + s.dy) * W + (uint64_t)s.x1 + s.dx; return 1; }   // :572, :584
    // q = floor(i * minor / major) and the remainder the reference carries in `rem`: exact in 32 bits while both extents
    // are below 2^16, else in 64 (a legal segment that wraps rows can be nearly as long as the whole buffer)
    uint32_t q, r;
    if ((major | minor) < 65536u) {
        const uint32_t t = i * minor;
        q = t / major; r = t - q * major;
    } else {
        const uint64_t t = (uint64_t)i * minor, q64 = t / major;
        q = (uint32_t)q64; r = (uint32_t)(t - q64 * major);
    }
    const uint64_t a = (uint64_t)(xmajor ? s.x1 : s.y1) + i, b = (uint64_t)(xmajor ? s.y1 : s.x1) + q;
    p[0] = xmajor ? b * W + a : a * W + b;
    if ((uint64_t)r + minor < major) return 1;
    p[1] = xmajor ? (b + 1ull) * W + a : a * W + b + 1ull;   // rem >= major: the minor coordinate steps, same column / row again
    return 2;
}

// frr_lines_bind_device: *first_bad (0xFFFFFFFF on entry) becomes the smallest segment number whose walk would leave the
// buffer (the reference's panic)
__global__ __launch_bounds__(256) void k_lines_check(const uint4 *__restrict__ xyxy, uint32_t nlines, uint32_t W, uint64_t npix, uint32_t *first_bad)
{
    uint32_t bad = 0xFFFFFFFFu;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < nlines; k += (uint64_t)gridDim.x * 256u) {
        const uint4 v = xyxy[k];
        if (line_max_index(line_setup(v.x, v.y, v.z, v.w), W) >= npix) bad = min(bad, (uint32_t)k);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor(bad, o));
    if ((threadIdx.x & 63) == 0 && bad != 0xFFFFFFFFu) atomicMin(first_bad, bad);
}

struct LinesArgs {
    // a list (frr_draw_lines)
    const uint4 *xyxy;        // [nlines] {x1, y1, x2, y2}
    const uint32_t *rgba;     // [nlines]
    uint32_t nlines;
    // the wireframe of a geometry pass (frr_draw_wireframe): segment 3v + e is edge e of the triangle at virtual slot v
    const RasterRec *recs;
    const uint32_t *tinfo;
    uint32_t fan_cap, wire_rgba;
    int32_t gpar, lane;       // whose Counters::gtab holds the pass's input count and fan cursors
    uint32_t W, H;
    RowOwner own;             // tile-row ownership over the whole frame
    uint32_t chunk;           // iterations a segment contributes to one round of a wave (option lines_chunk)
    uint32_t seq, epoch;      // the command's sequence number (Counters::first_bad)
    Counters *cnt;
    uint32_t *owner;          // [W * H] the owner plane of the stream the command runs on
    uint32_t *color;          // [W * H] RGBA8
};

constexpr uint32_t LINES_CHUNK = 1u << 24;   // 64 lanes x 2^24 iterations: the wave's prefix sums stay below 2^31

// One wavefront per workgroup.  A wave takes 64 segments, one per lane, prefix-sums their iteration counts and walks the
// concatenated iteration space 64 iterations to a step: lane l of a step finds its segment among the 64 sums.  A 1-pixel
// edge and a 10,000-pixel diagonal in the same wave therefore cost what their pixels cost.  PAINT: second launch.
template <bool WIRE, bool PAINT> __device__ __forceinline__ void lines_walk(const LinesArgs &a)
{
    __shared__ uint4 s_seg[64];       // x1, y1, dx, dy
    __shared__ uint32_t s_rgba[64];
    __shared__ uint32_t s_incl[64];   // inclusive prefix sums of this round's iteration counts
    __shared__ uint32_t s_done[64];   // iterations of each segment walked in earlier rounds
    const uint32_t lane = threadIdx.x;
    // A failed earlier command cancels this one (the host replays both).  The marks of a command that was cancelled only
    // after its first launch are still taken back: the plane has to be zero for the replay.
    const bool cancelled = __builtin_amdgcn_readfirstlane((int)seq_cancelled(a.cnt, a.seq, a.epoch, false)) != 0;
    if (!PAINT && cancelled) return;
    const uint64_t npix = (uint64_t)a.W * a.H;
    uint32_t nseg = a.nlines;
    FanMap fm = {};
    if (WIRE) {
        fm = fan_map(&a.cnt->lane[a.lane].gtab[a.gpar], a.fan_cap);
        nseg = (uint32_t)__builtin_amdgcn_readfirstlane((int)(3u * fan_map_total(fm)));
    }
    for (uint64_t k0 = (uint64_t)blockIdx.x * 64u; k0 < nseg; k0 += (uint64_t)gridDim.x * 64u) {
        const uint32_t k = (uint32_t)k0 + lane;
        LineSeg s = {0u, 0u, 0u, 0u};
        uint32_t iters = 0u, rgba = a.wire_rgba;
        if (k < nseg) {
            if (WIRE) {
                const uint32_t v = k / 3u, e = k - 3u * v;
                const bool fan = v >= fm.ntris;
                if (fan || (a.tinfo[v] & ((1u << FAN_BITS) - 1u)) == 1u) {   // (an input that emits one triangle lives at its own slot)
                    const RasterRec &r = a.recs[fan ? fan_map_slot(fm, v) : v];
                    const bool sw = r.flags & 1u;
                    // emission-order corners e and e + 1 (the record holds them after the orientation swap of corners 1, 2)
                    const uint32_t ca = e, cb = e == 2u ? 0u : e + 1u;
                    const uint32_t ia = sw && ca ? 3u - ca : ca, ib = sw && cb ? 3u - cb : cb;
                    const int32_t xa = spi_of(r.s[2 * ia]), ya = spi_of(r.s[2 * ia + 1]);
                    const int32_t xb = spi_of(r.s[2 * ib]), yb = spi_of(r.s[2 * ib + 1]);
                    // the library's rule for a wireframe: an edge with an endpoint off the screen is skipped whole
                    if (xa >= 0 && xb >= 0 && ya >= 0 && yb >= 0 && (uint32_t)xa < a.W && (uint32_t)xb < a.W && (uint32_t)ya < a.H && (uint32_t)yb < a.H) {
                        s = line_setup((uint32_t)xa, (uint32_t)ya, (uint32_t)xb, (uint32_t)yb);
                        iters = (uint32_t)line_iters(s);
                    }
                }
            } else {
                const uint4 v = a.xyxy[k];
                s = line_setup(v.x, v.y, v.z, v.w);
                rgba = a.rgba[k];
                // (a list rewritten without a re-bind: a segment that would leave the buffer is dropped, not walked)
                if (line_max_index(s, a.W) < npix) iters = (uint32_t)line_iters(s);
            }
        }
        __syncthreads();   // the previous batch's last step has read the tables
        s_seg[lane] = make_uint4(s.x1, s.y1, s.dx, s.dy);
        s_rgba[lane] = rgba;
        for (uint32_t done = 0u;;) {
            const uint32_t part = min(iters - done, a.chunk);
            const uint32_t incl = wave_incl_scan(part);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (total == 0u) break;
            __syncthreads();   // (the previous round's last step)
            s_incl[lane] = incl; s_done[lane] = done;
            __syncthreads();
            for (uint32_t it0 = 0u; it0 < total; it0 += 64u) {
                const uint32_t it = it0 + lane;
                if (it >= total) continue;
                uint32_t j = 0u;   // the first segment whose inclusive sum exceeds `it`
#pragma unroll
                for (uint32_t step = 32u; step; step >>= 1) if (s_incl[j + step - 1u] <= it) j += step;
                const uint32_t i = s_done[j] + (it - (j ? s_incl[j - 1u] : 0u));
                const uint4 q = s_seg[j];
                const LineSeg sj = {q.x, q.y, q.z, q.w};
                const uint32_t id = (uint32_t)k0 + j + 1u;
                uint64_t p[2];
                const int np = line_iter(sj, i, a.W, p);
                for (int w = 0; w < np; ++w) {
                    if (p[w] >= npix) continue;   // a guard for the machine, not a defined result
                    const uint32_t pi = (uint32_t)p[w];
                    if (a.own.world > 1 && !owns_tile_row((int)(pi / a.W / (uint32_t)TILE), a.own)) continue;
                    if (!PAINT) atomicMax(&a.owner[pi], id);
                    else if (a.owner[pi] == id) {
                        if (!cancelled) a.color[pi] = s_rgba[j];
                        a.owner[pi] = 0u;
                    }
                }
            }
            done += part;
        }
    }
}

template <bool WIRE> __global__ __launch_bounds__(64) void k_lines_mark(LinesArgs a) { lines_walk<WIRE, false>(a); }
template <bool WIRE> __global__ __launch_bounds__(64) void k_lines_paint(LinesArgs a) { lines_walk<WIRE, true>(a); }

} // namespace frr
