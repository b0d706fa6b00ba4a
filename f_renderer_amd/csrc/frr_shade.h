// frr_shade.h -- the step from a pixel's ShaderContext to its RGBA8 word (renderer.rs:380-381, 7-14, 497-503) as a command
// of its own: frr_shade_varyings runs a pixel shader, built-in or user, over a buffer of varyings (what frr_resolve_varyings
// writes, or anything the caller made) and stores the colour target.  run_ps and quantize_u8 are the very functions
// shade_pixel (frr_raster.h) calls, so a depth pre-pass + resolve + shade leaves the forward frame bit for bit.
//   k_shade_vary   one thread per window pixel: id -> range test -> K loads -> run_ps -> quantize -> one 32-bit store
//   k_shade_items  the same with per-ITEM pixel uniforms (frr_shade_items): id -> item of the latest pass (the span search
//                  of frr_visible.h) -> that item's frr_material over the call's uniforms -> the very same run_ps / quantize
// No atomics; LDS only for the u8 -> float table of the texture-sampling shaders.  Part of the text embedded for user
// shaders (frr_shader_register compiles the user's frr_user_ps into k_shade_vary<FRR_USER_K, FRR_SHADER_USER_BASE, *> and
// k_shade_items<the same>).
#pragma once
#include "frr_device.h"
#include "frr_visible.h"

namespace frr {

struct ShadeArgs {
    int32_t x0, x1, y0, y1;           // the window (depth index (cy - y0) * x1 + (cx - x0), renderer.rs:362; x0 >= 0)
    int32_t cstride;                  // colour row stride (fb.width)
    RowOwner own;                     // tile-row ownership over the window's tile rows
    uint32_t id_first, id_count;      // shaded: id != ~0 and id - id_first < id_count (frame-global emission indices)
    uint32_t seq, epoch;              // the command's sequence number (Counters::first_bad)
    const Counters *cnt;
    const uint32_t *tri_id;           // the frame's triangle-id target
    const float *in;                  // [in_entries][K], pixel-major (null with K == 0)
    uint64_t in_entries;
    uint32_t *color;                  // the frame's colour target as RGBA8 words
};

constexpr int SHADE_WG = 256;

// One thread per window pixel, a workgroup per run of SHADE_WG pixels of one row: the id loads and the 4-byte colour stores
// of a wavefront are contiguous.  K: floats per entry (what PS reads of them is its business: FRR_PS_FLAT is built with 0).
// VEC: K is a multiple of 4 and the buffer is 16-byte aligned, so every entry is: 16-byte loads; else scalar ones.  The
// host decides: it is the same for all pixels.  The buffer is indexed only by lanes that pass the range test.
template <int K, int PS, bool VEC> __global__ __launch_bounds__(SHADE_WG) void k_shade_vary(ShadeArgs a, DevUniforms u)
{
    constexpr bool TEXTURED = PS == FRR_PS_PHONG || PS == FRR_PS_BLINN || PS >= FRR_SHADER_USER_BASE;   // (the u8 -> float table of sample_2d)
    static_assert(!VEC || (K > 0 && K % 4 == 0), "16-byte loads need whole float4s");
    const int lx = (int)(blockIdx.x * SHADE_WG + threadIdx.x), ry = (int)blockIdx.y;
    // (both tests are the same for the whole workgroup: nobody is left alone at the barriers below)
    if (a.own.world > 1 && !owns_tile_row(ry / TILE, a.own)) return;
    // behind a failed command the ids are stale (the cancelled draw never wrote its own): nothing is written, and the
    // replay runs this command again in its place
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;
    const size_t i = (size_t)ry * (size_t)a.x1 + (size_t)lx;                    // :362
    bool shade = false;
    if (lx < a.x1 - a.x0) {
        const uint32_t id = a.tri_id[i];
        shade = id != 0xFFFFFFFFu && id - a.id_first < a.id_count && (K == 0 || i < a.in_entries);   // (the last: a guard for the machine)
    }
    const float *lut = nullptr;
    if constexpr (TEXTURED) {
        __shared__ float s_u8[256];
        __shared__ uint32_t s_any[SHADE_WG / 64];
        const bool wave_any = __ballot(shade) != 0ull;
        if ((threadIdx.x & 63u) == 0u) s_any[threadIdx.x >> 6] = wave_any ? 1u : 0u;
        __syncthreads();
        uint32_t any = 0u;
#pragma unroll
        for (int w = 0; w < SHADE_WG / 64; ++w) any |= s_any[w];
        if (any == 0u) return;                             // nothing of this run is in range: no table
        for (int k = threadIdx.x; k < 256; k += SHADE_WG) s_u8[k] = (float)k / 255.0f;
        __syncthreads();
        lut = s_u8;
    }
    if (!shade) return;
    float in[K > 0 ? K : 1];
    if constexpr (K > 0) {
        const float *e = a.in + i * (size_t)K;
        if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < K / 4; ++q) {
                const float4 x = *reinterpret_cast<const float4 *>(e + 4 * q);
                in[4 * q] = x.x; in[4 * q + 1] = x.y; in[4 * q + 2] = x.z; in[4 * q + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) in[k] = e[k];
        }
    } else {
        in[0] = 0.0f;
    }
    float col[4];
    run_ps<PS>(u, in, col, lut);                                                // :380
    a.color[(size_t)ry * (size_t)a.cstride + (size_t)lx] =
        quantize_u8(col[0]) | (quantize_u8(col[1]) << 8) | (quantize_u8(col[2]) << 16) | (quantize_u8(col[3]) << 24);   // :381, :7-14
}

// ---- frr_shade_items: the same pass with the pixel uniforms of each pixel's ITEM (phong.rs:34-47, 361-370 for a list) ------
struct ShadeItemsArgs {
    ShadeArgs s;                      // (id_first / id_count unused: the ids shaded are the pass's, [bounds[0], bounds[nitems]))
    const uint32_t *bounds;           // [nitems + 1] the ids of item k are [bounds[k], bounds[k + 1]) (k_visible_prep)
    uint32_t nitems;                  // >= 1
    const frr_material *mats;         // [>= nitems], 16-byte aligned
    const uint8_t *zero_tex;          // one RGBA8 texel of zeros: the texture of a material whose slot is empty
};

// u with the fields a material replaces taken from *m.  m is wave-uniform, so every value stays in SGPRs and the texture
// pointer stays scalar, as under k_shade_vary; the slot is clamped (a guard for the machine: the tables are checked).
// An EMPTY slot (no texture uploaded: only a user pixel shader gets here, the host refuses it for the lit built-ins) becomes
// the 1 x 1 texture *zero_tex, so that frr::sample_2d(u, ...) -- which, unlike sample_2d_slot, tests nothing -- reads a texel
// that exists and returns zeros, not address 0.
// (The loads are at a wave-uniform address; the compiler may still issue them per lane, since it cannot see that the
// kernel's colour stores leave the table alone -- wave_uniform tells it that every lane holds the same word.)
__device__ __forceinline__ float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ void material_apply(DevUniforms &u, const frr_material *m, const uint8_t *zero_tex)
{
    const float4 *q = reinterpret_cast<const float4 *>(m);
    float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    q0.x = wave_uniform(q0.x); q0.y = wave_uniform(q0.y); q0.z = wave_uniform(q0.z);
    q1.x = wave_uniform(q1.x); q1.y = wave_uniform(q1.y); q1.z = wave_uniform(q1.z); q1.w = wave_uniform(q1.w);
    q2.x = wave_uniform(q2.x); q2.y = wave_uniform(q2.y); q2.z = wave_uniform(q2.z); q2.w = wave_uniform(q2.w);
    q3.x = wave_uniform(q3.x); q3.y = wave_uniform(q3.y); q3.z = wave_uniform(q3.z); q3.w = wave_uniform(q3.w);
    const int slot = __float_as_int(q0.x);
    // (selects over constant indices, not u.slot_tex[slot]: a run-time index would put the whole of u into scratch)
    u.tex = u.slot_tex[0]; u.tex_w = u.slot_w[0]; u.tex_h = u.slot_h[0];
#pragma unroll
    for (int s = 1; s < FRR_MAX_TEXTURES; ++s)
        if (slot == s || (s == FRR_MAX_TEXTURES - 1 && slot > s)) { u.tex = u.slot_tex[s]; u.tex_w = u.slot_w[s]; u.tex_h = u.slot_h[s]; }
    if (!u.tex || u.tex_w == 0u || u.tex_h == 0u) { u.tex = zero_tex; u.tex_w = 1u; u.tex_h = 1u; }
    u.ambient_strength = q0.y; u.specular_strength = q0.z;
    u.flat_color[0] = q1.x; u.flat_color[1] = q1.y; u.flat_color[2] = q1.z; u.flat_color[3] = q1.w;
    u.user[0] = q2.x; u.user[1] = q2.y; u.user[2] = q2.z; u.user[3] = q2.w;
    u.user[4] = q3.x; u.user[5] = q3.y; u.user[6] = q3.z; u.user[7] = q3.w;
    static_assert(FRR_MATERIAL_USER == 8 && sizeof(frr_material) == 64, "four 16-byte loads");
}

// k_shade_vary's shape, exits, LDS table and loads; new is the item of each shaded lane and the loop over the DISTINCT
// items of the wavefront.  A wavefront is 64 consecutive entries of a row -- a span of frr_visible.h -- so the search is
// k_visible's: the span's smallest and largest in-pass id narrow the items to [lo, hi] (vis_span_range), and only where
// lo != hi does a lane search at all.  Then, while lanes wait: the first waiting lane's item (readlane), that item's
// material over the call's uniforms, the shader for the lanes that hold that item, which wait no longer.  One round for
// most spans; run_ps never sees a lane-varying uniform.  Lanes outside the pass leave before the loop.
template <int K, int PS, bool VEC> __global__ __launch_bounds__(SHADE_WG) void k_shade_items(ShadeItemsArgs b, DevUniforms u)
{
    constexpr bool TEXTURED = PS == FRR_PS_PHONG || PS == FRR_PS_BLINN || PS >= FRR_SHADER_USER_BASE;
    static_assert(!VEC || (K > 0 && K % 4 == 0), "16-byte loads need whole float4s");
    const ShadeArgs &a = b.s;
    const int lx = (int)(blockIdx.x * SHADE_WG + threadIdx.x), ry = (int)blockIdx.y;
    if (a.own.world > 1 && !owns_tile_row(ry / TILE, a.own)) return;
    if (seq_cancelled(a.cnt, a.seq, a.epoch, false)) return;   // (the boundaries were not built either: k_visible_prep)
    const uint32_t b0 = b.bounds[0], bn = b.bounds[b.nitems];
    const size_t i = (size_t)ry * (size_t)a.x1 + (size_t)lx;                    // :362
    uint32_t id = VIS_NONE;
    bool shade = false;
    if (lx < a.x1 - a.x0) {
        id = a.tri_id[i];
        shade = vis_in_pass(id, b0, bn) && (K == 0 || i < a.in_entries);        // (the last: a guard for the machine)
    }
    const float *lut = nullptr;
    if constexpr (TEXTURED) {
        __shared__ float s_u8[256];
        __shared__ uint32_t s_any[SHADE_WG / 64];
        const bool wave_any = __ballot(shade) != 0ull;
        if ((threadIdx.x & 63u) == 0u) s_any[threadIdx.x >> 6] = wave_any ? 1u : 0u;
        __syncthreads();
        uint32_t any = 0u;
#pragma unroll
        for (int w = 0; w < SHADE_WG / 64; ++w) any |= s_any[w];
        if (any == 0u) return;                             // nothing of this run is of the pass: no table
        for (int k = threadIdx.x; k < 256; k += SHADE_WG) s_u8[k] = (float)k / 255.0f;
        __syncthreads();
        lut = s_u8;
    }
    // (whole wavefront: the reductions below are over all 64 lanes)
    const uint32_t mn = vis_wave_min(shade ? id : VIS_NONE), mx = vis_wave_max(shade ? id : 0u);
    if (mn == VIS_NONE) return;                                // no lane of the span shades (wave-uniform)
    const VisRange r = vis_span_range(b.bounds, b.nitems, mn, mx);
    if (!shade) return;
    // (< nitems: id lies in [bounds[lo], bounds[hi + 1]); the min is a guard for the machine, so that every lane meets its round)
    const uint32_t item = min(vis_item_unit(b.bounds, r, id, true, b.nitems), b.nitems - 1u);
    float in[K > 0 ? K : 1];
    if constexpr (K > 0) {
        const float *e = a.in + i * (size_t)K;
        if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < K / 4; ++q) {
                const float4 x = *reinterpret_cast<const float4 *>(e + 4 * q);
                in[4 * q] = x.x; in[4 * q + 1] = x.y; in[4 * q + 2] = x.z; in[4 * q + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) in[k] = e[k];
        }
    } else {
        in[0] = 0.0f;
    }
    // The rounds.  The loop ends for all lanes at once, when none waits any more: a lane that left a loop early would take
    // the wave-uniform material of a LATER round with it (a value in SGPRs is one per wave, not one per lane and round).
    bool waiting = true;
    for (unsigned long long left = __ballot(waiting); left != 0ull; left = __ballot(waiting)) {
        const int head = __builtin_ctzll(left);                                 // the first lane that still waits
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)item, head);
        if (waiting && item == k) {
            material_apply(u, b.mats + k, b.zero_tex);
            float col[4];
            run_ps<PS>(u, in, col, lut);                                        // :380
            a.color[(size_t)ry * (size_t)a.cstride + (size_t)lx] =
                quantize_u8(col[0]) | (quantize_u8(col[1]) << 8) | (quantize_u8(col[2]) << 16) | (quantize_u8(col[3]) << 24);   // :381, :7-14
            waiting = false;
        }
    }
}

#ifndef __HIPCC_RTC__
// frr_materials_bind_device: a table in the caller's device memory.  cell[0] (0xFFFFFFFF on entry) becomes the smallest entry
// that material_ok refuses, cell[1] (0 on entry) the set of texture slots the good entries name.  (Not part of a user
// shader's program.)
__global__ __launch_bounds__(256) void k_materials_check(const frr_material *mats, uint32_t n, uint32_t *cell)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint4 q = *reinterpret_cast<const uint4 *>(mats + i);
        frr_material m = {};
        m.texture_slot = (int32_t)q.x; m.reserved = (int32_t)q.w;
        if (!material_ok(m)) atomicMin(&cell[0], i);
        else atomicOr(&cell[1], 1u << m.texture_slot);
    }
}
#endif

} // namespace frr
