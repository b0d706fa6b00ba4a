// frr_shade.h -- the step from a pixel's ShaderContext to its RGBA8 word (renderer.rs:380-381, 7-14, 497-503) as a command
// of its own: frr_shade_varyings runs a pixel shader, built-in or user, over a buffer of varyings (what frr_resolve_varyings
// writes, or anything the caller made) and stores the colour target.  run_ps and quantize_u8 are the very functions
// shade_pixel (frr_raster.h) calls, so a depth pre-pass + resolve + shade leaves the forward frame bit for bit.
//   k_shade_vary   one thread per window pixel: id -> range test -> K loads -> run_ps -> quantize -> one 32-bit store
// No atomics; LDS only for the u8 -> float table of the texture-sampling shaders.  Part of the text embedded for user
// shaders (frr_shader_register compiles the user's frr_user_ps into k_shade_vary<FRR_USER_K, FRR_SHADER_USER_BASE, *>).
#pragma once
#include "frr_device.h"

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

} // namespace frr
