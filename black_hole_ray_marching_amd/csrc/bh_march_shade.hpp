// bh_march_shade.hpp -- from a finished ray to its texel: the sky sample (texel_u32, decode, sample_sky), the sky
// coordinates and colour of a ray (sky_uv, shade, lens_record), the output encoders (store_px, store_px_planar,
// store_rgbm14) and the pixel store (write_pixel, out_index).
// Needs bh_march_ops.hpp and bh_srgb.hpp (the BGRA8 encoder, the row-major store, the workgroup's LDS tables).
#pragma once
#include <hip/hip_fp16.h>

#include "bh_march_ops.hpp"
#include "bh_srgb.hpp"

namespace bh {
namespace BH_NS {

// x, y clamped to the texture; 32-bit element index (bh_create: at most 2^30 texels), so the gather
// address is one 32-bit multiply-add and one 64-bit shift-add
__device__ __forceinline__ uint32_t texel_u32(const MarchArgs& a, int32_t x, int32_t y) {
    return a.sky[(uint32_t)y * a.sky_w + (uint32_t)x];
}
__device__ __forceinline__ v3 decode(const float* lut, uint32_t t) {
    return mk(lut[t & 0xffu], lut[(t >> 8) & 0xffu], lut[(t >> 16) & 0xffu]);
}
// lo <= hi: one v_med3_i32
__device__ __forceinline__ int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return min(max(v, lo), hi); }

// textureSampleLevel(t_diffuse, s_diffuse, uv, 0) on Rgba8UnormSrgb, mag=Linear, clamp-to-edge
// (src/texture.rs:41,62-70): decode texels, then bilinear with fp32 weights.
__device__ __forceinline__ v3 sample_sky(const MarchArgs& a, const float* lut, float u, float v) {
    if (u != u || v != v) return decode(lut, texel_u32(a, 0, 0));  // Q8
    float tx = u * (float)a.sky_w - 0.5f;
    float ty = v * (float)a.sky_h - 0.5f;
    // fminf(fmaxf(t, -1), n) for the non-NaN t here: one v_med3_f32
    tx = __builtin_amdgcn_fmed3f(tx, -1.0f, (float)a.sky_w);
    ty = __builtin_amdgcn_fmed3f(ty, -1.0f, (float)a.sky_h);
    float fx0 = floorf(tx), fy0 = floorf(ty);
    float fa = tx - fx0, fb = ty - fy0;
    int32_t x0 = (int32_t)fx0, y0 = (int32_t)fy0;
    const int32_t wm = (int32_t)a.sky_w - 1, hm = (int32_t)a.sky_h - 1;
    int32_t x1 = clampi(x0 + 1, 0, wm), y1 = clampi(y0 + 1, 0, hm);
    x0 = clampi(x0, 0, wm);
    y0 = clampi(y0, 0, hm);
    // the four gathers first, then the decodes: one wait for all four (in the source-order build each
    // decode would otherwise wait for its own load)
    const uint32_t w00 = texel_u32(a, x0, y0), w10 = texel_u32(a, x1, y0);
    const uint32_t w01 = texel_u32(a, x0, y1), w11 = texel_u32(a, x1, y1);
    v3 t00 = decode(lut, w00), t10 = decode(lut, w10);
    v3 t01 = decode(lut, w01), t11 = decode(lut, w11);
    float ia = 1.0f - fa, ib = 1.0f - fb;
    v3 top = add(muls(t00, ia), muls(t10, fa));
    v3 bot = add(muls(t01, ia), muls(t11, fa));
    return add(muls(top, ib), muls(bot, fb));
}

// The shading of a sky ray has two halves: where its final direction points in the sky (:329-336, sky_uv),
// and the sample there (:341-343).  shade() runs both; the lens epilogue (march_tile_lens_kernel) stores the
// first half's result, and bh_shade_lens runs the second on it later, with any sky (bh_lens.hpp: the same
// ops, written for host and device).
// (u, v): the two arguments of the sample at :341
__device__ __forceinline__ void sky_uv(v3 rd, float& u, float& v) {
#if BH_FAST
    const v3 n = normalize(rd);                             // :330
    const float az = atan2f(n.z, n.x);                      // :332
    const float x = (az + ONE_PI) / TWO_PI;                 // :334
#else
    const v3 n = normalize_x(rd);
    // RN_f32 of the f64 atan2 (:332): the short f64 core, and the library call for the lanes whose angle
    // lies too close to an f32 rounding midpoint for the core to decide (about 2^-21 of them)
    const crm::Atan2 at = crm::atan2_core(n.z, n.x);
    float az = at.f;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(at.near) != 0ull, 0)) {
        if (at.near) az = (float)atan2((double)n.z, (double)n.x);
    }
    // az + pi is +0 or in [2^-22, 7] (az is an f32 in [-RN(pi), RN(pi)]): inside the division core's
    // domain
    const float x = crm::div_core(az + ONE_PI, crm::Rcp{TWO_PI, 1.0f / TWO_PI});  // RN(1/2pi) folded
#endif
    const float y = (n.y + 1.0f) * 0.5f;                    // :336
    u = x;
    v = 1.0f - y;
}
// Colour of a finished ray (:329-345 for sky rays; :275/:281 blackout -> 0; :287 surface -> 1).
// (The sampling half stays in this function: as a function of its own -- shade_uv(a, lut, u, v) -- every
// march kernel's register allocation came out different; this form leaves their machine code as it was.)
__device__ __forceinline__ v3 shade(const MarchArgs& a, const float* lut, uint32_t fate, v3 rd) {
    if (fate == BH_FATE_BLACKOUT) return mk(0.0f, 0.0f, 0.0f);
    if (fate == BH_FATE_SURFACE) return mk(1.0f, 1.0f, 1.0f);
    float u, v;
    sky_uv(rd, u, v);
    v3 col = sample_sky(a, lut, u, v);                      // :341
#if BH_FAST
    col.y = col.y * __builtin_sqrtf(col.y);                 // :342
    col.z = col.z * __builtin_sqrtf(col.z);                 // :343
#else
    col.y = pow15_x(col.y);
    col.z = pow15_x(col.z);
#endif
    return col;
}
#if !BH_FAST
// The lens record of a finished ray (include/bh_render.h, bh_lens_px): a sentinel u for the two fates that
// have a colour of their own, else the sky coordinates -- what shade() hands to its sample.  Exact math only.
__device__ __forceinline__ float2 lens_record(uint32_t fate, v3 rd) {
    if (fate == BH_FATE_BLACKOUT) return make_float2(BH_LENS_BLACKOUT, 0.0f);
    if (fate == BH_FATE_SURFACE) return make_float2(BH_LENS_SURFACE, 0.0f);
    float u, v;
    sky_uv(rd, u, v);
    return make_float2(u, v);
}
#endif

// Output texel store of a row-major target (bh_srgb.hpp, store_rgb)
template <uint32_t FMT>
__device__ __forceinline__ void store_px(void* base, size_t idx, v3 c, const float* enc) { store_rgb<FMT>(base, idx, c.x, c.y, c.z, enc); }

// BH_LAYOUT_TILES_RGB(M) store: pixel idx = tile * 64 + lane goes to three channel planes of its tile
// (alpha, always 1, is dropped; the unpack restores it).  Each plane store of a wave is one
// contiguous 64-element run.  TE = the tile's size in channel elements (192, or 192 + the 8-byte
// blackout mask word of BH_LAYOUT_TILES_RGBM).
template <uint32_t FMT, uint32_t TE>
__device__ __forceinline__ void store_px_planar(void* base, size_t idx, v3 c, const float* enc) {
    const size_t o = (idx >> 6) * TE + (idx & 63u);
    if constexpr (FMT == BH_OUT_RGBA32F) {
        float* p = reinterpret_cast<float*>(base) + o;
        p[0] = c.x; p[64] = c.y; p[128] = c.z;
    } else if constexpr (FMT == BH_OUT_RGBA16F) {
        __half* p = reinterpret_cast<__half*>(base) + o;
        p[0] = __float2half_rn(c.x); p[64] = __float2half_rn(c.y); p[128] = __float2half_rn(c.z);
    } else {
        const uint32_t w = srgb_bgra8(c.x, c.y, c.z, enc);
        uint8_t* p = reinterpret_cast<uint8_t*>(base) + o;
        p[0] = (uint8_t)w; p[64] = (uint8_t)(w >> 8); p[128] = (uint8_t)(w >> 16);
    }
}

// Channel elements of one BH_LAYOUT_TILES_RGBM tile: three planes of 64, then the 8-byte mask word.
template <uint32_t FMT>
constexpr uint32_t rgbm_tile_elems() { return 192u + 8u / (FMT == BH_OUT_RGBA32F ? 4u : FMT == BH_OUT_RGBA16F ? 2u : 1u); }

// BH_LAYOUT_TILES_RGBM14 store (include/bh_render.h): the RGBA16F channels, each an fp16 in [0, 1] (bits
// 14-15 zero), as 64 words r | g << 14 | (b & 0xF) << 28, 64 bytes (b >> 4) & 0xFF, the wave's ballots of
// b's bits 12 and 13, and the blackout mask word -- 86 words per tile.  Every active lane of the wave
// must hold a pixel of the same tile (as for RGBM); its first active lane stores the three 64-bit words.
__device__ __forceinline__ void store_rgbm14(void* base, size_t idx, v3 c, bool zero) {
    const uint32_t r = __half_as_ushort(__float2half_rn(c.x)), g = __half_as_ushort(__float2half_rn(c.y));
    const uint32_t b = __half_as_ushort(__float2half_rn(c.z));
    uint32_t* W = reinterpret_cast<uint32_t*>(base) + (idx >> 6) * 86u;
    const uint32_t e = (uint32_t)idx & 63u;
    W[e] = r | (g << 14) | (b << 28);
    reinterpret_cast<uint8_t*>(W + 64)[e] = (uint8_t)(b >> 4);
    const uint64_t m12 = __builtin_amdgcn_ballot_w64(((b >> 12) & 1u) != 0u);
    const uint64_t m13 = __builtin_amdgcn_ballot_w64(((b >> 13) & 1u) != 0u);
    const uint64_t mz = __builtin_amdgcn_ballot_w64(zero);
    if (e == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec())) {
        uint64_t* M = reinterpret_cast<uint64_t*>(W + 80);
        M[0] = m12;
        M[1] = m13;
        M[2] = mz;
    }
}

// fs_main output (:365-369): col, blackout_col = dot(col,col) < 1 ? 0 : col, debug counters.
// BH_LAYOUT_TILES_RGBM: every active lane of the calling wave must hold a pixel of the same tile
// (true of the tile and pair schedules, bh_render rejects the others): the wave's ballot of the
// blackout test is the tile's mask word, stored by its first active lane.
template <uint32_t FMT>
__device__ __forceinline__ void write_pixel(const MarchArgs& a, const float* tab, size_t idx, v3 col, uint32_t n_rk,
                                            uint32_t fate, uint32_t steps) {
    const bool zero = dot(col, col) < 1.0f;
    const v3 bo = zero ? mk(0.0f, 0.0f, 0.0f) : col;
    if (a.layout == BH_LAYOUT_TILES_RGB) {
        store_px_planar<FMT, 192u>(a.out_col, idx, col, tab + 256);
        if (a.out_blackout) store_px_planar<FMT, 192u>(a.out_blackout, idx, bo, tab + 256);
    } else if (a.layout == BH_LAYOUT_TILES_RGBM) {
        constexpr uint32_t TE = rgbm_tile_elems<FMT>();
        constexpr uint32_t CB = FMT == BH_OUT_RGBA32F ? 4u : FMT == BH_OUT_RGBA16F ? 2u : 1u;
        store_px_planar<FMT, TE>(a.out_col, idx, col, tab + 256);
        if (a.out_blackout) store_px_planar<FMT, TE>(a.out_blackout, idx, bo, tab + 256);
        const uint64_t m = __builtin_amdgcn_ballot_w64(zero);
        if ((uint32_t)(idx & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec())) {
            const size_t w = ((idx >> 6) * TE + 192u) * CB / 8u;  // the mask word (8-byte aligned)
            reinterpret_cast<uint64_t*>(a.out_col)[w] = m;
            if (a.out_blackout) reinterpret_cast<uint64_t*>(a.out_blackout)[w] = m;
        }
    } else if (a.layout == BH_LAYOUT_TILES_RGBM14) {
        if constexpr (FMT == BH_OUT_RGBA16F) {  // bh_render admits this layout for RGBA16F only
            store_rgbm14(a.out_col, idx, col, zero);
            if (a.out_blackout) store_rgbm14(a.out_blackout, idx, bo, zero);
        }
    } else {
        store_px<FMT>(a.out_col, idx, col, tab + 256);
        if (a.out_blackout) store_px<FMT>(a.out_blackout, idx, bo, tab + 256);
    }
    if (a.dbg_n_rk) a.dbg_n_rk[idx] = (uint16_t)n_rk;
    if (a.dbg_fate) a.dbg_fate[idx] = (uint8_t)fate;
    if (a.dbg_steps) a.dbg_steps[idx] = (uint16_t)steps;
}
template <uint32_t FMT>
__device__ __forceinline__ void write_pixel(const MarchArgs& a, const float* tab, size_t idx, v3 col, uint32_t n_rk,
                                            uint32_t fate) {
    write_pixel<FMT>(a, tab, idx, col, n_rk, fate, n_rk);
}

// 32-bit pixel index: width, height <= 65536 (bh_render), so py * W + px < 2^32; a shard holds < 2^24 tiles
__device__ __forceinline__ uint32_t out_index(const MarchArgs& a, uint32_t t, uint32_t lane, uint32_t px, uint32_t py) {
    return (a.layout != BH_LAYOUT_ROWMAJOR) ? t * 64u + lane : py * a.width + px;
}

}  // namespace BH_NS
}  // namespace bh
