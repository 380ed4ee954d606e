// bh_lens.hpp — shading a lens map (include/bh_render.h, bh_lens_px): host and device share every function
// here.  The shade kernel (bh_lens.hip) runs them per output pixel, bh_lens_shade_host (bh_mirror.cpp) runs the
// very same functions in a loop on the CPU.  Both translation units are built without contraction, the device
// one with correctly rounded fp32 sqrt, so every op here rounds once, as the same op of the march kernel's
// shading does (bh_march_shade.hpp: sample_sky, write_pixel's blackout test; bh_march_ops.hpp: pow15_x; bh_march_resolve.hpp: ss_resolve's tree).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bh_render.h"

#ifndef BH_LENS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BH_LENS_HD __host__ __device__ inline
#else
#define BH_LENS_HD inline
#endif
#endif

namespace bh {
namespace lens {

struct Rgb { float r, g, b; };
struct SkyView { const uint32_t* texels; uint32_t w, h; };  // r | g << 8 | b << 16 | a << 24 per texel

BH_LENS_HD int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
BH_LENS_HD Rgb decode(const float* lut, uint32_t t) { return {lut[t & 0xffu], lut[(t >> 8) & 0xffu], lut[(t >> 16) & 0xffu]}; }
// a sky holds at most 2^30 texels (bh_create, bh_sky_create): a 32-bit element index
BH_LENS_HD uint32_t texel(const SkyView& s, int32_t x, int32_t y) { return s.texels[(uint32_t)y * s.w + (uint32_t)x]; }

// textureSampleLevel on Rgba8UnormSrgb, mag Linear, clamp to edge: sample_sky's arithmetic (bh_march_shade.hpp),
// op for op.  A NaN coordinate takes texel (0, 0).
BH_LENS_HD Rgb sample(const SkyView& s, const float* lut, float u, float v) {
    if (u != u || v != v) return decode(lut, texel(s, 0, 0));
    float tx = u * (float)s.w - 0.5f;
    float ty = v * (float)s.h - 0.5f;
    tx = fminf(fmaxf(tx, -1.0f), (float)s.w);
    ty = fminf(fmaxf(ty, -1.0f), (float)s.h);
    const float fx0 = floorf(tx), fy0 = floorf(ty);
    const float fa = tx - fx0, fb = ty - fy0;
    int32_t x0 = (int32_t)fx0, y0 = (int32_t)fy0;
    const int32_t wm = (int32_t)s.w - 1, hm = (int32_t)s.h - 1;
    const int32_t x1 = clampi(x0 + 1, 0, wm), y1 = clampi(y0 + 1, 0, hm);
    x0 = clampi(x0, 0, wm);
    y0 = clampi(y0, 0, hm);
    const uint32_t w00 = texel(s, x0, y0), w10 = texel(s, x1, y0);  // the four gathers first: one wait
    const uint32_t w01 = texel(s, x0, y1), w11 = texel(s, x1, y1);
    const Rgb t00 = decode(lut, w00), t10 = decode(lut, w10), t01 = decode(lut, w01), t11 = decode(lut, w11);
    const float ia = 1.0f - fa, ib = 1.0f - fb;
    const Rgb top = {t00.r * ia + t10.r * fa, t00.g * ia + t10.g * fa, t00.b * ia + t10.b * fa};
    const Rgb bot = {t01.r * ia + t11.r * fa, t01.g * ia + t11.g * fa, t01.b * ia + t11.b * fa};
    return {top.r * ib + bot.r * fb, top.g * ib + bot.g * fb, top.b * ib + bot.b * fb};
}

// col of one record
BH_LENS_HD Rgb shade(float u, float v, const SkyView& s, const float* lut) {
    if (u == BH_LENS_BLACKOUT) return {0.0f, 0.0f, 0.0f};
    if (u == BH_LENS_SURFACE) return {1.0f, 1.0f, 1.0f};
    Rgb c = sample(s, lut, u, v);
    c.g = c.g * sqrtf(c.g);  // c >= 0: a bilinear mix of decoded texels
    c.b = c.b * sqrtf(c.b);
    return c;
}
// blackout_col of a col (src/black_hole_maybe.wgsl:365-368)
BH_LENS_HD Rgb blackout(Rgb c) {
    const bool zero = (c.r * c.r + c.g * c.g) + c.b * c.b < 1.0f;
    return zero ? Rgb{0.0f, 0.0f, 0.0f} : c;
}

// 8-byte load of a record (the ABI asks for 8-byte aligned lenses)
BH_LENS_HD bh_lens_px load_px(const bh_lens_px* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float2 t = *reinterpret_cast<const float2*>(p);
    return {t.x, t.y};
#else
    return *p;
#endif
}

// The two targets' samples, or sums of samples, of one output pixel.  BO = false: col only (bo stays 0).
struct Acc { Rgb col, bo; };
template <bool BO>
BH_LENS_HD Acc add(const Acc& p, const Acc& q) {
    Acc r{{p.col.r + q.col.r, p.col.g + q.col.g, p.col.b + q.col.b}, {0.0f, 0.0f, 0.0f}};
    if constexpr (BO) r.bo = {p.bo.r + q.bo.r, p.bo.g + q.bo.g, p.bo.b + q.bo.b};
    return r;
}

// The normative resolve (include/bh_render.h, bh_render_ss) as two recursions: the pairwise tree over N = 2^n
// neighbouring records of one lens row -- level 1 adds neighbours, level 2 the pair sums, ... -- and the same
// tree over N rows' results; the sums the xor butterfly of bh_ss.hpp leaves in every lane of a group (fp32 add
// is commutative bit for bit).  Each record is shaded on its own, the blackout test per sample.
template <int N, int K, bool BO>
BH_LENS_HD Acc sum_x(const bh_lens_px* p, const SkyView& s, const float* lut) {
    if constexpr (N == 1) {
        const bh_lens_px r = load_px(p);
        Acc a{shade(r.u, r.v, s, lut), {0.0f, 0.0f, 0.0f}};
        if constexpr (BO) a.bo = blackout(a.col);
        return a;
    } else {
        const Acc lo = sum_x<N / 2, K, BO>(p, s, lut), hi = sum_x<N / 2, K, BO>(p + N / 2, s, lut);
        const Acc r = add<BO>(lo, hi);
#if defined(__HIP_DEVICE_COMPILE__)
        // K = 8: four samples in flight at a time.  Left free, the scheduler starts the loads of a whole row
        // of samples, or more, first and the kernel spills (248 VGPRs and scratch).
        if constexpr (K == 8 && N == 4) __builtin_amdgcn_sched_barrier(0);
#endif
        return r;
    }
}
template <int N, int K, bool BO>
BH_LENS_HD Acc sum_y(const bh_lens_px* row, size_t vw, const SkyView& s, const float* lut) {
    if constexpr (N == 1) {
        return sum_x<K, K, BO>(row, s, lut);
    } else {
        const Acc lo = sum_y<N / 2, K, BO>(row, vw, s, lut), hi = sum_y<N / 2, K, BO>(row + (N / 2) * vw, vw, s, lut);
        return add<BO>(lo, hi);
    }
}

// Output pixel (x, y) of a width-pixel-wide frame from the lens of its virtual frame (K * width records per
// row): its K x K records resolved as above, then one multiply by 1 / K^2 (a power of two: exact).
template <int K, bool BO>
BH_LENS_HD Acc shade_pixel(const bh_lens_px* lens, uint32_t width, uint32_t x, uint32_t y, const SkyView& s,
                           const float* lut) {
    const size_t vw = (size_t)width * K;
    Acc a = sum_y<K, K, BO>(lens + (size_t)y * K * vw + (size_t)x * K, vw, s, lut);
    if constexpr (K > 1) {
        constexpr float scale = 1.0f / (float)(K * K);
        a.col = {a.col.r * scale, a.col.g * scale, a.col.b * scale};
        if constexpr (BO) a.bo = {a.bo.r * scale, a.bo.g * scale, a.bo.b * scale};
    }
    return a;
}

}  // namespace lens
}  // namespace bh
