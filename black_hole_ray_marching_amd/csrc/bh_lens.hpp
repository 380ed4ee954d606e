// bh_lens.hpp — shading a lens map (include/bh_render.h, bh_lens_px): host and device share every function
// here.  The shade kernel (bh_lens.hip) runs them per output pixel, bh_lens_shade_host (bh_mirror.cpp) runs the
// very same functions in a loop on the CPU.  Both translation units are built without contraction, the device
// one with correctly rounded fp32 sqrt, so every op here rounds once, as the same op of the march kernel's
// shading does (bh_march_shade.hpp: sample_sky, write_pixel's blackout test; bh_march_ops.hpp: pow15_x; bh_march_resolve.hpp: ss_resolve's tree).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bh_render.h"
#if defined(__HIPCC__)
#include "bh_crmath.hpp"  // the disc shade's angle on the device (crm::atan2_core)
#endif

// BH_LENS_FI: the cursor form of the resolve tree, its cursors and the pixel entry points, inlined whatever their
// size -- left to the inliner, the filtered shade's K = 4 tree becomes a called function of 87 KB.
#ifndef BH_LENS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BH_LENS_HD __host__ __device__ inline
#define BH_LENS_FI __host__ __device__ __attribute__((always_inline)) inline
#else
#define BH_LENS_HD inline
#define BH_LENS_FI inline
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

// textureSampleLevel on Rgba8UnormSrgb, mag Linear, clamp to edge, of a w x h level: sample_sky's arithmetic
// (bh_march_shade.hpp), op for op.  load(x, y) fetches a texel, widen(t) makes it an Rgb.
template <class Load, class Widen>
BH_LENS_HD Rgb bilinear(uint32_t w, uint32_t h, float u, float v, Load load, Widen widen) {
    float tx = u * (float)w - 0.5f;
    float ty = v * (float)h - 0.5f;
    tx = fminf(fmaxf(tx, -1.0f), (float)w);
    ty = fminf(fmaxf(ty, -1.0f), (float)h);
    const float fx0 = floorf(tx), fy0 = floorf(ty);
    const float fa = tx - fx0, fb = ty - fy0;
    int32_t x0 = (int32_t)fx0, y0 = (int32_t)fy0;
    const int32_t wm = (int32_t)w - 1, hm = (int32_t)h - 1;
    const int32_t x1 = clampi(x0 + 1, 0, wm), y1 = clampi(y0 + 1, 0, hm);
    x0 = clampi(x0, 0, wm);
    y0 = clampi(y0, 0, hm);
    const auto w00 = load(x0, y0), w10 = load(x1, y0);  // the four gathers first: one wait
    const auto w01 = load(x0, y1), w11 = load(x1, y1);
    const Rgb t00 = widen(w00), t10 = widen(w10), t01 = widen(w01), t11 = widen(w11);
    const float ia = 1.0f - fa, ib = 1.0f - fb;
    const Rgb top = {t00.r * ia + t10.r * fa, t00.g * ia + t10.g * fa, t00.b * ia + t10.b * fa};
    const Rgb bot = {t01.r * ia + t11.r * fa, t01.g * ia + t11.g * fa, t01.b * ia + t11.b * fa};
    return {top.r * ib + bot.r * fb, top.g * ib + bot.g * fb, top.b * ib + bot.b * fb};
}
// Level 0: packed texels decoded through the table.  A NaN coordinate takes texel (0, 0).
BH_LENS_HD Rgb sample(const SkyView& s, const float* lut, float u, float v) {
    if (u != u || v != v) return decode(lut, texel(s, 0, 0));
    return bilinear(s.w, s.h, u, v, [&](int32_t x, int32_t y) { return texel(s, x, y); },
                    [&](uint32_t t) { return decode(lut, t); });
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
// A record is named by a cursor C: c.col() shades it, c.right(n) and c.down(n) name the record n columns or
// rows on, and C::barrier_at<K>() is the N at which sum_x holds the scheduler (0: nowhere).  The filtered shade's
// records (MipLens::Cursor) go through this form, the plain shade's through the pointer form below.
template <int N, int K, bool BO, class C>
BH_LENS_FI Acc sum_x(const C& c) {
    if constexpr (N == 1) {
        Acc a{c.col(), {0.0f, 0.0f, 0.0f}};
        if constexpr (BO) a.bo = blackout(a.col);
        return a;
    } else {
        const Acc lo = sum_x<N / 2, K, BO>(c), hi = sum_x<N / 2, K, BO>(c.right(N / 2));
        const Acc r = add<BO>(lo, hi);
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (N == C::template barrier_at<K>()) __builtin_amdgcn_sched_barrier(0);
#endif
        return r;
    }
}
template <int N, int K, bool BO, class C>
BH_LENS_FI Acc sum_y(const C& c) {
    if constexpr (N == 1) {
        return sum_x<K, K, BO>(c);
    } else {
        const Acc lo = sum_y<N / 2, K, BO>(c), hi = sum_y<N / 2, K, BO>(c.down(N / 2));
        return add<BO>(lo, hi);
    }
}
// The tree's result as the pixel: one multiply by 1 / K^2 (a power of two: exact)
template <int K, bool BO>
BH_LENS_HD Acc scaled(Acc a) {
    if constexpr (K > 1) {
        constexpr float scale = 1.0f / (float)(K * K);
        a.col = {a.col.r * scale, a.col.g * scale, a.col.b * scale};
        if constexpr (BO) a.bo = {a.bo.r * scale, a.bo.g * scale, a.bo.b * scale};
    }
    return a;
}

// The plain shade's tree: the same two recursions with a record named by its pointer and the rows vw records
// apart.  It is kept beside the cursor form: over a pointer cursor the K = 2, 4 and 8 kernels came out with other
// instruction order and measured 0.1 to 1.0 % slower at K = 8 in two sessions; this form
// gives the machine code they had.
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

// The plain shade's lens: the records of a width-pixel-wide output frame's virtual frame (K * width per row),
// each shaded from its own two words.  pixel<K, BO>(x, y): output pixel (x, y) from its K x K records.
struct PlainLens {
    const bh_lens_px* lens;
    uint32_t width;
    SkyView s;
    const float* lut;
    template <int K, bool BO>
    BH_LENS_FI Acc pixel(uint32_t x, uint32_t y) const {
        const size_t vw = (size_t)width * K;
        return scaled<K, BO>(sum_y<K, K, BO>(lens + (size_t)y * K * vw + (size_t)x * K, vw, s, lut));
    }
};

// Output pixel (x, y) from a lens L (PlainLens, MipLens)
template <int K, bool BO, class L>
BH_LENS_FI Acc shade_pixel(const L& lens, uint32_t x, uint32_t y) { return lens.template pixel<K, BO>(x, y); }

// ---- the filtered shade (include/bh_render.h, "Filtered lens shades"): a mip chain of the sky, the level of a
// record taken from its neighbours in the lens.  bh_lens.hip runs these per texel and per output pixel,
// bh_sky_mips_host and bh_lens_shade_mip_host (bh_mirror.cpp) the same functions in loops.
constexpr uint32_t MIP_MAX_LEVELS = 16;  // a side is at most 32768 = 2^15

BH_LENS_HD uint32_t mip_levels(uint32_t w0, uint32_t h0) {
    uint32_t m = w0 > h0 ? w0 : h0, n = 1;
    while (m >>= 1) ++n;
    return n;
}
BH_LENS_HD uint32_t mip_side(uint32_t s0, uint32_t l) { return (s0 >> l) != 0u ? s0 >> l : 1u; }
// off[l], l in 1..n-1: the first texel of level l in the chain's storage (levels 1.. back to back, 8 bytes per
// texel); off[0] = 0 is not used.  Returns the chain's texels: under 2^30 / 3 + 2^16.
BH_LENS_HD uint32_t mip_offsets(uint32_t w0, uint32_t h0, uint32_t off[MIP_MAX_LEVELS]) {
    uint32_t at = 0;
    const uint32_t n = mip_levels(w0, h0);
    for (uint32_t l = 0; l < MIP_MAX_LEVELS; ++l) {
        off[l] = l >= 1u && l < n ? at : 0u;
        if (l >= 1u && l < n) at += mip_side(w0, l) * mip_side(h0, l);
    }
    return at;
}

// A texel of a level >= 1: four halves r, g, b, 1.0 as two little-endian words (r | g << 16, b | a << 16).  The
// device converts with its instructions; the host spells both conversions out on the bits, so the mirrors need
// no half-float support from the host compiler's runtime.
struct Half4 { uint32_t lo, hi; };
BH_LENS_HD float half_to_f32(uint32_t h) {  // exact
#if defined(__HIP_DEVICE_COMPILE__)
    const uint16_t b = (uint16_t)h;
    return (float)*reinterpret_cast<const _Float16*>(&b);
#else
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    const float s = (h & 0x8000u) ? -1.0f : 1.0f;
    if (e == 0u) return s * ((float)m * 0x1p-24f);
    if (e == 31u) return m ? NAN : s * INFINITY;
    return s * ldexpf((float)(m | 1024u), (int)e - 25);
#endif
}
BH_LENS_HD uint32_t f32_to_half(float f) {  // round to nearest even
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = (_Float16)f;
    return *reinterpret_cast<const uint16_t*>(&h);
#else
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, ex = (x >> 23) & 255u;
    uint32_t man = x & 0x7fffffu;
    if (ex == 255u) return sign | 0x7c00u | (man ? 0x200u : 0u);
    const int32_t e = (int32_t)ex - 127 + 15;
    if (e >= 31) return sign | 0x7c00u;
    if (e <= 0) {  // a subnormal half, or zero: man * 2^(e - 14) in units of 2^-24
        if (e < -10) return sign;
        man |= 0x800000u;
        const uint32_t shift = (uint32_t)(14 - e), q = man >> shift, rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
    }
    const uint32_t q = ((uint32_t)e << 10) | (man >> 13), rem = man & 0x1fffu;
    return sign | (q + ((rem > 0x1000u || (rem == 0x1000u && (q & 1u))) ? 1u : 0u));  // a carry into the exponent is the rounding
#endif
}
BH_LENS_HD Rgb widen(Half4 t) { return {half_to_f32(t.lo & 0xffffu), half_to_f32(t.lo >> 16), half_to_f32(t.hi & 0xffffu)}; }

// 8-byte load and store of a texel of a level >= 1
BH_LENS_HD Half4 load_half4(const Half4* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    return {t.x, t.y};
#else
    return *p;
#endif
}
BH_LENS_HD void store_half4(Half4* p, Half4 t) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint2*>(p) = make_uint2(t.lo, t.hi);
#else
    *p = t;
#endif
}

// A texel of level l from its four sources a b / c d of level l - 1 (the normative average, alpha 1.0).
BH_LENS_HD Half4 mip_texel(Rgb a, Rgb b, Rgb c, Rgb d) {
    const float r = ((a.r + b.r) + (c.r + d.r)) * 0.25f, g = ((a.g + b.g) + (c.g + d.g)) * 0.25f;
    const float bl = ((a.b + b.b) + (c.b + d.b)) * 0.25f;
    return {f32_to_half(r) | f32_to_half(g) << 16, f32_to_half(bl) | 0x3c00u << 16};
}
// Texel (i, j) of level 1 from level 0 (w x h), and of a level l >= 2 from level l - 1 (w x h): the second
// source of an axis clamps to the last texel, so a side that has reached 1 (or an odd side's last texel) holds.
BH_LENS_HD Half4 mip_down0(const SkyView& s, const float* lut, uint32_t i, uint32_t j) {
    const int32_t wm = (int32_t)s.w - 1, hm = (int32_t)s.h - 1;
    const int32_t x0 = clampi((int32_t)(2u * i), 0, wm), x1 = clampi((int32_t)(2u * i + 1u), 0, wm);
    const int32_t y0 = clampi((int32_t)(2u * j), 0, hm), y1 = clampi((int32_t)(2u * j + 1u), 0, hm);
    const uint32_t a = texel(s, x0, y0), b = texel(s, x1, y0), c = texel(s, x0, y1), d = texel(s, x1, y1);
    return mip_texel(decode(lut, a), decode(lut, b), decode(lut, c), decode(lut, d));
}
BH_LENS_HD Half4 mip_down(const Half4* src, uint32_t w, uint32_t h, uint32_t i, uint32_t j) {
    const uint32_t x0 = 2u * i < w - 1u ? 2u * i : w - 1u, x1 = 2u * i + 1u < w - 1u ? 2u * i + 1u : w - 1u;
    const uint32_t y0 = 2u * j < h - 1u ? 2u * j : h - 1u, y1 = 2u * j + 1u < h - 1u ? 2u * j + 1u : h - 1u;
    const Half4 a = load_half4(src + y0 * w + x0), b = load_half4(src + y0 * w + x1);
    const Half4 c = load_half4(src + y1 * w + x0), d = load_half4(src + y1 * w + x1);
    return mip_texel(widen(a), widen(b), widen(c), widen(d));
}

// A sky with its chain: level 0 as SkyView, the levels >= 1 at chain + off[l].
struct MipView {
    SkyView s;
    const Half4* chain;
    const uint32_t* off;  // MIP_MAX_LEVELS entries (mip_offsets)
    uint32_t n_levels;
};

// sample() on level l >= 1: its sides, its half texels widened, no table.  The coordinates are a valid
// record's (no NaN: an invalid record never comes here).
BH_LENS_HD Rgb sample_mip(const MipView& m, uint32_t l, float u, float v) {
    const uint32_t w = mip_side(m.s.w, l), h = mip_side(m.s.h, l);
    const Half4* lev = m.chain + m.off[l];
    return bilinear(w, h, u, v, [&](int32_t x, int32_t y) { return load_half4(lev + (uint32_t)y * w + (uint32_t)x); },
                    [](Half4 t) { return widen(t); });
}

BH_LENS_HD bool valid_px(bh_lens_px r) { return r.u >= 0.0f && r.v == r.v; }
// F of one axis: the squared footprint, in level-0 texels, between a valid centre c and its neighbour n
BH_LENS_HD float footprint(bh_lens_px c, bh_lens_px n, float w0, float h0) {
    if (!valid_px(n)) return 0.0f;
    float du = fabsf(n.u - c.u);
    if (du > 0.5f) du = 1.0f - du;  // the seam
    const float dv = fabsf(n.v - c.v);
    const float su = du * w0, sv = dv * h0;
    return su * su + sv * sv;
}
BH_LENS_HD int32_t float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_int(f);
#else
    int32_t i;
    memcpy(&i, &f, 4);
    return i;
#endif
}

// col of the record c from its neighbours xn and yn: the level from the footprint, two levels blended.  An axis
// without a neighbour passes an invalid record: F = 0 either way.
BH_LENS_HD Rgb shade_mip_rec(bh_lens_px c, bh_lens_px xn, bh_lens_px yn, const MipView& m, const float* lut) {
    if (!valid_px(c) || m.n_levels == 1u) return shade(c.u, c.v, m.s, lut);
    const float w0 = (float)m.s.w, h0 = (float)m.s.h;
    const float rho2 = fmaxf(footprint(c, xn, w0, h0), footprint(c, yn, w0, h0));
    const int32_t q = float_bits(rho2) - 0x3f800000;  // log2(rho2), 9.23 fixed point
    if (q <= 0) return shade(c.u, c.v, m.s, lut);
    const uint32_t L = (uint32_t)(q >> 24);
    Rgb col;
    if (L >= m.n_levels - 1u) {
        col = sample_mip(m, m.n_levels - 1u, c.u, c.v);
    } else {
        const float f = (float)(q & 0xffffff) * 0x1p-24f, g = 1.0f - f;
        const Rgb lo = L == 0u ? sample(m.s, lut, c.u, c.v) : sample_mip(m, L, c.u, c.v);
        const Rgb hi = sample_mip(m, L + 1u, c.u, c.v);
        col = {lo.r * g + hi.r * f, lo.g * g + hi.g * f, lo.b * g + hi.b * f};
    }
    col.g = col.g * sqrtf(col.g);
    col.b = col.b * sqrtf(col.b);
    return col;
}
// Record (vx, vy) of a lens of vw x vh records and its neighbours, three loads.  Every index stays inside
// vw x vh: a last column or row looks backwards, a side of 1 has no neighbour.
BH_LENS_HD Rgb shade_mip(const bh_lens_px* lens, uint32_t vw, uint32_t vh, uint32_t vx, uint32_t vy, const MipView& m,
                         const float* lut) {
    const size_t at = (size_t)vy * vw + vx;
    const bh_lens_px none{BH_LENS_BLACKOUT, 0.0f};
    const bh_lens_px c = load_px(lens + at);
    const bh_lens_px xn = vw > 1u ? load_px(vx + 1u < vw ? lens + at + 1 : lens + at - 1) : none;
    const bh_lens_px yn = vh > 1u ? load_px(vy + 1u < vh ? lens + at + vw : lens + at - vw) : none;
    return shade_mip_rec(c, xn, yn, m, lut);
}

// The filtered shade's lens: the same records, each named by its place in the virtual frame (K * width x
// K * height), since a record's neighbour is the virtual grid's, not the output pixel's.
struct MipLens {
    const bh_lens_px* lens;
    uint32_t width, height;
    MipView m;
    const float* lut;
    struct Cursor {
        const MipLens& f;
        uint32_t vw, vh, vx, vy;
        BH_LENS_FI Rgb col() const { return shade_mip(f.lens, vw, vh, vx, vy, f.m, f.lut); }
        BH_LENS_FI Cursor right(int n) const { return {f, vw, vh, vx + n, vy}; }
        BH_LENS_FI Cursor down(int n) const { return {f, vw, vh, vx, vy + n}; }
        // K = 4: two records, up to four bilinear samples, in flight at a time (what the plain tree does at K = 8)
        template <int K>
        static constexpr int barrier_at() { return K == 4 ? 2 : 0; }
    };
    template <int K, bool BO>
    BH_LENS_FI Acc pixel(uint32_t x, uint32_t y) const {
        return scaled<K, BO>(sum_y<K, K, BO>(Cursor{*this, width * K, height * K, x * K, y * K}));
    }
};

// ---- the disc shade (include/bh_render.h, "Disc shades"): bh_shade_lens with the surface records looked up in a
// disc texture at the place the hit map names.  bh_disc.hip runs these per output pixel, bh_lens_shade_disc_host
// (bh_mirror.cpp) the same functions in a loop.  The header's rule, op for op: fp32, one rounding per op (both
// units are built without contraction, the device one with correctly rounded fp32 division and square root).
struct DiscView {
    const uint32_t* texels;  // n_phi x n_r, r | g << 8 | b << 16 | a << 24 per texel
    uint32_t n_phi, n_r;
    float rs;
    uint32_t scene_flags;
    float spin, gain;
};
constexpr float DISC_TWO_PI = 6.28318530718f, DISC_ONE_PI = 3.14159265359f;  // the sky's u (:82-83)

// RN_f32 of the f64 atan2(z, x): on the device the short f64 core with the library call for the lanes it cannot
// decide (sky_uv's pair, bh_march_shade.hpp), on the host the library call.
// (BH_DISC_ANGLE_F32, a measurement switch of variant builds only: the fp32 library atan2 in its place, not the
// rule's bits -- tools/bench_disc.py takes the share of the f64 angle in the shade's time from such a build.)
BH_LENS_HD float disc_angle(float z, float x) {
#if defined(BH_DISC_ANGLE_F32)
    return atan2f(z, x);
#elif defined(__HIP_DEVICE_COMPILE__)
    const crm::Atan2 at = crm::atan2_core(z, x);
    float az = at.f;
    if (__builtin_expect(at.near, 0)) az = (float)atan2((double)z, (double)x);
    return az;
#else
    return (float)atan2((double)z, (double)x);
#endif
}

// Steps 3 to 5 of the rule: the colour of a surface record whose ray ended at p = (x, y, z), disc enabled.
BH_LENS_HD Rgb disc_colour(float x, float y, float z, const DiscView& d, const float* lut) {
    const float rho = sqrtf(x * x + z * z);
    const float ri = 3.0f * d.rs, ro = 6.0f * d.rs;
    const float sd = fmaxf(fmaxf(rho - ro, -(rho - ri)), fabsf(y) - 0.02f);
    if (!(sd < 0.001f)) return {1.0f, 1.0f, 1.0f};  // a marker
    const float a = (rho - ri) / ri;
    const float k = ri / rho;
    const float w = k * sqrtf(k);
    const float t0 = (disc_angle(z, x) + DISC_ONE_PI) / DISC_TWO_PI;
    const float t1 = t0 - d.spin * w;
    float t = t1 - floorf(t1);
    if (!(t >= 0.0f)) t = 0.0f;  // a NaN t (a NaN hit component, or rs at which w is not finite)
    // bilinear's arithmetic, the x axis wrapping: t in [0, 1], so floor(tx) in [-1, n_phi - 1]
    const float tx = t * (float)d.n_phi - 0.5f;
    float ty = a * (float)d.n_r - 0.5f;
    ty = fminf(fmaxf(ty, -1.0f), (float)d.n_r);
    const float fx0 = floorf(tx), fy0 = floorf(ty);
    const float fa = tx - fx0, fb = ty - fy0;
    int32_t x0 = (int32_t)fx0, y0 = (int32_t)fy0;
    const int32_t np = (int32_t)d.n_phi, hm = (int32_t)d.n_r - 1;
    x0 = x0 < 0 ? x0 + np : x0;
    const int32_t x1 = x0 + 1 == np ? 0 : x0 + 1, y1 = clampi(y0 + 1, 0, hm);
    y0 = clampi(y0, 0, hm);
    const uint32_t w00 = d.texels[(uint32_t)y0 * d.n_phi + (uint32_t)x0], w10 = d.texels[(uint32_t)y0 * d.n_phi + (uint32_t)x1];
    const uint32_t w01 = d.texels[(uint32_t)y1 * d.n_phi + (uint32_t)x0], w11 = d.texels[(uint32_t)y1 * d.n_phi + (uint32_t)x1];
    const Rgb t00 = decode(lut, w00), t10 = decode(lut, w10), t01 = decode(lut, w01), t11 = decode(lut, w11);
    const float ia = 1.0f - fa, ib = 1.0f - fb;
    const Rgb top = {t00.r * ia + t10.r * fa, t00.g * ia + t10.g * fa, t00.b * ia + t10.b * fa};
    const Rgb bot = {t01.r * ia + t11.r * fa, t01.g * ia + t11.g * fa, t01.b * ia + t11.b * fa};
    const Rgb c = {top.r * ib + bot.r * fb, top.g * ib + bot.g * fb, top.b * ib + bot.b * fb};
    return {c.r * d.gain, c.g * d.gain, c.b * d.gain};
}
// col of one record and its hit (three floats, read for a surface record of a scene with the disc only)
BH_LENS_HD Rgb shade_disc(float u, float v, const float* hit, const DiscView& d, const SkyView& s, const float* lut) {
    if (u != BH_LENS_SURFACE) return shade(u, v, s, lut);
    if (!(d.scene_flags & BH_SCENE_DISC)) return {1.0f, 1.0f, 1.0f};
    return disc_colour(hit[0], hit[1], hit[2], d, lut);
}

// The disc shade's lens: the plain shade's records, each beside its 12 bytes of the hit map, through the cursor
// form of the tree.
struct DiscLens {
    const bh_lens_px* lens;
    const float* hits;
    uint32_t width;
    SkyView s;
    DiscView d;
    const float* lut;
    struct Cursor {
        const DiscLens& f;
        size_t vw, at;  // the virtual frame's width and the record's index
        BH_LENS_FI Rgb col() const {
            const bh_lens_px r = load_px(f.lens + at);
            return shade_disc(r.u, r.v, f.hits + at * 3u, f.d, f.s, f.lut);
        }
        BH_LENS_FI Cursor right(int n) const { return {f, vw, at + (size_t)n}; }
        BH_LENS_FI Cursor down(int n) const { return {f, vw, at + (size_t)n * vw}; }
        // K = 8: four samples in flight at a time, as the plain tree holds them
        template <int K>
        static constexpr int barrier_at() { return K == 8 ? 4 : 0; }
    };
    template <int K, bool BO>
    BH_LENS_FI Acc pixel(uint32_t x, uint32_t y) const {
        const size_t vw = (size_t)width * K;
        return scaled<K, BO>(sum_y<K, K, BO>(Cursor{*this, vw, (size_t)y * K * vw + (size_t)x * K}));
    }
};

// ---- the beamed disc shade (include/bh_render.h, "Beamed disc shades"): the disc shade with a disc hit's colour
// multiplied by the fourth power of the frequency ratio g of a Keplerian emitter, formed from the hit and the ray's
// arrival there (the lens's arrival map).  bh_disc.hip and bh_lens_shade_disc_beamed_host run these; the header's
// steps 6 to 8, op for op, as above.
struct BeamView {
    float beam;   // 0 .. 1
    float sense;  // +1.0f or -1.0f
    float dp;     // the uniforms' distortion_power
};
BH_LENS_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
// Step 3's test alone (disc_colour's first four lines, which the compiler merges with them): is p a disc hit, and rho.
BH_LENS_HD bool disc_on(float x, float y, float z, float rs, float* rho_out) {
    const float rho = sqrtf(x * x + z * z);
    const float ri = 3.0f * rs, ro = 6.0f * rs;
    const float sd = fmaxf(fmaxf(rho - ro, -(rho - ri)), fabsf(y) - 0.02f);
    *rho_out = rho;
    return sd < 0.001f;
}
// Steps 6 to 8 up to the factor f of a disc hit p = (x, y, z) with arrival d = (dx, dy, dz) and step 3's rho.
BH_LENS_HD float beam_factor(float x, float y, float z, float dx, float dy, float dz, float rho, float rs, const BeamView& b) {
    const float r2 = dot3(x, y, z, x, y, z), r = sqrtf(r2);                                       // 6.
    const float lx = y * dz - z * dy, ly = z * dx - x * dz, lz = x * dy - y * dx;
    const float h2 = dot3(lx, ly, lz, lx, ly, lz);
    const float e2 = dot3(dx, dy, dz, dx, dy, dz) - ((b.dp * rs) * h2) / (r2 * r);
    const float e = sqrtf(e2);
    const float om = sqrtf((0.5f * rs) / ((rho * rho) * rho));                                    // 7.
    const float q = 1.0f - (1.5f * rs) / rho;
    const float den = 1.0f - (b.sense * om) * (ly / e);
    float g = sqrtf(q) / den;
    if (!((e2 > 0.0f) & (q > 0.0f) & (den > 0.0f) & (g < INFINITY))) g = 1.0f;
    const float ge = 1.0f + b.beam * (g - 1.0f);                                                  // 8.
    // finite: g > 1 needs a finite om, so rs > 0 and q < 1, and a positive fp32 den is 2^-24 at least -- g < 2^24
    return (ge * ge) * (ge * ge);
}
// col of one record, its hit and its arrival: both 12-byte loads of a surface record of a scene with the disc issued
// before either is used; the arrival enters the colour of a disc hit alone
BH_LENS_HD Rgb shade_disc_beamed(float u, float v, const float* hit, const float* arr, const DiscView& d, const BeamView& b,
                                 const SkyView& s, const float* lut) {
    if (u != BH_LENS_SURFACE) return shade(u, v, s, lut);
    if (!(d.scene_flags & BH_SCENE_DISC)) return {1.0f, 1.0f, 1.0f};
    const float x = hit[0], y = hit[1], z = hit[2], dx = arr[0], dy = arr[1], dz = arr[2];
    const Rgb c = disc_colour(x, y, z, d, lut);
    float rho;
    if (!disc_on(x, y, z, d.rs, &rho)) return c;  // a marker: disc_colour's (1, 1, 1)
    const float f = beam_factor(x, y, z, dx, dy, dz, rho, d.rs, b);
    return {c.r * f, c.g * f, c.b * f};
}

// The beamed disc shade's lens: DiscLens with the record's 12 bytes of the arrival map beside its hit's.
struct BeamLens {
    const bh_lens_px* lens;
    const float* hits;
    const float* arrivals;
    uint32_t width;
    SkyView s;
    DiscView d;
    BeamView b;
    const float* lut;
    struct Cursor {
        const BeamLens& f;
        size_t vw, at;  // the virtual frame's width and the record's index
        BH_LENS_FI Rgb col() const {
            const bh_lens_px r = load_px(f.lens + at);
            return shade_disc_beamed(r.u, r.v, f.hits + at * 3u, f.arrivals + at * 3u, f.d, f.b, f.s, f.lut);
        }
        BH_LENS_FI Cursor right(int n) const { return {f, vw, at + (size_t)n}; }
        BH_LENS_FI Cursor down(int n) const { return {f, vw, at + (size_t)n * vw}; }
        template <int K>
        static constexpr int barrier_at() { return K == 8 ? 4 : 0; }
    };
    template <int K, bool BO>
    BH_LENS_FI Acc pixel(uint32_t x, uint32_t y) const {
        const size_t vw = (size_t)width * K;
        return scaled<K, BO>(sum_y<K, K, BO>(Cursor{*this, vw, (size_t)y * K * vw + (size_t)x * K}));
    }
};

}  // namespace lens
}  // namespace bh
