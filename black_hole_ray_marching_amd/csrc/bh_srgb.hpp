// bh_srgb.hpp — linear f32 -> sRGB byte, the store of a Bgra8UnormSrgb render target (the reference's
// surface/consumer format: src/scene.rs:259-274, src/copy.rs:132, src/remix.rs:160).
//
// Normative encode (oracle/bh_oracle.c bho_srgb_encode): clamp to [0, 1] (NaN -> 0), the sRGB OETF in
// double, round half up to 0..255.  It is monotone in x, so it is fully described by 255 thresholds:
// T[k] = the smallest float with code >= k (bh_host.cpp builds them from the definition; T[0] = 0,
// T[256] = +inf).  On the GPU a hardware-log2/exp2 evaluation of the OETF lands within one code of
// the answer, and the two neighbouring thresholds fix it: exact for every float (checked
// exhaustively on the device, bh_selftest_crmath op 4).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bh_render.h"

namespace bh {

constexpr int SRGB_TABLE = 257;

__device__ __forceinline__ uint32_t srgb_encode(float x, const float* T) {
    const float xc = fminf(fmaxf(x, 0.0f), 1.0f);  // fmaxf(NaN, 0) = 0
    const float s = xc <= 0.0031308f ? 12.92f * xc
                                     : 1.055f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(xc) * (1.0f / 2.4f)) - 0.055f;
    int c = (int)(s * 255.0f + 0.5f);
    c = c < 0 ? 0 : (c > 255 ? 255 : c);
    c = (xc < T[c]) ? c - 1 : c;        // T[0] = 0 <= xc: never below 0
    c = (xc >= T[c + 1]) ? c + 1 : c;   // T[256] = +inf: never above 255
    return (uint32_t)c;
}

// Table form without log2/exp2 (the bloom chain stores ~9 channels per pixel): on [2^-13, 1) every
// bucket of 2^-7 relative width (7 mantissa bits) spans at most one code boundary, so the code is
// the bucket's base code B[i] (the code of its lower end) plus one where x reaches T[B[i] + 1].
// Below 2^-13 the code is 0 (T[1] > 2^-13), which bucket 0 already gives.  Exhaustively checked on
// the device (bh_selftest_crmath op 6).  The host builds B from T (bh_host.cpp).
constexpr uint32_t SRGB_BUCKET_SHIFT = 16;
constexpr uint32_t SRGB_BUCKET_BASE = (127u - 13u) << 7;  // bucket index of 2^-13
constexpr int SRGB_BUCKETS = 13 * 128;                   // [2^-13, 1)

__device__ __forceinline__ uint32_t srgb_encode_lut(float x, const uint8_t* B, const float* T) {
    const float xc = fminf(fmaxf(x, 0.0f), 1.0f);  // fmaxf(NaN, 0) = 0
    int32_t i = (int32_t)(__float_as_uint(xc) >> SRGB_BUCKET_SHIFT) - (int32_t)SRGB_BUCKET_BASE;
    i = i < 0 ? 0 : (i > SRGB_BUCKETS - 1 ? SRGB_BUCKETS - 1 : i);
    const uint32_t c = B[i];
    return c + (xc >= T[c + 1] ? 1u : 0u);
}

// Code-table form (one LDS read instead of two dependent ones): within a bucket every float shares its
// upper 16 bits, so the one threshold a bucket may hold is fixed by its low 16 bits.  Entry i =
// base code | thr17 << 15, thr17 = the threshold's low 16 bits, or 0x10000 (never reached) when the
// bucket holds none: code = base + (low16(x) >= thr17).  Entry SRGB_BUCKETS is 1.0 (code 255); values
// below 2^-13 clamp to entry 0, which holds no threshold (T[1] > 2^-13 * (1 + 2^-7)).  Built by the host
// (bh_host.cpp, bh_srgb_code_table); exhaustively checked on the device (bh_selftest_crmath op 10).
constexpr int SRGB_CODES = SRGB_BUCKETS + 1;
__device__ __forceinline__ uint32_t srgb_encode_code(float x, const uint32_t* E) {
    const float xc = fminf(fmaxf(x, 0.0f), 1.0f);  // fmaxf(NaN, 0) = 0
    const uint32_t b = __float_as_uint(xc);
    int32_t i = (int32_t)(b >> SRGB_BUCKET_SHIFT) - (int32_t)SRGB_BUCKET_BASE;
    i = i < 0 ? 0 : (i > SRGB_BUCKETS ? SRGB_BUCKETS : i);
    const uint32_t e = E[i];
    return (e & 0xFFu) + ((b & 0xFFFFu) >= (e >> 15) ? 1u : 0u);
}

// BGRA8 texel (byte 0 = B) of linear rgb, alpha 1.
__device__ __forceinline__ uint32_t srgb_bgra8(float r, float g, float b, const float* T) {
    return srgb_encode(b, T) | (srgb_encode(g, T) << 8) | (srgb_encode(r, T) << 16) | 0xFF000000u;
}

// Output texel store of every row-major target (the march's, the lens shades'); the format is a template
// parameter (one kernel instantiation per format keeps the BGRA8 encoder out of the other formats' code: it
// measured 1.8 % on the RGBA16F march kernel).  Vector stores only.
template <uint32_t FMT>
__device__ __forceinline__ void store_rgb(void* base, size_t idx, float r, float g, float b, const float* enc) {
    if constexpr (FMT == BH_OUT_RGBA32F) {
        reinterpret_cast<float4*>(base)[idx] = make_float4(r, g, b, 1.0f);
    } else if constexpr (FMT == BH_OUT_RGBA16F) {
        __half2 lo = __floats2half2_rn(r, g);
        __half2 hi = __floats2half2_rn(b, 1.0f);
        uint2 w;
        w.x = *reinterpret_cast<uint32_t*>(&lo);
        w.y = *reinterpret_cast<uint32_t*>(&hi);
        reinterpret_cast<uint2*>(base)[idx] = w;
    } else {
        static_assert(FMT == BH_OUT_BGRA8_SRGB, "output format");
        reinterpret_cast<uint32_t*>(base)[idx] = srgb_bgra8(r, g, b, enc);
    }
}

// LDS tables of a workgroup of NT threads (a divisor or multiple of 256): tab[0, 256) the sRGB decode of sky
// texels, then for BGRA8 output the encoder's 257 thresholds (not read otherwise).  The caller's barrier follows.
// `a` is a launch's arguments, or any struct with their two table pointers srgb_lut and srgb_enc.  (The march
// kernels call this directly, with their MarchArgs: called through a wrapper of their own, the pair and
// persistent kernels came out with the pointer's load one instruction earlier or later than measured.)
struct SrgbTables { const float* srgb_lut; const float* srgb_enc; };
template <uint32_t FMT>
constexpr int lds_tables() { return FMT == BH_OUT_BGRA8_SRGB ? 256 + SRGB_TABLE : 256; }
// ONE_EACH: the workgroup is exactly 256 threads, one entry of each table per thread, no loop and no guard (the lens
// kernels: at ss 1 the guarded loop, which waits for its load inside the guard, measured 1 to 3 % of the launch).
template <uint32_t FMT, uint32_t NT, bool ONE_EACH = false, class Args>
__device__ __forceinline__ void load_srgb_tables(const Args& a, float* tab) {
    static_assert(!ONE_EACH || NT == 256u, "one entry per thread");
#pragma unroll
    for (uint32_t i = threadIdx.x; ONE_EACH ? i == threadIdx.x : i < 256u; i += NT) {
        tab[i] = a.srgb_lut[i];
        if constexpr (FMT == BH_OUT_BGRA8_SRGB) tab[256 + i] = a.srgb_enc[i];
    }
    if constexpr (FMT == BH_OUT_BGRA8_SRGB)
        if (threadIdx.x == 0) tab[256 + 256] = a.srgb_enc[256];
}

// The same copy by a workgroup of ONE wave, in two halves with the caller's own loads between them: 16 bytes of
// each table per lane (srgb_fetch: the loads, nothing waits for them), then one LDS store each (srgb_store: the
// first use, so the only wait), the barrier after it the caller's.  The guarded loop above waits for each of its
// four loads in turn.  Both tables are allocations of their own (bh_host.cpp, upload) and `tab` is 16-byte aligned.
template <uint32_t FMT>
struct SrgbRows { float4 lut, enc; float last; };
template <uint32_t FMT, class Args>
__device__ __forceinline__ SrgbRows<FMT> srgb_fetch(const Args& a) {
    SrgbRows<FMT> r;
    r.lut = reinterpret_cast<const float4*>(a.srgb_lut)[threadIdx.x];
    if constexpr (FMT == BH_OUT_BGRA8_SRGB) {
        r.enc = reinterpret_cast<const float4*>(a.srgb_enc)[threadIdx.x];
        r.last = a.srgb_enc[256];
    }
    return r;
}
template <uint32_t FMT>
__device__ __forceinline__ void srgb_store(const SrgbRows<FMT>& r, float* tab) {
    reinterpret_cast<float4*>(tab)[threadIdx.x] = r.lut;
    if constexpr (FMT == BH_OUT_BGRA8_SRGB) {
        reinterpret_cast<float4*>(tab)[64u + threadIdx.x] = r.enc;
        if (threadIdx.x == 0) tab[256 + 256] = r.last;
    }
}

}  // namespace bh

// The host's builders of B and E from the 257 thresholds (bh_host.cpp; the self-test builds its own copies)
extern "C" __attribute__((visibility("hidden"))) void bh_srgb_bucket_table(const float* T257, uint8_t* B);
extern "C" __attribute__((visibility("hidden"))) bool bh_srgb_code_table(const float* T257, uint32_t* E);
