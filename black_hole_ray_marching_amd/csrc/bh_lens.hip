// bh_lens.hip — bh_shade_lens: a lens map (include/bh_render.h, bh_lens_px) and a sky -> the frame's targets.
// Built -ffp-contract=off with correctly rounded fp32 sqrt: the arithmetic is bh_lens.hpp's, shared with the host.
//
// Per sample one 8-byte record is read and four sky texels gathered (L2-resident: neighbouring rays land on
// neighbouring texels), per output pixel 4 to 16 bytes are written per target.  One thread per OUTPUT pixel, a
// wave on 64 consecutive pixels of one row: the wave reads 64 * ss records of each of its ss lens rows as one
// contiguous run (512 B at ss 1, 4 KiB at ss 8) and stores one contiguous run per target; a thread loops over
// its ss x ss records.  Measured: 0.6-0.7 of a copy of its bytes at ss 1; from ss 2 on the
// ~140 VALU instructions per sample bound it.  (One lane per sample with bh_ss.hpp's butterfly over an 8x8
// block -- the march kernel's mapping -- reads 64-byte pieces of eight rows instead and measured 1.2-1.6x
// slower at ss 2 and 4.)
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "bh_common.hpp"
#include "bh_lens.hpp"
#include "bh_srgb.hpp"

namespace bh {
namespace lens {

constexpr uint32_t ROWS = 4;  // rows of 64 pixels per 256-thread workgroup

// the output formats' stores: store_px's (bh_march_shade.hpp), vector stores only
template <uint32_t FMT>
__device__ __forceinline__ void store_texel(void* base, size_t idx, Rgb c, const float* enc) {
    if constexpr (FMT == BH_OUT_RGBA32F) {
        reinterpret_cast<float4*>(base)[idx] = make_float4(c.r, c.g, c.b, 1.0f);
    } else if constexpr (FMT == BH_OUT_RGBA16F) {
        __half2 lo = __floats2half2_rn(c.r, c.g);
        __half2 hi = __floats2half2_rn(c.b, 1.0f);
        uint2 w;
        w.x = *reinterpret_cast<uint32_t*>(&lo);
        w.y = *reinterpret_cast<uint32_t*>(&hi);
        reinterpret_cast<uint2*>(base)[idx] = w;
    } else {
        static_assert(FMT == BH_OUT_BGRA8_SRGB, "output format");
        reinterpret_cast<uint32_t*>(base)[idx] = srgb_bgra8(c.r, c.g, c.b, enc);
    }
}

template <uint32_t FMT, int K>
__global__ void __launch_bounds__(64 * ROWS) lens_shade_kernel(LensShadeArgs a) {
    // [0, 256) the sRGB decode of sky texels, then for BGRA8 output the encoder's 257 thresholds
    __shared__ float tab[FMT == BH_OUT_BGRA8_SRGB ? 256 + SRGB_TABLE : 256];
    tab[threadIdx.x] = a.srgb_lut[threadIdx.x];
    if constexpr (FMT == BH_OUT_BGRA8_SRGB) {
        tab[256 + threadIdx.x] = a.srgb_enc[threadIdx.x];
        if (threadIdx.x == 0) tab[256 + 256] = a.srgb_enc[256];
    }
    __syncthreads();
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * ROWS + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;  // a partial last column or row: no load, no store
    const SkyView s{a.sky, a.sky_w, a.sky_h};
    const size_t idx = (size_t)y * a.width + x;
    if (a.out_blackout) {  // uniform over the launch
        const Acc p = shade_pixel<K, true>(a.lens, a.width, x, y, s, tab);
        store_texel<FMT>(a.out_col, idx, p.col, tab + 256);
        store_texel<FMT>(a.out_blackout, idx, p.bo, tab + 256);
    } else {
        const Acc p = shade_pixel<K, false>(a.lens, a.width, x, y, s, tab);
        store_texel<FMT>(a.out_col, idx, p.col, tab + 256);
    }
}
static_assert(64 * ROWS == 256, "the table load is one entry per thread");

template <uint32_t FMT>
int launch(const LensShadeArgs& a, uint32_t ss, hipStream_t s) {
    const dim3 grid((a.width + 63u) / 64u, (a.height + ROWS - 1u) / ROWS), block(64u * ROWS);
    switch (ss) {
        case 1u: hipLaunchKernelGGL((lens_shade_kernel<FMT, 1>), grid, block, 0, s, a); break;
        case 2u: hipLaunchKernelGGL((lens_shade_kernel<FMT, 2>), grid, block, 0, s, a); break;
        case 4u: hipLaunchKernelGGL((lens_shade_kernel<FMT, 4>), grid, block, 0, s, a); break;
        case 8u: hipLaunchKernelGGL((lens_shade_kernel<FMT, 8>), grid, block, 0, s, a); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

}  // namespace lens
}  // namespace bh

// width, height <= 65536 (bh_shade_lens): at most 1024 x 16384 workgroups
extern "C" __attribute__((visibility("hidden"))) int bh_launch_lens_shade(const bh::LensShadeArgs& a, uint32_t ss,
                                                                        uint32_t format, hipStream_t s) {
    switch (format) {
        case BH_OUT_RGBA32F: return bh::lens::launch<BH_OUT_RGBA32F>(a, ss, s);
        case BH_OUT_RGBA16F: return bh::lens::launch<BH_OUT_RGBA16F>(a, ss, s);
        case BH_OUT_BGRA8_SRGB: return bh::lens::launch<BH_OUT_BGRA8_SRGB>(a, ss, s);
        default: return (int)hipErrorInvalidValue;
    }
}
