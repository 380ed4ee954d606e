// bh_lens_mip.hip — bh_sky_create_mips' chain kernels and bh_shade_lens_mip's shade kernel (include/bh_render.h,
// "Filtered lens shades").  Built as bh_lens.hip is: -ffp-contract=off, correctly rounded fp32 sqrt, no SLP; the
// arithmetic is bh_lens.hpp's, shared with the host mirrors.
//
// The shade kernel has lens_shade_kernel's mapping: one thread per OUTPUT pixel, a wave on 64 consecutive pixels
// of one row, 4 rows per workgroup.  Beside its own ss x ss records a thread reads their +1 neighbours in x and
// y straight from the lens: they are the next lane's and the next row's records (the workgroup reads them
// anyway), so the loads hit the L1/L2 lines the centre loads brought in, and no record is staged in LDS -- the
// kernel's one barrier is the table load's, before any thread leaves.  Taps of levels >= 1 are 8-byte loads.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "bh_common.hpp"
#include "bh_lens.hpp"
#include "bh_srgb.hpp"

namespace bh {
namespace lens {

constexpr uint32_t MIP_ROWS = 4;  // rows of 64 pixels (or texels) per 256-thread workgroup
static_assert(sizeof(Half4) == 8, "a texel of a level >= 1 is one 8-byte load or store");
static_assert(sizeof(LensMipArgs::level_off) == MIP_MAX_LEVELS * sizeof(uint32_t), "one offset per level");

// ---- the chain: one launch per level, one thread per destination texel, one 8-byte store each ---------------
__global__ void __launch_bounds__(64 * MIP_ROWS) mip_level1_kernel(const uint32_t* sky, uint32_t w0, uint32_t h0,
                                                                  const float* srgb_lut, Half4* dst, uint32_t w, uint32_t h) {
    __shared__ float tab[256];  // the sRGB decode of level 0's texels
    tab[threadIdx.x] = srgb_lut[threadIdx.x];
    __syncthreads();  // reached by every thread of the workgroup: the bounds test comes after it
    const uint32_t i = blockIdx.x * 64u + (threadIdx.x & 63u), j = blockIdx.y * MIP_ROWS + (threadIdx.x >> 6);
    if (i >= w || j >= h) return;
    store_half4(dst + j * w + i, mip_down0(SkyView{sky, w0, h0}, tab, i, j));
}
__global__ void __launch_bounds__(64 * MIP_ROWS) mip_level_kernel(const Half4* src, uint32_t sw, uint32_t sh, Half4* dst,
                                                                 uint32_t w, uint32_t h) {
    const uint32_t i = blockIdx.x * 64u + (threadIdx.x & 63u), j = blockIdx.y * MIP_ROWS + (threadIdx.x >> 6);
    if (i >= w || j >= h) return;  // no barrier in this kernel
    store_half4(dst + j * w + i, mip_down(src, sw, sh, i, j));
}

// ---- the shade ------------------------------------------------------------------------------------------------
// the output formats' stores, as bh_lens.hip's store_texel (that unit keeps its own copy: its code does not change)
template <uint32_t FMT>
__device__ __forceinline__ void store_out(void* base, size_t idx, Rgb c, const float* enc) {
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
__global__ void __launch_bounds__(64 * MIP_ROWS) lens_shade_mip_kernel(LensMipArgs a) {
    // [0, 256) the sRGB decode of sky texels, then for BGRA8 output the encoder's 257 thresholds
    __shared__ float tab[FMT == BH_OUT_BGRA8_SRGB ? 256 + SRGB_TABLE : 256];
    __shared__ uint32_t off[MIP_MAX_LEVELS];
    tab[threadIdx.x] = a.srgb_lut[threadIdx.x];
    if constexpr (FMT == BH_OUT_BGRA8_SRGB) {
        tab[256 + threadIdx.x] = a.srgb_enc[threadIdx.x];
        if (threadIdx.x == 0) tab[256 + 256] = a.srgb_enc[256];
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t l = 0; l < MIP_MAX_LEVELS; ++l) off[l] = a.level_off[l];  // constant indices: scalar loads
    }
    // The kernel's only barrier.  Every thread of the workgroup reaches it: out-of-frame lanes leave after it,
    // and nothing below waits for another thread (the neighbour records come from the lens, not from LDS).
    __syncthreads();
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * MIP_ROWS + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;  // a partial last column or row: no load, no store
    const MipView m{{a.sky, a.sky_w, a.sky_h}, static_cast<const Half4*>(a.chain), off, a.n_levels};
    const size_t idx = (size_t)y * a.width + x;
    if (a.out_blackout) {  // uniform over the launch
        const Acc p = shade_pixel_mip<K, true>(a.lens, a.width, a.height, x, y, m, tab);
        store_out<FMT>(a.out_col, idx, p.col, tab + 256);
        store_out<FMT>(a.out_blackout, idx, p.bo, tab + 256);
    } else {
        const Acc p = shade_pixel_mip<K, false>(a.lens, a.width, a.height, x, y, m, tab);
        store_out<FMT>(a.out_col, idx, p.col, tab + 256);
    }
}
static_assert(64 * MIP_ROWS == 256, "the table load is one entry per thread");

template <uint32_t FMT>
int launch_mip(const LensMipArgs& a, uint32_t ss, hipStream_t s) {
    const dim3 grid((a.width + 63u) / 64u, (a.height + MIP_ROWS - 1u) / MIP_ROWS), block(64u * MIP_ROWS);
    switch (ss) {
        case 1u: hipLaunchKernelGGL((lens_shade_mip_kernel<FMT, 1>), grid, block, 0, s, a); break;
        case 2u: hipLaunchKernelGGL((lens_shade_mip_kernel<FMT, 2>), grid, block, 0, s, a); break;
        case 4u: hipLaunchKernelGGL((lens_shade_mip_kernel<FMT, 4>), grid, block, 0, s, a); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

}  // namespace lens
}  // namespace bh

// width, height <= 65536 (bh_shade_lens_mip): at most 1024 x 16384 workgroups
extern "C" __attribute__((visibility("hidden"))) int bh_launch_lens_shade_mip(const bh::LensMipArgs& a, uint32_t ss,
                                                                            uint32_t format, hipStream_t s) {
    switch (format) {
        case BH_OUT_RGBA32F: return bh::lens::launch_mip<BH_OUT_RGBA32F>(a, ss, s);
        case BH_OUT_RGBA16F: return bh::lens::launch_mip<BH_OUT_RGBA16F>(a, ss, s);
        case BH_OUT_BGRA8_SRGB: return bh::lens::launch_mip<BH_OUT_BGRA8_SRGB>(a, ss, s);
        default: return (int)hipErrorInvalidValue;
    }
}

// The chain of a w0 x h0 sky into `chain` (lens::mip_offsets texels), level after level on the stream; a level
// has at most 16384 x 16384 texels: at most 256 x 4096 workgroups.
extern "C" __attribute__((visibility("hidden"))) int bh_launch_sky_mips(const uint32_t* sky, uint32_t w0, uint32_t h0,
                                                                      const float* srgb_lut, void* chain, hipStream_t s) {
    using namespace bh::lens;
    uint32_t off[MIP_MAX_LEVELS];
    mip_offsets(w0, h0, off);
    Half4* base = static_cast<Half4*>(chain);
    const uint32_t n = mip_levels(w0, h0);
    for (uint32_t l = 1; l < n; ++l) {
        const uint32_t sw = mip_side(w0, l - 1u), sh = mip_side(h0, l - 1u), w = mip_side(w0, l), h = mip_side(h0, l);
        const dim3 grid((w + 63u) / 64u, (h + MIP_ROWS - 1u) / MIP_ROWS), block(64u * MIP_ROWS);
        if (l == 1u)
            hipLaunchKernelGGL(mip_level1_kernel, grid, block, 0, s, sky, w0, h0, srgb_lut, base + off[1], w, h);
        else
            hipLaunchKernelGGL(mip_level_kernel, grid, block, 0, s, base + off[l - 1u], sw, sh, base + off[l], w, h);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}
