// bh_lens.hip — bh_shade_lens and bh_shade_lens_mip: a lens map (include/bh_render.h, bh_lens_px) and a sky -> the
// frame's targets; bh_sky_create_mips' chain kernels (include/bh_render.h, "Filtered lens shades").
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
//
// The filtered shade has the same mapping.  Beside its own ss x ss records a thread reads their +1 neighbours in
// x and y straight from the lens: they are the next lane's and the next row's records (the workgroup reads them
// anyway), so the loads hit the L1/L2 lines the centre loads brought in, and no record is staged in LDS -- the
// kernel's one barrier is the table load's, before any thread leaves.  Taps of levels >= 1 are 8-byte loads.
#include <hip/hip_runtime.h>

#include "bh_common.hpp"
#include "bh_lens.hpp"
#include "bh_srgb.hpp"

namespace bh {
namespace lens {

constexpr uint32_t ROWS = 4;  // rows of 64 pixels (or texels) per 256-thread workgroup
static_assert(64 * ROWS == 256, "the table load is one entry per thread");
static_assert(sizeof(Half4) == 8, "a texel of a level >= 1 is one 8-byte load or store");
static_assert(sizeof(LensMipArgs::level_off) == MIP_MAX_LEVELS * sizeof(uint32_t), "one offset per level");

// ---- the chain: one launch per level, one thread per destination texel, one 8-byte store each ---------------
__global__ void __launch_bounds__(64 * ROWS) mip_level1_kernel(const uint32_t* sky, uint32_t w0, uint32_t h0,
                                                              const float* srgb_lut, Half4* dst, uint32_t w, uint32_t h) {
    __shared__ float tab[256];  // the sRGB decode of level 0's texels
    load_srgb_tables<BH_OUT_RGBA32F, 64u * ROWS, true>(SrgbTables{srgb_lut, nullptr}, tab);
    __syncthreads();  // reached by every thread of the workgroup: the bounds test comes after it
    const uint32_t i = blockIdx.x * 64u + (threadIdx.x & 63u), j = blockIdx.y * ROWS + (threadIdx.x >> 6);
    if (i >= w || j >= h) return;
    store_half4(dst + j * w + i, mip_down0(SkyView{sky, w0, h0}, tab, i, j));
}
__global__ void __launch_bounds__(64 * ROWS) mip_level_kernel(const Half4* src, uint32_t sw, uint32_t sh, Half4* dst,
                                                             uint32_t w, uint32_t h) {
    const uint32_t i = blockIdx.x * 64u + (threadIdx.x & 63u), j = blockIdx.y * ROWS + (threadIdx.x >> 6);
    if (i >= w || j >= h) return;  // no barrier in this kernel
    store_half4(dst + j * w + i, mip_down(src, sw, sh, i, j));
}

// ---- the shades ------------------------------------------------------------------------------------------------
// Both shade kernels' body.  stage() fills what the shade keeps in LDS beside the tables; lens(tab) is its lens
// (bh_lens.hpp: PlainLens, MipLens) once the tables are there.
// The barrier is the kernel's only one.  Every thread of the workgroup reaches it: out-of-frame lanes leave after
// it, and nothing below waits for another thread (the filtered shade's neighbour records come from the lens, not
// from LDS).
template <uint32_t FMT, int K, class Stage, class Lens>
__device__ __forceinline__ void shade_body(const LensShadeArgs& a, Stage stage, Lens lens) {
    // [0, 256) the sRGB decode of sky texels, then for BGRA8 output the encoder's 257 thresholds
    __shared__ float tab[lds_tables<FMT>()];
    load_srgb_tables<FMT, 64u * ROWS, true>(a, tab);
    stage();
    __syncthreads();
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * ROWS + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;  // a partial last column or row: no load, no store
    const auto l = lens(tab);
    const size_t idx = (size_t)y * a.width + x;
    if (a.out_blackout) {  // uniform over the launch
        const Acc p = shade_pixel<K, true>(l, x, y);
        store_rgb<FMT>(a.out_col, idx, p.col.r, p.col.g, p.col.b, tab + 256);
        store_rgb<FMT>(a.out_blackout, idx, p.bo.r, p.bo.g, p.bo.b, tab + 256);
    } else {
        const Acc p = shade_pixel<K, false>(l, x, y);
        store_rgb<FMT>(a.out_col, idx, p.col.r, p.col.g, p.col.b, tab + 256);
    }
}

template <uint32_t FMT, int K>
__global__ void __launch_bounds__(64 * ROWS) lens_shade_kernel(LensShadeArgs a) {
    shade_body<FMT, K>(a, [] {}, [&](const float* tab) { return PlainLens{a.lens, a.width, {a.sky, a.sky_w, a.sky_h}, tab}; });
}
template <uint32_t FMT, int K>
__global__ void __launch_bounds__(64 * ROWS) lens_shade_mip_kernel(LensMipArgs a) {
    __shared__ uint32_t off[MIP_MAX_LEVELS];
    shade_body<FMT, K>(
        a,
        [&] {
            if (threadIdx.x == 0) {
#pragma unroll
                for (uint32_t l = 0; l < MIP_MAX_LEVELS; ++l) off[l] = a.level_off[l];  // constant indices: scalar loads
            }
        },
        [&](const float* tab) {
            return MipLens{a.lens, a.width, a.height, {{a.sky, a.sky_w, a.sky_h}, static_cast<const Half4*>(a.chain), off, a.n_levels}, tab};
        });
}

// f(K) with the launch's ss as a compile-time constant, up to the largest K the shade builds
template <int MAX_K, class F>
int with_ss(uint32_t ss, F&& f) {
    switch (ss) {
        case 1u: return f(Const<1u>{});
        case 2u: return f(Const<2u>{});
        case 4u: return f(Const<4u>{});
        case 8u:
            if constexpr (MAX_K >= 8) return f(Const<8u>{});
            [[fallthrough]];
        default: return (int)hipErrorInvalidValue;
    }
}
// kernel(fmt, k): the shade's kernel of that format and K.  width, height <= 65536 (bh_shade_lens,
// bh_shade_lens_mip): at most 1024 x 16384 workgroups
template <int MAX_K, class Args, class Kernel>
int launch(const Args& a, uint32_t ss, uint32_t format, hipStream_t s, Kernel kernel) {
    const dim3 grid((a.width + 63u) / 64u, (a.height + ROWS - 1u) / ROWS), block(64u * ROWS);
    return with_format(format, [&](auto fmt) {
        return with_ss<MAX_K>(ss, [&](auto k) {
            const auto kern = kernel(fmt, k);
            hipLaunchKernelGGL(kern, grid, block, 0, s, a);
            return (int)hipGetLastError();
        });
    });
}

}  // namespace lens
}  // namespace bh

extern "C" __attribute__((visibility("hidden"))) int bh_launch_lens_shade(const bh::LensShadeArgs& a, uint32_t ss,
                                                                        uint32_t format, hipStream_t s) {
    return bh::lens::launch<8>(a, ss, format, s, [](auto fmt, auto k) {
        return bh::lens::lens_shade_kernel<decltype(fmt)::value, (int)decltype(k)::value>;
    });
}
extern "C" __attribute__((visibility("hidden"))) int bh_launch_lens_shade_mip(const bh::LensMipArgs& a, uint32_t ss,
                                                                            uint32_t format, hipStream_t s) {
    return bh::lens::launch<4>(a, ss, format, s, [](auto fmt, auto k) {
        return bh::lens::lens_shade_mip_kernel<decltype(fmt)::value, (int)decltype(k)::value>;
    });
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
        const dim3 grid((w + 63u) / 64u, (h + ROWS - 1u) / ROWS), block(64u * ROWS);
        if (l == 1u)
            hipLaunchKernelGGL(mip_level1_kernel, grid, block, 0, s, sky, w0, h0, srgb_lut, base + off[1], w, h);
        else
            hipLaunchKernelGGL(mip_level_kernel, grid, block, 0, s, base + off[l - 1u], sw, sh, base + off[l], w, h);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}
