// bh_disc.hip — bh_shade_lens_disc: a lens map, its hit map, a sky and a disc texture -> the frame's targets
// (include/bh_render.h, "Disc shades").  Built as bh_lens.hip is: -ffp-contract=off with correctly rounded fp32
// division and square root; the arithmetic is bh_lens.hpp's, shared with the host.
//
// bh_lens.hip's mapping: one thread per OUTPUT pixel, a wave on 64 consecutive pixels of one row, a thread loops over
// its ss x ss records.  A record that is no surface record costs what it costs the plain shade; a surface record of a
// scene with the disc reads its 12 bytes of the hit map and gathers four disc texels in place of the sky's, after the
// f64 angle of the hit (crm::atan2_core).  The kernel's one barrier is the table load's, before any thread leaves.
// A unit of its own: the plain and filtered shades' kernels keep the machine code they were measured with.
#include <hip/hip_runtime.h>

#include "bh_common.hpp"
#include "bh_lens.hpp"
#include "bh_srgb.hpp"

namespace bh {
namespace lens {

constexpr uint32_t DISC_ROWS = 4;  // rows of 64 pixels per 256-thread workgroup
static_assert(64 * DISC_ROWS == 256, "the table load is one entry per thread");

template <uint32_t FMT, int K>
__global__ void __launch_bounds__(64 * DISC_ROWS) lens_shade_disc_kernel(LensDiscArgs a) {
    // [0, 256) the sRGB decode of sky and disc texels, then for BGRA8 output the encoder's 257 thresholds
    __shared__ float tab[lds_tables<FMT>()];
    load_srgb_tables<FMT, 64u * DISC_ROWS, true>(a, tab);
    __syncthreads();  // reached by every thread of the workgroup: the bounds test comes after it
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * DISC_ROWS + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;  // a partial last column or row: no load, no store
    const DiscLens l{a.lens, a.hits, a.width, {a.sky, a.sky_w, a.sky_h},
                     {a.disc, a.n_phi, a.n_r, a.rs, a.scene_flags, a.spin, a.gain}, tab};
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
int launch_disc(const LensDiscArgs& a, hipStream_t s) {
    // width, height <= 65536 (bh_shade_lens_disc): at most 1024 x 16384 workgroups
    const dim3 grid((a.width + 63u) / 64u, (a.height + DISC_ROWS - 1u) / DISC_ROWS), block(64u * DISC_ROWS);
    hipLaunchKernelGGL((lens_shade_disc_kernel<FMT, K>), grid, block, 0, s, a);
    return (int)hipGetLastError();
}

// bh_shade_lens_disc_beamed ("Beamed disc shades"): the kernel above over BeamLens -- a surface record of a scene
// with the disc reads its 12 bytes of the arrival map with its hit's, and a disc hit's colour takes the factor of
// bh_lens.hpp's beam_factor (two divisions and four square roots more than the disc shade's, all fp32).  A kernel of its
// own beside the disc shade's, which keeps its machine code.
template <uint32_t FMT, int K>
__global__ void __launch_bounds__(64 * DISC_ROWS) lens_shade_disc_beamed_kernel(LensBeamArgs a) {
    __shared__ float tab[lds_tables<FMT>()];
    load_srgb_tables<FMT, 64u * DISC_ROWS, true>(a, tab);
    __syncthreads();  // reached by every thread of the workgroup: the bounds test comes after it
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * DISC_ROWS + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;  // a partial last column or row: no load, no store
    const BeamLens l{a.lens, a.hits, a.arrivals, a.width, {a.sky, a.sky_w, a.sky_h},
                     {a.disc, a.n_phi, a.n_r, a.rs, a.scene_flags, a.spin, a.gain}, {a.beam, a.sense, a.dp}, tab};
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
int launch_disc_beamed(const LensBeamArgs& a, hipStream_t s) {
    const dim3 grid((a.width + 63u) / 64u, (a.height + DISC_ROWS - 1u) / DISC_ROWS), block(64u * DISC_ROWS);
    hipLaunchKernelGGL((lens_shade_disc_beamed_kernel<FMT, K>), grid, block, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace lens
}  // namespace bh

extern "C" __attribute__((visibility("hidden"))) int bh_launch_lens_shade_disc(const bh::LensDiscArgs& a, uint32_t ss,
                                                                             uint32_t format, hipStream_t s) {
    return bh::with_format(format, [&](auto fmt) {
        constexpr uint32_t FMT = decltype(fmt)::value;
        switch (ss) {
            case 1u: return bh::lens::launch_disc<FMT, 1>(a, s);
            case 2u: return bh::lens::launch_disc<FMT, 2>(a, s);
            case 4u: return bh::lens::launch_disc<FMT, 4>(a, s);
            case 8u: return bh::lens::launch_disc<FMT, 8>(a, s);
            default: return (int)hipErrorInvalidValue;
        }
    });
}

extern "C" __attribute__((visibility("hidden"))) int bh_launch_lens_shade_disc_beamed(const bh::LensBeamArgs& a, uint32_t ss,
                                                                                    uint32_t format, hipStream_t s) {
    return bh::with_format(format, [&](auto fmt) {
        constexpr uint32_t FMT = decltype(fmt)::value;
        switch (ss) {
            case 1u: return bh::lens::launch_disc_beamed<FMT, 1>(a, s);
            case 2u: return bh::lens::launch_disc_beamed<FMT, 2>(a, s);
            case 4u: return bh::lens::launch_disc_beamed<FMT, 4>(a, s);
            case 8u: return bh::lens::launch_disc_beamed<FMT, 8>(a, s);
            default: return (int)hipErrorInvalidValue;
        }
    });
}
