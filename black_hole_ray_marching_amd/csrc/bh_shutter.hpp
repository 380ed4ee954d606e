// bh_shutter.hpp — index logic of the shutter render (bh_render_shutter): every output frame averages the
// frames of its n sub-frame cameras, n in {2, 4, 8, 16}, resolved inside the workgroup that marched them.  Host
// and device share every function here: the shutter kernel (bh_march_tile.hpp, march_tile_shutter_kernel) runs
// them per workgroup, wave and writer lane, bh_shutter_resolve_host (bh_mirror.cpp) runs the very same functions
// workgroup by workgroup over sample frames.
//
// One workgroup of n waves owns one 8x8 tile (of the virtual frame when ss > 1) of ONE output frame; wave w
// marches that tile with the frame's camera w and leaves its lanes' samples where the others can read them.
// A writer lane then sums the n samples of its pixel in the order below.
//
// Resolve of one channel, fp32, no FMA (normative, include/bh_render.h): a pairwise tree over the time samples
// (level 1 adds t and t^1, level 2 the pair sums t and t^2, ...), then one multiply by 1 / n (a power of two:
// exact).  tree_sum walks that tree depth first: sum(t0, N) = sum(t0, N/2) + sum(t0 + N/2, N/2), the lower
// half on the left; fp32 add is commutative bit for bit (no NaN among the samples).
#pragma once
#include <stdint.h>

#ifndef BH_SHUTTER_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BH_SHUTTER_HD __host__ __device__ inline
#else
#define BH_SHUTTER_HD inline
#endif
#endif

namespace bh {
namespace shutter {

constexpr uint32_t MAX_LOG2 = 4u;  // n <= 16: the waves of one workgroup

// log2 n for n in {1, 2, 4, 8, 16}; 0xFFFFFFFF for anything else
BH_SHUTTER_HD uint32_t log2_n(uint32_t n) {
    return n == 1u ? 0u : n == 2u ? 1u : n == 4u ? 2u : n == 8u ? 3u : n == 16u ? 4u : 0xFFFFFFFFu;
}
// 1 / n
BH_SHUTTER_HD float scale(uint32_t ln) {
    return ln == 0u ? 1.0f : ln == 1u ? 0.5f : ln == 2u ? 0.25f : ln == 3u ? 0.125f : 0.0625f;
}

// Workgroup g of a launch of n_frames output frames: the existing frame interleave (bh_march_tile.hpp), one
// level up -- order index g / n_frames of frame g % n_frames.
BH_SHUTTER_HD uint32_t group_order(uint32_t g, uint32_t n_frames) { return g / n_frames; }
BH_SHUTTER_HD uint32_t group_frame(uint32_t g, uint32_t n_frames) { return g - (g / n_frames) * n_frames; }
// Wave w of a workgroup of frame f marches with camera f * n + w of the call's camera array.
BH_SHUTTER_HD uint32_t wave_camera(uint32_t f, uint32_t w, uint32_t ln) { return (f << ln) + w; }
// The dispatch slot of march_slot's own interleave (slot s = order index s / n_cameras, camera s % n_cameras)
// that this wave takes.
BH_SHUTTER_HD uint32_t wave_slot(uint32_t g, uint32_t w, uint32_t n_frames, uint32_t ln) {
    return group_order(g, n_frames) * (n_frames << ln) + wave_camera(group_frame(g, n_frames), w, ln);
}

// The tree over samples t0 .. t0 + N - 1; `sample(t)` returns time sample t.  A separate statement per add:
// nothing here can contract.
template <uint32_t N, class Sample>
BH_SHUTTER_HD float tree(uint32_t t0, Sample&& sample) {
    if constexpr (N == 1u) {
        return sample(t0);
    } else {
        const float lo = tree<N / 2u>(t0, sample);
        const float hi = tree<N / 2u>(t0 + N / 2u, sample);
        const float s = lo + hi;
        return s;
    }
}
// ... for n = 2^ln samples (ln <= MAX_LOG2)
template <class Sample>
BH_SHUTTER_HD float tree_sum(uint32_t ln, Sample&& sample) {
    switch (ln) {
        case 0u: return tree<1u>(0u, sample);
        case 1u: return tree<2u>(0u, sample);
        case 2u: return tree<4u>(0u, sample);
        case 3u: return tree<8u>(0u, sample);
        default: return tree<16u>(0u, sample);
    }
}

}  // namespace shutter
}  // namespace bh
