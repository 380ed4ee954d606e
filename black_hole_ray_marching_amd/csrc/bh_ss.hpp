// bh_ss.hpp — lane logic of the supersampled render (bh_render_ss): k x k rays per output pixel, k in
// {2, 4, 8}, resolved inside the wave that marched them.  Host and device share every function here: the
// march kernel's epilogue (bh_march_resolve.hpp, ss_resolve_store) runs them per lane, bh_ss_resolve_host
// (bh_mirror.cpp) runs the very same functions over a 64-entry array per wave.
//
// A wave64 owns one 8x8 tile of the VIRTUAL frame (kW x kH), lane = (y & 7) * 8 + (x & 7).  k divides 8,
// so the tile holds (8 / k)^2 whole groups of k x k lanes, one group per output pixel, and the sides of
// the virtual frame are multiples of k, so the frame's edge never cuts a group:
//
//     a group's k^2 lanes are either all valid (inside the virtual frame) or all invalid.
//
// Nothing else is relied on.  Invalid lanes hold 0 and their groups store nothing.
//
// Resolve of one channel, fp32, no FMA (normative, include/bh_render.h): a pairwise tree along x (level 1
// adds neighbours i and i^1, level 2 the pair sums i and i^2, level 3 -- k = 8 -- i and i^4), the same
// tree along y over the row results, then one multiply by 1 / k^2 (a power of two: exact).  fp32 add is
// commutative bit for bit (no NaN among the samples), so the xor butterfly `v += lane[l ^ m]` over the
// masks 1, 2, 4 (x) then 8, 16, 32 (y), up to k, leaves exactly that tree's sum in every lane of a group.
#pragma once
#include <stdint.h>

#ifndef BH_SS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BH_SS_HD __host__ __device__ inline
#else
#define BH_SS_HD inline
#endif
#endif

namespace bh {
namespace ss {

// log2 k for k in {1, 2, 4, 8}; 0xFFFFFFFF for anything else
BH_SS_HD uint32_t log2_k(uint32_t k) { return k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : k == 8u ? 3u : 0xFFFFFFFFu; }

// The butterfly's levels: 2 * lk of them, level i reads lane l ^ level_mask(i, lk).
BH_SS_HD uint32_t levels(uint32_t lk) { return 2u * lk; }
BH_SS_HD uint32_t level_mask(uint32_t i, uint32_t lk) { return i < lk ? (1u << i) : (8u << (i - lk)); }

// One level for one lane: `other(m)` returns this level's input value of lane l ^ m (every lane of the
// wave takes the level together).  A separate statement per add: nothing here can contract.
template <class Other>
BH_SS_HD float level_add(float v, uint32_t m, Other&& other) {
    const float o = other(m);
    return v + o;
}
// 1 / k^2
BH_SS_HD float scale(uint32_t lk) { return lk == 0u ? 1.0f : lk == 1u ? 0.25f : lk == 2u ? 0.0625f : 0.015625f; }

// The lane that stores its group's pixel: the group's top-left one.
BH_SS_HD bool writer(uint32_t lane, uint32_t lk) {
    const uint32_t m = (1u << lk) - 1u;
    return ((lane & 7u) & m) == 0u && ((lane >> 3) & m) == 0u;
}
// Row-major index of the output pixel of virtual pixel (px, py); out_w = the OUTPUT frame's width.
// 32 bits: k * out_w and k * out_h are at most 65536, so the index is below 2^32 / k^2.
BH_SS_HD uint32_t out_index(uint32_t px, uint32_t py, uint32_t lk, uint32_t out_w) {
    return (py >> lk) * out_w + (px >> lk);
}

}  // namespace ss
}  // namespace bh
