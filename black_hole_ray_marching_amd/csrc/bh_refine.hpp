// bh_refine.hpp — lane logic of the adaptive supersampled render (bh_render_adaptive): which 8x8 OUTPUT
// tiles of a plain frame show an edge, and which tiles of the virtual frame (bh_ss.hpp) re-march them.
// Host and device share every function here: the detect kernel (bh_tiles.hip) and the work-list march
// (bh_march_tile.hpp, march_refine_kernel) run them per lane / per wave, bh_refine_mask_host and
// bh_refine_cover_host (bh_mirror.cpp) run the very same functions lane by lane.
//
// The rule (normative, include/bh_render.h): a pixel is an edge pixel when it differs from one of its
// 4-neighbours inside the frame (x +- 1 or y +- 1; a row's end has no neighbour in the next row) in one of
// the targets; a tile is refined when it holds an edge pixel.  Two texels differ when the largest of their
// three colour channels' |a - b| (alpha is not looked at) exceeds the threshold, strictly.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef BH_RF_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define BH_RF_HD __host__ __device__ __forceinline__
#else
#define BH_RF_HD inline
#endif
#endif

namespace bh {
namespace refine {

// the output formats (BH_OUT_* of include/bh_render.h, which this header does not need otherwise)
constexpr uint32_t FMT_RGBA32F = 0u, FMT_RGBA16F = 1u, FMT_BGRA8 = 2u;

struct Texel { float c[3]; };  // r, g, b as the rule compares them (BGRA8: the bytes, 0..255, exact in fp32)

BH_RF_HD float bits_f32(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// binary16 -> binary32, exact (subnormals, infinities and NaNs included)
BH_RF_HD float half_f32(uint32_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);  // v_cvt_f32_f16: the same exact conversion
#else
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 31u) return bits_f32(s | 0x7F800000u | (m << 13));
    if (e != 0u) return bits_f32(s | ((e + 112u) << 23) | (m << 13));
    const float v = (float)m * 0x1p-24f;  // m * 2^-24: exact
    return s ? -v : v;
#endif
}

// The texel value of pixel idx of a row-major target in format fmt.
BH_RF_HD Texel texel(uint32_t fmt, const void* img, size_t idx) {
    Texel t;
    if (fmt == FMT_RGBA32F) {
        struct alignas(16) W4 { float x, y, z, w; };
        const W4 v = static_cast<const W4*>(img)[idx];
        t.c[0] = v.x; t.c[1] = v.y; t.c[2] = v.z;
    } else if (fmt == FMT_RGBA16F) {
        struct alignas(8) W2 { uint32_t x, y; };
        const W2 v = static_cast<const W2*>(img)[idx];
        t.c[0] = half_f32(v.x & 0xFFFFu); t.c[1] = half_f32(v.x >> 16); t.c[2] = half_f32(v.y & 0xFFFFu);
    } else {  // b | g << 8 | r << 16 | a << 24
        const uint32_t v = static_cast<const uint32_t*>(img)[idx];
        t.c[0] = (float)((v >> 16) & 0xFFu); t.c[1] = (float)((v >> 8) & 0xFFu); t.c[2] = (float)(v & 0xFFu);
    }
    return t;
}

// What the distance is compared against: T in the float formats, T * 255 (one fp32 multiply) for the bytes.
BH_RF_HD float threshold(uint32_t fmt, float T) {
    return fmt != FMT_BGRA8 ? T : T * 255.0f;  // compared, never added to: nothing can contract into it
}

// d = max over the channels of |a_c - b_c| (one fp32 subtract each; a NaN difference is no maximum), d > thr.
BH_RF_HD bool differ(const Texel& a, const Texel& b, float thr) {
    float d = 0.0f;
    for (int ch = 0; ch < 3; ++ch) {
        float v = a.c[ch] - b.c[ch];
        v = v < 0.0f ? -v : v;
        d = v > d ? v : d;
    }
    return d > thr;
}

// Tile and lane index arithmetic: lane l of tile (tx, ty) is pixel (8 tx + (l & 7), 8 ty + (l >> 3)).
BH_RF_HD uint32_t tiles_of(uint32_t n) { return (n + 7u) / 8u; }
BH_RF_HD uint32_t lane_x(uint32_t tx, uint32_t lane) { return tx * 8u + (lane & 7u); }
BH_RF_HD uint32_t lane_y(uint32_t ty, uint32_t lane) { return ty * 8u + (lane >> 3); }

// Pixel (x, y) of one w x h target differs from a 4-neighbour inside the frame; false outside the frame.
// w * h is below 2^32 (w, h <= 32768).
BH_RF_HD bool edge_pixel(uint32_t fmt, const void* img, uint32_t w, uint32_t h, uint32_t x, uint32_t y, float thr) {
    if (x >= w || y >= h) return false;
    const size_t i = (size_t)y * w + x;
    const Texel own = texel(fmt, img, i);
    bool e = false;
    if (x > 0u) e |= differ(own, texel(fmt, img, i - 1u), thr);
    if (x + 1u < w) e |= differ(own, texel(fmt, img, i + 1u), thr);
    if (y > 0u) e |= differ(own, texel(fmt, img, i - w), thr);
    if (y + 1u < h) e |= differ(own, texel(fmt, img, i + w), thr);
    return e;
}
// One lane's decision for its pixel of tile (tx, ty): an edge in `col`, or in `blackout` when there is one.
BH_RF_HD bool lane_edge(uint32_t fmt, const void* col, const void* blackout, uint32_t w, uint32_t h, uint32_t tx,
                        uint32_t ty, uint32_t lane, float thr) {
    const uint32_t x = lane_x(tx, lane), y = lane_y(ty, lane);
    bool e = edge_pixel(fmt, col, w, h, x, y, thr);
    if (blackout) e |= edge_pixel(fmt, blackout, w, h, x, y, thr);
    return e;
}

// ---- the work list -------------------------------------------------------------------------------------
// Entry e of the list is a refined tile: two words, the frame and the output tile ty * tiles_x + tx.  Work
// item `item` is (entry item >> 2 lk, sub-tile item & (k^2 - 1)); sub-tile s = i + k j marches virtual tile
// (k tx + i, k ty + j): the k x k virtual tiles that hold the output tile's 64 k^2 samples.
constexpr uint32_t ENTRY_WORDS = 2u;
// The list is filled from both ends: tiles whose plain march was long (the pass-1 cost of the tile, the
// dispatch order's own measure: min(255, longest ray's steps / 2)) from the front, the others from the back,
// so that the items of the long chains are pulled first and the launch does not end on them.  Only the order
// of the work depends on it, never a byte of output.  Entry e of n_front + n_back lives in slot:
constexpr uint32_t COST_FIRST = 64u;
BH_RF_HD uint32_t entry_slot(uint32_t e, uint32_t n_front, uint32_t capacity) {
    return e < n_front ? e : capacity - 1u - (e - n_front);
}
BH_RF_HD uint32_t item_entry(uint32_t item, uint32_t lk) { return item >> (2u * lk); }
BH_RF_HD uint32_t item_sub(uint32_t item, uint32_t lk) { return item & ((1u << (2u * lk)) - 1u); }
// The virtual tile of (output tile, sub-tile), false when the tile is no tile of the output grid or the
// virtual tile lies outside the virtual frame's grid vtiles_x x vtiles_y (a partial last tile column or row:
// nothing to march).
BH_RF_HD bool item_tile(uint32_t tile, uint32_t sub, uint32_t lk, uint32_t tiles_x, uint32_t tiles_y, uint32_t vtiles_x,
                        uint32_t vtiles_y, uint32_t* vtx, uint32_t* vty) {
    if (tile >= tiles_x * tiles_y) return false;
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t i = sub & ((1u << lk) - 1u), j = sub >> lk;
    *vtx = (tx << lk) + i;
    *vty = (ty << lk) + j;
    return *vtx < vtiles_x && *vty < vtiles_y;
}

}  // namespace refine
}  // namespace bh
