// bh_march_resolve.hpp -- the supersampled render's resolve, in the wave: a ray's two samples (ss_samples; the
// fast build stages them through the wave's LDS area, ss_stage_sample), the butterfly over the k x k group
// (ss_lane_xor, ss_level, ss_resolve) and the group's store (ss_resolve_store); and the shutter render's resolve
// across the waves of a workgroup (shutter_stage, shutter_resolve_store).  Needs bh_march_shade.hpp,
// bh_march_ray.hpp (the LDS area), bh_ss.hpp and bh_shutter.hpp (the level sequence and the time tree, shared with
// the host).
#pragma once
#include "bh_march_ray.hpp"
#include "bh_march_shade.hpp"
#include "bh_shutter.hpp"
#include "bh_ss.hpp"

namespace bh {
namespace BH_NS {

// ---- supersampled render (bh_render_ss): the resolve of k x k rays per output pixel, in the wave -------
// The wave's tile is an 8x8 block of the VIRTUAL frame (MarchArgs' geometry fields); lane l holds the
// linear fp32 samples of its ray, 0 where the lane is outside the virtual frame.  Run by all 64 lanes
// (outside any `if (valid)`): the butterfly reads other lanes' registers.  k divides 8 and the virtual
// frame's sides are multiples of k, so a pixel's k^2 lanes are either all valid or all invalid (bh_ss.hpp):
// a valid writer lane's sum holds valid samples only.  The blackout test runs per sample, before the resolve,
// as fs_main runs it per fragment (:365-369).
#if BH_FAST
// The fast build takes its samples where the plain kernel stores them: a valid lane hands its colour to
// write_pixel -- the plain kernel's own output code, blackout test included -- which stores the ray's two
// RGBA32F texels into the wave's two 8x8 sample tiles in LDS (the cycle history's area, free once the march
// has ended) as it would into a kW x kH frame, through pointers made opaque first; then every lane reads its
// samples back.  This build contracts, and which product of a sum it fuses follows how the compiler pairs the
// channels up on their way into those stores (fma(a, b, RN(c d)) or fma(c, d, RN(a b)): the last bit
// differs); behind opaque pointers the shading and the stores are the plain RGBA32F kernel's code,
// instruction for instruction, and so are the bits (tests/test_gpu_ss.py::test_fast_math_by_composition;
// handing the lane's `col` straight to the resolve fused two of the bilinear sums the other way round).  A
// sample read back from LDS is opaque too: no multiply can fuse into the resolve's first add, which would
// also round a lane's copy unlike its partner's.  (The exact build contracts nothing and takes `col` as it
// is: the detour's flat stores and their wait measured 0.6 % of a frame there)
constexpr uint32_t SS_TILES_AT = 64u;  // float4 offset of the tiles in the area
constexpr uint32_t SS_BO_TILE = 64u;   // float4 offset of the blackout samples' tile from the colour samples'
static_assert((SS_TILES_AT + 2u * 64u) * sizeof(float4) <= sizeof(HistLds), "the two sample tiles fit the history area");
__device__ __forceinline__ void ss_stage_sample(const MarchArgs& a, const float* tab, float4* tiles, uint32_t lane,
                                                v3 col, uint32_t n_rk, uint32_t fate, uint32_t steps) {
    MarchArgs t = a;  // row-major, no dbg_* outputs (bh_render_ss): the tile's texel index is the lane
    void* pc = tiles;
    void* pb = tiles + SS_BO_TILE;
    asm volatile("" : "+v"(pc), "+v"(pb));
    t.out_col = pc;
    t.out_blackout = pb;
    write_pixel<BH_OUT_RGBA32F>(t, tab, lane, col, n_rk, fate, steps);
}
#endif
// The two samples of this lane's ray (0 for a lane outside the virtual frame); every lane of the wave.
// SHUT: a wave of the shutter kernel (its LDS area: wave_hist).
template <bool SHUT = false>
__device__ __forceinline__ void ss_samples(const MarchArgs& a, const float* lut, uint32_t lane, bool valid, uint32_t fate,
                                           const RayState& st, uint32_t steps, v3& sc, v3& sb) {
#if BH_FAST
    float4* tiles = reinterpret_cast<float4*>(&wave_hist<SHUT>()) + SS_TILES_AT;
    if (valid) {
        ss_stage_sample(a, lut, tiles, lane, shade(a, lut, fate, st.rd), st.n_rk, fate, steps);
    } else {
        tiles[lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        tiles[SS_BO_TILE + lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    // the staging stores went through generic pointers: workgroup scope makes the wave wait for them before
    // it reads the tiles (a wave-scope fence orders nothing between the flat and the LDS path)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const float4 c = tiles[lane], b = tiles[SS_BO_TILE + lane];
    sc = mk(c.x, c.y, c.z);
    sb = mk(b.x, b.y, b.z);
#else
    v3 col = mk(0.0f, 0.0f, 0.0f);
    if (valid) col = shade(a, lut, fate, st.rd);
    const bool zero = dot(col, col) < 1.0f;  // write_pixel's test
    sc = col;
    sb = zero ? mk(0.0f, 0.0f, 0.0f) : col;
#endif
}
// Lane l reads lane l ^ M's v, every lane of the wave active.  M = 1, 2: a quad permute, M = 8: a rotate by 8
// within the 16-lane row (both DPP: a VALU operand modifier, no LDS trip; no source lane is ever out of range, and
// bound_ctrl spares the destination's initialisation); M = 4, 16: ds_swizzle's bit-mask
// mode (xor within 32 lanes, no address register); M = 32: ds_bpermute.  (__shfl_xor for all of them cost 8
// VALU of index arithmetic and one LDS round trip per value and level: 3.7 % of a frame at k = 2, 6.4 % at
// k = 4)
template <uint32_t M>
__device__ __forceinline__ float ss_lane_xor(float v, uint32_t lane) {
    const int x = (int)__float_as_uint(v);
    int r;
    if constexpr (M == 1u) r = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, true);        // quad_perm:[1,0,3,2]
    else if constexpr (M == 2u) r = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, true);   // quad_perm:[2,3,0,1]
    else if constexpr (M == 8u) r = __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, true);  // row_ror:8
    else if constexpr (M == 4u || M == 16u) r = __builtin_amdgcn_ds_swizzle(x, (int)(0x1Fu | (M << 10)));
    else {
        static_assert(M == 32u, "a butterfly mask of the 8x8 tile");
        r = __builtin_amdgcn_ds_bpermute((int)((lane ^ 32u) << 2), x);
    }
    return __uint_as_float((uint32_t)r);
}
// One butterfly level for the N values of a lane: the N reads first, then the N adds (one wait for all).
template <uint32_t M, int N>
__device__ __forceinline__ void ss_level(float (&v)[N], uint32_t lane) {
#pragma clang fp contract(off)
    float o[N];
#pragma unroll
    for (int c = 0; c < N; ++c) o[c] = ss_lane_xor<M>(v[c], lane);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = ss::level_add(v[c], M, [&](uint32_t) { return o[c]; });
}
// The resolve of N channels at once: bh_ss.hpp's level sequence (a wave-uniform mask per level), then the scale.
template <int N>
__device__ __forceinline__ void ss_resolve(float (&v)[N], uint32_t lk, uint32_t lane) {
#pragma clang fp contract(off)
    for (uint32_t i = 0; i < ss::levels(lk); ++i) {
        switch (ss::level_mask(i, lk)) {
            case 1u: ss_level<1u>(v, lane); break;
            case 2u: ss_level<2u>(v, lane); break;
            case 4u: ss_level<4u>(v, lane); break;
            case 8u: ss_level<8u>(v, lane); break;
            case 16u: ss_level<16u>(v, lane); break;
            default: ss_level<32u>(v, lane); break;
        }
    }
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = v[c] * ss::scale(lk);
}
// Resolve the lane's two samples with its group and store the group's pixel; every lane of the wave.
template <uint32_t FMT>
__device__ __forceinline__ void ss_resolve_store(const MarchArgs& a, const float* tab, uint32_t lane, uint32_t px,
                                                 uint32_t py, bool valid, v3 sc, v3 sb) {
    const uint32_t lk = a.ss_log2;  // 1..3 (bh_render_ss), wave-uniform
    const bool w = valid && ss::writer(lane, lk);
    const size_t idx = ss::out_index(px, py, lk, a.ss_out_width);
    if (a.out_blackout) {  // wave-uniform: the second target is neither resolved nor written without it
        float v[6] = {sc.x, sc.y, sc.z, sb.x, sb.y, sb.z};
        ss_resolve(v, lk, lane);
        if (w) {
            store_px<FMT>(a.out_col, idx, mk(v[0], v[1], v[2]), tab + 256);
            store_px<FMT>(a.out_blackout, idx, mk(v[3], v[4], v[5]), tab + 256);
        }
    } else {
        float v[3] = {sc.x, sc.y, sc.z};
        ss_resolve(v, lk, lane);
        if (w) store_px<FMT>(a.out_col, idx, mk(v[0], v[1], v[2]), tab + 256);
    }
}

// ---- shutter render (bh_render_shutter): the resolve of n cameras per output frame, in the workgroup ----
// Wave w of a workgroup marched the tile with camera w (bh_shutter.hpp).  Once its march has ended it leaves
// its lanes' six sample channels in its OWN history area -- a plane of 64 floats per channel, beside the fast
// build's sample tiles, which ss_samples has read by then -- and after the workgroup's barrier the writer lanes
// of one wave per target read the n waves' planes in bh_shutter.hpp's tree order.
// float offset of channel plane c (0..2 col, 3..5 blackout_col) in a wave's area
__host__ __device__ constexpr uint32_t shutter_plane_at(uint32_t c) { return c < 4u ? c * 64u : 768u + (c - 4u) * 64u; }
static_assert(shutter_plane_at(5u) + 64u <= sizeof(HistLds) / sizeof(float), "the sample planes fit the history area");
#if BH_FAST
static_assert(shutter_plane_at(3u) + 64u <= SS_TILES_AT * 4u && shutter_plane_at(4u) >= (SS_TILES_AT + 2u * 64u) * 4u,
              "the sample planes lie beside the fast build's sample tiles");
#endif
// This lane's samples (ss > 1: its k x k group's resolved pixel, in every lane of the group) into the wave's
// planes; every lane of the wave, invalid lanes hold 0.
__device__ __forceinline__ void shutter_stage(const MarchArgs& a, const float* lut, uint32_t lane, bool valid,
                                              uint32_t fate, const RayState& st, uint32_t steps) {
    v3 sc, sb;
    ss_samples<true>(a, lut, lane, valid, fate, st, steps, sc, sb);
    float v[6] = {sc.x, sc.y, sc.z, sb.x, sb.y, sb.z};
    if (a.ss_log2 != 0u) ss_resolve(v, a.ss_log2, lane);  // wave-uniform
    float* P = reinterpret_cast<float*>(&wave_hist<true>());
#pragma unroll
    for (uint32_t c = 0; c < 6u; ++c) P[shutter_plane_at(c) + lane] = v[c];
}
// A writer lane, after the barrier: target 0 (col) or 1 (blackout_col; wave-uniform) of its pixel from the
// n = 2^ln waves' planes -- tree, scale, encode, store.
template <uint32_t FMT>
__device__ __forceinline__ void shutter_resolve_store(void* out, uint32_t target, uint32_t ln, uint32_t lane,
                                                      size_t idx, const float* tab) {
#pragma clang fp contract(off)
    const float* base = reinterpret_cast<const float*>(shutter_hist_lds());
    float v[3];
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
        const uint32_t off = shutter_plane_at(3u * target + c) + lane;
        const float s = shutter::tree_sum(ln, [&](uint32_t t) { return base[t * (uint32_t)(sizeof(HistLds) / sizeof(float)) + off]; });
        v[c] = s * shutter::scale(ln);
    }
    store_px<FMT>(out, idx, mk(v[0], v[1], v[2]), tab + 256);
}

}  // namespace BH_NS
}  // namespace bh
