// bh_common.hpp — host/device shared definitions for the geodesic ray-marcher (no math here).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/bh_render.h"

namespace bh {

// A launch's run-time word as a compile-time constant: what every launcher's ladder hands to its kernel choice.
template <uint32_t V>
struct Const { static constexpr uint32_t value = V; };
// f(FMT) with the launch's output format (validated by the entry points) as a compile-time constant
template <class F>
__attribute__((visibility("hidden"))) inline int with_format(uint32_t format, F&& f) {
    switch (format) {
        case BH_OUT_RGBA32F: return f(Const<BH_OUT_RGBA32F>{});
        case BH_OUT_RGBA16F: return f(Const<BH_OUT_RGBA16F>{});
        default: return f(Const<BH_OUT_BGRA8_SRGB>{});
    }
}

// Frames whose arguments travel inline in the kernel argument; a bh_render_frames call of more
// (up to BH_MAX_FRAMES) stages them in a device table (bh_host.hpp, FrameTable).
constexpr uint32_t BH_INLINE_FRAMES = 32;
static_assert(BH_INLINE_FRAMES <= BH_MAX_FRAMES, "inline frames");

// The per-frame part of a launch that renders several frames (bh_render_frames): camera, the
// photon-sphere centre derived from its position, and the frame's outputs.
struct FrameArgs {
    float pos[3];
    float c0[3], c1[3], c2[3];
    float cps[3];
    void* out_col;
    void* out_blackout;
    uint16_t* dbg_n_rk;
    uint8_t* dbg_fate;
    uint16_t* dbg_steps;
};

// A frame's first-step record (bh_host.cpp, first_step_record): what iteration 0 of the march computes from
// ro = camera.pos alone, the same number in every lane of the frame -- dt0 = the step's dt, Q0 = (r^2 r^2) r and
// rq0 = RN(1 / Q0) of k1's rd_derivative -- formed once on the host in IEEE f32.  Q0 == 0 marks a frame whose
// record is not valid: its waves run iteration 0 themselves.
struct FirstStep { float dt0, Q0, rq0; };

// Everything one launch needs, passed by value as the kernel argument (lives in SGPRs / kernarg).
// The per-frame fields (pos, c0..c2, cps, outputs) are frame 0's; a multi-frame launch (n_frames > 1,
// tile schedule) also carries every frame's in `frames` and each wave selects its own.
struct MarchArgs {
    // camera uniform (src/black_hole_maybe.wgsl:9-17): ro0 and the three interpolated corner rays
    float pos[3];
    float c0[3], c1[3], c2[3];
    // Uniforms (src/black_hole_maybe.wgsl:58-69)
    float rs, dtm, max_dist, dp;
    uint32_t blackout_eh;
    uint32_t skip_sdf;         // the root-free step may run (bh_march_step.hpp, sdf_skip_slack: dtm > 0, 0 < rs <= 8)
    float far_r2;              // r^2 beyond which a step needs no SDF argument (bh_host.cpp sdf_far_r2; +inf: off)
    // unused: the per-term radii of a root-free-step variant measured slower and removed;
    // kept so that the kernel argument layout -- and the kernels' machine code -- stay those measured
    // The supersampled render (bh_render_ss, ss = k > 1; bh_ss.hpp) uses two of those words: log2 k and the
    // OUTPUT frame's width.  The geometry fields below then describe the virtual frame (kW x kH).  Both
    // are 0 for every other launch, whose kernels never read them.
    uint32_t ss_log2;
    uint32_t ss_out_width;
    // The third: != 0 for bh_render_lens, whose kernels store a lens record per ray into out_col (row-major)
    // instead of shading it.  Read by the launchers only, never by a kernel.
    uint32_t lens;
    // frame
    uint32_t width, height, max_iters, scene_flags;
    uint32_t format, layout;
    uint32_t shard_index, shard_count;
    uint32_t tiles_x, tiles_y;
    uint32_t n_tiles;          // tiles owned by this shard (= grid work items)
    uint32_t order_block;      // centre-out dispatch: shard-local tiles permuted in blocks of this
    uint32_t order_centre;     //   many tiles (~ one tile row), starting at block order_centre
    const uint32_t* order;     // optional dispatch order (slot -> shard-local tile), else centre-out
    const uint32_t* tile_list; // optional (weighted partition): shard-local tile -> tx | ty << 16
    uint8_t* tile_cost;        // optional output: per shard-local tile, min(255, max n_rk / 2)
    uint32_t* order_tot;       // with tile_cost: per-bucket tile counts of those costs (buckets < B-1)
    // per-frame invariants, computed on the host with the same correctly rounded f32 ops as the
    // oracle: photon-sphere centre -normalize(ro0) * 1.5 * RS (:294) and (DP * RS) * -1.5 (:126)
    float cps[3];
    float kfac;
    // RN(1 / (2W)) and RN(1 / (2H)): the reciprocals of vs_main's interpolation denominators (IEEE on the
    // host; equal to crm::rcp_refined of 2W, 2H, which is RN(1/d) for every normal d)
    float rw2, rh2;
    // sky (Rgba8UnormSrgb texels as packed u32, little endian: r | g<<8 | b<<16 | a<<24)
    const uint32_t* sky;
    const float* srgb_lut;     // 256 entries, sRGB byte -> linear
    const float* srgb_enc;     // 257 thresholds of the BGRA8 sRGB encode (bh_srgb.hpp)
    uint32_t sky_w, sky_h;
    // outputs
    void* out_col;
    void* out_blackout;
    uint16_t* dbg_n_rk;
    uint8_t* dbg_fate;
    uint16_t* dbg_steps;
    // frames of one launch (bh_render_frames): wave slot s marches frame s % n_frames, tile s / n_frames;
    // up to BH_INLINE_FRAMES of them inline, more from a device table (frame_table, else null)
    uint32_t n_frames;
    // slot / n_frames as a multiply-high (div_magic below; 0: none, the wave divides).  In what was the padding
    // in front of the pointer; tx_magic, for tile / tiles_x of an unsharded launch, in the padding behind clk_mask
    uint32_t nf_magic;
    const FrameArgs* frame_table;
    // shader-clock probe (bh_set_clock_probe): per-XCD accumulators, sampled slots: (slot + slot / 256) & clk_mask == 0
    unsigned long long* clk;
    uint32_t clk_mask;
    uint32_t tx_magic;
    FrameArgs frames[BH_INLINE_FRAMES];
    // the frames' first-step records, behind everything the kernels were compiled against: read by the exact builds'
    // tile-schedule kernels alone (bh_march_tile.hpp, slot_head).  A launch of more than BH_INLINE_FRAMES frames has
    // them behind its staged table instead, at frame_table + n_frames (MarchArgs has no free pointer word)
    FirstStep first[BH_INLINE_FRAMES];
};
// The multiply-high form of a wave-uniform division by a launch constant: m with (n * m) >> 32 == n / d for every
// n <= n_max, or 0 when no 32-bit m does that.  m = floor(2^32 / d) + 1 overshoots 2^32 / d by e / (d 2^32) with
// e = m d - 2^32 in [1, d], so n m / 2^32 = n / d + n e / (d 2^32): the floor is n / d's as long as the excess stays
// under 1 / d, the least distance from n / d up to the next integer, that is n e < 2^32.  d = 1 has no such m.
inline uint32_t div_magic(uint32_t d, uint32_t n_max) {
    if (d < 2u) return 0u;
    const uint64_t m = (1ull << 32) / d + 1u, e = m * d - (1ull << 32);
    return (uint64_t)n_max * e < (1ull << 32) ? (uint32_t)m : 0u;
}
// passed by value: the kernel argument segment holds at most 4 KiB, with the arguments some kernels take behind
// it -- the persistent kernel's pointer (8 bytes), the ray-map kernels' map (8), the origin-map kernels' two (16), the
// shutter kernels' map and log2 n (16 with padding); the work-list march's RefineArgs, the largest, is asserted below it
static_assert(sizeof(MarchArgs) + 16 <= 4096, "MarchArgs must fit the kernel argument segment");
// the layout the existing kernels were compiled against: the supersampling words took the place of three
// unused ones and moved nothing
static_assert(offsetof(MarchArgs, far_r2) == 72 && offsetof(MarchArgs, ss_log2) == 76 &&
                  offsetof(MarchArgs, ss_out_width) == 80 && offsetof(MarchArgs, lens) == 84 &&
                  offsetof(MarchArgs, width) == 88,
              "MarchArgs: the supersampling words must stay inside the former reserved_[3]");
static_assert(offsetof(MarchArgs, order) == 144 && offsetof(MarchArgs, sky) == 200 && offsetof(MarchArgs, out_col) == 232 &&
                  offsetof(MarchArgs, n_frames) == 272 && offsetof(MarchArgs, frames) == 304 &&
                  sizeof(FrameArgs) == 104 && offsetof(MarchArgs, first) == 304 + BH_INLINE_FRAMES * sizeof(FrameArgs) &&
                  sizeof(FirstStep) == 12 && sizeof(MarchArgs) == 304 + BH_INLINE_FRAMES * (sizeof(FrameArgs) + sizeof(FirstStep)),
              "MarchArgs: kernel argument layout changed");

// What a march launch carries besides MarchArgs, from the entry point (bh_host.cpp, Launch) to the unit's launcher
// (bh_march.hpp, BH_MARCH_UNIT).  Host side only, never a kernel argument: a launcher hands its kernels the fields
// of its family, each as an argument of its own.
struct MarchLaunch {
    const float* dirs = nullptr;   // the ray-map families: the device map the rays' directions come from
    const float* orgs = nullptr;   // ... with an origin map: the rays' origins
    float* hits = nullptr;         // the hit-map family: where surface rays ended
    float* arrivals = nullptr;     // the arrival-map family, beside hits: the direction they ended with
    uint32_t shutter_log2 = 0;     // the shutter forms: log2 of the cameras per output frame (a.n_frames counts cameras)
    // the plain family: a bh_schedule without its flags, and the persistent schedule's work counters and grid
    uint32_t schedule = BH_SCHED_TILE;
    uint32_t* counters = nullptr;
    uint32_t grid = 0;
};

// The adaptive render's device-side work (bh_render_adaptive; bh_refine.hpp), a second kernel argument of
// the two kernels that use it -- MarchArgs stays as the existing kernels were compiled against.  The detect
// kernel (bh_tiles.hip) fills mask, list and counts from the plain frame in the frames' targets; the
// work-list march (bh_march_tile.hpp, march_refine_kernel) consumes the list.
struct RefineArgs {
    uint32_t* list;      // `capacity` entries of refine::ENTRY_WORDS words: frame, output tile
    uint32_t* ctr;       // [0] entries appended at the front, [1] at the back; from word REFINE_HEAD0 on the
                         // work-list march's head words, REFINE_HEAD_STRIDE apart (REFINE_CTR_WORDS words).  The two
                         // entry counts are zeroed on the stream before the detect, the heads by the detect kernel
    const uint8_t* tile_cost;  // optional: pass 1's cost of each output tile (frame 0's), the list's order
    uint8_t* mask;       // n_frames * tiles_x * tiles_y bytes, frame-major: 1 = refined
    uint32_t* refined;   // optional (the caller's): n_frames counts, zeroed on the stream before the detect
    uint32_t width, height;     // the OUTPUT frame (MarchArgs' geometry is the virtual frame's)
    uint32_t tiles_x, tiles_y;  // its 8x8 tile grid
    uint32_t n_frames;
    uint32_t capacity;   // entries the list holds: n_frames * tiles_x * tiles_y at least
    uint32_t n_heads;    // 1..REFINE_HEADS head words in use (bh_march_tile.hpp, march_refine_kernel)
    float thr;           // refine::threshold(format, T)
};
static_assert(sizeof(MarchArgs) + sizeof(RefineArgs) <= 4096, "march_refine_kernel's arguments must fit the kernel argument segment");

// One bh_shade_lens launch (bh_lens.hip): the lens of the virtual frame ss*width x ss*height, the sky to
// sample and the row-major targets of width x height.
struct LensShadeArgs {
    const bh_lens_px* lens;
    const uint32_t* sky;       // Rgba8UnormSrgb texels, as MarchArgs::sky
    const float* srgb_lut;     // 256 entries
    const float* srgb_enc;     // 257 thresholds (BGRA8 output)
    void* out_col;
    void* out_blackout;        // or null
    uint32_t width, height;    // the OUTPUT frame
    uint32_t sky_w, sky_h;
};

// One bh_shade_lens_mip launch (bh_lens.hip): the same and the sky's chain -- the levels >= 1, 8 bytes per
// texel, level l at chain + level_off[l] texels (lens::mip_offsets).
struct LensMipArgs : LensShadeArgs {
    const void* chain;
    uint32_t n_levels;
    uint32_t level_off[16];
};

// One bh_shade_lens_disc launch (bh_disc.hip): the same, the lens's hit map (three floats per record) and the disc
// with its scene and its turn (include/bh_render.h, bh_disc_desc).
struct LensDiscArgs : LensShadeArgs {
    const float* hits;
    const uint32_t* disc;      // n_phi x n_r Rgba8UnormSrgb texels
    uint32_t n_phi, n_r;
    float rs;
    uint32_t scene_flags;
    float spin, gain;
};

// One bh_shade_lens_disc_beamed launch (bh_disc.hip): the same, the lens's arrival map beside its hit map and the
// beam (include/bh_render.h, bh_beam_desc); sense as a float, +1 or -1.
struct LensBeamArgs : LensDiscArgs {
    const float* arrivals;
    float beam, sense, dp;
};

constexpr uint32_t REFINE_HEADS = 8, REFINE_HEAD_STRIDE = 32, REFINE_HEAD0 = 32;  // 128-byte lines
constexpr uint32_t REFINE_CTR_WORDS = REFINE_HEAD0 + REFINE_HEADS * REFINE_HEAD_STRIDE;

// Shard ownership: tile (tx, ty) belongs to shard (tx + 3*ty) % S (SURVEY §8e diagonal interleave).
// Row ty's first owned column for shard k.
__host__ __device__ inline uint32_t shard_row_start(uint32_t ty, uint32_t k, uint32_t S) {
    // (k - 3*ty) mod S, computed without negatives
    uint32_t m = (3u * (ty % S)) % S;
    return (k + S - m) % S;
}
__host__ __device__ inline uint32_t shard_row_count(uint32_t tiles_x, uint32_t ty, uint32_t k, uint32_t S) {
    uint32_t st = shard_row_start(ty, k, S);
    return st < tiles_x ? (tiles_x - st + S - 1u) / S : 0u;
}
// Tiles owned in one full period of rows.  Period P = S / gcd(S, 3).
__host__ __device__ inline uint32_t shard_period(uint32_t S) { return (S % 3u == 0u) ? S / 3u : S; }

__host__ __device__ inline uint64_t shard_tile_count(uint32_t tiles_x, uint32_t tiles_y, uint32_t k, uint32_t S) {
    const uint32_t P = shard_period(S);
    uint64_t per = 0;
    for (uint32_t r = 0; r < P && r < tiles_y; ++r) per += shard_row_count(tiles_x, r, k, S);
    uint64_t full = tiles_y / P, n = full * per;
    for (uint32_t r = 0; r < tiles_y % P; ++r) n += shard_row_count(tiles_x, r, k, S);
    return n;
}

// The rows of one period of shard k, walked without divisions (these run once per wave in the
// march kernel and once per tile in the unpack; the division-per-row form cost ~1000 VALU
// instructions per tile at S = 8).  Row r of a period starts at column st = (k - 3r) mod S and
// owns q0 + (st < r0) tiles, with tiles_x = q0*S + r0.
struct ShardRows {
    uint32_t k, S, q0, r0, m;  // m = 3r mod S of the current row
    __host__ __device__ ShardRows(uint32_t tiles_x, uint32_t k_, uint32_t S_) : k(k_), S(S_), m(0u) {
        q0 = tiles_x / S; r0 = tiles_x - q0 * S;
    }
    __host__ __device__ uint32_t start() const { return k >= m ? k - m : k + S - m; }
    __host__ __device__ uint32_t count() const { return q0 + (start() < r0 ? 1u : 0u); }
    __host__ __device__ void next() { m += 3u; while (m >= S) m -= S; }
};

// Shard-local tile index t -> global tile coordinates.
__host__ __device__ inline void shard_tile_coords(uint32_t t, uint32_t tiles_x, uint32_t k, uint32_t S,
                                                  uint32_t* tx, uint32_t* ty) {
    if (S == 1u) { *ty = t / tiles_x; *tx = t - *ty * tiles_x; return; }
    const uint32_t P = shard_period(S);
    uint32_t per = 0;
    ShardRows R(tiles_x, k, S);
    for (uint32_t r = 0; r < P; ++r, R.next()) per += R.count();
    const uint32_t period = t / per;
    uint32_t rem = t - period * per, row = 0;
    ShardRows Q(tiles_x, k, S);
    for (; row + 1u < P; ++row, Q.next()) {
        const uint32_t c = Q.count();
        if (rem < c) break;
        rem -= c;
    }
    *ty = period * P + row;
    *tx = Q.start() + rem * S;
}

// Inverse of shard_tile_coords: global tile (tx, ty) -> its shard and its shard-local index.
__host__ __device__ inline uint32_t shard_tile_index(uint32_t tx, uint32_t ty, uint32_t tiles_x, uint32_t S,
                                                     uint32_t* shard) {
    const uint32_t k = (tx + 3u * (ty % S)) % S;
    *shard = k;
    if (S == 1u) return ty * tiles_x + tx;
    const uint32_t P = shard_period(S);
    const uint32_t rp = ty % P;
    uint32_t per = 0, pre = 0;
    ShardRows R(tiles_x, k, S);
    for (uint32_t r = 0; r < P; ++r, R.next()) {
        const uint32_t c = R.count();
        per += c;
        pre += r < rp ? c : 0u;
    }
    return (ty / P) * per + pre + tx / S;  // tx = row start + j*S with the row start < S
}

// Centre-out dispatch order (a bijection of [0, n)): the shard-local tile range is cut into blocks
// of L tiles (~ one tile row); block slot k of the dispatch takes block c, c+1, c-1, c+2, c-2, ...
// (clipped to the range) and the partial tail block stays last.  c is the block holding the black
// hole's projected screen row, so the photon-ring tiles -- where the capped "Zeno" rays that run
// the full 512-step chain live -- start first and their serial chains overlap the rest of the frame.
// Only the order changes, never a result.
__host__ __device__ inline uint32_t centre_out(uint32_t b, uint32_t n, uint32_t L, uint32_t c) {
    if (L == 0u) return b;
    const uint32_t nb = n / L;
    const uint32_t j = b / L, i = b - j * L;
    if (j >= nb) return b;
    if (c >= nb) c = nb - 1u;
    const uint32_t m = c < nb - 1u - c ? c : nb - 1u - c;  // full pairs on both sides
    uint32_t J;
    if (j == 0u) J = c;
    else if (j <= 2u * m) J = (j & 1u) ? c + (j + 1u) / 2u : c - j / 2u;
    else J = (c - m == 0u) ? c + m + (j - 2u * m) : c - m - (j - 2u * m);
    return J * L + i;
}

}  // namespace bh

namespace bh {
// Dispatch-order buckets by the previous frame's per-tile cost (max n_rk / 2): expensive first.
constexpr uint32_t ORDER_BUCKETS = 6;
// Words of a temporal-order state's counters: [0, B-1) the cost histogram, [B, 2B) the order kernel's
// cursors, [2B] its block ticket.
constexpr uint32_t ORDER_WORDS = 2 * ORDER_BUCKETS + 1;
__host__ __device__ inline uint32_t cost_bucket(uint32_t c) {
    return c >= 128u ? 0u : c >= 64u ? 1u : c >= 32u ? 2u : c >= 20u ? 3u : c >= 12u ? 4u : 5u;
}

// Max over the wave's 64 lanes, every lane active: an inclusive DPP scan (row_shr 1/2/4/8 within each
// 16-lane row, then row_bcast:15 and row_bcast:31 across rows) leaves the max in lane 63.  Out-of-range
// DPP sources read 0, the identity of an unsigned max.  (__shfl_xor: six ds_bpermute round trips and
// ~36 VALU of index arithmetic.)
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp_max_step(uint32_t v) {
    return max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = dpp_max_step<0x111>(v);         // row_shr:1
    v = dpp_max_step<0x112>(v);         // row_shr:2
    v = dpp_max_step<0x114>(v);         // row_shr:4
    v = dpp_max_step<0x118>(v);         // row_shr:8
    v = dpp_max_step<0x142, 0xa>(v);    // row_bcast:15 into rows 1 and 3
    v = dpp_max_step<0x143, 0xc>(v);    // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
}  // namespace bh

// bh_bloom.hip pass shaders (bh::bloom::Shader)
constexpr uint32_t bh_bloom_shader_copy = 0, bh_bloom_shader_down = 1, bh_bloom_shader_up = 2, bh_bloom_shader_remix = 3;

// bh_host.cpp for the host translation units that see only the public ABI (bh_present.cpp): the thread's last
// error, an argument failure, a ctx's device.  Every other host-only declaration lives in bh_host.hpp.
extern "C" __attribute__((visibility("hidden"))) void bh_set_last_error(const std::string& msg);
extern "C" __attribute__((visibility("hidden"))) int bh_bad_arg(const char* fn, int line);
extern "C" __attribute__((visibility("hidden"))) int bh_ctx_device(const bh_ctx* c);
