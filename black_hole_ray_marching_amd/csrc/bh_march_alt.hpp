// bh_march_alt.hpp -- the two A/B schedules, kept for comparison (tests and the benchmark run them): persistent
// waves with per-lane refill (BH_SCHED_PERSISTENT) and two rays per lane (BH_SCHED_PAIR).  Needs
// bh_march_step.hpp, bh_march_shade.hpp and bh_march_ray.hpp (PRIO_ITERS).
#pragma once
#include "bh_march_ray.hpp"
#include "bh_march_shade.hpp"
#include "bh_march_step.hpp"

namespace bh {
namespace BH_NS {

// ---- schedule BH_SCHED_PERSISTENT: persistent waves with per-lane refill (A/B option) ------------
//
// Each wave keeps all 64 lanes marching.  Rays are prepared (pixel_ray + s, :362-363, :262-263) in
// full-width batches of one 8x8 tile into an LDS "ready" queue, and a lane whose ray terminates pops
// the next ready ray at once, so no lane idles while a slow (photon-sphere "Zeno", capped) ray runs
// on.  Finished rays are pushed into an LDS "done" queue and shaded (sky lookup, :329-345) in
// full-width batches of 64.  Tiles are dequeued from NQ work counters (one 128-B line each; the
// shard-local tile range is split into NQ contiguous parts; a wave starts on part blockIdx % NQ and
// moves on when it is exhausted), so the result never depends on dispatch order or placement.
constexpr uint32_t NQ = 8;
constexpr uint32_t CTR_STRIDE = 32;  // u32 words between counters (128 B)
constexpr uint32_t READY_CAP = 128;
constexpr uint32_t DONE_CAP = 128;

struct WaveQueues {
    float r_x[READY_CAP], r_y[READY_CAP], r_z[READY_CAP], r_s[READY_CAP];
    uint32_t r_idx[READY_CAP];
    float d_x[DONE_CAP], d_y[DONE_CAP], d_z[DONE_CAP];
    uint32_t d_idx[DONE_CAP], d_meta[DONE_CAP];  // meta = fate << 16 | n_rk
};

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {  // set lanes below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

template <uint32_t FMT>
__global__ void __launch_bounds__(256) march_persistent_kernel(MarchArgs a, uint32_t* __restrict__ counters) {
    __shared__ float lut[lds_tables<FMT>()];
    __shared__ WaveQueues queues[4];
    load_srgb_tables<FMT, 256u>(a, lut);
    __syncthreads();  // the only workgroup barrier: waves run independently afterwards

    const uint32_t lane = threadIdx.x & 63u;
    WaveQueues& Q = queues[threadIdx.x >> 6];
    const Frame f = make_frame(a);
    const uint32_t T = a.n_tiles;

    uint32_t part = blockIdx.x % NQ, parts_left = NQ;  // work-queue cursor (wave-uniform)
    uint32_t n_ready = 0, n_done = 0;                  // queue fill levels (wave-uniform)

    RayState st;
    st.ro = f.ro0; st.rd = f.ro0; st.s = 0.0f; st.travelled = 0.0f; st.n_rk = 0; st.outside = 0u;
    uint32_t idx = 0;
    bool alive = false;

    for (;;) {
        // -- refill dead lanes from the ready queue; top the queue up with one tile if short --
        const uint64_t dead = __ballot(!alive);
        const uint32_t n_dead = __popcll(dead);
        if (n_dead != 0u) {
            while (n_ready < n_dead && parts_left != 0u) {
                // dequeue one tile
                uint32_t t = 0xFFFFFFFFu;
                if (lane == 0) {
                    const uint32_t lo = (uint32_t)((uint64_t)T * part / NQ);
                    const uint32_t hi = (uint32_t)((uint64_t)T * (part + 1u) / NQ);
                    const uint32_t i = atomicAdd(&counters[part * CTR_STRIDE], 1u);
                    t = (lo + i < hi) ? lo + i : 0xFFFFFFFFu;
                }
                t = __builtin_amdgcn_readfirstlane(t);
                if (t == 0xFFFFFFFFu) { part = (part + 1u) % NQ; --parts_left; continue; }
                uint32_t tx, ty;
                shard_tile_coords(t, a.tiles_x, a.shard_index, a.shard_count, &tx, &ty);
                const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
                const bool valid = px < a.width && py < a.height;
                const uint64_t vm = __ballot(valid);
                if (valid) {
                    const v3 rd0 = pixel_ray(a, px, py);
                    const uint32_t e = n_ready + lane_rank(vm);
                    Q.r_x[e] = rd0.x; Q.r_y[e] = rd0.y; Q.r_z[e] = rd0.z;
                    Q.r_s[e] = ray_s(f, rd0);
                    Q.r_idx[e] = (uint32_t)out_index(a, t, lane, px, py);
                }
                n_ready += (uint32_t)__popcll(vm);
            }
            __builtin_amdgcn_wave_barrier();
            if (n_ready != 0u) {
                if (!alive) {
                    const uint32_t k = lane_rank(dead);
                    if (k < n_ready) {
                        const uint32_t e = n_ready - 1u - k;
                        st.ro = f.ro0;
                        st.rd = mk(Q.r_x[e], Q.r_y[e], Q.r_z[e]);
                        st.s = Q.r_s[e];
                        idx = Q.r_idx[e];
                        st.travelled = 0.0f; st.n_rk = 0; st.outside = 0u;
                        alive = true;
                    }
                }
                n_ready -= (n_dead < n_ready) ? n_dead : n_ready;
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (__ballot(alive) == 0ull) break;  // no rays left anywhere for this wave

        // -- one RK iteration for every live lane --
        uint32_t fate = 0xFFu;
        if (alive) fate = march_step(a, f, st);
        const bool fin = fate != 0xFFu;
        const uint64_t fm = __ballot(fin);
        if (fm != 0ull) {
            if (fin) {
                const uint32_t e = n_done + lane_rank(fm);
                Q.d_x[e] = st.rd.x; Q.d_y[e] = st.rd.y; Q.d_z[e] = st.rd.z;
                Q.d_idx[e] = idx;
                Q.d_meta[e] = (fate << 16) | st.n_rk;
                alive = false;
            }
            n_done += (uint32_t)__popcll(fm);
            __builtin_amdgcn_wave_barrier();
            // -- shade a full batch of 64 finished rays --
            if (n_done >= 64u) {
                const uint32_t e = n_done - 64u + lane;
                const uint32_t meta = Q.d_meta[e];
                const v3 col = shade(a, lut, meta >> 16, mk(Q.d_x[e], Q.d_y[e], Q.d_z[e]));
                write_pixel<FMT>(a, lut, Q.d_idx[e], col, meta & 0xFFFFu, meta >> 16);
                n_done -= 64u;
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    // -- shade what is left --
    if (lane < n_done) {
        const uint32_t meta = Q.d_meta[lane];
        const v3 col = shade(a, lut, meta >> 16, mk(Q.d_x[lane], Q.d_y[lane], Q.d_z[lane]));
        write_pixel<FMT>(a, lut, Q.d_idx[lane], col, meta & 0xFFFFu, meta >> 16);
    }
}

// ---- schedule BH_SCHED_PAIR: two rays per lane (A/B option) --------------------------------------
// One wave64 = two consecutive shard-local 8x8 tiles; each lane marches the pixel at the same (x&7,
// y&7) position in both (8 px apart for an unsharded frame: coherent step counts) and the loop body
// interleaves the two rays' iterations: on gfx950 one dependent chain per wave issues only every
// ~4-5 cycles however many waves share the SIMD, two chains reach the ~2.3-cycle peak
// (tools/ubench/latency.hip).  Measured slower than the tile schedule (113 VGPRs: 4 waves per
// SIMD instead of 8).
template <uint32_t FMT>
__global__ void __launch_bounds__(256) march_pair_kernel(MarchArgs a) {
    __shared__ float lut[lds_tables<FMT>()];
    load_srgb_tables<FMT, 256u>(a, lut);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pair = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t npairs = (a.n_tiles + 1u) / 2u;
    if (pair >= npairs) return;
    // centre-out over pairs (block = half a tile row of pairs); tiles 2p, 2p+1 stay adjacent
    const uint32_t pp = centre_out(pair, a.n_tiles / 2u, a.order_block / 2u, a.order_centre);
    const uint32_t t0 = 2u * pp, t1 = t0 + 1u;
    const Frame f = make_frame(a);
    uint32_t px0 = 0, py0 = 0, px1 = 0, py1 = 0;
    {
        uint32_t tx, ty;
        shard_tile_coords(t0, a.tiles_x, a.shard_index, a.shard_count, &tx, &ty);
        px0 = tx * 8u + (lane & 7u); py0 = ty * 8u + (lane >> 3);
        if (t1 < a.n_tiles) {
            shard_tile_coords(t1, a.tiles_x, a.shard_index, a.shard_count, &tx, &ty);
            px1 = tx * 8u + (lane & 7u); py1 = ty * 8u + (lane >> 3);
        }
    }
    bool alive0 = px0 < a.width && py0 < a.height;
    bool alive1 = t1 < a.n_tiles && px1 < a.width && py1 < a.height;
    const bool valid0 = alive0, valid1 = alive1;
    RayState s0, s1;
    s0.ro = f.ro0; s0.travelled = 0.0f; s0.n_rk = 0; s0.outside = 0u;
    s1 = s0;
    s0.rd = sel(valid0, pixel_ray(a, px0, py0), f.ro0);
    s1.rd = sel(valid1, pixel_ray(a, px1, py1), f.ro0);
    s0.s = ray_s(f, s0.rd);
    s1.s = ray_s(f, s1.rd);
    uint32_t fate0 = BH_FATE_CAP, fate1 = BH_FATE_CAP;
    for (uint32_t it = 0; alive0 || alive1; ++it) {
        if (it == PRIO_ITERS) __builtin_amdgcn_s_setprio(2);
        march_step2(a, f, s0, s1, alive0, alive1, fate0, fate1);
    }
    if (valid0) write_pixel<FMT>(a, lut, out_index(a, t0, lane, px0, py0), shade(a, lut, fate0, s0.rd), s0.n_rk, fate0);
    if (valid1) write_pixel<FMT>(a, lut, out_index(a, t1, lane, px1, py1), shade(a, lut, fate1, s1.rd), s1.n_rk, fate1);
}

}  // namespace BH_NS
}  // namespace bh
