// bh_march_ray.hpp -- one ray to its end, as the tile schedule's waves march it: the ping-pong loop of the first
// PRIO_ITERS iterations (march_ray), then the tail's loop with the cycle fast-forward (march_cycles) and its
// history in the wave's LDS area (HistLds, hist_lds).  Needs bh_march_step.hpp.
#pragma once
#include "bh_march_step.hpp"

namespace bh {
namespace BH_NS {

// Iterations after which a still-marching wave raises its issue priority (the frame's tail: measured
// +34 % of kernel time at cap 512 vs cap 64 without it) and the tile schedule starts checking for
// cycles (march_cycles).
constexpr uint32_t PRIO_ITERS = 48;

// Waves per workgroup of the tile schedule.  One: a workgroup's LDS (1 KiB decode table + 4 KiB
// cycle history) is released when its one wave ends, and a new wave needs no three other free
// slots on the CU; no workgroup barrier beyond the wave's own table load.  1 vs 4 waves (interleaved
// A/B, profiles/r02d/ab_wg/): headline -0.6 %, 1920x1080 -0.8 %, cap 1000 -1.0 %, one frame per
// launch -1.4 %, 256x256 cap 64 +0.6 % (noise level).  32 such workgroups per CU fill its 160 KiB.
constexpr uint32_t WG_WAVES = 1u;

// ---- cycle fast-forward ----------------------------------------------------------------------------
// One loop iteration is a pure function of (ro, rd, travelled, outside) (s and the uniforms are
// per-ray constants; n_rk only feeds the cap test).  Some rays stop moving in f32: dt rounds to 0 on
// the photon-sphere marker (dps == 0 exactly, a fixed point) or flips sign every step around it (a
// 2-cycle); they then iterate unchanged until the cap (SURVEY §8d "Zeno" rays, up to 512 steps).
// After step j, if the state equals the state two steps back bit for bit (and `outside` did not
// change across those two steps), the sequence is periodic with period 1 or 2 from then on; no
// termination test can fire (both states of the cycle already passed them), so the ray ends with
// fate CAP, n_rk = max_iters and the cycle state of matching parity: the loop's own result,
// without running it.  Checked from PRIO_ITERS on (the cycles found start at median iteration 30).
struct Hist { v3 ro, rd; float tr; uint32_t outside; };

__device__ __forceinline__ bool same_bits(float x, float y) { return __float_as_uint(x) == __float_as_uint(y); }
__device__ __forceinline__ bool same_state(const RayState& st, const Hist& h) {
    // bitwise & (no short-circuit branches)
    return same_bits(st.ro.x, h.ro.x) & same_bits(st.ro.y, h.ro.y) & same_bits(st.ro.z, h.ro.z) &
           same_bits(st.rd.x, h.rd.x) & same_bits(st.rd.y, h.rd.y) & same_bits(st.rd.z, h.rd.z) &
           same_bits(st.travelled, h.tr) & (st.outside == h.outside);
}

// March `st` to termination with the fast-forward; `steps` = RK updates actually executed.  The two
// history states live in LDS (ping-pong slots by iteration parity), not VGPRs: holding them in
// registers takes the kernel from 61 to 73 VGPRs (8 -> 6 waves per SIMD) and measured slower.
struct HistLds { float4 a[2][2][64]; };  // [slot][ro+tr | rd+outside][lane]
// XOR-fold of the state compared by same_state: equal states have equal hashes, so a hash match is
// only a candidate and the full states (in LDS) decide.  The hashes live in 2 VGPRs, so the common
// case reads no LDS and never waits for it (the serial chain of a lone tail wave is the frame's
// critical path).
__device__ __forceinline__ uint32_t state_hash(const RayState& st) {
    return (__float_as_uint(st.ro.x) ^ __float_as_uint(st.ro.y) ^ __float_as_uint(st.ro.z) ^
            __float_as_uint(st.rd.x) ^ __float_as_uint(st.rd.y) ^ __float_as_uint(st.rd.z) ^
            __float_as_uint(st.travelled)) + st.outside * 0x9E3779B9u;
}
// The workgroup's history areas (4 KiB per wave: 8 waves per SIMD still fit, 5 KiB x 32).
template <int>
__device__ __forceinline__ HistLds* hist_lds() {
    __shared__ HistLds hist[WG_WAVES];
    return hist;
}
// The shutter kernel's workgroups (march_tile_shutter_kernel: n waves, n a launch-time value) hold their n
// areas at the start of the dynamic LDS instead, the tables behind them.
__device__ __forceinline__ HistLds* shutter_hist_lds() {
    extern __shared__ float4 shutter_lds[];
    return reinterpret_cast<HistLds*>(shutter_lds);
}
// This wave's area; SHUT: in a workgroup of the shutter kernel.
template <bool SHUT>
__device__ __forceinline__ HistLds& wave_hist() {
    if constexpr (SHUT) return shutter_hist_lds()[threadIdx.x >> 6];
    else return hist_lds<0>()[threadIdx.x >> 6];
}

// March `st` to termination with the fast-forward; `steps` = RK updates actually executed.
// (The tail waves are latency-bound: a ping-pong / uniform-trip form of this loop measured slower.)
// Cycles are looked for until iteration CYCLE_ITERS_END only: the ones found start by iteration ~50
// (median 30); the rays still marching after that crawl or orbit without repeating, and
// stopping the search never changes a result -- the loop then just runs to its normative end.
constexpr uint32_t CYCLE_ITERS_END = 192u;
template <uint32_t SF>
__device__ __forceinline__ uint32_t march_cycles(const MarchArgs& a, const Frame& f, RayState& st, uint32_t& steps,
                                                 HistLds& H, uint32_t lane) {
    // h2: hash of the state two iterations back (none yet: a value that forces a full compare
    // against slot 1, whose travelled is a NaN pattern no arithmetic produces -- no match)
    H.a[1][0][lane] = make_float4(st.ro.x, st.ro.y, st.ro.z, __uint_as_float(0xFFFFFFFFu));
    H.a[1][1][lane] = make_float4(st.rd.x, st.rd.y, st.rd.z, __uint_as_float(st.outside));
    uint32_t h2 = ~state_hash(st), h1 = 0;
    for (uint32_t p = 0;; p ^= 1u) {
        H.a[p][0][lane] = make_float4(st.ro.x, st.ro.y, st.ro.z, st.travelled);
        H.a[p][1][lane] = make_float4(st.rd.x, st.rd.y, st.rd.z, __uint_as_float(st.outside));
        h1 = state_hash(st);
        const uint32_t fate = march_step_tail<SF>(a, f, st);
        if (fate != 0xFFu) { steps = st.n_rk; return fate; }
        if (st.n_rk >= CYCLE_ITERS_END) break;  // wave-uniform: every live lane is at the same iteration
        if (state_hash(st) == h2) {
            const float4 q0 = H.a[p ^ 1u][0][lane], q1 = H.a[p ^ 1u][1][lane];
            const Hist hs{mk(q0.x, q0.y, q0.z), mk(q1.x, q1.y, q1.z), q0.w, __float_as_uint(q1.w)};
            if (same_state(st, hs)) {
                steps = st.n_rk;
                if ((a.max_iters - st.n_rk) & 1u) {
                    const float4 r0 = H.a[p][0][lane], r1 = H.a[p][1][lane];
                    st.ro = mk(r0.x, r0.y, r0.z); st.rd = mk(r1.x, r1.y, r1.z); st.travelled = r0.w;
                }
                st.n_rk = a.max_iters;
                return BH_FATE_CAP;
            }
        }
        h2 = h1;
    }
    // past CYCLE_ITERS_END: the plain loop, no history writes or hashes (a lone tail wave's step is
    // issue-bound, and those were ~8 % of its instructions)
    for (;;) {
        const uint32_t fate = march_step_tail<SF>(a, f, st);
        if (fate != 0xFFu) { steps = st.n_rk; return fate; }
    }
}

// March one ray to its end (the tile schedule's loop): `fate` and `steps` (RK updates executed).
// PEEL (the exact builds' forms that take iteration 0 from the frame's first-step record, march_slot_body): the loop
// starts at iteration it0 = st.n_rk, 0 or 1 (wave-uniform), and *prev is the other state of the ping-pong -- st itself
// before step_first when it0 is 1 (n_rk 0: the roles the comment below describes), any copy of st when it is 0.  The
// PRIO_ITERS iterations then end at PRIO_ITERS + it0, where the priority is raised and the cycle search begins: it reads
// n_rk and is valid from any iteration.  The PEEL loop's steps check k1's numerators as floats (march_step_io, K1F): a
// wave with it0 = 0 runs its iteration 0 through them, and a lane whose ray starts on a coordinate plane then re-runs
// that one step in IEEE ops.
template <uint32_t SF, bool SHUT = false, bool PEEL = false>
__device__ __forceinline__ void march_ray(const MarchArgs& a, const Frame& f, RayState& st, uint32_t& fate,
                                          uint32_t& steps, uint32_t lane, [[maybe_unused]] const RayState* prev = nullptr,
                                          [[maybe_unused]] uint32_t it0 = 0u) {
    // Two iterations per trip, ping-ponging the state between st and sb (march_step_io never
    // writes its input, so no per-step register copies).  The lane's final state is the output
    // of its last iteration, or its input for the fates decided before the RK update: the one of
    // st / sb with the larger n_rk.  The steps of this loop keep no n_rk (step_bf, UNI): the two
    // registers hold what they held at the loop's start -- st 0 or (after step_first) 1, sb 0 --
    // until the lane ends at iteration i, where lane_end writes the one that names the final state:
    // i into the step's input for a fate before the RK update (i >= the input's old value, and a
    // tie goes to st, which is the input at i = 0), i + 1 into its output otherwise (> 1).  So no
    // per-step flag records where the state is, and no per-step count.  (The flag: -6 VALU per step,
    // headline -0.5 %, A/B r02, profiles/r02c/ab_inb/; the count and the late fate: round 24.)
    // The trip condition is wave-uniform and each lane's iteration is
    // predicated: with a divergent loop exit the state would be live out of the loop at a
    // different iteration per lane, which costs a register copy of every state value per
    // iteration.  (390 -> 370 VALU per step; with the flag template and the guard pooling
    // 0.842 -> 0.837 ms headline, 0.99 -> 0.92 ms at cap 1000, A/B r01.)
    RayState sb = st;
    if constexpr (PEEL) sb = *prev;
    const uint32_t first = PEEL ? it0 : 0u;
    bool alive = true;
    // iteration i of a live lane, from `in` into `out`, and the lane's end if it ends there: e is the step's StepEnd,
    // pf the fate it wrote if before_rk (both this step's own: nothing of them is carried from step to step)
    auto iterate = [&](RayState& in, RayState& out, uint32_t i) {
        StepEnd e;
        uint32_t pf;
        if (march_step_io<SF, true, false, PEEL>(a, f, in, out, pf, i, &e)) {
            alive = false;
            if (e.before_rk) {
                in.n_rk = i;
                fate = pf;
            } else {
                out.n_rk = i + 1u;
                // the select stays here, behind an opaque operand: as a plain zext of the step's compare it is
                // formed in the step's own block, on every step
                uint32_t esc = (uint32_t)BH_FATE_ESCAPE;
                asm volatile("" : "+v"(esc));
                fate = e.escape ? esc : (uint32_t)BH_FATE_CAP;
            }
        }
    };
    // TRIP_PAIRS ping-pong pairs per trip of the wave-uniform loop (1 / 2 / 3 pairs: 0.689 / 0.688
    // / 0.686 ms, A/B r01): fewer trip tests and their ballot materialisation per step.
    constexpr uint32_t TRIP_PAIRS = 3;
    static_assert(PRIO_ITERS % (2u * TRIP_PAIRS) == 0u, "whole trips");
    for (uint32_t it = first; it < PRIO_ITERS + first && __builtin_amdgcn_ballot_w64(alive) != 0ull; it += 2u * TRIP_PAIRS) {
#pragma unroll
        for (uint32_t j = 0; j < TRIP_PAIRS; ++j) {
            if (alive) iterate(st, sb, it + 2u * j);
            if (alive) iterate(sb, st, it + 2u * j + 1u);
        }
    }
    if (sb.n_rk > st.n_rk) st = sb;
    if (alive) {
        // still marching: the whole trips ended in st, at iteration PRIO_ITERS + first; the tail's steps keep the
        // books themselves (n_rk, and `outside`, which a camera-outside step of the loop above never wrote)
        st.n_rk = PRIO_ITERS + first;
        if constexpr (sf_cam_out(SF)) st.outside = 1u;
    }
    steps = st.n_rk;
    if (alive) {
        // A wave still marching after PRIO_ITERS iterations (~4x the mean step count) holds a
        // photon-sphere ray that may run to the cap: raise its issue priority so its serial chain
        // is not stretched by the SIMD's other waves (the frame's tail), and watch for cycles.
        __builtin_amdgcn_s_setprio(2);
        fate = march_cycles<SF>(a, f, st, steps, wave_hist<SHUT>(), lane);
    }
}

}  // namespace BH_NS
}  // namespace bh
