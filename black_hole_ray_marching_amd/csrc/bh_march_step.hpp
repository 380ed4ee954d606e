// bh_march_step.hpp -- one iteration of the march loop: the per-ray state (Frame, RayState, pixel_ray, ray_s),
// the scene-flag folds (SF_*), the root-free tests (sdf_term_slacks, sdf_skip_slack), the step itself (step_bf),
// the latency build's packed tail step (step_tail), and the forms the schedules call: march_step_io, march_step,
// march_step_tail, march_step2.  Needs bh_march_ops.hpp.
#pragma once
#include "bh_march_ops.hpp"

namespace bh {
namespace BH_NS {

// ---- per-ray pieces of get_col (:259-345) -------------------------------------------------------

// Per-frame invariants (identical for every pixel: ro0 == camera.pos, :363).
struct Frame {
    v3 ro0;
    v3 cps;      // photon-sphere centre -normalize(ro0) * 1.5 * RS  (:294)
    float k;     // (DP * RS) * -1.5: the scalar prefix of rd_derivative (:126)
};
__device__ __forceinline__ Frame make_frame(const MarchArgs& a) {
    Frame f;  // invariants precomputed on the host (bh_host.cpp, frame_constants)
    f.ro0 = mk(a.pos[0], a.pos[1], a.pos[2]);
    f.cps = mk(a.cps[0], a.cps[1], a.cps[2]);
    f.k = a.kfac;
    return f;
}

// vs_main + rasteriser interpolation + fs_main :362 for pixel (px, py): the world-space corner rays of
// the screen triangle (3,1),(-1,1),(-1,-3) interpolated at the pixel centre, normalised.
// Exact mode: the two divisions use the division core (numerators in [0.5, 2^32], denominators 2W,
// 2H in [2, 2^33]: always inside its domain) with the reciprocals RN(1/2W), RN(1/2H) from the host, and
// the normalisation normalize_x.
__device__ __forceinline__ v3 pixel_ray(const MarchArgs& a, uint32_t px, uint32_t py) {
#if BH_FAST
    const float l0 = ((float)px + 0.5f) / (2.0f * (float)a.width);
    const float l2 = ((float)py + 0.5f) / (2.0f * (float)a.height);
#else
    const float l0 = crm::div_core((float)px + 0.5f, crm::Rcp{2.0f * (float)a.width, a.rw2});
    const float l2 = crm::div_core((float)py + 0.5f, crm::Rcp{2.0f * (float)a.height, a.rh2});
#endif
    const float l1 = (1.0f - l0) - l2;
    const v3 d = add(add(smul(l0, mk(a.c0[0], a.c0[1], a.c0[2])), smul(l1, mk(a.c1[0], a.c1[1], a.c1[2]))),
                     smul(l2, mk(a.c2[0], a.c2[1], a.c2[2])));
#if BH_FAST
    return normalize(d);
#else
    return normalize_x(d);
#endif
}

// s = ((DP*RS)*-1.5) * h2 with h2 = |ro0 x rd0|^2 (:262-263), hoisted out of rd_derivative.
__device__ __forceinline__ float ray_s(const Frame& f, v3 rd0) {
    const v3 c = cross(f.ro0, rd0);
    return f.k * dot(c, c);
}

struct RayState {
    v3 ro, rd;
    float travelled;
    float s;
    uint32_t n_rk;
    uint32_t outside;  // 0 / 1: the WGSL's `outside` (:270); u32, so the blackout test stays compare + select
};

// ---- one RK iteration, branch-free ---------------------------------------------------------------
//
// The early exits of the loop body (:272-288) are predicates and the state update is a select, so a
// whole iteration is one basic block: the pair schedule interleaves two rays' iterations and the
// scheduler fills each ray's dependency stalls with the other's instructions.  (Ops: bh_march_ops.hpp.)

// One iteration of the loop body (:266-328) from `in` into `out`.  Returns BH_FATE_* if the ray
// terminates in this iteration (n_rk counts completed RK updates), or 0xFF if it continues.
//
// BRANCHY = true (single-ray schedules): a lane whose ray terminates before the RK update (surface /
// blackout, fate >= BH_FATE_SURFACE) returns at once WITHOUT writing `out`: its final state is `in`
// (only n_rk is read for those fates).  Every other lane gets the whole updated state in `out`.
// `in` is never written, so the caller ping-pongs two states and no register copies are needed
// (the IEEE re-run of march_step_io reads `in` again); the RK block is skipped when every active
// lane terminates.  BRANCHY = false keeps one basic block for the pair schedule: `out` is always
// written (selects).  `in` and `out` may alias only when BRANCHY = false.
// Scene flags: a kernel instantiated for one flag set (SF) drops the per-step flag selects.
constexpr uint32_t SF_DYN = 0xFFFFFFFFu;
// SF_CAM_OUT (with a fixed flag set only): the frame's camera lies outside the unit sphere, so the
// blackout test reduces to `!(r > 1)` (march_slot picks the instantiation per wave).  Every ray starts
// at the camera (:363), so at iteration 0 r > 1, no exit fires and `has_been_outside_eh` becomes true;
// from then on a ray with !(r > 1) returns black through :280-281 whether or not :273-274's
// `dot(rd, ro) < 0` holds.  The step then needs neither that product nor the `outside` state (kept
// at 1): -8 VALU per step.  march_slot also requires |s| <= 2^30 on every lane of the wave (the
// division cores' numerator bound, a per-ray constant), so this step does not re-check it.
constexpr uint32_t SF_CAM_OUT = 0x100u;
constexpr uint32_t sf_scene(uint32_t sf) { return sf == SF_DYN ? SF_DYN : (sf & BH_SCENE_DEFAULT); }
constexpr bool sf_cam_out(uint32_t sf) { return sf != SF_DYN && (sf & SF_CAM_OUT) != 0u; }

// r > 1 for r = RN(sqrt(r2)) exactly when r2 > 1 + 2^-23 (step_bf)
constexpr float R2_GT1 = 0x1.000002p0f;

__device__ __forceinline__ bool fate_before_rk(uint32_t fate) { return fate >= BH_FATE_SURFACE; }

// The lanes (of those active) where p holds.  For p a single compare this is the compare's result as it stands.
__device__ __forceinline__ uint64_t lane_mask(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// (Measured and not kept, DESIGN.md §5: a "sticky" root-free test that skips the test after a step that took
// the roots; per-term ballots deciding the all-terms test too, 0.5189 vs 0.5193 ms, profiles/r05/sdf_terms3/;
// terms cleared by the lane's radius alone, 0.5217 -> 0.5261 ms, profiles/r05/sdf_radii/, §5 item 29.)
#ifdef BH_DIAG_SLOW
__device__ uint32_t g_diag_skip_wave_steps, g_diag_all_wave_steps, g_diag_far_wave_steps;
// one count per wave: the lowest active lane adds (a global atomic: a vector memory op)
#define BH_DIAG_SKIP_COUNT()                                                                              \
    do {                                                                                                  \
        if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true)))          \
            atomicAdd(&g_diag_skip_wave_steps, 1u);                                                       \
    } while (0)
#define BH_DIAG_FAR_COUNT()                                                                               \
    do {                                                                                                  \
        if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true)))          \
            atomicAdd(&g_diag_far_wave_steps, 1u);                                                        \
    } while (0)
#else
#define BH_DIAG_SKIP_COUNT() do {} while (0)
#define BH_DIAG_FAR_COUNT() do {} while (0)
#endif

#if !BH_FAST
// Does this lane's step have dt == dtm*r (:307-310) and no surface hit (:286-288), whatever its three SDF
// roots are?  From the step's own rounded values (r = RN(sqrt r2), dtr = RN(dtm r), rho2, y*y, the markers'
// qm and the photon sphere's qps, all formed exactly as the full step forms them), with no root:
//   T = RN(1.125 dtr + 0.002);  a distance term d = RN(RN(sqrt v) - c) passes when v >= u*u, u = RN(T + c)
//   (tested as fma(-u, u, v) >= 0: one rounding, which keeps the sign of the exact difference):
//   disc (:121)     rho2 >= (T + RN(6 rs))^2  or  y*y >= (T + 0.02)^2   [disc >= RN(rho - 6rs) and
//                   >= RN(|y| - 0.02): fmaxf is >= each non-NaN operand]
//   markers         qm  >= (T + 0.5)^2        photon sphere (:294)  qps >= (T + 0.075)^2
// Proof that a passing lane has dt == dtr and no surface (exact mode: RN sqrt, IEEE ops; dtm > 0 and
// 0 < rs <= 8, the host's skip_sdf gate, so dtr >= 0 and T >= 0.002 (1 - 2^-24)): u = RN(T + c) >=
// (T + c)(1 - 2^-24), so sqrt v >= (T + c)(1 - 2^-24) (for y*y = RN(y^2) one more factor) and
// RN(sqrt v) >= (T + c)(1 - 2^-22); d >= RN(T - (T + c) 2^-22) >= T (1 - 2^-17.6)
// (c <= 48.0001, T >= 0.00199).  So dist = min of the enabled terms >= that bound >= 0.00199 > MIN_DIST
// (no surface), and 0.9f d >= (0.9f * 1.125) dtr (1 - 2^-17.5) = 1.0125 dtr (1 - 2^-17.5) > dtr, so
// RN(0.9f dist) >= dtr (dtr is a float) and fminf(RN(dist * 0.9), dtr) == dtr.  The terms combine with
// the step's own fmaxf / fminf, so a NaN term is dropped exactly where the step drops that distance (a NaN
// argument makes the step's term NaN too); a NaN T (r or dtr NaN) makes every term NaN and the slack NaN,
// which fails; T = +inf gives -inf (finite v) or NaN (v = +inf) terms, which fail or are dropped.
// In the exact build's core pass a wrong r (r2 outside the root core's domain) also raises the k1
// division guard, so that step re-runs in IEEE ops, where the proof holds as written.
// tests/test_skip.py checks the implication on adversarial samples of the step's float32 arithmetic.
// The same test term by term: each term's slack >= 0 alone proves that term's distance
// >= T (1 - 2^-17.6) by the argument above, so a term whose slack holds can be left out of dist (taken as
// +inf): if it was the minimum, every other term is at least as large and still gives RN(0.9 dist) >= dtr;
// its surface test could not fire; and fminf drops a NaN term exactly as it drops +inf.
// tests/test_skip.py::test_per_term_skip_keeps_dt_and_surface checks every subset of cleared terms.
struct SdfSlack { float disc, mark, ps; };
__device__ __forceinline__ SdfSlack sdf_term_slacks(const MarchArgs& a, uint32_t flags, float dtr, float rho2, float yy,
                                                   float qm, float qps) {
    const float T = __builtin_fmaf(dtr, 1.125f, 0.002f);
    const float u6 = T + 6.0f * a.rs, uy = T + 0.02f;
    // v - u^2 rounded once (fma): its sign is the sign of the exact v - u*u
    float disc = fmaxf(__builtin_fmaf(-u6, u6, rho2), __builtin_fmaf(-uy, uy, yy));
    const float um = T + 0.5f;
    float mark = __builtin_fmaf(-um, um, qm);
    const float up = T + 0.075f;
    float ps = __builtin_fmaf(-up, up, qps);
    // a disabled term clears -- unless T is NaN: sdf_skip_slack's fminf would drop the other terms' NaN for it, and
    // with no surfaces at all the step's dt is then fminf(+inf, NaN) = +inf, not dtm r
    const float off = T != T ? T : __builtin_inff();
    if (!(flags & BH_SCENE_DISC)) disc = off;
    if (!(flags & BH_SCENE_MARKERS)) mark = off;
    return {disc, mark, ps};
}
__device__ __forceinline__ float sdf_skip_slack(const SdfSlack& t) { return fminf(fminf(t.disc, t.mark), t.ps); }
#endif

// How a lane's step ended, where step_bf returned true under the UNI contract: before the RK update (`fate` written)
// or after it, by escape or by the cap.  Lane masks.
struct StepEnd { bool before_rk, escape; };
// UNI: every active lane of the wave is at loop iteration `it` (the ping-pong loop, march_ray), so the cap test is a
// wave-uniform (scalar) compare -- and the step keeps no books that only a lane's end reads: it neither reads nor
// writes n_rk (the caller knows `it`), and it writes `fate` only where a lane ends before the RK update; *end says
// which end it was (StepEnd), and for a lane that ends after the update the caller's done-block forms the fate from
// it, so no step that ends nothing pays for a fate (-2 VALU on every step).
// SF_CAM_OUT steps do not write `outside` either: nothing in them reads it (march_ray sets it where the tail begins).
// TINY (the tail's steps): rd + 0.5 k unfused -- the WGSL's own op order, exact for any dt -- where the fused
// form's premise (|dt| >= 2^-25) would send a step with a tiny dt to the IEEE re-run.  The photon-sphere rays whose steps shrink below 2^-25 without
// settling into an exact cycle take hundreds of such steps (camera B: 42 rays, ~210 tiny steps each).
template <bool BRANCHY, class Ops, uint32_t SF = SF_DYN, bool UNI = false, bool TINY = false>
__device__ __forceinline__ bool step_bf(const MarchArgs& a, const Frame& f, const RayState& in, RayState& out, Ops& X,
                                        uint32_t& fate, uint32_t it = 0u, [[maybe_unused]] StepEnd* end = nullptr) {
    constexpr uint32_t SFS = sf_scene(SF);
    constexpr bool CO = sf_cam_out(SF);
    static_assert(!UNI || BRANCHY, "the uniform-iteration contract is the single-ray step's");
    const uint32_t scene_flags = (SFS == SF_DYN) ? a.scene_flags : SFS;
    const v3 ro = in.ro, rd = in.rd;
    const float travelled = in.travelled, s = in.s;
    const uint32_t n_rk = UNI ? it : in.n_rk;
    const float r2 = dot(ro, ro);
    const float r = X.sqrt(r2);                                        // :271
    // :272-283: blackout if (r < 1 and rd.ro < 0), or if !(r > 1) and the ray was outside before;
    // r > 1 sets `outside`.  Bitwise (not short-circuit) logic: lane masks, no branches.
    // The tests read r^2: for r = RN(sqrt(r2)),  r < 1  <=>  r2 < 1  and  r > 1  <=>  r2 > 1 + 2^-23
    // (RN(sqrt) is monotone; sqrt(1 + 2^-23) < 1 + 2^-24, the midpoint above 1, and
    // sqrt(next float) > it; NaN fails every compare either way; tests/test_oracle.py checks every
    // float in [1/4, 4]).  So the exits do not wait for the root, and lanes that leave here need no
    // guard on it.
    const bool bo_on = a.blackout_eh != 0u;
    const bool not_out = !(r2 > R2_GT1);                               // NaN: "else" branch, as the WGSL
    // Lane masks (MASKS: the exact builds' single-ray step, whose wave-uniform tests below read them): 64-bit masks,
    // each the ballot of ONE compare -- that is the compare's own SGPR pair -- combined by scalar ops.  (The ballot
    // of an and/or of predicates goes through a VGPR instead: v_cndmask 0,1 + v_cmp_ne, 2 VALU each, on every step.)
    // bo_all: all lanes when the blackout test is on; m_bo: the lanes that leave by it, which no test below waits for.
    constexpr bool MASKS = BRANCHY && !BH_FAST;
    [[maybe_unused]] const uint64_t bo_all = bo_on ? ~0ull : 0ull;
    bool blackout;
    [[maybe_unused]] uint64_t m_bo = 0ull;
    if constexpr (CO) {
        blackout = bo_on & not_out;  // `outside` is 1 from iteration 0 on (SF_CAM_OUT)
        if constexpr (MASKS) m_bo = lane_mask(not_out) & bo_all;
    } else if constexpr (MASKS) {
        // rd.ro < 0 only matters for lanes inside r < 1; formed on every step all the same (behind a wave-uniform
        // test the compiler speculates the product into the step anyway, and the test's own ballot costs 2 VALU)
        const bool ingoing = dot(rd, ro) < 0.0f, was_out = in.outside != 0u;
        blackout = bo_on & (((r2 < 1.0f) & ingoing) | (not_out & was_out));
        m_bo = ((lane_mask(r2 < 1.0f) & lane_mask(ingoing)) | (lane_mask(not_out) & lane_mask(was_out))) & bo_all;
    } else {
        // The pair schedule's block and the fast build keep the form their code was measured and, in fast math,
        // contracted with: rd.ro < 0 behind a wave-uniform test.  (The pair kernel inlines the step once per ray of a
        // lane; in fast math the two copies must contract alike, or a pixel's bytes depend on which of the two it is.)
        bool ingoing = false;
        if (__builtin_amdgcn_ballot_w64(bo_on & (r2 < 1.0f)) != 0ull) ingoing = dot(rd, ro) < 0.0f;
        blackout = bo_on & (((r2 < 1.0f) & ingoing) | (not_out & (in.outside != 0u)));
    }
    float rho2, yy, qm;
    const float dtr = a.dtm * r;                                       // :307-310's second operand
    float dt;
    bool surface = false;
#if !BH_FAST
    // Far field: a lane with a.far_r2 <= r^2 <= FLT_MAX (the host's sdf_far_r2, +inf when off) is so far
    // from the disc, the markers and the photon sphere that every distance term exceeds the root-free
    // test's threshold by construction (proof at sdf_far_r2, bh_host.cpp): when every lane that stays is
    // there, the wave forms no SDF argument at all.  (r^2 = +inf is excluded: there dtm r is +inf while a
    // distance term may stay finite.)
    if (BRANCHY && ((lane_mask(!(r2 >= a.far_r2)) | lane_mask(!(r2 <= 0x1.fffffep127f))) & ~m_bo) == 0ull) {
        BH_DIAG_FAR_COUNT();
        if (blackout) {
            fate = (uint32_t)BH_FATE_BLACKOUT;
            if constexpr (UNI) end->before_rk = true;
            return true;
        }
        dt = dtr;
    } else
#endif
    {
    X.sdf_args(ro, rho2, yy, qm);                                      // the SDF roots' arguments
    [[maybe_unused]] bool full = true;  // BRANCHY: no root-free arm below has formed dt (else constant)
#if !BH_FAST
    // Root-free step (BRANCHY): dt = min(0.9 dist, dtm r) needs dist only where it could fall below
    // dtm r / 0.9, and the surface test only below MIN_DIST.  sdf_skip_slack decides "dt == dtm r, no surface"
    // from the squared arguments; when it holds on every live lane (blackout lanes leave either way)
    // the wave skips the three roots, their guards and the distance arithmetic.  Same bits: see sdf_term_slacks.
    // The photon-sphere argument (:294) is formed before the exits for the test.
    if constexpr (BRANCHY) {
        const v3 dc = sub(f.cps, ro);
        const float qps = dot(dc, dc);
        // lanes that need the roots: slack < 0 or NaN, except those that leave by the blackout exit (masked as
        // integers: m_bo).  (Round 4 measured this form 0.9 % slower, profiles/r04/ab_skip_forms/, before the kernel
        // was issue-bound; DESIGN.md §10 round 24 has the measurement that replaced it.)
        const SdfSlack terms = sdf_term_slacks(a, scene_flags, dtr, rho2, yy, qm, qps);
        const bool fast = a.skip_sdf != 0u && (lane_mask(!(sdf_skip_slack(terms) >= 0.0f)) & ~m_bo) == 0ull;
        if (fast) {
            BH_DIAG_SKIP_COUNT();
            if (blackout) {
                fate = (uint32_t)BH_FATE_BLACKOUT;
                if constexpr (UNI) end->before_rk = true;
                return true;
            }
            dt = dtr;
            full = false;
        } else if (a.skip_sdf != 0u) {
            // per term: a root only where some lane that stays needs it (sdf_term_slacks); where the disc
            // and markers both clear, the photon sphere alone keeps the wave here (about 98 % of these
            // wave-steps clear it, and 80 % one of the other two: tools/skip_sim.py)
            const bool nd = (lane_mask(!(terms.disc >= 0.0f)) & ~m_bo) != 0ull;
            const bool nm = (lane_mask(!(terms.mark >= 0.0f)) & ~m_bo) != 0ull;
            const bool np = (lane_mask(!(terms.ps >= 0.0f)) & ~m_bo) != 0ull;
            float dv = __builtin_inff(), mv = __builtin_inff();
            if (nd) {
                dv = X.disc_from(ro, a.rs, rho2);
                X.sq_arg(rho2);
            }
            if (nm) {
                mv = X.mark_from(qm);
                X.sq_arg(qm);
            }
            // (the mins of this arm: fmin_quiet -- dv, mv and dps are a root's distance or +inf, never signalling)
            const float ds = sdf_of_terms_quiet(scene_flags, dv, mv);    // :285
            if (blackout | (ds < MIN_DIST)) {                            // :286-288
                fate = blackout ? (uint32_t)BH_FATE_BLACKOUT : (uint32_t)BH_FATE_SURFACE;
                if constexpr (UNI) end->before_rk = true;
                return true;
            }
            float dps = __builtin_inff();
            if (np) {
                dps = X.sqrt(qps) - 0.075f;
                X.sq_arg(qps);
            }
            const float dist = fmin_quiet(ds, dps);                      // :299
            dt = fmin_quiet(dist * 0.9f, dtr);                           // :307-310
            full = false;
        }
        // else the root-free step is off (the host's skip_sdf gate): every root, below
    }
#endif
    if (!BRANCHY || full) {
        const float ds = X.sdf_from(ro, a.rs, scene_flags, rho2, qm);  // :285
        // the root guards of the enabled terms (a disabled term's value is discarded; a kernel built for
        // one flag set drops its arithmetic entirely)
        if constexpr (SFS == SF_DYN || SFS == BH_SCENE_DEFAULT) X.sq_args(rho2, qm);
        else if constexpr (SFS == BH_SCENE_DISC) X.sq_arg(rho2);
        else if constexpr (SFS == BH_SCENE_MARKERS) X.sq_arg(qm);
        surface = ds < MIN_DIST;                                           // :286-288
        if constexpr (BRANCHY) {
            if (blackout | surface) {
                fate = blackout ? (uint32_t)BH_FATE_BLACKOUT : (uint32_t)BH_FATE_SURFACE;
                if constexpr (UNI) end->before_rk = true;
                return true;
            }
        }
        // :294 after the exits (measured: 1.5 % faster than before them, A/B r01; neutral without
        // machine scheduling)
        const v3 dc = sub(f.cps, ro);
        const float qps = dot(dc, dc);
        const float dps = X.sqrt(qps) - 0.075f;
        X.sq_arg(qps);
        const float dist = fminf(ds, dps);                                 // :299
        dt = fminf(dist * 0.9f, dtr);                                      // :307-310
    }
    }
    // get_delta_photon_rk4 (:134-151).  UNF (the tail's steps, TINY): rd + 0.5 k as its two IEEE ops, the WGSL's
    // order, exact for any dt (XOps::rd_half's fma equals it only for |dt| >= 2^-25); the rest keeps the cores
    // and their guards (the x/6 core's domain, |x| >= 2^-60, is checked as always).
    v3 dro, drd;
    auto rk_update = [&](auto UNFc) {
        constexpr bool UNF = decltype(UNFc)::value;
        auto rd_half = [&](v3 v, v3 k) { return UNF ? add(v, smul(0.5f, k)) : X.rd_half(v, k); };
        const v3 ro_k1 = smul(dt, rd);
        const v3 rd_k1 = smul(dt, X.template accel_qs<1>(ro, s, r2, r));
        const v3 ro_k2 = smul(dt, rd_half(rd, rd_k1));
        const v3 rd_k2 = smul(dt, X.template accel<2>(X.ro_half(ro, ro_k1), s));
        const v3 ro_k3 = smul(dt, rd_half(rd, rd_k2));
        const v3 rd_k3 = smul(dt, X.template accel<3>(X.ro_half(ro, ro_k2), s));
        const v3 ro_k4 = smul(dt, add(rd, rd_k3));
        const v3 rd_k4 = smul(dt, X.template accel<4>(add(ro, ro_k3), s));
        const v3 sro = add(X.add2(X.add2(ro_k1, ro_k2), ro_k3), ro_k4);
        const v3 srd = add(X.add2(X.add2(rd_k1, rd_k2), rd_k3), rd_k4);
        dro = X.template div6<0>(sro);
        drd = X.template div6<1>(srd);
#if !BH_FAST
        if constexpr (Ops::kCR) {
            // Domain of the division cores: every numerator is 0 or >= 2^-60 in magnitude, and
            // |s| <= 2^30, which with Q <= 2^60 (|p| <= 2^12) bounds every |s*p_i| <= 2^42.
            if constexpr (!Ops::kK1F) X.bad |= X.kmin < crm::KEY_ACC_MIN;  // K1F: k1's numerators are in amin
            X.bad |= !(X.amin >= crm::ACC_N_MIN);
            if constexpr (!UNF) X.bad |= (fabsf(dt) < 0x1p-25f) & (dt != 0.0f);  // rd_half's premise
            X.bad |= !(X.amin6 >= crm::DIV_N_MIN) & (dt != 0.0f);
            if constexpr (!CO) X.bad |= !(fabsf(s) <= 0x1p30f);  // SF_CAM_OUT: checked once per wave
        }
#endif
    };
#if BH_FAST
    rk_update(std::false_type{});
#else
    rk_update(std::bool_constant<TINY && Ops::kCR>{});
#endif
    const v3 nro = add(ro, dro), nrd = add(rd, drd);                   // :315, :322
    const float ntr = travelled + dt;                                  // :324
    out.s = s;
    if constexpr (!CO) out.outside = not_out ? in.outside : 1u;        // only read when bo_on
    const bool escape = ntr > a.max_dist;                              // :325-327
    const bool capped = n_rk + 1u >= a.max_iters;                      // loop end (:266)
    if constexpr (BRANCHY) {
        out.ro = nro;
        out.rd = nrd;
        out.travelled = ntr;
        if constexpr (UNI) {
            *end = StepEnd{false, escape};
        } else {
            out.n_rk = n_rk + 1u;
            fate = escape ? (uint32_t)BH_FATE_ESCAPE : (uint32_t)BH_FATE_CAP;
        }
        return escape | capped;
    }
    const bool pre = blackout | surface;
    const bool go = !pre;
    out.ro = sel(go, nro, ro);
    out.rd = sel(go, nrd, rd);
    out.travelled = go ? ntr : travelled;
    out.n_rk = n_rk + (go ? 1u : 0u);
    // flat selects (a nested ?: becomes exec-mask branches)
    const uint32_t pre_fate = blackout ? (uint32_t)BH_FATE_BLACKOUT : (uint32_t)BH_FATE_SURFACE;
    const uint32_t post_fate = escape ? (uint32_t)BH_FATE_ESCAPE : (uint32_t)BH_FATE_CAP;
    fate = go ? post_fate : pre_fate;
    return pre | escape | capped;
}

#ifdef BH_DIAG_SLOW
__device__ uint32_t g_diag_slow_lane_steps, g_diag_slow_wave_steps;  // (g_diag_skip/all_wave_steps above)
#endif

#ifndef BH_TAIL_PACKED
#define BH_TAIL_PACKED 0
#endif
#if !BH_FAST && BH_TAIL_PACKED
// ---- the tail's step, in packed FP32 (exact mode) ---------------------------------------------------
// The same arithmetic as step_bf<true, XOps<true>> -- every rounding identical, in the same order, the
// same guards -- with the x and y components of each vector in one 64-bit register pair, so that one
// v_pk_{add,mul,fma}_f32 does both.  It runs only in the cycle-watch loop (march_cycles), i.e. in waves
// still marching after PRIO_ITERS iterations, which are few per SIMD: a wave alone issues a packed op
// in the slot of a scalar one (tools/ubench/lone_wave.hip: 4.6 vs 4.7 cycles, profiles/r02/lone_wave.log),
// so the tail's serial step chain gets shorter; at 8 waves per SIMD a packed op costs more than two
// scalar ones (5.7 vs 2 x 2.3 cycles), so the bulk keeps the scalar step.
typedef float f2 __attribute__((ext_vector_type(2)));
struct p3 { f2 xy; float z; };
__device__ __forceinline__ p3 pk(v3 a) { return {f2{a.x, a.y}, a.z}; }
__device__ __forceinline__ v3 unpk(p3 a) { return mk(a.xy.x, a.xy.y, a.z); }
__device__ __forceinline__ f2 bc(float s) { return f2{s, s}; }
__device__ __forceinline__ f2 pfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ p3 padd(p3 a, p3 b) { return {a.xy + b.xy, a.z + b.z}; }
__device__ __forceinline__ p3 psub(p3 a, p3 b) { return {a.xy - b.xy, a.z - b.z}; }
__device__ __forceinline__ p3 psmul(float s, p3 a) { return {bc(s) * a.xy, s * a.z}; }  // s*x == x*s
// dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
__device__ __forceinline__ float pdot(p3 a, p3 b) {
    const f2 m = a.xy * b.xy;
    return (m.x + m.y) + a.z * b.z;
}
// div_core of the three components by one refined reciprocal
__device__ __forceinline__ p3 pdiv(p3 n, const crm::Rcp& R) {
    const p3 y{n.xy * bc(R.r), n.z * R.r};
    const p3 e{pfma(bc(R.d), y.xy, -n.xy), __builtin_fmaf(R.d, y.z, -n.z)};
    return {pfma(-e.xy, bc(R.r), y.xy), __builtin_fmaf(-e.z, R.r, y.z)};
}
__device__ __forceinline__ p3 pdiv6(p3 x) {  // crm::div6 per component
    return {pfma(x.xy, bc(crm::R6_H), x.xy * bc(crm::R6_L)), crm::div6(x.z)};
}
__device__ __forceinline__ p3 pro_half(p3 ro, p3 k) {  // ro + 0.5 k, as XOps<true>::ro_half
    return {pfma(bc(0.5f), k.xy, ro.xy), __builtin_fmaf(0.5f, k.z, ro.z)};
}
__device__ __forceinline__ p3 padd2(p3 a, p3 b) {  // a + 2b, as XOps<true>::add2
    return {pfma(bc(2.0f), b.xy, a.xy), __builtin_fmaf(2.0f, b.z, a.z)};
}

struct PkGuard {
    bool bad = false;
    uint32_t kmin;
    float amin, amin6;
};

// rd_derivative as XOps<true>::accel_qs<K>
template <int K>
__device__ __forceinline__ p3 paccel_qs(p3 p, float s, float q, float sq, PkGuard& G) {
    const float Q = (q * q) * sq;
    const p3 n = psmul(s, p);
    G.bad |= crm::div_d_bad(Q);
    if constexpr (K == 1) G.kmin = crm::kmin3(crm::key(n.xy.x), crm::key(n.xy.y), crm::key(n.z));
    else if constexpr (K == 2) G.amin = XOps<true>::absmin3(n.xy.x, n.xy.y, n.z);
    else G.amin = XOps<true>::absmin3(G.amin, n.xy.x, n.xy.y, n.z);
    return pdiv(n, crm::rcp_refined(Q));
}
template <int K>
__device__ __forceinline__ p3 paccel(p3 p, float s, PkGuard& G) {
    const float q = pdot(p, p);
    return paccel_qs<K>(p, s, q, crm::sqrt_core(q), G);
}

// step_bf<true, XOps<true>, SF> with packed pairs (see above): same contract (`out` is not written for
// the fates decided before the RK update), `G.bad` set when an operand left a core's domain.
template <uint32_t SF>
__device__ __forceinline__ bool step_tail(const MarchArgs& a, const Frame& f, const RayState& in, RayState& out,
                                          PkGuard& G, uint32_t& fate) {
    constexpr uint32_t SFS = sf_scene(SF);
    constexpr bool CO = sf_cam_out(SF);
    const uint32_t scene_flags = (SFS == SF_DYN) ? a.scene_flags : SFS;
    const p3 ro = pk(in.ro), rd = pk(in.rd);
    const float travelled = in.travelled, s = in.s;
    const uint32_t n_rk = in.n_rk;
    const f2 sq_xy = ro.xy * ro.xy;                 // x*x, y*y
    const float zz0 = ro.z * ro.z;
    const float r2 = (sq_xy.x + sq_xy.y) + zz0;     // dot(ro, ro)
    const float r = crm::sqrt_core(r2);
    const bool bo_on = a.blackout_eh != 0u;
    const bool not_out = !(r2 > R2_GT1);
    bool blackout;
    if constexpr (CO) {
        blackout = bo_on & not_out;
    } else {
        bool ingoing = false;
        if (__builtin_amdgcn_ballot_w64(bo_on & (r2 < 1.0f)) != 0ull) ingoing = pdot(rd, ro) < 0.0f;
        blackout = bo_on & (((r2 < 1.0f) & ingoing) | (not_out & (in.outside != 0u)));
    }
    // sdf (XOps::sdf_args, sdf_from): disc from rho^2 = x*x + z*z, markers from the near sphere of each pair
    const float rho2 = sq_xy.x + zz0;
    const float rho = crm::sqrt_core(rho2);
    const float disc = fmaxf(fmaxf(rho - 6.0f * a.rs, -(rho - 3.0f * a.rs)), fabsf(ro.xy.y - 0.0f) - 0.02f);
    const float dz = -10.0f - ro.z, zz = dz * dz;
    const f2 t{10.0f - fabsf(ro.xy.x), 10.0f - fabsf(ro.xy.y)};  // (tx, ty)
    const f2 t2 = t * t;                                            // (tx*tx, ty*ty)
    // (qy, qx) = ((xx + ty*ty) + zz, (yy + tx*tx) + zz); tx*tx + yy == yy + tx*tx exactly
    const f2 qyx = (sq_xy + t2.yx) + bc(zz);
    const float qm = fminf(qyx.x, qyx.y);
    const float m = crm::sqrt_core(qm) - 0.5f;
    const float ds = sdf_of_terms(scene_flags, disc, m);
    if constexpr (SFS == SF_DYN || SFS == BH_SCENE_DEFAULT) G.bad |= crm::sqrt_bad2(rho2, qm);
    else if constexpr (SFS == BH_SCENE_DISC) G.bad |= crm::sqrt_bad(rho2);
    else if constexpr (SFS == BH_SCENE_MARKERS) G.bad |= crm::sqrt_bad(qm);
    const bool surface = ds < MIN_DIST;
    if (blackout | surface) {
        fate = blackout ? (uint32_t)BH_FATE_BLACKOUT : (uint32_t)BH_FATE_SURFACE;
        return true;
    }
    const p3 dc = psub(pk(f.cps), ro);
    const float qps = pdot(dc, dc);
    const float dps = crm::sqrt_core(qps) - 0.075f;
    G.bad |= crm::sqrt_bad(qps);
    const float dist = fminf(ds, dps);
    const float dt = fminf(dist * 0.9f, a.dtm * r);
    // the RK update in the tail's form (step_bf TINY): rd + 0.5 k unfused, exact for any dt
    auto rd_half = [&](p3 v, p3 k) { return padd(v, psmul(0.5f, k)); };
    const p3 ro_k1 = psmul(dt, rd);
    const p3 rd_k1 = psmul(dt, paccel_qs<1>(ro, s, r2, r, G));
    const p3 ro_k2 = psmul(dt, rd_half(rd, rd_k1));
    const p3 rd_k2 = psmul(dt, paccel<2>(pro_half(ro, ro_k1), s, G));
    const p3 ro_k3 = psmul(dt, rd_half(rd, rd_k2));
    const p3 rd_k3 = psmul(dt, paccel<3>(pro_half(ro, ro_k2), s, G));
    const p3 ro_k4 = psmul(dt, padd(rd, rd_k3));
    const p3 rd_k4 = psmul(dt, paccel<4>(padd(ro, ro_k3), s, G));
    const p3 sro = padd(padd2(padd2(ro_k1, ro_k2), ro_k3), ro_k4);
    const p3 srd = padd(padd2(padd2(rd_k1, rd_k2), rd_k3), rd_k4);
    G.amin6 = XOps<true>::absmin3(XOps<true>::absmin3(sro.xy.x, sro.xy.y, sro.z), srd.xy.x, srd.xy.y, srd.z);
    const p3 dro = pdiv6(sro), drd = pdiv6(srd);
    G.bad |= !(G.amin6 >= crm::DIV_N_MIN) & (dt != 0.0f);
    G.bad |= G.kmin < crm::KEY_ACC_MIN;
    G.bad |= !(G.amin >= crm::ACC_N_MIN);
    if constexpr (!CO) G.bad |= !(fabsf(s) <= 0x1p30f);
    const float ntr = travelled + dt;
    out.s = s;
    out.outside = CO ? 1u : (not_out ? in.outside : 1u);
    out.ro = unpk(padd(ro, dro));
    out.rd = unpk(padd(rd, drd));
    out.travelled = ntr;
    out.n_rk = n_rk + 1u;
    const bool escape = ntr > a.max_dist;
    fate = escape ? (uint32_t)BH_FATE_ESCAPE : (uint32_t)BH_FATE_CAP;
    return escape | (n_rk + 1u >= a.max_iters);
}
#endif

#if !BH_FAST
// Iteration 0 of a frame whose first-step record is valid (bh_common.hpp FirstStep; bh_host.cpp, first_step_record),
// from `in` -- the ray at the camera: ro = ro0, travelled 0, n_rk 0 -- into `out`.  Every ray of the frame starts at
// ro0 (:363), so what step_bf forms from ro alone before the RK update is one number per frame and the host holds
// it: dt = fs.dt0, and k1's denominator Q = fs.Q0 with RN(1 / Q) = fs.rq0 (rcp_refined's value for a normal Q).  The
// host's gate rules out every exit of this iteration (blackout, surface, escape, cap: no fate) and every guard whose
// operands are the frame's (Q's range, dt's); what is left is step_bf's RK update in its XOps<true> form -- the same
// ops in the same order -- with its per-lane guards.  Returns their verdict: true when an operand of this lane left
// a core's domain, and `out` is then not to be used -- the wave runs iteration 0 by the loop's own step instead.
__device__ __forceinline__ bool step_first(const RayState& in, RayState& out, const FirstStep& fs) {
    XOps<true> X;
    const v3 ro = in.ro, rd = in.rd;
    const float s = in.s, dt = fs.dt0;
    // k1 = rd_derivative(ro0): accel_qs<1> with the frame's reciprocal
    const float nx = s * ro.x, ny = s * ro.y, nz = s * ro.z;
    X.kmin = crm::kmin3(crm::key(nx), crm::key(ny), crm::key(nz));
    const crm::Rcp R{fs.Q0, fs.rq0};
    const v3 ro_k1 = smul(dt, rd);
    const v3 rd_k1 = smul(dt, mk(crm::div_core(nx, R), crm::div_core(ny, R), crm::div_core(nz, R)));
    const v3 ro_k2 = smul(dt, X.rd_half(rd, rd_k1));
    const v3 rd_k2 = smul(dt, X.template accel<2>(X.ro_half(ro, ro_k1), s));
    const v3 ro_k3 = smul(dt, X.rd_half(rd, rd_k2));
    const v3 rd_k3 = smul(dt, X.template accel<3>(X.ro_half(ro, ro_k2), s));
    const v3 ro_k4 = smul(dt, add(rd, rd_k3));
    const v3 rd_k4 = smul(dt, X.template accel<4>(add(ro, ro_k3), s));
    const v3 sro = add(X.add2(X.add2(ro_k1, ro_k2), ro_k3), ro_k4);
    const v3 srd = add(X.add2(X.add2(rd_k1, rd_k2), rd_k3), rd_k4);
    const v3 dro = X.template div6<0>(sro);
    const v3 drd = X.template div6<1>(srd);
    X.bad |= X.kmin < crm::KEY_ACC_MIN;
    X.bad |= !(X.amin >= crm::ACC_N_MIN);
    X.bad |= !(X.amin6 >= crm::DIV_N_MIN);  // dt0 != 0
    X.bad |= !(fabsf(s) <= 0x1p30f);
    out.ro = add(ro, dro);
    out.rd = add(rd, drd);
    out.travelled = in.travelled + dt;
    out.s = s;
    out.n_rk = in.n_rk + 1u;
    out.outside = 1u;  // r0 > 1
    return X.bad;
}
#endif

// One iteration for one ray from `in` into `out` (step_bf<true> contract: `out` is not written for
// fates before the RK update), with the exact mode's guarded fast path and its rare IEEE re-run.
// UNI: step_bf's contract for the ping-pong loop (*end).  K1F: the guarded pass checks k1's numerators on the float
// chain (XOps), for the loop whose steps follow a peeled iteration 0.
template <uint32_t SF = SF_DYN, bool UNI = false, bool TINY = false, bool K1F = false>
__device__ __forceinline__ bool march_step_io(const MarchArgs& a, const Frame& f, const RayState& in, RayState& out,
                                              uint32_t& fate, uint32_t it = 0u, StepEnd* end = nullptr) {
#if BH_FAST
    FOps X;
    return step_bf<true, FOps, SF, UNI>(a, f, in, out, X, fate, it, end);
#else
    using GOps = XOps<true, K1F>;
    GOps X;
#ifdef BH_DIAG_SLOW
    if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true)))
        atomicAdd(&g_diag_all_wave_steps, 1u);
#endif
    bool done = step_bf<true, GOps, SF, UNI, TINY>(a, f, in, out, X, fate, it, end);
#ifdef BH_DIAG_SLOW
    const uint64_t badm = __builtin_amdgcn_ballot_w64(X.bad);
    if (badm != 0ull && (threadIdx.x & 63u) == 0u) {
        atomicAdd(&g_diag_slow_wave_steps, 1u);
        atomicAdd(&g_diag_slow_lane_steps, (uint32_t)__popcll(badm));
    }
#endif
    // rare IEEE re-run: a divergent `if` on the guard's lane mask (s_and_saveexec + execz skip; a
    // ballot here costs a v_cndmask + v_cmp per step to materialise the mask)
    if (__builtin_expect(X.bad, 0)) {
        XOps<false> Y;
        done = step_bf<true, XOps<false>, SF, UNI>(a, f, in, out, Y, fate, it, end);
    }
    return done;
#endif
}

// One iteration for one ray in place (persistent schedule; TINY: the tail's scalar step): BH_FATE_* if the ray
// terminates, else 0xFF.
template <uint32_t SF = SF_DYN, bool TINY = false>
__device__ __forceinline__ uint32_t march_step(const MarchArgs& a, const Frame& f, RayState& st) {
    // t = st / st = t rather than a select on the fate: the copies fill the tail waves' dependency
    // stalls (a select form measured 9 % slower at cap 1000, A/B r01)
    RayState t = st;  // lanes that leave before the RK update keep `st` (n_rk is what they need)
    uint32_t fate;
    const bool done = march_step_io<SF, false, TINY>(a, f, st, t, fate);
    st = t;
    return done ? fate : 0xFFu;
}

// One iteration of a tail wave (the tile schedule's cycle watch), in place: BH_FATE_* if the ray
// terminates, else 0xFF.  The latency build of the exact kernels (BH_TAIL_PACKED, the -DBH_LAT=1 units)
// runs the packed step, with the same rare IEEE re-run: a lone tail wave's step 0.89 -> 0.79 us, config
// 5 (one frame, cap 1000) 0.824 -> 0.734 ms.  The issue-order build keeps the scalar step: in
// multi-frame launches the tail waves share their SIMDs with other frames' bulk, where a packed op
// costs more than two scalar ones, and the packed tail measured 0.4 % slower there (A/B r02,
// profiles/r02/ab_tail.log).
template <uint32_t SF = SF_DYN>
__device__ __forceinline__ uint32_t march_step_tail(const MarchArgs& a, const Frame& f, RayState& st) {
#if BH_FAST || !BH_TAIL_PACKED
    return march_step<SF, true>(a, f, st);
#else
    RayState t = st;
    uint32_t fate;
    PkGuard G;
    bool done = step_tail<SF>(a, f, st, t, G, fate);
    if (__builtin_expect(G.bad, 0)) {
        XOps<false> Y;
        done = step_bf<true, XOps<false>, SF>(a, f, st, t, Y, fate);
    }
    st = t;
    return done ? fate : 0xFFu;
#endif
}

// One iteration for two independent rays of the same lane (pair schedule).  Dead rays (alive_k
// false) are computed on their frozen state and discarded, so the two iterations stay one block.
__device__ __forceinline__ void march_step2(const MarchArgs& a, const Frame& f, RayState& s0, RayState& s1,
                                            bool& alive0, bool& alive1, uint32_t& fate0, uint32_t& fate1) {
    RayState t0, t1;
#if BH_FAST
    FOps X0, X1;
    uint32_t f0, f1;
    const bool d0 = step_bf<false>(a, f, s0, t0, X0, f0);
    const bool d1 = step_bf<false>(a, f, s1, t1, X1, f1);
#else
    XOps<true> X0, X1;
    uint32_t f0, f1;
    bool d0 = step_bf<false>(a, f, s0, t0, X0, f0);
    bool d1 = step_bf<false>(a, f, s1, t1, X1, f1);
    const bool bad0 = X0.bad & alive0, bad1 = X1.bad & alive1;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad0 | bad1) != 0ull, 0)) {   // rare IEEE re-runs
        if (bad0) { XOps<false> Y; d0 = step_bf<false>(a, f, s0, t0, Y, f0); }
        if (bad1) { XOps<false> Y; d1 = step_bf<false>(a, f, s1, t1, Y, f1); }
    }
#endif
    // selects, not branches
    s0.ro = sel(alive0, t0.ro, s0.ro); s0.rd = sel(alive0, t0.rd, s0.rd);
    s0.travelled = alive0 ? t0.travelled : s0.travelled; s0.n_rk = alive0 ? t0.n_rk : s0.n_rk;
    s0.outside = alive0 ? t0.outside : s0.outside;
    s1.ro = sel(alive1, t1.ro, s1.ro); s1.rd = sel(alive1, t1.rd, s1.rd);
    s1.travelled = alive1 ? t1.travelled : s1.travelled; s1.n_rk = alive1 ? t1.n_rk : s1.n_rk;
    s1.outside = alive1 ? t1.outside : s1.outside;
    const bool e0 = alive0 & d0, e1 = alive1 & d1;
    fate0 = e0 ? f0 : fate0;
    fate1 = e1 ? f1 : fate1;
    alive0 = alive0 & !e0;
    alive1 = alive1 & !e1;
}

}  // namespace BH_NS
}  // namespace bh
