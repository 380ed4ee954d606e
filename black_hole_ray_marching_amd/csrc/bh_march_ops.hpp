// bh_march_ops.hpp -- the march's arithmetic: the vector type v3 and its helpers, the scene constants, and the op
// set of each math mode that the step (bh_march_step.hpp) is written against: FOps (fast) or XOps<CR> (exact).
// Needs bh_common.hpp (the scene flags) and bh_crmath.hpp (the correctly rounded cores).  Like every
// bh_march_*.hpp it is a part of bh_march.hpp, which the unit includes after defining BH_FAST and BH_NS.
#pragma once
#include <hip/hip_runtime.h>

#include "bh_common.hpp"
#include "bh_crmath.hpp"

namespace bh {
namespace BH_NS {

struct v3 { float x, y, z; };

__device__ __forceinline__ v3 mk(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ v3 add(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ v3 smul(float s, v3 a) { return mk(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ v3 muls(v3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// per-component select (an aggregate `c ? a : b` keeps the struct in scratch memory)
__device__ __forceinline__ v3 sel(bool c, v3 a, v3 b) { return mk(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
__device__ __forceinline__ v3 cross(v3 a, v3 b) {
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

#if BH_FAST
__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ v3 normalize(v3 a) { return muls(a, rsq(dot(a, a))); }
#else
__device__ __forceinline__ float len(v3 a) { return __builtin_sqrtf(dot(a, a)); }  // correctly rounded
__device__ __forceinline__ v3 divs(v3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ v3 normalize(v3 a) { return divs(a, len(a)); }

// The per-ray set-up and shading ops on the cheap correctly rounded cores of bh_crmath.hpp (the same
// bits as the IEEE forms above, proofs at each).
//
// normalize(v) = v / sqrt(dot(v, v)): exact when q = dot(v, v) is in [2^-80, 2^120] (inside the sqrt
// core's domain, and then the length is in the division core's [2^-40, 2^60], which also bounds
// every |v_i| <= 2^60) and every component is 0 or >= 2^-60 in magnitude.  Otherwise the lanes
// concerned take the IEEE form (a wave-uniform branch; never seen on real frames).
__device__ __forceinline__ v3 normalize_x(v3 v) {
    const float q = dot(v, v);
    const float l = crm::sqrt_core(q);
    const crm::Rcp R = crm::rcp_refined(l);
    const v3 n = mk(crm::div_core(v.x, R), crm::div_core(v.y, R), crm::div_core(v.z, R));
    const bool bad = !(q >= 0x1p-80f && q <= 0x1p120f) |
                     (crm::kmin3(crm::key(v.x), crm::key(v.y), crm::key(v.z)) < crm::KEY_MIN);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0ull, 0)) {
        if (bad) return normalize(v);
    }
    return n;
}
// c * sqrt(c) for a bilinear sky sample c: c is +0 or in [2^-60, 1] (texels decode to 0 or
// >= 3.0e-4, the bilinear weights are 0 or >= 2^-24: two weight products keep c >= 1.8e-18), so
// the sqrt core is exact for every c > 0 and c = +0 gives +0 as c * sqrt(c) does.
__device__ __forceinline__ float pow15_x(float c) { return c > 0.0f ? c * crm::sqrt_core(c) : c; }
#endif

constexpr float MIN_DIST = 0.001f;        // :80
constexpr float TWO_PI = 6.28318530718f;  // :82
constexpr float ONE_PI = 3.14159265359f;  // :83

// Ops supplies sqrt / sdf / rd_derivative / x/6 for the math mode:
//   exact: XOps<true>  correctly rounded cores + domain guard (bh_crmath.hpp);
//          XOps<false> plain IEEE ops (the guard's fallback);  both = the oracle's arithmetic;
//   fast:  FOps        hardware rsq / sqrt, FMA contraction.

// sdf (:119-123) from its two terms: a disabled term is left out, as the WGSL leaves it out -- not taken as +inf,
// since fminf(NaN, +inf) == +inf would drop the enabled term's NaN with it (a ray whose position is NaN)
__device__ __forceinline__ float sdf_of_terms(uint32_t flags, float disc, float m) {
    if (!(flags & BH_SCENE_MARKERS)) return (flags & BH_SCENE_DISC) ? disc : __builtin_inff();
    return (flags & BH_SCENE_DISC) ? fminf(disc, m) : m;
}

#if !BH_FAST
// fminf(a, b) for operands that are never signalling NaNs -- results of arithmetic ops, or +inf: the one v_min_f32,
// without the v_max_f32 x, x, x that fminf spends on quieting each operand it cannot trace to an op (a value merged
// from two arms).  The same result for every such pair, a quiet NaN operand dropped as fminf drops it.
// (-0.5 % on the headline alone, three times just below the rule; kept with the K1F loop)
__device__ __forceinline__ float fmin_quiet(float a, float b) {
    float m;
    asm("v_min_f32 %0, %1, %2" : "=v"(m) : "v"(a), "v"(b));
    return m;
}
// sdf_of_terms on such operands (the per-term arm of step_bf: each term a root's distance or +inf)
__device__ __forceinline__ float sdf_of_terms_quiet(uint32_t flags, float disc, float m) {
    if (!(flags & BH_SCENE_MARKERS)) return (flags & BH_SCENE_DISC) ? disc : __builtin_inff();
    return (flags & BH_SCENE_DISC) ? fmin_quiet(disc, m) : m;
}
#endif

#if BH_FAST
struct FOps {
    bool bad = false;  // no guard in fast mode
    __device__ __forceinline__ float sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }  // raw v_sqrt_f32
    template <int K>
    __device__ __forceinline__ v3 div6(v3 x) { return muls(x, 1.0f / 6.0f); }
    __device__ __forceinline__ v3 add2(v3 a, v3 b) {  // a + 2b
        return mk(__builtin_fmaf(2.0f, b.x, a.x), __builtin_fmaf(2.0f, b.y, a.y), __builtin_fmaf(2.0f, b.z, a.z));
    }
    __device__ __forceinline__ v3 ro_half(v3 ro, v3 k) {  // ro + 0.5 k
        return mk(__builtin_fmaf(0.5f, k.x, ro.x), __builtin_fmaf(0.5f, k.y, ro.y), __builtin_fmaf(0.5f, k.z, ro.z));
    }
    __device__ __forceinline__ v3 rd_half(v3 rd, v3 k) { return ro_half(rd, k); }
    template <int K>
    __device__ __forceinline__ v3 accel_qs(v3 p, float s, float q, float) {
        const float iq = rsq(q), iq2 = iq * iq;
        return muls(p, s * (iq2 * iq2 * iq));
    }
    template <int K>
    __device__ __forceinline__ v3 accel(v3 p, float s) { return accel_qs<K>(p, s, dot(p, p), 0.0f); }
    __device__ __forceinline__ void sq_args(float, float) {}
    __device__ __forceinline__ void sq_arg(float) {}
    __device__ __forceinline__ void sdf_args(v3, float&, float&, float&) {}
    __device__ __forceinline__ float sdf_from(v3 p, float rs, uint32_t flags, float, float) {
        const float rho = __builtin_amdgcn_sqrtf(p.x * p.x + p.z * p.z);
        const float disc = fmaxf(fmaxf(rho - 6.0f * rs, -(rho - 3.0f * rs)), fabsf(p.y) - 0.02f);
        // min of the four sphere SDFs == sqrt(min of squared distances) - 0.5 (sqrt is monotone)
        const float ay = fabsf(p.y) - 10.0f, ax = fabsf(p.x) - 10.0f, dz = p.z + 10.0f;
        const float m = __builtin_amdgcn_sqrtf(fminf(p.x * p.x + ay * ay, ax * ax + p.y * p.y) + dz * dz) - 0.5f;
        return fminf((flags & BH_SCENE_DISC) ? disc : __builtin_inff(),
                     (flags & BH_SCENE_MARKERS) ? m : __builtin_inff());
    }
};
#else
// Exact mode.  The arithmetic is the normative op sequence of oracle/bh_oracle.c: every rounding
// the same as IEEE f32 evaluated in WGSL source order.  CR = true evaluates the divisions and
// square roots with the cheap correctly rounded cores of bh_crmath.hpp and raises `bad` for any
// operand outside their proven domain; CR = false is plain IEEE ops (hipcc's expansions).  Both
// produce identical bits wherever `bad` stays false.
// K1F (with CR): the form of the loop behind the peeled first step (march_ray, PEEL), see below.
template <bool CR, bool K1F = false>
struct XOps {
    static constexpr bool kCR = CR;
    static constexpr bool kK1F = CR && K1F;
    bool bad = false;
    // Numerator domain of the division cores: 0 or >= DIV_N_MIN in magnitude, held to the stricter
    // ACC_N_MIN for the acceleration numerators (rd_half's premise).  Zeros are legal (the
    // cores are exact for them) and occur in two places:
    //  * k1's numerators s*ro at a ray's iteration 0: camera-A rays start on two coordinate planes.
    //    Checked through crm::key (zeros map high, tiny values low): one v_lshl_add per value +
    //    v_min3_u32 + its compare.  K1F -- the loop that follows the peeled first step, whose steps
    //    are iterations >= 1 unless the wave could not take the record -- drops the key: k1's
    //    numerators start the float chain `amin` (kmin is unused) and a zero takes the IEEE path
    //    like any other stage's, -3 VALU per step.  The float test fires wherever the key test fires
    //    (0 < |n| < ACC_N_MIN) and on zeros besides, and the re-run is exact for any input, so
    //    the bytes are the same.  What it costs: a ray with a component of ro and rd exactly zero --
    //    in a coordinate plane for good: the centre column of an odd-width frame from camera A, a
    //    ray map's row with d.y = 0 -- re-runs every step of that loop;
    //  * the x/6 numerators when dt == 0 exactly (a ray frozen on the photon-sphere marker): all RK
    //    sums are then +-0.
    // Everywhere else a zero numerator needs an exact cancellation, so those are checked as a float
    // min |n| (one v_min3_f32 with |.| modifiers per three values) and a zero just takes the IEEE
    // path; the x/6 check is waived when dt == 0.  (min |n| everywhere: measured 7 % slower, frozen
    // rays fell back at every step.)
    // Each accumulator is one running chain started by its first value (an explicit +inf start is
    // not folded away, since fminf(inf, NaN) is not NaN), so consecutive values pair up into
    // v_min3_f32: -5 VALU per step, 0.6 % (A/B r01).  (Pooling the denominators' range checks into
    // one min/max over the squared lengths r^2, |ro - cps|^2 and the k-point dot products -- a range
    // of q that implies Q's -- is 5 VALU fewer again but measured 12 % slower at cap 64 and 512 with
    // the same IEEE re-run count: the compiler then interleaves k3's and k4's rsq/rcp chains; the
    // max-ilp and iterative-ilp scheduling strategies did not recover it.  Round 3, with machine
    // scheduling off: one unsigned v_min3_u32 / v_max3_u32 pool over the bit patterns of r^2, rho^2,
    // the marker and photon-sphere arguments and the k-point q's, range [2^-16, 2^24] (implies every
    // root's and Q's domain), 286 -> 280 VALU per step and the same re-run count
    // (tools/diag_slow.py), measured 3.5 % slower on the headline and 11 % on cap 1000 at one frame
    // per launch (packed tail); a float pool the same; profiles/r03/ab_pool/.  Round 25, issue-bound
    // kernel: the three stage denominators Q2..Q4 alone as one v_min3_u32 / v_max3_u32 pool over their
    // bit patterns, two unsigned compares -- exactly div_d_bad of each, 4 VALU for 6 -- measured
    // 0.7 % slower with the test beside k4's v_rcp (+2 VGPRs) and 2.2 % slower with it at the block's
    // end; profiles/r25/step_guards/ab.txt.  Each Q keeps its two compares beside its producer.)
    uint32_t kmin;  // k1 numerators (keys; not K1F)
    float amin;     // k2..k4 numerators (K1F: k1..k4)
    float amin6;    // x/6 numerators
    __device__ __forceinline__ static float absmin3(float m, float x, float y, float z) {
        return fminf(fminf(fminf(m, fabsf(x)), fabsf(y)), fabsf(z));
    }
    __device__ __forceinline__ static float absmin3(float x, float y, float z) {
        return fminf(fminf(fabsf(x), fabsf(y)), fabsf(z));
    }
    // Square roots.  The core is exact for x in [SQRT_MIN, FLT_MAX]; outside that the caller must
    // raise `bad`.  Which check covers which root (one v_cmp per bound, so they are pooled):
    //  * r = |ro| and the pow(q, 2.5) roots of rd_derivative: x < 2^-96 makes q*q underflow to 0 and
    //    x = inf makes it inf, so the denominator Q = (q*q)*sqrt(q) is 0, inf or NaN and
    //    div_d_bad(Q) raises `bad` already.  The step's exit tests (before k1) compare r^2, not r
    //    (step_bf), so a lane that leaves early never reads r;
    //  * rho (disc) and the marker distance: one shared range check on the min and max of their
    //    arguments (sq_args; a flag-disabled term can only cause a spare re-run); the photon-sphere
    //    distance (sq_arg, evaluated after the step's early exits).
    __device__ __forceinline__ float sqrt(float x) {
        if constexpr (CR) return crm::sqrt_core(x);
        else return __builtin_sqrtf(x);
    }
    __device__ __forceinline__ void sq_args(float a, float b) {
        if constexpr (CR) bad |= crm::sqrt_bad2(a, b);
    }
    __device__ __forceinline__ void sq_arg(float a) {
        if constexpr (CR) bad |= crm::sqrt_bad(a);
    }
    template <int K>  // K = 0 for the first call of a step, 1 for the second
    __device__ __forceinline__ v3 div6(v3 x) {
        if constexpr (CR) {
            amin6 = (K == 0) ? absmin3(x.x, x.y, x.z) : absmin3(amin6, x.x, x.y, x.z);
            return mk(crm::div6(x.x), crm::div6(x.y), crm::div6(x.z));
        } else {
            return mk(x.x / 6.0f, x.y / 6.0f, x.z / 6.0f);
        }
    }
    // a + 2b (the RK4 weights): 2b is exact, so the FMA rounds once exactly like the two IEEE adds
    // whenever 2b does not overflow, which the guarded domain rules out (|p| <= 2^12, dt <= 2^13)
    __device__ __forceinline__ v3 add2(v3 a, v3 b) {
        if constexpr (CR) {
            return mk(__builtin_fmaf(2.0f, b.x, a.x), __builtin_fmaf(2.0f, b.y, a.y), __builtin_fmaf(2.0f, b.z, a.z));
        } else {
            return add(a, smul(2.0f, b));
        }
    }
    // ro + 0.5 k, the RK stage positions of k2 and k3 (:140, :143).  CR: fma(0.5, k, ro), one op per
    // component instead of two, and the same bits on every step whose guard stays clear:
    //  * where 0.5 k is exact (|k| >= 2^-125) both forms round ro + 0.5 k once;
    //  * else |0.5 k| < 2^-126: when |ro_i| >= 2^-100 it is below half an ulp of ro_i and both give ro_i;
    //    when ro_i is 0 or smaller, the stage position is 0 or below 2^-99, so this stage's numerator
    //    s * p_i (|s| <= 2^30 on a clear step) is 0 or below ACC_N_MIN and `amin` raises the guard: the
    //    step re-runs in IEEE ops.
    __device__ __forceinline__ v3 ro_half(v3 ro, v3 k) {
        if constexpr (CR) {
            return mk(__builtin_fmaf(0.5f, k.x, ro.x), __builtin_fmaf(0.5f, k.y, ro.y), __builtin_fmaf(0.5f, k.z, ro.z));
        } else {
            return add(ro, smul(0.5f, k));
        }
    }
    // rd + 0.5 k, the RK stage directions of ro_k2 and ro_k3 (:139, :142), k = rd_k1 or rd_k2 = dt * a.
    // CR: fma(0.5, k, rd), exact on every clear step: the acceleration numerators are 0 or >= 2^-40
    // (ACC_N_MIN, and non-zero for k2) and Q <= 2^60, so a_i is 0 or >= 2^-100, and the guard holds dt
    // to 0 or |dt| >= 2^-25 (step_bf), so k_i is 0 or >= 2^-125: 0.5 k is exact and both forms round the
    // same sum once.
    __device__ __forceinline__ v3 rd_half(v3 rd, v3 k) {
        if constexpr (CR) {
            return mk(__builtin_fmaf(0.5f, k.x, rd.x), __builtin_fmaf(0.5f, k.y, rd.y), __builtin_fmaf(0.5f, k.z, rd.z));
        } else {
            return add(rd, smul(0.5f, k));
        }
    }
    // rd_derivative (:125-127): (s * p) / pow(dot(p,p), 2.5), pow(q, 2.5) := (q*q)*sqrt(q);
    // q and sqrt(q) passed in when already known (k1: q = r^2, sqrt(q) = r).
    // K = 1..4: the RK stage (k1's numerators may be zeros unless K1F, see above)
    // (a v_rcp of Q seeds RN(1/Q), not the root's own v_rsq: see the top of the file)
    template <int K>
    __device__ __forceinline__ v3 accel_qs(v3 p, float s, float q, float sq) {
        // normative pow(q, 2.5) (oracle/bh_oracle.c header): (q * q) * sqrt(q), three correctly rounded f32 ops
        const float Q = (q * q) * sq;
        const float nx = s * p.x, ny = s * p.y, nz = s * p.z;
        if constexpr (CR) {
            bad |= crm::div_d_bad(Q);
            if constexpr (K == 1 && !kK1F) kmin = crm::kmin3(crm::key(nx), crm::key(ny), crm::key(nz));
            else if constexpr (K == (kK1F ? 1 : 2)) amin = absmin3(nx, ny, nz);
            else amin = absmin3(amin, nx, ny, nz);
            const crm::Rcp R = crm::rcp_refined(Q);
            return mk(crm::div_core(nx, R), crm::div_core(ny, R), crm::div_core(nz, R));
        } else {
            return mk(nx / Q, ny / Q, nz / Q);
        }
    }
    template <int K>
    __device__ __forceinline__ v3 accel(v3 p, float s) {
        const float q = dot(p, p);
        return accel_qs<K>(p, s, q, sqrt(q));
    }
    // sdf (:119-123); markers: min(sqrt(qi) - 0.5) == sqrt(min qi) - 0.5 exactly (monotone ops)
    // sdf_args: the arguments of its two roots (rho^2, the markers' qm) and y*y; sdf_from: the rest
    __device__ __forceinline__ void sdf_args(v3 p, float& rho2, float& yy, float& qm) {
        rho2 = p.x * p.x + p.z * p.z;
        // The four sphere arguments are q1,2 = (xx + (+-10 - y)^2) + zz and q3,4 = ((+-10 - x)^2 + yy)
        // + zz.  Of each pair only the sphere on the point's side can be the minimum, and its
        // argument is computed from t = RN(10 - |y|) (resp. |x|): RN(-10 - y) = -RN(10 + y) and
        // |10 - y| <= 10 + y for y >= 0 (mirrored for y < 0), and every later op (square, sums) is
        // monotone in |t|, so the rounded q of the near sphere is <= the far one's and equals
        // (xx + t*t) + zz bit for bit.  min(q1..q4) == min(qy, qx): 11 ops instead of 20
        // (tests/test_oracle.py::test_marker_pair_reduction checks the identity).
        const float xx = p.x * p.x;
        yy = p.y * p.y;
        const float dz = -10.0f - p.z, zz = dz * dz;
        const float ty = 10.0f - fabsf(p.y), tx = 10.0f - fabsf(p.x);
        const float qy = (xx + ty * ty) + zz, qx = (tx * tx + yy) + zz;
        qm = fminf(qy, qx);
    }
    // the disc and marker terms of sdf_from one by one (the per-term root-free step)
    __device__ __forceinline__ float disc_from(v3 p, float rs, float rho2) {
        const float rho = sqrt(rho2);
        return fmaxf(fmaxf(rho - 6.0f * rs, -(rho - 3.0f * rs)), fabsf(p.y - 0.0f) - 0.02f);
    }
    __device__ __forceinline__ float mark_from(float qm) { return sqrt(qm) - 0.5f; }
    __device__ __forceinline__ float sdf_from(v3 p, float rs, uint32_t flags, float rho2, float qm) {
        const float rho = sqrt(rho2);
        const float disc = fmaxf(fmaxf(rho - 6.0f * rs, -(rho - 3.0f * rs)), fabsf(p.y - 0.0f) - 0.02f);
        const float m = sqrt(qm) - 0.5f;
        return sdf_of_terms(flags, disc, m);
    }
};
#endif

}  // namespace BH_NS
}  // namespace bh
