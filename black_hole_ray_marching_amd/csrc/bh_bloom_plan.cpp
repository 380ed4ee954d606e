// bh_bloom_plan.cpp -- the host side of the bloom's kernels (bh_bloom.hip): the plan builders, which replay the
// kernels' texcoord / tap / sample_coord arithmetic in IEEE f32 (identical on the host: this unit is compiled
// without contraction, and the kernels' div_core == IEEE division in its domain), the host-side bound checks of
// every launch form, and the dry run of bh_bloom_check.  Plain C++: no device code and no HIP call, so that a host
// compiler and its sanitizers reach all of it (tests/test_bloom_bounds.py links it with tools/bloom_fixup_addr.cpp).
#include "bh_bloom_plan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace bh {
namespace bloom {
namespace {
float h_sample_coord(float u, uint32_t n) {
    const float t = u * (float)n - 0.5f;
    return fminf(fmaxf(t, -1.0f), (float)n);
}
float h_texcoord(uint32_t i, uint32_t n) { return ((float)i + 0.5f) / (float)n; }
// Taps::du / dv on the host: (hx * m) * 3 with hx = 0.5 / res
float h_tap(uint32_t res, int axis, int i) { return ((0.5f / (float)res) * (float)tap_m(axis, i)) * 3.0f; }
float h_tap_min(uint32_t res, int axis) { return h_tap(res, axis, axis ? 6 : 0); }
float h_tap_max(uint32_t res, int axis) { return h_tap(res, axis, axis ? 2 : 4); }
int32_t h_floor(float t) { return (int32_t)floorf(t); }

// the point-tap proof of one axis: every pixel's coordinate integral (or clamped)
bool axis_point(uint32_t on, uint32_t tn, float d) {
    for (uint32_t x = 0; x < on; ++x) {
        const float t = h_sample_coord(((float)x + 0.5f) / (float)on + d, tn);
        if (t != floorf(t)) return false;
    }
    return true;
}

// One axis of tap i (offset d in texcoord units) over an on-pixel pass of an tn-texel texture: the
// integer offset o and half flag f with u*tn - 0.5 == x + o + f/2 exactly for every x, else false.
bool axis_plan(uint32_t on, uint32_t tn, float d, int32_t* o, bool* half) {
    const float t0 = ((0.5f / (float)on) + d) * (float)tn - 0.5f;
    const float f0 = floorf(t0);
    if (!(t0 - f0 == 0.0f || t0 - f0 == 0.5f) || !(fabsf(f0) < 4096.0f)) return false;
    *o = (int32_t)f0;
    *half = t0 != f0;
    const float fr = t0 - f0;
    for (uint32_t x = 0; x < on; ++x) {
        const float t = (((float)x + 0.5f) / (float)on + d) * (float)tn - 0.5f;
        if (t != (float)((int32_t)x + *o) + fr) return false;
    }
    return true;
}

// One axis of tap i (offset d in texcoord units) of a 2:1 pass (on == 2 tn): per pixel parity p the
// integer o[p] and weight f[p] with floor(t) == (x >> 1) + o[p] and t - floor(t) == f[p] for every x,
// t = u*tn - 0.5 the sampler's unclamped coordinate; [lo, hi] = the pixels whose two texels floor(t),
// floor(t) + 1 both lie in [0, tn) (there the sampler's clamps change nothing).  False if not so.
bool axis_plan2(uint32_t on, uint32_t tn, float d, int32_t o[2], float f[2], int32_t* lo, int32_t* hi) {
    if (on != 2u * tn || tn < 2u) return false;
    bool seen[2] = {false, false};
    int32_t ilo = INT_MAX, ihi = -1, count = 0;
    for (uint32_t x = 0; x < on; ++x) {
        const float t = (((float)x + 0.5f) / (float)on + d) * (float)tn - 0.5f;
        const float fl = floorf(t);
        if (!(fabsf(fl) < 16777216.0f)) return false;
        const uint32_t p = x & 1u;
        const int32_t oo = (int32_t)fl - (int32_t)(x >> 1);
        const float ff = t - fl;
        if (!seen[p]) {
            o[p] = oo;
            f[p] = ff;
            seen[p] = true;
        } else if (oo != o[p] || std::memcmp(&ff, &f[p], sizeof ff) != 0) {
            return false;
        }
        if (fl >= 0.0f && fl + 1.0f <= (float)tn - 1.0f) {
            ilo = std::min(ilo, (int32_t)x);
            ihi = std::max(ihi, (int32_t)x);
            ++count;
        }
    }
    if (count != 0 && count != ihi - ilo + 1) return false;  // t is monotone: an interval
    *lo = count ? ilo : 0;
    *hi = count ? ihi : -1;
    return true;
}

// The last 16 plans of one kind that this thread built, by shape (a bloom chain uses a few)
template <class Plan, class Build>
Plan cached_plan(const PlanKey& key, Build build) {
    static thread_local PlanKey keys[16];
    static thread_local Plan plans[16];
    static thread_local uint32_t n = 0, next = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (keys[i] == key) return plans[i];
    const Plan P = build();
    keys[next] = key;
    plans[next] = P;
    next = (next + 1u) % 16u;
    n = n < 16u ? n + 1u : 16u;
    return P;
}
}  // namespace

// The TapPlan of an 8-tap pass (see TapPlan); valid == 0 when a tap's coordinate is not x + o + {0, 1/2} for every x
TapPlan tap_plan(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry) {
    return cached_plan<TapPlan>({ow, oh, tw, th, rx, ry}, [&] {
        TapPlan P{};
        P.valid = 1u;
        P.lo_x = P.lo_y = 1 << 20;
        P.hi_x = P.hi_y = -(1 << 20);
        for (int i = 0; i < 8; ++i) {
            bool fx, fy;
            if (!axis_plan(ow, tw, h_tap(rx, 0, i), &P.ox[i], &fx) || !axis_plan(oh, th, h_tap(ry, 1, i), &P.oy[i], &fy))
                return TapPlan{};
            P.hx |= (uint32_t)fx << i;
            P.hy |= (uint32_t)fy << i;
            P.lo_x = std::min(P.lo_x, P.ox[i]); P.hi_x = std::max(P.hi_x, P.ox[i] + (int32_t)fx);
            P.lo_y = std::min(P.lo_y, P.oy[i]); P.hi_y = std::max(P.hi_y, P.oy[i] + (int32_t)fy);
        }
        return P;
    });
}

// The Up2Plan of an up pass (see Up2Plan); valid == 0 when the pass is not 2:1 or a tap's offset or weight varies
// within a parity class.
Up2Plan up2_plan(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry) {
    return cached_plan<Up2Plan>({ow, oh, tw, th, rx, ry}, [&] {
        Up2Plan P{};
        P.valid = 1u;
        P.x_lo = P.y_lo = 0;
        P.x_hi = (int32_t)ow - 1;
        P.y_hi = (int32_t)oh - 1;
        for (int i = 0; i < 8; ++i) {
            int32_t ox[2], oy[2], xl, xh, yl, yh;
            float fx[2], fy[2];
            if (!axis_plan2(ow, tw, h_tap(rx, 0, i), ox, fx, &xl, &xh) || !axis_plan2(oh, th, h_tap(ry, 1, i), oy, fy, &yl, &yh))
                return Up2Plan{};
            for (int p = 0; p < 2; ++p) {
                P.ox[p][i] = ox[p]; P.fx[p][i] = fx[p];
                P.oy[p][i] = oy[p]; P.fy[p][i] = fy[p];
            }
            if (ox[1] - ox[0] < 0 || ox[1] - ox[0] > 1 || oy[1] - oy[0] < 0 || oy[1] - oy[0] > 1) return Up2Plan{};  // the quad's 3x3
            P.x_lo = std::max(P.x_lo, xl); P.x_hi = std::min(P.x_hi, xh);
            P.y_lo = std::max(P.y_lo, yl); P.y_hi = std::min(P.y_hi, yh);
        }
        return P;
    });
}

// The standard plan (see quad_tap_std) a runtime plan equals, or 0: A = 12 or 3 for a 2:1 up pass, A =
// 12 or 48 for a same-size TapPlan pass.  BH_BLOOM_NO_STD (A/B) disables them.
static const bool g_no_std = std::getenv("BH_BLOOM_NO_STD") != nullptr;
int std_up2_plan(const Up2Plan& P) {
    if (!P.valid || g_no_std) return 0;
    for (int A : {12, 3}) {
        bool eq = true;
        for (int i = 0; i < 8 && eq; ++i)
            for (int p = 0; p < 2 && eq; ++p) {
                const int vx = A * tap_m(0, i) + (p ? 2 : -2), vy = A * tap_m(1, i) + (p ? 2 : -2);
                eq = P.ox[p][i] == fdiv8(vx) && P.oy[p][i] == fdiv8(vy) && P.fx[p][i] == (float)fmod8(vx) / 8.0f &&
                     P.fy[p][i] == (float)fmod8(vy) / 8.0f;
            }
        if (eq) return A;
    }
    return 0;
}
int std_tap_plan(const TapPlan& P) {
    if (!P.valid || g_no_std) return 0;
    for (int A : {12, 48}) {
        bool eq = true;
        for (int i = 0; i < 8 && eq; ++i) {
            const int vx = A * tap_m(0, i), vy = A * tap_m(1, i);
            eq = (fmod8(vx) == 0 || fmod8(vx) == 4) && (fmod8(vy) == 0 || fmod8(vy) == 4) && P.ox[i] == fdiv8(vx) &&
                 P.oy[i] == fdiv8(vy) && ((P.hx >> i) & 1u) == (fmod8(vx) == 4 ? 1u : 0u) &&
                 ((P.hy >> i) & 1u) == (fmod8(vy) == 4 ? 1u : 0u);
        }
        if (eq) return A;
    }
    return 0;
}

// ---- host-side bound checks of the kernels' index arithmetic ------------------------------------
// Round 4's memory-access fault ("Bound checks") was a fix-up launch with a count read
// from a freed plan record.  Every form a launcher can take stages a block's input footprint in an LDS
// tile and reads it at offsets that a plan (or the kernel's own sampler arithmetic) gives; these checks
// replay that arithmetic on the host, in the kernels' own f32 operations, per block and per tap along
// each axis (every footprint here is separable), and require every staged extent to fit its tile, every
// tile read to fall inside the staged extent, and every plan index and list entry to fall inside its
// texture.  A separable or same-size plan that fails is never used (the pass takes the general form:
// bh_bloom_sep_verify / bh_bloom_same_verify, called where the host builds the plans), and in the dry
// mode of bh_bloom_check every launch of a chain runs its form's check instead of launching (the CPU
// test over frame sizes and levels, tests/test_bloom_bounds.py).
namespace {
struct DryRun {
    uint64_t launches = 0, checks = 0;
    std::string fail;
    std::string plan;  // one line per launch: its form, output size, input size, resolution uniform
};
thread_local DryRun* g_dry = nullptr;
// Test hook (tests/test_bloom_bounds.py): the checks treat every tile as this many entries smaller, so a
// footprint that fills its tile exactly must be reported -- the checks' own negative test.  0 in use.
const int g_check_slack = [] {
    const char* e = std::getenv("BH_BLOOM_CHECK_SLACK");
    return e ? std::atoi(e) : 0;
}();
thread_local std::string* g_why = nullptr;  // where a failing check writes its message (first one kept)

bool chk(bool ok, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
bool chk(bool ok, const char* fmt, ...) {
    if (g_dry) ++g_dry->checks;
    if (ok) return true;
    std::string* w = g_dry ? &g_dry->fail : g_why;
    if (w && w->empty()) {
        char buf[256];
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        *w = buf;
    }
    return false;
}
// the dry run's launch list (bh_bloom_check): "form ow oh tw th rx ry"
void note_launch(const char* form, uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry) {
    if (!g_dry) return;
    ++g_dry->launches;
    char buf[128];
    std::snprintf(buf, sizeof buf, "%s %u %u %u %u %u %u\n", form, ow, oh, tw, th, rx, ry);
    g_dry->plan += buf;
}

// One axis of up_sep_kernel (B = 16) / up_sepq_kernel (B = 32): the footprint the kernel derives from the
// sampler arithmetic of its first and last column, c = hi - lo + 2 entries (floor .. floor + 1), which the
// kernel cuts to FP -- the cut must never happen -- and for every tap and column of the block the plan's
// floor f with both of its texels f - lo, f + 1 - lo inside those c entries.  e: the axis's [8][on] entries.
bool sep_axis_ok(const SepEntry* e, uint32_t on, uint32_t tn, uint32_t res, int axis, uint32_t B, int FP) {
    const float dmin = h_tap_min(res, axis), dmax = h_tap_max(res, axis);
    for (uint32_t b = 0; b < on; b += B) {
        const uint32_t l = std::min(b + B - 1u, on - 1u);
        const int32_t lo = h_floor(h_sample_coord(h_texcoord(b, on) + dmin, tn));
        const int32_t hi = h_floor(h_sample_coord(h_texcoord(l, on) + dmax, tn));
        const int32_t c = hi - lo + 2;
        if (!chk(c >= 2 && c <= FP - g_check_slack, "separable %s footprint of block %u: %d entries, tile side %d", axis ? "row" : "column",
                 b, c, FP))
            return false;
        for (int i = 0; i < 8; ++i)
            for (uint32_t x = b; x <= l; ++x) {
                const SepEntry& s = e[(size_t)i * on + x];
                if (!chk(s.f >= -1 && s.f <= (int32_t)tn, "separable plan floor %d outside [-1, %u] (tap %d, %s %u)", s.f,
                         tn, i, axis ? "row" : "column", x) ||
                    !chk(s.f - lo >= 0 && s.f + 1 - lo <= c - 1,
                         "separable tap %d of %s %u reads entries %d..%d of a %d-entry footprint", i, axis ? "row" : "column",
                         x, s.f - lo, s.f + 1 - lo, c) ||
                    !chk(s.fa >= 0.0f && s.fa <= 1.0f && s.ia == 1.0f - s.fa, "separable plan weight %g at %s %u", (double)s.fa,
                         axis ? "row" : "column", x))
                    return false;
            }
    }
    return true;
}
// A tile of FP rows at stride FS, with a row-pair shift of (ly + p) >> 1 entries when shift = p + 1 (the quad
// tiles: p = 0; bloom_yq_kernel: p up to 1): its largest entry for rows and columns below FP must stay below
// the declared size.
bool tile_ok(int FP, int FS, int shift, int size) {
    const int last = (FP - 1) * FS + (shift ? (FP - 1 + shift - 1) >> 1 : 0) + (FP - 1);
    return chk(FS >= FP && last < size, "tile FP %d stride %d: last entry %d of %d", FP, FS, last, size);
}

// One axis of with_source's (and up2_kernel's outer blocks') fallback: the kernel's tap_span over a block of
// B pixels, and, when it fits FP, every tap's two clamped texels inside it.
bool span_axis_ok(uint32_t on, uint32_t tn, uint32_t res, int axis, uint32_t B, int FP) {
    const float dmin = h_tap_min(res, axis), dmax = h_tap_max(res, axis);
    const int32_t hm = (int32_t)tn - 1;
    auto clampi_h = [&](int32_t v) { return std::min(std::max(v, 0), hm); };
    for (uint32_t b = 0; b < on; b += B) {
        const uint32_t l = std::min(b + B - 1u, on - 1u);
        const int32_t lo = clampi_h(h_floor(h_sample_coord(h_texcoord(b, on) + dmin, tn)));
        const int32_t hi = clampi_h(h_floor(h_sample_coord(h_texcoord(l, on) + dmax, tn)) + 1);
        const int32_t n = hi - lo + 1;
        if (n > FP) continue;  // block-uniform: this block reads global memory through clamped indices
        if (!chk(n <= FP - g_check_slack, "staged span of %s block %u: %d texels, tile side %d", axis ? "row" : "column",
                 b, n, FP))
            return false;
        for (int i = 0; i < 8; ++i)
            for (uint32_t x = b; x <= l; ++x) {
                const int32_t f = h_floor(h_sample_coord(h_texcoord(x, on) + h_tap(res, axis, i), tn));
                const int32_t x0 = clampi_h(f), x1 = clampi_h(f + 1);
                if (!chk(x0 >= lo && x1 <= hi, "staged tap %d of %s %u reads texels %d..%d of span %d..%d", i,
                         axis ? "row" : "column", x, x0, x1, lo, hi))
                    return false;
            }
    }
    return true;
}

// One axis of a TapPlan form over blocks of B pixels and a tile of side FP: the kernel takes the form when
// hi - lo + B <= FP (launch-uniform), and then a pixel p of a block reads entries p - b + (o_i - lo) and
// + half_i; otherwise the span fallback.
bool tapplan_axis_ok(const TapPlan& P, uint32_t on, uint32_t tn, uint32_t res, int axis, uint32_t B, int FP) {
    const int32_t lo = axis ? P.lo_y : P.lo_x, hi = axis ? P.hi_y : P.hi_x;
    if (!P.valid || hi - lo + (int32_t)B > FP) return span_axis_ok(on, tn, res, axis, B, FP);
    if (!chk(hi - lo + (int32_t)B <= FP - g_check_slack, "tap plan footprint %d of a %d tile", hi - lo + (int32_t)B, FP))
        return false;
    for (int i = 0; i < 8; ++i) {
        const int32_t o = axis ? P.oy[i] : P.ox[i];
        const int32_t h = (int32_t)(((axis ? P.hy : P.hx) >> i) & 1u);
        if (!chk(o - lo >= 0 && (int32_t)B - 1 + o + h - lo <= hi - lo + (int32_t)B - 1,
                 "tap plan tap %d offset %d (+%d) outside the footprint %d..%d", i, o, h, lo, hi))
            return false;
    }
    return true;
}

// One axis of up2_kernel: blocks of 32 pixels staged when the span fits FP_UPQ; inside P's interior the quad
// reads texels (x >> 1) + o[0] .. (x >> 1) + o[1] + 1 of every tap, which must lie in the span.
bool up2_axis_ok(const Up2Plan& P, uint32_t on, uint32_t tn, uint32_t res, int axis, int FP) {
    if (!span_axis_ok(on, tn, res, axis, 32u, FP)) return false;
    const float dmin = h_tap_min(res, axis), dmax = h_tap_max(res, axis);
    const int32_t hm = (int32_t)tn - 1;
    const int32_t ilo = axis ? P.y_lo : P.x_lo, ihi = axis ? P.y_hi : P.x_hi;
    for (uint32_t b = 0; b < on; b += 32u) {
        const uint32_t l = std::min(b + 31u, on - 1u);
        const int32_t lo = std::min(std::max(h_floor(h_sample_coord(h_texcoord(b, on) + dmin, tn)), 0), hm);
        const int32_t hi = std::min(std::max(h_floor(h_sample_coord(h_texcoord(l, on) + dmax, tn)) + 1, 0), hm);
        if (hi - lo + 1 > FP || (int32_t)b < ilo || (int32_t)b + 31 > ihi) continue;  // not an inner block
        for (int i = 0; i < 8; ++i) {
            const int32_t o0 = axis ? P.oy[0][i] : P.ox[0][i], o1 = axis ? P.oy[1][i] : P.ox[1][i];
            for (uint32_t x = b; x <= l; x += 2u) {
                const int32_t first = (int32_t)(x >> 1) + o0, last = (int32_t)(x >> 1) + o1 + 1;
                if (!chk(first >= lo && last <= hi && first >= 0 && last <= hm,
                         "2:1 quad tap %d of %s %u reads texels %d..%d of span %d..%d", i, axis ? "row" : "column", x,
                         first, last, lo, hi))
                    return false;
            }
        }
    }
    return true;
}

// The same-size plan (bh_bloom_same_plan) and its list of inexact columns, then rows: every texel index
// inside the frame, weights in [0, 1], and the list exactly the columns / rows of nonzero weight, ascending
// (the fused epilogues skip those pixels and fixup_gather_kernel recomputes them: a missing entry leaves a pixel
// unwritten, an extra one writes it twice with the same value).
bool same_ok(uint32_t w, uint32_t h, const uint32_t* plan, const uint32_t* list, uint32_t nc, uint32_t nr,
             bool with_list = true) {
    if (!chk(nc <= w && nr <= h, "same-size plan: %u inexact columns of %u, %u rows of %u", nc, w, nr, h)) return false;
    for (int axis = 0; axis < 2; ++axis) {
        const uint32_t n = axis ? h : w, base = axis ? w : 0u, cnt = axis ? nr : nc;
        const uint32_t* L = with_list ? list + (axis ? nc : 0u) : nullptr;
        uint32_t k = 0;
        for (uint32_t x = 0; x < n; ++x) {
            const uint32_t e = plan[2u * (base + x)];
            float wgt;
            std::memcpy(&wgt, &plan[2u * (base + x) + 1u], 4);
            const uint32_t x0 = e & 0xFFFFu, x1 = e >> 16;
            if (!chk(x0 < n && x1 < n && wgt >= 0.0f && wgt <= 1.0f, "same-size plan %s %u: texels %u, %u, weight %g of %u",
                     axis ? "row" : "column", x, x0, x1, (double)wgt, n) ||
                !chk(wgt != 0.0f || x0 == x, "same-size plan: exact %s %u samples texel %u", axis ? "row" : "column", x, x0))
                return false;
            if (wgt != 0.0f && with_list) {
                if (!chk(k < cnt && L[k] == x, "same-size list: %s %u missing", axis ? "row" : "column", x)) return false;
                ++k;
            }
        }
        if (with_list && !chk(k == cnt, "same-size list: %u %s entries for %u inexact", cnt, axis ? "row" : "column", k)) return false;
    }
    return true;
}
// The fix-up records of a list (bh_bloom_fixup_records): entry k's column (row) and the plan entries of it and
// of its clamped neighbours, exactly as the kernel would read them from the plan.
bool records_ok(uint32_t w, uint32_t h, const uint32_t* plan, const uint32_t* list, uint32_t nc, uint32_t nr,
                const uint32_t* rec) {
    for (uint32_t k = 0; k < nc + nr; ++k) {
        const uint32_t n = k < nc ? w : h, base = k < nc ? 0u : w, u = list[k];
        const uint32_t* r = rec + 8u * k;
        if (!chk(r[0] == u && u < n, "fix-up record %u names %u, its list %u", k, r[0], u)) return false;
        const uint32_t nb[3] = {u ? u - 1u : 0u, u, std::min(u + 1u, n - 1u)};
        for (int t = 0; t < 3; ++t)
            if (!chk(r[1 + 2 * t] == plan[2u * (base + nb[t])] && r[2 + 2 * t] == plan[2u * (base + nb[t]) + 1u],
                     "fix-up record %u: plan entry %u differs", k, nb[t]))
                return false;
    }
    return true;
}
// The inexact columns of a same-size plan (its list's column count)
uint32_t n_inexact(uint32_t w, const uint32_t* plan) {
    uint32_t n = 0;
    for (uint32_t x = 0; x < w; ++x) n += plan[2u * x + 1u] != 0u;
    return n;
}
// The column records' word 7: 1 + the column's strip column (fixup_gather_kernel's qx)
bool strip_records_ok(const uint32_t* list, uint32_t nc, const uint32_t* stc, const uint32_t* rec) {
    for (uint32_t k = 0; k < nc; ++k)
        if (!chk(rec[8u * k + 7u] == stc[list[k]], "fix-up record %u: strip column %u, table %u", k, rec[8u * k + 7u], stc[list[k]]))
            return false;
    return true;
}
// The fix-up's column strips (bh_bloom_strip_table, up_sepq_kernel's STRIPS epilogue, fixup_gather_kernel):
// stc[c] is 0 or 1 + column c's strip column, distinct and below tw, so each strip word has one writer; and
// every texel a column lane of inexact column x reads (its own sample and F's at the sample's texels) lies in
// x's strip at the same offset: stc[c] - stc[x] == c - x.
bool strip_ok(uint32_t w, uint32_t h, const uint32_t* plan, const uint32_t* list, uint32_t nc, const uint32_t* stc,
              uint32_t tw) {
    if (!chk(tw > 0u && tw <= w && nc <= w, "strips: %u strip columns, %u inexact columns of %u", tw, nc, w)) return false;
    std::vector<uint8_t> seen(tw, 0u);
    for (uint32_t c = 0; c < w; ++c) {
        if (stc[c] == 0u) continue;
        const uint32_t q = stc[c] - 1u;
        if (!chk(q < tw && !seen[q], "strip table: column %u -> strip column %u of %u", c, q, tw)) return false;
        seen[q] = 1u;
    }
    for (uint32_t k = 0; k < nc; ++k) {
        const uint32_t x = list[k];
        if (!chk(x < w && stc[x] != 0u, "strips: inexact column %u outside every strip", x)) return false;
        auto same_strip = [&](uint32_t c) { return c < w && stc[c] != 0u && (int64_t)stc[c] - stc[x] == (int64_t)c - x; };
        const uint32_t e = plan[2u * x], ex = plan[2u * x + 1u];
        const uint32_t px[2] = {e & 0xFFFFu, e >> 16};
        for (int t = 0; t < (ex != 0u ? 2 : 1); ++t) {
            const uint32_t ep = plan[2u * px[t]], wp = plan[2u * px[t] + 1u];
            if (!chk(same_strip(px[t]) && same_strip(ep & 0xFFFFu) && (wp == 0u || same_strip(ep >> 16)),
                     "strips: column %u reads texel %u (samples %u, %u) outside its strip", x, px[t], ep & 0xFFFFu, ep >> 16))
                return false;
        }
    }
    (void)h;
    return true;
}
}  // namespace

static const bool g_no_sepq = std::getenv("BH_BLOOM_NO_SEPQ") != nullptr;  // A/B: the one-pixel kernel
SepForm sep_form(int ext) {
    const int e16 = ext & 0xFFFF, e32 = (ext >> 16) & 0xFFFF;
    const int one = e16 <= 0 ? 0 : e16 <= 24 ? 24 : e16 <= 44 ? 44 : 0;
    const int q = g_no_sepq || e32 <= 0 ? 0 : e32 <= 28 ? 28 : e32 <= 40 ? 40 : e32 <= 60 ? 60 : 0;
    SepForm f;
    if (q != 0) {
        f.quad = true;
        f.FP = q;
        f.raw = q == 60;  // the wide tile as raw words, decoded per read
        f.FS = q == 60 ? SEPQ_FS60 : q == 28 ? 32 : 40;
    } else if (one != 0) {
        f.FP = one;
        f.raw = one == 44;
        f.FS = f.raw ? sep_stride<44, true>() : sep_stride<24, false>();
    }
    return f;
}
static const bool g_no_up2 = std::getenv("BH_BLOOM_NO_UP2") != nullptr;  // A/B: the general up pass
static const bool g_no_sep = std::getenv("BH_BLOOM_NO_SEP") != nullptr;  // A/B: the per-pixel sampler
bool up2_enabled() { return !g_no_up2; }
bool sep_enabled() { return !g_no_sep; }

// ---- the launchers' dry-run branches: the launch's line in the dry run's list, then its form's checks ----
bool check_sep_launch(uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t rx, uint32_t ry, const uint32_t* sep,
                      int ext, uint32_t epi, const uint32_t* same, const uint32_t* stc, uint32_t strip_w) {
    const SepForm f = sep_form(ext);
    char form[32];
    std::snprintf(form, sizeof form, "%s%d%s/%u", f.quad ? "sepq" : "sep", f.FP, f.raw ? "r" : "", epi);
    note_launch(form, ow, oh, aw, ah, rx, ry);
    // stc: the column strips the quad kernel's final epilogue writes for its fix-up
    if (stc && !strip_ok(ow, oh, same, same + 2u * ((size_t)ow + oh), n_inexact(ow, same), stc, strip_w)) return false;
    return bh_bloom_sep_verify(ow, oh, aw, ah, rx, ry, sep, ext, nullptr) &&
           (epi == EPI_PLAIN || chk(same != nullptr, "separable epilogue without a same-size plan"));
}
bool check_fixup_launch(uint32_t epi, uint32_t w, uint32_t h, const uint32_t* same, const uint32_t* list, uint32_t n_cols,
                        uint32_t n_rows, const uint32_t* recs, const uint32_t* stc, uint32_t strip_w) {
    note_launch(epi == EPI_Y ? "fixup/1" : "fixup/2", w, h, n_cols, n_rows, 0u, 0u);
    return same_ok(w, h, same, list, n_cols, n_rows) &&
           chk(list == same + 2u * ((size_t)w + h), "fix-up list is not its plan's") &&
           records_ok(w, h, same, list, n_cols, n_rows, recs) &&
           (!stc || (strip_ok(w, h, same, list, n_cols, stc, strip_w) && strip_records_ok(list, n_cols, stc, recs)));
}
// every index of down2_kernel is clamped to its texture (down_at): only the sizes to check
bool check_down2_launch(uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t mw, uint32_t mh) {
    note_launch("down2", ow, oh, aw, ah, mw, mh);
    return chk(aw > 0u && ah > 0u && ow > 0u && oh > 0u, "down2 of an empty texture");
}
// the same-size plan's texel indices (host copy)
bool check_same_launch(const char* form, uint32_t w, uint32_t h, const uint32_t* plan) {
    note_launch(form, w, h, w, h, w, h);
    return chk(plan != nullptr, "%s without a plan", form) && same_ok(w, h, plan, nullptr, 0u, 0u, false);
}
bool check_up2_launch(const Up2Plan& Q, uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t rx, uint32_t ry) {
    note_launch(std_up2_plan(Q) == 12 ? "up2_12" : std_up2_plan(Q) == 3 ? "up2_3" : "up2_0", ow, oh, aw, ah, rx, ry);
    return tile_ok(FP_UPQ, FS_UPQ, 0, FP_UPQ * FS_UPQ) && up2_axis_ok(Q, ow, aw, rx, 0, FP_UPQ) &&
           up2_axis_ok(Q, oh, ah, ry, 1, FP_UPQ);
}
// pass_kernel: an up pass stages through with_source<FP_UP>; the others read clamped indices
bool check_pass_launch(uint32_t shader, const TapPlan& P, uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t rx,
                       uint32_t ry) {
    note_launch(shader == SH_UP ? (P.valid ? "pass_up_tap" : "pass_up") : shader == SH_COPY ? "pass_copy"
                : shader == SH_DOWN ? "pass_down" : "pass_remix", ow, oh, aw, ah, rx, ry);
    return chk(aw > 0u && ah > 0u && ow > 0u && oh > 0u, "pass over an empty texture") &&
           (shader != SH_UP || (tile_ok(FP_UP, FP_UP, 0, FP_UP * FP_UP) && tapplan_axis_ok(P, ow, aw, rx, 0, 16u, FP_UP) &&
                                tapplan_axis_ok(P, oh, ah, ry, 1, 16u, FP_UP)));
}
// the Y pass: the quad form's tile (row-pair shift) or with_source<FP_Y>; d2: the two downsamples fused into it
bool check_y_launch(const TapPlan& P, bool quad, bool d2, uint32_t w, uint32_t h) {
    note_launch(quad ? (std_tap_plan(P) == 12 ? "yq12" : "yq0") : "y1", w, h, w, h, w, h);
    if (d2) note_launch("down2f", w / 4u, h / 4u, w, h, w / 2u, h / 2u);
    return quad ? tile_ok(FP_YQ, FS_YQ, 2, FP_YQ * FS_YQ + FP_YQ / 2 + 1) && tapplan_axis_ok(P, w, w, w, 0, 32u, FP_YQ) &&
                      tapplan_axis_ok(P, h, h, h, 1, 32u, FP_YQ)
                : tile_ok(FP_Y, FP_Y, 0, FP_Y * FP_Y) && tapplan_axis_ok(P, w, w, w, 0, 16u, FP_Y) &&
                      tapplan_axis_ok(P, h, h, h, 1, 16u, FP_Y);
}
// the final pass's with_source<FP_FINAL>: the TapPlan form (raw words) or the span fallback
bool check_final_launch(const TapPlan& P, uint32_t w, uint32_t h, uint32_t rx, uint32_t ry) {
    note_launch(P.valid ? (std_tap_plan(P) == 48 ? "final48" : "final0") : "final", w, h, w, h, rx, ry);
    return tile_ok(FP_FINAL, FP_FINAL, 0, FP_FINAL * FP_FINAL) && tapplan_axis_ok(P, w, w, rx, 0, 16u, FP_FINAL) &&
           tapplan_axis_ok(P, h, h, ry, 1, 16u, FP_FINAL);
}

}  // namespace bloom
}  // namespace bh

using namespace bh::bloom;

// The strip table of a same-size plan's nc inexact columns (list, ascending): the columns within 2 of an
// inexact column, merged into contiguous runs (inexact columns cluster), numbered left to right: stc[c] = 1 +
// c's strip column, 0 outside.  Returns the number of strip columns (0: no inexact column).
uint32_t bh_bloom_strip_table(uint32_t w, const uint32_t* list, uint32_t nc, uint32_t* stc) {
    std::fill(stc, stc + w, 0u);
    uint32_t tw = 0;
    for (uint32_t k = 0; k < nc; ++k) {
        const int64_t lo = std::max<int64_t>((int64_t)list[k] - 2, 0), hi = std::min<int64_t>((int64_t)list[k] + 2, (int64_t)w - 1);
        for (int64_t c = lo; c <= hi; ++c)
            if (stc[c] == 0u) stc[c] = ++tw;
    }
    return tw;
}

// The fix-up records of a list of n_cols columns then n_rows rows into out (8 words per entry, see
// fixup_gather_kernel).
void bh_bloom_fixup_records(uint32_t w, uint32_t h, const uint32_t* plan, const uint32_t* list, uint32_t nc, uint32_t nr,
                            uint32_t* out) {
    for (uint32_t k = 0; k < nc + nr; ++k) {
        const uint32_t n = k < nc ? w : h, base = k < nc ? 0u : w, u = std::min(list[k], n - 1u);
        const uint32_t nb[3] = {u ? u - 1u : 0u, u, std::min(u + 1u, n - 1u)};
        uint32_t* r = out + 8u * k;
        r[0] = list[k];
        for (int t = 0; t < 3; ++t) {
            r[1 + 2 * t] = plan[2u * (base + nb[t])];
            r[2 + 2 * t] = plan[2u * (base + nb[t]) + 1u];
        }
        r[7] = 0u;
    }
}

// bh_bloom_sep_plan's plan (host copy `plan`, extents `ext`) checked for the form bh_launch_bloom_sep takes:
// false (and the reason in *why) when any block's footprint exceeds its tile or any read leaves it.
bool bh_bloom_sep_verify(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry, const uint32_t* plan,
                         int ext, std::string* why) {
    std::string* prev = g_why;
    g_why = why;
    const SepForm f = sep_form(ext);
    const SepEntry* e = reinterpret_cast<const SepEntry*>(plan);
    const uint32_t B = f.quad ? 32u : 16u;
    const int size = f.quad ? f.FP * f.FS + f.FP / 2 : f.FP * f.FS;
    // FP == 0: no staged form fits these extents, and the launcher refuses the plan (the general pass runs)
    const bool ok = f.FP == 0 || (tile_ok(f.FP, f.FS, f.quad ? 1 : 0, size) && sep_axis_ok(e, ow, tw, rx, 0, B, f.FP) &&
                                  sep_axis_ok(e + 8u * (size_t)ow, oh, th, ry, 1, B, f.FP));
    g_why = prev;
    return ok;
}
bool bh_bloom_same_verify(uint32_t w, uint32_t h, const uint32_t* plan, uint32_t nc, uint32_t nr, std::string* why) {
    std::string* prev = g_why;
    g_why = why;
    const bool ok = same_ok(w, h, plan, plan + 2u * ((size_t)w + h), nc, nr);
    g_why = prev;
    return ok;
}
// The fix-up records of a list (records_ok) and, when stc != nullptr, the column strips of the plan's full list
// with the column records' word 7 (strip_ok, strip_records_ok): what bh_bloom_check's dry run checks at each
// launch, run by sep_plan on every real plan before it is uploaded.
bool bh_bloom_records_verify(uint32_t w, uint32_t h, const uint32_t* plan, const uint32_t* list, uint32_t nc, uint32_t nr,
                             const uint32_t* rec, const uint32_t* stc, uint32_t strip_w, std::string* why) {
    std::string* prev = g_why;
    g_why = why;
    const bool ok = records_ok(w, h, plan, list, nc, nr, rec) &&
                    (!stc || (strip_ok(w, h, plan, list, nc, stc, strip_w) && strip_records_ok(list, nc, stc, rec)));
    g_why = prev;
    return ok;
}
// Dry mode (bh_bloom_check): while it is on, the launchers below check their launch's form on the host and
// return without launching; the plan pointers they receive are host copies.
void bh_bloom_dry_begin(void) {
    delete g_dry;
    g_dry = new DryRun();
}
bool bh_bloom_dry_end(uint64_t* launches, uint64_t* checks, std::string* fail, std::string* plan) {
    if (!g_dry) return false;
    if (launches) *launches = g_dry->launches;
    if (checks) *checks = g_dry->checks;
    if (fail) *fail = g_dry->fail;
    if (plan) *plan = g_dry->plan;
    const bool ok = g_dry->fail.empty();
    delete g_dry;
    g_dry = nullptr;
    return ok;
}
bool bh_bloom_dry(void) { return g_dry != nullptr; }

// The separable plan of an 8-tap pass (see SepEntry / up_sep_kernel): 8 * (ow + oh) entries of 4 words
// into `outp` (per tap and column, then per tap and row), from the kernel's own f32 arithmetic: texcoord
// (x + 0.5) / n (the division core is IEEE division in its domain), the tap offset, sample_coord and
// floor.  Returns the largest 16x16 block footprint along either axis (the staged tile's side of
// up_sep_kernel) in the low 16 bits and the largest 32x32 block footprint (up_sepq_kernel) in the high ones, or
// -1 (texture sides above 65535).
int bh_bloom_sep_plan(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry, uint32_t* outp) {
    if (tw > 65535u || th > 65535u || tw == 0u || th == 0u || ow == 0u || oh == 0u) return -1;
    auto axis = [](uint32_t on, uint32_t tn, float d, uint32_t x, uint32_t* o) {
        const float t = h_sample_coord(((float)x + 0.5f) / (float)on + d, tn);
        const float f = floorf(t), fa = t - f, ia = 1.0f - fa;
        const int32_t fi = (int32_t)f;
        std::memcpy(&o[0], &fi, 4);
        std::memcpy(&o[1], &fa, 4);
        std::memcpy(&o[2], &ia, 4);
        o[3] = 0u;
    };
    auto fl = [&](size_t e) { int32_t v; std::memcpy(&v, outp + 4u * e, 4); return v; };
    for (int i = 0; i < 8; ++i) {
        const float du = h_tap(rx, 0, i), dv = h_tap(ry, 1, i);
        for (uint32_t x = 0; x < ow; ++x) axis(ow, tw, du, x, outp + 4u * ((size_t)i * ow + x));
        for (uint32_t y = 0; y < oh; ++y) axis(oh, th, dv, y, outp + 4u * (8u * (size_t)ow + (size_t)i * oh + y));
    }
    int ext[2] = {0, 0};  // 16- and 32-pixel blocks
    for (int q = 0; q < 2; ++q) {
        const uint32_t B = q ? 32u : 16u;
        for (int ax = 0; ax < 2; ++ax) {
            const uint32_t n = ax ? oh : ow;
            const size_t base = ax ? 8u * (size_t)ow : 0u;
            for (uint32_t b = 0; b < n; b += B) {
                const uint32_t l = std::min(b + B - 1u, n - 1u);
                int32_t lo = INT_MAX, hi = INT_MIN;
                for (int i = 0; i < 8; ++i) {
                    lo = std::min(lo, fl(base + (size_t)i * n + b));
                    hi = std::max(hi, fl(base + (size_t)i * n + l));
                }
                ext[q] = std::max(ext[q], hi - lo + 2);
            }
        }
    }
    return std::min(ext[0], 0x7FFF) | std::min(ext[1], 0x7FFF) << 16;  // up_sep_kernel's | up_sepq_kernel's
}

// The same-size plan of a w x h frame (remix_plan_kernel): per column, then per row, the two clamped
// texels and the weight of a sample at the pixel's own texcoord ((x + 0.5) / n, sample_coord, floor).
// Texel indices are 16-bit fields: w, h <= 65536.
bool bh_bloom_same_plan(uint32_t w, uint32_t h, uint32_t* outp) {
    if (w > 65536u || h > 65536u || w == 0u || h == 0u) return false;
    auto axis = [](uint32_t n, uint32_t x, uint32_t* o) {
        const float t = h_sample_coord(((float)x + 0.5f) / (float)n, n);
        const float f = floorf(t), wgt = t - f;
        const int32_t hi = (int32_t)n - 1;
        const int32_t a0 = std::min(std::max((int32_t)f, 0), hi), a1 = std::min(std::max((int32_t)f + 1, 0), hi);
        o[0] = (uint32_t)a0 | (uint32_t)a1 << 16;
        std::memcpy(&o[1], &wgt, 4);
    };
    for (uint32_t x = 0; x < w; ++x) axis(w, x, outp + 2u * x);
    for (uint32_t y = 0; y < h; ++y) axis(h, y, outp + 2u * ((size_t)w + y));
    return true;
}

// bit i: tap i of kawase_upsample.wgsl samples texel centres exactly for every pixel of an
// ow x oh pass over a tw x th texture with resolution uniform (rx, ry)
uint32_t bh_bloom_point_mask(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry) {
    uint32_t m = 0;
    for (int i = 0; i < 8; ++i)
        if (axis_point(ow, tw, h_tap(rx, 0, i)) && axis_point(oh, th, h_tap(ry, 1, i))) m |= 1u << i;
    return m;
}

// Whether bh_launch_bloom_pass runs an up pass of this shape with up_sep_kernel (neither the TapPlan nor
// the Up2Plan form applies): only then does the host build the shape's separable plan (bh_bloom_sep_plan).
bool bh_bloom_up_uses_sep(uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t rx, uint32_t ry) {
    if (g_no_sep || tap_plan(ow, oh, aw, ah, rx, ry).valid) return false;
    return g_no_up2 || !up2_plan(ow, oh, aw, ah, rx, ry).valid;
}

// Whether the Y quad pass can run the blur's first two downsamples in its epilogue (bloom_yq_kernel's D2)
bool bh_bloom_down2_fusable(uint32_t w, uint32_t h) {
    // the sides multiples of 32 (the Y quad kernel's block: every lane inside the frame), and down2_kernel's
    // sample arithmetic (down_at) on every pixel of both levels: texel 2 x' and 2 x' + 1, weight 0.5 -- which
    // holds at powers of two, not at display sizes such as 1920 x 1080 (37 and 32 inexact samples per axis)
    auto axis = [](uint32_t n) {
        if (n % 32u != 0u) return false;
        for (uint32_t on = n / 2u, tn = n; on >= n / 4u; tn = on, on /= 2u)
            for (uint32_t x = 0; x < on; ++x) {
                const float t = h_sample_coord(h_texcoord(x, on), tn), f = floorf(t);
                if (f != (float)(2u * x) || t - f != 0.5f || 2u * x + 1u > tn - 1u) return false;
            }
        return true;
    };
    return axis(w) && axis(h);
}

