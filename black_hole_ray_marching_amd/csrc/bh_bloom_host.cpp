// bh_bloom_host.cpp — the host side of bh_bloom (include/bh_render.h): which same-size passes are identities,
// the separable plans of the up passes, the chain of launches (bh_bloom.hip holds the kernels and their
// launchers, bh_bloom_plan.cpp the plan builders and host checks) and bh_bloom_check's dry run of it.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "bh_bloom_plan.hpp"
#include "bh_host.hpp"

void free_bloom_scratch(bh_ctx::BloomScratch& b) {
    for (uint32_t* t : b.tex) (void)hipFree(t);
    for (auto& p : b.sep_plans)
        if (!p.host) {
            (void)hipFree(p.dev);
            (void)hipFree(p.strips);
        }
    b.tex.clear();
    b.sep_plans.clear();
}

namespace {

// A same-size pass (copy, the blur's same-size downsample, a remix input: n texels sampled at n pixels)
// is the identity on stored texels when every pixel's bilinear sample encodes back to its own texel's
// byte.  Along one axis pixel x samples texels x0, x1 = clamp(floor(t)), clamp(floor(t) + 1) with
// weights 1 - fa, fa (t = RN(RN((x + 0.5) / n) * n) - 0.5, sample()'s arithmetic); where t == x the
// weights are exactly 1 and 0, elsewhere (e.g. 51 of 1920 columns, 42 of 1080 rows) t misses x by a few
// ulps and the weight on the other texel is tiny but not 0.  Every rounding of the 2-D lerp is monotone
// in each texel (weights >= 0), so with texel (x, y) = D the result lies between the lerp with every
// other texel 0 and with every other texel 1 (the largest decoded value); when both bounds encode to D's
// own byte for every byte value, every weight class of the two axes and both channel kinds (sRGB colour,
// linear alpha k/255), the pass returns its input's bytes whatever the other texels are.  Powers of two
// (t == x everywhere) pass trivially.
struct AxisClass {
    float ia, fa;  // the weights on texels x0 and x1
    bool d0, d1;   // x0 == x, x1 == x
    bool operator==(const AxisClass& o) const { return ia == o.ia && fa == o.fa && d0 == o.d0 && d1 == o.d1; }
};
bool same_size_axis(uint32_t n, std::vector<AxisClass>& cls) {
    cls.clear();
    const int32_t hi = (int32_t)n - 1;
    for (uint32_t x = 0; x < n; ++x) {
        const float u = ((float)x + 0.5f) / (float)n;
        const float t = fminf(fmaxf(u * (float)n - 0.5f, -1.0f), (float)n);
        const float f = floorf(t);
        const float fa = t - f;
        const int32_t x0 = std::min(std::max((int32_t)f, 0), hi), x1 = std::min(std::max((int32_t)f + 1, 0), hi);
        const AxisClass c{1.0f - fa, fa, x0 == (int32_t)x, x1 == (int32_t)x};
        if (!c.d0 && !c.d1) return false;
        if (std::find(cls.begin(), cls.end(), c) == cls.end()) cls.push_back(c);
    }
    return true;
}
uint8_t unorm8_ref(float a) {
    if (!(a > 0.0f)) return 0;
    if (a >= 1.0f) return 255;
    return (uint8_t)std::floor((double)a * 255.0 + 0.5);
}
// Every pixel of a same-size pass samples its own texel centre exactly (t == x): weights 1 and 0, the
// sample is the texel itself, before any quantisation (powers of two).
bool same_size_exact(uint32_t n) {
    for (uint32_t x = 0; x < n; ++x) {
        const float u = ((float)x + 0.5f) / (float)n;
        if (u * (float)n - 0.5f != (float)x) return false;
    }
    return true;
}
bool same_size_identity(uint32_t w, uint32_t h) {
    static thread_local std::vector<std::pair<uint64_t, bool>> memo;
    const uint64_t key = (uint64_t)w << 32 | h;
    for (const auto& m : memo)
        if (m.first == key) return m.second;
    std::vector<AxisClass> cx, cy;
    bool ok = same_size_axis(w, cx) && same_size_axis(h, cy);
    float lut[256];
    srgb_lut(lut);
    for (const AxisClass& X : cx)
        for (const AxisClass& Y : cy)
            for (int kind = 0; kind < 2 && ok; ++kind)
                for (int b = 0; b < 256 && ok; ++b) {
                    const float D = kind == 0 ? lut[b] : (float)b / 255.0f;
                    for (float O : {0.0f, 1.0f}) {
                        const float t00 = X.d0 && Y.d0 ? D : O, t10 = X.d1 && Y.d0 ? D : O;
                        const float t01 = X.d0 && Y.d1 ? D : O, t11 = X.d1 && Y.d1 ? D : O;
                        const float r = (t00 * X.ia + t10 * X.fa) * Y.ia + (t01 * X.ia + t11 * X.fa) * Y.fa;
                        if ((kind == 0 ? srgb_encode_ref(r) : unorm8_ref(r)) != b) ok = false;
                    }
                }
    if (memo.size() >= 16) memo.erase(memo.begin());
    memo.push_back({key, ok});
    return ok;
}

struct BloomPlan {
    uint32_t W, H, levels;
    uint32_t res[16][2];
};

// kawase_*sampling.rs:30-39: level l is (W, H) halved l times (integer), at least 1
BloomPlan bloom_plan(uint32_t W, uint32_t H, uint32_t levels) {
    BloomPlan p{W, H, levels, {}};
    uint32_t w = W, h = H;
    for (uint32_t l = 0; l < levels; ++l) {
        w = w ? w : 1u;
        h = h ? h : 1u;
        p.res[l][0] = w;
        p.res[l][1] = h;
        w /= 2u;
        h /= 2u;
    }
    return p;
}

// The separable plan of an up pass of this shape (bh_bloom_sep_plan), on the device, built at its first
// use and kept with the scratch set (64 B per column and row).  rx == 0: the same-size plan of the remixes
// (bh_bloom_same_plan, 8 B per column and row) followed by the list of its inexact columns, then rows (the
// fused epilogues' fix-up pixels).  Every plan is checked on the host before it is uploaded
// (bh_bloom_sep_verify / bh_bloom_same_verify: every block footprint inside its LDS tile, every read and
// index inside its tile and texture); a shape the builder refuses (texture sides above 65536) or whose
// check fails gets a plan with dev == nullptr, cached like the others, and its pass runs the general
// kernel -- with `dry_fail` (bh_bloom_check) a failed check is reported there instead.  In dry mode the
// plan stays on the host (dev points into `host`).  A capturing call never builds one (bh_bloom refuses a
// set not prepared outside capture).
// The column strips' storage limit per plan (3 words per strip column and row: 1.3 MB at 1920 x 1080)
constexpr size_t BH_STRIPS_BUDGET = (size_t)64 << 20;
// A plan the host check refused: in dry mode the check's failure; in a real bh_bloom a process-wide count and
// last message (bh_bloom_plan_failures) and one line on stderr, so that a regression in plan generation --
// bit-exact, but the slower general kernel -- does not pass silently.
std::atomic<uint64_t> g_plan_failures{0};
std::string g_plan_last;  // guarded by g_plan_mu
std::atomic_flag g_plan_mu = ATOMIC_FLAG_INIT;
void plan_failure(std::string* dry_fail, uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry,
                  const std::string& why) {
    const std::string msg = "plan " + std::to_string(ow) + "x" + std::to_string(oh) + " <- " + std::to_string(tw) + "x" +
                            std::to_string(th) + " res " + std::to_string(rx) + "x" + std::to_string(ry) + ": " + why;
    if (dry_fail) {
        if (dry_fail->empty()) *dry_fail = msg;
        return;
    }
    while (g_plan_mu.test_and_set(std::memory_order_acquire)) std::this_thread::yield();
    g_plan_last = msg;
    g_plan_mu.clear(std::memory_order_release);
    if (g_plan_failures.fetch_add(1) == 0)
        std::fprintf(stderr, "bh_bloom: a host check refused a plan; its pass runs the general kernel (same bytes, "
                             "slower): %s\n", msg.c_str());
}
// Returned by value: the cache is a vector that later plans reallocate.  (Round 4's memory-access fault:
// a pointer into it, held across the next call, read a freed record's fix-up counts)
bh_ctx::SepPlan sep_plan(bh_ctx::BloomScratch* b, bool capturing, std::string* dry_fail, uint32_t ow, uint32_t oh,
                         uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry, int* err) {
    const std::array<uint32_t, 6> key{ow, oh, tw, th, rx, ry};
    for (const auto& p : b->sep_plans)
        if (p.key == key) return p;
    bh_ctx::SepPlan P;
    P.key = key;
    if (capturing) {
        *err = (int)hipErrorStreamCaptureUnsupported;
        return P;
    }
    auto h = std::make_shared<std::vector<uint32_t>>();
    std::string why;
    bool ok;
    if (rx) {
        h->resize(32u * ((size_t)ow + oh));
        P.ext = bh_bloom_sep_plan(ow, oh, tw, th, rx, ry, h->data());
        ok = P.ext >= 0 && bh_bloom_sep_verify(ow, oh, tw, th, rx, ry, h->data(), P.ext, &why);
    } else {
        h->resize(2u * ((size_t)ow + oh));
        ok = bh_bloom_same_plan(ow, oh, h->data());
        if (ok) {
            std::vector<uint32_t> cols, rows;
            for (uint32_t x = 0; x < ow; ++x)
                if ((*h)[2u * x + 1u] != 0u) cols.push_back(x);
            for (uint32_t y = 0; y < oh; ++y)
                if ((*h)[2u * ((size_t)ow + y) + 1u] != 0u) rows.push_back(y);
            P.nc = (uint32_t)cols.size();
            P.nr = (uint32_t)rows.size();
            h->insert(h->end(), cols.begin(), cols.end());
            h->insert(h->end(), rows.begin(), rows.end());
            ok = bh_bloom_same_verify(ow, oh, h->data(), P.nc, P.nr, &why);
            if (ok) {
                // the list's records, 16-byte aligned (the kernel reads them as uint4), as the fix-up kernel reads
                // them (a failure drops the plan)
                const size_t lists = 2u * ((size_t)ow + oh);
                h->resize((h->size() + 3u) & ~(size_t)3u, 0u);
                P.rec = h->size();
                h->resize(P.rec + 8u * ((size_t)P.nc + P.nr), 0u);
                bh_bloom_fixup_records(ow, oh, h->data(), h->data() + lists, P.nc, P.nr, h->data() + P.rec);
                ok = bh_bloom_records_verify(ow, oh, h->data(), h->data() + lists, P.nc, P.nr, h->data() + P.rec, nullptr, 0u,
                                             &why);
                // the column strips of the final fix-up (BH_BLOOM_NO_STRIPS: off, A/B), within a storage budget
                static const bool no_strips = std::getenv("BH_BLOOM_NO_STRIPS") != nullptr;
                if (ok && !no_strips && P.nc > 0u) {
                    const size_t at = h->size();
                    h->resize(at + ow, 0u);
                    const uint32_t stw = bh_bloom_strip_table(ow, h->data() + lists, P.nc, h->data() + at);
                    if (stw > 0u && 3u * (size_t)stw * oh * 4u <= BH_STRIPS_BUDGET) {
                        // word 7 of each column record: 1 + the column's strip column
                        for (uint32_t k = 0; k < P.nc; ++k) (*h)[P.rec + 8u * k + 7u] = (*h)[at + (*h)[lists + k]];
                        // checked before upload: the gather kernel clamps its strip column, so a wrong table would
                        // give wrong pixels, not a fault; a failing table drops the strips (the plain fix-up runs)
                        std::string swhy;
                        if (bh_bloom_records_verify(ow, oh, h->data(), h->data() + lists, P.nc, 0u, h->data() + P.rec,
                                                    h->data() + at, stw, &swhy)) {
                            P.stc = at;
                            P.stw = stw;
                        } else {
                            for (uint32_t k = 0; k < P.nc; ++k) (*h)[P.rec + 8u * k + 7u] = 0u;
                            h->resize(at);
                            plan_failure(dry_fail, ow, oh, tw, th, rx, ry, "strips dropped: " + swhy);
                        }
                    } else {
                        h->resize(at);
                    }
                }
            }
        }
    }
    if (!ok) {
        if (!why.empty()) plan_failure(dry_fail, ow, oh, tw, th, rx, ry, why);
        bh_ctx::SepPlan none;
        none.key = key;
        b->sep_plans.push_back(none);
        return none;
    }
    if (dry_fail) {
        P.host = h;
        P.dev = h->data();
    } else {
        hipError_t e = hipMalloc(&P.dev, h->size() * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(P.dev, h->data(), h->size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess && P.stc) e = hipMalloc(&P.strips, 3u * (size_t)P.stw * oh * 4u);
        if (e != hipSuccess) {
            if (P.dev) (void)hipFree(P.dev);
            if (P.strips) (void)hipFree(P.strips);
            *err = (int)e;
            bh_ctx::SepPlan none;
            none.key = key;
            return none;
        }
    }
    b->sep_plans.push_back(P);
    return P;
}

struct BloomRun {
    bh_ctx* c;
    bh_ctx::BloomScratch* B;
    bool capturing;
    hipStream_t s;
    std::string* dry_fail;  // bh_bloom_check's dry mode: plans on the host, launches checked, not launched
    int err = 0;
    void pass(uint32_t sh, const uint32_t* a, uint32_t aw, uint32_t ah, const uint32_t* b, const uint32_t* res,
              uint32_t* out, uint32_t ow, uint32_t oh) {
        if (err != 0) return;
        bh_ctx::SepPlan sp{};
        if (sh == bh_bloom_shader_up && bh_bloom_up_uses_sep(ow, oh, aw, ah, res[0], res[1]))
            sp = sep_plan(B, capturing, dry_fail, ow, oh, aw, ah, res[0], res[1], &err);
        if (err == 0)
            err = bh_launch_bloom_pass(sh, c->lut, c->enc, c->enc_b, c->enc_e, a, aw, ah, b, res[0], res[1], out, ow, oh,
                                       sp.dev, sp.ext, s);
    }
    // the fused chains' blur downsamples src (res[0]) -> down[1] -> ... -> down[levels - 1]; returns the
    // last level.  An intermediate level is read by nothing but the next downsample, so pairs run as one
    // pass (bh_launch_bloom_down2, the intermediate not stored); BH_BLOOM_NO_DOWN2 runs them one by one (A/B)
    // first = 3: the Y pass already wrote down[2] (bh_launch_bloom_y's fused down2)
    const uint32_t* downs(const uint32_t* src, uint32_t levels, uint32_t** down, const BloomPlan& P, uint32_t first = 1) {
        static const bool no_down2 = std::getenv("BH_BLOOM_NO_DOWN2") != nullptr;
        const uint32_t* dn = first == 3 ? down[2] : src;
        uint32_t l = first;
        for (; !no_down2 && l + 1 < levels && err == 0; l += 2) {
            err = bh_launch_bloom_down2(c->lut, c->enc, c->enc_b, c->enc_e, dn, P.res[l - 1][0], P.res[l - 1][1],
                                        P.res[l][0], P.res[l][1], down[l + 1], P.res[l + 1][0], P.res[l + 1][1], s);
            dn = down[l + 1];
        }
        for (; l < levels; ++l) {
            pass(bh_bloom_shader_down, dn, P.res[l - 1][0], P.res[l - 1][1], nullptr, P.res[l - 1], down[l], P.res[l][0],
                 P.res[l][1]);
            dn = down[l];
        }
        return dn;
    }
};

// bh_bloom's chain on scratch set B: the reference's passes one by one (literal) or the fused forms.
// dry_fail (bh_bloom_check): the plans stay on the host and the launchers check their launch instead of
// launching (bh_bloom.hip dry mode); the scratch pointers are then placeholders that nothing dereferences.
int bloom_chain(bh_ctx* c, bh_ctx::BloomScratch* B, bool capturing, std::string* dry_fail, const void* col,
                const void* blackout, uint32_t W, uint32_t H, uint32_t levels, uint32_t schedule, void* out,
                hipStream_t s) {
    const BloomPlan P = bloom_plan(W, H, levels);
    // AUTO: the fused chain when every same-size sample is exact (powers of two); else the general fused chain
    // (the remixes sample through the same-size plan; the same-size copies vanish where they are proven identities
    // on stored texels, same_size_identity, and run as same-size copy passes where not: 3840x2160, 3440x1440,
    // ...); the literal pass list when a plan is refused (or BH_BLOOM_NO_GENERAL_COPIES and a copy is not an
    // identity: the round-5 rule, A/B)
    const uint32_t wl = P.res[levels - 1][0], hl = P.res[levels - 1][1];
    const bool fused = schedule == BH_BLOOM_AUTO && same_size_exact(W) && same_size_exact(H) && same_size_exact(wl) &&
                       same_size_exact(hl);
    const bool id_full = same_size_identity(W, H), id_low = same_size_identity(wl, hl);
    static const bool no_copies = std::getenv("BH_BLOOM_NO_GENERAL_COPIES") != nullptr;
    const bool general = schedule == BH_BLOOM_AUTO && !fused && (!no_copies || (id_full && id_low));
    bh_ctx::SepPlan same;
    uint32_t** T = B->tex.data();
    uint32_t **copy_in = T, **remix_in0 = T + levels, **remix_in1 = T + 2 * levels;
    uint32_t* blur_in = T[3 * levels];
    uint32_t* final_in1 = T[3 * levels + 1];
    uint32_t **down = T + 3 * levels + 2, **up = T + 4 * levels + 2;
    const uint32_t* X = (const uint32_t*)blackout;
    const uint32_t* C = (const uint32_t*)col;
    uint32_t* O = (uint32_t*)out;
    const uint32_t full[2] = {W, H};
    BloomRun R{c, B, capturing, s, dry_fail};
    const uint32_t L = levels - 1;
    if (fused) {
        // same-size passes are identities (same_size_identity): see bh_bloom.hip
        const uint32_t* S = X;
        bool d2 = false;  // the Y pass also wrote the blur's first two downsamples (down[2])
        if (levels > 1) {
            if (R.err == 0)
                R.err = bh_launch_bloom_y(c->lut, c->enc, c->enc_b, c->enc_e, X, copy_in[1], W, H,
                                          levels >= 3 ? down[2] : nullptr, &d2, s);
            S = copy_in[1];
        }
        // down[0] == S; up[levels-1] == down[levels-1]
        const uint32_t* u_src = R.downs(S, levels, down, P, d2 ? 3u : 1u);
        for (uint32_t l = 0; l + 1 < levels; ++l) {
            const uint32_t ti = levels - l - 2;
            R.pass(bh_bloom_shader_up, u_src, P.res[ti + 1][0], P.res[ti + 1][1], nullptr, P.res[l], up[ti],
                   P.res[ti][0], P.res[ti][1]);
            u_src = up[ti];
        }
        if (R.err == 0)
            R.err = bh_launch_bloom_final(c->lut, c->enc, c->enc_b, c->enc_e, C, S, u_src, P.res[L][0], P.res[L][1], O, W, H, s);
    } else if (general && (same = sep_plan(B, capturing, dry_fail, W, H, W, H, 0u, 0u, &R.err), same.dev != nullptr)) {
        // general fused chain (same-size passes are identities, same_size_identity): U1 = up(X) at full
        // size, Y = remix(X, U1) through the same-size plan, the blur's downsamples and upsamples from Y,
        // B = its last up pass, out = remix(col, q(remix(Y, B))) through the plan.  The two full-size
        // up passes with a separable plan carry the remixes as epilogues for the pixels whose column and
        // row sample exactly (bh_bloom.hip up_sep_kernel, EPI_Y / EPI_FINAL) and a fix-up pass covers the
        // inexact columns and rows; other plans run the plain pass and the plan remix kernels.
        const uint32_t* plan = same.dev;
        const uint32_t* list = plan ? plan + 2u * ((size_t)W + H) : nullptr;
        // an up pass at full size into `aux` with epilogue `epi` (own0, own1 its own-texel inputs), then the
        // fix-up of the inexact pixels -- or the plain pass and the remix kernel
        auto fused_up = [&](uint32_t epi, const uint32_t* src, uint32_t sw, uint32_t sh, const uint32_t* res,
                            uint32_t* aux, const uint32_t* own0, const uint32_t* own1, uint32_t* dst) {
            if (R.err != 0) return;
            bh_ctx::SepPlan sp{};
            if (bh_bloom_up_uses_sep(W, H, sw, sh, res[0], res[1]))
                sp = sep_plan(B, capturing, dry_fail, W, H, sw, sh, res[0], res[1], &R.err);
            if (R.err != 0) return;
            // the final epilogue writes the column strips its fix-up reads (bh_bloom.hip STRIPS)
            const uint32_t* stc = epi == 2u && same.stc ? plan + same.stc : nullptr;
            bool strips = false;
            if (sp.dev && bh_launch_bloom_sep(c->lut, c->enc, c->enc_b, c->enc_e, src, sw, sh, res[0], res[1], sp.dev,
                                              sp.ext, epi, own0, own1, plan, dst, aux, W, H, stc, same.strips, same.stw,
                                              &strips, s) == 0) {
                R.err = bh_launch_bloom_fixup(c->lut, c->enc, c->enc_b, c->enc_e, epi, own0, epi == 1u ? aux : own1, aux,
                                              plan, list, same.nc, same.nr, dst, W, H, plan + same.rec,
                                              strips ? stc : nullptr, same.strips, same.stw, s);
                return;
            }
            R.pass(bh_bloom_shader_up, src, sw, sh, nullptr, res, aux, W, H);
            if (R.err != 0) return;
            R.err = epi == 1u ? bh_launch_bloom_remix_plan(c->lut, c->enc, c->enc_b, c->enc_e, own0, aux, plan, dst, W, H, s)
                              : bh_launch_bloom_remix2_plan(c->lut, c->enc, c->enc_b, c->enc_e, own0, own1, aux, plan, dst,
                                                            W, H, s);
        };
        // A copy that is not an identity (same_size_identity) runs as the literal chain's pass: X1 = copy(X) (the
        // first loop's down[0] and remix_in0[0]), X2 = its same-size down (the blur of one level), S1 = copy(Y)
        // (the last blur's down[0] and remix_in0[L]), and the same-size down at the blur's smallest level.
        const uint32_t* S = X;  // levels 1: the loop never runs, the blur reads X itself
        if (levels > 1) {
            const uint32_t *X1 = X, *X2 = X;
            if (!id_full) {  // same_copy_kernel, twice
                if (R.err == 0)
                    R.err = bh_launch_bloom_same_copy(c->lut, c->enc, c->enc_b, c->enc_e, X, plan, remix_in0[0], W, H, s);
                if (R.err == 0)
                    R.err = bh_launch_bloom_same_copy(c->lut, c->enc, c->enc_b, c->enc_e, remix_in0[0], plan, blur_in, W, H, s);
                X1 = remix_in0[0];
                X2 = blur_in;
            }
            fused_up(1u, X2, W, H, full, remix_in1[0], X1, nullptr, copy_in[1]);
            S = copy_in[1];
        }
        if (!id_full) {
            if (R.err == 0)
                R.err = bh_launch_bloom_same_copy(c->lut, c->enc, c->enc_b, c->enc_e, S, plan, remix_in0[L], W, H, s);
            S = remix_in0[L];
        }
        const uint32_t* u_src = R.downs(S, levels, down, P);
        if (!id_low) {
            R.pass(bh_bloom_shader_down, u_src, wl, hl, nullptr, P.res[L], up[L], wl, hl);
            u_src = up[L];
        }
        for (uint32_t l = 0; l + 1 < levels; ++l) {
            const uint32_t ti = levels - l - 2;
            R.pass(bh_bloom_shader_up, u_src, P.res[ti + 1][0], P.res[ti + 1][1], nullptr, P.res[l], up[ti],
                   P.res[ti][0], P.res[ti][1]);
            u_src = up[ti];
        }
        const uint32_t uw = levels > 1 ? P.res[0][0] : W, uh = levels > 1 ? P.res[0][1] : H;  // up[0] is W x H
        fused_up(2u, u_src, uw, uh, P.res[L], remix_in1[L], C, S, O);
    } else if (R.err == 0) {
        // literal: the reference's render passes in order (also the general chain's fallback when the host
        // refuses its same-size plan) (oracle/bh_bloom_oracle.c, bho_bloom)
        hipError_t e;
        if (!dry_fail && (e = hipMemcpyAsync(copy_in[0], X, (size_t)W * H * 4u, hipMemcpyDeviceToDevice, s)) != hipSuccess)
            return hip_fail(e, "hipMemcpyAsync(bloom)");
        auto blur = [&](uint32_t lv, uint32_t* dst) {
            // blurs[k] with `lv` levels; its input (down[0]) was written by the copy pass
            for (uint32_t l = 1; l < lv; ++l)
                R.pass(bh_bloom_shader_down, down[l - 1], P.res[l - 1][0], P.res[l - 1][1], nullptr, P.res[l - 1],
                       down[l], P.res[l][0], P.res[l][1]);
            R.pass(bh_bloom_shader_down, down[lv - 1], P.res[lv - 1][0], P.res[lv - 1][1], nullptr, P.res[lv - 1],
                   up[lv - 1], P.res[lv - 1][0], P.res[lv - 1][1]);
            for (uint32_t l = 0; l + 1 < lv; ++l)
                R.pass(bh_bloom_shader_up, up[lv - l - 1], P.res[lv - l - 1][0], P.res[lv - l - 1][1], nullptr, P.res[l],
                       up[lv - l - 2], P.res[lv - l - 2][0], P.res[lv - l - 2][1]);
            R.pass(bh_bloom_shader_up, up[0], W, H, nullptr, P.res[lv - 1], dst, W, H);
        };
        for (uint32_t level = 0; level + 1 < levels; ++level) {
            R.pass(bh_bloom_shader_copy, copy_in[0], W, H, nullptr, full, down[0], W, H);
            R.pass(bh_bloom_shader_copy, copy_in[0], W, H, nullptr, full, remix_in0[0], W, H);
            blur(1, remix_in1[0]);
            R.pass(bh_bloom_shader_remix, remix_in0[0], W, H, remix_in1[0], full, copy_in[level + 1], W, H);
        }
        R.pass(bh_bloom_shader_copy, copy_in[L], W, H, nullptr, full, down[0], W, H);
        R.pass(bh_bloom_shader_copy, copy_in[L], W, H, nullptr, full, remix_in0[L], W, H);
        blur(levels, remix_in1[L]);
        R.pass(bh_bloom_shader_remix, remix_in0[L], W, H, remix_in1[L], full, final_in1, W, H);
        R.pass(bh_bloom_shader_remix, C, W, H, final_in1, full, O, W, H);
        (void)blur_in;
    }
    if (R.err != 0) return hip_fail((hipError_t)R.err, "bloom launch");
    return BH_OK;
}
}  // namespace

extern "C" {

int bh_bloom(bh_ctx* c, const void* col, const void* blackout, uint32_t W, uint32_t H, uint32_t levels,
             uint32_t schedule, void* out, void* stream) {
    // W, H <= 65536 as bh_render: the bloom kernels index texels with 32 bits (y * w + x < 2^32)
    if (!c || !col || !blackout || !out || W == 0 || H == 0 || W > 65536u || H > 65536u || levels < 1 || levels > 12 ||
        schedule > BH_BLOOM_LITERAL)
        return bad_arg(__func__, __LINE__);
    hipError_t e;
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    hipStream_t s = (hipStream_t)stream;
    const BloomPlan P = bloom_plan(W, H, levels);
    // scratch: [0, 3*levels) copy_in / remix_in0 / remix_in1 (full), then blur_in, final_in1 (full),
    // then down[levels], up[levels] at res[l]
    const uint64_t key = ((uint64_t)W << 40) ^ ((uint64_t)H << 16) ^ levels;
    const bool capturing = stream_capturing(s);
    bh_ctx::BloomScratch* B = nullptr;
    for (auto& b : c->blooms)
        if (b.key == key) B = &b;
    if (capturing) {
        // graph contract: nothing is allocated or uploaded under capture, and a set a graph uses is kept
        if (!B || !(B->prepared & (1u << schedule))) {
            bh_set_last_error("bh_bloom: the first call of a (size, levels, schedule) allocates; run it once before "
                              "capturing it into a graph");
            return BH_ERR_UNSUPPORTED;
        }
        B->captured = true;
    }
    if (!B) {
        bh_ctx::BloomScratch n;
        n.key = key;
        auto alloc = [&](size_t bytes) {
            uint32_t* t = nullptr;
            if ((e = hipMalloc(&t, bytes)) == hipSuccess) n.tex.push_back(t);
            return e == hipSuccess;
        };
        bool ok = true;
        for (uint32_t i = 0; ok && i < 3u * levels + 2u; ++i) ok = alloc((size_t)W * H * 4u);
        for (uint32_t k = 0; ok && k < 2; ++k)
            for (uint32_t l = 0; ok && l < levels; ++l) ok = alloc((size_t)P.res[l][0] * P.res[l][1] * 4u);
        if (!ok) {
            free_bloom_scratch(n);
            return alloc_fail(e, "hipMalloc(bloom)");
        }
        if (c->blooms.size() >= BH_BLOOM_SETS) {  // evict the least recently used set no graph holds
            size_t v = c->blooms.size();
            for (size_t i = 0; i < c->blooms.size(); ++i)
                if (!c->blooms[i].captured && (v == c->blooms.size() || c->blooms[i].last_use < c->blooms[v].last_use))
                    v = i;
            if (v < c->blooms.size()) {
                free_bloom_scratch(c->blooms[v]);
                c->blooms.erase(c->blooms.begin() + (long)v);
            }
        }
        c->blooms.push_back(std::move(n));
        B = &c->blooms.back();
    }
    B->last_use = ++c->bloom_clock;
    const int st = bloom_chain(c, B, capturing, nullptr, col, blackout, W, H, levels, schedule, out, s);
    if (st != BH_OK) return st;
    if (!capturing) B->prepared |= 1u << schedule;
    return BH_OK;
}

int bh_bloom_check(uint32_t W, uint32_t H, uint32_t levels, uint32_t schedule, uint64_t* out_launches, char* out_plan,
                   size_t plan_len) {
    if (W == 0 || H == 0 || W > 65536u || H > 65536u || levels < 1 || levels > 12 || schedule > BH_BLOOM_LITERAL)
        return bad_arg(__func__, __LINE__);
    bh_ctx c;  // no device: nothing below allocates, uploads or launches
    bh_ctx::BloomScratch B;
    for (uint32_t i = 0; i < 5u * levels + 2u; ++i) B.tex.push_back(reinterpret_cast<uint32_t*>((uintptr_t)(i + 1u) << 20));
    const void* in = reinterpret_cast<const void*>((uintptr_t)1 << 40);
    std::string fail, dfail, plan;
    uint64_t launches = 0, checks = 0;
    bh_bloom_dry_begin();
    const int st = bloom_chain(&c, &B, false, &fail, in, in, W, H, levels, schedule, const_cast<void*>(in), nullptr);
    const bool ok = bh_bloom_dry_end(&launches, &checks, &dfail, &plan);
    if (out_launches) *out_launches = launches;
    if (out_plan && plan_len) {
        const size_t n = std::min(plan.size(), plan_len - 1);
        std::memcpy(out_plan, plan.data(), n);
        out_plan[n] = '\0';
    }
    if (!ok || !fail.empty() || st != BH_OK) {
        bh_set_last_error("bh_bloom_check " + std::to_string(W) + "x" + std::to_string(H) + " levels " +
                          std::to_string(levels) + ": " + (!dfail.empty() ? dfail : !fail.empty() ? fail : bh_last_error()));
        return BH_ERR_INTERNAL;
    }
    return BH_OK;
}

int64_t bh_bloom_plan_failures(char* out_last, size_t len) {
    if (out_last && len) {
        while (g_plan_mu.test_and_set(std::memory_order_acquire)) std::this_thread::yield();
        const size_t n = std::min(g_plan_last.size(), len - 1);
        std::memcpy(out_last, g_plan_last.data(), n);
        out_last[n] = '\0';
        g_plan_mu.clear(std::memory_order_release);
    }
    return (int64_t)g_plan_failures.load();
}

}  // extern "C"
