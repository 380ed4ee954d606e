// bh_bloom_plan.hpp -- what the bloom's kernels (bh_bloom.hip), its host plan unit (bh_bloom_plan.cpp) and the
// chain (bh_bloom_host.cpp) share: the plan structs the kernels read, the tile constants the host checks against,
// the plan builders and the host-side bound checks with their dry run.  Plain C++, no HIP: bh_bloom_plan.cpp and
// tools/bloom_fixup_addr.cpp compile with any host compiler (the constexpr functions below are host and device
// functions to the HIP compiler as they stand).
#pragma once
#include <cstdint>
#include <string>

#pragma GCC visibility push(hidden)  // internal to the library
namespace bh {
namespace bloom {

// tap i's offset multiplier along an axis (Taps::du / dv: kawase_upsample.wgsl's (mx, my)), and floor / remainder
// in eighths (the standard plans, see quad_tap_std)
constexpr int tap_m(int axis, int i) { return (int)(((axis ? 0x10123432u : 0x12343210u) >> (4 * i)) & 15u) - 2; }
constexpr int fdiv8(int v) { return v >= 0 ? v / 8 : -((7 - v) / 8); }
constexpr int fmod8(int v) { return v - 8 * fdiv8(v); }

// The structured form of an 8-tap pass, proven by the host for every pixel of a launch (tap_plan): along each
// axis tap i's unclamped texel coordinate u*n - 0.5 equals x + o_i + f_i exactly, with an integer offset o_i and
// a weight f_i of 0 (point) or 1/2 (half).  The bilinear sample then reads texels clamp(x + o_i) and
// clamp(x + o_i + 1) at constant offsets, and its lerps reduce exactly: with weights 1/2 (products by 1/2 exact
// for the decoded texels, which are 0 or >= 2^-12)
//   (t0 * 0.5 + t1 * 0.5) == (t0 + t1) * 0.5,   both axes: ((t00 + t10) + (t01 + t11)) * 0.25,
// and with weight 0 the lerp returns t0 (t * 1 + t' * 0 == t).  Clamping agrees at the edges: a coordinate
// clamped to -1 or n has weight 0 and selects the edge texel, which both reads of a half tap then clamp to
// (t + t) * 0.5 == t).
struct TapPlan {
    int32_t ox[8], oy[8];
    uint32_t hx, hy;                 // bit i: tap i's weight along x (y) is 1/2, else 0
    int32_t lo_x, hi_x, lo_y, hi_y;  // the footprint's offsets: min o_i, max (o_i + half_i)
    uint32_t valid;
};
// The 2:1 form of an 8-tap pass (up2_kernel): per pixel parity and tap the texel offset and weight, and the
// interior where no tap is clamped.
struct Up2Plan {
    int32_t ox[2][8], oy[2][8];      // [pixel parity][tap]: floor(t) - (x >> 1)
    float fx[2][8], fy[2][8];        // t - floor(t)
    int32_t x_lo, x_hi, y_lo, y_hi;  // the interior's output pixels (inclusive; empty when lo > hi)
    uint32_t valid;
};
// Entry of a separable plan per tap and column (then per tap and row), see up_sep_kernel: the UNCLAMPED floor f
// of the sampler's coordinate t (t clamped to [-1, n] as sample_coord does, so f is in [-1, n]) and the weights
// fa = t - f (in [0, 1]: a t just below an integer rounds t - f up to 1), ia = 1 - fa.
struct SepEntry { int32_t f; float fa, ia; int32_t pad; };
static_assert(sizeof(SepEntry) == 16, "one ds_read_b128 per entry");
// the shape a TapPlan / Up2Plan is proven (and cached) for
struct PlanKey {
    uint32_t ow, oh, tw, th, rx, ry;
    bool operator==(const PlanKey& o) const {
        return ow == o.ow && oh == o.oh && tw == o.tw && th == o.th && rx == o.rx && ry == o.ry;
    }
};

// the render passes of the reference (include/bh_render.h's bh_bloom_shader values)
enum Shader : uint32_t { SH_COPY = 0, SH_DOWN = 1, SH_UP = 2, SH_REMIX = 3 };
// Epilogues of the separable up pass (up_sep_kernel / up_sepq_kernel)
enum SepEpi : uint32_t { EPI_PLAIN = 0, EPI_Y = 1, EPI_FINAL = 2 };

// ---- the kernels' LDS tiles: side FP, row stride FS --------------------------------------------------
constexpr int FP_UP = 24;     // staged footprint of a generic up pass (taps within a few texels)
constexpr int FP_Y = 24;      // blur1 at full size: taps within +-3 texels (22 x 22)
constexpr int FP_FINAL = 44;  // the last up pass at res / 4: taps within +-12 texels (42 x 42)
constexpr int FP_YQ = 40;     // bloom_yq_kernel: 32 + the taps' reach (38 at 4096x2048)
constexpr int FS_YQ = 40;     // its row stride (with the row-pair shift, see bloom_yq_kernel)
constexpr int FP_UPQ = 28;    // up2_kernel: footprint of 16 texels + the taps' reach (24 at 4096x2048)
constexpr int FS_UPQ = 32;    // its row stride in float4, a multiple of 16 (see up2_kernel)
// up_sep_kernel's row stride: a multiple of 16 float4 for the decoded tile (ds_read_b128 lane groups take two
// rows: see FS_YQ; in a same-size pass lane l reads column ~l & 15 of row ~l >> 4) and 16 mod 32 words for the
// raw one (ds_read_b32: lanes 0-15 row r, 16-31 row r + 1 land on the other banks)
template <int FP, bool RAW>
constexpr int sep_stride() { return RAW ? (FP + 16) / 32 * 32 + 16 : (FP + 15) / 16 * 16; }
// The quad kernel's raw 60-word tile's row stride (any stride keeps the quad rows' bank parity: the next quad
// row is 2 FS + 1 words further, an odd number).  64 instead of 80: 15 KiB of tile instead of 19
constexpr int SEPQ_FS60 = 64;

// The separable up pass's launch form for a plan's extents (low 16 bits: 16x16 blocks, high: 32x32): the quad
// kernel when its footprint fits a 28 / 40 / 60 tile (BH_BLOOM_NO_SEPQ, A/B: never), else the one-pixel kernel
// at 24 / 44, else none (FP 0: the general pass).  One definition for the launcher and its check.
struct SepForm {
    int FP = 0, FS = 0;
    bool quad = false, raw = false;
};
SepForm sep_form(int ext);

// ---- plans of an 8-tap pass, proven per shape and cached (a few per bloom chain) ------------------------
TapPlan tap_plan(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry);
Up2Plan up2_plan(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry);
// The standard plan (see quad_tap_std) a runtime plan equals, or 0: A = 12 or 3 for a 2:1 up pass, A = 12 or 48
// for a same-size TapPlan pass.  BH_BLOOM_NO_STD (A/B) disables them.
int std_up2_plan(const Up2Plan& P);
int std_tap_plan(const TapPlan& P);
// A/B switches of bh_launch_bloom_pass: BH_BLOOM_NO_UP2 (the general up pass instead of the 2:1 form),
// BH_BLOOM_NO_SEP (the per-pixel sampler instead of the separable plan)
bool up2_enabled();
bool sep_enabled();

// ---- a launcher's dry-run branch (bh_bloom_dry()): note the launch and check its form's every index --------
// Each takes what its launcher takes (plans are host copies in dry mode) and returns whether the launch is sound.
bool check_sep_launch(uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t rx, uint32_t ry, const uint32_t* sep,
                      int ext, uint32_t epi, const uint32_t* same, const uint32_t* stc, uint32_t strip_w);
bool check_fixup_launch(uint32_t epi, uint32_t w, uint32_t h, const uint32_t* same, const uint32_t* list, uint32_t n_cols,
                        uint32_t n_rows, const uint32_t* recs, const uint32_t* stc, uint32_t strip_w);
bool check_down2_launch(uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t mw, uint32_t mh);
// remix_plan_kernel, same_copy_kernel, remix2_plan_kernel: `form` names the launch
bool check_same_launch(const char* form, uint32_t w, uint32_t h, const uint32_t* plan);
bool check_up2_launch(const Up2Plan& Q, uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t rx, uint32_t ry);
bool check_pass_launch(uint32_t shader, const TapPlan& P, uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t rx,
                       uint32_t ry);
bool check_y_launch(const TapPlan& P, bool quad, bool d2, uint32_t w, uint32_t h);
bool check_final_launch(const TapPlan& P, uint32_t w, uint32_t h, uint32_t rx, uint32_t ry);

}  // namespace bloom
}  // namespace bh

// ---- C linkage: shared with bh_bloom_host.cpp (and tools/bloom_fixup_addr.cpp) ---------------------------
extern "C" {
// The separable plan of an 8-tap pass: 8 * (ow + oh) entries of 4 words (SepEntry) into outp; returns the
// largest 16x16 block footprint side in the low 16 bits and the largest 32x32 one in the high ones, or -1
int bh_bloom_sep_plan(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry, uint32_t* outp);
// the same-size plan of a w x h frame: (w + h) uint2 entries (the plan remixes, the fused epilogues)
bool bh_bloom_same_plan(uint32_t w, uint32_t h, uint32_t* outp);
// the column strips' table of a same-size plan's inexact columns; returns the number of strip columns
uint32_t bh_bloom_strip_table(uint32_t w, const uint32_t* list, uint32_t nc, uint32_t* stc);
// the fix-up kernel's records of a list (8 words per entry: the index and the plan entries of it and its neighbours)
void bh_bloom_fixup_records(uint32_t w, uint32_t h, const uint32_t* plan, const uint32_t* list, uint32_t nc, uint32_t nr,
                            uint32_t* out);
// bit i: tap i samples texel centres exactly for every pixel of the pass
uint32_t bh_bloom_point_mask(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry);
// whether bh_launch_bloom_pass runs an up pass of this shape from its separable plan
bool bh_bloom_up_uses_sep(uint32_t ow, uint32_t oh, uint32_t aw, uint32_t ah, uint32_t rx, uint32_t ry);
// whether the Y quad pass can also run the blur's first two downsamples (bloom_yq_kernel's D2)
bool bh_bloom_down2_fusable(uint32_t w, uint32_t h);
// Host-side bound checks of the kernels' index arithmetic: a separable plan for the form bh_launch_bloom_sep
// takes, a same-size plan with its fix-up list, a list's records (and, with stc, the column strips); false with
// the first violation in *why.
bool bh_bloom_sep_verify(uint32_t ow, uint32_t oh, uint32_t tw, uint32_t th, uint32_t rx, uint32_t ry, const uint32_t* plan,
                         int ext, std::string* why);
bool bh_bloom_same_verify(uint32_t w, uint32_t h, const uint32_t* plan, uint32_t nc, uint32_t nr, std::string* why);
bool bh_bloom_records_verify(uint32_t w, uint32_t h, const uint32_t* plan, const uint32_t* list, uint32_t nc, uint32_t nr,
                             const uint32_t* rec, const uint32_t* stc, uint32_t strip_w, std::string* why);
// Dry mode (bh_bloom_check): between begin and end the bloom launchers check their launch instead of launching.
void bh_bloom_dry_begin(void);
bool bh_bloom_dry_end(uint64_t* launches, uint64_t* checks, std::string* fail, std::string* plan);
bool bh_bloom_dry(void);
}
#pragma GCC visibility pop
