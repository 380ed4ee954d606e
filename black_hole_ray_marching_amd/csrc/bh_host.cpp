// bh_host.cpp — C ABI of include/bh_render.h: the context and its tables, the skies, and the render dispatch
// (the march launches and what they learn from frame to frame, the lens shade).  No CPU rendering path exists
// here by design: bh_render runs the HIP kernel or fails with a status code.  The rest of the ABI's host side:
// bh_camera.cpp, bh_bloom_host.cpp, bh_tiles_host.cpp, bh_mirror.cpp, bh_present.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "bh_host.hpp"
#include "bh_srgb.hpp"
#include "bh_lens.hpp"
#include "bh_refine.hpp"
#include "bh_shutter.hpp"
#include "bh_ss.hpp"

namespace {
thread_local std::string g_last_error;
}
static void free_frame_table(bh_ctx::FrameTable& t);

// sRGB byte -> linear, in double (the Rgba8UnormSrgb decode; DESIGN.md "Normative arithmetic").
void srgb_lut(float lut[256]) {
    for (int i = 0; i < 256; ++i) {
        double c = (double)i / 255.0;
        lut[i] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
    }
}

// linear -> sRGB byte of a Bgra8UnormSrgb store: clamp to [0, 1] (NaN -> 0), the sRGB OETF in double,
// round half up (the normative encode, DESIGN.md "Output formats").
uint8_t srgb_encode_ref(float x) {
    if (!(x > 0.0f)) return 0;
    if (x >= 1.0f) return 255;
    const double v = (double)x;
    const double e = v <= 0.0031308 ? 12.92 * v : 1.055 * std::pow(v, 1.0 / 2.4) - 0.055;
    const double q = std::floor(e * 255.0 + 0.5);
    return (uint8_t)(q > 255.0 ? 255.0 : q);
}

namespace {

// Thresholds of the encode (bh_srgb.hpp): T[k] = the smallest float in (0, 1] with code >= k,
// found by bisection over the ordered bit patterns of positive floats.
void srgb_encode_table(float T[257]) {
    T[0] = 0.0f;
    for (int k = 1; k < 256; ++k) {
        uint32_t lo = 0u, hi = 0x3F800000u;  // code(lo) < k <= code(hi)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            float x;
            std::memcpy(&x, &mid, 4);
            if (srgb_encode_ref(x) >= k) hi = mid; else lo = mid;
        }
        std::memcpy(&T[k], &hi, 4);
    }
    T[256] = std::numeric_limits<float>::infinity();
}

}  // namespace

// The code-table form of the encoder (bh_srgb.hpp srgb_encode_code): false if a bucket held two thresholds
// (never, for the normative table: the form would not be exact).
extern "C" __attribute__((visibility("hidden"))) bool bh_srgb_code_table(const float* T, uint32_t* E) {
    bool ok = true;
    for (int i = 0; i < bh::SRGB_CODES; ++i) {
        const uint32_t hi = (bh::SRGB_BUCKET_BASE + (uint32_t)i) << bh::SRGB_BUCKET_SHIFT;
        float lo;
        std::memcpy(&lo, &hi, 4);
        int k = 0;  // code of the bucket's lower end
        while (k < 255 && lo >= T[k + 1]) ++k;
        uint32_t thr = 0x10000u;
        if (k < 255) {
            uint32_t tb;
            std::memcpy(&tb, &T[k + 1], 4);
            if ((tb >> 16) == (hi >> 16)) {
                thr = tb & 0xFFFFu;
                uint32_t t2 = 0;
                if (k < 254) std::memcpy(&t2, &T[k + 2], 4);
                if (k < 254 && (t2 >> 16) == (hi >> 16)) ok = false;
            }
        }
        if (i == 0 && thr != 0x10000u) ok = false;  // values below 2^-13 clamp to entry 0
        E[i] = (uint32_t)k | (thr << 15);
    }
    return ok;
}

extern "C" __attribute__((visibility("hidden"))) void bh_srgb_bucket_table(const float* T, uint8_t* B) {
    for (int i = 0; i < bh::SRGB_BUCKETS; ++i) {
        const uint32_t bits = (bh::SRGB_BUCKET_BASE + (uint32_t)i) << bh::SRGB_BUCKET_SHIFT;
        float lo;
        std::memcpy(&lo, &bits, 4);
        int k = 0;  // code of the bucket's lower end: the largest k with T[k] <= lo
        while (k < 255 && lo >= T[k + 1]) ++k;
        B[i] = (uint8_t)k;
    }
}

namespace {

// Screen row (in tiles) of the black hole's projection: solve C1 + l0 (C0 - C1) + l2 (C2 - C1) = -t ro0
// (t > 0) for the barycentrics of the pixel looking at the origin; py = 2 H l2 - 0.5.  Falls back to
// the middle row when the origin is behind the camera or the system is degenerate.
uint32_t bh_tile_row(const bh_camera_uniform* c, uint32_t height) {
    const double C0[3] = {c->world_tri[0][0], c->world_tri[0][1], c->world_tri[0][2]};
    const double C1[3] = {c->world_tri[1][0], c->world_tri[1][1], c->world_tri[1][2]};
    const double C2[3] = {c->world_tri[2][0], c->world_tri[2][1], c->world_tri[2][2]};
    const double A[3] = {C0[0] - C1[0], C0[1] - C1[1], C0[2] - C1[2]};
    const double B[3] = {C2[0] - C1[0], C2[1] - C1[1], C2[2] - C1[2]};
    const double P[3] = {c->pos[0], c->pos[1], c->pos[2]};  // l0 A + l2 B + t P = -C1
    auto det3 = [](const double* x, const double* y, const double* z) {
        return x[0] * (y[1] * z[2] - y[2] * z[1]) - y[0] * (x[1] * z[2] - x[2] * z[1]) + z[0] * (x[1] * y[2] - x[2] * y[1]);
    };
    const double R[3] = {-C1[0], -C1[1], -C1[2]};
    const double D = det3(A, B, P);
    const uint32_t tiles_y = (height + 7u) / 8u;
    if (std::fabs(D) < 1e-12) return tiles_y / 2u;
    const double l2 = det3(A, R, P) / D, t = det3(A, B, R) / D;
    if (!(t > 0.0)) return tiles_y / 2u;
    double py = 2.0 * height * l2 - 0.5;
    py = py < 0.0 ? 0.0 : (py > height - 1.0 ? height - 1.0 : py);
    return (uint32_t)(py / 8.0);
}

// The default screen triangle: the only one the kernels' pixel_ray inverts.
constexpr float SCREEN_TRI[3][2] = {{3.0f, 1.0f}, {-1.0f, 1.0f}, {-1.0f, -3.0f}};
bool screen_tri_default(const bh_camera_uniform* c) {
    for (int i = 0; i < 3; ++i)
        if (c->screen_tri[i][0] != SCREEN_TRI[i][0] || c->screen_tri[i][1] != SCREEN_TRI[i][1]) return false;
    return true;
}
// A camera that holds only the position (the ray-map renders: their kernels do not read the corner rays).
void position_camera(bh_camera_uniform* cam, const float* pos) {
    std::memset(cam, 0, sizeof *cam);
    for (int i = 0; i < 3; ++i) {
        cam->pos[i] = pos[i];
        cam->screen_tri[i][0] = SCREEN_TRI[i][0];
        cam->screen_tri[i][1] = SCREEN_TRI[i][1];
    }
}

}  // namespace

extern "C" {

int bh_abi_version(void) { return BH_ABI_VERSION; }

// for the other host translation units (bh_present.cpp)
__attribute__((visibility("hidden"))) void bh_set_last_error(const std::string& msg) { g_last_error = msg; }
__attribute__((visibility("hidden"))) int bh_bad_arg(const char* fn, int line) {
    g_last_error = std::string(fn) + ": invalid argument (line " + std::to_string(line) + ")";
    return BH_ERR_INVALID_ARG;
}
__attribute__((visibility("hidden"))) int bh_ctx_device(const bh_ctx* c) { return c->device; }

const char* bh_status_string(int st) {
    switch (st) {
        case BH_OK: return "ok";
        case BH_ERR_INVALID_ARG: return "invalid argument";
        case BH_ERR_UNSUPPORTED: return "unsupported";
        case BH_ERR_HIP: return "HIP runtime error";
        case BH_ERR_NO_DEVICE: return "no HIP device";
        case BH_ERR_OUT_OF_MEMORY: return "out of device memory";
        case BH_ERR_INTERNAL: return "internal consistency check failed";
        default: return "unknown status";
    }
}

const char* bh_last_error(void) { return g_last_error.c_str(); }

int bh_srgb_encode_table(float* out257) {
    if (!out257) return bad_arg(__func__, __LINE__);
    srgb_encode_table(out257);
    return BH_OK;
}

int64_t bh_div_magic_misses(uint32_t d, uint32_t n_max, uint32_t* magic) {
    if (d == 0u || !magic) return bad_arg(__func__, __LINE__);
    const uint32_t m = *magic = bh::div_magic(d, n_max);
    if (m == 0u) return 0;
    int64_t misses = 0;
    uint32_t n = 0;
    do misses += (uint32_t)(((uint64_t)n * m) >> 32) != n / d; while (n++ != n_max);
    return misses;
}

}  // extern "C"

// One of the context's device tables: allocated and, with `src`, filled.  A failure is labelled hipMalloc(what) or
// hipMemcpy(what); `malloc_fail` gives the failed allocation's status (alloc_fail: out of memory has its own).
template <class T>
static int upload(T** dst, const void* src, size_t bytes, const char* what, int (*malloc_fail)(hipError_t, const char*)) {
    hipError_t e = hipMalloc(dst, bytes);
    if (e != hipSuccess) return malloc_fail(e, (std::string("hipMalloc(") + what + ")").c_str());
    if (src && (e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(e, (std::string("hipMemcpy(") + what + ")").c_str());
    return BH_OK;
}

extern "C" {

int bh_create(const uint8_t* sky, uint32_t sky_w, uint32_t sky_h, int device, bh_ctx** out) {
    if (!sky || !out || sky_w == 0 || sky_h == 0 || sky_w > 32768u || sky_h > 32768u) return bad_arg(__func__, __LINE__);
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_last_error = "no HIP device"; return BH_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { g_last_error = "device index out of range"; return BH_ERR_NO_DEVICE; }
    DeviceScope dev(device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    bh_ctx* c = new (std::nothrow) bh_ctx();
    if (!c) return BH_ERR_OUT_OF_MEMORY;
    c->device = device;
    c->sky_w = sky_w;
    c->sky_h = sky_h;
    const size_t bytes = (size_t)sky_w * sky_h * 4u;
    float lut[256], enc[257];
    uint8_t enc_b[bh::SRGB_BUCKETS];
    uint32_t enc_e[bh::SRGB_CODES];
    srgb_lut(lut);
    srgb_encode_table(enc);
    bh_srgb_bucket_table(enc, enc_b);
    if (!bh_srgb_code_table(enc, enc_e)) {
        g_last_error = "sRGB code table";
        delete c;
        return BH_ERR_UNSUPPORTED;
    }
    int st = upload(&c->sky, sky, bytes, "sky", alloc_fail);
    if (st == BH_OK) st = upload(&c->lut, lut, sizeof(lut), "lut", hip_fail);
    if (st == BH_OK) st = upload(&c->enc, enc, sizeof(enc), "enc", hip_fail);
    if (st == BH_OK) st = upload(&c->enc_b, enc_b, sizeof(enc_b), "enc_b", hip_fail);
    if (st == BH_OK) st = upload(&c->enc_e, enc_e, sizeof(enc_e), "enc_e", hip_fail);
    if (st == BH_OK) st = upload(&c->counters, nullptr, 1024, "counters", hip_fail);
    if (st == BH_OK) {
        int cus = 0;
        if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess || cus <= 0) {
            st = hip_fail(e, "hipDeviceGetAttribute(CU count)");
        } else {
            c->cus = (uint32_t)cus;
            c->grid_exact = (uint32_t)(cus * bh_march_blocks_per_cu_exact());
            c->grid_fast = (uint32_t)(cus * bh_march_blocks_per_cu_fast());
        }
    }
    if (st != BH_OK) { bh_destroy(c); return st; }
    *out = c;
    return BH_OK;
}

int bh_destroy(bh_ctx* c) {
    if (!c) return BH_OK;
    DeviceScope dev(c->device);
    if (c->sky) (void)hipFree(c->sky);
    if (c->lut) (void)hipFree(c->lut);
    if (c->enc) (void)hipFree(c->enc);
    if (c->enc_b) (void)hipFree(c->enc_b);
    if (c->enc_e) (void)hipFree(c->enc_e);
    if (c->counters) (void)hipFree(c->counters);
    for (auto& o : c->orders) o.free_buffers();
    for (auto& b : c->blooms) free_bloom_scratch(b);
    for (auto& t : c->frame_tables) free_frame_table(t);
    for (bh_sky* k : c->skies) {
        (void)hipFree(k->texels);
        if (k->chain) (void)hipFree(k->chain);
        delete k;
    }
    for (bh_disc* k : c->discs) {
        (void)hipFree(k->texels);
        delete k;
    }
    delete c;
    return BH_OK;
}

int bh_graph_release(bh_ctx* c) {
    if (!c) return bad_arg(__func__, __LINE__);
    for (auto& o : c->orders) o.captured = false;
    for (auto& b : c->blooms) b.captured = false;
    return BH_OK;
}

// Which build of the exact kernels runs a launch (BH_SCHED_FLAG_ISSUE_ORDER / _LATENCY force one).  The
// source-order build issues the bulk of the steps faster; the machine-scheduled one, whose tail loop
// also runs the packed step, marches a lone wave's serial chain faster.  A launch is throughput-bound
// when its tiles in flight (all frames') outlast the capped rays' chains: about 384 tiles per CU at
// cap 512 (the bulk runs ~1.2 us per tile and CU, a cap-512 chain ~0.45 ms), scaled by the cap.
// Measured (A/B r02, profiles/r02/variants.log, ms per frame, source-order / scheduled): 4096x2048
// cap 512 one frame (512 tiles/CU) 0.644 / 0.687; its 1/8 shard 0.445 / 0.363; 8192x4096's 1/8 shard
// 0.61 / 0.39; cap 1000 camera C 0.957 / 0.737; 1920x1080 cap 256 0.253 / 0.205; in 8-frame launches
// cap 1000 0.669 / 0.698, 1920x1080 0.165 / 0.171, 8192x4096's 1/8 shard 0.322 / 0.337.
static bool march_variant_issue_order(const bh_render_desc* d, uint32_t n_tiles, uint32_t n_frames, uint32_t cus) {
    if (d->schedule & BH_SCHED_FLAG_ISSUE_ORDER) return true;
    if (d->schedule & BH_SCHED_FLAG_LATENCY) return false;
    const uint64_t tiles = (uint64_t)n_tiles * n_frames;
    return tiles * 512ull >= 384ull * (cus ? cus : 256u) * d->max_iters;
}

static void free_frame_table(bh_ctx::FrameTable& t) {
    for (uint32_t k = 0; k < bh_ctx::FRAME_RING; ++k) {
        if (t.done[k]) { (void)hipEventSynchronize(t.done[k]); (void)hipEventDestroy(t.done[k]); }
        if (t.host[k]) (void)hipHostFree(t.host[k]);
    }
    if (t.dev) (void)hipFree(t.dev);
    t = bh_ctx::FrameTable{};
}

// Stage the n frames' arguments in the device table of stream s (created at its first use): a pinned
// ring slot is filled once its previous copy has executed, then copied in on the stream, ahead of the
// order and march kernels that read it.  *dev receives the table.
static int stage_frame_table(bh_ctx* c, hipStream_t s, const bh::FrameArgs* frames, const bh::FirstStep* first,
                             uint32_t n, const bh::FrameArgs** dev) {
    if (stream_capturing(s)) {
        g_last_error = "bh_render_frames: more than 32 frames per call cannot be captured into a graph";
        return BH_ERR_UNSUPPORTED;
    }
    bh_ctx::FrameTable* t = nullptr;
    for (auto& x : c->frame_tables)
        if (x.stream == (void*)s) t = &x;
    if (!t) {
        bh_ctx::FrameTable n_t;
        n_t.stream = (void*)s;
        const size_t bytes = (sizeof(bh::FrameArgs) + sizeof(bh::FirstStep)) * BH_MAX_FRAMES;
        hipError_t he = hipMalloc(&n_t.dev, bytes);
        for (uint32_t k = 0; he == hipSuccess && k < bh_ctx::FRAME_RING; ++k) {
            he = hipHostMalloc(&n_t.host[k], bytes, hipHostMallocDefault);
            if (he == hipSuccess) he = hipEventCreateWithFlags(&n_t.done[k], hipEventDisableTiming);
        }
        if (he != hipSuccess) {
            free_frame_table(n_t);
            return alloc_fail(he, "frame table");
        }
        c->frame_tables.push_back(n_t);
        t = &c->frame_tables.back();
    }
    *dev = t->dev;
    // the same frames as the stream's previous table (a re-rendered camera path): nothing to copy,
    // the stream's earlier copy precedes this launch
    // (the frames' first-step records stand behind the n frames, where the kernels look for them: frame_table + n)
    const size_t fb = sizeof(bh::FrameArgs) * n, rb = sizeof(bh::FirstStep) * n;
    if (t->last.size() == n && std::memcmp(t->last.data(), frames, fb) == 0 &&
        std::memcmp(t->last_first.data(), first, rb) == 0)
        return BH_OK;
    const uint32_t k = t->next;
    t->next = (k + 1u) % bh_ctx::FRAME_RING;
    hipError_t he = hipEventSynchronize(t->done[k]);  // a never-recorded event is complete
    if (he == hipSuccess) {
        std::memcpy(t->host[k], frames, fb);
        std::memcpy(reinterpret_cast<unsigned char*>(t->host[k]) + fb, first, rb);
        he = hipMemcpyAsync(t->dev, t->host[k], fb + rb, hipMemcpyHostToDevice, s);
    }
    if (he == hipSuccess) he = hipEventRecord(t->done[k], s);
    if (he != hipSuccess) {
        t->last.clear();
        return hip_fail(he, "frame table upload");
    }
    t->last.assign(frames, frames + n);
    t->last_first.assign(first, first + n);
    return BH_OK;
}

// The temporal-order state of (geometry, shard, stream): found, or created (allocating; the LRU state
// is evicted beyond BH_ORDER_STATES).  New states start with all costs 0 and an empty histogram.
// Graph contract (include/bh_render.h): a state used by a launch captured into a graph is marked and
// never evicted (its buffers are what the graph's kernels read and write); when every state is marked
// the ctx keeps more than BH_ORDER_STATES instead of evicting one.  A capturing stream cannot create a
// state (the allocation and the reset are not capturable work): BH_ERR_UNSUPPORTED.
static int order_state(bh_ctx* c, const bh_render_desc* d, const bh::MarchLaunch& m, uint64_t nt, hipStream_t s,
                       bool capturing, bh_ctx::OrderState** out) {
    const bool from_map = m.dirs != nullptr;  // a ray-map launch's tile costs are its own
    const uint64_t pser = d->partition ? d->partition->serial : 0u;
    for (auto& o : c->orders)
        if (o.matches(d, pser, nt, s, from_map)) {
            o.last_use = ++c->order_clock;
            if (capturing) {
                if (!o.valid) {
                    g_last_error = "bh_render: this (geometry, shard, stream) must be rendered once outside graph capture";
                    return BH_ERR_UNSUPPORTED;
                }
                o.captured = true;
            }
            *out = &o;
            return BH_OK;
        }
    if (capturing) {
        g_last_error = "bh_render: the first render of a (geometry, shard, stream) allocates; render it once "
                       "before capturing it into a graph";
        return BH_ERR_UNSUPPORTED;
    }
    bh_ctx::OrderState n;
    n.width = d->width; n.height = d->height; n.shard_index = d->shard_index; n.shard_count = d->shard_count;
    n.partition = pser;
    n.n_tiles = nt;
    n.stream = (void*)s;
    n.ray_map = from_map;
    const size_t cw = bh::ORDER_WORDS * sizeof(uint32_t);
    hipError_t he;
    if ((he = hipMalloc(&n.tile_cost, nt)) != hipSuccess || (he = hipMalloc(&n.order, nt * sizeof(uint32_t))) != hipSuccess ||
        (he = hipMalloc(&n.counters, cw)) != hipSuccess) {
        if (n.tile_cost) (void)hipFree(n.tile_cost);
        if (n.order) (void)hipFree(n.order);
        return alloc_fail(he, "hipMalloc(temporal order)");
    }
    if (c->orders.size() >= BH_ORDER_STATES) {  // evict the least recently used state no graph holds
        size_t v = c->orders.size();
        for (size_t i = 0; i < c->orders.size(); ++i)
            if (!c->orders[i].captured && (v == c->orders.size() || c->orders[i].last_use < c->orders[v].last_use)) v = i;
        if (v < c->orders.size()) {
            auto& o = c->orders[v];
            o.free_buffers();
            c->orders.erase(c->orders.begin() + (long)v);
        }
    }
    n.last_use = ++c->order_clock;
    c->orders.push_back(n);
    *out = &c->orders.back();
    return BH_OK;
}

// Per-frame invariants with the oracle's op sequence (correctly rounded f32, no contraction):
// c_ps = ((-normalize(ro0)) * 1.5) * RS (src/black_hole_maybe.wgsl:294).
static void frame_args(const bh_camera_uniform* cam, float rs, const bh_render_desc* d, bh::FrameArgs* F) {
    for (int k = 0; k < 3; ++k) {
        F->pos[k] = cam->pos[k];
        F->c0[k] = cam->world_tri[0][k];
        F->c1[k] = cam->world_tri[1][k];
        F->c2[k] = cam->world_tri[2][k];
    }
    const float x = F->pos[0], y = F->pos[1], z = F->pos[2];
    const float len = std::sqrt((x * x + y * y) + z * z);
    const float n[3] = {x / len, y / len, z / len};
    for (int k = 0; k < 3; ++k) F->cps[k] = (-n[k] * 1.5f) * rs;
    F->out_col = d->out_col; F->out_blackout = d->out_blackout;
    F->dbg_n_rk = d->dbg_n_rk; F->dbg_fate = d->dbg_fate; F->dbg_steps = d->dbg_steps;
}

// A/B switch (diagnostics): BH_NO_FIRST_STEP set => no frame has a first-step record, every wave runs iteration 0
static bool first_step_disabled() {
    static const bool off = std::getenv("BH_NO_FIRST_STEP") != nullptr;
    return off;
}

// The frame's first-step record (bh_common.hpp, FirstStep): iteration 0 of the march loop up to k1's denominator, for
// ro = camera.pos, restated from bh_march_step.hpp's step_bf in its XOps<false> form -- IEEE f32, one rounding per op,
// in the device's association (this unit is built without contraction); tests/test_first_step_host.py ties it to the
// oracle's own iteration 0.  The record is valid (true) only where every guard of step_bf whose operands are
// frame-uniform holds and no exit of iteration 0 can fire, each comparison written so that a NaN fails it:
//   finite inputs, dtm > 0, rs > 0;  1.01 < r^2 <= 2^24 (the camera outside the unit sphere: no blackout at
//   iteration 0, `outside` becomes 1; and Q0 = r^5 <= 2^60 >= 2^-40, the division core's denominator domain);
//   sdf >= MIN_DIST (no surface);  2^-25 <= dt0 <= 2^13 (rd_half's and add2's premises);  dt0 <= max_dist (no
//   escape: travelled = 0 + dt0);  max_iters >= 2 (no cap).
// An invalid record is all zeros: Q0 == 0 is the mark the waves test.
static bool first_step_record(const float pos[3], const float cps[3], float rs, float dtm, float max_dist,
                              uint32_t scene_flags, uint32_t max_iters, bh::FirstStep* out) {
    *out = bh::FirstStep{0.0f, 0.0f, 0.0f};
    const float x = pos[0], y = pos[1], z = pos[2];
    const float in[8] = {x, y, z, cps[0], cps[1], cps[2], rs, dtm};
    for (float v : in)
        if (!std::isfinite(v)) return false;
    if (!(dtm > 0.0f) || !(rs > 0.0f) || !(max_iters >= 2u)) return false;
    const float r2 = (x * x + y * y) + z * z;                          // dot(ro, ro)
    if (!(r2 > 1.01f && r2 <= 0x1p24f)) return false;
    const float r0 = std::sqrt(r2);                                    // :271
    const float dtr = dtm * r0;
    // sdf (:119-123), as XOps::sdf_args / sdf_from form it; sdf_of_terms' rule for a disabled term
    const float rho = std::sqrt(x * x + z * z);
    const float disc = std::fmax(std::fmax(rho - 6.0f * rs, -(rho - 3.0f * rs)), std::fabs(y - 0.0f) - 0.02f);
    const float xx = x * x, yy = y * y;
    const float dz = -10.0f - z, zz = dz * dz;
    const float ty = 10.0f - std::fabs(y), tx = 10.0f - std::fabs(x);
    const float qy = (xx + ty * ty) + zz, qx = (tx * tx + yy) + zz;
    const float m = std::sqrt(std::fmin(qy, qx)) - 0.5f;
    float ds;
    if (!(scene_flags & BH_SCENE_MARKERS)) ds = (scene_flags & BH_SCENE_DISC) ? disc : INFINITY;
    else ds = (scene_flags & BH_SCENE_DISC) ? std::fmin(disc, m) : m;
    if (!(ds >= 0.001f)) return false;                                 // :286-288 (MIN_DIST)
    const float dx = cps[0] - x, dy = cps[1] - y, dzp = cps[2] - z;    // :294
    const float dps = std::sqrt((dx * dx + dy * dy) + dzp * dzp) - 0.075f;
    const float dist = std::fmin(ds, dps);                             // :299
    const float dt0 = std::fmin(dist * 0.9f, dtr);                     // :307-310
    if (!(dt0 >= 0x1p-25f && dt0 <= 0x1p13f) || !(dt0 <= max_dist)) return false;
    const float Q0 = (r2 * r2) * r0;                                   // pow(r2, 2.5) (:126)
    const float rq0 = 1.0f / Q0;
    if (!(Q0 >= 0x1p-40f && Q0 <= 0x1p60f)) return false;              // implied by r2's range; kept as the core states it
    *out = bh::FirstStep{dt0, Q0, rq0};
    return true;
}

int bh_first_step_host(const bh_camera_uniform* cam, const bh_uniforms* U, uint32_t scene_flags, uint32_t max_iters,
                       float* dt0, float* Q0, float* rq0) {
    if (!cam || !U) return 0;
    bh::FrameArgs F;
    bh_render_desc d{};
    frame_args(cam, U->rs, &d, &F);
    bh::FirstStep fs;
    const bool ok = first_step_record(F.pos, F.cps, U->rs, U->delta_time_mult, U->max_dist, scene_flags, max_iters, &fs);
    if (dt0) *dt0 = fs.dt0;
    if (Q0) *Q0 = fs.Q0;
    if (rq0) *rq0 = fs.rq0;
    return ok ? 1 : 0;
}

// ---- one march launch --------------------------------------------------------------------------------------
// What a render entry point asks for, as its caller passed it and nothing derived.  Every entry point but the
// adaptive pair fills one and calls render_request, which checks it in one order, whatever the form; the adaptive
// render fills one for its second pass.
enum : uint32_t { TAKES_DIRS = 1u, TAKES_ORGS = 2u, TAKES_LENS = 4u, TAKES_HITS = 8u, TAKES_ARRIVALS = 16u };
enum RaySource : uint32_t { PINHOLE, WORLD_MAP, POSED_MAP };
struct Request {
    const char* fn;                            // the entry point, for messages
    uint32_t n_frames = 1u, n_sub = 1u, ss = 1u;
    RaySource source = PINHOLE;                // which one of the next three the entry point takes
    const bh_camera_uniform* cams = nullptr;   // PINHOLE: n_frames * n_sub cameras
    const float* pos = nullptr;                // WORLD_MAP: a world-space ray map's one position
    const bh_ray_pose* poses = nullptr;        // POSED_MAP: a camera-space ray map's n_frames * n_sub poses
    const bh_uniforms* U = nullptr;
    const bh_render_desc* descs = nullptr;     // n_frames of them
    uint32_t takes = 0u;                       // TAKES_*: which of the next five the entry point has (each required)
    const float* dirs = nullptr;               // the ray map, 4-byte aligned
    const float* orgs = nullptr;               // the origin map, 4-byte aligned
    bh_lens_px* lens = nullptr;                // the lens, 8-byte aligned: written in place of target 0
    float* hits = nullptr;                     // the hit map, 4-byte aligned
    float* arrivals = nullptr;                 // the arrival map, 4-byte aligned (with a hit map)
    uint32_t n_cams() const { return n_frames * n_sub; }
    const void* rays() const { return source == PINHOLE ? (const void*)cams : source == WORLD_MAP ? (const void*)pos : (const void*)poses; }
    // bh_render(_frames): nothing but cameras and descs
    bool plain() const { return source == PINHOLE && !takes && ss == 1u && n_sub == 1u; }
};

// The launch of a checked request: check_launch leaves its desc and tile count, fill_args everything else; then
// either learned_order and launch_march (render_request) or launch_refine (bh_render_frames_adaptive's second pass).
// A supersampled render (ss = k > 1) is the launch of the virtual frame k*width x k*height -- geometry, order state,
// repeat-frame key and all -- with log2 k and the output width for the kernel's resolve epilogue.
struct Launch {
    bh_render_desc d;                  // the launch's desc: the virtual frame's (per-frame outputs stay in descs[i])
    bh::MarchArgs a;                   // the kernel argument
    std::vector<bh::FrameArgs> table;  // more than BH_INLINE_FRAMES frames: staged in the stream's device table
    std::vector<bh::FirstStep> first_table;  // ... and their first-step records, staged behind the table
    uint64_t n_tiles = 0;              // the shard's tiles
    bh::MarchLaunch m;                 // what the unit's launcher takes beside `a`: the maps, the shutter, the schedule
    const bh_ray_pose* poses = nullptr;  // the posed ray-map forms: one pose per camera (a.n_frames of them), else null
    bh_camera_uniform cam0;            // camera 0: the caller's, or a ray map's position-only camera (order centre, key)
};

// What a frame's per-tile costs (the march's step counts) depend on: the camera, the shader uniforms and the
// launch shape -- FNV-1a over those fields' bits (padding and the unused bg_brightness left out).  The
// outputs, their format and the sky do not change a step count.  A ray-map launch's rays are its map's: the map's
// address enters the key (its contents cannot: a map rewritten in place may meet a stale order, never other bytes),
// and so does every pose of a posed launch (after a marker: a posed launch is never taken for an unposed one), and
// an origin map's address beside the direction map's (after a marker of its own: a launch with origins is never
// taken for one without).  A hit map's address enters the same way: the march's step counts do not depend on it, but
// a launch that writes one is another launch of the frame, as one into another lens is not; and an arrival map's after
// the hit map's.
static uint64_t frame_cost_key(const bh_camera_uniform* cam, const bh_uniforms* U, const Launch& L) {
    const bh_render_desc* d = &L.d;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    };
    mix(cam->pos, sizeof(float) * 3);
    for (int k = 0; k < 3; ++k) mix(cam->world_tri[k], sizeof(float) * 3);
    for (int k = 0; k < 3; ++k) mix(cam->screen_tri[k], sizeof(float) * 3);
    mix(&U->rs, 4); mix(&U->delta_time_mult, 4); mix(&U->blackout_eh, 4); mix(&U->max_dist, 4);
    mix(&U->distortion_power, 4);
    const uint64_t pser = d->partition ? d->partition->serial : 0u;
    const uint32_t f[9] = {d->width, d->height, d->max_iters, d->scene_flags, d->math, d->layout, d->shard_index,
                           d->shard_count, d->schedule};
    mix(f, sizeof f);
    mix(&pser, sizeof pser);
    if (L.m.dirs) mix(&L.m.dirs, sizeof L.m.dirs);
    if (L.poses) {  // a.n_frames of them
        mix(&L.a.n_frames, sizeof L.a.n_frames);
        mix(L.poses, sizeof(bh_ray_pose) * L.a.n_frames);
    }
    if (L.m.orgs) {
        const uint32_t marker = 0x4F524947u;  // "ORIG"
        mix(&marker, sizeof marker);
        mix(&L.m.orgs, sizeof L.m.orgs);
    }
    if (L.m.hits) {
        const uint32_t marker = 0x48495453u;  // "HITS"
        mix(&marker, sizeof marker);
        mix(&L.m.hits, sizeof L.m.hits);
    }
    if (L.m.arrivals) {
        const uint32_t marker = 0x41525256u;  // "ARRV"
        mix(&marker, sizeof marker);
        mix(&L.m.arrivals, sizeof L.m.arrivals);
    }
    return h | 1u;  // never 0: 0 marks the fresh state's all-zero costs
}

static bool same_launch(const bh_render_desc* a, const bh_render_desc* b) {
    return a->width == b->width && a->height == b->height && a->max_iters == b->max_iters &&
           a->scene_flags == b->scene_flags && a->format == b->format && a->math == b->math &&
           a->layout == b->layout && a->shard_index == b->shard_index && a->shard_count == b->shard_count &&
           a->schedule == b->schedule && a->partition == b->partition;
}

int bh_render(bh_ctx* c, const bh_camera_uniform* cam, const bh_uniforms* U, const bh_render_desc* d,
              void* stream) {
    return bh_render_frames(c, 1u, cam, U, d, stream);
}

// The far-field radius of the root-free step (bh_march_step.hpp, step_bf): r^2 beyond which every SDF term of a step
// provably exceeds the root-free test's threshold T = RN(1.125 RN(dtm r) + 0.002) <= 1.1251 dtm R + 0.003
// (R = |p| exact; the roundings of r, dtm r and T are within 2^-21 of R).  For a point at distance R:
//   disc (:121)  >= R / sqrt2 - max(6 rs, 0.02)   (rho^2 + y^2 = R^2: rho or |y| is >= R / sqrt2, and the
//                                                 sdf is >= rho - 6 rs and >= |y| - 0.02)
//   markers      >= R - 10 sqrt2 - 0.5            (the four centres lie at 10 sqrt2 from the origin)
//   photon (:294) >= R - 1.5 rs - 0.075           (its centre lies at 1.5 rs)
// R0 = the largest R at which one of them meets 1.1251 dtm R + 0.003; beyond 1.01 R0 each exceeds the
// threshold by >= 0.01 R0 (0.7071 - 1.1251 dtm) > 0.001 absolute, far above the step's own rounding of
// those terms (relative 2^-21: a few 1e-5 at R ~ 40), so the computed distance exceeds T and the root-free
// test's chain gives dt == dtm r and no surface.  r^2 is compared as computed (within 2^-22 of R^2: inside
// the 1 % margin).  +inf (off) when dtm is too large for the disc bound to ever clear (dtm >= 0.62).
static float sdf_far_r2(float rs, float dtm) {
    const double k = 1.1251 * (double)dtm, a1 = std::sqrt(0.5) - k, a2 = 1.0 - k;
    if (!(a1 > 0.01) || !(rs > 0.0f)) return INFINITY;
    const double R0 = std::max({(std::max(6.0 * rs, 0.02) + 0.003) / a1, (10.0 * std::sqrt(2.0) + 0.5 + 0.003) / a2,
                                (1.5 * rs + 0.075 + 0.003) / a2});
    const double R = 1.01 * R0;
    return std::nextafter((float)(R * R), INFINITY);
}

// A/B switch (diagnostics): BH_NO_SDF_SKIP set => every step evaluates its SDF roots (bh_march_step.hpp, sdf_skip_slack)
static bool sdf_skip_disabled() {
    static const bool off = std::getenv("BH_NO_SDF_SKIP") != nullptr;
    return off;
}

// What the resolve in the wave does not cover (include/bh_render.h), checked on every frame's desc: what the
// launch needs instead, or null.  per_ray_dbg: the dbg_* outputs are allowed (a ray-map render that resolves nothing).
static const char* ss_needs(const bh_render_desc* descs, uint32_t n_frames, bool per_ray_dbg = false) {
    for (uint32_t i = 0; i < n_frames; ++i) {
        const bh_render_desc* e = &descs[i];
        const char* why = e->layout != BH_LAYOUT_ROWMAJOR      ? "a row-major output (BH_LAYOUT_ROWMAJOR)"
                          : e->shard_count != 1u               ? "the whole frame (shard_count 1)"
                          : e->partition                       ? "no partition"
                          : (e->schedule & 0xFFu) != BH_SCHED_TILE ? "the tile schedule (BH_SCHED_TILE)"
                          : !per_ray_dbg && (e->dbg_n_rk || e->dbg_fate || e->dbg_steps) ? "no dbg_* outputs (they are per ray, not per pixel)"
                                                               : nullptr;
        if (why) return why;
    }
    return nullptr;
}

// What the request's form refuses of its descs (BH_ERR_UNSUPPORTED): what it needs instead, or null.  A pinhole render
// that resolves in the wave (ss > 1, a shutter) needs what ss_needs lists; a lens and a ray map need it always, a lens
// no colour target, and both exact math.
static const char* request_needs(const Request& r) {
    if (r.plain()) return nullptr;
    const bool map = r.source != PINHOLE, lens = (r.takes & TAKES_LENS) != 0u;
    for (uint32_t i = 0; i < r.n_frames; ++i) {
        const bh_render_desc* e = &r.descs[i];
        // the two families' own predicates, kept as they are: a pinhole lens refuses every math but exact here (an
        // unknown one too); a ray map refuses fast math alone (an unknown one is check_launch's invalid argument)
        if (map && e->math == BH_MATH_FAST) return "exact math (BH_MATH_EXACT): a ray map has no fast-math kernels";
        if (!map && lens && e->math != BH_MATH_EXACT) return "exact math (BH_MATH_EXACT): fast math has no defined bits to promise";
        if (lens && (e->out_col || e->out_blackout)) return "no out_col or out_blackout (it writes only the lens)";
    }
    // a ray map's dbg_* outputs are per ray: allowed where bh_render_frames allows them (nothing resolved, no lens)
    return ss_needs(r.descs, r.n_frames, map && !lens && r.ss == 1u && r.n_sub == 1u);
}

// The checks of a launch's desc, cameras and tile count, after render_request's (or the adaptive render's) own; no HIP
// call.  Leaves the launch's desc and tile count in L.
static int check_launch(const bh_ctx* c, const Request& r, Launch* L) {
    const uint32_t n_frames = r.n_cams();  // a frame of the launch is a camera
    if (!c || !r.rays() || !r.U || !r.descs || n_frames == 0 || n_frames > BH_MAX_FRAMES) return bad_arg(r.fn, __LINE__);
    const bool lens = (r.takes & TAKES_LENS) != 0u;
    const bh_render_desc* const d0 = &r.descs[0];
    L->d = *d0;
    if (r.ss > 1u) { L->d.width *= r.ss; L->d.height *= r.ss; }
    if (lens) {  // bh_render's launch of the frame with the lens in place of target 0; the format word is not read
        L->d.format = BH_OUT_RGBA32F;
        L->d.out_col = r.lens;
    }
    const bh_render_desc* d = &L->d;
    if (!d->out_col) return bad_arg(r.fn, __LINE__);
    if (!frame_shape_ok(d->width, d->height, 1u)) return bad_arg(r.fn, __LINE__);
    if (d->max_iters == 0 || d->max_iters > 65535u) return bad_arg(r.fn, __LINE__);
    if (d->format > BH_OUT_BGRA8_SRGB || d->math > BH_MATH_FAST || d->layout > BH_LAYOUT_TILES_RGBM14) return bad_arg(r.fn, __LINE__);
    if ((d->schedule & 0xFFu) > BH_SCHED_PERSISTENT || (d->schedule & ~(0xFFu | BH_SCHED_FLAG_STATIC_ORDER | BH_SCHED_FLAG_ISSUE_ORDER | BH_SCHED_FLAG_LATENCY))) return bad_arg(r.fn, __LINE__);
    if (d->scene_flags & ~BH_SCENE_DEFAULT) return bad_arg(r.fn, __LINE__);
    if (d->shard_count == 0 || d->shard_index >= d->shard_count) return bad_arg(r.fn, __LINE__);
    if (d->layout == BH_LAYOUT_ROWMAJOR && d->shard_count != 1) return bad_arg(r.fn, __LINE__);
    for (uint32_t i = 0; i < n_frames; ++i) {
        const bh_render_desc* e = &r.descs[i / r.n_sub];
        if ((!lens && !e->out_col) || !same_launch(d0, e)) return bad_arg(r.fn, __LINE__);
        if (r.cams && !screen_tri_default(&r.cams[i])) { g_last_error = "non-default screen triangle"; return BH_ERR_UNSUPPORTED; }
    }
    const uint32_t sched = d->schedule & 0xFFu;
    if ((d->layout == BH_LAYOUT_TILES_RGBM || d->layout == BH_LAYOUT_TILES_RGBM14) && sched == BH_SCHED_PERSISTENT) {
        g_last_error = "BH_LAYOUT_TILES_RGBM(14) needs the tile or pair schedule";
        return BH_ERR_UNSUPPORTED;
    }
    if (d->layout == BH_LAYOUT_TILES_RGBM14 && d->format != BH_OUT_RGBA16F) {
        g_last_error = "BH_LAYOUT_TILES_RGBM14 packs RGBA16F only";
        return BH_ERR_UNSUPPORTED;
    }
    if (const bh_partition* P = d->partition) {
        if (P->width != d->width || P->height != d->height || P->shard_count != d->shard_count ||
            P->device != c->device || d->layout == BH_LAYOUT_ROWMAJOR) {
            g_last_error = "partition: frame size, shard count, device or layout do not match";
            return BH_ERR_INVALID_ARG;
        }
        if (sched != BH_SCHED_TILE) {
            g_last_error = "a weighted partition needs the tile schedule";
            return BH_ERR_UNSUPPORTED;
        }
        L->n_tiles = P->count[d->shard_index];
    } else {
        L->n_tiles = bh::shard_tile_count((d->width + 7u) / 8u, (d->height + 7u) / 8u, d->shard_index, d->shard_count);
    }
    // the launch's wave slots; the frames of another schedule than the tile schedule launch one by one
    if (L->n_tiles * (sched == BH_SCHED_TILE ? n_frames : 1u) > 0xFFFFFFF0ull) return bad_arg(r.fn, __LINE__);
    return BH_OK;
}

// The whole launch of a checked request: the kernel argument, the frames' table when they do not fit inline, the maps
// and the form's words.  Pure; no caller writes into L afterwards.  One FrameArgs entry per camera: frame f's outputs
// in every entry of its n_sub cameras (a shutter's writer wave reads its own camera's entry), the lens in place of
// target 0; a ray map's camera holds only its position -- the map kernels do not read the corner rays -- and a posed
// one its pose's basis rows in c0..c2, where march_slot's POSE form reads them.
static void fill_args(const bh_ctx* c, const Request& r, Launch* L) {
    const bh_uniforms* U = r.U;
    const bh_render_desc* descs = r.descs;
    const uint32_t n_frames = r.n_cams(), ss = r.ss;
    const bh_render_desc* d = &L->d;
    bh::MarchArgs& a = L->a;
    std::memset(&a, 0, sizeof(a));
    a.rs = U->rs; a.dtm = U->delta_time_mult; a.max_dist = U->max_dist; a.dp = U->distortion_power;
    a.blackout_eh = U->blackout_eh;
    a.skip_sdf = (U->delta_time_mult > 0.0f && U->rs > 0.0f && U->rs <= 8.0f && !sdf_skip_disabled()) ? 1u : 0u;
    a.far_r2 = a.skip_sdf ? sdf_far_r2(U->rs, U->delta_time_mult) : INFINITY;
    a.width = d->width; a.height = d->height; a.max_iters = d->max_iters; a.scene_flags = d->scene_flags;
    if (ss > 1u) a.ss_log2 = bh::ss::log2_k(ss);
    // the resolve's output width; the shutter kernels index the output through it at every ss
    if (ss > 1u || r.n_sub > 1u) a.ss_out_width = descs[0].width;
    a.lens = (r.takes & TAKES_LENS) ? 1u : 0u;
    a.format = d->format; a.layout = d->layout;
    a.shard_index = d->shard_index; a.shard_count = d->shard_count;
    a.tiles_x = (d->width + 7u) / 8u; a.tiles_y = (d->height + 7u) / 8u;
    if (const bh_partition* P = d->partition) a.tile_list = P->tile_list + P->offset[d->shard_index];
    a.n_tiles = (uint32_t)L->n_tiles;
    // centre-out dispatch blocks of ~one tile row of this shard, centred on the black hole's row
    a.order_block = (uint32_t)((L->n_tiles + a.tiles_y - 1u) / a.tiles_y);
    a.sky = c->sky; a.srgb_lut = c->lut; a.srgb_enc = c->enc; a.sky_w = c->sky_w; a.sky_h = c->sky_h;
    // k = (DP * RS) * -1.5 (:126); the per-frame fields (camera, c_ps, outputs)
    a.kfac = (a.dp * a.rs) * -1.5f;
    a.rw2 = 1.0f / (2.0f * (float)a.width);
    a.rh2 = 1.0f / (2.0f * (float)a.height);
    a.n_frames = n_frames;
    // the waves' two divisions by launch constants (bh_march_tile.hpp, slot_head): a slot by the frames, a tile
    // by the tiles of a row; the largest dividend of each is known here
    const uint64_t slots = L->n_tiles * n_frames;
    a.nf_magic = slots - 1u <= 0xFFFFFFFFull ? bh::div_magic(n_frames, (uint32_t)(slots - 1u)) : 0u;
    a.tx_magic = a.shard_count == 1u && a.n_tiles != 0u ? bh::div_magic(a.tiles_x, a.n_tiles - 1u) : 0u;
    a.clk = c->clk;
    a.clk_mask = c->clk_mask;
    L->m.schedule = d->schedule & 0xFFu;
    L->m.counters = c->counters;
    L->m.grid = d->math != BH_MATH_EXACT ? c->grid_fast : c->grid_exact;
    L->m.shutter_log2 = bh::shutter::log2_n(r.n_sub);
    L->m.dirs = r.dirs; L->m.orgs = r.orgs; L->m.hits = r.hits; L->m.arrivals = r.arrivals;
    L->poses = r.poses;
    if (n_frames > bh::BH_INLINE_FRAMES) L->table.resize(n_frames);
    bh::FrameArgs* fa = L->table.empty() ? a.frames : L->table.data();
    for (uint32_t i = 0; i < n_frames; ++i) {
        bh_camera_uniform of_map;
        if (!r.cams) position_camera(&of_map, r.pos ? r.pos : r.poses[i].pos);
        const bh_camera_uniform* cam = r.cams ? &r.cams[i] : &of_map;
        frame_args(cam, a.rs, &descs[i / r.n_sub], &fa[i]);
        if (a.lens) fa[i].out_col = r.lens;
        for (int k = 0; r.poses && k < 3; ++k) {
            fa[i].c0[k] = r.poses[i].r[k]; fa[i].c1[k] = r.poses[i].u[k]; fa[i].c2[k] = r.poses[i].f[k];
        }
        if (i == 0u) L->cam0 = *cam;
    }
    a.order_centre = bh_tile_row(&L->cam0, d->height);
    // the frames' first-step records, for the exact builds' tile-schedule kernels (the others never read them); the
    // records of a staged launch ride behind its table
    if (!L->table.empty()) L->first_table.assign(n_frames, bh::FirstStep{0.0f, 0.0f, 0.0f});
    bh::FirstStep* fs = L->table.empty() ? a.first : L->first_table.data();
    if (d->math == BH_MATH_EXACT && (d->schedule & 0xFFu) == BH_SCHED_TILE && !first_step_disabled())
        for (uint32_t i = 0; i < n_frames; ++i)
            (void)first_step_record(fa[i].pos, fa[i].cps, a.rs, a.dtm, a.max_dist, a.scene_flags, a.max_iters, &fs[i]);
    // frame 0's fields again in the argument itself: what the kernels of a one-frame launch read
    const bh::FrameArgs& F = fa[0];
    for (int k = 0; k < 3; ++k) {
        a.pos[k] = F.pos[k]; a.c0[k] = F.c0[k]; a.c1[k] = F.c1[k]; a.c2[k] = F.c2[k]; a.cps[k] = F.cps[k];
    }
    a.out_col = F.out_col; a.out_blackout = F.out_blackout;
    a.dbg_n_rk = F.dbg_n_rk; a.dbg_fate = F.dbg_fate; a.dbg_steps = F.dbg_steps;
}

// The frames' table of a launch of more than BH_INLINE_FRAMES frames, staged on the stream
static int stage_frames(bh_ctx* c, hipStream_t s, Launch* L) {
    if (L->table.empty()) return BH_OK;
    return stage_frame_table(c, s, L->table.data(), L->first_table.data(), L->a.n_frames, &L->a.frame_table);
}

// The dispatch order the tile schedule learned from this (geometry, shard, stream)'s last frame: a.order, and
// a.tile_cost / a.order_tot for the march to write the next frame's costs to (null: none written).  *os is
// the state, or null when the launch has none (another schedule, BH_SCHED_FLAG_STATIC_ORDER).
static int learned_order(bh_ctx* c, Launch* L, const bh_camera_uniform* cam0, const bh_uniforms* U, hipStream_t s,
                         bh_ctx::OrderState** out) {
    const bh_render_desc* d = &L->d;
    bh::MarchArgs& a = L->a;
    *out = nullptr;
    if ((d->schedule & 0xFFu) != BH_SCHED_TILE || (d->schedule & BH_SCHED_FLAG_STATIC_ORDER)) return BH_OK;
    // temporal order of this (geometry, shard, stream): allocated at its first render only
    bh_ctx::OrderState* os = nullptr;
    int st = order_state(c, d, L->m, L->n_tiles, s, stream_capturing(s), &os);
    if (st != BH_OK) return st;
    if (!os->valid) {
        // all costs 0 (one bucket, the uncounted last) and an empty histogram: consistent
        hipError_t he = hipMemsetAsync(os->counters, 0, bh::ORDER_WORDS * sizeof(uint32_t), s);
        if (he == hipSuccess) he = hipMemsetAsync(os->tile_cost, 0, L->n_tiles, s);
        if (he != hipSuccess) return hip_fail(he, "temporal order reset");
        os->valid = true;
        os->cost_key = 0u;
        os->order_key = ~0ull;
    }
    // The order build consumes the histogram the last march accumulated (and zeroes the counters), and
    // the march accumulates the next: at every launch boundary the counters hold the histogram of the
    // costs in tile_cost, also across graph replays, which repeat a captured launch as it was.  A launch
    // whose frame repeats the one the order was learned from (its key equals both the order's and the
    // costs') skips the pair: no build, and a march that writes no costs -- the pending histogram still
    // describes the unchanged costs.  The host's keys only decide the skip; a replay that changed the
    // buffers behind them costs at most a stale order, never a disagreement.  BH_ORDER_ALWAYS (A/B):
    // build and write on every launch, as before round 5.
    static const bool always = std::getenv("BH_ORDER_ALWAYS") != nullptr;
    const uint64_t key = frame_cost_key(cam0, U, *L);
    const bool repeat = !always && os->order_key == os->cost_key && os->cost_key == key;
    if (!repeat) {
        int oe = bh_launch_build_order(os->tile_cost, a.n_tiles, a.order_block, a.order_centre, os->counters,
                                       os->order, s);
        if (oe != 0) { os->valid = false; return hip_fail((hipError_t)oe, "order kernels"); }
        os->order_key = os->cost_key;
        os->cost_key = key;
    }
    a.order = os->order;
    a.tile_cost = repeat ? nullptr : os->tile_cost;
    a.order_tot = repeat ? nullptr : os->counters;
    *out = os;
    return BH_OK;
}

// ---- the march units: which serves a launch ------------------------------------------------------------------
// The build of a unit (build.py): the exact kernels in issue order or scheduled for latency, or the fast kernels.
enum MarchBuild : uint32_t { BUILD_ISSUE, BUILD_LAT, BUILD_FAST, N_BUILDS };
// The family of a launch: which source's kernels march it (bh_march.hpp).
enum MarchFamily : uint32_t { FAMILY_PLAIN, FAMILY_RAYS, FAMILY_POSE, FAMILY_ORG, FAMILY_HITS, FAMILY_ARRIVALS, N_FAMILIES };

// [family][build]: the unit's launcher; null: no such unit (the entry points refuse fast math for ray maps and lenses).
static constexpr MarchUnitFn* MARCH_UNITS[N_FAMILIES][N_BUILDS] = {
    /* FAMILY_PLAIN */ {bh_launch_unit_exact, bh_launch_unit_exact_lat, bh_launch_unit_fast},
    /* FAMILY_RAYS  */ {bh_launch_unit_exact_rays, bh_launch_unit_exact_rays_lat, nullptr},
    /* FAMILY_POSE  */ {bh_launch_unit_exact_rays_pose, bh_launch_unit_exact_rays_pose_lat, nullptr},
    /* FAMILY_ORG   */ {bh_launch_unit_exact_rays_org, bh_launch_unit_exact_rays_org_lat, nullptr},
    /* FAMILY_HITS  */ {bh_launch_unit_exact_hits, bh_launch_unit_exact_hits_lat, nullptr},
    /* FAMILY_ARRIVALS */ {bh_launch_unit_exact_arr, bh_launch_unit_exact_arr_lat, nullptr},  // the hit-map units' second
};
// the work-list march: the plain family's units, the scheduled build's in a unit of its own (bh_march_exact.hip)
static constexpr RefineUnitFn* REFINE_UNITS[N_BUILDS] = {bh_launch_refine_unit_exact, bh_launch_refine_unit_exact_lat_refine,
                                                         bh_launch_refine_unit_fast};
static constexpr bool exact_units_filled() {
    for (uint32_t f = 0; f < N_FAMILIES; ++f)
        if (!MARCH_UNITS[f][BUILD_ISSUE] || !MARCH_UNITS[f][BUILD_LAT]) return false;
    return true;
}
static_assert(exact_units_filled(), "every family has both exact builds");

// The most specific form first: a launch with an arrival map always has a hit map, one with a hit map may also be posed and have a ray map (the hit-map kernels take
// both forms), one with an origin map is always posed, and a posed one always has a ray map -- so each test must come
// before those of the fields it implies.
static MarchFamily march_family(const Launch& L) {
    return L.m.arrivals ? FAMILY_ARRIVALS  // bh_march_lens_arrivals; posed: L.m.dirs
           : L.m.hits ? FAMILY_HITS   // one frame's lens (bh_render_lens_hits; posed: L.m.dirs)
           : L.m.orgs ? FAMILY_ORG    // no shutter form (bh_render_frames_rays_origins and its lens)
           : L.poses  ? FAMILY_POSE   // a posed map; the shutter form when shutter_log2 != 0
           : L.m.dirs ? FAMILY_RAYS   // a world-space map (bh_render_rays)
                      : FAMILY_PLAIN; // the shutter march when shutter_log2 != 0, else by the schedule
}
static MarchBuild march_build(const bh_render_desc* d, bool issue) {
    return d->math != BH_MATH_EXACT ? BUILD_FAST : issue ? BUILD_ISSUE : BUILD_LAT;
}

// The march over every tile, by the launch's family's unit of one of the three builds.
static int launch_march(bh_ctx* c, const Launch& L, bh_ctx::OrderState* os, hipStream_t s) {
    const bh_render_desc* d = &L.d;
    const bh::MarchArgs& a = L.a;
    const bool issue = march_variant_issue_order(d, a.n_tiles, a.n_frames, c->cus);  // every camera's tiles
    MarchUnitFn* const unit = MARCH_UNITS[march_family(L)][march_build(d, issue)];
    if (!unit) {
        g_last_error = "march launch: this form has no kernels in the fast-math build";
        return BH_ERR_INTERNAL;
    }
    const int e = unit(a, L.m, s);
    if (e != 0) {
        // the costs and their histogram are written together by the march kernel; without it they
        // may disagree, so the next frame of this state starts the temporal order afresh
        if (os) os->valid = false;
        return hip_fail((hipError_t)e, "march kernel launch");
    }
    return BH_OK;
}

// In place of the march over every tile (bh_render_frames_adaptive): the detect kernel over the plain frames
// in the targets, and the march over the work list it leaves.
static int launch_refine(bh_ctx* c, const Launch& L, const bh::RefineArgs& R, hipStream_t s) {
    const bh_render_desc* d = &L.d;
    const bh::MarchArgs& a = L.a;
    // the work-list march pulls with one wave per SIMD slot (WG_WAVES = 1: 32 workgroups fill a CU), never
    // more waves than there could be items; a wave that finds no work left ends at once
    const uint64_t items = ((uint64_t)R.tiles_x * R.tiles_y * a.n_frames) << (2u * a.ss_log2);
    const uint32_t waves = (uint32_t)std::min<uint64_t>(items, 32ull * (c->cus ? c->cus : 256u));
    hipError_t he = hipMemsetAsync(R.ctr, 0, 2 * sizeof(uint32_t), s);  // the entry counts (the heads: detect)
    if (he == hipSuccess && R.refined) he = hipMemsetAsync(R.refined, 0, a.n_frames * sizeof(uint32_t), s);
    if (he != hipSuccess) return hip_fail(he, "work list reset");
    int e = bh_launch_refine_detect(a, R, s);
    if (e != 0) return hip_fail((hipError_t)e, "detect kernel launch");
    // The refined tiles are the frame's long chains (disc edge, photon ring), a fraction of the virtual frame's
    // tiles: the list's march is latency-bound where bh_render_ss of the same k is throughput-bound, so it
    // runs the scheduled build unless BH_SCHED_FLAG_ISSUE_ORDER asks for the other (measured: DESIGN.md §7f).
    // BH_REFINE_VARIANT_RULE (A/B): bh_render_ss's choice for the whole virtual frame instead.
    static const bool by_rule = std::getenv("BH_REFINE_VARIANT_RULE") != nullptr;
    const bool issue = by_rule ? march_variant_issue_order(d, a.n_tiles, a.n_frames, c->cus)
                               : (d->schedule & BH_SCHED_FLAG_ISSUE_ORDER) != 0u;
    e = REFINE_UNITS[march_build(d, issue)](a, R, waves, s);
    if (e != 0) return hip_fail((hipError_t)e, "work-list march launch");
    return BH_OK;
}

// order -> march: the tail of every launch but the adaptive render's second pass
static int march_in_order(bh_ctx* c, Launch* L, const bh_uniforms* U, void* stream) {
    if (L->a.n_tiles == 0) return BH_OK;
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int st = stage_frames(c, s, L);
    if (st != BH_OK) return st;
    bh_ctx::OrderState* os = nullptr;
    st = learned_order(c, L, &L->cam0, U, s, &os);
    if (st != BH_OK) return st;
    return launch_march(c, *L, os, s);
}

// ---- the render entry points (include/bh_render.h) -----------------------------------------------------------
// Every one of them but the adaptive pair: the request's checks in one order, then its launch.  The launch is the one
// bh_render_frames(_ss) makes of the n_frames * n_sub cameras -- geometry, order state, repeated-frame key (camera 0 of
// frame 0: the order it stands for is the same array of tiles whichever kernel walks it), frame table -- whatever
// marches it: the shutter kernels, a lens in place of target 0, a ray map's kernels (with an order state and a key of
// their own: the maps in the launch's record).
static int render_request(bh_ctx* c, const Request& r, void* stream) {
    auto misaligned = [](const void* p, uintptr_t to) { return !p || (reinterpret_cast<uintptr_t>(p) & (to - 1u)); };
    // 1. the pointers; a map or output the entry point takes is required, and aligned
    if (!c || !r.rays() || !r.U || !r.descs) return bad_arg(r.fn, __LINE__);
    if (((r.takes & TAKES_DIRS) && misaligned(r.dirs, 4u)) || ((r.takes & TAKES_ORGS) && misaligned(r.orgs, 4u)) ||
        ((r.takes & TAKES_HITS) && misaligned(r.hits, 4u)) || ((r.takes & TAKES_ARRIVALS) && misaligned(r.arrivals, 4u)) ||
        ((r.takes & TAKES_LENS) && misaligned(r.lens, 8u)))
        return bad_arg(r.fn, __LINE__);
    // 2. ss and n_sub; an origin map has no shutter form
    if (bh::ss::log2_k(r.ss) > 3u || bh::shutter::log2_n(r.n_sub) > bh::shutter::MAX_LOG2) return bad_arg(r.fn, __LINE__);
    if ((r.takes & TAKES_ORGS) && r.n_sub != 1u) return bad_arg(r.fn, __LINE__);
    // 3. the frame count: nothing beyond descs[0], cams[0] or poses[0] is read before it has passed
    if (r.n_frames == 0 || (uint64_t)r.n_frames * r.n_sub > BH_MAX_FRAMES) return bad_arg(r.fn, __LINE__);
    // 4. the frame shape
    if (!frame_shape_ok(r.descs[0].width, r.descs[0].height, r.ss)) return bad_arg(r.fn, __LINE__);
    // 5. what the form needs of its descs
    if (const char* why = request_needs(r)) {
        g_last_error = r.source != PINHOLE       ? std::string(r.fn) + ": a ray-map render needs "
                       : (r.takes & TAKES_LENS)  ? std::string(r.fn) + ": a lens render needs "
                       : r.n_sub > 1u            ? "bh_render_shutter: a shutter render (n_sub > 1) needs "
                                                 : "bh_render_ss: a supersampled render (ss > 1) needs ";
        g_last_error += std::string(why) + ".";
        return BH_ERR_UNSUPPORTED;
    }
    // 6. the launch's own
    Launch L;
    int st = check_launch(c, r, &L);
    if (st != BH_OK) return st;
    // only a plain request gets here with another schedule than the tile schedule: one launch per frame
    if (r.n_frames > 1u && (L.d.schedule & 0xFFu) != BH_SCHED_TILE) {
        Request one = r;
        one.n_frames = 1u;
        for (uint32_t i = 0; i < r.n_frames && st == BH_OK; ++i) {
            one.cams = &r.cams[i];
            one.descs = &r.descs[i];
            st = render_request(c, one, stream);
        }
        return st;
    }
    try {
        fill_args(c, r, &L);
    } catch (const std::bad_alloc&) {  // the frames' table of a launch of more than BH_INLINE_FRAMES cameras
        return BH_ERR_OUT_OF_MEMORY;
    }
    return march_in_order(c, &L, r.U, stream);
}

static Request request(const char* fn, uint32_t n_frames, uint32_t n_sub, const bh_uniforms* U,
                       const bh_render_desc* descs, uint32_t ss) {
    Request r{fn};
    r.n_frames = n_frames; r.n_sub = n_sub; r.ss = ss;
    r.U = U; r.descs = descs;
    return r;
}
static Request pinhole(const char* fn, uint32_t n_frames, uint32_t n_sub, const bh_camera_uniform* cams,
                       const bh_uniforms* U, const bh_render_desc* descs, uint32_t ss) {
    Request r = request(fn, n_frames, n_sub, U, descs, ss);
    r.cams = cams;
    return r;
}
// one frame of a world-space ray map, from `pos`
static Request world_map(const char* fn, const float* pos, const bh_uniforms* U, const bh_render_desc* d,
                         const float* dirs, uint32_t ss) {
    Request r = request(fn, 1u, 1u, U, d, ss);
    r.source = WORLD_MAP; r.pos = pos;
    r.takes = TAKES_DIRS; r.dirs = dirs;
    return r;
}
// n_frames * n_sub poses of a camera-space ray map
static Request posed_map(const char* fn, uint32_t n_frames, uint32_t n_sub, const bh_ray_pose* poses,
                         const bh_uniforms* U, const bh_render_desc* descs, const float* dirs, uint32_t ss) {
    Request r = request(fn, n_frames, n_sub, U, descs, ss);
    r.source = POSED_MAP; r.poses = poses;
    r.takes = TAKES_DIRS; r.dirs = dirs;
    return r;
}
static Request& with_lens(Request& r, bh_lens_px* out_lens) { r.takes |= TAKES_LENS; r.lens = out_lens; return r; }
static Request& with_hits(Request& r, float* out_hits) { r.takes |= TAKES_HITS; r.hits = out_hits; return r; }
static Request& with_arrivals(Request& r, float* out_arrivals) { r.takes |= TAKES_ARRIVALS; r.arrivals = out_arrivals; return r; }
static Request& with_origins(Request& r, const float* origins) { r.takes |= TAKES_ORGS; r.orgs = origins; return r; }

int bh_render_frames(bh_ctx* c, uint32_t n_frames, const bh_camera_uniform* cams, const bh_uniforms* U,
                     const bh_render_desc* descs, void* stream) {
    return render_request(c, pinhole(__func__, n_frames, 1u, cams, U, descs, 1u), stream);
}

int bh_render_ss(bh_ctx* c, const bh_camera_uniform* cam, const bh_uniforms* U, const bh_render_desc* d, uint32_t ss,
                 void* stream) {
    return bh_render_frames_ss(c, 1u, cam, U, d, ss, stream);
}

// ss == 1 is the plain call, its messages' name included
int bh_render_frames_ss(bh_ctx* c, uint32_t n_frames, const bh_camera_uniform* cams, const bh_uniforms* U,
                        const bh_render_desc* descs, uint32_t ss, void* stream) {
    if (ss == 1u) return bh_render_frames(c, n_frames, cams, U, descs, stream);
    return render_request(c, pinhole(__func__, n_frames, 1u, cams, U, descs, ss), stream);
}

// ---- shutter renders (include/bh_render.h; the mapping and the tree: bh_shutter.hpp) -----------------------
int bh_render_shutter(bh_ctx* c, uint32_t n_sub, const bh_camera_uniform* cams, const bh_uniforms* U,
                      const bh_render_desc* d, uint32_t ss, void* stream) {
    return bh_render_frames_shutter(c, 1u, n_sub, cams, U, d, ss, stream);
}

// n_sub == 1 is the ss call (an ss this call would refuse stays this call's to refuse)
int bh_render_frames_shutter(bh_ctx* c, uint32_t n_frames, uint32_t n_sub, const bh_camera_uniform* cams,
                             const bh_uniforms* U, const bh_render_desc* descs, uint32_t ss, void* stream) {
    if (n_sub == 1u && bh::ss::log2_k(ss) <= 3u) return bh_render_frames_ss(c, n_frames, cams, U, descs, ss, stream);
    return render_request(c, pinhole(__func__, n_frames, n_sub, cams, U, descs, ss), stream);
}

// ---- lens maps (include/bh_render.h; the shading of a record: bh_lens.hpp) and hit maps: the lens march also
// stores where its surface rays ended ----------------------------------------------------------------------------
int bh_render_lens(bh_ctx* c, const bh_camera_uniform* cam, const bh_uniforms* U, const bh_render_desc* d,
                   bh_lens_px* out_lens, void* stream) {
    Request r = pinhole(__func__, 1u, 1u, cam, U, d, 1u);
    return render_request(c, with_lens(r, out_lens), stream);
}

int bh_render_lens_hits(bh_ctx* c, const bh_camera_uniform* cam, const bh_uniforms* U, const bh_render_desc* d,
                        bh_lens_px* out_lens, float* out_hits, void* stream) {
    Request r = pinhole(__func__, 1u, 1u, cam, U, d, 1u);
    return render_request(c, with_hits(with_lens(r, out_lens), out_hits), stream);
}

// ... and with an arrival map beside it, the direction they ended with: the request of bh_render_lens_hits and one map
int bh_march_lens_arrivals(bh_ctx* c, const bh_camera_uniform* cam, const bh_uniforms* U, const bh_render_desc* d,
                            bh_lens_px* out_lens, float* out_hits, float* out_arrivals, void* stream) {
    Request r = pinhole(__func__, 1u, 1u, cam, U, d, 1u);
    return render_request(c, with_arrivals(with_hits(with_lens(r, out_lens), out_hits), out_arrivals), stream);
}

// ---- ray maps (include/bh_render.h): the caller's direction per pixel; world-space with one origin per frame, or
// posed (bh_ray_pose): one camera-space map, one pose per camera, and with an origin map an origin per ray (the ORG
// kernels form the photon-sphere centre per lane: FrameArgs::cps, filled as ever, is not read by them) ------------
int bh_render_rays(bh_ctx* c, const float pos[3], const bh_uniforms* U, const bh_render_desc* d, const float* dirs_dev,
                   uint32_t ss, void* stream) {
    return render_request(c, world_map(__func__, pos, U, d, dirs_dev, ss), stream);
}

int bh_render_lens_rays(bh_ctx* c, const float pos[3], const bh_uniforms* U, const bh_render_desc* d,
                        const float* dirs_dev, bh_lens_px* out_lens, void* stream) {
    Request r = world_map(__func__, pos, U, d, dirs_dev, 1u);
    return render_request(c, with_lens(r, out_lens), stream);
}

int bh_render_frames_rays(bh_ctx* c, uint32_t n_frames, const bh_ray_pose* poses, const bh_uniforms* U,
                          const bh_render_desc* descs, const float* dirs_dev, uint32_t ss, void* stream) {
    return render_request(c, posed_map(__func__, n_frames, 1u, poses, U, descs, dirs_dev, ss), stream);
}

int bh_render_frames_shutter_rays(bh_ctx* c, uint32_t n_frames, uint32_t n_sub, const bh_ray_pose* poses,
                                  const bh_uniforms* U, const bh_render_desc* descs, const float* dirs_dev, uint32_t ss,
                                  void* stream) {
    return render_request(c, posed_map(__func__, n_frames, n_sub, poses, U, descs, dirs_dev, ss), stream);
}

int bh_render_lens_rays_posed(bh_ctx* c, const bh_ray_pose* pose, const bh_uniforms* U, const bh_render_desc* d,
                              const float* dirs_dev, bh_lens_px* out_lens, void* stream) {
    Request r = posed_map(__func__, 1u, 1u, pose, U, d, dirs_dev, 1u);
    return render_request(c, with_lens(r, out_lens), stream);
}

int bh_render_lens_rays_posed_hits(bh_ctx* c, const bh_ray_pose* pose, const bh_uniforms* U, const bh_render_desc* d,
                                   const float* dirs_dev, bh_lens_px* out_lens, float* out_hits, void* stream) {
    Request r = posed_map(__func__, 1u, 1u, pose, U, d, dirs_dev, 1u);
    return render_request(c, with_hits(with_lens(r, out_lens), out_hits), stream);
}

int bh_march_lens_rays_posed_arrivals(bh_ctx* c, const bh_ray_pose* pose, const bh_uniforms* U, const bh_render_desc* d,
                                       const float* dirs_dev, bh_lens_px* out_lens, float* out_hits, float* out_arrivals,
                                       void* stream) {
    Request r = posed_map(__func__, 1u, 1u, pose, U, d, dirs_dev, 1u);
    return render_request(c, with_arrivals(with_hits(with_lens(r, out_lens), out_hits), out_arrivals), stream);
}

int bh_render_frames_rays_origins(bh_ctx* c, uint32_t n_frames, const bh_ray_pose* poses, const bh_uniforms* U,
                                  const bh_render_desc* descs, const float* dirs_dev, const float* origins_dev,
                                  uint32_t ss, void* stream) {
    Request r = posed_map(__func__, n_frames, 1u, poses, U, descs, dirs_dev, ss);
    return render_request(c, with_origins(r, origins_dev), stream);
}

int bh_render_lens_rays_origins(bh_ctx* c, const bh_ray_pose* pose, const bh_uniforms* U, const bh_render_desc* d,
                                const float* dirs_dev, const float* origins_dev, bh_lens_px* out_lens, void* stream) {
    Request r = posed_map(__func__, 1u, 1u, pose, U, d, dirs_dev, 1u);
    return render_request(c, with_lens(with_origins(r, origins_dev), out_lens), stream);
}

// bh_sky_create and bh_sky_create_mips: the texels, and with `mips` the chain built from them (a synchronous call)
static int sky_create(bh_ctx* c, const uint8_t* rgba8, uint32_t w, uint32_t h, bool mips, bh_sky** out, const char* fn) {
    if (!c || !rgba8 || !out || w == 0 || h == 0 || w > 32768u || h > 32768u) return bad_arg(fn, __LINE__);
    *out = nullptr;
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    bh_sky* k = new (std::nothrow) bh_sky();
    if (!k) return BH_ERR_OUT_OF_MEMORY;
    k->ctx = c;
    k->w = w;
    k->h = h;
    const size_t bytes = (size_t)w * h * 4u;
    hipError_t e = hipMalloc(&k->texels, bytes);
    if (e == hipSuccess) e = hipMemcpy(k->texels, rgba8, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && mips) {
        uint32_t off[bh::lens::MIP_MAX_LEVELS];
        const size_t texels = bh::lens::mip_offsets(w, h, off);
        e = hipMalloc(&k->chain, (texels ? texels : 1u) * sizeof(bh::lens::Half4));  // a 1x1 sky has no level >= 1
        if (e == hipSuccess) e = (hipError_t)bh_launch_sky_mips(k->texels, w, h, c->lut, k->chain, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        k->n_levels = bh::lens::mip_levels(w, h);
    }
    if (e != hipSuccess) {
        if (k->texels) (void)hipFree(k->texels);
        if (k->chain) (void)hipFree(k->chain);
        delete k;
        return alloc_fail(e, fn);
    }
    c->skies.push_back(k);
    *out = k;
    return BH_OK;
}

int bh_sky_create(bh_ctx* c, const uint8_t* rgba8, uint32_t w, uint32_t h, bh_sky** out) {
    return sky_create(c, rgba8, w, h, false, out, __func__);
}

int bh_sky_create_mips(bh_ctx* c, const uint8_t* rgba8, uint32_t w, uint32_t h, bh_sky** out) {
    return sky_create(c, rgba8, w, h, true, out, __func__);
}

int bh_sky_levels(const bh_sky* k, uint32_t* out) {
    if (!k || !out) return bad_arg(__func__, __LINE__);
    *out = k->n_levels;
    return BH_OK;
}

int bh_sky_read_level(const bh_sky* k, uint32_t level, uint32_t* out_w, uint32_t* out_h, void* host_out) {
    if (!k || !out_w || !out_h || level < 1u || level >= k->n_levels) return bad_arg(__func__, __LINE__);
    uint32_t off[bh::lens::MIP_MAX_LEVELS];
    bh::lens::mip_offsets(k->w, k->h, off);
    *out_w = bh::lens::mip_side(k->w, level);
    *out_h = bh::lens::mip_side(k->h, level);
    if (!host_out) return BH_OK;
    DeviceScope dev(k->ctx->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    const hipError_t e = hipMemcpy(host_out, static_cast<const bh::lens::Half4*>(k->chain) + off[level],
                                   (size_t)*out_w * *out_h * sizeof(bh::lens::Half4), hipMemcpyDeviceToHost);
    return e == hipSuccess ? BH_OK : hip_fail(e, "hipMemcpy(sky level)");
}

int bh_sky_destroy(bh_sky* k) {
    if (!k) return BH_OK;
    bh_ctx* c = k->ctx;
    DeviceScope dev(c->device);
    c->skies.erase(std::remove(c->skies.begin(), c->skies.end(), k), c->skies.end());
    (void)hipFree(k->texels);
    if (k->chain) (void)hipFree(k->chain);
    delete k;
    return BH_OK;
}

// what bh_shade_lens and bh_shade_lens_mip refuse alike
static bool shade_desc_ok(const bh_ctx* c, const bh_shade_desc* d) {
    if (!c || !d || !d->lens || !d->out_col || (reinterpret_cast<uintptr_t>(d->lens) & 7u)) return false;
    if (bh::ss::log2_k(d->ss) > 3u || !frame_shape_ok(d->width, d->height, d->ss) || d->format > BH_OUT_BGRA8_SRGB) return false;
    return !d->sky || d->sky->ctx == c;
}

// the arguments both shades share; sky: the desc's, or (bh_shade_lens only) the ctx's own
static void fill_shade_args(const bh_ctx* c, const bh_shade_desc* d, bh::LensShadeArgs* a) {
    a->lens = d->lens;
    a->sky = d->sky ? d->sky->texels : c->sky;
    a->sky_w = d->sky ? d->sky->w : c->sky_w;
    a->sky_h = d->sky ? d->sky->h : c->sky_h;
    a->srgb_lut = c->lut;
    a->srgb_enc = c->enc;
    a->out_col = d->out_col;
    a->out_blackout = d->out_blackout;
    a->width = d->width;
    a->height = d->height;
}

// Validation and one kernel launch: no allocation, no synchronisation, no state (capturable from the first call).
int bh_shade_lens(bh_ctx* c, const bh_shade_desc* d, void* stream) {
    if (!shade_desc_ok(c, d)) return bad_arg(__func__, __LINE__);
    bh::LensShadeArgs a;
    fill_shade_args(c, d, &a);
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    const int e = bh_launch_lens_shade(a, d->ss, d->format, reinterpret_cast<hipStream_t>(stream));
    if (e != 0) return hip_fail((hipError_t)e, "lens shade kernel launch");
    return BH_OK;
}

// The same contract; the chain and its offsets travel in the launch's arguments.
int bh_shade_lens_mip(bh_ctx* c, const bh_shade_desc* d, void* stream) {
    if (!shade_desc_ok(c, d) || !d->sky || d->sky->n_levels == 0u) return bad_arg(__func__, __LINE__);
    if (d->ss == 8u) {
        g_last_error = "bh_shade_lens_mip: ss = 8 is not built: the plain shade is at its register limit there, and "
                       "the filter is what replaces a large ss.";
        return BH_ERR_UNSUPPORTED;
    }
    bh::LensMipArgs a;
    fill_shade_args(c, d, &a);
    a.chain = d->sky->chain;
    a.n_levels = d->sky->n_levels;
    bh::lens::mip_offsets(a.sky_w, a.sky_h, a.level_off);
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    const int e = bh_launch_lens_shade_mip(a, d->ss, d->format, reinterpret_cast<hipStream_t>(stream));
    if (e != 0) return hip_fail((hipError_t)e, "filtered lens shade kernel launch");
    return BH_OK;
}

// ---- disc shades (include/bh_render.h; the colour of a record: bh_lens.hpp, shade_disc) -------------------
int bh_disc_create(bh_ctx* c, const uint8_t* rgba8, uint32_t n_phi, uint32_t n_r, bh_disc** out) {
    if (!c || !rgba8 || !out || n_phi == 0 || n_r == 0 || n_phi > 32768u || n_r > 32768u) return bad_arg(__func__, __LINE__);
    *out = nullptr;
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    bh_disc* k = new (std::nothrow) bh_disc();
    if (!k) return BH_ERR_OUT_OF_MEMORY;
    k->ctx = c;
    k->n_phi = n_phi;
    k->n_r = n_r;
    const size_t bytes = (size_t)n_phi * n_r * 4u;
    hipError_t e = hipMalloc(&k->texels, bytes);
    if (e == hipSuccess) e = hipMemcpy(k->texels, rgba8, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (k->texels) (void)hipFree(k->texels);
        delete k;
        return alloc_fail(e, __func__);
    }
    c->discs.push_back(k);
    *out = k;
    return BH_OK;
}

int bh_disc_destroy(bh_disc* k) {
    if (!k) return BH_OK;
    bh_ctx* c = k->ctx;
    DeviceScope dev(c->device);
    c->discs.erase(std::remove(c->discs.begin(), c->discs.end(), k), c->discs.end());
    (void)hipFree(k->texels);
    delete k;
    return BH_OK;
}

// bh_shade_lens's contract: validation and one kernel launch.
// The checks and the arguments both disc shades share.
static bool disc_desc_ok(const bh_ctx* c, const bh_shade_desc* d, const bh_disc_desc* dd) {
    if (!shade_desc_ok(c, d) || !dd) return false;
    if (!dd->hits || (reinterpret_cast<uintptr_t>(dd->hits) & 3u) || !dd->disc || dd->disc->ctx != c) return false;
    if (dd->scene_flags & ~BH_SCENE_DEFAULT) return false;
    return std::isfinite(dd->spin) && std::isfinite(dd->gain) && dd->gain >= 0.0f;
}
static void fill_disc_args(const bh_ctx* c, const bh_shade_desc* d, const bh_disc_desc* dd, bh::LensDiscArgs* a) {
    fill_shade_args(c, d, a);
    a->hits = dd->hits;
    a->disc = dd->disc->texels;
    a->n_phi = dd->disc->n_phi;
    a->n_r = dd->disc->n_r;
    a->rs = dd->rs;
    a->scene_flags = dd->scene_flags;
    a->spin = dd->spin;
    a->gain = dd->gain;
}

int bh_shade_lens_disc(bh_ctx* c, const bh_shade_desc* d, const bh_disc_desc* dd, void* stream) {
    if (!disc_desc_ok(c, d, dd)) return bad_arg(__func__, __LINE__);
    bh::LensDiscArgs a;
    fill_disc_args(c, d, dd, &a);
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    const int e = bh_launch_lens_shade_disc(a, d->ss, d->format, reinterpret_cast<hipStream_t>(stream));
    if (e != 0) return hip_fail((hipError_t)e, "disc shade kernel launch");
    return BH_OK;
}

// ---- beamed disc shades (include/bh_render.h; the factor of a disc hit: bh_lens.hpp, beam_factor) ----------
int bh_shade_lens_disc_beamed(bh_ctx* c, const bh_shade_desc* d, const bh_disc_desc* dd, const bh_beam_desc* bd,
                              void* stream) {
    if (!disc_desc_ok(c, d, dd) || !bd) return bad_arg(__func__, __LINE__);
    if (!bd->arrivals || (reinterpret_cast<uintptr_t>(bd->arrivals) & 3u)) return bad_arg(__func__, __LINE__);
    if ((bd->sense != 1 && bd->sense != -1) || !(bd->beam >= 0.0f && bd->beam <= 1.0f) || !std::isfinite(bd->distortion_power))
        return bad_arg(__func__, __LINE__);
    bh::LensBeamArgs a;
    fill_disc_args(c, d, dd, &a);
    a.arrivals = bd->arrivals;
    a.beam = bd->beam;
    a.sense = (float)bd->sense;
    a.dp = bd->distortion_power;
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    const int e = bh_launch_lens_shade_disc_beamed(a, d->ss, d->format, reinterpret_cast<hipStream_t>(stream));
    if (e != 0) return hip_fail((hipError_t)e, "beamed disc shade kernel launch");
    return BH_OK;
}

// ---- adaptive supersampling (include/bh_render.h; the rule and the work list: bh_refine.hpp) ------------
static_assert(bh::refine::FMT_RGBA32F == BH_OUT_RGBA32F && bh::refine::FMT_RGBA16F == BH_OUT_RGBA16F &&
                  bh::refine::FMT_BGRA8 == BH_OUT_BGRA8_SRGB, "bh_refine.hpp's formats are the ABI's");

// The state of (geometry, whole frame, stream) if it exists (order_state's key, nothing created).
static bh_ctx::OrderState* find_order_state(bh_ctx* c, const bh_render_desc* d, uint64_t nt, hipStream_t s) {
    for (auto& o : c->orders)
        if (o.matches(d, 0u, nt, s)) return &o;  // no partition: an adaptive render takes none (ss_needs)
    return nullptr;
}

int bh_render_adaptive(bh_ctx* c, const bh_camera_uniform* cam, const bh_uniforms* U, const bh_render_desc* d,
                       const bh_adaptive_desc* ad, void* stream) {
    return bh_render_frames_adaptive(c, 1u, cam, U, d, ad, stream);
}

int bh_render_frames_adaptive(bh_ctx* c, uint32_t n_frames, const bh_camera_uniform* cams, const bh_uniforms* U,
                              const bh_render_desc* descs, const bh_adaptive_desc* ad, void* stream) {
    static const char* const fn = "bh_render_adaptive";
    if (!c || !cams || !U || !descs || !ad || n_frames == 0 || n_frames > BH_MAX_FRAMES) return bad_arg(fn, __LINE__);
    const uint32_t ss = ad->ss, lk = bh::ss::log2_k(ss);
    if (lk < 1u || lk > 3u) return bad_arg(fn, __LINE__);
    if (!(ad->threshold >= 0.0f) || std::isinf(ad->threshold)) return bad_arg(fn, __LINE__);  // NaN fails the >=
    const bh_render_desc* d = &descs[0];
    if (!frame_shape_ok(d->width, d->height, ss)) return bad_arg(fn, __LINE__);
    if (const char* why = ss_needs(descs, n_frames)) {
        g_last_error = std::string(fn) + ": an adaptive render needs " + why + ".";
        return BH_ERR_UNSUPPORTED;
    }
    const uint32_t tiles_x = bh::refine::tiles_of(d->width), tiles_y = bh::refine::tiles_of(d->height);
    const uint64_t nt = (uint64_t)tiles_x * tiles_y;
    // the work items of a fully refined call, and the virtual frame's slots as bh_render_ss counts them
    if (((nt * n_frames) << (2u * lk)) > 0xFFFF0000ull ||
        (uint64_t)bh::refine::tiles_of(d->width * ss) * bh::refine::tiles_of(d->height * ss) * n_frames > 0xFFFFFFF0ull)
        return bad_arg(fn, __LINE__);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    bool capturing;
    {
        DeviceScope dev(c->device);
        if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
        capturing = stream_capturing(s);
    }
    if (capturing) {
        // nothing may be allocated: refused before pass 1 is queued, so the targets stay as they are
        bh_ctx::OrderState* os = find_order_state(c, d, nt, s);
        if (!os || os->refine_frames < n_frames) {
            g_last_error = std::string(fn) + ": the first adaptive render of a (geometry, stream), or of more frames "
                           "than before, allocates; render it once before capturing it into a graph";
            return BH_ERR_UNSUPPORTED;
        }
    }
    // pass 1: the plain frame, exactly bh_render_frames (every remaining argument check is its own)
    int st = bh_render_frames(c, n_frames, cams, U, descs, stream);
    if (st != BH_OK) return st;
    DeviceScope dev(c->device);
    if (dev.err != hipSuccess) return hip_fail(dev.err, "hipSetDevice");
    bh_ctx::OrderState* os = nullptr;
    if (capturing) {
        os = find_order_state(c, d, nt, s);  // pass 1 creates no state under capture: still there
        if (!os) return bad_arg(fn, __LINE__);
        os->captured = true;
        os->last_use = ++c->order_clock;
    } else {
        // pass 1's own (a plain launch's: no map), or (BH_SCHED_FLAG_STATIC_ORDER) a new one
        st = order_state(c, d, bh::MarchLaunch{}, nt, s, false, &os);
        if (st != BH_OK) return st;
        if (os->refine_frames < n_frames && os->captured) {
            g_last_error = std::string(fn) + ": a captured graph holds this (geometry, stream)'s work list, which is "
                           "too small for this many frames (bh_graph_release once the graph is destroyed)";
            return BH_ERR_UNSUPPORTED;
        }
        if (os->refine_frames < n_frames) {
            uint32_t* list = nullptr;
            uint32_t* ctr = nullptr;
            uint8_t* mask = nullptr;
            const size_t entries = (size_t)nt * n_frames;
            hipError_t he;
            if ((he = hipMalloc(&list, entries * bh::refine::ENTRY_WORDS * sizeof(uint32_t))) != hipSuccess ||
                (he = hipMalloc(&ctr, bh::REFINE_CTR_WORDS * sizeof(uint32_t))) != hipSuccess || (he = hipMalloc(&mask, entries)) != hipSuccess) {
                (void)hipFree(list); (void)hipFree(ctr);
                return alloc_fail(he, "hipMalloc(work list)");
            }
            // hipFree waits for the device: no earlier call's kernels still use the smaller buffers
            (void)hipFree(os->refine_list); (void)hipFree(os->refine_ctr); (void)hipFree(os->refine_mask);
            os->refine_list = list; os->refine_ctr = ctr; os->refine_mask = mask;
            os->refine_frames = n_frames;
        }
    }
    bh::RefineArgs R;
    std::memset(&R, 0, sizeof R);
    R.list = os->refine_list; R.ctr = os->refine_ctr;
    R.mask = ad->tile_mask ? ad->tile_mask : os->refine_mask;
    R.refined = ad->refined_tiles;
    // pass 1 left frame 0's tile costs in the state (or, for a repeated frame, found them there): the list's order
    static const bool unordered = std::getenv("BH_REFINE_UNORDERED") != nullptr;  // A/B switch (diagnostics)
    R.tile_cost = (os->valid && !(d->schedule & BH_SCHED_FLAG_STATIC_ORDER) && !unordered) ? os->tile_cost : nullptr;
    R.width = d->width; R.height = d->height; R.tiles_x = tiles_x; R.tiles_y = tiles_y;
    R.n_frames = n_frames;
    R.capacity = (uint32_t)std::min<uint64_t>(nt * os->refine_frames, 0xFFFFFFFFull);
    static const bool one_head = std::getenv("BH_REFINE_ONE_HEAD") != nullptr;  // A/B switch (diagnostics)
    R.n_heads = one_head ? 1u : bh::REFINE_HEADS;
    R.thr = bh::refine::threshold(d->format, ad->threshold);
    // pass 2: the virtual frame's launch, over the tiles the detect pass lists
    const Request r = pinhole(fn, n_frames, 1u, cams, U, descs, ss);
    Launch L;
    st = check_launch(c, r, &L);
    if (st != BH_OK) return st;
    fill_args(c, r, &L);
    if (L.a.n_tiles == 0) return BH_OK;
    st = stage_frames(c, s, &L);
    if (st != BH_OK) return st;
    return launch_refine(c, L, R, s);
}

int bh_set_clock_probe(bh_ctx* c, uint64_t* acc, uint32_t stride) {
    if (!c || (acc && (stride == 0u || (stride & (stride - 1u)) != 0u))) return bad_arg(__func__, __LINE__);
    c->clk = reinterpret_cast<unsigned long long*>(acc);
    c->clk_mask = acc ? stride - 1u : 0u;
    return BH_OK;
}

}  // extern "C"
