// bh_host.hpp -- what the host translation units of the library share (bh_host.cpp, bh_camera.cpp,
// bh_bloom_host.cpp, bh_tiles_host.cpp, bh_mirror.cpp): the objects behind the ABI's handles, the error
// helpers and the launchers the .hip units define.  Host only: no kernel unit includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bh_common.hpp"
#include "bh_srgb.hpp"

// not part of the library's surface (the handles' types are the ABI's own names, so they stay as they are)
#define BH_HIDDEN __attribute__((visibility("hidden")))
#define BH_INTERNAL extern "C" BH_HIDDEN  // defined in another unit of the library

struct bh_ctx {
    int device = 0;
    uint32_t* sky = nullptr;       // device RGBA8 texels
    float* lut = nullptr;          // device sRGB->linear table (256 floats)
    float* enc = nullptr;          // device linear->sRGB threshold table (257 floats)
    uint8_t* enc_b = nullptr;      // device base codes of the table-form encoder (SRGB_BUCKETS bytes)
    uint32_t* enc_e = nullptr;     // device code table of the code-table encoder (SRGB_CODES words)
    uint32_t* counters = nullptr;  // persistent-schedule work counters (1 KiB, zeroed per launch)
    uint32_t sky_w = 0, sky_h = 0;
    uint32_t grid_exact = 0, grid_fast = 0;  // resident blocks of the persistent kernels
    uint32_t cus = 0;                        // compute units of the device
    // temporal dispatch order (tile schedule): per-tile cost of the previous frame -> order, one state
    // per (frame geometry, shard, stream).  Never freed before bh_destroy except by LRU eviction beyond
    // BH_ORDER_STATES states, so a graph captured after the first call of a key keeps valid pointers,
    // and renders on different streams (frames in flight) never share costs or counters.
    struct OrderState {
        uint32_t width = 0, height = 0, shard_index = 0, shard_count = 0;
        uint64_t partition = 0;              // bh_partition::serial, 0 = none
        uint64_t n_tiles = 0;                // the buffers' size in tiles
        void* stream = nullptr;
        bool ray_map = false;                // a ray-map launch's state (bh_render_rays): its tile costs are its own
        uint64_t last_use = 0;
        bool valid = false;                  // costs and histogram agree (false: start afresh)
        bool captured = false;               // used by a launch captured into a graph: never evicted
        // Which frames the buffers describe (frame_cost_key): the costs in tile_cost (and the histogram the
        // counters hold of them, always pending) are those of a frame with key cost_key; the current order
        // was built from costs with key order_key.  A launch whose frame 0 has the key of both (a repeated
        // frame: a fixed camera) needs neither the order build nor new costs -- the march's step counts, and
        // so the costs, are a function of that key.
        uint64_t cost_key = 0, order_key = ~0ull;
        uint8_t* tile_cost = nullptr;
        uint32_t* order = nullptr;
        uint32_t* counters = nullptr;        // ORDER_WORDS words (bh_common.hpp)
        // the adaptive render's scratch for this geometry and stream (bh_render_adaptive; allocated by its
        // first call of the key, or of more frames than before): the work list, its two counters and the
        // mask of calls that pass no tile_mask, for refine_frames frames.  Same life as the buffers above.
        uint32_t* refine_list = nullptr;
        uint32_t* refine_ctr = nullptr;
        uint8_t* refine_mask = nullptr;
        uint32_t refine_frames = 0;
        // the state's key: the frame geometry and shard of `d`, a partition's serial (0: none), the tile count, the
        // stream, and whether the rays come from a map
        bool matches(const bh_render_desc* d, uint64_t partition_serial, uint64_t tiles, const void* on_stream,
                     bool from_map = false) const {
            return width == d->width && height == d->height && shard_index == d->shard_index &&
                   shard_count == d->shard_count && partition == partition_serial && n_tiles == tiles &&
                   stream == on_stream && ray_map == from_map;
        }
        void free_buffers() {
            (void)hipFree(tile_cost); (void)hipFree(order); (void)hipFree(counters);
            (void)hipFree(refine_list); (void)hipFree(refine_ctr); (void)hipFree(refine_mask);
        }
    };
    std::vector<OrderState> orders;
    uint64_t order_clock = 0;
    // per-frame arguments of bh_render_frames calls of more than BH_INLINE_FRAMES frames, one table per
    // stream: the kernels of one stream run in order, so one device table serves every call on it; the
    // host writes a pinned slot of a ring and copies it in on the stream (the slot is reused once its
    // copy has run: its event)
    static constexpr uint32_t FRAME_RING = 4;
    struct FrameTable {
        void* stream = nullptr;
        bh::FrameArgs* dev = nullptr;                 // BH_MAX_FRAMES entries, and room for as many FirstStep records
        bh::FrameArgs* host[FRAME_RING] = {};         // pinned, the same size each
        hipEvent_t done[FRAME_RING] = {};             // the slot's copy has executed
        uint32_t next = 0;
        std::vector<bh::FrameArgs> last;              // what the table holds once the stream's copies ran
        std::vector<bh::FirstStep> last_first;        // ... and the first-step records behind its frames
    };
    std::vector<FrameTable> frame_tables;
    // post-processing (bh_bloom) scratch: one set of textures per (width, height, levels), with the
    // separable plans of its up passes (sep_plan).  Graph contract as the order states: a set used under
    // stream capture is never evicted (bh_graph_release clears the mark); others are evicted least
    // recently used beyond BH_BLOOM_SETS.
    // ext: the largest block footprint side (up passes); nc, nr: the inexact columns / rows (same plan)
    // host: the plan's host copy in bh_bloom_check's dry mode (dev then points into it; never freed as device memory)
    struct SepPlan {
        std::array<uint32_t, 6> key{};  // ow, oh, tw, th, rx, ry
        uint32_t* dev = nullptr;
        int ext = 0;
        uint32_t nc = 0, nr = 0;
        size_t rec = 0;  // same-size plan: word offset of the list's fix-up records (8 words each)
        // the final epilogue's column strips (bh_bloom_strip_table): word offset of the table (0: none), its
        // strip columns and the strip storage (3 images x stw columns x oh rows; not allocated in dry mode)
        size_t stc = 0;
        uint32_t stw = 0;
        uint32_t* strips = nullptr;
        std::shared_ptr<std::vector<uint32_t>> host;
    };
    struct BloomScratch {
        uint64_t key = 0;
        std::vector<uint32_t*> tex;
        std::vector<SepPlan> sep_plans;
        uint32_t prepared = 0;   // bit s: schedule s ran once outside capture (every plan it uses exists)
        bool captured = false;
        uint64_t last_use = 0;
    };
    std::vector<BloomScratch> blooms;
    uint64_t bloom_clock = 0;
    // shader-clock probe of the march launches (bh_set_clock_probe): device accumulators or null
    unsigned long long* clk = nullptr;
    uint32_t clk_mask = 0;
    // the skies of bh_sky_create that are still alive (bh_destroy frees what is left)
    std::vector<bh_sky*> skies;
    // ... and the discs of bh_disc_create
    std::vector<bh_disc*> discs;
};

// A sky beside the context's own (include/bh_render.h, bh_sky_create): immutable device texels.
struct bh_sky {
    bh_ctx* ctx = nullptr;
    uint32_t* texels = nullptr;
    uint32_t w = 0, h = 0;
    // bh_sky_create_mips: the levels >= 1 (csrc/bh_lens.hpp, mip_offsets), n_levels != 0; both unset otherwise
    void* chain = nullptr;
    uint32_t n_levels = 0;
};

// A disc texture (include/bh_render.h, bh_disc_create): immutable device texels, n_phi around and n_r outwards.
struct bh_disc {
    bh_ctx* ctx = nullptr;
    uint32_t* texels = nullptr;
    uint32_t n_phi = 0, n_r = 0;
};

// A weighted tile partition (include/bh_render.h, bh_partition_create).
struct bh_partition {
    uint32_t width = 0, height = 0, shard_count = 0, tiles_x = 0, tiles_y = 0;
    int device = 0;
    std::vector<uint32_t> count, offset;  // per shard: tiles, first entry in tile_list
    uint32_t* tile_list = nullptr;        // device: every shard's tiles in packed order (tx | ty << 16)
    uint32_t* tile_loc = nullptr;         // device: per tile (ty * tiles_x + tx): packed index | shard << 24
    uint64_t serial = 0;                  // unique per created partition: the temporal-order key (an
                                          // address can be reused by a later partition)
};

// True when `s` is capturing -- or when the runtime cannot say (e.g. the legacy stream while another
// stream captures in global mode): the callers then refuse to allocate, which a capture would not survive.
BH_HIDDEN inline bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

// ---- errors: the thread's last message (bh_last_error) and the status that goes with it ----------------
// a validation failure without its own message: name the entry point and the check's file and line
BH_HIDDEN inline int bad_arg(const char* fn, int line, const char* file = __builtin_FILE()) {
    const char* base = std::strrchr(file, '/');
    bh_set_last_error(std::string(fn) + ": invalid argument (" + (base ? base + 1 : file) + ":" + std::to_string(line) + ")");
    return BH_ERR_INVALID_ARG;
}
BH_HIDDEN inline int hip_fail(hipError_t e, const char* what) {
    bh_set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    return BH_ERR_HIP;
}
// a failed allocation: out of memory has a status of its own (and no message)
BH_HIDDEN inline int alloc_fail(hipError_t e, const char* what) {
    return e == hipErrorOutOfMemory ? BH_ERR_OUT_OF_MEMORY : hip_fail(e, what);
}

// A frame of width x height pixels rendered at ss x ss rays per pixel (ss = 1: the frame itself): neither
// side 0, and the sides of the frame the kernels index, ss * width and ss * height, at most 65536.
BH_HIDDEN inline bool frame_shape_ok(uint32_t width, uint32_t height, uint32_t ss) {
    return width != 0 && height != 0 && (uint64_t)width * ss <= 65536u && (uint64_t)height * ss <= 65536u;
}

// Makes `device` current for one ABI call and restores the caller's device on every return path.
struct BH_HIDDEN DeviceScope {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) err = hipSetDevice(device);
    }
    ~DeviceScope() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// ---- shared between the host units --------------------------------------------------------------------
BH_HIDDEN void srgb_lut(float lut[256]);        // bh_host.cpp: sRGB byte -> linear
BH_HIDDEN uint8_t srgb_encode_ref(float x);     // bh_host.cpp: the normative linear -> sRGB byte
BH_HIDDEN void free_bloom_scratch(bh_ctx::BloomScratch& b);  // bh_bloom_host.cpp

// ---- launchers and host-side planners, defined in the .hip translation units ----------------------------
// The march units' launchers (bh_march.hpp, BH_MARCH_UNIT and BH_REFINE_UNIT), one per unit and named after its
// namespace: bh_launch_unit_<ns> of every tile-march unit, all of the one type MarchUnitFn, and
// bh_launch_refine_unit_<ns> of the three units that hold the adaptive render's work-list march (a.ss_log2 in 1..3,
// `waves` pulling waves).  bh_host.cpp's tables say which unit serves which family and build.
#define BH_MARCH_UNIT_NAMESPACES(X)                                                                  \
    X(exact) X(exact_lat) X(fast) X(exact_rays) X(exact_rays_lat) X(exact_rays_pose) X(exact_rays_pose_lat) \
    X(exact_rays_org) X(exact_rays_org_lat) X(exact_hits) X(exact_hits_lat) X(exact_arr) X(exact_arr_lat)
#define BH_REFINE_UNIT_NAMESPACES(X) X(exact) X(exact_lat_refine) X(fast)
using MarchUnitFn = int(const bh::MarchArgs& a, const bh::MarchLaunch& m, hipStream_t s);
using RefineUnitFn = int(const bh::MarchArgs& a, const bh::RefineArgs& r, uint32_t waves, hipStream_t s);
#define BH_DECLARE_MARCH_UNIT(ns) BH_INTERNAL MarchUnitFn bh_launch_unit_##ns;
#define BH_DECLARE_REFINE_UNIT(ns) BH_INTERNAL RefineUnitFn bh_launch_refine_unit_##ns;
BH_MARCH_UNIT_NAMESPACES(BH_DECLARE_MARCH_UNIT)
BH_REFINE_UNIT_NAMESPACES(BH_DECLARE_REFINE_UNIT)
#undef BH_DECLARE_MARCH_UNIT
#undef BH_DECLARE_REFINE_UNIT
// the adaptive render's detect kernel (bh_tiles.hip)
BH_INTERNAL int bh_launch_refine_detect(const bh::MarchArgs& a, const bh::RefineArgs& r, hipStream_t s);
// the lens shade (bh_lens.hip): ss in {1, 2, 4, 8}, format a bh_out_format
BH_INTERNAL int bh_launch_lens_shade(const bh::LensShadeArgs& a, uint32_t ss, uint32_t format, hipStream_t s);
// the filtered lens shade and the chain it reads (bh_lens.hip): ss in {1, 2, 4}; the chain's kernels on `s`
BH_INTERNAL int bh_launch_lens_shade_mip(const bh::LensMipArgs& a, uint32_t ss, uint32_t format, hipStream_t s);
// the disc shade (bh_disc.hip): ss in {1, 2, 4, 8}
BH_INTERNAL int bh_launch_lens_shade_disc(const bh::LensDiscArgs& a, uint32_t ss, uint32_t format, hipStream_t s);
// the beamed disc shade (bh_disc.hip): ss in {1, 2, 4, 8}
BH_INTERNAL int bh_launch_lens_shade_disc_beamed(const bh::LensBeamArgs& a, uint32_t ss, uint32_t format, hipStream_t s);
BH_INTERNAL int bh_launch_sky_mips(const uint32_t* sky, uint32_t w0, uint32_t h0, const float* srgb_lut, void* chain,
                hipStream_t s);
BH_INTERNAL int bh_march_blocks_per_cu_exact(void);
BH_INTERNAL int bh_march_blocks_per_cu_fast(void);
BH_INTERNAL int bh_launch_build_order(const uint8_t* cost, uint32_t n_tiles, uint32_t block, uint32_t centre,
                uint32_t* counters, uint32_t* order, hipStream_t s);
BH_INTERNAL int bh_launch_tiles_unpack_rgbm(const void* packed, void* out, void* out_bo, uint32_t width,
                uint32_t height, uint32_t shard_count, uint64_t stride_tiles, const uint32_t* tile_loc, uint32_t format,
                uint32_t rows_in_flight, hipStream_t s);
BH_INTERNAL int bh_launch_tiles_unpack_rgb(const void* packed, void* out, uint32_t width, uint32_t height,
                uint32_t shard_count, uint64_t stride_tiles, uint32_t format, uint32_t rows_in_flight, hipStream_t s);
// an up pass from its separable plan with an epilogue (bh_bloom.hip SepEpi: 0 plain, 1 Y, 2 final)
BH_INTERNAL int bh_launch_bloom_sep(const float* lut, const float* enc, const uint8_t* buckets, const uint32_t* codes,
                const uint32_t* a, uint32_t aw, uint32_t ah, uint32_t rx, uint32_t ry, const uint32_t* sep, int ext,
                uint32_t epi, const uint32_t* own0, const uint32_t* own1, const uint32_t* same, uint32_t* out,
                uint32_t* aux, uint32_t ow, uint32_t oh, const uint32_t* stc, uint32_t* strips, uint32_t strip_w,
                bool* strips_written, hipStream_t s);
// the fix-up pass of a fused epilogue over the same-size plan's list and its records; stc / strips: the final epilogue's column strips (the up pass wrote them)
BH_INTERNAL int bh_launch_bloom_fixup(const float* lut, const float* enc, const uint8_t* buckets, const uint32_t* codes,
                uint32_t epi, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* same,
                const uint32_t* list, uint32_t n_cols, uint32_t n_rows, uint32_t* out, uint32_t w, uint32_t h,
                const uint32_t* recs, const uint32_t* stc, const uint32_t* strips, uint32_t strip_w, hipStream_t s);
// two downsamples a -> mw x mh -> out in one pass (the intermediate level not stored)
BH_INTERNAL int bh_launch_bloom_down2(const float* lut, const float* enc, const uint8_t* buckets, const uint32_t* codes,
                const uint32_t* a, uint32_t aw, uint32_t ah, uint32_t mw, uint32_t mh, uint32_t* out, uint32_t ow,
                uint32_t oh, hipStream_t s);
// the remixes and the same-size copy through the same-size plan (bh_bloom_same_plan)
BH_INTERNAL int bh_launch_bloom_remix_plan(const float* lut, const float* enc, const uint8_t* buckets,
                const uint32_t* codes, const uint32_t* a, const uint32_t* b, const uint32_t* plan, uint32_t* out,
                uint32_t w, uint32_t h, hipStream_t s);
BH_INTERNAL int bh_launch_bloom_same_copy(const float* lut, const float* enc, const uint8_t* buckets,
                const uint32_t* codes, const uint32_t* src, const uint32_t* plan, uint32_t* out, uint32_t w, uint32_t h,
                hipStream_t s);
BH_INTERNAL int bh_launch_bloom_remix2_plan(const float* lut, const float* enc, const uint8_t* buckets,
                const uint32_t* codes, const uint32_t* col, const uint32_t* Y, const uint32_t* Bt, const uint32_t* plan,
                uint32_t* out, uint32_t w, uint32_t h, hipStream_t s);
BH_INTERNAL int bh_launch_bloom_pass(uint32_t shader, const float* lut, const float* enc, const uint8_t* buckets,
                const uint32_t* codes, const uint32_t* a, uint32_t aw, uint32_t ah, const uint32_t* b, uint32_t rx,
                uint32_t ry, uint32_t* out, uint32_t ow, uint32_t oh, const uint32_t* sep, int sep_ext, hipStream_t s);
BH_INTERNAL int bh_launch_bloom_y(const float* lut, const float* enc, const uint8_t* buckets, const uint32_t* codes,
                const uint32_t* X, uint32_t* Y, uint32_t w, uint32_t h, uint32_t* d2out, bool* d2_done, hipStream_t s);
BH_INTERNAL int bh_launch_bloom_final(const float* lut, const float* enc, const uint8_t* buckets, const uint32_t* codes,
                const uint32_t* col, const uint32_t* Y, const uint32_t* U0, uint32_t rx, uint32_t ry, uint32_t* out,
                uint32_t w, uint32_t h, hipStream_t s);
BH_INTERNAL int bh_launch_tiles_unpack(const void* packed, void* out, uint32_t width, uint32_t height,
                uint32_t shard_count, uint64_t shard_stride_tiles, uint32_t bytes_per_pixel, hipStream_t s);
