/*
 * bh_render.h — C ABI of the MI355X-native geodesic ray-marcher.
 *
 * This is the drop-in boundary for ONE hot path of jonathandw743/black_hole_ray_marching:
 * the per-pixel Schwarzschild photon integrator `fs_main -> get_col`
 * (src/black_hole_maybe.wgsl:259-370), which the reference drives through
 * `Scene::render(encoder, output_view, blackout_output_view)` (src/scene.rs:470-522).
 *
 * Mapping of reference interfaces onto entry points (all paths relative to the reference repo):
 *
 *   bh_camera_uniform          == WGSL `Camera` (src/black_hole_maybe.wgsl:9-17), packed by
 *                                 `CameraUniform` (src/uniforms.rs:98-106) with encase: 112 B.
 *   bh_uniforms                == WGSL `Uniforms` (src/black_hole_maybe.wgsl:58-69), packed by
 *                                 `OtherUniforms::uniform_buffer_content` (src/otheruniforms.rs:105-118): 32 B.
 *   bh_camera                  == `Camera` (src/camera.rs:11-20).
 *   bh_uniforms_default        == the six `OtherUniform` defaults of `Scene::new` (src/scene.rs:89-137),
 *                                 including the inverted PodBool (src/podbool.rs:21-26) => blackout_eh = 1.
 *   bh_camera_default          == the camera literal of `Scene::new` (src/scene.rs:68-76).
 *   bh_camera_uniform_update   == `CameraUniform::update` (src/uniforms.rs:123-133) ->
 *                                 `Camera::pos_to_world_space_screen_triangle` (src/camera.rs:89-112).
 *   bh_create                  == the sky-texture half of `Scene::new`: `Texture::from_bytes` /
 *                                 `from_image` (src/texture.rs:11-77, Rgba8UnormSrgb, clamp, mag Linear)
 *                                 as bound at src/scene.rs:186-232.
 *   bh_render                  == `Scene::render` (src/scene.rs:470-522): one full-screen pass writing
 *                                 `col` (target 0) and optionally `blackout_col` (target 1; NULL == None).
 *   bh_destroy                 == dropping the `Scene`'s GPU resources.
 *
 * Conventions: every function returns BH_OK (0) or a negative bh_status; nothing aborts or throws
 * across the ABI.  Output pointers are caller-owned DEVICE pointers (the reference's consumer, Bloom,
 * owns its textures and lends views: src/bloom.rs:31-37).  bh_render is asynchronous on the given
 * HIP stream (NULL = the legacy default stream).  It never synchronises the host, with one exception:
 * a bh_render_frames call of more than 32 frames may wait for the copy of the call four before it on
 * the same stream (its pinned staging ring, see bh_render_frames).  The tile schedule's temporal
 * dispatch order keeps small per-(frame geometry, shard, stream) device buffers in the ctx: the FIRST
 * bh_render of such a key allocates them (hipMalloc) and must not be captured -- on a capturing stream
 * it returns BH_ERR_UNSUPPORTED and launches nothing; every later call with that key allocates nothing
 * and may be captured into a hipGraph.  Those buffers are never freed or moved before bh_destroy
 * while a graph may use them: a key rendered under stream capture is never evicted.  Other keys are
 * evicted least-recently-used beyond BH_ORDER_STATES (when every key has been captured the ctx keeps
 * more instead).  bh_bloom keeps one scratch set per (size, levels) under the same contract: the first
 * call of a (size, levels, schedule) allocates and must not be captured (BH_ERR_UNSUPPORTED on a
 * capturing stream), a set used under capture is never freed, others are evicted least-recently-used
 * beyond BH_BLOOM_SETS.  A stream whose capture status the runtime cannot report (e.g. the legacy
 * stream while another stream captures globally) counts as capturing.  Captured states stay pinned
 * until bh_destroy, or until bh_graph_release (call it once the graphs that used them are destroyed).
 * Renders of one ctx on different streams with the TILE or PAIR schedule use
 * different order state and no other shared scratch, so they may run concurrently (frames in flight);
 * the PERSISTENT schedule (shared work counters) and bh_bloom (shared scratch textures) must not run
 * concurrently with themselves on one ctx.  One bh_ctx per device; a ctx is not thread-safe, distinct
 * ctx objects may be used from distinct threads (one per rank).
 */
#ifndef BH_RENDER_H
#define BH_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BH_ABI_VERSION 8

/* Temporal-order states (frame geometry x shard x stream) one ctx keeps (see above). */
#define BH_ORDER_STATES 32
/* bh_bloom scratch sets (size x levels) one ctx keeps (see above). */
#define BH_BLOOM_SETS 4

typedef enum {
    BH_OK = 0,
    BH_ERR_INVALID_ARG = -1,   /* NULL/zero/out-of-range argument */
    BH_ERR_UNSUPPORTED = -2,   /* valid for the reference but not implemented (e.g. non-default screen triangle: another projection is a ray map, bh_render_rays) */
    BH_ERR_HIP = -3,           /* a HIP runtime call failed; see bh_last_error() */
    BH_ERR_NO_DEVICE = -4,     /* no HIP device / device index out of range */
    BH_ERR_OUT_OF_MEMORY = -5,
    BH_ERR_INTERNAL = -6       /* a host-side consistency check failed (bh_bloom_check); see bh_last_error() */
} bh_status;

/* WGSL `Camera` (src/black_hole_maybe.wgsl:9-17), std140/encase layout, 112 bytes:
 *   pos @0 (vec3, padded to 16), screen_space_screen_triangle @16 (3 x vec4),
 *   pos_to_world_space_screen_triangle @64 (3 x vec4). */
typedef struct {
    float pos[3];
    float _pad0;
    float screen_tri[3][4];
    float world_tri[3][4];
} bh_camera_uniform;

/* WGSL `Uniforms` (src/black_hole_maybe.wgsl:58-69), 32 bytes.
 * bg_brightness is carried for layout fidelity but unused by the shader (as in the reference). */
typedef struct {
    float rs;               /* RS: Schwarzschild radius (default 1.0) */
    float delta_time_mult;  /* DELTA_TIME_MULT (default 0.5) */
    float bg_brightness;    /* BG_BRIGHTNESS (default 0.5, unused) */
    uint32_t blackout_eh;   /* BLACKOUT_EH: != 0 enables event-horizon blackout (default 1) */
    float max_dist;         /* MAX_DIST (default 250.0) */
    float distortion_power; /* DISTORTION_POWER (default 1.0) */
    uint32_t _pad[2];
} bh_uniforms;

/* `Camera` (src/camera.rs:11-20). */
typedef struct {
    float pos[3];
    float dir[3];
    float up[3];
    float aspect;
    float fovy;
    float znear;
    float zfar;
} bh_camera;

/* Output texel formats.  The reference stores into Bgra8UnormSrgb surfaces (src/copy.rs:132,
 * src/remix.rs:160); RGBA32F is the parity format, RGBA16F the production format. */
typedef enum {
    BH_OUT_RGBA32F = 0,     /* 16 B / pixel, linear */
    BH_OUT_RGBA16F = 1,     /*  8 B / pixel, linear, round-to-nearest-even from the fp32 result */
    BH_OUT_BGRA8_SRGB = 2   /*  4 B / pixel, sRGB-encoded (round(255 * OETF(clamp(x, 0, 1))), NaN -> 0),
                               byte order B,G,R,A: the Bgra8UnormSrgb store of the reference */
} bh_out_format;

/* Arithmetic mode of the integrator (see DESIGN.md "Math modes"). */
typedef enum {
    BH_MATH_EXACT = 0,      /* IEEE div/sqrt, no contraction, same op order as the oracle: bit-exact parity */
    BH_MATH_FAST = 1        /* rsq/rcp/FMA reformulation: production speed, tolerance parity */
} bh_math_mode;

/* Scene contents (bit mask).  The reference always has both (src/black_hole_maybe.wgsl:119-123);
 * 0 removes every surface (sdf == +inf), BASELINE config 1. */
#define BH_SCENE_DISC    1u
#define BH_SCENE_MARKERS 2u
#define BH_SCENE_DEFAULT (BH_SCENE_DISC | BH_SCENE_MARKERS)

/* Output layout. */
typedef enum {
    BH_LAYOUT_ROWMAJOR = 0, /* out[y * width + x]; requires shard_count == 1 */
    BH_LAYOUT_TILES = 1,    /* the shard's 8x8 tiles packed in shard order, 64 pixels per tile,
                               pixel (x & 7) + 8 * (y & 7) inside a tile; pixels outside the frame
                               are left untouched */
    BH_LAYOUT_TILES_RGB = 2, /* BH_LAYOUT_TILES without alpha (both targets' alpha is always 1,
                               src/black_hole_maybe.wgsl:369): each tile is three planes of 64
                               channel values in the format's memory order less alpha (R, G, B for
                               RGBA16F/RGBA32F; B, G, R for BGRA8), 3/4 of the bytes to gather */
    BH_LAYOUT_TILES_RGBM = 3, /* BH_LAYOUT_TILES_RGB plus, after each tile's three planes, one 64-bit
                               little-endian word whose bit i is set when pixel i of the tile has
                               blackout_col == 0, i.e. dot(col, col) < 1 in fp32 (src/black_hole_maybe.wgsl:365-368):
                               the multi-GPU transport.  blackout_col is a per-pixel function of the
                               fp32 col, but not of its quantised RGBA16F / BGRA8 bytes, so the decision
                               travels with them (0.125 B/pixel) and the gathered col alone restores both
                               targets bit for bit (bh_tiles_unpack_rgbm).  Tile bytes: 776 (RGBA32F),
                               392 (RGBA16F), 200 (BGRA8).  Schedules TILE and PAIR only. */
    BH_LAYOUT_TILES_RGBM14 = 4 /* BH_LAYOUT_TILES_RGBM for RGBA16F in 344 B per tile (5.375 B/pixel instead
                               of 6.125): every colour channel is an fp16 in [0, 1] -- sky samples are
                               bilinear mixes of decoded texels in [0, 1] (and g, b their c * sqrt(c)),
                               surfaces 1, blackout 0 -- so its top two bits are 0 and 14 bits carry it.
                               Per tile: 64 words r | g << 14 | (b & 0xF) << 28, 64 bytes (b >> 4) & 0xFF,
                               two 64-bit words holding bit 12 / bit 13 of b for pixel i at bit i, then the
                               blackout mask word.  RGBA16F, schedules TILE and PAIR only; unpack with
                               bh_tiles_unpack_rgbm(_partition) and format BH_OUT_RGBA16F | BH_UNPACK_RGBM14. */
} bh_layout;
/* format flag of bh_tiles_unpack_rgbm / bh_tiles_unpack_rgbm_partition: the shards are
 * BH_LAYOUT_TILES_RGBM14 (with BH_OUT_RGBA16F) */
#define BH_UNPACK_RGBM14 0x100u

/* Work schedule of the march kernel (same results, different speed). */
typedef enum {
    BH_SCHED_TILE = 0,       /* one wave64 per 8x8 tile (default); dispatch order: the previous frame's
                                per-tile cost, most expensive first (ties / first frame: centre-out
                                around the black hole's screen row) */
    BH_SCHED_PAIR = 1,       /* one wave64 per two 8x8 tiles, two interleaved rays per lane */
    BH_SCHED_PERSISTENT = 2  /* resident waves, per-lane refill from an LDS ray queue */
} bh_schedule;
/* OR into `schedule` to use the static centre-out order only (no per-tile cost feedback). */
#define BH_SCHED_FLAG_STATIC_ORDER 0x100u
/* Exact math: which build of the march kernels runs (same bits either way).  By default bh_render
 * picks per launch: the source-order build when it is throughput-bound (its tiles in flight, over
 * all frames of a bh_render_frames launch, >= 384 per CU x max_iters / 512), else the
 * machine-scheduled build, whose lone tail waves step faster (packed-FP32 tail step).
 * These flags force one (BH_SCHED_FLAG_ISSUE_ORDER wins if both are set). */
#define BH_SCHED_FLAG_ISSUE_ORDER 0x200u
#define BH_SCHED_FLAG_LATENCY 0x400u

/* Per-pixel fate codes written to dbg_fate. */
#define BH_FATE_CAP      0u  /* loop ran out (max_iters); still shades sky with its current rd */
#define BH_FATE_ESCAPE   1u  /* distance_travelled > MAX_DIST (src/black_hole_maybe.wgsl:325-327) */
#define BH_FATE_SURFACE  2u  /* sdf < MIN_DIST (:286-288) -> colour 1 */
#define BH_FATE_BLACKOUT 3u  /* event-horizon blackout (:272-283) -> colour 0 */

#define BH_TILE 8u           /* tile edge in pixels (multi-GPU sharding and BH_LAYOUT_TILES) */

typedef struct bh_partition bh_partition;

typedef struct {
    uint32_t width, height;   /* frame size in pixels */
    uint32_t max_iters;       /* MAX_ITERATIONS (WGSL const 1000, src/black_hole_maybe.wgsl:85), 1..65535 */
    uint32_t scene_flags;     /* BH_SCENE_* */
    uint32_t format;          /* bh_out_format */
    uint32_t math;            /* bh_math_mode */
    uint32_t layout;          /* bh_layout */
    uint32_t shard_index;     /* this rank's tile share: tile (tx,ty) belongs to shard (tx + 3*ty) % shard_count */
    uint32_t shard_count;     /* 1 = whole frame */
    uint32_t schedule;        /* bh_schedule | BH_SCHED_FLAG_* (results never depend on it) */
    void* out_col;            /* target 0 (`col`), device pointer, never NULL */
    void* out_blackout;       /* target 1 (`blackout_col`), device pointer or NULL (== Option::None) */
    uint16_t* dbg_n_rk;       /* optional: completed RK4 steps per pixel (same layout as outputs, 1 elem/px) */
    uint8_t* dbg_fate;        /* optional: BH_FATE_* per pixel */
    uint16_t* dbg_steps;      /* optional: RK4 iterations actually executed per pixel; below dbg_n_rk
                                 only where a ray that had entered an exact cycle (see DESIGN.md
                                 "Cycle fast-forward") was advanced to the cap without iterating */
    const bh_partition* partition; /* optional, BH_LAYOUT_TILES* only: a weighted tile partition
                                 (bh_partition_create) with this frame size and shard_count, used
                                 instead of the default (tx + 3*ty) % shard_count interleave */
} bh_render_desc;

typedef struct bh_ctx bh_ctx;

int bh_abi_version(void);
const char* bh_status_string(int status);
/* Thread-local text of the last HIP error seen by this library ("" if none). */
const char* bh_last_error(void);

/* Defaults of Scene::new (src/scene.rs:68-137). */
int bh_uniforms_default(bh_uniforms* out);
int bh_camera_default(uint32_t width, uint32_t height, bh_camera* out);
/* CameraController (src/camera.rs:115-366), the host camera layer of an animated / offline camera
 * path: the controller's key state (process_event, :186-261, as booleans), its two speeds
 * (CameraController::new(5.0, 0.5) at src/scene.rs:78; Q / E scale `speed` by 1/1.5 and 1.5) and
 * the last two cursor positions (as f32, the conversion of :270-276). */
typedef struct {
    uint8_t forward, backward, left, right, up, down;  /* W, S, A, D, Space, F */
    uint8_t pan_up, pan_down, pan_left, pan_right;     /* arrow keys */
    uint8_t exp_towards_origin, exp_away_origin;       /* P, O */
    uint8_t mouse_pressed;                             /* left button */
    uint8_t has_prev_cursor, has_curr_cursor;          /* Option::Some */
    uint8_t _pad;
    float prev_cursor[2], curr_cursor[2];
    float speed, pan_speed;
} bh_controller;

/* CameraController::update_camera(camera, delta_time, do_pan) (src/camera.rs:280-366): moves and
 * rotates *camera by dt seconds of the controller's state, glam f32 arithmetic (Quat::from_axis_angle,
 * Quat::mul_vec3).  *moved (optional) = the function's return value. */
int bh_controller_update(const bh_controller* ctrl, bh_camera* camera, float dt, int do_pan, int* moved);

/* CameraUniform::new (src/uniforms.rs:108-122) + ::update (:123-133). */
int bh_camera_uniform_update(const bh_camera* camera, bh_camera_uniform* out);
/* Camera aimed at `target` from `pos` (up +Y, fovy pi/2): SURVEY §8d cameras B and C. */
int bh_camera_look_at(const float pos[3], const float target[3], uint32_t width, uint32_t height,
                      bh_camera* out);

/* Deterministic synthetic equirectangular sky (RGBA8, sRGB-encoded, alpha 255):
 * splitmix64-seeded value-noise nebula + sparse stars.  Stand-in for src/space_4096x2048.jpg. */
int bh_synthetic_sky(uint8_t* out_rgba8, uint32_t width, uint32_t height, uint64_t seed);

/* Upload the sky (width*height*4 bytes, Rgba8UnormSrgb semantics) to `device` and build the
 * sRGB->linear table.  The context owns the device copy. */
int bh_create(const uint8_t* sky_rgba8_srgb, uint32_t sky_width, uint32_t sky_height, int device,
              bh_ctx** out);
int bh_destroy(bh_ctx* ctx);

/* Scene::render.  Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream). */
int bh_render(bh_ctx* ctx, const bh_camera_uniform* camera, const bh_uniforms* uniforms,
              const bh_render_desc* desc, void* hip_stream);

/* Several frames in ONE launch: n_frames (1..BH_MAX_FRAMES) calls of Scene::render -- e.g. consecutive
 * frames of an offline camera path, cameras[i] for frame i -- with one `uniforms` and descs that agree in
 * everything but their output and debug pointers (frame size, cap, scene, format, math, layout, shard,
 * schedule; else BH_ERR_INVALID_ARG).  Each frame's results are exactly bh_render's.  With the tile
 * schedule the frames' tiles are interleaved in one grid (slot s = tile s / n of frame s % n, most
 * expensive tiles first), so the frames' serial tails -- the few rays that march to the cap -- overlap
 * each other's bulk instead of each ending a launch alone; other schedules run n launches.  The
 * temporal order of (geometry, shard, stream) learns from frame 0 of each call.  Up to 32 frames travel
 * in the kernel argument; a call of more stages the frames' arguments through a pinned host ring into a
 * device table of the stream (allocated at the first such call, never captured into a HIP graph: a
 * capturing stream gets BH_ERR_UNSUPPORTED for n_frames > 32).  The ring has 4 slots: such a call
 * blocks the host until the copy of the 4th such call before it on the stream has executed. */
#define BH_MAX_FRAMES 256
int bh_render_frames(bh_ctx* ctx, uint32_t n_frames, const bh_camera_uniform* cameras, const bh_uniforms* uniforms,
                     const bh_render_desc* descs, void* hip_stream);

/* Supersampled render: ss x ss rays per output pixel, ss = k in {1, 2, 4, 8}, resolved inside the march
 * kernel (not in the reference: it shoots one ray through each pixel centre).  desc->width x desc->height is
 * the OUTPUT size.  The samples are the pixels of the VIRTUAL frame k*width x k*height -- exactly what
 * bh_render produces for that size with the same camera uniform, uniforms, cap, scene flags and math mode,
 * as linear fp32 values before any output encode -- so output pixel (x, y) averages virtual pixels
 * (kx+i, ky+j), 0 <= i, j < k: the regular k x k grid inside the pixel.
 *   Per sample: col_s and bo_s = dot(col_s, col_s) < 1 ? 0 : col_s (the blackout test runs per sample, as
 *     fs_main runs it per fragment; never on the average).
 *   Resolve, per channel r, g, b, in fp32, no FMA, in this order: a pairwise tree along x (level 1 adds
 *     neighbours i and i^1, level 2 the pair sums i and i^2, level 3 -- k = 8 -- i and i^4), the same tree
 *     along y over the row results, then one multiply by 1 / k^2 (exact).
 *   Alpha is 1 (255).  Encode: the output format's existing one, applied to the resolved fp32 value (bit
 *     copy for RGBA32F, round-to-nearest-even for RGBA16F, the sRGB encode in B, G, R, A order for BGRA8).
 *   out_blackout == NULL: that target is neither resolved nor written.
 * ss = 1 is bh_render / bh_render_frames exactly (the call is passed on).  ss outside {1, 2, 4, 8}, or
 * ss * width or ss * height above 65536: BH_ERR_INVALID_ARG.  With ss > 1 the tile schedule's waves resolve
 * their own 8x8 block of samples (k divides 8: a block holds whole pixels), so BH_ERR_UNSUPPORTED, with a
 * sentence in bh_last_error(), for: a layout other than BH_LAYOUT_ROWMAJOR, shard_count != 1, a partition,
 * a base schedule other than BH_SCHED_TILE, any dbg_* pointer.  The BH_SCHED_FLAG_* flags are allowed.
 * bh_render_frames_ss: up to BH_MAX_FRAMES frames in one launch, as bh_render_frames.
 * Order state and graph contract: the launch is the virtual frame's.  Its temporal-order state and its
 * repeated-frame key are those of geometry (k*width, k*height) on the stream -- SHARED with a plain
 * bh_render of k*width x k*height on the same stream, which marches the same tiles and rays at the same
 * costs.  The graph contract is unchanged: the first render of that key allocates and is refused under
 * capture. */
int bh_render_ss(bh_ctx* ctx, const bh_camera_uniform* camera, const bh_uniforms* uniforms,
                 const bh_render_desc* desc, uint32_t ss, void* hip_stream);
int bh_render_frames_ss(bh_ctx* ctx, uint32_t n_frames, const bh_camera_uniform* cameras, const bh_uniforms* uniforms,
                        const bh_render_desc* descs, uint32_t ss, void* hip_stream);
/* Host only (no device needed): the supersampled kernel's own lane code (csrc/bh_ss.hpp: butterfly levels,
 * writer lanes, output index) run wave by wave over an fp32 RGBA virtual frame (ss*height rows of ss*width
 * pixels) -> the fp32 RGBA resolve, width x height, alpha 1.  BH_ERR_INVALID_ARG as above. */
int bh_ss_resolve_host(const float* samples_rgba, uint32_t width, uint32_t height, uint32_t ss, float* out_rgba);

/* Shutter render: every output frame integrates over a shutter interval -- it takes n_sub in {1, 2, 4, 8, 16}
 * camera uniforms (the sub-frame cameras of its exposure) and is the average of the n_sub frames bh_render would
 * produce for them, resolved inside the march kernel in linear fp32 before the one output encode (not in the
 * reference, which renders one instantaneous camera per frame).  Composes with ss.
 *   bh_render_shutter: cameras[n_sub], one desc.  bh_render_frames_shutter: n_frames output frames in one
 *     launch, frame f uses cameras[f * n_sub + t], t = 0 .. n_sub - 1, and descs[f].
 *   Samples: for time sample t, col_t and bo_t are the linear fp32 values before any encode -- with ss = 1 the
 *     values bh_render computes for that camera, with ss = k in {2, 4, 8} the values bh_render_ss computes
 *     (the k x k tree and the multiply by 1 / k^2 included).  The blackout test runs per ray sample, as it does
 *     there, never on an average.
 *   Resolve, per channel r, g, b and per target, in fp32, no FMA: a pairwise tree over t (level 1 adds t and
 *     t^1, level 2 the pair sums t and t^2, and so on), then one multiply by 1 / n_sub (exact).  Alpha is 1.
 *   Encode: the output format's existing one, applied to the resolved value.  out_blackout == NULL: that
 *     target is neither resolved nor written.
 * n_sub = 1 is bh_render_frames / bh_render_frames_ss exactly (the call is passed on).  BH_ERR_INVALID_ARG:
 * n_sub outside {1, 2, 4, 8, 16}; n_frames * n_sub above BH_MAX_FRAMES; the ss and size limits of bh_render_ss.
 * With n_sub > 1 one workgroup of n_sub waves marches a tile once per camera and resolves it, so
 * BH_ERR_UNSUPPORTED, with a sentence in bh_last_error() that starts with "bh_render_shutter", for everything
 * bh_render_ss refuses: a layout other than BH_LAYOUT_ROWMAJOR, shard_count != 1, a partition, a base schedule
 * other than BH_SCHED_TILE, any dbg_* pointer.  The BH_SCHED_FLAG_* flags are allowed.  A refused call leaves
 * the outputs untouched.
 * Order state, repeated-frame skip and graph contract are those of bh_render_frames(_ss) of the same
 * n_frames * n_sub cameras: the key is the (virtual) geometry on the stream, shared with plain renders of it --
 * the dispatch order it holds is the same order of the same tiles whichever kernel walks it, learned from
 * camera 0 of frame 0 only (each tile counted once), and a call whose camera 0 repeats the last launch's skips
 * the order build as a plain render does.  More than 32 cameras in a call go through the pinned ring and device
 * table of bh_render_frames and are refused on a capturing stream.  The first call of a key allocates and is
 * refused under capture; later calls allocate nothing. */
int bh_render_shutter(bh_ctx* ctx, uint32_t n_sub, const bh_camera_uniform* cameras, const bh_uniforms* uniforms,
                      const bh_render_desc* desc, uint32_t ss, void* hip_stream);
int bh_render_frames_shutter(bh_ctx* ctx, uint32_t n_frames, uint32_t n_sub, const bh_camera_uniform* cameras,
                             const bh_uniforms* uniforms, const bh_render_desc* descs, uint32_t ss, void* hip_stream);
/* Host only (no device needed): the shutter kernel's own mapping and tree (csrc/bh_shutter.hpp: workgroup ->
 * frame and tile, wave -> camera, the time tree) with bh_ss_resolve_host's lane code for ss > 1, run workgroup
 * by workgroup over n_frames * n_sub fp32 RGBA sample frames (camera after camera, each ss*height rows of
 * ss*width pixels) -> n_frames fp32 RGBA frames, width x height, alpha 1.  BH_ERR_INVALID_ARG as above;
 * BH_ERR_INTERNAL if any (frame, tile, camera) is visited other than exactly once or a store index falls
 * outside the frame. */
int bh_shutter_resolve_host(const float* samples_rgba, uint32_t n_frames, uint32_t n_sub, uint32_t width,
                            uint32_t height, uint32_t ss, float* out_rgba);

/* Adaptive supersampling: every pixel gets the plain one-ray value, and every 8x8 output tile that shows an
 * edge is marched again with ss x ss rays per pixel and overwritten with the supersampled value.
 * Normative definition.  For one frame of size W x H, format F, ss = k in {2, 4, 8} and threshold T, let
 *   P = the bytes bh_render writes for that frame (both targets),
 *   S = the bytes bh_render_ss with ss = k writes.
 * Texel values: the stored colour channels of P, without alpha -- RGBA32F: the fp32 values as stored;
 *   RGBA16F: each channel converted to fp32 (exact); BGRA8: the three colour bytes as integers.
 * Neighbour distance of two 4-neighbours a and b (x +- 1 or y +- 1, both inside the frame, no wrap across
 *   row ends): float formats, d = max over the 3 channels of |a_c - b_c|, one fp32 subtract each, then abs;
 *   BGRA8, d = (float) max |a_c - b_c| over the integer bytes.  They DIFFER when d > T in the float formats,
 *   when d > T * 255.0f (one fp32 multiply) in BGRA8; the comparison is strict.
 * Edge pixels: a pixel that differs from any 4-neighbour in `col`; when out_blackout is non-NULL, also one
 *   that differs from any 4-neighbour in `blackout_col`.  With out_blackout == NULL only `col` counts.
 * Refined tiles: an 8x8 output tile (tx, ty) that holds at least one edge pixel (a differing pair that
 *   straddles a tile boundary refines both tiles).
 * Output: pixels of refined tiles hold S's bytes, all other pixels P's; both targets, alpha unchanged.
 * Arguments: T must be finite and >= 0 and ss one of 2, 4, 8, else BH_ERR_INVALID_ARG; the size limits are
 * bh_render_ss's; everything bh_render_ss refuses with BH_ERR_UNSUPPORTED is refused here the same way
 * (layout, shards, partition, base schedule, dbg_* pointers), the sentence in bh_last_error() starting
 * "bh_render_adaptive".
 * tile_mask (optional, device): n_frames * tiles_x * tiles_y bytes, frame-major, row-major tiles of
 * ceil(W / 8) x ceil(H / 8), 1 = refined.  refined_tiles (optional, device): n_frames counts.  Both are
 * written on the stream; every byte of outputs, mask and counts is the same from run to run.
 * How it runs: bh_render_frames on the stream (pass 1, with the W x H geometry's order state as ever), a
 * detect kernel over the plain frame that leaves a work list on the device, and the supersampled march
 * over that list (pass 2), which reads and writes no order state -- the virtual geometry's state, which
 * bh_render_ss uses, is not touched.  The host never reads the list's length.
 * Graph contract: the list and its counters belong to the (W x H geometry, stream) state of bh_render.  The
 * first adaptive call of that key -- or the first of more frames than any before it -- allocates and is
 * refused on a capturing stream with BH_ERR_UNSUPPORTED before anything is queued; later calls allocate
 * nothing, never block the host and enqueue only capturable work (two memsets, the detect kernel, the
 * march).  An error after pass 1 was queued leaves the stream ordered. */
typedef struct {
    uint32_t ss;             /* 2, 4 or 8 */
    float threshold;         /* T above */
    uint8_t* tile_mask;      /* optional, device */
    uint32_t* refined_tiles; /* optional, device */
} bh_adaptive_desc;
int bh_render_adaptive(bh_ctx* ctx, const bh_camera_uniform* camera, const bh_uniforms* uniforms,
                       const bh_render_desc* desc, const bh_adaptive_desc* adaptive, void* hip_stream);
int bh_render_frames_adaptive(bh_ctx* ctx, uint32_t n_frames, const bh_camera_uniform* cameras,
                              const bh_uniforms* uniforms, const bh_render_desc* descs,
                              const bh_adaptive_desc* adaptive, void* hip_stream);
/* Host only (no device needed): the detect kernel's own lane code (csrc/bh_refine.hpp) over one frame's
 * row-major target(s) in `format` -> tile_mask, ceil(width / 8) * ceil(height / 8) bytes.  width and height
 * up to 32768; BH_ERR_INVALID_ARG as above. */
int bh_refine_mask_host(const void* col, const void* blackout_or_NULL, uint32_t width, uint32_t height,
                        uint32_t format, float threshold, uint8_t* tile_mask);
/* Host only: the stores of pass 2 for a mask -- the work items of its refined tiles mapped to tiles of the
 * virtual frame (csrc/bh_refine.hpp), their lanes to output pixels (csrc/bh_ss.hpp) -> pixel_writes,
 * width * height bytes: the number of stores each output pixel receives (1 inside refined tiles, else 0).
 * BH_ERR_INTERNAL if a store index falls outside the frame. */
int bh_refine_cover_host(uint32_t width, uint32_t height, uint32_t ss, const uint8_t* tile_mask, uint8_t* pixel_writes);

/* Lens maps: march a view once, shade it with any sky (not in the reference, whose every frame marches).
 * For a fixed camera the march's result per pixel -- where the ray ended and, for a sky ray, the two texture
 * coordinates of its sample (src/black_hole_maybe.wgsl:334-341) -- is a function of camera, uniforms, cap and
 * scene flags only, not of the sky or its size.  bh_render_lens stores it, 8 bytes per pixel; bh_shade_lens
 * turns it into the bytes bh_render would have written with that sky, bit for bit.  Exact math only.
 * The record (normative):
 *   sky rays (fate BH_FATE_CAP or BH_FATE_ESCAPE): (u, v) = the two fp32 arguments of the sample at :341 from
 *     the exact-math path: n = rd / sqrt(dot(rd, rd)), u = (RN_f32(atan2_f64(n.z, n.x)) + ONE_PI) / TWO_PI,
 *     v = 1 - (n.y + 1) * 0.5.  A sky ray's u is never negative (az + pi is +0 or >= 2^-22).  NaNs are stored
 *     as they come; the sampler's "NaN -> texel (0, 0)" rule applies at shade time.
 *   the other two fates: the sentinels below in u, v = +0.
 * Shading a record with a sky of w x h texels is the existing arithmetic and nothing else:
 *   u == BH_LENS_BLACKOUT -> col (0, 0, 0); u == BH_LENS_SURFACE -> col (1, 1, 1); otherwise the bilinear
 *   sample of :341 (Rgba8UnormSrgb, clamp to edge), then g, b <- c * sqrt(c) (:342-343);
 *   blackout_col = dot(col, col) < 1 ? 0 : col, in fp32 before the encode; alpha 1.
 * With ss = k in {2, 4, 8} the lens is that of the virtual frame k*width x k*height (bh_render_lens of that
 *   size with the output frame's camera uniform): each record is shaded as above, the blackout test per sample,
 *   the k x k block resolved by bh_render_ss's normative tree (pairwise along x, the same along y, one multiply
 *   by 1 / k^2, fp32, no FMA), then the format's encode -- the bytes of bh_render_ss, the march paid once per
 *   view instead of once per sky. */
typedef struct { float u, v; } bh_lens_px;      /* 8 bytes, row-major, lens[y * width + x] */
#define BH_LENS_BLACKOUT (-1.0f)                /* u of a ray with fate BH_FATE_BLACKOUT; v = +0 */
#define BH_LENS_SURFACE  (-2.0f)                /* u of a ray with fate BH_FATE_SURFACE;  v = +0 */
/* March the frame of `desc` and write only out_lens (device, width * height records, 8-byte aligned).  Taken
 * from the desc: width, height, max_iters, scene_flags, math, schedule.  BH_ERR_UNSUPPORTED, with a sentence in
 * bh_last_error(), for: math != BH_MATH_EXACT (fast math has no defined bits to promise), a layout other than
 * BH_LAYOUT_ROWMAJOR, shard_count != 1, a partition, a base schedule other than BH_SCHED_TILE, any dbg_*
 * pointer, a non-NULL out_col or out_blackout.  The BH_SCHED_FLAG_* flags are allowed.  It marches exactly
 * bh_render's rays in bh_render's tile order and shares that geometry's order state and repeated-frame key on
 * the stream, under bh_render's graph contract: the first call of a key allocates and is refused under capture. */
int bh_render_lens(bh_ctx* ctx, const bh_camera_uniform* camera, const bh_uniforms* uniforms, const bh_render_desc* desc,
                   bh_lens_px* out_lens, void* hip_stream);
/* A sky beside the context's own: rgba8_srgb as bh_create's (w * h * 4 bytes, each side 1..32768), uploaded to
 * the context's device before the call returns.  A bh_sky belongs to its context, is immutable, and must be
 * destroyed before bh_destroy -- after the shades that read it have completed; bh_destroy frees any that are
 * left (their handles are dangling from then on). */
typedef struct bh_sky bh_sky;
int bh_sky_create(bh_ctx* ctx, const uint8_t* rgba8_srgb, uint32_t w, uint32_t h, bh_sky** out);
int bh_sky_destroy(bh_sky* sky);
typedef struct {
    uint32_t width, height, ss, format;   /* output size; ss in {1,2,4,8}; bh_out_format */
    const bh_lens_px* lens;               /* (ss*height) x (ss*width) records, device, 8-byte aligned */
    const bh_sky* sky;                    /* NULL = the context's own sky */
    void* out_col; void* out_blackout;    /* row-major device images; out_blackout may be NULL */
} bh_shade_desc;
/* Shade a lens.  Asynchronous on the stream; allocates nothing and never synchronises, so it is capturable
 * from its first call; keeps no state between calls.  BH_ERR_INVALID_ARG for: ss outside {1, 2, 4, 8}, a NULL
 * or misaligned lens, a NULL out_col, a zero size, ss * width or ss * height above 65536, an unknown format, a
 * sky of another context. */
int bh_shade_lens(bh_ctx* ctx, const bh_shade_desc* desc, void* hip_stream);
/* Host only (no device needed): what the shade kernel runs (csrc/bh_lens.hpp), on the CPU, for tests -- the
 * render path never calls it.  lens: (ss*height) x (ss*width) records; sky_rgba8: sky_w x sky_h texels; the
 * outputs are fp32 RGBA, width x height (the RGBA32F bytes of bh_shade_lens).  BH_ERR_INVALID_ARG as above. */
int bh_lens_shade_host(const bh_lens_px* lens, uint32_t width, uint32_t height, uint32_t ss,
                       const uint8_t* sky_rgba8, uint32_t sky_w, uint32_t sky_h,
                       float* out_col_rgba, float* out_blackout_rgba_or_NULL);

/* Filtered lens shades: a mip chain of the sky, the level of each record taken from the lens (not in the
 * reference, whose one tap is textureSampleLevel(..., 0.0)).  bh_shade_lens takes one bilinear tap of level 0
 * per record, which aliases once neighbouring records land more than a texel apart: a sky finer than the frame,
 * and around the shadow rim whatever the sky.  A lens holds what a texture unit would use -- every record's
 * (u, v) beside its neighbours' -- so the footprint is a difference of two records.  Normative:
 * The chain of a sky of w0 x h0 texels.  Level 0 is the sky's RGBA8-sRGB texels.  Level l >= 1 is
 *   w_l x h_l = max(1, w_(l-1) >> 1) x max(1, h_(l-1) >> 1); n_levels = 1 + floor(log2(max(w0, h0))).  Texel
 *   (i, j) of level l, channels r, g, b: the sources are level l-1 at x0 = min(2i, w_(l-1) - 1),
 *   x1 = min(2i + 1, w_(l-1) - 1), y0 and y1 likewise, read as fp32 linear values (level 0 through the 256-entry
 *   sRGB decode table, levels >= 1 the stored half widened, which is exact); the value is
 *   RNE_f16(((a + b) + (c + d)) * 0.25f), a = T(x0, y0), b = T(x1, y0), c = T(x0, y1), d = T(x1, y1), in fp32
 *   without FMA.  Alpha is stored as 1.0.  A level is 4 halves per texel (r, g, b, a), row-major; the chain
 *   costs about 2/3 of level 0's bytes.
 * The level of a record (x, y) of a lens grid of Wv x Hv records (with ss, the virtual frame).  A record is
 *   valid iff u >= 0 && v == v (a sky ray, no NaN).  An invalid centre record is shaded as bh_shade_lens shades
 *   it and nothing else (the sentinels, NaN -> texel (0, 0)).  The neighbour on axis x is x + 1 if x + 1 < Wv,
 *   else x - 1, none if Wv == 1; the same on y.  Per axis, if the neighbour exists and is valid:
 *     du = |u_n - u|, if du > 0.5f then du = 1.0f - du (the seam; the sampler itself still does not wrap),
 *     dv = |v_n - v|, su = du * (float)w0, sv = dv * (float)h0, F = su * su + sv * sv; otherwise F = 0.
 *   rho2 = fmaxf(F_x, F_y).  q = (int32)bits(rho2) - 0x3f800000: log2(rho2) in 9.23 fixed point, the mantissa
 *   read as the fraction (no transcendentals).  If q <= 0 or n_levels == 1 the record is shaded as bh_shade_lens
 *   shades it, bit for bit.  Otherwise L = q >> 24, f = (float)(q & 0xffffff) * 0x1p-24f (exact), and
 *     if L >= n_levels - 1: c = sample_l(n_levels - 1); otherwise per channel c = cL * (1.0f - f) + cH * f with
 *     cL = sample_l(L), cH = sample_l(L + 1) (two multiplies and one add, no FMA, for f == 0 too);
 *     then g, b <- c * sqrtf(c).
 *   sample_l(0) is the bilinear sample of bh_shade_lens; sample_l(l >= 1) is the same arithmetic with (w_l, h_l)
 *   and the half texels widened, without the table.  The blackout test, the ss tree, the 1 / k^2 multiply and
 *   the encode are exactly bh_shade_lens's.
 * Not built: the filter inside bh_render and its ss / shutter / adaptive / presenter forms, anisotropic
 * footprints, a chain for the context's own sky, ss = 8, fast math, tiled or sharded layouts. */
/* bh_sky_create with the chain built on the device before the call returns.  Such a sky is usable wherever a
 * bh_sky is; bh_shade_lens reads its level 0 only. */
int bh_sky_create_mips(bh_ctx* ctx, const uint8_t* rgba8_srgb, uint32_t w, uint32_t h, bh_sky** out);
/* n_levels of a sky of bh_sky_create_mips, 0 for a sky of bh_sky_create. */
int bh_sky_levels(const bh_sky* sky, uint32_t* out_levels);
/* For tests: the sides of level `level` (1 .. n_levels - 1) and, with a non-NULL host_out, a synchronous copy of
 * its w * h * 4 halves.  BH_ERR_INVALID_ARG for a sky without a chain or a level outside that range. */
int bh_sky_read_level(const bh_sky* sky, uint32_t level, uint32_t* out_w, uint32_t* out_h, void* host_out_or_NULL);
/* bh_shade_lens with the filter above; the same contract (asynchronous, allocates nothing, keeps no state,
 * capturable from its first call).  BH_ERR_INVALID_ARG for everything bh_shade_lens refuses, and for a NULL sky
 * or a sky without a chain.  ss == 8 is BH_ERR_UNSUPPORTED with a sentence in bh_last_error(): filtering is what
 * replaces a large ss. */
int bh_shade_lens_mip(bh_ctx* ctx, const bh_shade_desc* desc, void* hip_stream);
/* Host only: level `level` (1 .. n_levels - 1) of the chain of a sky, w_l * h_l * 4 halves, by the functions
 * the chain kernels run (csrc/bh_lens.hpp). */
int bh_sky_mips_host(const uint8_t* sky_rgba8, uint32_t sky_w, uint32_t sky_h, uint32_t level, uint16_t* out_halves);
/* Host only: bh_lens_shade_host for bh_shade_lens_mip (ss in {1, 2, 4}). */
int bh_lens_shade_mip_host(const bh_lens_px* lens, uint32_t width, uint32_t height, uint32_t ss,
                           const uint8_t* sky_rgba8, uint32_t sky_w, uint32_t sky_h,
                           float* out_col_rgba, float* out_blackout_rgba_or_NULL);

/* Ray maps: the caller's direction per pixel, any projection (not in the reference, whose rays are its pinhole's).
 * A ray map (normative) is a device array of height x width x 3 fp32 values, row-major, 12 bytes per pixel, 4-byte
 * aligned: dirs[(y * width + x) * 3 + c].  Pixel (x, y) of a ray-map render is fs_main
 * (src/black_hole_maybe.wgsl:362-369) with in.camera_to_vertex = dirs[y][x] and camera.pos = pos: the kernel
 * normalises the vector exactly as the exact-math path normalises the interpolated one -- d / sqrt(dot(d, d)), one
 * rounding per op -- computes the ray's constant from it and marches; it does nothing else to the direction.  The
 * map is an input like the sky's bytes: how the caller made it is outside parity.  A vector whose normalisation is
 * not finite (the zero vector, an inf, a NaN) renders what the WGSL gives that normalised direction; a kernel reads
 * the 12 bytes of its own pixel and nothing else of the map, whatever they hold.  One origin per frame: `pos`.
 * Exact math only.  Several frames per call, a moving camera and shutter renders over one map: the posed forms
 * below (bh_ray_pose); an origin per ray beside a posed map: the origin maps below them.  Not built for ray maps:
 * adaptive renders, the tiled layouts, shards and partitions, fast math.
 *
 * bh_render_rays: bh_render (ss == 1; the dbg_* outputs are allowed) or bh_render_ss (ss = k in {2, 4, 8}: `dirs_dev`
 * is the map of the virtual frame, k*height x k*width x 3, its samples resolved by bh_render_ss's normative tree and
 * encoded once; dbg_* refused) with the map as the source of the directions.  Both targets (out_blackout may be
 * NULL), the three formats.  bh_render_lens_rays: bh_render_lens likewise; its records feed bh_shade_lens and
 * bh_shade_lens_mip as any lens does.
 * BH_ERR_INVALID_ARG: a NULL or misaligned dirs_dev, a NULL pos, ss outside {1, 2, 4, 8}, the size limits of
 * bh_render(_ss).  BH_ERR_UNSUPPORTED, with a sentence in bh_last_error() that starts with the function's name:
 * math != BH_MATH_EXACT, a layout other than BH_LAYOUT_ROWMAJOR, shard_count != 1, a partition, a base schedule
 * other than BH_SCHED_TILE (the BH_SCHED_FLAG_* flags are accepted; results never depend on them), and what
 * bh_render_ss / bh_render_lens refuse of the outputs.  A refused call launches nothing and writes nothing.
 * Graph contract: bh_render's -- the first call of a key allocates and is refused under capture, later calls are
 * capturable.  The temporal order and the repeated-frame key of a ray-map launch are its own: keyed by geometry,
 * stream and "ray map" (the map's address enters the repeated-frame key), so a bh_render of the same size on the
 * same stream neither inherits the map's tile costs nor loses its own.  A map rewritten in place under the same
 * address may meet a stale order: that costs time, never bytes. */
int bh_render_rays(bh_ctx* ctx, const float pos[3], const bh_uniforms* uniforms, const bh_render_desc* desc,
                   const float* dirs_dev, uint32_t ss, void* hip_stream);
int bh_render_lens_rays(bh_ctx* ctx, const float pos[3], const bh_uniforms* uniforms, const bh_render_desc* desc,
                        const float* dirs_dev, bh_lens_px* out_lens, void* hip_stream);
/* Host only: the map of bh_render's own projection -- for every pixel the UNNORMALISED interpolated vector of the
 * camera's screen triangle at the pixel centre, by the kernel's fp32 operations in its order (IEEE divisions by 2W
 * and 2H, l1 = (1 - l0) - l2, (l0 c0 + l1 c1) + l2 c2) -- into out_dirs (height * width * 3 floats).
 * bh_render_rays over it (uploaded, pos = camera->pos) is bh_render, bit for bit.  The starting point of any
 * "pinhole plus distortion" map.  BH_ERR_INVALID_ARG: a NULL pointer, a side of 0 or above 65536;
 * BH_ERR_UNSUPPORTED: a non-default screen triangle. */
int bh_ray_map_pinhole_host(const bh_camera_uniform* camera, uint32_t width, uint32_t height, float* out_dirs);

/* Posed ray maps: one map in CAMERA space, one pose per camera -- a camera path, several frames per launch and a
 * shutter through any projection without a new map per frame.  A pose (normative) is a position and three rows: */
typedef struct { float pos[3]; float r[3], u[3], f[3]; } bh_ray_pose;   /* 48 bytes */
/* Pixel (x, y) of camera i is fs_main with camera.pos = pose[i].pos and, with (mx, my, mz) = dirs[y][x],
 *     in.camera_to_vertex[c] = (mx * r[c] + my * u[c]) + mz * f[c]        (c = 0, 1, 2)
 * -- five fp32 operations per component, each rounded once, no contraction, in exactly this association -- and
 * then what bh_render_rays does with a map's vector: normalize_x, the ray's constant, the shared march.  The nine
 * basis floats are any values: nothing requires them to be orthonormal, so a mirror, a shear or a scale is a pose.
 * A non-finite product (inf * 0) gives what IEEE gives, and from there bh_render_rays' rule for non-finite vectors
 * applies.  A pose of unit axes (r, u, f = x, y, z) is NOT promised bit-equal to bh_render_rays of the same map for
 * vectors that hold a -0 or a non-finite component: x + (-0) is x only when x is not +0 ((+0) + (-0) = +0, so a -0
 * component can come out +0 after the sum with the other two products), and inf * 0 is NaN, so an infinite
 * component makes the other two components NaN.  Every finite vector without a -0 renders bh_render_rays' bytes.
 *
 * bh_render_frames_rays: bh_render_frames (ss == 1; the dbg_* outputs are allowed) or bh_render_frames_ss (ss = k in
 * {2, 4, 8}; dbg_* refused) with one shared map -- of the virtual frame when ss > 1 -- and one pose per frame:
 * n_frames in 1..BH_MAX_FRAMES (the inline table up to 32 frames, the stream's device table above), the three
 * formats, one or two targets.  bh_render_frames_shutter_rays: bh_render_frames_shutter over the map --
 * n_frames * n_sub poses, those of output frame f at poses[f * n_sub ..], n_sub in {2, 4, 8, 16} resolved by that
 * call's normative tree; n_sub == 1 is bh_render_frames_rays (a shutter kernel's lanes beyond the frame's right or
 * bottom edge read the map's pixel (0, 0) and drop it: reads stay inside the map).  bh_render_lens_rays_posed:
 * bh_render_lens_rays with a pose.  Refusals: those of bh_render_rays (a NULL or misaligned dirs_dev, math, layout, shards, partition, base
 * schedule, and what the outputs' form refuses) and of bh_render_frames(_shutter) (the frame and camera counts, descs
 * that differ in more than their outputs), with `poses` NULL as `pos` NULL; BH_ERR_UNSUPPORTED comes with a sentence
 * in bh_last_error() that starts with the function's name.  A refused call launches nothing and writes nothing.
 * Graph contract, temporal order: bh_render_rays' -- a posed launch is a ray-map launch of its geometry and stream
 * (it shares that state with bh_render_rays), and the map's address and every pose enter the repeated-frame key. */
int bh_render_frames_rays(bh_ctx* ctx, uint32_t n_frames, const bh_ray_pose* poses, const bh_uniforms* uniforms,
                          const bh_render_desc* descs, const float* dirs_dev, uint32_t ss, void* hip_stream);
int bh_render_frames_shutter_rays(bh_ctx* ctx, uint32_t n_frames, uint32_t n_sub, const bh_ray_pose* poses,
                                  const bh_uniforms* uniforms, const bh_render_desc* descs, const float* dirs_dev,
                                  uint32_t ss, void* hip_stream);
int bh_render_lens_rays_posed(bh_ctx* ctx, const bh_ray_pose* pose, const bh_uniforms* uniforms,
                              const bh_render_desc* desc, const float* dirs_dev, bh_lens_px* out_lens, void* hip_stream);
/* Host only: the formula above in plain C++ over a host map (height * width * 3 floats) into out_dirs (the same
 * size; may be `dirs` itself) -- the world-space map whose bh_render_rays, from pose->pos, is the posed render of
 * `dirs`, bit for bit.  BH_ERR_INVALID_ARG: a NULL pointer, a side of 0 or above 65536. */
int bh_ray_pose_apply_host(const bh_ray_pose* pose, const float* dirs, uint32_t width, uint32_t height, float* out_dirs);

/* Origin maps: a ray origin per pixel beside a posed direction map -- a finite aperture (thin-lens depth of field: the
 * k x k samples of ss are the lens samples), an eye per column (omnidirectional stereo), an orthographic view, a
 * side-by-side stereo pair in one frame.  An origin map (normative) is a device array of height x width x 3 fp32
 * values, row-major, 12 bytes per pixel, 4-byte aligned, of the geometry of the direction map it accompanies (with
 * ss = k both are the virtual frame's), in CAMERA space like that map.  For camera i and pixel (x, y), with
 * (ox, oy, oz) = origins[y][x], (mx, my, mz) = dirs[y][x] and pose[i] = (pos, r, u, f):
 *     w[c]   = (ox * r[c] + oy * u[c]) + oz * f[c]      five fp32 roundings, this association, no contraction
 *     ro0[c] = pos[c] + w[c]                            one more rounding
 *     d[c]   = (mx * r[c] + my * u[c]) + mz * f[c]      as bh_render_frames_rays
 * and the pixel is fs_main with camera.pos = ro0 and in.camera_to_vertex = d, that is get_col(Photon(ro0,
 * normalize(d))): the ray's constant is |ro0 x rd0|^2 and the photon-sphere marker's centre ((-normalize(ro0)) * 1.5)
 * * RS, with normalize(v) = v / sqrt((x x + y y) + z z) in IEEE fp32 -- what every frame's position gets today, here
 * per ray.  The origin bytes are an input like the direction bytes, any bit pattern: an origin at 0 (a NaN centre, a
 * zero constant), inside the unit sphere or non-finite renders what the WGSL gives that photon; a kernel reads the 12
 * bytes of its own pixel of each map and nothing else of either.
 * Identity: an origin map of all +0 renders bh_render_frames_rays' bytes for every pose whose nine basis floats are
 * finite and whose position has no -0 component: pos + (+0) = pos.  NOT promised otherwise: a -0 component of pos
 * becomes +0 ((-0) + (+0) = +0, which changes no radius but can change the sign of a zero downstream), and 0 * inf
 * is NaN, so a non-finite basis float makes every origin NaN.
 *
 * bh_render_frames_rays_origins: bh_render_frames_rays with origins_dev after dirs_dev -- n_frames poses over the one
 * pair of maps, ss in {1, 2, 4, 8}, the three formats, one or two targets, the dbg_* outputs where that call allows
 * them.  bh_render_lens_rays_origins: bh_render_lens_rays_posed likewise.  Refusals: those of the call it extends, and
 * BH_ERR_INVALID_ARG for a NULL or misaligned origins_dev; BH_ERR_UNSUPPORTED comes with a sentence in
 * bh_last_error() that starts with the function's name.  A refused call launches nothing and writes nothing.  Graph
 * contract, temporal order: bh_render_rays' -- the launch is a ray-map launch of its geometry and stream, and the
 * origin map's address enters the repeated-frame key beside the direction map's (a map rewritten in place may meet a
 * stale order: time, never bytes).  Not built with an origin map: the shutter form, adaptive renders, the tiled
 * layouts, shards and partitions, fast math, the pair and persistent schedules. */
int bh_render_frames_rays_origins(bh_ctx* ctx, uint32_t n_frames, const bh_ray_pose* poses, const bh_uniforms* uniforms,
                                  const bh_render_desc* descs, const float* dirs_dev, const float* origins_dev,
                                  uint32_t ss, void* hip_stream);
int bh_render_lens_rays_origins(bh_ctx* ctx, const bh_ray_pose* pose, const bh_uniforms* uniforms,
                                const bh_render_desc* desc, const float* dirs_dev, const float* origins_dev,
                                bh_lens_px* out_lens, void* hip_stream);
/* Host only: ro0 above in plain C++ over a host origin map (height * width * 3 floats) into out_origins (the same
 * size; may be `origins` itself) -- the world-space origins of the pose's rays, bit for bit what the kernels form.
 * BH_ERR_INVALID_ARG: a NULL pointer, a side of 0 or above 65536. */
int bh_ray_origins_apply_host(const bh_ray_pose* pose, const float* origins, uint32_t width, uint32_t height,
                              float* out_origins);

/* Hit maps: the lens march also stores where its surface rays ended (not in the reference, whose surfaces are white).
 * A hit map (normative) is a device array of height x width x 3 fp32 values, row-major, 12 bytes per pixel, 4-byte
 * aligned -- a ray map's layout: hits[(y * width + x) * 3 + c].  For a ray of fate BH_FATE_SURFACE the three values
 * are the ray's final ro: the position the loop's SDF test (:285-286) saw when it returned the surface colour, the
 * state before that iteration's RK update, bit for bit.  For every other fate they are (+0, +0, +0).
 * bh_render_lens_hits: bh_render_lens, which also writes out_hits -- the same lens bytes, the same refusals, order
 * state, repeated-frame key (which the hit map's address enters: a launch that writes one is not taken for one that
 * does not) and graph contract.  bh_render_lens_rays_posed_hits: bh_render_lens_rays_posed likewise; a pose of
 * unit axes (r, u, f = x, y, z) covers a plain world-space ray map, as far as that call promises.  BH_ERR_INVALID_ARG for a NULL or misaligned
 * out_hits; every bh_last_error() sentence starts with the function's name.  A refused call launches nothing and
 * writes nothing.  Not built: hit maps with an origin map, with ss resolved in the march (a hit map is per ray, as a
 * lens is: march the virtual frame and let the shade resolve), in fast math, in the tiled layouts, with shards or
 * partitions.  Additive, like the disc shades below: BH_ABI_VERSION unchanged, callers probe for the symbols. */
int bh_render_lens_hits(bh_ctx* ctx, const bh_camera_uniform* camera, const bh_uniforms* uniforms,
                        const bh_render_desc* desc, bh_lens_px* out_lens, float* out_hits, void* hip_stream);
int bh_render_lens_rays_posed_hits(bh_ctx* ctx, const bh_ray_pose* pose, const bh_uniforms* uniforms,
                                   const bh_render_desc* desc, const float* dirs_dev, bh_lens_px* out_lens,
                                   float* out_hits, void* hip_stream);

/* Arrival maps: the lens march also stores the direction its surface rays ended with.  An arrival map (normative) is a
 * device array with a hit map's layout: height x width x 3 fp32 values, row-major, 12 bytes per pixel, 4-byte aligned.
 * For a ray of fate BH_FATE_SURFACE the three values are the ray's final rd: the unnormalised direction of the state
 * the loop's SDF test saw -- the state whose ro the hit map holds -- before that iteration's RK update, bit for bit.
 * For every other fate they are (+0, +0, +0).
 * bh_march_lens_arrivals: bh_render_lens_hits, which also writes out_arrivals -- the same lens bytes and hit bytes, the
 * same refusals in the same order, order state, repeated-frame key (which the arrival map's address enters after the
 * hit map's) and graph contract.  bh_march_lens_rays_posed_arrivals: bh_render_lens_rays_posed_hits likewise.
 * BH_ERR_INVALID_ARG for a NULL or misaligned out_arrivals, with the other pointers' check; every bh_last_error()
 * sentence starts with the function's name.  A refused call launches nothing and writes nothing.  Not built, as for hit
 * maps: arrival maps with an origin map, with ss resolved in the march, in fast math, in the tiled layouts, with shards
 * or partitions.  Additive: BH_ABI_VERSION unchanged, callers probe for the symbols.  The names: bh_render_* are the
 * eighteen entry points whose refusals the census records (tests/test_gpu_refusals.py, which holds that list closed);
 * these two are the _hits requests with one more map, named for what they do -- the lens march -- and their refusals
 * are tested beside them (tests/test_gpu_beam.py). */
int bh_march_lens_arrivals(bh_ctx* ctx, const bh_camera_uniform* camera, const bh_uniforms* uniforms,
                            const bh_render_desc* desc, bh_lens_px* out_lens, float* out_hits, float* out_arrivals,
                            void* hip_stream);
int bh_march_lens_rays_posed_arrivals(bh_ctx* ctx, const bh_ray_pose* pose, const bh_uniforms* uniforms,
                                       const bh_render_desc* desc, const float* dirs_dev, bh_lens_px* out_lens,
                                       float* out_hits, float* out_arrivals, void* hip_stream);

/* Disc shades: bh_shade_lens with the surface records looked up in a disc texture (not in the reference).  The disc
 * is an immutable object beside bh_sky: n_phi x n_r RGBA8-sRGB texels (n_phi * n_r * 4 bytes, each side 1..32768),
 * x running around the disc and y from its inner edge to its outer edge, decoded through the 256-entry table the sky
 * uses, uploaded before bh_disc_create returns.  A bh_disc belongs to its context and is destroyed as a bh_sky is;
 * bh_destroy frees any that are left.
 * The colour of one record (u, v) whose entry of the hit map is p = (x, y, z) (normative; fp32, one rounding per op,
 * no FMA, except the angle):
 *   1. u != BH_LENS_SURFACE: bh_shade_lens's colour of the record, bit for bit.
 *   2. scene_flags without BH_SCENE_DISC: (1, 1, 1).
 *   3. rho = sqrtf(x*x + z*z); ri = 3.0f * rs; ro = 6.0f * rs;
 *      sd = fmaxf(fmaxf(rho - ro, -(rho - ri)), fabsf(y) - 0.02f)   -- sdf_accretion_disk (:103-105, :120) on p;
 *      unless sd < 0.001f is true the colour is (1, 1, 1): a marker hit, and every hit with a non-finite component
 *      that sd keeps.  fmaxf drops a NaN operand, as the march's own test does: a hit whose x or z is NaN and whose
 *      |y| < 0.021 classifies as disc and goes on.
 *   4. a = (rho - ri) / ri; k = ri / rho; w = k * sqrtf(k)   -- Keplerian: one turn of `spin` at the inner edge;
 *      t0 = (RN_f32(atan2_f64(z, x)) + ONE_PI) / TWO_PI   -- the constants and the division of the lens record's u;
 *      t1 = t0 - spin * w; t = t1 - floorf(t1); a t that is not >= 0 (NaN: a NaN component of p, or an rs at which
 *      w or a is not finite, rs = 0 among them) is taken as 0.  So t is in [0, 1] (1 when t1 is a tiny negative).
 *   5. the bilinear sample of :341's arithmetic (see bh_shade_lens) with the x axis wrapping:
 *      tx = t * (float)n_phi - 0.5f; x0 = floorf(tx) modulo n_phi (floorf(tx) is in [-1, n_phi - 1]); x1 = (x0 + 1)
 *      modulo n_phi; weight tx - floorf(tx).  ty = a * (float)n_r - 0.5f clamped to [-1, n_r] by fminf(fmaxf(ty,
 *      -1.0f), (float)n_r) (a NaN becomes -1), y0 = floorf(ty), y1 = y0 + 1, both clamped to [0, n_r - 1]; weight
 *      ty - floorf(ty).  top = t00 * (1 - fa) + t10 * fa, bot likewise, c = top * (1 - fb) + bot * fb per channel;
 *      then each channel is multiplied once by gain.  The c * sqrt(c) step of the sky sample is not applied.
 * blackout_col, ss and the encode are bh_shade_lens's: the blackout test per sample on this colour, the same tree.
 * Identity: a 1 x 1 disc of (255, 255, 255) with gain 1 gives bh_shade_lens's bytes for any spin. */
typedef struct bh_disc bh_disc;
int bh_disc_create(bh_ctx* ctx, const uint8_t* rgba8_srgb, uint32_t n_phi, uint32_t n_r, bh_disc** out);
int bh_disc_destroy(bh_disc* disc);
typedef struct {
    const float* hits;        /* the lens's hit map: (ss*height) x (ss*width) x 3 floats, device, 4-byte aligned */
    const bh_disc* disc;
    float rs;                 /* the uniforms' rs the lens was marched with */
    uint32_t scene_flags;     /* the desc's scene flags the lens was marched with */
    float spin;               /* turns of the inner edge, subtracted from the hit's angle; finite */
    float gain;               /* finite, >= 0 */
} bh_disc_desc;
/* bh_shade_lens's contract (asynchronous, allocates nothing, keeps no state, capturable from its first call; ss in
 * {1, 2, 4, 8}, the three formats, one or two targets).  BH_ERR_INVALID_ARG for everything bh_shade_lens refuses, and
 * for a NULL disc desc, a NULL or misaligned hits, a NULL disc or one of another context, unknown scene flags, a
 * non-finite spin, a gain that is negative or non-finite. */
int bh_shade_lens_disc(bh_ctx* ctx, const bh_shade_desc* desc, const bh_disc_desc* disc_desc, void* hip_stream);
/* Host only: bh_lens_shade_host for bh_shade_lens_disc -- hits: (ss*height) x (ss*width) x 3 floats; disc_rgba8:
 * n_phi x n_r texels.  BH_ERR_INVALID_ARG as above. */
int bh_lens_shade_disc_host(const bh_lens_px* lens, const float* hits, uint32_t width, uint32_t height, uint32_t ss,
                            const uint8_t* sky_rgba8, uint32_t sky_w, uint32_t sky_h,
                            const uint8_t* disc_rgba8, uint32_t n_phi, uint32_t n_r,
                            float rs, uint32_t scene_flags, float spin, float gain,
                            float* out_col_rgba, float* out_blackout_rgba_or_NULL);

/* Beamed disc shades: bh_shade_lens_disc with a disc hit's colour scaled by the fourth power of the frequency ratio g
 * between a Keplerian emitter in the disc and a static observer far away -- Doppler beaming and gravitational redshift:
 * the approaching side bright, the receding side dim, the inner edge darkened (not in the reference).  g is formed at
 * the hit from the hit map's p and the arrival map's d alone: in this integrator the acceleration is radial, so
 * L = p x d is conserved along a ray, and so is E^2 = |d|^2 - distortion_power * rs * |L|^2 / r^3 (to the RK4 step's
 * accuracy); the disc, 3 rs .. 6 rs, starts at the Schwarzschild ISCO, so a circular orbit exists over all of it.
 * The colour of one record (normative; fp32, one rounding per op, no FMA, dot(a, b) = (ax*bx + ay*by) + az*bz):
 *   1 to 5. bh_shade_lens_disc's.  Only a record that reaches step 5 -- a surface record of a scene with BH_SCENE_DISC
 *      whose hit p = (x, y, z) has sd < 0.001f -- goes on, with c its colour after the gain, rho, ri and rs as in step
 *      3 and d = (dx, dy, dz) its entry of the arrival map; no other record's arrival enters its colour.
 *   6. r2 = dot(p, p); r = sqrtf(r2);
 *      L = (y*dz - z*dy, z*dx - x*dz, x*dy - y*dx); h2 = dot(L, L);
 *      E2 = dot(d, d) - ((distortion_power * rs) * h2) / (r2 * r); E = sqrtf(E2).
 *   7. om = sqrtf((0.5f * rs) / ((rho * rho) * rho))   -- Kepler: Omega^2 = M / rho^3 with M = rs / 2;
 *      q = 1.0f - (1.5f * rs) / rho                    -- 1 / (u^t)^2 of the circular orbit;
 *      den = 1.0f - ((float)sense * om) * (L.y / E)    -- the traced ray runs backwards, so the photon's angular
 *      momentum about the disc's sense of rotation is L.y of p x d;
 *      g = sqrtf(q) / den.  Unless E2 > 0, q > 0, den > 0 and g < INFINITY are all true, g = 1: a zero arrival, NaN
 *      components, an rs at which the terms are not finite.
 *   8. ge = 1.0f + beam * (g - 1.0f); f = (ge * ge) * (ge * ge); colour = c * f per channel -- the bolometric
 *      I ~ g^4.  f is finite: a g other than 1 has q in (0, 1) and den >= 2^-24, so g < 2^24.
 * blackout_col, ss, the tree and the encode are bh_shade_lens_disc's.  beam = 0 gives bh_shade_lens_disc's bytes for
 * any arrival map; scaling every arrival by a power of two leaves the bytes unchanged (short of overflow).
 * Not applied: the camera's own gravitational blueshift (uniform over the frame: it belongs in `gain`) and the
 * camera's velocity -- g is the ratio seen by a static observer far away. */
typedef struct {
    const float* arrivals;    /* the lens's arrival map: (ss*height) x (ss*width) x 3 floats, device, 4-byte aligned */
    float beam;               /* 0 .. 1: 0 = bh_shade_lens_disc's bytes, 1 = the full factor */
    int32_t sense;            /* +1: the disc's matter moves towards growing atan2(z, x), the way a growing `spin`
                                 carries the texture; -1: the other way */
    float distortion_power;   /* the uniforms' distortion_power the lens was marched with; finite */
} bh_beam_desc;
/* bh_shade_lens_disc's contract and refusals; BH_ERR_INVALID_ARG also for a NULL beam desc, a NULL or misaligned
 * arrivals, a sense other than +1 or -1, a beam outside [0, 1] or not finite, a distortion_power that is not finite. */
int bh_shade_lens_disc_beamed(bh_ctx* ctx, const bh_shade_desc* desc, const bh_disc_desc* disc_desc,
                              const bh_beam_desc* beam_desc, void* hip_stream);
/* Host only: bh_lens_shade_disc_host for bh_shade_lens_disc_beamed -- arrivals: (ss*height) x (ss*width) x 3 floats. */
int bh_lens_shade_disc_beamed_host(const bh_lens_px* lens, const float* hits, uint32_t width, uint32_t height, uint32_t ss,
                                   const uint8_t* sky_rgba8, uint32_t sky_w, uint32_t sky_h,
                                   const uint8_t* disc_rgba8, uint32_t n_phi, uint32_t n_r,
                                   float rs, uint32_t scene_flags, float spin, float gain,
                                   float* out_col_rgba, float* out_blackout_rgba_or_NULL,
                                   const float* arrivals, float beam, int32_t sense, float distortion_power);

/* Bloom::render (src/bloom.rs:53-71): the reference's Kawase bloom + remix chain over the scene's two
 * targets, on BGRA8-sRGB images (bh_render with BH_OUT_BGRA8_SRGB): `col` (full_image_input),
 * `blackout` (blackout_input) -> `out` (the surface), all width x height (1..65536 each, as bh_render),
 * row-major, device memory.  `levels` = the Bloom's level count (src/state.rs:125 uses 3; 1..12).  Scratch textures live in
 * the context (allocated at the first call for a size; graph contract above).  `schedule`: BH_BLOOM_AUTO
 * fuses passes whenever that gives identical bytes (the host proves the chain's same-size samples are
 * identities on stored texels: powers of two, 1920x1080, 1280x720, ...), BH_BLOOM_LITERAL runs the
 * reference's render passes one by one.  Asynchronous on `hip_stream`. */
#define BH_BLOOM_AUTO    0u
#define BH_BLOOM_LITERAL 1u
int bh_bloom(bh_ctx* ctx, const void* col_bgra8, const void* blackout_bgra8, uint32_t width, uint32_t height,
             uint32_t levels, uint32_t schedule, void* out_bgra8, void* hip_stream);

/* Host only (no device needed): plan bh_bloom's chain for width x height, `levels`, `schedule` exactly as
 * bh_bloom does -- the same schedule choice, plans and kernel forms -- and, instead of launching, check
 * every launch's index arithmetic on the host: every block's staged footprint fits its LDS tile, every
 * tile read falls inside the staged footprint, every plan index and fix-up list entry inside its texture
 * (the kernels' own f32 sampler arithmetic, per block and tap).  BH_OK, or BH_ERR_INTERNAL with the first
 * violation in bh_last_error().  *out_launches (optional) = the launches the chain makes; out_plan (optional,
 * plan_len bytes, NUL-terminated, truncated) = one line per launch: "form ow oh tw th rx ry" (the kernel form,
 * its output and input sizes and resolution uniform; tools/bloom_roofline.py reads it). */
int bh_bloom_check(uint32_t width, uint32_t height, uint32_t levels, uint32_t schedule, uint64_t* out_launches,
                   char* out_plan, size_t plan_len);

/* Process-wide count of the plans real bh_bloom calls built and whose host check (the checks of
 * bh_bloom_check) refused: such a pass runs its general kernel -- the same bytes, slower -- and the first
 * refusal is also reported on stderr.  out_last (optional, len bytes, NUL-terminated, truncated) = the last
 * refusal's message.  0 for every frame size the tests name. */
int64_t bh_bloom_plan_failures(char* out_last, size_t len);

/* The frame the reference application presents per redraw, State::render (src/state.rs:270-286):
 * Scene::render into the two Bgra8UnormSrgb targets, then Bloom::render from them to the surface -- as one
 * pipelined path.  A presenter owns `depth` banks of `batch` target pairs, `march_streams` march streams and
 * one bloom stream of `ctx`'s device: call c marches its n frames (one bh_render_frames launch,
 * BH_OUT_BGRA8_SRGB, both targets) into bank c % depth on march stream c % march_streams, then blooms them on
 * the bloom stream.  So the bloom of call c fills the CUs the march of call c + 1 leaves idle instead of
 * adding to it, and (march_streams 2) the march of call c + 1 starts while the serial tail of call c's march
 * -- the few rays that run to the cap -- still runs, as the frames of one multi-frame launch overlap each
 * other's tails.  A call of 4 or more frames fills the GPU by itself (its frames overlap each other's tails in
 * one launch): it runs its march and then its blooms on the caller's stream, in order.  Each surface holds exactly the
 * bytes of bh_render + bh_bloom run one after the other.  Asynchronous: the blooms wait for the caller's
 * stream as it is at the call (earlier users of the surfaces), and the caller's stream waits for the
 * call's last bloom (later users see the finished surfaces); the host never blocks.  `bloom_cus` = 0: the
 * bloom's stream shares every CU at the device's highest priority; k > 0: the bloom runs on k CUs (spread
 * over the mask), the march on the others (hipExtStreamCreateWithCUMask).  The presenter's blooms share
 * `ctx`'s bloom scratch: do not run bh_bloom of the same ctx concurrently with it.  The first call of a
 * presenter allocates (order state, bloom scratch): do not capture it into a graph. */
#define BH_PRESENT_BATCH_MAX 32
#define BH_PRESENT_DEPTH_MAX 8
typedef struct bh_presenter bh_presenter;
typedef struct {
    uint32_t width, height;   /* frame size (1..65536) */
    uint32_t max_iters;       /* MAX_ITERATIONS, 1..65535 */
    uint32_t scene_flags;     /* BH_SCENE_* */
    uint32_t math;            /* bh_math_mode */
    uint32_t levels;          /* the Bloom's levels (src/state.rs:125: 3), 1..12 */
    uint32_t batch;           /* frames per bh_present_frames call, 1..BH_PRESENT_BATCH_MAX (1: one frame per redraw) */
    uint32_t bloom_cus;       /* 0: shared CUs, high-priority bloom stream; else CUs given to the bloom */
    uint32_t depth;           /* calls in flight: target banks, 2..BH_PRESENT_DEPTH_MAX (0: 3) */
    uint32_t march_streams;   /* 1 or 2, at most depth (0: 2 when the call's frames hold at most 64 tiles
                                 per CU -- a march that leaves the GPU mostly idle -- else 1) */
} bh_presenter_desc;
int bh_presenter_create(bh_ctx* ctx, const bh_presenter_desc* desc, bh_presenter** out);
int bh_presenter_destroy(bh_presenter* presenter);
/* n (1..batch) frames: cameras[i] -> out_surfaces[i] (width x height BGRA8 device images, caller-owned). */
int bh_present_frames(bh_presenter* presenter, uint32_t n, const bh_camera_uniform* cameras, const bh_uniforms* uniforms,
                      void* const* out_surfaces, void* hip_stream);
/* bh_present_frames of one frame: State::render. */
int bh_present(bh_presenter* presenter, const bh_camera_uniform* camera, const bh_uniforms* uniforms, void* out_surface,
               void* hip_stream);

/* Graph contract (see the top of this file): unpin every order state and bloom scratch set that a
 * capture marked, so that LRU eviction may free them again.  Call it only after destroying every HIP
 * graph captured from this ctx (their kernels read and write those buffers). */
int bh_graph_release(bh_ctx* ctx);

/* Number of 8x8 tiles owned by `shard_index` of `shard_count` in a width x height frame. */
int64_t bh_shard_tile_count(uint32_t width, uint32_t height, uint32_t shard_index, uint32_t shard_count);

/* Scatter the gathered tile-packed shards back into a row-major frame (rank 0 after the gather).
 * `packed` holds shard 0's tiles, then shard 1's, ... (the concatenation a gather produces, each
 * shard's block padded to `shard_stride_tiles` tiles); `bytes_per_pixel` is 4, 8 or 16. */
int bh_tiles_unpack(const void* packed, void* out_rowmajor, uint32_t width, uint32_t height,
                    uint32_t shard_count, uint64_t shard_stride_tiles, uint32_t bytes_per_pixel,
                    void* hip_stream);

/* As bh_tiles_unpack for BH_LAYOUT_TILES_RGB shards of `format` (bh_out_format): restores the
 * constant alpha (1.0 / 255) of the row-major frame. */
int bh_tiles_unpack_rgb(const void* packed, void* out_rowmajor, uint32_t width, uint32_t height,
                        uint32_t shard_count, uint64_t shard_stride_tiles, uint32_t format,
                        void* hip_stream);

/* As bh_tiles_unpack_rgb with at most `rows_in_flight` 8-pixel tile rows of the frame in flight at
 * once (0 = all; the kernel grid-strides over the rest).  For an unpack that overlaps a render on
 * the same GPU (rank 0 of the multi-GPU pipeline) a bounded value keeps it from displacing the
 * render's waves: at N=8 on the 4096x2048 frame, rank 0's render + unpack measured 0.099 ms per
 * frame with 64 rows in flight, 0.100 with all, 0.138 with 16. */
int bh_tiles_unpack_rgb_rows(const void* packed, void* out_rowmajor, uint32_t width, uint32_t height,
                             uint32_t shard_count, uint64_t shard_stride_tiles, uint32_t format,
                             uint32_t rows_in_flight, void* hip_stream);

/* Rank 0 of the multi-GPU frame: gathered BH_LAYOUT_TILES_RGBM shards of `format` -> BOTH targets of
 * Scene::render (src/scene.rs:476-509), row-major: `out_col` (alpha restored) and, unless NULL
 * (== Option::None), `out_blackout` = the tile mask's pixels zeroed (alpha kept), else col.  Equal
 * bit for bit to a single-GPU two-target bh_render.  `rows_in_flight` as bh_tiles_unpack_rgb_rows. */
int bh_tiles_unpack_rgbm(const void* packed, void* out_col, void* out_blackout, uint32_t width, uint32_t height,
                         uint32_t shard_count, uint64_t shard_stride_tiles, uint32_t format,
                         uint32_t rows_in_flight, void* hip_stream);
/* Weighted tile partitions (multi-GPU).  The default ownership gives every shard 1/shard_count of
 * the tiles; a partition gives shard k weights[k] of every M = sum(weights) residues: tile (tx, ty)
 * belongs to owner[(tx + 3*ty) % M], the M residues dealt to the shards by smooth weighted round
 * robin (each shard's residues spread evenly over the M), so that a shard with more work beside its
 * render -- rank 0, which also unpacks every frame -- can take a smaller share.  A shard's packed
 * order is row-major over its tiles, as for the default interleave.  weights[k] may be 0 (a shard
 * that renders nothing); M <= 4096.  The partition holds device tables on `device` (each shard's
 * tile list, and every tile's shard and packed index for the unpack); destroy it after the renders
 * and unpacks that use it have completed. */
int bh_partition_create(uint32_t width, uint32_t height, uint32_t shard_count, const uint32_t* weights, int device,
                        bh_partition** out);
int bh_partition_destroy(bh_partition* partition);
/* Tiles owned by `shard_index` (a shard's packed buffer holds this many tiles), or a negative status. */
int64_t bh_partition_tile_count(const bh_partition* partition, uint32_t shard_index);
/* Host only (no device needed): the same partition's map, tile t = ty * tiles_x + tx:
 * owner_out[t] = its shard, index_out[t] = its index in that shard's packed order (arrays of
 * tiles_x * tiles_y entries; either may be NULL). */
int bh_partition_map(uint32_t width, uint32_t height, uint32_t shard_count, const uint32_t* weights, uint32_t* owner_out,
                     uint32_t* index_out);
/* bh_tiles_unpack_rgbm for shards rendered with `partition` (its frame size and shard count). */
int bh_tiles_unpack_rgbm_partition(const void* packed, void* out_col, void* out_blackout, const bh_partition* partition,
                                   uint64_t shard_stride_tiles, uint32_t format, uint32_t rows_in_flight,
                                   void* hip_stream);

/* Bytes of one tile of `layout` (BH_LAYOUT_TILES*) in `format`, or a negative bh_status. */
int64_t bh_tile_bytes(uint32_t layout, uint32_t format);

/* The BGRA8 sRGB encoder's threshold table: out[k] (k = 1..255) = the smallest float x with
 * encode(x) >= k, out[0] = 0, out[256] = +inf; encode(x) = the largest k with x >= out[k]. */
int bh_srgb_encode_table(float* out257);

/* Diagnostics of a launch's host-side constants: the multiply-high magic a launch passes for its waves' divisions
 * by d with dividends up to n_max (0: none, the waves divide) in *magic; returns the number of n in [0, n_max] at
 * which (n * magic) >> 32 differs from n / d (0 when magic is 0), or a negative status. */
int64_t bh_div_magic_misses(uint32_t d, uint32_t n_max, uint32_t* magic);

/* Diagnostics of a launch's host-side constants: the first-step record of a frame -- what iteration 0 of the march
 * loop computes from the camera's position alone, the same in every ray of the frame: *dt0 = the step's dt,
 * *Q0 = (r^2 r^2) r and *rq0 = RN(1 / Q0) of the first rd_derivative, in IEEE f32.  Returns 1 when the record is valid
 * (the exact tile-schedule kernels then take iteration 0 from it), 0 when it is not (the outputs are then 0 and the
 * waves run iteration 0 themselves: non-finite inputs, delta_time_mult <= 0, rs <= 0, a camera at r^2 <= 1.01 or
 * > 2^24, a camera on a surface, dt0 outside [2^-25, 2^13] or above max_dist, max_iters < 2).  Output pointers may
 * be NULL.  Additive: BH_ABI_VERSION unchanged, callers probe for the symbol. */
int bh_first_step_host(const bh_camera_uniform* camera, const bh_uniforms* uniforms, uint32_t scene_flags,
                       uint32_t max_iters, float* dt0, float* Q0, float* rq0);

/* Diagnostics: check the correctly rounded division/sqrt cores the exact kernel uses against IEEE
 * results on `device` (op 0: sqrt over float bit patterns [base, base+count); op 1: x/6 over bit
 * patterns [base, base+count); op 2: n/d on `count` random pairs seeded by base; op 3: n/d near exact
 * quotients; op 4: the BGRA8 sRGB encoder over float bit patterns [base, base+count) against a
 * binary search of bh_srgb_encode_table; op 5: x/12 as the bloom chain computes it, over bit
 * patterns [base, base+count); op 6: the bloom chain's table-form sRGB encoder against op 4's; op 7:
 * n/d over all 2^23 numerator significands for the denominator significands (fraction bits)
 * [base, base + count/2^23); op 8: the shading's f32-rounded atan2 (short f64 core + library fallback)
 * against (float)atan2((double)y, (double)x) on `count` random (y, x) pairs seeded by base; op 9:
 * the number of those pairs the core hands to the fallback; op 10: the bloom chain's code-table form of
 * the sRGB encoder against op 4's over bit patterns [base, base+count); op 11: the march kernel's
 * wave-wide max of the tile costs (DPP scan) against a serial max, `count` random rounds per wave
 * seeded by base; op 12: the march step's reciprocal of rd_derivative's denominator seeded from the
 * square-root core's v_rsq, over q bit patterns [base, base+count), against the IEEE 1/Q; op 13: for the
 * q of that range whose seeded reciprocal differs from 1/Q, the division core with it over every numerator
 * significand against the IEEE quotient).  *out_mismatches = number of differing results;
 * out_examples (8 u32, optional) = up to two (a, b, got, want) bit patterns.  Synchronous. */
int bh_selftest_crmath(int op, uint64_t base, uint64_t count, uint64_t* out_mismatches,
                       uint32_t* out_examples, int device);

/* Diagnostics: the shader clock DURING march launches (the bench's "clock" block).  While armed
 * (acc != NULL), one wave in `stride` (a power of two) of the tile schedule's march kernels of this ctx --
 * dispatch slots k with (k + k / 256) % stride == 0, spread over the XCDs -- reads the shader-clock
 * counter (s_memtime) and the constant
 * 100 MHz counter (s_memrealtime) when it starts and when it ends, and adds the differences to its
 * XCD's slot: acc[16*x + 0] += shader ticks, acc[16*x + 1] += 100 MHz ticks, acc[16*x + 2] += 1 (x =
 * the XCD, 0..7; acc = 128 u64 of device memory, zeroed by the caller, 128 B per XCD).  The clock of
 * XCD x over the sampled waves' lifetimes is 100 MHz * acc[16x] / acc[16x+1].  Takes effect from the
 * next bh_render* call; never changes a result.  acc = NULL disarms. */
int bh_set_clock_probe(bh_ctx* ctx, uint64_t* acc, uint32_t stride);

#ifdef __cplusplus
}
#endif

#endif /* BH_RENDER_H */
