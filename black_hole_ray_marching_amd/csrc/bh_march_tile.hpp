// bh_march_tile.hpp -- the tile schedule (BH_SCHED_TILE, the default): the form mask (F_*), one dispatch slot marched
// by one wave in a form (march_slot), the shader-clock probe, the tile-schedule wave (march_tile_wave) and the shutter
// workgroup (shutter_workgroup) with the kernels that are their shells -- plain, supersampled, lens, ray-map, shutter --
// the work-list kernel, and the three launchers (launch_tile_schedule, launch_shutter_schedule,
// launch_refine_schedule).
// Needs bh_march_ray.hpp, bh_march_shade.hpp, bh_march_resolve.hpp and bh_refine.hpp (the work list).
#pragma once
#include "bh_march_ray.hpp"
#include "bh_march_resolve.hpp"
#include "bh_march_shade.hpp"
#include "bh_refine.hpp"

namespace bh {
namespace BH_NS {

// ---- schedule BH_SCHED_TILE: one wave64 = one 8x8 tile (default) ---------------------------------
// Dispatch slot -> tile through `order` (previous frame's per-tile cost, expensive tiles first) or
// the centre-out permutation; each wave records its tile's max n_rk for the next frame's order.
// wave_max_u32: bh_common.hpp

// The per-frame fields of frame fi of a launch: its camera (read before and in the march loop) and its outputs
// (read after it).  frames[0] == the top-level fields for a one-frame launch; launches of more than
// BH_INLINE_FRAMES frames read them from the device table.  Either way the frame's record is read through the
// constant address space -- the kernel argument lives there, and the table was staged on the stream before this
// launch -- at a wave-uniform index: scalar loads into SGPRs (one flat pointer chosen per wave made them vector
// loads into 15 VGPRs, three of which -- cps -- stayed live through every step of the loop).
#define BH_CONST_AS __attribute__((address_space(4)))
template <class T>
__device__ __forceinline__ const BH_CONST_AS T* const_as(const T* p) { return (const BH_CONST_AS T*)p; }
__device__ __forceinline__ const BH_CONST_AS FrameArgs* frame_args_of(const MarchArgs& A, uint32_t fi) {
    return (A.frame_table ? const_as(A.frame_table) : const_as(&A.frames[0])) + fi;
}
struct FrameCamera { float pos[3], c0[3], c1[3], c2[3], cps[3]; };
__device__ __forceinline__ FrameCamera load_camera(const BH_CONST_AS FrameArgs* F) {
    FrameCamera c;
    for (int k = 0; k < 3; ++k) {
        c.pos[k] = F->pos[k]; c.c0[k] = F->c0[k]; c.c1[k] = F->c1[k]; c.c2[k] = F->c2[k]; c.cps[k] = F->cps[k];
    }
    return c;
}
__device__ __forceinline__ void select_camera(MarchArgs& a, const FrameCamera& c) {
    for (int k = 0; k < 3; ++k) {
        a.pos[k] = c.pos[k]; a.c0[k] = c.c0[k]; a.c1[k] = c.c1[k]; a.c2[k] = c.c2[k]; a.cps[k] = c.cps[k];
    }
}
__device__ __forceinline__ void select_outputs(MarchArgs& a, const BH_CONST_AS FrameArgs* F) {
    a.out_col = F->out_col; a.out_blackout = F->out_blackout;
    a.dbg_n_rk = F->dbg_n_rk; a.dbg_fate = F->dbg_fate; a.dbg_steps = F->dbg_steps;
}

// What a wave learns from its dispatch slot before it touches a pixel, all of it wave-uniform and held in SGPRs:
// the frame and its camera, the shard-local tile and its coordinates.  slot_head issues the loads behind it (the
// order entry, the tile list's, the frame's record: scalar loads of data another kernel or the host wrote before
// this launch) so that a kernel can have them in flight while its table copy is (march_tile_wave).  The two
// divisions by launch constants are multiply-highs by the host's magics (bh_host.cpp, div_magic; 0: none, divide).
// ok == false: the order entry is out of range (defensive: a corrupt order must not address outside the shard).
// FS: the frame's first-step record too (bh_common.hpp FirstStep), three more words of the same trip -- behind the
// inline frames in the argument, or behind the n_frames entries of the staged table.  form_first_step says which forms
// ask for it: the exact builds', except the origin-map forms, whose rays do not start at the frame's position.
struct SlotHead {
    uint32_t fi, t, tx, ty;
    FrameCamera cam;
    FirstStep fs;
    bool ok;
};
__device__ __forceinline__ FirstStep load_first_step(const MarchArgs& A, uint32_t fi) {
    const BH_CONST_AS FirstStep* p = A.frame_table ? (const BH_CONST_AS FirstStep*)(const_as(A.frame_table) + A.n_frames)
                                                   : const_as(&A.first[0]);
    return {p[fi].dt0, p[fi].Q0, p[fi].rq0};
}
template <bool ITEM, bool FS = false>
__device__ __forceinline__ SlotHead slot_head(const MarchArgs& A, uint32_t slot, uint32_t item_tx = 0u, uint32_t item_ty = 0u) {
    SlotHead h{};
    const uint32_t nf = A.n_frames;
    uint32_t fi = 0, j = slot;
    if constexpr (ITEM) {
        fi = slot;
    } else if (nf > 1u) {
        j = A.nf_magic ? __umulhi(slot, A.nf_magic) : slot / nf;
        fi = slot - j * nf;
    }
    h.fi = fi;
    h.cam = load_camera(frame_args_of(A, fi));
    if constexpr (FS) h.fs = load_first_step(A, fi);
    if constexpr (ITEM) {
        h.tx = item_tx;
        h.ty = item_ty;
    } else {
        const uint32_t t = A.order ? const_as(A.order)[j] : centre_out(j, A.n_tiles, A.order_block, A.order_centre);
        h.t = t;
        if (t >= A.n_tiles) return h;
        if (A.tile_list) {  // weighted partition (bh_partition): the shard's tile list
            const uint32_t v = const_as(A.tile_list)[t];
            h.tx = v & 0xFFFFu;
            h.ty = v >> 16;
        } else if (A.shard_count == 1u && A.tx_magic) {
            h.ty = __umulhi(t, A.tx_magic);
            h.tx = t - h.ty * A.tiles_x;
        } else {
            shard_tile_coords(t, A.tiles_x, A.shard_index, A.shard_count, &h.tx, &h.ty);
        }
    }
    h.ok = true;
    return h;
}

// Several frames in one launch (bh_render_frames): dispatch slot s is tile s / n_frames of the order
// in frame s % n_frames, so every frame's expensive tiles start first and one frame's serial tail
// overlaps the others' bulk instead of ending the launch alone.  Only frame 0
// records the tile costs for the next launch's order (the histogram must count each tile once).
//
// One dispatch slot, marched by one wave in the form FORM: a mask of the bits F_SS ... F_ORG (below), named here
// without the prefix, as march_slot_body unpacks them.  SS: the supersampled form (march_tile_ss_kernel).  ITEM (with
// SS): a work item of the adaptive render (march_refine_kernel) -- `slot` is the frame and (item_tx, item_ty) the
// tile of the virtual frame, both given by the caller's work list: no dispatch order, no cost feedback.
// LENS (exact math, march_tile_lens_kernel): the epilogue stores the ray's lens record instead of shading it;
// `lut` is not read.
// SHUT (march_tile_shutter_kernel): a wave of a shutter workgroup -- the epilogue leaves the lane's samples in the
// wave's LDS area (after the k x k butterfly when A.ss_log2 != 0) and stores nothing; *sl receives the lane's
// pixel for the workgroup's resolve.  It stays as the caller set it (ok = false) when the tile is out of range.
// RAYS (exact math, the march_tile_rays_*_kernel forms): the lane's direction is the caller's -- normalize_x of the 12
// bytes of its pixel in the ray map `dirs` (bh_render_rays: row-major, the launch's width x height) -- instead of
// pixel_ray's; c0..c2, rw2 and rh2 are not read.  A lane outside the frame loads nothing and takes (0, 0, 1).
// POSE (with RAYS; the march_tile_rays_pose_*_kernel forms and march_tile_shutter_rays_kernel): the map is in camera
// space and the frame's c0, c1, c2 hold its camera's basis rows r, u, f (bh_ray_pose): the loaded (mx, my, mz) becomes
// (mx r + my u) + mz f, five roundings per component, before normalize_x.  The basis is wave-uniform and dead before
// the loop; with POSE a ray map also feeds a shutter wave (SHUT), whose n waves read the same 12 bytes per pixel --
// there without a branch: a lane outside the frame reads pixel (0, 0), inside any map, and still takes (0, 0, 1).
// ORG (with RAYS and POSE, not SHUT or ITEM; the march_tile_rays_org_*_kernel forms): the ray's origin is the lane's
// too -- its 12 bytes of the origin map `orgs` (bh_render_frames_rays_origins: camera space, the direction map's
// geometry), turned as the direction is and added to the frame's position -- so the Frame is formed per lane
// (org_load, slot_frame): ro0 and cps live in VGPRs through the loop, in these kernels alone.  The Frame of every
// other form comes from the same call, slot_frame<false>: a forced-inline template keeps their machine code byte for
// byte, which a lambda around the choice did not.
// HIT (with LENS, not ORG; the march_tile_lens_hits_kernel and march_tile_rays_pose_lens_hits_kernel forms): the epilogue
// stores the lens record as LENS does and, beside it, 12 bytes of the lane's pixel in the hit map `hits` (a ray map's
// layout): st.ro where the fate is BH_FATE_SURFACE, (+0, +0, +0) otherwise.  st.ro of such a lane is the position the
// step's SDF test saw, on every path through march_ray: a surface fate is decided before the RK update, and a step
// never writes its input.  The peeled first step ends no ray (step_first: the host's gate rules out every exit of
// iteration 0), so a surface fate comes from a step of the loop or of the tail.  In the ping-pong loop either arm
// leaves the step's input untouched and lane_end writes the iteration i into that input's n_rk; the other state holds
// 0 or 1 from the loop's start, so `sb.n_rk > st.n_rk` selects the input whenever it is sb (i >= 1, or i >= 2 behind
// a peeled step) and keeps st otherwise, the tie at i = 0 included -- whole states, ro with n_rk.  In the tail
// (march_cycles) march_step_tail copies st, steps into the copy and copies back: a lane that ends before the update
// gets its own state back.  The cycle fast-forward ends rays by the cap only.
// ARR (with HIT only; the march_tile_lens_arrivals_kernel and march_tile_rays_pose_lens_arrivals_kernel forms): the
// epilogue stores, beside the hit, 12 bytes of the lane's pixel in the arrival map `arrs` (the hit map's layout): st.rd,
// unnormalised, where the fate is BH_FATE_SURFACE, (+0, +0, +0) otherwise.  The argument above is about whole
// RayStates, so st.rd is the direction of the state whose ro the hit map holds; lens_record reads it already, so it
// is live here in every lens form.
// A form is a mask of these bits, one template argument of march_slot_body, march_slot, march_tile_wave and
// shutter_workgroup; march_slot_body's static_asserts say which masks are forms.
constexpr uint32_t F_SS = 1u, F_ITEM = 2u, F_LENS = 4u, F_SHUT = 8u, F_RAYS = 16u, F_POSE = 32u, F_ORG = 64u,
                   F_HIT = 128u, F_ARR = 256u;
constexpr bool form_first_step(uint32_t form) { return !BH_FAST && !(form & F_ORG); }
struct ShutterLane { uint32_t px, py; bool valid, ok; };
// The ORG form's prologue.  org_load: both 12-byte loads of a valid lane issued before either is used (one wait), and
//     d = (mx r + my u) + mz f,   ro0 = pos + ((ox r + oy u) + oz f)
// per component, one rounding per op in this association (bh_ray_pose's formula, twice); a lane outside the frame
// loads nothing and takes d = (0, 0, 1) and ro0 = pos.  slot_frame<true>: make_frame's per-frame invariants per lane
// -- cps = ((-normalize(ro0)) * 1.5) * RS as the host forms it per frame (bh_host.cpp, frame_args; normalize_x holds
// the IEEE form's bits, fallback included); FrameArgs::cps is not read.  slot_frame<false> is make_frame.
struct OrgRay { v3 d, ro0; };
__device__ __forceinline__ OrgRay org_load(const MarchArgs& a, const float* dirs, const float* orgs, uint32_t px,
                                           uint32_t py, bool valid) {
    OrgRay g;
    g.d = mk(0.0f, 0.0f, 1.0f);
    g.ro0 = mk(a.pos[0], a.pos[1], a.pos[2]);
    if (valid) {
        const size_t i = ((size_t)py * a.width + px) * 3u;
        const float* p = dirs + i;
        const float* q = orgs + i;
        const v3 m = mk(p[0], p[1], p[2]);
        const v3 o = mk(q[0], q[1], q[2]);
        const v3 r = mk(a.c0[0], a.c0[1], a.c0[2]), u = mk(a.c1[0], a.c1[1], a.c1[2]), fw = mk(a.c2[0], a.c2[1], a.c2[2]);
        g.d = add(add(smul(m.x, r), smul(m.y, u)), smul(m.z, fw));
        g.ro0 = add(g.ro0, add(add(smul(o.x, r), smul(o.y, u)), smul(o.z, fw)));
    }
    return g;
}
template <bool ORG>
__device__ __forceinline__ Frame slot_frame(const MarchArgs& a, const OrgRay& g) {
#if !BH_FAST
    if constexpr (ORG) {
        Frame f;
        f.ro0 = g.ro0;
        const v3 n = normalize_x(g.ro0);
        f.cps = muls(muls(mk(-n.x, -n.y, -n.z), 1.5f), a.rs);
        f.k = a.kfac;
        return f;
    } else
#endif
    return make_frame(a);
}
template <uint32_t FMT, uint32_t SF, uint32_t FORM>
__device__ __forceinline__ void march_slot_body(const MarchArgs& A, const SlotHead& h, const float* lut,
                                                uint32_t lane, ShutterLane* sl = nullptr, const float* dirs = nullptr,
                                                const float* orgs = nullptr, [[maybe_unused]] float* hits = nullptr,
                                                [[maybe_unused]] float* arrs = nullptr) {
    constexpr bool SS = FORM & F_SS, ITEM = FORM & F_ITEM, LENS = FORM & F_LENS, SHUT = FORM & F_SHUT,
                   RAYS = FORM & F_RAYS, POSE = FORM & F_POSE, ORG = FORM & F_ORG, HIT = FORM & F_HIT,
                   ARR = FORM & F_ARR;
    static_assert(SS || !ITEM, "work items are supersampled tiles");
    static_assert(!LENS || (!SS && !BH_FAST), "a lens is one record per ray, in exact math");
    static_assert(!SHUT || (!SS && !ITEM && !LENS), "a shutter wave takes its ss from the argument");
    static_assert(!RAYS || (!BH_FAST && !ITEM && (!SHUT || POSE)),
                  "a ray map feeds the exact plain, supersampled and lens forms, and posed the shutter form");
    static_assert(!POSE || RAYS, "a pose turns a ray map");
    static_assert(!ORG || (RAYS && POSE && !SHUT && !ITEM), "an origin map goes with a posed ray map, outside the shutter form");
    static_assert(!HIT || (LENS && !ORG), "a hit map goes with a lens, pinhole or posed ray map, without an origin map");
    static_assert(!ARR || HIT, "an arrival map goes with a hit map");
    const uint32_t fi = h.fi, t = h.t, tx = h.tx, ty = h.ty;
    MarchArgs a = A;
    select_camera(a, h.cam);
    if (ITEM || fi != 0u) a.tile_cost = nullptr;
    const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
    const bool valid = px < a.width && py < a.height;
    [[maybe_unused]] OrgRay og;  // ORG: the lane's turned direction and its origin
    if constexpr (ORG) og = org_load(a, dirs, orgs, px, py, valid);
    const Frame f = slot_frame<ORG>(a, og);
    RayState st;
    st.ro = f.ro0;
#if !BH_FAST
    if constexpr (RAYS) {
        // fs_main :362 with in.camera_to_vertex = the map's vector: any bit pattern, normalised as pixel_ray's is
        v3 d = mk(0.0f, 0.0f, 1.0f);
        if constexpr (ORG) {
            d = og.d;
        } else
        if constexpr (SHUT) {
            // a shutter wave: no branch on the lane -- a lane outside the frame reads pixel (0, 0), always inside
            // the map, and keeps (0, 0, 1)
            const float* p = dirs + ((size_t)(valid ? py : 0u) * a.width + (valid ? px : 0u)) * 3u;
            const v3 m = mk(p[0], p[1], p[2]);
            const v3 t = add(add(smul(m.x, mk(a.c0[0], a.c0[1], a.c0[2])), smul(m.y, mk(a.c1[0], a.c1[1], a.c1[2]))),
                             smul(m.z, mk(a.c2[0], a.c2[1], a.c2[2])));
            d = sel(valid, t, d);
        } else
        if (valid) {
            const float* p = dirs + ((size_t)py * a.width + px) * 3u;
            d = mk(p[0], p[1], p[2]);
            if constexpr (POSE)  // bh_ray_pose (include/bh_render.h): (mx r + my u) + mz f, in this association
                d = add(add(smul(d.x, mk(a.c0[0], a.c0[1], a.c0[2])), smul(d.y, mk(a.c1[0], a.c1[1], a.c1[2]))),
                        smul(d.z, mk(a.c2[0], a.c2[1], a.c2[2])));
        }
        st.rd = normalize_x(d);
    } else
#endif
    st.rd = pixel_ray(a, valid ? px : 0u, valid ? py : 0u);
    st.s = ray_s(f, st.rd);
    st.travelled = 0.0f;
    st.n_rk = 0;
    st.outside = 0u;
    uint32_t fate = 0xFFu, steps = 0;
    constexpr bool PEEL = form_first_step(FORM);
    if (valid) {
        // Iteration 0 from the frame's first-step record where it is valid (Q0 != 0: a scalar branch), ahead of the
        // choice of the step below: st becomes the ray after one RK update and s0 keeps the ray at the camera, the
        // loop's other state.  A lane whose operands leave a core's domain (step_first) sends the whole wave to the
        // loop's own iteration 0, which re-runs such lanes in IEEE ops.
        [[maybe_unused]] RayState s0 = st;
        [[maybe_unused]] uint32_t it0 = 0u;
#if !BH_FAST
        if constexpr (PEEL) {
            if (h.fs.Q0 != 0.0f) {
                RayState s1;
                const bool bad = step_first(st, s1, h.fs);
                if (__builtin_amdgcn_ballot_w64(bad) == 0ull) {
                    st = s1;
                    it0 = 1u;
                }
            }
        }
#endif
        // the camera outside the unit sphere (1.01 leaves room for any rounding of |ro0|^2 against the
        // step's own r^2 > 1 + 2^-23 at iteration 0) and |s| <= 2^30 on every lane: the step without the
        // ingoing test and the |s| guard (wave-uniform: a scalar branch)
        if constexpr (SF != SF_DYN) {
            // ORG: the origin is the lane's, so the choice is a property of the wave's valid lanes -- every one of
            // them outside, in the one ballot; any other mix takes the general step, which covers each lane
            // (a wave that took iteration 0 from the record has both: the record's gate and step_first's guard)
            const bool out = ORG ? __builtin_amdgcn_ballot_w64(!((dot(f.ro0, f.ro0) > 1.01f) & (fabsf(st.s) <= 0x1p30f))) == 0ull
                                 : (PEEL && it0 != 0u) ||
                                   ((dot(f.ro0, f.ro0) > 1.01f) && (__builtin_amdgcn_ballot_w64(!(fabsf(st.s) <= 0x1p30f)) == 0ull));
            if (__builtin_amdgcn_readfirstlane((int)out)) {
                march_ray<SF | SF_CAM_OUT, SHUT, PEEL>(a, f, st, fate, steps, lane, &s0, it0);
            } else {
                // it0 == 0 here: the ray at the camera, named as such -- this arm then needs nothing of step_first's,
                // which the camera-outside arm ahead of it would otherwise hold in registers through its loop
                if constexpr (PEEL) st = s0;
                march_ray<SF, SHUT>(a, f, st, fate, steps, lane);
            }
        } else {
            march_ray<SF, SHUT, PEEL>(a, f, st, fate, steps, lane, &s0, it0);
        }
    }
    if constexpr (SHUT) {
        // every lane (the k x k butterfly reads the wave's other lanes); no output pointer is read here
        shutter_stage(a, lut, lane, valid, fate, st, steps);
        *sl = ShutterLane{px, py, valid, true};
    } else
    if constexpr (SS) {
        // every lane takes the resolve (its butterfly reads the wave's other lanes); invalid lanes hold 0
        uint32_t fo = fi;
        asm volatile("" : "+s"(fo));
        select_outputs(a, frame_args_of(A, fo));
        v3 sc, sb;
        ss_samples(a, lut, lane, valid, fate, st, steps, sc, sb);
        ss_resolve_store<FMT>(a, lut, lane, px, py, valid, sc, sb);
    } else
    if (valid) {
        // the frame's output pointers are loaded here, from an opaque copy of the frame index: loaded
        // up front they would hold 10 SGPRs through the march loop, over the 80 that keep 8
        // workgroups per CU resident (MI355X_MICROARCH.md, Residency)
        uint32_t fo = fi;
        asm volatile("" : "+s"(fo));
        select_outputs(a, frame_args_of(A, fo));
#if !BH_FAST
        if constexpr (LENS) {
            // out_col is the lens (bh_render_lens: row-major, whole frame): one 8-byte vector store per lane
            reinterpret_cast<float2*>(a.out_col)[(size_t)py * a.width + px] = lens_record(fate, st.rd);
            if constexpr (HIT) {
                // the hit map (row-major, whole frame, 4-byte aligned): where a surface ray ended, +0 for any other
                const bool on = fate == (uint32_t)BH_FATE_SURFACE;
                float* q = hits + ((size_t)py * a.width + px) * 3u;
                q[0] = on ? st.ro.x : 0.0f;
                q[1] = on ? st.ro.y : 0.0f;
                q[2] = on ? st.ro.z : 0.0f;
                if constexpr (ARR) {
                    // the arrival map (the hit map's layout): the direction that ray ended with, +0 for any other
                    float* w = arrs + ((size_t)py * a.width + px) * 3u;
                    w[0] = on ? st.rd.x : 0.0f;
                    w[1] = on ? st.rd.y : 0.0f;
                    w[2] = on ? st.rd.z : 0.0f;
                }
            }
        } else
#endif
        {
        const v3 col = shade(a, lut, fate, st.rd);
        write_pixel<FMT>(a, lut, out_index(a, t, lane, px, py), col, st.n_rk, fate, steps);
        }
    }
    if (a.tile_cost) {
        // the next frame's cost and its bucket histogram (a no-return atomic: the wave does not wait);
        // the last bucket is the remainder and is not counted
        const uint32_t m = min(wave_max_u32(steps) >> 1, 255u);
        if (lane == 0u) {
            a.tile_cost[t] = (uint8_t)m;
            const uint32_t b = cost_bucket(m);
            if (b < ORDER_BUCKETS - 1u)
                __hip_atomic_fetch_add(&a.order_tot[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// Head and body back to back: the shutter workgroups' waves and the work-list march's items.
template <uint32_t FMT, uint32_t SF, uint32_t FORM>
__device__ __forceinline__ void march_slot(const MarchArgs& A, uint32_t slot, const float* lut,
                                           uint32_t lane, uint32_t item_tx = 0u, uint32_t item_ty = 0u,
                                           ShutterLane* sl = nullptr, const float* dirs = nullptr,
                                           const float* orgs = nullptr) {
    const SlotHead h = slot_head<(FORM & F_ITEM) != 0u, form_first_step(FORM)>(A, slot, item_tx, item_ty);
    if (!h.ok) return;
    march_slot_body<FMT, SF, FORM>(A, h, lut, lane, sl, dirs, orgs);
}

// Shader-clock probe (bh_set_clock_probe): a sampled wave reads both counters when it starts and adds
// the differences at its end to its XCD's accumulators (vector atomics from lane 0, no return).  (A
// divergent lane-0 branch before the march trips an "illegal VGPR to SGPR copy" in this compiler, so
// the start values are held in 2 SGPRs instead: their low 32 bits, since a wave lives far less than
// 2^32 shader cycles.)
struct ClockStart { uint32_t t, r; };
__device__ __forceinline__ ClockStart clock_start() {
    return {(uint32_t)__builtin_amdgcn_s_memtime(), (uint32_t)__builtin_amdgcn_s_memrealtime()};
}
__device__ __forceinline__ void clock_end(unsigned long long* acc, const ClockStart& c0) {
    const uint32_t t = (uint32_t)__builtin_amdgcn_s_memtime() - c0.t;      // shader clock
    const uint32_t r = (uint32_t)__builtin_amdgcn_s_memrealtime() - c0.r;  // constant 100 MHz
    const uint32_t x = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u;  // HW_REG_XCC_ID[2:0]
    // a sample whose ratio is outside 0.5-4 GHz is dropped: a wave saved and restored elsewhere (queue
    // preemption) reads another XCD's shader counter at its end (seen once: 20 GHz on two XCDs)
    const bool sane = (uint64_t)t >= 5ull * r && (uint64_t)t <= 40ull * r;
    if ((threadIdx.x & 63u) == 0u && sane) {
        unsigned long long* p = acc + 16u * x;
        __hip_atomic_fetch_add(p, (unsigned long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(p + 1, (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(p + 2, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One wave of the tile schedule: its dispatch slot (the grid covers every slot, WG_WAVES waves per workgroup),
// marched in march_slot_body's form FORM (of F_SS, F_LENS, F_RAYS, F_POSE, F_ORG, F_HIT, F_ARR), between the clock probe's two
// readings.
// The wave's start is one trip to memory deep where it can be: the table copy's loads (lut != null: 16 bytes of
// each table per lane, srgb_fetch) are issued first and awaited last, and the slot's own chain -- kernel argument,
// order entry and frame record, tile list -- runs on the scalar unit while they fly (slot_head); then the one LDS
// store per table and the workgroup's barrier.  (The copy by four guarded loads, each awaited, then the barrier,
// then the chain through vector loads put about eight dependent round trips in front of pixel_ray's first
// multiply: DESIGN.md §5 item 32.)
template <uint32_t FMT, uint32_t SF, uint32_t FORM>
__device__ __forceinline__ void march_tile_wave(const MarchArgs& A, float* lut, const float* dirs = nullptr,
                                                const float* orgs = nullptr, float* hits = nullptr,
                                                float* arrs = nullptr) {
    static_assert(WG_WAVES == 1u, "the table copy is one wave's: 64 lanes x 16 bytes per table");
    static_assert(!(FORM & (F_ITEM | F_SHUT)), "work items and shutter waves have kernels of their own");
    constexpr bool LENS = FORM & F_LENS;
    // every argument word the start branches on or indexes with, wanted here: one group of scalar loads and one
    // wait for them (left to their uses, each is loaded in the block of its use and waited for there in turn)
    asm volatile("" ::"s"(A.srgb_lut), "s"(A.n_tiles), "s"(A.n_frames), "s"(A.nf_magic), "s"(A.frame_table),
                 "s"(A.order), "s"(A.tile_list), "s"(A.shard_count), "s"(A.tx_magic), "s"(A.tiles_x), "s"(A.clk),
                 "s"(A.clk_mask), "s"(A.width), "s"(A.height), "s"(A.rw2), "s"(A.rh2));
    SrgbRows<FMT> rows;
    if constexpr (!LENS) rows = srgb_fetch<FMT>(A);
    const uint32_t slot = __builtin_amdgcn_readfirstlane(blockIdx.x * WG_WAVES + (threadIdx.x >> 6));
    if (slot >= A.n_tiles * A.n_frames) return;  // wave-uniform, and the wave is its workgroup: nobody waits for it
    const SlotHead h = slot_head<false, form_first_step(FORM)>(A, slot);
    if constexpr (!LENS) {
        srgb_store<FMT>(rows, lut);
        __syncthreads();
    }
    // one slot in `stride`, rotated by slot / stride: the dispatcher deals workgroups to the 8 XCDs
    // round robin, so plain multiples of the stride would all land on one XCD
    const bool probe = A.clk && ((slot + (slot >> 8)) & A.clk_mask) == 0u;
    ClockStart c0{0u, 0u};
    if (probe) c0 = clock_start();
    if (h.ok) march_slot_body<FMT, SF, FORM>(A, h, lut, threadIdx.x & 63u, nullptr, dirs, orgs, hits, arrs);
    if (probe) clock_end(A.clk, c0);
}

// The plain form.
template <uint32_t FMT, uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_kernel(MarchArgs A) {
    __shared__ __attribute__((aligned(16))) float lut[lds_tables<FMT>()];
    march_tile_wave<FMT, SF, 0u>(A, lut);
}

// The tile schedule's supersampled form (bh_render_ss, ss > 1): the same waves over the virtual frame's
// tiles -- order, cost feedback, cycle fast-forward, frame interleave and shading as march_tile_kernel --
// with the k x k resolve as the epilogue (ss_resolve_store).  k is a run-time value (a.ss_log2): one more
// kernel per format and scene-flag fold, not three.
template <uint32_t FMT, uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_ss_kernel(MarchArgs A) {
    __shared__ __attribute__((aligned(16))) float lut[lds_tables<FMT>()];
    march_tile_wave<FMT, SF, F_SS>(A, lut);
}

// The tile schedule's shutter form (bh_render_shutter): one workgroup of n = 2^ln waves per (output frame, tile)
// -- workgroup g takes order index g / n_frames of output frame g % n_frames, wave w the frame's camera w
// (bh_shutter.hpp; A.n_frames counts CAMERAS, n per output frame, and wave_slot names march_slot's own slot of
// that pair) -- marched by march_slot as any other tile: order, cost feedback (camera 0 of frame 0 only), cycle
// fast-forward, shading, and bh_render_ss's butterfly when A.ss_log2 != 0.  Then the resolve: each wave leaves
// its samples in its own history area (shutter_stage), one barrier, and the writer lanes of wave 0 (col) and
// wave 1 (blackout_col, when the frame has that target) sum the n waves' samples in tree order, scale, encode
// and store (shutter_resolve_store).  No intermediate in global memory.
// Dynamic LDS: n history areas, then one copy of the tables (shutter_lds_bytes) -- 9 to 10 KiB at n = 2 (per wave no
// more than the plain kernel's workgroups hold), 65 to 66 KiB at n = 16 (two workgroups per CU).
// Registers: 8 waves per SIMD are asked for (64 VGPRs; the exact builds' default-scene kernels then spill 3 to 5
// of them to scratch).  At the 67 to 71 the compiler takes unasked, a SIMD holds 7 waves, a CU 28, and a
// workgroup of 16 waves fits once, not twice: n = 16 measured 1.41x its yardstick, 1.05 to 1.07x with the
// request, n = 8 1.03 to 1.05x in place of 1.07 to 1.08x, n = 4 unchanged.
template <uint32_t FMT>
constexpr uint32_t shutter_lds_bytes(uint32_t ln) { return (uint32_t)(sizeof(HistLds) << ln) + (uint32_t)(lds_tables<FMT>() * sizeof(float)); }
// One wave of shutter workgroup g, from its wave index on: the march in the form FORM (F_SHUT, over a posed ray map
// with F_RAYS | F_POSE and `dirs`), the workgroup's second barrier, the writer waves' resolve and store.  The kernels
// are shells around it that keep what comes before: the table copy, its barrier and the early return.
// Barrier discipline: every wave of the workgroup arrives at the barrier here, whatever its march did.  Between the
// table copy's barrier and this one there is one return, the shell's, on blockIdx and kernel arguments alone (the
// whole workgroup or none of it); march_slot's defensive return (a tile index out of range: the same order entry for
// all n waves) only returns to this function, ahead of the barrier; and no code on the way sits under a lane- or
// wave-dependent branch that holds a barrier -- the ray map is loaded inside march_slot without a branch or a return
// of its own (a lane outside the frame reads pixel (0, 0) and a select drops what it read).  A wave whose lanes are
// all outside the frame marches nothing and stages zeros.  The shell's return stays in the shells because the
// compiler emits other code for it from here: with the whole kernel in this function the table copy's prologue comes
// out in another order, with the return alone its compare and branch flip polarity, in all 42 shutter kernels.
template <uint32_t FMT, uint32_t SF, uint32_t FORM>
__device__ __forceinline__ void shutter_workgroup(const MarchArgs& A, uint32_t ln, uint32_t g, uint32_t n_out, float* lut,
                                                  const float* dirs = nullptr) {
    static_assert((FORM & F_SHUT) != 0u, "a shutter workgroup marches shutter waves");
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t slot = shutter::wave_slot(g, w, n_out, ln);
    const bool probe = A.clk && ((slot + (slot >> 8)) & A.clk_mask) == 0u;  // as march_tile_wave
    ClockStart c0{0u, 0u};
    if (probe) c0 = clock_start();
    ShutterLane sl{0u, 0u, false, false};
    march_slot<FMT, SF, FORM>(A, slot, lut, lane, 0u, 0u, &sl, dirs);
    if (probe) clock_end(A.clk, c0);
    __syncthreads();
    if (!sl.ok || w > 1u) return;
    const BH_CONST_AS FrameArgs* F = frame_args_of(A, slot % A.n_frames);
    void* out = w == 0u ? F->out_col : F->out_blackout;
    if (!out) return;  // wave 1 of a frame without the second target: neither resolved nor written
    const uint32_t lk = A.ss_log2;
    if (sl.valid && ss::writer(lane, lk))
        shutter_resolve_store<FMT>(out, w, ln, lane, ss::out_index(sl.px, sl.py, lk, A.ss_out_width), lut);
}
template <uint32_t FMT, uint32_t SF>
__global__ void __launch_bounds__(64u << shutter::MAX_LOG2) __attribute__((amdgpu_waves_per_eu(8)))
march_tile_shutter_kernel(MarchArgs A, uint32_t ln) {
    float* lut = reinterpret_cast<float*>(shutter_hist_lds() + (1u << ln));
    // the tables by a loop of its own: load_srgb_tables' stride is a compile-time constant, this workgroup's size
    // is not, and its form of the loop gives these kernels other machine code than the one they were measured with
    const uint32_t nt = 64u << ln;
    for (uint32_t i = threadIdx.x; i < (uint32_t)lds_tables<FMT>(); i += nt)
        lut[i] = i < 256u ? A.srgb_lut[i] : A.srgb_enc[i - 256u];
    __syncthreads();
    const uint32_t n_out = A.n_frames >> ln;  // output frames
    const uint32_t g = blockIdx.x;
    if (g >= A.n_tiles * n_out) return;  // blockIdx and kernel arguments only: the whole workgroup or none of it
    shutter_workgroup<FMT, SF, F_SHUT>(A, ln, g, n_out, lut);
}

// The kernels from here to the work-list march are the exact builds' alone (march_slot_body's static_asserts).
// The tile schedule's lens form (bh_render_lens): march_tile_kernel's waves -- order, cost feedback, cycle
// fast-forward -- with the lens record as the epilogue: no sky, no tables, no encode, one kernel per
// scene-flag fold.
template <uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_lens_kernel(MarchArgs A) {
    march_tile_wave<BH_OUT_RGBA32F, SF, F_LENS>(A, nullptr);
}

// The tile schedule's ray-map forms (bh_render_rays, bh_render_lens_rays): the plain, supersampled and lens kernels
// with march_slot's RAYS switch -- the lane's direction from the caller's map, everything after it shared.  The map
// is a second kernel argument of these kernels only (MarchArgs has no free word, and its layout is what the other
// kernels were compiled against); it is read once per lane, before the loop.
template <uint32_t FMT, uint32_t SF, bool SS>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_rays_kernel(MarchArgs A, const float* dirs) {
    __shared__ __attribute__((aligned(16))) float lut[lds_tables<FMT>()];
    march_tile_wave<FMT, SF, (SS ? F_SS : 0u) | F_RAYS>(A, lut, dirs);
}
template <uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_rays_lens_kernel(MarchArgs A, const float* dirs) {
    march_tile_wave<BH_OUT_RGBA32F, SF, F_LENS | F_RAYS>(A, nullptr, dirs);
}

// The posed ray-map forms (bh_render_frames_rays, bh_render_lens_rays_posed): the ray-map kernels over a map in camera
// space, with march_slot_body's POSE switch and any number of frames -- frame fi's FrameArgs holds its camera's
// position and basis (bh_ray_pose), every frame reads the one map.
template <uint32_t FMT, uint32_t SF, bool SS>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_rays_pose_kernel(MarchArgs A, const float* dirs) {
    __shared__ __attribute__((aligned(16))) float lut[lds_tables<FMT>()];
    march_tile_wave<FMT, SF, (SS ? F_SS : 0u) | F_RAYS | F_POSE>(A, lut, dirs);
}
template <uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_rays_pose_lens_kernel(MarchArgs A, const float* dirs) {
    march_tile_wave<BH_OUT_RGBA32F, SF, F_LENS | F_RAYS | F_POSE>(A, nullptr, dirs);
}

// The posed ray-map forms with an origin map (bh_render_frames_rays_origins, bh_render_lens_rays_origins): the posed
// kernels with march_slot_body's ORG switch -- the lane's origin from a second camera-space map of the same geometry,
// the third argument of these kernels only (MarchArgs and FrameArgs keep their layout).
template <uint32_t FMT, uint32_t SF, bool SS>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_rays_org_kernel(MarchArgs A, const float* dirs, const float* orgs) {
    __shared__ __attribute__((aligned(16))) float lut[lds_tables<FMT>()];
    march_tile_wave<FMT, SF, (SS ? F_SS : 0u) | F_RAYS | F_POSE | F_ORG>(A, lut, dirs, orgs);
}
template <uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_rays_org_lens_kernel(MarchArgs A, const float* dirs, const float* orgs) {
    march_tile_wave<BH_OUT_RGBA32F, SF, F_LENS | F_RAYS | F_POSE | F_ORG>(A, nullptr, dirs, orgs);
}

// The lens forms with a hit map (bh_render_lens_hits, bh_render_lens_rays_posed_hits): the pinhole and the posed
// ray-map lens kernels with march_slot_body's HIT switch -- the epilogue's second store -- and the map as the last
// argument of these kernels only.
template <uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_lens_hits_kernel(MarchArgs A, float* hits) {
    march_tile_wave<BH_OUT_RGBA32F, SF, F_LENS | F_HIT>(A, nullptr, nullptr, nullptr, hits);
}
template <uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_rays_pose_lens_hits_kernel(MarchArgs A, const float* dirs, float* hits) {
    march_tile_wave<BH_OUT_RGBA32F, SF, F_LENS | F_RAYS | F_POSE | F_HIT>(A, nullptr, dirs, nullptr, hits);
}

// The same two with an arrival map (bh_march_lens_arrivals, bh_march_lens_rays_posed_arrivals): march_slot_body's ARR
// switch -- the epilogue's third store -- and the map as the last argument, after `hits`.
template <uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_lens_arrivals_kernel(MarchArgs A, float* hits, float* arrs) {
    march_tile_wave<BH_OUT_RGBA32F, SF, F_LENS | F_HIT | F_ARR>(A, nullptr, nullptr, nullptr, hits, arrs);
}
template <uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_tile_rays_pose_lens_arrivals_kernel(MarchArgs A, const float* dirs, float* hits,
                                                                                          float* arrs) {
    march_tile_wave<BH_OUT_RGBA32F, SF, F_LENS | F_RAYS | F_POSE | F_HIT | F_ARR>(A, nullptr, dirs, nullptr, hits, arrs);
}

// The shutter form over a posed ray map (bh_render_frames_shutter_rays): march_tile_shutter_kernel's shell with the
// map as the second argument, and shutter_workgroup with the F_RAYS and F_POSE bits -- the n waves of a workgroup read
// the same 12 bytes per pixel and differ in their FrameArgs' pose.
template <uint32_t FMT, uint32_t SF>
__global__ void __launch_bounds__(64u << shutter::MAX_LOG2) __attribute__((amdgpu_waves_per_eu(8)))
march_tile_shutter_rays_kernel(MarchArgs A, const float* dirs, uint32_t ln) {
    float* lut = reinterpret_cast<float*>(shutter_hist_lds() + (1u << ln));
    const uint32_t nt = 64u << ln;
    for (uint32_t i = threadIdx.x; i < (uint32_t)lds_tables<FMT>(); i += nt)
        lut[i] = i < 256u ? A.srgb_lut[i] : A.srgb_enc[i - 256u];
    __syncthreads();
    const uint32_t n_out = A.n_frames >> ln;  // output frames
    const uint32_t g = blockIdx.x;
    if (g >= A.n_tiles * n_out) return;  // blockIdx and kernel arguments only: the whole workgroup or none of it
    shutter_workgroup<FMT, SF, F_SHUT | F_RAYS | F_POSE>(A, ln, g, n_out, lut, dirs);
}

// The adaptive render's second pass (bh_render_adaptive; bh_refine.hpp): the supersampled march over a work
// list that the detect kernel (bh_tiles.hip) left on the device.  The host never learns the list's length, so
// the grid is a bounded number of waves (RefineArgs::capacity bounds the list, the launcher the grid) and each
// wave pulls work items until they pass entries * k^2: lane 0's vector atomic on a head word, broadcast.  One
// head word serves about 88 pulls per microsecond however many waves pull (MI355X), less than these waves ask
// for, so the items are dealt to R.n_heads heads (item i to head i % n_heads, its pulls in order, each head on
// a 128-byte line of its own): a wave starts on head blockIdx % n_heads -- workgroups go to the XCDs round
// robin -- and moves to the next head when one is exhausted, after a plain look at it.  An
// item marches one tile of the virtual frame with march_slot's supersampled code -- ray, march, samples,
// resolve and stores are march_tile_ss_kernel's, so a refined pixel holds bh_render_ss's bytes -- and reads or
// writes no order state (A.order, A.tile_cost and A.order_tot are null).  An entry or a virtual tile out of
// range touches no memory.
template <uint32_t FMT, uint32_t SF>
__global__ void __launch_bounds__(64 * WG_WAVES) march_refine_kernel(MarchArgs A, RefineArgs R) {
    __shared__ float lut[lds_tables<FMT>()];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lk = A.ss_log2;
    const uint32_t n_front = __builtin_amdgcn_readfirstlane(
        min(__hip_atomic_load(R.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), R.capacity));
    const uint32_t n_back = __builtin_amdgcn_readfirstlane(
        min(__hip_atomic_load(R.ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), R.capacity - n_front));
    const uint32_t total = (n_front + n_back) << (2u * lk);  // <= 0xFFFF0000 (bh_host.cpp)
    if (total == 0u) return;  // nothing refined (the same for every wave of the launch): no table, no pull
    load_srgb_tables<FMT, 64u * WG_WAVES>(A, lut);
    __syncthreads();
    const uint32_t nh = R.n_heads ? R.n_heads : 1u;
    uint32_t q = (blockIdx.x * WG_WAVES + (threadIdx.x >> 6)) % nh, tried = 0u;
    while (tried < nh) {  // wave-uniform throughout
        uint32_t* head = R.ctr + REFINE_HEAD0 + REFINE_HEAD_STRIDE * q;
        // pull n of head q is item n * nh + q; a head seen exhausted is not pulled from again
        uint32_t n = 0xFFFFFFFFu;
        if (tried == 0u || (uint64_t)__builtin_amdgcn_readfirstlane(__hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) * nh + q < total) {
            if (lane == 0u) n = __hip_atomic_fetch_add(head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            n = __builtin_amdgcn_readfirstlane(n);
        }
        const uint64_t item64 = (uint64_t)n * nh + q;
        if (item64 >= total) {
            q = q + 1u == nh ? 0u : q + 1u;
            ++tried;
            continue;
        }
        const uint32_t item = (uint32_t)item64;
        const uint32_t* e = R.list + (size_t)refine::ENTRY_WORDS * refine::entry_slot(refine::item_entry(item, lk), n_front, R.capacity);
        const uint32_t fi = __builtin_amdgcn_readfirstlane(e[0]), tile = __builtin_amdgcn_readfirstlane(e[1]);
        uint32_t vtx, vty;
        if (fi >= A.n_frames ||
            !refine::item_tile(tile, refine::item_sub(item, lk), lk, R.tiles_x, R.tiles_y, A.tiles_x, A.tiles_y, &vtx, &vty))
            continue;
        march_slot<FMT, SF, F_SS | F_ITEM>(A, fi, lut, lane, vtx, vty);
        __builtin_amdgcn_s_setprio(0);  // a tail wave raised it (march_ray); the next item starts as any wave does
    }
}

// Host side: launch the tile schedule, one wave per dispatch slot; `kernel` is march_tile_kernel, its
// supersampled form (a.ss_log2 in 1..3, the geometry fields the virtual frame's) or its lens form (a.lens set,
// out_col the lens).  (A persistent form -- resident
// waves claiming slots in order from one device-scope counter -- measured 2.5x slower: a returning
// atomic on one word is serialised across the 8 XCDs at ~85 M claims/s)
// The ray-map forms take the same grid; `maps`: their direction map, then their origin map or their hit map and their
// arrival map, the kernel's arguments after the first.
template <class K, class... Maps>
inline void launch_tile_schedule(K kernel, const MarchArgs& a, hipStream_t s, Maps... maps) {
    const uint32_t waves = a.n_tiles * a.n_frames;
    const uint32_t blocks = (waves + (WG_WAVES - 1u)) / WG_WAVES;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64u * WG_WAVES), 0, s, a, maps...);
}
// ... its shutter form: one workgroup of 2^ln waves per (output frame, tile); a.n_frames counts cameras.  KERNEL is
// march_tile_shutter_kernel<FMT, SF> or, with the map (its second argument), march_tile_shutter_rays_kernel<FMT, SF>:
// a template argument, so that each kernel has its own `raised`.
template <uint32_t FMT, auto KERNEL, class... Map>
inline void launch_shutter_schedule(const MarchArgs& a, uint32_t ln, hipStream_t s, Map... map) {
    const uint32_t blocks = a.n_tiles * (a.n_frames >> ln), lds = shutter_lds_bytes<FMT>(ln);
    if (lds > 64u * 1024u) {  // above the default limit of a launch's dynamic LDS: once per kernel
        static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                                              hipFuncAttributeMaxDynamicSharedMemorySize,
                                                              (int)shutter_lds_bytes<FMT>(shutter::MAX_LOG2));
        (void)raised;
    }
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(64u << ln), lds, s, a, map..., ln);
}
// ... and the adaptive render's work-list march: `waves` resident waves that pull (march_refine_kernel)
template <uint32_t FMT, uint32_t SF>
inline void launch_refine_schedule(const MarchArgs& a, const RefineArgs& r, uint32_t waves, hipStream_t s) {
    const uint32_t blocks = (waves + (WG_WAVES - 1u)) / WG_WAVES;
    hipLaunchKernelGGL((march_refine_kernel<FMT, SF>), dim3(blocks), dim3(64u * WG_WAVES), 0, s, a, r);
}

}  // namespace BH_NS
}  // namespace bh
