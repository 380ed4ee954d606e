// bh_march.hpp — the geodesic ray-march kernel for gfx950 (CDNA4), one lane per pixel.
//
// Included by the march sources, each after defining BH_FAST and BH_NS.  A source is a family of kernels; a unit
// is a row of build.py's UNITS over it (name, source, flags, defines), and a source has one row per build:
//   bh_march_exact.hip      the plain family (tile / ss / lens / shutter kernels, the A/B schedules, the work list)
//   bh_march_rays.hip       the ray-map kernels alone
//   bh_march_rays_pose.hip  the posed ray-map kernels, their shutter form
//   bh_march_rays_org.hip   those with an origin map
//   bh_march_hits.hip       the lens kernels with a hit map, and those with an arrival map beside it
//       BH_FAST 0; built -ffp-contract=off, correctly-rounded f32 div/sqrt: same op sequence as the normative
//       arithmetic of oracle/bh_oracle.c -> bit-exact parity.  Two rows each: the issue-order build, and with
//       -DBH_LAT=1 the scheduled (latency) build -- a namespace of its own, the packed tail step (BH_TAIL_PACKED,
//       set below).  bh_march_exact.hip has a third, -DBH_LAT=1 -DBH_REFINE_ONLY=1: the work-list march alone.
//   bh_march_fast.hip       the plain family again (one row)
//       BH_FAST 1; built -ffp-contract=fast, hardware rcp/rsq/sqrt: algebraically identical reformulation for
//       throughput -> tolerance parity.
// A unit exports one hidden launcher, named after its namespace (BH_MARCH_UNIT at the end of this file); the host
// finds it in its table of [family][build] (bh_host.cpp, MARCH_UNITS).
//
// Semantics follow src/black_hole_maybe.wgsl (reference): fs_main :360-370, get_col :259-345,
// get_delta_photon_rk4 :134-151, rd_derivative :125-127, sdf* :91-123.  Layout: each wave64 owns
// one 8x8 pixel tile (SIMD efficiency 0.72 vs 0.67 for 64x1 rows); RK state stays in
// VGPRs; the 256-entry sRGB decode table is staged in LDS once per workgroup; the 32 MiB RGBA8 sky
// is read with 4 dword gathers per escaped ray (L2/MALL-resident).
//
// This file holds the dispatch: with_scene_fold, with_tile_form (the tile schedule's choice of form, once) and one
// launch_* per hidden entry point.  The kernels are in its parts, each of which names what it needs:
//   bh_march_ops.hpp      v3, the constants, the math modes' op sets (FOps, XOps)
//   bh_march_step.hpp     one iteration: the ray state, the root-free tests, step_bf, the packed tail step
//   bh_march_shade.hpp    sky sample, shading, the output encoders, write_pixel
//   bh_march_ray.hpp      one ray to its end: the ping-pong loop, the tail's cycle fast-forward
//   bh_march_resolve.hpp  the supersampled render's resolve in the wave, the shutter render's in the workgroup
//   bh_march_tile.hpp     the tile schedule: the form mask, march_slot, the tile-schedule wave and the shutter
//                         workgroup, their kernels (tile / ss / lens / ray map / shutter / work list) and launchers
//   bh_march_alt.hpp      the persistent and pair schedules (A/B options)
#pragma once
#include <hip/hip_runtime.h>

#include "bh_common.hpp"

#ifndef BH_FAST
#error "define BH_FAST to 0 or 1"
#endif
#if defined(BH_LAT) && !defined(BH_TAIL_PACKED)
#define BH_TAIL_PACKED 1  // the scheduled builds' tail loop runs the packed-FP32 step (bh_march_step.hpp, step_tail)
#endif
// (rd_derivative's reciprocal from the root's own v_rsq, crm::rcp_from_rsq, instead of a v_rcp of Q: four
// fewer transcendentals per RK step, but NOT exact -- 60 (numerator, Q) pairs, at Q significands next to
// 2 (e.g. n = 1, Q = 0x2cffffff), round the other way (selftest op 13) -- so the march keeps rcp_refined.)

#include "bh_march_alt.hpp"
#include "bh_march_tile.hpp"

namespace bh {
namespace BH_NS {

// ---- one launcher per family, for every build of its kernels -------------------------------------------------
// A launcher is a template, so a unit holds the kernels of the launchers it calls and no others; hidden, like
// the entry points that call them.  Each takes the launch's record (bh_common.hpp, MarchLaunch) and reads its
// family's fields of it.
// f(SF) with the launch's scene flags as a compile-time constant where the build folds them: the reference's
// scene always (Const and with_format: bh_common.hpp); no surfaces (BASELINE config 1: the sdf folds to +inf) with FOLD_NONE, which the exact builds
// set and the fast build does not; otherwise SF_DYN, the kernels that read the flags.
template <bool FOLD_NONE, class F>
__attribute__((visibility("hidden"))) inline void with_scene_fold(uint32_t flags, F&& f) {
    if (flags == BH_SCENE_DEFAULT) return f(Const<BH_SCENE_DEFAULT>{});
    if constexpr (FOLD_NONE)
        if (flags == 0u) return f(Const<0u>{});
    f(Const<SF_DYN>{});
}
// The tile schedule's choice of form, written once for its four families of kernels (plain, ray map, posed ray map,
// with an origin map): a lens launch (a.lens set: exact builds) by the scene-flag fold alone, whatever the format word
// says -- lens(sf); any other by format and fold, supersampled when a.ss_log2 != 0 (bh_render_ss, ss > 1) --
// tile(fmt, sf, ss), ss a Const<0 or 1>.  The two callables launch their family's kernel of that form.  Returns a
// hipError_t.
template <bool FOLD_NONE, class L, class T>
__attribute__((visibility("hidden"))) inline int with_tile_form(const MarchArgs& a, L&& lens, T&& tile) {
#if !BH_FAST
    if (a.lens != 0u) {
        with_scene_fold<FOLD_NONE>(a.scene_flags, lens);
        return (int)hipGetLastError();
    }
#endif
    return with_format(a.format, [&](auto fmt) {
        with_scene_fold<FOLD_NONE>(a.scene_flags, [&](auto sf) {
            if (a.ss_log2 != 0u) tile(fmt, sf, Const<1u>{});
            else tile(fmt, sf, Const<0u>{});
        });
        return (int)hipGetLastError();
    });
}
// The march over every tile under m.schedule (a bh_schedule without its flags); m.counters, m.grid: the persistent
// schedule's.  Returns a hipError_t.
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_march(const MarchArgs& a, const MarchLaunch& m, hipStream_t s) {
    if (m.schedule == BH_SCHED_TILE)
        return with_tile_form<FOLD_NONE>(
            a, [&](auto sf) { launch_tile_schedule(march_tile_lens_kernel<decltype(sf)::value>, a, s); },
            [&](auto fmt, auto sf, auto ss) {
                constexpr uint32_t FMT = decltype(fmt)::value, SF = decltype(sf)::value;
                if constexpr (decltype(ss)::value != 0u) launch_tile_schedule(march_tile_ss_kernel<FMT, SF>, a, s);
                else launch_tile_schedule(march_tile_kernel<FMT, SF>, a, s);
            });
#if !BH_FAST
    if (a.lens != 0u) return (int)hipErrorInvalidValue;  // bh_render_lens: the tile schedule only
#endif
    return with_format(a.format, [&](auto fmt) {
        constexpr uint32_t FMT = decltype(fmt)::value;
        if (m.schedule == BH_SCHED_PAIR) {
            const uint32_t pairs = (a.n_tiles + 1u) / 2u;
            hipLaunchKernelGGL(march_pair_kernel<FMT>, dim3((pairs + 3u) / 4u), dim3(256), 0, s, a);
        } else {
            hipError_t e = hipMemsetAsync(m.counters, 0, NQ * CTR_STRIDE * sizeof(uint32_t), s);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL(march_persistent_kernel<FMT>, dim3(m.grid), dim3(256), 0, s, a, m.counters);
        }
        return (int)hipGetLastError();
    });
}
#if !BH_FAST
// The ray-map march (bh_render_rays, bh_render_lens_rays; tile schedule, one frame).
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_rays(const MarchArgs& a, const MarchLaunch& m, hipStream_t s) {
    if (!m.dirs || a.n_frames != 1u) return (int)hipErrorInvalidValue;
    return with_tile_form<FOLD_NONE>(
        a, [&](auto sf) { launch_tile_schedule(march_tile_rays_lens_kernel<decltype(sf)::value>, a, s, m.dirs); },
        [&](auto fmt, auto sf, auto ss) {
            constexpr uint32_t FMT = decltype(fmt)::value, SF = decltype(sf)::value;
            launch_tile_schedule(march_tile_rays_kernel<FMT, SF, decltype(ss)::value != 0u>, a, s, m.dirs);
        });
}
// The posed ray-map march (bh_render_frames_rays, bh_render_frames_shutter_rays, bh_render_lens_rays_posed; tile
// schedule): any number of frames over one camera-space map; ln != 0: the shutter form, 2^ln cameras per output frame.
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_rays_pose(const MarchArgs& a, const MarchLaunch& m, hipStream_t s) {
    const uint32_t ln = m.shutter_log2;
    if (!m.dirs || a.n_frames == 0u) return (int)hipErrorInvalidValue;
    if (a.lens != 0u ? (ln != 0u || a.n_frames != 1u) : (ln > shutter::MAX_LOG2 || (a.n_frames & ((1u << ln) - 1u)) != 0u))
        return (int)hipErrorInvalidValue;
    return with_tile_form<FOLD_NONE>(
        a, [&](auto sf) { launch_tile_schedule(march_tile_rays_pose_lens_kernel<decltype(sf)::value>, a, s, m.dirs); },
        [&](auto fmt, auto sf, auto ss) {
            constexpr uint32_t FMT = decltype(fmt)::value, SF = decltype(sf)::value;
            if (ln != 0u) launch_shutter_schedule<FMT, march_tile_shutter_rays_kernel<FMT, SF>>(a, ln, s, m.dirs);
            else launch_tile_schedule(march_tile_rays_pose_kernel<FMT, SF, decltype(ss)::value != 0u>, a, s, m.dirs);
        });
}
// The posed ray-map march with an origin map (bh_render_frames_rays_origins, bh_render_lens_rays_origins; tile
// schedule, no shutter form): any number of frames over one pair of camera-space maps.
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_rays_org(const MarchArgs& a, const MarchLaunch& m, hipStream_t s) {
    if (!m.dirs || !m.orgs || a.n_frames == 0u || (a.lens != 0u && a.n_frames != 1u)) return (int)hipErrorInvalidValue;
    return with_tile_form<FOLD_NONE>(
        a, [&](auto sf) { launch_tile_schedule(march_tile_rays_org_lens_kernel<decltype(sf)::value>, a, s, m.dirs, m.orgs); },
        [&](auto fmt, auto sf, auto ss) {
            constexpr uint32_t FMT = decltype(fmt)::value, SF = decltype(sf)::value;
            launch_tile_schedule(march_tile_rays_org_kernel<FMT, SF, decltype(ss)::value != 0u>, a, s, m.dirs, m.orgs);
        });
}
// The lens march with a hit map (bh_render_lens_hits: dirs null, the pinhole form; bh_render_lens_rays_posed_hits: the
// posed ray-map form; tile schedule, one frame): one kernel per form and scene-flag fold.
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_lens_hits(const MarchArgs& a, const MarchLaunch& m, hipStream_t s) {
    if (!m.hits || a.lens == 0u || a.n_frames != 1u) return (int)hipErrorInvalidValue;
    with_scene_fold<FOLD_NONE>(a.scene_flags, [&](auto sf) {
        constexpr uint32_t SF = decltype(sf)::value;
        if (m.dirs) launch_tile_schedule(march_tile_rays_pose_lens_hits_kernel<SF>, a, s, m.dirs, m.hits);
        else launch_tile_schedule(march_tile_lens_hits_kernel<SF>, a, s, m.hits);
    });
    return (int)hipGetLastError();
}
// The same with an arrival map beside the hit map (bh_march_lens_arrivals, bh_march_lens_rays_posed_arrivals).
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_lens_arrivals(const MarchArgs& a, const MarchLaunch& m, hipStream_t s) {
    if (!m.hits || !m.arrivals || a.lens == 0u || a.n_frames != 1u) return (int)hipErrorInvalidValue;
    with_scene_fold<FOLD_NONE>(a.scene_flags, [&](auto sf) {
        constexpr uint32_t SF = decltype(sf)::value;
        if (m.dirs) launch_tile_schedule(march_tile_rays_pose_lens_arrivals_kernel<SF>, a, s, m.dirs, m.hits, m.arrivals);
        else launch_tile_schedule(march_tile_lens_arrivals_kernel<SF>, a, s, m.hits, m.arrivals);
    });
    return (int)hipGetLastError();
}
#endif
// The shutter render's march (bh_render_shutter, n = 2^ln cameras per output frame; tile schedule): the same folds.
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_shutter(const MarchArgs& a, const MarchLaunch& m, hipStream_t s) {
    const uint32_t ln = m.shutter_log2;
    if (ln == 0u || ln > shutter::MAX_LOG2 || (a.n_frames & ((1u << ln) - 1u)) != 0u) return (int)hipErrorInvalidValue;
    return with_format(a.format, [&](auto fmt) {
        with_scene_fold<FOLD_NONE>(a.scene_flags, [&](auto sf) {
            constexpr uint32_t FMT = decltype(fmt)::value;
            launch_shutter_schedule<FMT, march_tile_shutter_kernel<FMT, decltype(sf)::value>>(a, ln, s);
        });
        return (int)hipGetLastError();
    });
}
// The plain family's launcher: the shutter march when m.shutter_log2 != 0, else the march under m.schedule.
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_plain(const MarchArgs& a, const MarchLaunch& m, hipStream_t s) {
    return m.shutter_log2 != 0u ? launch_shutter<FOLD_NONE>(a, m, s) : launch_march<FOLD_NONE>(a, m, s);
}
// The adaptive render's work-list march (bh_render_adaptive): the supersampled kernels' folds.
template <bool FOLD_NONE>
__attribute__((visibility("hidden"))) inline int launch_refine(const MarchArgs& a, const RefineArgs& r, uint32_t waves, hipStream_t s) {
    return with_format(a.format, [&](auto fmt) {
        with_scene_fold<FOLD_NONE>(a.scene_flags, [&](auto sf) {
            launch_refine_schedule<decltype(fmt)::value, decltype(sf)::value>(a, r, waves, s);
        });
        return (int)hipGetLastError();
    });
}

}  // namespace BH_NS
}  // namespace bh

// ---- a unit's launcher ---------------------------------------------------------------------------------------
// The one symbol a tile-march unit exports to the host units: bh_launch_unit_<namespace>, of the one type
// int (const bh::MarchArgs&, const bh::MarchLaunch&, hipStream_t), forwarding to the family's template above.  A
// unit that holds the work-list march exports bh_launch_refine_unit_<namespace> the same way.  bh_host.hpp declares
// them from its list of namespaces.
#define BH_PASTE_(a, b) a##b
#define BH_PASTE(a, b) BH_PASTE_(a, b)
#define BH_MARCH_UNIT(family, FOLD_NONE) BH_MARCH_UNIT_AS(BH_NS, family, FOLD_NONE)
// A unit that holds a second family exports that family's launcher under a name of its own (bh_march_hits.hip).
#define BH_MARCH_UNIT_AS(name, family, FOLD_NONE)                                                                     \
    extern "C" __attribute__((visibility("hidden"))) int BH_PASTE(bh_launch_unit_, name)(                             \
        const bh::MarchArgs& a, const bh::MarchLaunch& m, hipStream_t s) {                                            \
        return bh::BH_NS::family<FOLD_NONE>(a, m, s);                                                                 \
    }
#define BH_REFINE_UNIT(FOLD_NONE)                                                                                     \
    extern "C" __attribute__((visibility("hidden"))) int BH_PASTE(bh_launch_refine_unit_, BH_NS)(                     \
        const bh::MarchArgs& a, const bh::RefineArgs& r, uint32_t waves, hipStream_t s) {                             \
        return bh::BH_NS::launch_refine<FOLD_NONE>(a, r, waves, s);                                                   \
    }
