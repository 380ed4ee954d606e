// Exact (parity) instantiation of the march kernel.  Built with -ffp-contract=off and the default
// correctly-rounded f32 division/sqrt: same op sequence as oracle/bh_oracle.c (bit-exact parity).
//
// Three builds of this file (same source, same arithmetic, different instruction schedules; the rows of build.py):
//   bh_march_exact       namespace exact             no machine scheduling: the step in source order, the faster
//                                                    issue stream for throughput-bound frames;
//   bh_march_exact_lat   namespace exact_lat         -DBH_LAT=1: LLVM's machine schedulers: interleaved chains, the
//                                                    shorter latency per step of a lone tail wave; its tail loop runs
//                                                    the packed-FP32 step (bh_march_step.hpp, step_tail);
//   bh_march_refine_lat  namespace exact_lat_refine  -DBH_LAT=1 -DBH_REFINE_ONLY=1: the adaptive render's work-list
//                                                    march alone (bh_march_tile.hpp, march_refine_kernel), scheduled.
// bh_render picks one of the first two per frame (bh_host.cpp, march_variant_issue_order).  The
// work-list march has a unit of its own in the scheduled build because that unit is built without machine LICM: the
// kernel is a loop of march_slot calls, and machine LICM hoists the march's loop invariants out of that loop and keeps
// them live across it -- 129 VGPRs and 29 spilled SGPRs, 3 waves per SIMD, against 78 VGPRs and 6 waves without it
// (the scheduled build's other kernels keep LICM: DESIGN.md §5 item 8, §7f).  The issue-order unit holds both.
#define BH_FAST 0
#if defined(BH_REFINE_ONLY)
#define BH_NS exact_lat_refine
#elif defined(BH_LAT)
#define BH_NS exact_lat
#else
#define BH_NS exact
#endif
#include "bh_march.hpp"

// The launchers: bh_march.hpp's, with the no-surfaces fold (FOLD_NONE) that the exact builds hold kernels for.
#ifndef BH_REFINE_ONLY
BH_MARCH_UNIT(launch_plain, true)
#endif
#if defined(BH_REFINE_ONLY) || !defined(BH_LAT)
BH_REFINE_UNIT(true)
#endif

#ifndef BH_LAT
// Resident 256-thread blocks per CU of the persistent kernel (sizes its grid: every block resident).
extern "C" __attribute__((visibility("hidden"))) int bh_march_blocks_per_cu_exact(void) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bh::BH_NS::march_persistent_kernel<BH_OUT_BGRA8_SRGB>, 256, 0) != hipSuccess) return 1;
    return n > 0 ? n : 1;
}
#endif

#if defined(BH_DIAG_SLOW) && !defined(BH_LAT)
// diagnostics build only (the first build's): read and reset the fallback counters
extern "C" int bh_diag_slow_counts(uint32_t* lane_steps, uint32_t* wave_steps) {
    uint32_t z = 0;
    if (hipMemcpyFromSymbol(lane_steps, HIP_SYMBOL(bh::BH_NS::g_diag_slow_lane_steps), 4) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(wave_steps, HIP_SYMBOL(bh::BH_NS::g_diag_slow_wave_steps), 4) != hipSuccess) return -1;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(bh::BH_NS::g_diag_slow_lane_steps), &z, 4);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(bh::BH_NS::g_diag_slow_wave_steps), &z, 4);
    return 0;
}
// and the root-free step's counters: wave-steps that skipped the SDF roots (far field included), all
// wave-steps, far-field wave-steps
extern "C" int bh_diag_far_count(uint32_t* far_wave_steps) {
    uint32_t z = 0;
    if (hipMemcpyFromSymbol(far_wave_steps, HIP_SYMBOL(bh::BH_NS::g_diag_far_wave_steps), 4) != hipSuccess) return -1;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(bh::BH_NS::g_diag_far_wave_steps), &z, 4);
    return 0;
}
extern "C" int bh_diag_skip_counts(uint32_t* skip_wave_steps, uint32_t* all_wave_steps) {
    uint32_t z = 0;
    if (hipMemcpyFromSymbol(skip_wave_steps, HIP_SYMBOL(bh::BH_NS::g_diag_skip_wave_steps), 4) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(all_wave_steps, HIP_SYMBOL(bh::BH_NS::g_diag_all_wave_steps), 4) != hipSuccess) return -1;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(bh::BH_NS::g_diag_skip_wave_steps), &z, 4);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(bh::BH_NS::g_diag_all_wave_steps), &z, 4);
    return 0;
}
#endif
