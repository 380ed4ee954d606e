// Exact (parity) instantiation of the march kernel.  Built with -ffp-contract=off and the default
// correctly-rounded f32 division/sqrt: same op sequence as oracle/bh_oracle.c (bit-exact parity).
//
// Two builds of this file (same source, same arithmetic, different instruction schedules; build.py):
//   bh_march_exact.hip      namespace exact      no machine scheduling: the step in source order, the
//                                                faster issue stream for throughput-bound frames;
//   bh_march_exact_lat.hip  namespace exact_lat  LLVM's machine schedulers: interleaved chains, the
//                                                shorter latency per step of a lone tail wave.
// bh_render picks one per frame (bh_host.cpp, march_variant).
// A third build holds the adaptive render's work-list march alone (bh_march_refine_lat.hip).
#define BH_FAST 0
#ifndef BH_NS
#define BH_NS exact
#define BH_EXACT_LAUNCH bh_launch_march_exact
#define BH_EXACT_BLOCKS bh_march_blocks_per_cu_exact
#define BH_EXACT_SHUTTER bh_launch_shutter_exact
#define BH_EXACT_REFINE bh_launch_refine_exact
#define BH_EXACT_AUX 1
#endif
#include "bh_march.hpp"

// The launchers: bh_march.hpp's, with the no-surfaces fold (FOLD_NONE) that the exact builds hold kernels for.
#ifndef BH_REFINE_ONLY
extern "C" __attribute__((visibility("hidden"))) int BH_EXACT_LAUNCH(const bh::MarchArgs& a, uint32_t schedule,
                                                                     uint32_t* counters, uint32_t grid, hipStream_t s) {
    return bh::BH_NS::launch_march<true>(a, schedule, counters, grid, s);
}
// Resident 256-thread blocks per CU of the persistent kernel (sizes its grid: every block resident).
extern "C" __attribute__((visibility("hidden"))) int BH_EXACT_BLOCKS(void) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bh::BH_NS::march_persistent_kernel<BH_OUT_BGRA8_SRGB>, 256, 0) != hipSuccess) return 1;
    return n > 0 ? n : 1;
}
// The shutter render's march (bh_render_shutter): 2^ln cameras per output frame.
extern "C" __attribute__((visibility("hidden"))) int BH_EXACT_SHUTTER(const bh::MarchArgs& a, uint32_t ln, hipStream_t s) {
    return bh::BH_NS::launch_shutter<true>(a, ln, s);
}
#endif  // BH_REFINE_ONLY

#ifdef BH_EXACT_REFINE
extern "C" __attribute__((visibility("hidden"))) int BH_EXACT_REFINE(const bh::MarchArgs& a, const bh::RefineArgs& r,
                                                                     uint32_t waves, hipStream_t s) {
    return bh::BH_NS::launch_refine<true>(a, r, waves, s);
}
#endif  // BH_EXACT_REFINE

#if defined(BH_DIAG_SLOW) && defined(BH_EXACT_AUX)
// diagnostics build only: read and reset the fallback counters
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
