// Fast (production) instantiation of the march kernel.  Built with -ffp-contract=fast and
// -fno-hip-fp32-correctly-rounded-divide-sqrt: hardware rcp/rsq/sqrt, FMA contraction.
#define BH_FAST 1
#define BH_NS fast
#include "bh_march.hpp"

// The launchers: bh_march.hpp's, without the no-surfaces fold (this build holds no kernels for it).
extern "C" __attribute__((visibility("hidden"))) int bh_launch_march_fast(const bh::MarchArgs& a, uint32_t schedule,
                                                                        uint32_t* counters, uint32_t grid, hipStream_t s) {
    return bh::fast::launch_march<false>(a, schedule, counters, grid, s);
}
extern "C" __attribute__((visibility("hidden"))) int bh_launch_refine_fast(const bh::MarchArgs& a, const bh::RefineArgs& r,
                                                                         uint32_t waves, hipStream_t s) {
    return bh::fast::launch_refine<false>(a, r, waves, s);
}
extern "C" __attribute__((visibility("hidden"))) int bh_launch_shutter_fast(const bh::MarchArgs& a, uint32_t ln, hipStream_t s) {
    return bh::fast::launch_shutter<false>(a, ln, s);
}
// Resident 256-thread blocks per CU of the persistent kernel (sizes its grid: every block resident).
extern "C" __attribute__((visibility("hidden"))) int bh_march_blocks_per_cu_fast(void) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bh::fast::march_persistent_kernel<BH_OUT_BGRA8_SRGB>, 256, 0) != hipSuccess) return 1;
    return n > 0 ? n : 1;
}
