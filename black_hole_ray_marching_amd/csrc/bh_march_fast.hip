// Fast (production) instantiation of the march kernel.  Built with -ffp-contract=fast and
// -fno-hip-fp32-correctly-rounded-divide-sqrt: hardware rcp/rsq/sqrt, FMA contraction.
#define BH_FAST 1
#define BH_NS fast
#include "bh_march.hpp"

// The launchers: bh_march.hpp's, without the no-surfaces fold (this build holds no kernels for it).
BH_MARCH_UNIT(launch_plain, false)
BH_REFINE_UNIT(false)
// Resident 256-thread blocks per CU of the persistent kernel (sizes its grid: every block resident).
extern "C" __attribute__((visibility("hidden"))) int bh_march_blocks_per_cu_fast(void) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bh::fast::march_persistent_kernel<BH_OUT_BGRA8_SRGB>, 256, 0) != hipSuccess) return 1;
    return n > 0 ? n : 1;
}
