// The lens march with a hit map (bh_render_lens_hits, bh_render_lens_rays_posed_hits; bh_march_tile.hpp:
// march_tile_lens_hits_kernel, march_tile_rays_pose_lens_hits_kernel) as translation units of their own, as
// bh_march_rays_pose.hip is: the exact builds' arithmetic and flags, and none of the other units' kernels -- 6 kernels
// that compile beside them.
//
// Two builds of this file (build.py):
//   bh_march_hits.hip      namespace exact_hits      no machine scheduling: the throughput-bound build;
//   bh_march_hits_lat.hip  namespace exact_hits_lat  LLVM's machine schedulers and the packed tail step.
// The entry points pick one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifndef BH_NS
#define BH_NS exact_hits
#define BH_HITS_LAUNCH bh_launch_lens_hits_exact
#endif
#include "bh_march.hpp"

extern "C" __attribute__((visibility("hidden"))) int BH_HITS_LAUNCH(const bh::MarchArgs& a, const float* dirs, float* hits,
                                                                    hipStream_t s) {
    return bh::BH_NS::launch_lens_hits<true>(a, dirs, hits, s);
}
