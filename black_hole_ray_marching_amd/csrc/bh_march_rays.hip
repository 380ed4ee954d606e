// The ray-map march (bh_render_rays, bh_render_lens_rays; bh_march_tile.hpp, march_tile_rays_kernel and
// march_tile_rays_lens_kernel) as translation units of their own: the exact builds' arithmetic and flags, and none
// of their kernels -- those units' code objects stay what they were, and these 21 kernels compile beside them
// instead of after them.
//
// Two builds of this file, as of bh_march_exact.hip (build.py):
//   bh_march_rays.hip      namespace exact_rays      no machine scheduling: the throughput-bound frames' build;
//   bh_march_rays_lat.hip  namespace exact_rays_lat  LLVM's machine schedulers and the packed tail step.
// bh_render_rays picks one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifndef BH_NS
#define BH_NS exact_rays
#define BH_RAYS_LAUNCH bh_launch_rays_exact
#endif
#include "bh_march.hpp"

extern "C" __attribute__((visibility("hidden"))) int BH_RAYS_LAUNCH(const bh::MarchArgs& a, const float* dirs, hipStream_t s) {
    return bh::BH_NS::launch_rays<true>(a, dirs, s);
}
