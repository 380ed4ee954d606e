// The posed ray-map march with an origin map (bh_render_frames_rays_origins, bh_render_lens_rays_origins;
// bh_march_tile.hpp: march_tile_rays_org_kernel, march_tile_rays_org_lens_kernel) as translation units of their own, as
// bh_march_rays_pose.hip is: the exact builds' arithmetic and flags, and none of the other units' kernels -- 21 kernels
// that compile beside them.
//
// Two builds of this file (build.py):
//   bh_march_rays_org.hip      namespace exact_rays_org      no machine scheduling: the throughput-bound build;
//   bh_march_rays_org_lat.hip  namespace exact_rays_org_lat  LLVM's machine schedulers and the packed tail step.
// The entry points pick one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifndef BH_NS
#define BH_NS exact_rays_org
#define BH_RAYS_ORG_LAUNCH bh_launch_rays_org_exact
#endif
#include "bh_march.hpp"

extern "C" __attribute__((visibility("hidden"))) int BH_RAYS_ORG_LAUNCH(const bh::MarchArgs& a, const float* dirs,
                                                                        const float* orgs, hipStream_t s) {
    return bh::BH_NS::launch_rays_org<true>(a, dirs, orgs, s);
}
