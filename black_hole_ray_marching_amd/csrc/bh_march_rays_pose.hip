// The posed ray-map march (bh_render_frames_rays, bh_render_frames_shutter_rays, bh_render_lens_rays_posed;
// bh_march_tile.hpp: march_tile_rays_pose_kernel, march_tile_rays_pose_lens_kernel, march_tile_shutter_rays_kernel) as
// translation units of their own, as bh_march_rays.hip is: the exact builds' arithmetic and flags, and none of the
// other units' kernels -- 30 kernels that compile beside them.
//
// Two builds of this file (build.py):
//   bh_march_rays_pose.hip      namespace exact_rays_pose      no machine scheduling: the throughput-bound build;
//   bh_march_rays_pose_lat.hip  namespace exact_rays_pose_lat  LLVM's machine schedulers and the packed tail step.
// The entry points pick one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifndef BH_NS
#define BH_NS exact_rays_pose
#define BH_RAYS_POSE_LAUNCH bh_launch_rays_pose_exact
#endif
#include "bh_march.hpp"

extern "C" __attribute__((visibility("hidden"))) int BH_RAYS_POSE_LAUNCH(const bh::MarchArgs& a, const float* dirs,
                                                                         uint32_t shutter_log2, hipStream_t s) {
    return bh::BH_NS::launch_rays_pose<true>(a, dirs, shutter_log2, s);
}
