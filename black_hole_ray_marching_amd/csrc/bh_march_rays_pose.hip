// The posed ray-map march (bh_render_frames_rays, bh_render_frames_shutter_rays, bh_render_lens_rays_posed;
// bh_march_tile.hpp: march_tile_rays_pose_kernel, march_tile_rays_pose_lens_kernel, march_tile_shutter_rays_kernel) as
// translation units of their own, as bh_march_rays.hip is: the exact builds' arithmetic and flags, and none of the
// other units' kernels -- 30 kernels that compile beside them.
//
// Two builds of this file (the rows of build.py):
//   bh_march_rays_pose      namespace exact_rays_pose      no machine scheduling: the throughput-bound build;
//   bh_march_rays_pose_lat  namespace exact_rays_pose_lat  -DBH_LAT=1: the machine schedulers and the packed tail step.
// The entry points pick one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifdef BH_LAT
#define BH_NS exact_rays_pose_lat
#else
#define BH_NS exact_rays_pose
#endif
#include "bh_march.hpp"

BH_MARCH_UNIT(launch_rays_pose, true)
