// The posed ray-map march with an origin map (bh_render_frames_rays_origins, bh_render_lens_rays_origins;
// bh_march_tile.hpp: march_tile_rays_org_kernel, march_tile_rays_org_lens_kernel) as translation units of their own, as
// bh_march_rays_pose.hip is: the exact builds' arithmetic and flags, and none of the other units' kernels -- 21 kernels
// that compile beside them.
//
// Two builds of this file (the rows of build.py):
//   bh_march_rays_org      namespace exact_rays_org      no machine scheduling: the throughput-bound build;
//   bh_march_rays_org_lat  namespace exact_rays_org_lat  -DBH_LAT=1: the machine schedulers and the packed tail step.
// The entry points pick one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifdef BH_LAT
#define BH_NS exact_rays_org_lat
#else
#define BH_NS exact_rays_org
#endif
#include "bh_march.hpp"

BH_MARCH_UNIT(launch_rays_org, true)
