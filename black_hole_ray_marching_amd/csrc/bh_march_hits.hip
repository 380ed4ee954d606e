// The lens march with a hit map (bh_render_lens_hits, bh_render_lens_rays_posed_hits; bh_march_tile.hpp:
// march_tile_lens_hits_kernel, march_tile_rays_pose_lens_hits_kernel) as translation units of their own, as
// bh_march_rays_pose.hip is: the exact builds' arithmetic and flags, and none of the other units' kernels -- 6 kernels
// that compile beside them.
//
// Two builds of this file (the rows of build.py):
//   bh_march_hits      namespace exact_hits      no machine scheduling: the throughput-bound build;
//   bh_march_hits_lat  namespace exact_hits_lat  -DBH_LAT=1: the machine schedulers and the packed tail step.
// The entry points pick one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifdef BH_LAT
#define BH_NS exact_hits_lat
#else
#define BH_NS exact_hits
#endif
#include "bh_march.hpp"

BH_MARCH_UNIT(launch_lens_hits, true)
