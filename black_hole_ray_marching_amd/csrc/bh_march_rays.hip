// The ray-map march (bh_render_rays, bh_render_lens_rays; bh_march_tile.hpp, march_tile_rays_kernel and
// march_tile_rays_lens_kernel) as translation units of their own: the exact builds' arithmetic and flags, and none
// of their kernels -- those units' code objects stay what they were, and these 21 kernels compile beside them
// instead of after them.
//
// Two builds of this file (the rows of build.py):
//   bh_march_rays      namespace exact_rays      no machine scheduling: the throughput-bound build;
//   bh_march_rays_lat  namespace exact_rays_lat  -DBH_LAT=1: the machine schedulers and the packed tail step.
// bh_render_rays picks one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifdef BH_LAT
#define BH_NS exact_rays_lat
#else
#define BH_NS exact_rays
#endif
#include "bh_march.hpp"

BH_MARCH_UNIT(launch_rays, true)
