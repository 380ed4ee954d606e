// The lens march with a hit map (bh_render_lens_hits, bh_render_lens_rays_posed_hits; bh_march_tile.hpp:
// march_tile_lens_hits_kernel, march_tile_rays_pose_lens_hits_kernel) as translation units of their own, as
// bh_march_rays_pose.hip is: the exact builds' arithmetic and flags, and none of the other units' kernels -- 6 kernels
// that compile beside them.  And the same march with an arrival map beside the hit map (bh_march_lens_arrivals,
// bh_march_lens_rays_posed_arrivals; march_tile_lens_arrivals_kernel, march_tile_rays_pose_lens_arrivals_kernel): 6 more
// kernels of their own beside the first 6, which keep their machine code (a kernel is compiled on its own; the
// function-by-function comparison: profiles/r29/beam), behind a launcher of their own -- a second family in the
// units the table of units already names.
//
// Two builds of this file (the rows of build.py):
//   bh_march_hits      namespace exact_hits      no machine scheduling: the throughput-bound build;
//   bh_march_hits_lat  namespace exact_hits_lat  -DBH_LAT=1: the machine schedulers and the packed tail step.
// The entry points pick one per launch by bh_render's rule (bh_host.cpp, march_variant_issue_order).
#define BH_FAST 0
#ifdef BH_LAT
#define BH_NS exact_hits_lat
#define BH_ARR_UNIT exact_arr_lat
#else
#define BH_NS exact_hits
#define BH_ARR_UNIT exact_arr
#endif
#include "bh_march.hpp"

BH_MARCH_UNIT(launch_lens_hits, true)
BH_MARCH_UNIT_AS(BH_ARR_UNIT, launch_lens_arrivals, true)
