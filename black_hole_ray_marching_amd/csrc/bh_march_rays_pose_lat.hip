// The posed ray-map march built WITH machine scheduling (see bh_march_rays_pose.hip, bh_march_exact_lat.hip): the
// variant for latency-bound launches.
#define BH_NS exact_rays_pose_lat
#define BH_TAIL_PACKED 1
#define BH_RAYS_POSE_LAUNCH bh_launch_rays_pose_exact_lat
#include "bh_march_rays_pose.hip"
