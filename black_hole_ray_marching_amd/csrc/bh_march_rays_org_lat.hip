// The posed ray-map march with an origin map built WITH machine scheduling (see bh_march_rays_org.hip,
// bh_march_exact_lat.hip): the variant for latency-bound launches.
#define BH_NS exact_rays_org_lat
#define BH_TAIL_PACKED 1
#define BH_RAYS_ORG_LAUNCH bh_launch_rays_org_exact_lat
#include "bh_march_rays_org.hip"
