// The lens march with a hit map built WITH machine scheduling (see bh_march_hits.hip, bh_march_exact_lat.hip): the
// variant for latency-bound launches.
#define BH_NS exact_hits_lat
#define BH_TAIL_PACKED 1
#define BH_HITS_LAUNCH bh_launch_lens_hits_exact_lat
#include "bh_march_hits.hip"
