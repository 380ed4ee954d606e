// The adaptive render's work-list march (bh_render_adaptive; bh_march_tile.hpp, march_refine_kernel) in the
// scheduled build's arithmetic and schedule (bh_march_exact_lat.hip), as a translation unit of its own: the
// kernel is a loop of march_slot calls, and machine LICM hoists the march's loop invariants out of that loop and
// keeps them live across it -- 129 VGPRs and 29 spilled SGPRs, 3 waves per SIMD, against 78 VGPRs and 6 waves
// without it (build.py; the scheduled build's other kernels keep LICM: DESIGN.md §5 item 8, §7f).
#define BH_NS exact_lat_refine
#define BH_TAIL_PACKED 1
#define BH_REFINE_ONLY 1
#define BH_EXACT_REFINE bh_launch_refine_exact_lat
#include "bh_march_exact.hip"
