// frp_ipm_lds_q4.hip -- third translation unit of the LDS-resident solver: the FOUR-problems-per-CU variants.  Same sources as
// frp_ipm_lds.hip on the Q4 record layout (241 doubles per stage instead of 309: packed P_k in an L2-resident workspace in global
// memory, T' and p in the slots of the consumed Hessian) and on workgroups of three wavefronts (Riccati; model + a bound round;
// faces + the other bound rounds): 4 x 40 KB of LDS and 12 waves at 168 VGPRs per CU.  Contributes frp::launch_ipm_lds_q4.
#define FRP_LDS_Q4_TU
// The factorisation sweep inlined: as a function of its own it saves and restores 38 callee-saved registers per call whether or not the
// caller holds anything in them -- 0.858 -> 0.853 ms per 4096-problem launch; inlining the vector sweeps as well loses that again
// (profiles/r05_q4_flags.txt).
#define FRP_INLINE_FACTOR
#include "frp_ipm_lds.hip"
