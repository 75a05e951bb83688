// ccsd_lgw.hip -- product translation unit: k_lg_fin_w, the final MLP of ScoreNetworkA on the tiled graph-network route for 57 to 64
// channels (the chain shape of CCSD_CHAIN_AFIN_LG; PlanBuilder::afin_lg).  The body is k_lg_fin's (ccsd_lg_fin.inc); a unit of its own, so
// that the code of ccsd_lg.hip's kernels does not move with it.
#include "ccsd_dev.h"
#include "ccsd_k_lg.h"
#include "ccsd_lg_fin_w.inc"
