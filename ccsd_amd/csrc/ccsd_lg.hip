// ccsd_lg.hip -- product translation unit: the tiled graph-network kernels k_lg_* (ccsd_k_lg.h); ccsd_hip.hip launches them.
#define CCSD_LG_UNIT
#include "ccsd_dev.h"
#include "ccsd_k_lg.h"
