// ccsd_lg_fin_w.inc -- k_lg_fin_w: k_lg_fin's body (ccsd_lg_fin.inc) with the one chain shape of CCSD_CHAIN_AFIN_LG.  Included by the
// product unit ccsd_lgw.hip and, for the host emulation, by ccsd_k_lg.h.
#define LG_FIN_KERNEL k_lg_fin_w
#define LG_FIN_CHAIN mlp_chain_tile<4, 8, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);
#include "ccsd_lg_fin.inc"
#undef LG_FIN_KERNEL
#undef LG_FIN_CHAIN
