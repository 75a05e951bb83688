// ccsd_kernels.h -- hand-written gfx950 kernels for the CCSD predictor-corrector sampling path (umbrella header).
//
// Data layout in HBM (all fp32, contiguous, batch-major; same as the reference tensors):
//   x (B,N,F)   adj (B,N,N)   rank2 (B,E,K)   flags (B,N) of exact 0/1
//   H (B,E,E) = F F^T (diag zeroed)            P_l (B*E, wc_l) = hodge Q|K projections of layer l
//
// Source map
//   ccsd_dev.h       device helpers: Philox4x32-10, fast math, MFMA building blocks (block_linear, mlp_chain_tile, gcn_tile)
//   ccsd_rank2_common.h  masks, epilogue modes, ScoreNetworkF per element, wave-level tile loops (shared helpers)
//   ccsd_k_rank2.h   k_flagbits, k_gemm_h (H = F F^T), k_gemm_p / k_gemm_p0 (hodge projections), k_edgecoef,
//                    k_hf_score ((H F) + ScoreNetworkF epilogue + fused predictor update / Langevin norms): the tiled rank-2 path
//   ccsd_k_r2.h      k_r2: the fused rank-2 kernel, one complex per workgroup with its rank2 block LDS-resident (E <= 64)
//   ccsd_k_xa.h      k_xa: ScoreNetworkX + ScoreNetworkA(_CC): one workgroup per graph, everything LDS-resident
//                    (+ ccsd_attn_stack.inc: the AttentionLayer stack)
//   ccsd_k_lg.h      k_lg_*: the tiled graph-network path (graph-only plans above 64 nodes, plans without a k_xa LDS layout, one-hodge-layer
//                    ScoreNetworkA_CC among them): ScoreNetworkX + ScoreNetworkA(_CC) over the HBM workspace, each graph tiled over many
//                    workgroups (definitions compiled in ccsd_lg.hip; + ccsd_lg_fin.inc: the body of k_lg_fin and of k_lg_fin_w, which
//                    ccsd_lgw.hip compiles)
//   ccsd_k_update.h  k_normsum, k_langevin_apply, k_s4_apply, k_init_state, k_quantize, k_rank2_cells
//   ccsd_k_finish.h  k_finish_rank2, k_finish_graph: quantised outputs, cell bitmask and per-complex descriptors in one pass per tensor
//   ccsd_k_eval.h    k_cluster_hist, k_mmd_prep, k_mmd_pairs, k_mmd_final: clustering-coefficient histograms and the fp64 MMD of two
//                    sets of histograms (the evaluation of finished samples)
//   ccsd_k_orbit.h   k_orbit_counts: the 4-node graphlet orbit counts per node and per graph from the same bit-mask rows, by a closed
//                    form (what the reference's "orbit" score reads from the external orca program)
//   ccsd_k_nspdk.h   k_nspdk_features, k_nspdk_chunks, k_nspdk_dots, k_nspdk_final: the NSPDK feature vector per graph (breadth-first
//                    layers as mask operations, CPython's tuple hash in 64-bit integers, integer counting) and the linear-kernel MMD
//                    of two sets of such rows (the reference's "nspdk" score of molecule runs)
//   ccsd_k_eig.h     k_eigvalsh, k_norm_laplacian, k_hodge_laplacian: a batched symmetric eigenvalue solver (parallel Jacobi) and the
//                    two matrices whose spectra the reference scores (normalised graph Laplacian, hodge Laplacian F F^T)
//   ccsd_k_lift.h    k_lift_paths, k_lift_cycles, k_lift_dense: graphs lifted to combinatorial complexes (rank-2 cells from the paths of
//                    three nodes or from networkx's cycle basis) as ccsd_finish's cell bitmask and descriptors, and the dense incidence tensor
//   ccsd_plan.h      PlanD (what the kernels read of a plan) and the planner: ccsd_build_plan = plan_geometry, plan_xnet, plan_anet_graph,
//                    plan_anet_hodge, plan_fnet, plan_route (k_xa's LDS layout: xa_layout per candidate, plan_xa_layout the search);
//                    the packers and table builders of plan creation (ccsd_pack_*, ccsd_edge_table, ccsd_cell_table, ccsd_hodge_pairs)
//   ccsd_api.h       host side of the C ABI: plan, route, workspace, launchers, the sampler loop; its last line includes
//   ccsd_api_samples.h   the host side of the plan-free entry points (ccsd_quantize .. ccsd_mol_correct: operations on finished samples)
// The product library is built from several translation units compiled in parallel (ccsd_hip.hip: C ABI + the small kernels;
// ccsd_r2*.hip / ccsd_xa.hip: the explicit instantiations of the two big kernel templates); the host emulation used by the
// CPU tests includes everything in one unit.  Reference file:line citations sit next to each restated formula.
#pragma once
#include "ccsd_dev.h"
#include "ccsd_rank2_common.h"
#include "ccsd_k_rank2.h"
#include "ccsd_k_r2.h"
#include "ccsd_k_xa.h"
#include "ccsd_k_update.h"
#include "ccsd_k_finish.h"
#include "ccsd_k_eval.h"
#include "ccsd_k_orbit.h"
#include "ccsd_k_nspdk.h"
#include "ccsd_k_eig.h"
#include "ccsd_k_lift.h"
#include "ccsd_k_mol.h"
#include "ccsd_k_lg.h"
