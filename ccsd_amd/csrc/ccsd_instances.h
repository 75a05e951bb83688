// ccsd_instances.h -- the ONE list of every compile-time instance the host chooses between (k_r2, k_xa, the geometry pairs of the
// general-path kernels, k_gemm_p0).  Everything else is generated from these lists:
//   * the `template` / `extern template` lines: CCSD_INST expands to `template` in the translation unit that owns an instance
//     (ccsd_r2*.hip, ccsd_xa.hip) and to `extern template` in ccsd_hip.hip (the C ABI, which launches them) -- the units compile in
//     parallel, each kernel is compiled once;
//   * the host tables resolve_route (ccsd_api.h) searches once per plan (CCSD_INST_TABLES, defined by ccsd_api.h).  The host emulation
//     has no explicit instantiations: taking an entry's address in the table instantiates it.
// Include protocol (three sections, each emitted once however often the file is included): the lists always; the instantiation lines
// when the includer has defined CCSD_INST (`template` / `extern template`) and the CCSD_INST_R2_A .. _D / CCSD_INST_XA groups it wants,
// AFTER the kernel templates (ccsd_k_r2.h / ccsd_k_xa.h); the host tables when CCSD_INST_TABLES is defined -- by ccsd_api.h alone, after
// ccsd_kernels.h.  ccsd_hip.hip therefore includes the file twice: once itself for the extern lines, once through ccsd_api.h for the tables.
#ifndef CCSD_INSTANCE_LISTS
#define CCSD_INSTANCE_LISTS
// k_r2<MT, RS, AFFINE, GEN1, QM9>: (MT, RS) from E -- MT = ceil(E / 16) row tiles, RS = plain MFMA steps covering E mod 16 behind the
// full 16-wide blocks of phase 2's contraction index (0: last block taken whole; only shapes the affine phase 2, the non-affine
// instances have RS = 0) --, AFFINE ScoreNetworkF, GEN1 = general hodge mlp_value, QM9: 0 run-time geometry, 1 the qm9 geometry
// compiled in, 2 the whole baked qm9_CC plan.  E = N (N - 1) / 2 <= 64, i.e. E in {1, 3, 6, 10, 15, 21, 28, 36, 45, 55}: the (MT, RS)
// pairs that occur.  Four units (ccsd_r2.hip: the qm9 geometry E = 36; ccsd_r2b.hip / ccsd_r2c.hip: the other affine shapes;
// ccsd_r2d.hip: the non-affine ScoreNetworkF path) so that they compile in parallel.
#define CCSD_R2_PAIR(X, MT_, RS_, A_) X(MT_, RS_, A_, false, 0) X(MT_, RS_, A_, true, 0)
#define CCSD_R2_LIST_A(X) CCSD_R2_PAIR(X, 3, 1, true) X(3, 1, true, false, 1) X(3, 1, true, false, 2)
#define CCSD_R2_LIST_B(X) CCSD_R2_PAIR(X, 3, 0, true) CCSD_R2_PAIR(X, 4, 2, true) CCSD_R2_PAIR(X, 2, 2, true) CCSD_R2_PAIR(X, 2, 3, true)
#define CCSD_R2_LIST_C(X) CCSD_R2_PAIR(X, 1, 0, true) CCSD_R2_PAIR(X, 1, 1, true) CCSD_R2_PAIR(X, 1, 2, true) CCSD_R2_PAIR(X, 1, 3, true)
#define CCSD_R2_LIST_D(X) CCSD_R2_PAIR(X, 1, 0, false) CCSD_R2_PAIR(X, 2, 0, false) CCSD_R2_PAIR(X, 3, 0, false) CCSD_R2_PAIR(X, 4, 0, false) \
                          X(3, 0, false, false, 1)                   /* non-affine ScoreNetworkF on the qm9 geometry (qm9_Base_CC) */
// the qm9 geometry of the QM9 != 0 instances: N, E, K and the LDS row strides the planner gives it
#define CCSD_R2_QM9_N 9
#define CCSD_R2_QM9_E 36
#define CCSD_R2_QM9_K 466
#define CCSD_R2_QM9_LDK 488
#define CCSD_R2_QM9_LDH 36
// k_xa<GCH, VAR>: GCH = channel stack in the HBM workspace, VAR = XA_* (ccsd_k_xa.h); MAXT_ = most threads the instance may be
// launched with, F256_ = its 256 threads are compiled in (both checked against the kernel's __launch_bounds__ below)
#define CCSD_XA_LIST(X) \
    X(false, XA_PLAIN, 1024, 0) X(false, XA_HB, 1024, 0) X(false, XA_GMH, 1024, 0) X(false, XA_GEN, 1024, 0) \
    X(false, XA_PLAIN9, 256, 1) X(false, XA_BAKED9, 256, 1) X(false, XA_BAKEDENZ, 1024, 0) \
    X(true, XA_PLAIN, 256, 0) X(true, XA_HB, 256, 0) X(true, XA_GMH, 256, 0) X(true, XA_GEN, 256, 0) \
    X(true, XA_PLAIN20, 256, 0) X(true, XA_BAKED20, 1024, 0) X(true, XA_BAKED38, 1024, 0) X(true, XA_PLAIN38, 256, 0)
// geometry a plain k_xa<., XA_PLAIN> plan must have for the instance with it compiled in: X(GCH, VAR, N, F (0: any), E, ldn)
#define CCSD_XA_GEO_LIST(X) X(false, XA_PLAIN9, 9, 4, 36, 16) X(true, XA_PLAIN20, 20, 0, 190, 24) X(true, XA_PLAIN38, 38, 0, 703, 40)
// (E, K) of the shipped geometries the general-path kernels (k_gemm_h, k_hf_score, k_ew1, k_noise_norm, k_langevin_apply) have
// instances for -- loop bounds, row strides and divisions fold; index 0 = run-time values: X(index, EC, KC, A_), A_ handed through
#define CCSD_GEO_LIST(X, A_) \
    X(1, 190, 1140, A_)    /* community_small (d_min 2 .. d_max) */ \
    X(2, 703, 8436, A_)    /* N = 38 (zinc250k), the 5b substitute's cells */ \
    X(3, 66, 715, A_)      /* ENZYMES_small */
// the geometry k_gemm_h_full / k_hp_full (one workgroup per complex) are instantiated for: community_small
#define CCSD_FULL_E 190
#define CCSD_FULL_K 1140
// k_gemm_p0<NT, KC, mode>: NT = ceil(wc / 16) column tiles of a narrow layer-0 projection, KC = K compiled in (0: the argument)
#define CCSD_P0_LIST(X) X(1, 1140) X(1, 8436) X(1, 0) X(2, 0) X(3, 0) X(4, 0)
#endif

#if defined(CCSD_INST) && !defined(CCSD_INST_DECLARED)
#define CCSD_INST_DECLARED
#define CCSD_R2_DECL(MT_, RS_, A_, G_, Q_) \
    CCSD_INST __global__ void k_r2<MT_, RS_, A_, G_, Q_>(const PlanD* __restrict__, const float* __restrict__, const unsigned char* __restrict__, \
                                                         const unsigned long long* __restrict__, R2Args, RankEpi, NoiseArgs);
#ifdef CCSD_INST_R2_A
CCSD_R2_LIST_A(CCSD_R2_DECL)
#endif
#ifdef CCSD_INST_R2_B
CCSD_R2_LIST_B(CCSD_R2_DECL)
#endif
#ifdef CCSD_INST_R2_C
CCSD_R2_LIST_C(CCSD_R2_DECL)
#endif
#ifdef CCSD_INST_R2_D
CCSD_R2_LIST_D(CCSD_R2_DECL)
#endif
#ifdef CCSD_INST_XA
#define CCSD_XA_DECL(G_, V_, MAXT_, F256_) \
    CCSD_INST __global__ void k_xa<G_, V_>(const PlanD* __restrict__, const float* __restrict__, const unsigned char* __restrict__, XaArgs, NoiseArgs);
CCSD_XA_LIST(CCSD_XA_DECL)
#endif
#endif

#if defined(CCSD_INST_TABLES) && !defined(CCSD_INST_TABLES_DONE)
#define CCSD_INST_TABLES_DONE
typedef void (*R2Fn)(const PlanD* __restrict__, const float* __restrict__, const unsigned char* __restrict__, const unsigned long long* __restrict__,
                     R2Args, RankEpi, NoiseArgs);
typedef void (*XaFn)(const PlanD* __restrict__, const float* __restrict__, const unsigned char* __restrict__, XaArgs, NoiseArgs);
struct R2Entry { int mt, rs, affine, gen1, qm9; R2Fn fn; };
struct XaEntry { int gch, var, max_threads, fixed256; XaFn fn; };
struct GeoEntry { int idx, E, K; };
#define CCSD_R2_ROW(MT_, RS_, A_, G_, Q_) {MT_, RS_, A_, G_, Q_, k_r2<MT_, RS_, A_, G_, Q_>},
static const R2Entry R2_TABLE[] = {CCSD_R2_LIST_A(CCSD_R2_ROW) CCSD_R2_LIST_B(CCSD_R2_ROW) CCSD_R2_LIST_C(CCSD_R2_ROW) CCSD_R2_LIST_D(CCSD_R2_ROW)};
#undef CCSD_R2_ROW
// the thread-limit columns restate k_xa's __launch_bounds__ (ccsd_k_xa.h): 1024 only for the XA_4WAVES instances without a compiled-in count
#define CCSD_XA_ROW(G_, V_, MAXT_, F256_) \
    static_assert((F256_) == ((V_) == XA_PLAIN9 || (V_) == XA_BAKED9) && (MAXT_) == (((F256_) || !XA_4WAVES(G_, V_)) ? 256 : 1024), \
                  "CCSD_XA_LIST: thread limits out of step with k_xa's __launch_bounds__");
CCSD_XA_LIST(CCSD_XA_ROW)
#undef CCSD_XA_ROW
#define CCSD_XA_ROW(G_, V_, MAXT_, F256_) {G_, V_, MAXT_, F256_, k_xa<G_, V_>},
static const XaEntry XA_TABLE[] = {CCSD_XA_LIST(CCSD_XA_ROW)};
#undef CCSD_XA_ROW
#define CCSD_XA_ROW(G_, V_, N_, F_, E_, LDN_) {G_, V_, N_, F_, E_, LDN_},
static const struct { int gch, var, N, F, E, ldn; } XA_GEO_TABLE[] = {CCSD_XA_GEO_LIST(CCSD_XA_ROW)};
#undef CCSD_XA_ROW
#define CCSD_GEO_ROW(I_, E_, K_, A_) {I_, E_, K_},
static const GeoEntry GEO_TABLE[] = {CCSD_GEO_LIST(CCSD_GEO_ROW, 0)};
#undef CCSD_GEO_ROW
// X(EC, KC) expanded with the pair of geometry index geo_ (Route::geo) as compile-time constants, (0, 0) = run-time values
#define CCSD_GEO_CASE(I_, E_, K_, X) case I_: X(E_, K_); break;
#define GEO_EK(geo_, X) \
    do { switch (geo_) { CCSD_GEO_LIST(CCSD_GEO_CASE, X) default: X(0, 0); break; } } while (0)
// (k_gemm_p0 is a GPU-only kernel: the emulation knows the shapes, resolves the same route and launches its stand-in)
#ifdef CCSD_EMU
struct P0Entry { int nt, kc; };
#define CCSD_P0_ROW(NT_, KC_) {NT_, KC_},
#else
typedef void (*P0Fn)(const float* __restrict__, const float* __restrict__, float* __restrict__, int, int, int, int, P0Fuse);
struct P0Entry { int nt, kc; P0Fn fn[5]; };      // fn[P0Fuse::mode]
#define CCSD_P0_ROW(NT_, KC_) {NT_, KC_, {k_gemm_p0<NT_, KC_, 0>, k_gemm_p0<NT_, KC_, 1>, k_gemm_p0<NT_, KC_, 2>, k_gemm_p0<NT_, KC_, 3>, k_gemm_p0<NT_, KC_, 4>}},
#endif
static const P0Entry P0_TABLE[] = {CCSD_P0_LIST(CCSD_P0_ROW)};
#undef CCSD_P0_ROW
#endif
