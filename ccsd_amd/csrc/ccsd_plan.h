// ccsd_plan.h -- device-visible description of the three score networks (offsets into the flat
// weight blob, channel bookkeeping, LDS carve-up) and the host code that derives it from
// ccsd_config_t.  The canonical blob order written here is the contract with
// ccsd_amd/plan.py::pack_weights.
#pragma once
#include "../../include/ccsd_hip.h"
#include "ccsd_rt.h"

#define CCSD_MAXLIN 4     // linears per MLP
#define CCSD_MAXL 8       // attention layers / GCN depth
#define CCSD_MAXHL 2      // hodge layers in the hot part of the plan (PlanD::hl); CCSD_MAXHLX more behind it (PlanD::hlx)
#define CCSD_MAXHLX 6
#define CCSD_MAXFL 4      // HodgeNetworkLayers in ScoreNetworkF
#define CCSD_MAXCN 4      // channels [F, HF, H^2 F, H^3 F] of ScoreNetworkF's input (cnum, cc_utils.py:961-979)
#define CCSD_SMALLW 8     // widest per-thread MLP in the hodge branch (k_xa, k_r2), and the ceiling on its channel counts
#define CCSD_HWIDE 16     // widest hidden Linear of the hodge branch's MLPs: above CCSD_SMALLW only the tiled graph-network route and the tiled rank-2 family serve
#define CCSD_FW 16        // widest per-thread MLP in ScoreNetworkF's general path (fused kernel; hodge baseline mlp_hodge)
#define CCSD_FWMAX 32     // ... in the tiled k_hf_score path
#define CCSD_XA_MAXN 64   // k_xa: one graph per workgroup, its working set in one CU's LDS (node masks: one 64-bit word per graph)
#define CCSD_LG_MAXN 512  // tiled graph-network route (ccsd_k_lg.h): ceiling on N (a graph's channel stack, fdim N^2 floats, is indexed in 32 bits)
#define CCSD_LG_HAD 16    // ... and on the attention dimensions of its ScoreNetworkA_CC hodge branch (k_lg_hodge1: a Q | K row per thread in LDS; k_lg_hd_conv: two MFMA column tiles)
#define CCSD_LG_HD_MAXE 703   // ... on E of ScoreNetworkA_CC stacks of two or more layers (k_lg_hd_*: zinc250k's geometry, N = 38; the dense buffer is c_hid_h E^2 floats per complex)
#define CCSD_LG_MAXHB 8   // ... on the HodgeBaselineLayers of ScoreNetworkA_Base_CC (k_lg_hb_*; PlanD::hb holds the first CCSD_MAXHL, PlanBuilder::hbx all)
#define CCSD_LG_HBW 16    // ... and on their BaselineBlocks' hidden widths: one MFMA column tile (k_lg_hb_hid)

struct MlpD {
    int n, in, hid, out;
    int w[CCSD_MAXLIN], b[CCSD_MAXLIN];
    // register-resident chain (mlp_chain_tile): chain = index into CCSD_CHAIN_SHAPES (0: not chained, block_linear
    // path); offsets of the zero-padded copies Wp[16*to][16*ti], bp[16*to] of every linear in the packed weight buffer,
    // padded to the chosen shape's tile counts.
    // chain == 0 and pb[0] == CCSD_MLP_WT: pw[i] = offset of the TRANSPOSED zero-padded copy Wt_i[in][pad16(out)] of linear i in the packed
    // buffer -- block_linear's B operands: the 16 lanes of a load read 64 consecutive bytes instead of one word from each of 16 rows of W
    // (ScoreNetworkX's 107 -> 214 -> 214 -> 11 head on community_small: 174 k -> 81 k cycles of k_xa; PlanBuilder::transposed)
    int chain;
    int pw[CCSD_MAXLIN], pb[CCSD_MAXLIN];
};
// (input, hidden, output) widths in 16-feature tiles the chain is instantiated for (index 0 = none)
#define CCSD_NSHAPES 8
static const int CCSD_CHAIN_SHAPES[CCSD_NSHAPES][3] = {{0, 0, 0}, {1, 1, 1}, {2, 3, 1}, {2, 4, 1}, {3, 5, 1}, {3, 6, 1}, {4, 7, 1}, {4, 8, 1}};
#define CCSD_CHAIN_EDGE 0x02u      /* shapes allowed per call site (bit = shape index) */
#define CCSD_CHAIN_XFIN 0x24u
#define CCSD_CHAIN_AFIN 0x78u
#define CCSD_CHAIN_AFIN_LG 0x80u   /* the tiled route alone (k_lg_fin_w): ScoreNetworkA's final MLP with 57 .. 64 channels, PlanBuilder::afin_lg */
static inline __host__ __device__ int pad16(int v) { return (v + 15) & ~15; }
#define CCSD_MLP_WT 0x5754
// dims of linear i of an MlpD
static inline __host__ __device__ int mlp_in(const MlpD& m, int i) { return i == 0 ? m.in : m.hid; }
static inline __host__ __device__ int mlp_out(const MlpD& m, int i) { return i == m.n - 1 ? m.out : m.hid; }

struct AttnLayerD {
    int cin, cout, fin, adim, fout, dsplit, nchunk;
    int ci0, co0;             // first input / output channel inside the channel stack
    int attn_base, attn_stride;  // per-channel block: Wq[fin][ad] bq Wk bk Wv[fin][fo] bv
    int conv_mlp;                // conv="MLP": Q / K blocks are W1[2ad][fin] b1[2ad] W2[ad][2ad] b2[ad] (attention.py:168-178)
    MlpD mlp, mc;
    // packed buffer (conv = "GCN"): per input channel [fin][cp] weights + [cp] biases with the Q | K | V columns side by side,
    // zero padded to cp = pad16(2 adim + fout) -- the B operand / bias of gcn_tile_multi without column-part arithmetic
    int qkvp, cp;
    // packed buffer: multi_channel's first Linear W0[hid][cin*fout] as MFMA A fragments, [hidden tile][channel][k-step][lane]
    // with lane = 16 (k & 3) + (unit & 15) and every channel's fout columns zero padded to mcs = ceil(fout / 4) k-steps:
    // one coalesced 256-byte load per k-step (ccsd_pack_mc)
    int mcp, mcs;
};
struct HodgeLayerD {
    int cin, cout, adim, dsplit, nchunk, wc;   // wc = cin*2*adim columns of Wcat
    int wcat, bcat;                             // Wcat[K][wc], bcat[wc]
    int wcatT;                                  // packed buffer: Wcat^T [pad16(wc)][Kp], zero padded (k_r2 float4 B operands)
    MlpD mval, matt;
};

// HodgeBaselineLayer of ScoreNetworkA_Base_CC (hodge_layers.py:273-416).  Per input channel a BaselineBlock: row-wise
// MLP E -> hid -> E (block = W1[hid][E] b1[hid] W2[E][hid] b2[E]); mlp_hodge mixes the channels per (e, e').  The layer's
// rank-2 output (bmm + mlp_rank2) never reaches the score (ScoreNetwork_A_Base_CC.py:303-321) and is not evaluated.
struct HodgeBaseD {
    int cin, cout, hid;
    int blk_base, blk_stride;
    int w2t, w1t;            // packed buffer: per channel W2^T [hid][E] / W1^T [E][hid] (coalesced reads along e / along hid)
    MlpD mh;
};

struct PlanD {
    int N, F, E, K, is_cc;
    float snr, seps;
    // ScoreNetworkX
    int x_depth, x_nhid, x_fdim;
    int x_gw[CCSD_MAXL], x_gb[CCSD_MAXL];
    MlpD x_fin;
    // ScoreNetworkA(_CC)
    int a_L, a_cinit, a_is_cc, a_nch_graph, a_nch_hodge, a_fdim;
    AttnLayerD al[CCSD_MAXL];
    int h_L;
    HodgeLayerD hl[CCSD_MAXHL];
    MlpD a_fin;
    // ScoreNetworkF
    int f_L, f_cnum, f_hmask, f_fdim, f_affine;
    float f_alpha, f_beta, f_gamma;
    MlpD fl[CCSD_MAXFL];
    MlpD f_fin;
    // k_xa LDS carve-up (float offsets) and strides
    int ldn, ldp, pch;          // node-row stride; final-MLP chunk: stride, pairs per chunk
    int cg, pchp, ldpp, pw_pair; // attention channels per group; edge-MLP chunk: pairs, stride, widest hidden layer
    int o_flags, o_x, o_adj, o_an, o_xcat, o_h1, o_h2, o_chan, o_att, o_xcur, o_xnext, o_vcat, o_c0, o_hq, o_hd, o_red;
    int xa_lds_floats;
    int o_hw, hw_stride;        // zero-padded hodge mlp_attention weight blocks (stride between the two layers)
    int o_deg;                  // degree scratch of the dense hodge layer
    int o_edge;                 // LDS copy of the edge table (E ints)
    int x_lds_floats;           // LDS of an X-network-only launch (the ScoreNetworkX phase's regions)
    int chan_global;            // 1: the channel stack [a_fdim][N*N] lives in the HBM workspace (large graphs), not in LDS
    // ---- variants off the headline path, kept behind the fields every launch reads (scalar-cache footprint)
    int chan_rows;               // rows of the channel stack: max(a_fdim, g_nch)
    int f_blk;                   // ScoreNetworkF's general path from zero-padded 8x8 blocks behind the weight blob (-1: none)
    int hb_L;                     // ScoreNetworkA_Base_CC: HodgeBaselineLayers (0 otherwise; above CCSD_MAXHL only on the tiled route,
    HodgeBaseD hb[CCSD_MAXHL];    // whose kernels take their layer's descriptor as an argument: ccsd_plan::hbx)
    int o_hbw;                    // k_xa LDS: mlp_hodge weight blocks of both layers (2 * CCSD_MAXLIN * (16*16+16) floats)
    int o_hbg, o_hbd, hb_rows;    // k_xa LDS: hidden rows of layer 0 [cin][E][hid]; diagonals of layer 1's blocks [cin][E]; rows per chunk
    // HodgeAdjAttentionLayers 2.. (num_layers_h > 2; k_xa<., XA_GEN>), and the layout of the projections k_r2 hands over for
    // layers >= 1: P1 = [E][h_pw] with layer l's wc_l columns at h_poff[l] (each earlier layer padded to 16), U1 = [h_pw]
    HodgeLayerD hlx[CCSD_MAXHLX];
    int h_pw, h_poff[CCSD_MAXHL + CCSD_MAXHLX];
    int geo_off;                  // 1: CCSD_NO_GEO set when the plan was created -- never the compile-time-geometry instances; 2: CCSD_NO_BAKE -- never the baked-plan ones (A/B, parity tests)
    int x_late, o_lx;             // ScoreNetworkX in the idle wave of the A-network's MLP-chain intervals (k_xa); its own LDS region
    int o_h2m, o_hM, o_hX;        // k_xa LDS (h_L > 2): second dense hodge buffer; M_j = sum_c w_c H_c of layers 1..h_L-2; two [E][wc] buffers
    // ScoreNetworkX_GMH (x_gmh = 1): x_depth AttentionLayers gl[] on g_cinit adjacency powers, g_nch channels in all
    int x_gmh, g_cinit, g_nch;
    AttnLayerD gl[CCSD_MAXL];
    float f_betas[CCSD_MAXCN];    // affine ScoreNetworkF with cnum > 2: coefficient of H^j F, j = 1 .. cnum - 1 (f_betas[1] == f_beta)
};
static inline __host__ __device__ const HodgeLayerD& ccsd_hl(const PlanD& p, int l) { return l < CCSD_MAXHL ? p.hl[l] : p.hlx[l - CCSD_MAXHL]; }
static inline HodgeLayerD& ccsd_hl_mut(PlanD& p, int l) { return l < CCSD_MAXHL ? p.hl[l] : p.hlx[l - CCSD_MAXHL]; }

#ifndef CCSD_DEVICE_ONLY
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

// The plan without its weight-derived fields (the affine fold of ScoreNetworkF) and without the sampler's run-time scalars (snr,
// scale_eps: the kernels receive them as launch arguments -- LangArgs / CorrFuse -- and never read them from the plan): what the
// ARCHITECTURE alone determines (network hyper-parameters, geometry, the LDS layout the batch bucket selects).  A kernel instance
// with a BAKED plan (ccsd_baked_*.h) serves exactly the plans whose architecture bytes equal the baked ones -- whatever snr /
// scale_eps / predictor the sampling configuration names.
static inline void ccsd_plan_arch_bytes(const PlanD& p, unsigned char* out) {
    PlanD q;
    memcpy(&q, &p, sizeof(PlanD));
    q.snr = q.seps = 0.f;
    q.f_alpha = q.f_beta = q.f_gamma = 0.f;
    for (int j = 0; j < CCSD_MAXCN; ++j) q.f_betas[j] = 0.f;
    memcpy(out, &q, sizeof(PlanD));
}
// ... written as a C header (CCSD_DUMP_PLAN; tools/bake_plan.py).  nm: the macro infix, CCSD_BAKED_<nm>_PLAN
static inline void ccsd_dump_plan(const PlanD& p, const char* path, const char* nm) {
    unsigned char bytes[sizeof(PlanD)];
    ccsd_plan_arch_bytes(p, bytes);
    FILE* f = fopen(path, "w");
    if (!f) return;
    fprintf(f, "// GENERATED by tools/bake_plan.py (do not edit): the PlanD of a shipped configuration at its bench batch as a compile-time\n"
               "// constant (architecture bytes: ccsd_plan_arch_bytes, the weight-derived affine fold zeroed).  The baked kernel instances read\n"
               "// their plan from it instead of from memory; the host selects them only for plans whose architecture bytes are equal.\n"
               "#pragma once\n#define CCSD_BAKED_%s_SIZE %zu\n#define CCSD_BAKED_%s_A_L %d      /* AttentionLayers of ScoreNetworkA: unroll count */\n"
               "alignas(16) static constexpr unsigned char CCSD_BAKED_%s_PLAN[CCSD_BAKED_%s_SIZE] = {", nm, sizeof(PlanD), nm, p.a_L, nm, nm);
    for (size_t i = 0; i < sizeof(PlanD); ++i) fprintf(f, "%s%u,", (i % 40) ? "" : "\n    ", (unsigned)bytes[i]);
    fprintf(f, "\n};\n");
    fclose(f);
}

static inline int64_t ccsd_comb(int n, int k) {
    if (k < 0 || k > n) return 0;
    long double r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
    return (int64_t)(r + 0.5L);
}
static inline void ccsd_dims(const ccsd_config_t* c, int* E, int64_t* K) {
    *E = c->N * (c->N - 1) / 2;
    int64_t k = 0;
    if (c->is_cc)
        for (int d = c->d_min; d <= c->d_max; ++d) k += ccsd_comb(c->N, d);
    *K = k;
}

// What the planner decides beside PlanD, for the tiled route's launches and the packed buffer: ccsd_plan keeps a copy (one assignment).
// Its verdicts lg and h_wide are not in here: they are fields of the plan's Route (ccsd_api.h), which resolve_route completes
struct PlanRouteOut {
    HodgeBaseD hbx[CCSD_LG_MAXHB] = {};   // every HodgeBaselineLayer of ScoreNetworkA_Base_CC (PlanD::hb holds the first two): arguments of the k_lg_hb_* launches
    // route plans with two or more HodgeAdjAttentionLayers: mlp_attention of every layer but the last with packed copies for
    // mlp_chain_tile (k_lg_hd_dense).  Kept out of PlanD, and reserved behind everything else in the packed buffer: no plan k_xa serves moves.
    // Plans with hodge MLPs wider than 8 (h_wide): EVERY layer's -- the last layer's diagonal runs the chain too (k_lg_hd_diag_w, k_lg_hodge1_w)
    MlpD hdm[CCSD_MAXHL + CCSD_MAXHLX] = {};
    // wide plans whose PlanD::a_fin has no chained shape, 57 to 64 channels (k_xa runs those through block_linear, and narrow plans with such
    // a final MLP stay with it): the final MLP with packed copies in the route's own shape (CCSD_CHAIN_AFIN_LG, k_lg_fin_w); chain == 0: none
    MlpD afin_lg = {};
    size_t npacked = 0;                   // floats of the packed buffer
};
struct PlanBuilder : PlanRouteOut {
    int cur = 0;
    int pcur = 0;     // packed (chain) weight buffer
    // reserve padded copies of an MLP's linears for mlp_chain_tile
    void chainify(MlpD& m, unsigned allowed);
    void transposed(MlpD& m) {          // (non-chained MLPs that run through block_linear; no_mlp_wt: diagnostic)
        if (m.chain || no_mlp_wt) return;
        for (int i = 0; i < m.n; ++i) { m.pw[i] = pcur; pcur += (i == 0 ? m.in : m.hid) * (((i == m.n - 1 ? m.out : m.hid) + 15) & ~15); }
        m.pb[0] = CCSD_MLP_WT;
    }
    std::string err;
    int status = CCSD_OK;
    // in: the plan-shaping switches, read from the environment once by ccsd_plan_create (read_knobs, ccsd_api.h)
    int lg_force = 0;   // CCSD_LARGE_GRAPH: the tiled route for any eligible graph-only plan (1), for eligible combinatorial complexes too (2)
    int no_mlp_wt = 0;  // CCSD_NO_MLP_WT
    int xa_pass = -1;   // CCSD_XA_PASS: first k_xa LDS budget candidate tried (-1: by batch_hint)
    int xa_gch = 0;     // CCSD_XA_GCH: the channel stack in the HBM workspace first
    int verbose = 0;    // CCSD_VERBOSE
    int lg = 0;         // out: the plan takes the tiled graph-network route (ccsd_k_lg.h) instead of k_xa
    // out: some Linear of the hodge branch's MLPs is wider than CCSD_SMALLW (num_linears_h >= 2, hid = 9 .. 16).  Such a plan takes the route
    // at any N, never k_xa or k_r2 (their per-thread small_mlp stays 8 wide)
    int h_wide = 0;
    // the packed copies only route plans read (hdm, afin_lg), reserved behind everything else in the packed buffer (no plan k_xa serves moves)
    void route_copies(const PlanD& p) {
        if (h_wide && !p.a_fin.chain) {
            afin_lg = p.a_fin; chainify(afin_lg, CCSD_CHAIN_AFIN_LG);
            // (ccsd_lg_ineligible admitted the plan for this shape: launch_lg must never meet an unchained final MLP)
            if (!afin_lg.chain) fail(CCSD_ERR_RUNTIME, "tiled graph-network route: no chained shape for the final MLP");
        }
        for (int l = 0; l + (h_wide ? 0 : 1) < p.h_L; ++l) {
            hdm[l] = ccsd_hl(p, l).matt;
            chainify(hdm[l], CCSD_CHAIN_EDGE);
        }
    }
    int take(int64_t n) {
        int o = cur;
        cur += (int)n;
        return o;
    }
    void fail(int st, const std::string& m) {
        if (status == CCSD_OK) { status = st; err = m; }
    }
    bool reject(int st, const std::string& m) { fail(st, m); return false; }   // (for the planning steps, which return whether to go on)
    MlpD mlp(int n, int in, int hid, int out) {
        MlpD m{};
        m.n = n; m.in = in; m.hid = hid; m.out = out;
        if (n < 1 || n > CCSD_MAXLIN) { fail(CCSD_ERR_UNSUPPORTED, "MLP with more than 4 (or fewer than 1) linears"); m.n = 1; }
        for (int i = 0; i < m.n; ++i) {
            m.w[i] = take((int64_t)mlp_out(m, i) * mlp_in(m, i));
            m.b[i] = take(mlp_out(m, i));
        }
        return m;
    }
};

inline void PlanBuilder::chainify(MlpD& m, unsigned allowed) {
    m.chain = 0;
    const int ni = pad16(m.in) / 16, nh = m.n > 1 ? pad16(m.hid) / 16 : 1, no = pad16(m.out) / 16;
    for (int sidx = 1; sidx < CCSD_NSHAPES && !m.chain; ++sidx) {
        const int* sh = CCSD_CHAIN_SHAPES[sidx];
        if (((allowed >> sidx) & 1u) && sh[0] >= ni && sh[1] >= nh && sh[2] >= no) m.chain = sidx;
    }
    if (!m.chain) return;
    const int* sh = CCSD_CHAIN_SHAPES[m.chain];
    for (int i = 0; i < m.n; ++i) {
        const int ip = 16 * (i == 0 ? sh[0] : sh[1]), op = 16 * (i == m.n - 1 ? sh[2] : sh[1]);
        m.pw[i] = pcur; pcur += op * ip;
        m.pb[i] = pcur; pcur += op;
    }
}
// Position of W[o][k] inside a chain linear's packed block: MFMA A-fragment order [out tile][in tile][lane][4] with
// lane = 16 ((k & 15) >> 2) + (o & 15) -- the float4 a lane feeds to four consecutive k-steps; one wave-level load is 1 KB
// contiguous (eight full cache lines; the row-major copy cost sixteen half-used ones per load)
static inline __host__ __device__ int ccsd_chain_widx(int o, int k, int ip) {
    return (((o >> 4) * (ip >> 4) + (k >> 4)) * 64 + (((k & 15) >> 2) << 4) + (o & 15)) * 4 + (k & 3);
}
// zero-padded copies of a chain MLP's linears (torch layout [out][in]) into the packed buffer
static inline void ccsd_pack_mlp(const MlpD& m, const float* w, float* packed) {
    if (!m.chain && m.pb[0] == CCSD_MLP_WT) {       // transposed copies (block_linear)
        for (int i = 0; i < m.n; ++i) {
            const int in = mlp_in(m, i), out = mlp_out(m, i), op = pad16(out);
            for (int k = 0; k < in; ++k)
                for (int o = 0; o < out; ++o) packed[(size_t)m.pw[i] + (size_t)k * op + o] = w[(size_t)m.w[i] + (size_t)o * in + k];
        }
    }
    if (!m.chain) return;
    const int* sh = CCSD_CHAIN_SHAPES[m.chain];
    for (int i = 0; i < m.n; ++i) {
        const int in = i == 0 ? m.in : m.hid, out = i == m.n - 1 ? m.out : m.hid, ip = 16 * (i == 0 ? sh[0] : sh[1]);
        for (int o = 0; o < out; ++o) {
            for (int k = 0; k < in; ++k) packed[m.pw[i] + ccsd_chain_widx(o, k, ip)] = w[m.w[i] + o * in + k];
            packed[m.pb[i] + o] = w[m.b[i] + o];
        }
    }
}

// multi_channel's first Linear in MFMA A-fragment order, zero padded (AttnLayerD::mcp)
static inline void ccsd_pack_mc(const AttnLayerD& a, const float* w, float* packed) {
    const int hid = a.mc.hid, nht = pad16(hid) >> 4;
    for (int ht = 0; ht < nht; ++ht)
        for (int c = 0; c < a.cin; ++c)
            for (int st = 0; st < a.mcs; ++st)
                for (int lane = 0; lane < 64; ++lane) {
                    const int hh = 16 * ht + (lane & 15), o = 4 * st + (lane >> 4);
                    packed[a.mcp + (size_t)((ht * a.cin + c) * a.mcs + st) * 64 + lane] =
                        (hh < hid && o < a.fout) ? w[a.mc.w[0] + (size_t)hh * a.mc.in + c * a.fout + o] : 0.f;
                }
}
// Q | K | V weights of a GCN-conv AttentionLayer side by side, zero padded (AttnLayerD::qkvp)
static inline void ccsd_pack_qkv(const AttnLayerD& a, const float* w, float* packed) {
    if (a.conv_mlp) return;
    const int ad = a.adim, fo = a.fout, fi = a.fin, cp = a.cp;
    for (int c = 0; c < a.cin; ++c) {
        const float* blk = w + a.attn_base + (size_t)c * a.attn_stride;      // Wq[fi][ad] bq[ad] Wk[fi][ad] bk[ad] Wv[fi][fo] bv[fo]
        float* dst = packed + a.qkvp + (size_t)c * (fi * cp + cp);
        for (int part = 0; part < 3; ++part) {
            const int ow = part == 2 ? fo : ad, c0 = part * ad;
            const float* wp_ = blk + part * (fi * ad + ad);
            for (int k = 0; k < fi; ++k)
                for (int o = 0; o < ow; ++o) dst[k * cp + c0 + o] = wp_[k * ow + o];
            for (int o = 0; o < ow; ++o) dst[fi * cp + c0 + o] = wp_[fi * ow + o];
        }
    }
}

// transposed copies of a HodgeBaselineLayer's BaselineBlocks (HodgeBaseD::w2t, w1t)
static inline void ccsd_pack_hb_blocks(const HodgeBaseD& h, int E, const float* w, float* packed) {
    for (int c = 0; c < h.cin; ++c) {
        const float* blk = w + h.blk_base + (size_t)c * h.blk_stride;    // W1[hid][E] b1[hid] W2[E][hid] b2[E]
        const float* w2 = blk + h.hid * E + h.hid;
        for (int e = 0; e < E; ++e)
            for (int hh = 0; hh < h.hid; ++hh) {
                packed[(size_t)h.w2t + ((size_t)c * h.hid + hh) * E + e] = w2[e * h.hid + hh];
                packed[(size_t)h.w1t + ((size_t)c * E + e) * h.hid + hh] = blk[hh * E + e];
            }
    }
}
// The packed weight buffer (ccsd_plan::wp; 4 floats of slack behind it): every copy the planner reserved, zero padded.  lg: the plan takes
// the tiled route, whose own copies (x.hdm, x.afin_lg) are packed too
static inline std::vector<float> ccsd_pack_weights(const PlanD& p, const PlanRouteOut& x, int lg, const float* w) {
    std::vector<float> packed(x.npacked + 4, 0.f);
    float* out = packed.data();
    auto attn = [&](const AttnLayerD& a) { ccsd_pack_mlp(a.mlp, w, out); ccsd_pack_mlp(a.mc, w, out); ccsd_pack_qkv(a, w, out); ccsd_pack_mc(a, w, out); };
    ccsd_pack_mlp(p.x_fin, w, out);
    for (int l = 0; l < p.a_L; ++l) attn(p.al[l]);
    if (p.x_gmh) for (int l = 0; l < p.x_depth; ++l) attn(p.gl[l]);
    for (int l = 0; l < p.hb_L; ++l) {      // mlp_hodge of the dense layers; the BaselineBlocks' weights
        ccsd_pack_mlp(x.hbx[l].mh, w, out);
        ccsd_pack_hb_blocks(x.hbx[l], p.E, w, out);
    }
    ccsd_pack_mlp(p.a_fin, w, out);
    if (lg) {
        for (int l = 0; l < p.h_L; ++l) ccsd_pack_mlp(x.hdm[l], w, out);     // (the last layer's: wide plans only)
        if (x.afin_lg.chain) ccsd_pack_mlp(x.afin_lg, w, out);
    }
    const int Kp = (p.K + 31) & ~31;
    for (int l = 0; l < p.h_L; ++l) {       // Wcat^T of the hodge projections for k_r2
        const HodgeLayerD& h = ccsd_hl(p, l);
        for (int k = 0; k < p.K; ++k)
            for (int n = 0; n < h.wc; ++n) out[(size_t)h.wcatT + (size_t)n * Kp + k] = w[(size_t)h.wcat + (size_t)k * h.wc + n];
    }
    return packed;
}

// Enumeration tables (get_cells, cc_utils.py:72-94).  Edges: combinations(range(N), 2) row-major, (i, j) in bytes (2 bytes of slack)
static inline std::vector<unsigned char> ccsd_edge_table(int N, int E) {
    std::vector<unsigned char> edges((size_t)2 * E + 2);
    int e = 0;
    for (int i = 0; i < N; ++i)
        for (int j = i + 1; j < N; ++j) { edges[2 * e] = (unsigned char)i; edges[2 * e + 1] = (unsigned char)j; ++e; }
    return edges;
}
// Cells: combinations(range(N), k) for k = d_min .. d_max, lexicographic, as node bitmasks (one word of slack).  false: not K of them
static inline bool ccsd_cell_table(const ccsd_config_t* cfg, int K, std::vector<unsigned long long>* cells) {
    cells->assign((size_t)K + 1, 0ull);
    if (!cfg->is_cc) return true;
    const int N = cfg->N;
    size_t c = 0;
    std::vector<int> idx;
    for (int k = cfg->d_min; k <= cfg->d_max; ++k) {
        idx.resize(k);
        for (int i = 0; i < k; ++i) idx[i] = i;
        while (true) {
            unsigned long long m = 0;
            for (int i = 0; i < k; ++i) m |= 1ull << idx[i];
            (*cells)[c++] = m;
            int i = k - 1;
            while (i >= 0 && idx[i] == N - k + i) --i;
            if (i < 0) break;
            ++idx[i];
            for (int j = i + 1; j < k; ++j) idx[j] = idx[j - 1] + 1;
        }
    }
    return (int)c == K;
}
// k_xa's pair table of the dense hodge layer: (e, e2), e <= e2, row-major, in bytes (E <= 255)
static inline std::vector<unsigned char> ccsd_hodge_pairs(int E) {
    std::vector<unsigned char> hp;
    for (int e = 0; e < E; ++e)
        for (int e2 = e; e2 < E; ++e2) { hp.push_back((unsigned char)e); hp.push_back((unsigned char)e2); }
    return hp;
}

static inline int round_ld(int rows) {  // node-row stride of the feature-major LDS arrays: multiple of 8, never a multiple of 32
    int r = (rows + 7) / 8 * 8;          // (== 16 mod 32 is conflict-free for the MFMA A-fragment reads, 8 / 24 mod 32 two-way)
    if (r % 32 == 0) r += 8;
    return r;
}

// dynamic LDS of the route's per-node MLP kernel k_lg_nmlp for one MLP: 16 rows of its input and of two activations (bytes)
static inline size_t lg_nmlp_lds_of(const MlpD& m) {
    const int wmax = m.hid > m.out ? m.hid : m.out;
    return (size_t)16 * ((m.in > wmax ? m.in : wmax) + wmax) * 4;
}
static inline size_t lg_nmlp_lds(const PlanD& p) {
    size_t v = lg_nmlp_lds_of(p.x_fin);
    for (int l = 0; l < p.a_L; ++l) if (lg_nmlp_lds_of(p.al[l].mc) > v) v = lg_nmlp_lds_of(p.al[l].mc);
    return v;
}
// Why the tiled graph-network route (ccsd_k_lg.h) cannot serve a plan whose networks `p` holds (nullptr: it can).  It covers plans
// with the plain ScoreNetworkX and a GCN-conv ScoreNetworkA whose edge MLPs are the 16-wide MFMA chains and whose final MLP is a
// chained shape (fdim <= 64): graph-only ones, and combinatorial complexes (N <= 64) with ScoreNetworkA_CC -- ONE
// HodgeAdjAttentionLayer, whose hodge adjacency is diagonal (k_lg_hodge1), or 2 to 8 of them up to E = CCSD_LG_HD_MAXE (k_lg_hd_*),
// attention dimensions at most CCSD_LG_HAD -- or with ScoreNetworkA_Base_CC, 1 to CCSD_LG_MAXHB HodgeBaselineLayers and BaselineBlocks
// at most CCSD_LG_HBW wide (k_lg_hb_*); the dense E x E layers of both are tiled through the workspace.
// ScoreNetworkX_GMH, conv = "MLP", wider BaselineBlocks and ScoreNetworkA_CC stacks of two or more layers beyond E = 703 stay with k_xa.
static inline const char* ccsd_lg_ineligible(const ccsd_config_t* c, const PlanD* p, int h_wide) {
    if (p->a_is_cc == 2 && (c->h_nhid > CCSD_LG_HBW || (c->h_num_layers > 1 && c->h_adim > CCSD_LG_HBW)))
        return "ScoreNetworkA_Base_CC with BaselineBlocks wider than 16";
    if (p->h_L > 1 && p->E > CCSD_LG_HD_MAXE) return "hodge stacks of two or more layers beyond E = 703 (the dense E x E hodge layer)";
    if (c->is_cc && p->a_is_cc != 2 && (p->a_is_cc != 1 || p->h_L < 1)) return "combinatorial-complex plans without ScoreNetworkA_CC";
    for (int l = 0; l < p->h_L; ++l) if (ccsd_hl(*p, l).adim > CCSD_LG_HAD) return "hodge attention dimensions above 16";
    if (p->x_gmh) return "ScoreNetworkX_GMH";
    for (int l = 0; l < p->a_L; ++l) {
        const AttnLayerD& a = p->al[l];
        if (a.conv_mlp) return "conv = \"MLP\" attention";
        if (a.mlp.chain != 1) return "edge MLPs wider than 16 features";
        if (a.adim > 64) return "attention dimensions above 64";
    }
    // (57 to 64 channels: the route's own shape, for the plans that have no other kernel -- wide hodge MLPs; any other such plan stays with k_xa)
    if (!p->a_fin.chain && p->a_fdim > 64) return "final MLPs wider than 64 input channels";
    if (!p->a_fin.chain && !h_wide) return "final MLPs of 57 to 64 input channels without hodge MLPs wider than 8";
    if (lg_nmlp_lds(*p) > 160 * 1024) return "per-node MLPs whose 16-row activations exceed the 160 KB LDS of a CU";
    return nullptr;
}

// ---- ccsd_build_plan, step by step.  Each step returns whether to go on (false: pb holds the failure).  The ORDER of the pb.take /
// pb.mlp calls is the blob order shared with ccsd_amd/plan.py; the order of the pb.pcur reservations fixes the packed offsets the plan stores.

// Channels into and out of layer l of a stack of L: c_init into the first, c_hid between the layers, c_final out of the last -- a single
// layer counts as a first one and puts out c_hid (the channel-count checks then demand c_hid == c_final).  plan.py: stack_io
static inline void ccsd_stack_io(int l, int L, int c_init, int c_hid, int c_final, int* cin, int* cout) {
    *cin = l == 0 ? c_init : c_hid;
    *cout = (l == L - 1 && l != 0) ? c_final : c_hid;
}

// geometry and range checks
static inline bool plan_geometry(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    if (!c || c->abi_version != CCSD_ABI_VERSION) return pb.reject(CCSD_ERR_INVALID, "abi_version mismatch");
    if (c->N < 2 || c->F < 1) return pb.reject(CCSD_ERR_UNSUPPORTED, "need 2 <= N <= 512 and F >= 1");
    if (c->N > CCSD_LG_MAXN)
        return pb.reject(CCSD_ERR_UNSUPPORTED, "N = " + std::to_string(c->N) + " exceeds the ceiling of the tiled graph-network route (N <= 512)");
    // (above 64 nodes only the tiled route serves: checked once the networks are known, plan_route)
    if (c->N > CCSD_XA_MAXN && c->is_cc)
        return pb.reject(CCSD_ERR_UNSUPPORTED, "combinatorial-complex plans need N <= 64 (the tiled route above 64 nodes is graph-only)");
    int E; int64_t K64;
    ccsd_dims(c, &E, &K64);
    if (c->is_cc && (c->d_min < 1 || c->d_max < c->d_min || c->d_max > c->N)) return pb.reject(CCSD_ERR_INVALID, "bad d_min/d_max");
    if (K64 > (1 << 24)) return pb.reject(CCSD_ERR_UNSUPPORTED, "rank-2 width K too large");
    p->N = c->N; p->F = c->F; p->E = E; p->K = (int)K64; p->is_cc = c->is_cc;
    p->snr = c->snr; p->seps = c->scale_eps;
    return true;
}

// hyper-parameters of a stack of AttentionLayers (ScoreNetworkA's graph branch, ScoreNetworkX_GMH)
struct AttnStackCfg { int L, c_init, c_hid, c_final, nhid, adim, heads, num_linears, conv_mlp; };
// one AttentionLayer (attention.py:203-304) of a stack: dims, blob ranges, chained edge MLP.  ch: the stack's channels so far
static inline bool plan_attn_layer(PlanBuilder& pb, AttnLayerD& a, int l, const AttnStackCfg& s, int F, int& ch) {
    const bool first = l == 0;
    ccsd_stack_io(l, s.L, s.c_init, s.c_hid, s.c_final, &a.cin, &a.cout);
    a.fin = first ? F : s.nhid;
    a.adim = first ? s.nhid : s.adim;
    a.fout = s.nhid;
    a.dsplit = a.adim / s.heads;
    if (a.dsplit < 1 || a.adim % a.dsplit) return pb.reject(CCSD_ERR_INVALID, "attn_dim not divisible into head chunks");
    a.nchunk = a.adim / a.dsplit;
    a.ci0 = ch - a.cin; a.co0 = ch; ch += a.cout;
    a.conv_mlp = s.conv_mlp ? 1 : 0;
    a.attn_stride = (a.conv_mlp ? 2 * (2 * a.adim * a.fin + 2 * a.adim + a.adim * 2 * a.adim + a.adim) : 2 * (a.fin * a.adim + a.adim)) +
                    a.fin * a.fout + a.fout;
    a.attn_base = pb.take((int64_t)a.cin * a.attn_stride);
    a.cp = pad16(2 * a.adim + a.fout);
    a.qkvp = pb.pcur;
    if (!a.conv_mlp) pb.pcur += a.cin * (a.fin * a.cp + a.cp);
    const int hid = 2 * (a.cin > a.cout ? a.cin : a.cout);
    a.mlp = pb.mlp(s.num_linears, 2 * a.cin, hid, a.cout);
    pb.chainify(a.mlp, CCSD_CHAIN_EDGE);
    pb.transposed(a.mlp);
    a.mc = pb.mlp(2, a.cin * a.fout, hid, a.fout);
    pb.transposed(a.mc);
    a.mcs = (a.fout + 3) >> 2;
    a.mcp = pb.pcur;
    pb.pcur += (pad16(hid) >> 4) * a.cin * a.mcs * 64;
    return true;
}
// ... and the whole stack; *nch: its channels, the c_init inputs included
static inline bool plan_attn_stack(PlanBuilder& pb, AttnLayerD* layers, const AttnStackCfg& s, int F, int* nch) {
    int ch = s.c_init;
    for (int l = 0; l < s.L; ++l)
        if (!plan_attn_layer(pb, layers[l], l, s, F, ch)) return false;
    *nch = ch;
    return true;
}

// ScoreNetworkX, plain (GCN layers) or GMH (AttentionLayers on g_cinit adjacency powers)
static inline bool plan_xnet(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    if (c->x_depth < 1 || c->x_depth > CCSD_MAXL) return pb.reject(CCSD_ERR_UNSUPPORTED, "x_depth out of range");
    p->x_depth = c->x_depth; p->x_nhid = c->x_nhid; p->x_fdim = c->F + c->x_depth * c->x_nhid;
    p->x_gmh = c->x_gmh ? 1 : 0;
    if (p->x_gmh) {
        if (c->x_num_heads < 1 || c->x_c_init < 1) return pb.reject(CCSD_ERR_INVALID, "bad heads/c_init (ScoreNetworkX_GMH)");
        p->g_cinit = c->x_c_init;
        const AttnStackCfg s = {c->x_depth, c->x_c_init, c->x_c_hid, c->x_c_final, c->x_nhid, c->x_adim, c->x_num_heads, c->x_num_linears, c->x_conv_mlp};
        if (!plan_attn_stack(pb, p->gl, s, c->F, &p->g_nch)) return false;
        p->x_gw[0] = p->gl[0].attn_base;
    } else {
        for (int l = 0; l < c->x_depth; ++l) {
            p->x_gw[l] = pb.take((int64_t)(l ? c->x_nhid : c->F) * c->x_nhid);
            p->x_gb[l] = pb.take(c->x_nhid);
        }
    }
    p->x_fin = pb.mlp(3, p->x_fdim, 2 * p->x_fdim, c->F);
    pb.chainify(p->x_fin, CCSD_CHAIN_XFIN);
    pb.transposed(p->x_fin);
    return true;
}

// ScoreNetworkA, graph branch
static inline bool plan_anet_graph(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    if (c->a_num_layers < 1 || c->a_num_layers > CCSD_MAXL) return pb.reject(CCSD_ERR_UNSUPPORTED, "a_num_layers out of range");
    if (c->a_num_heads < 1 || c->a_c_init < 1) return pb.reject(CCSD_ERR_INVALID, "bad heads/c_init");
    p->a_L = c->a_num_layers; p->a_cinit = c->a_c_init; p->a_is_cc = c->a_is_cc_net;
    const AttnStackCfg s = {c->a_num_layers, c->a_c_init, c->a_c_hid, c->a_c_final, c->a_nhid, c->a_adim, c->a_num_heads, c->a_num_linears, c->a_conv_mlp};
    if (!plan_attn_stack(pb, p->al, s, c->F, &p->a_nch_graph)) return false;
    if (c->a_c_hid * (p->a_L - 1) + c->a_c_final + c->a_c_init != p->a_nch_graph)
        return pb.reject(CCSD_ERR_INVALID, "ScoreNetworkA channel count inconsistent (num_layers==1 needs c_hid==c_final)");
    return true;
}

// ScoreNetworkA_Base_CC's hodge branch: every HodgeBaselineLayer into pb.hbx, the first CCSD_MAXHL into p->hb as well
static inline bool plan_hodge_base(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    if (!c->is_cc) return pb.reject(CCSD_ERR_INVALID, "ScoreNetworkA_Base_CC is only for combinatorial complexes");
    if (c->h_num_layers < 1 || c->h_num_layers > CCSD_LG_MAXHB) return pb.reject(CCSD_ERR_UNSUPPORTED, "HIP path supports 1 to 8 HodgeBaselineLayers");
    p->hb_L = c->h_num_layers;
    const int E = p->E;
    for (int l = 0; l < p->hb_L; ++l) {
        HodgeBaseD& h = pb.hbx[l];
        ccsd_stack_io(l, p->hb_L, c->a_c_init, c->h_c_hid, c->h_c_final, &h.cin, &h.cout);
        h.hid = l == 0 ? c->h_nhid : c->h_adim;
        if (h.hid < 1) return pb.reject(CCSD_ERR_INVALID, "HodgeBaselineLayer hidden width < 1");
        h.blk_stride = 2 * h.hid * E + h.hid + E;
        h.blk_base = pb.take((int64_t)h.cin * h.blk_stride);
        h.w2t = pb.pcur; pb.pcur += h.cin * h.hid * E;
        h.w1t = pb.pcur; pb.pcur += h.cin * h.hid * E;
        const int hid = 2 * (h.cin > h.cout ? h.cin : h.cout);
        h.mh = pb.mlp(c->h_num_linears, h.cin, hid, h.cout);
        // a dense layer evaluates it per (e, e') pair on MFMA: the first one (k_xa, k_lg_hb_dense) and, on the tiled route, every other
        // layer but the last (only stacks of more than two have such a layer: no plan k_xa serves moves)
        if (l == 0 || l < p->hb_L - 1) pb.chainify(h.mh, CCSD_CHAIN_EDGE);
        if (h.cin > CCSD_FW || (c->h_num_linears > 1 && hid > CCSD_FW) || h.cout > CCSD_FW)
            return pb.reject(CCSD_ERR_UNSUPPORTED, "HodgeBaselineLayer mlp_hodge wider than 16");
        if (l < CCSD_MAXHL) p->hb[l] = h;
        p->a_nch_hodge += h.cout;
    }
    return true;
}
// ScoreNetworkA_CC's hodge branch: HodgeAdjAttentionLayers
static inline bool plan_hodge_attn(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    if (!c->is_cc) return pb.reject(CCSD_ERR_INVALID, "ScoreNetworkA_CC is only for combinatorial complexes");
    if (c->h_num_layers < 1 || c->h_num_layers > CCSD_MAXHL + CCSD_MAXHLX)
        return pb.reject(CCSD_ERR_UNSUPPORTED, "HIP path supports 1 to 8 HodgeAdjAttentionLayers");
    p->h_L = c->h_num_layers;
    const int K = p->K;
    for (int l = 0; l < p->h_L; ++l) {
        HodgeLayerD& h = ccsd_hl_mut(*p, l);
        ccsd_stack_io(l, p->h_L, c->a_c_init, c->h_c_hid, c->h_c_final, &h.cin, &h.cout);
        h.adim = l == 0 ? c->h_nhid : c->h_adim;
        h.dsplit = h.adim / c->h_num_heads;
        if (h.dsplit < 1 || h.adim % h.dsplit) return pb.reject(CCSD_ERR_INVALID, "hodge attn_dim not divisible into head chunks");
        h.nchunk = h.adim / h.dsplit;
        h.wc = h.cin * 2 * h.adim;
        h.wcat = pb.take((int64_t)K * h.wc);
        h.bcat = pb.take(h.wc);
        h.wcatT = pb.pcur; pb.pcur += pad16(h.wc) * ((K + 31) & ~31);
        const int hid = 2 * (h.cin > h.cout ? h.cin : h.cout);
        h.mval = pb.mlp(c->h_num_linears, h.cin, hid, 1);
        h.matt = pb.mlp(c->h_num_linears, h.cin, hid, h.cout);
        const int hidw = c->h_num_linears > 1 ? hid : 0;        // (a single-Linear MLP has no Linear of width hid)
        if (h.cin > CCSD_SMALLW || hidw > CCSD_HWIDE || h.cout > CCSD_SMALLW) return pb.reject(CCSD_ERR_UNSUPPORTED, "hodge MLP wider than 16");
        if (hidw > CCSD_SMALLW) pb.h_wide = 1;
        p->a_nch_hodge += h.cout;
    }
    return true;
}
// ScoreNetworkA's hodge branch (none for the graph-only network) and its final MLP over the channels of both branches
static inline bool plan_anet_hodge(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    if (c->a_is_cc_net) {
        p->a_nch_hodge = c->a_c_init;
        if (!(c->a_is_cc_net == 2 ? plan_hodge_base(c, p, pb) : plan_hodge_attn(c, p, pb))) return false;
        if (c->h_c_hid * (p->hb_L + p->h_L - 1) + c->h_c_final + c->a_c_init != p->a_nch_hodge)
            return pb.reject(CCSD_ERR_INVALID, "hodge channel count inconsistent (num_layers_h==1 needs c_hid_h==c_final_h)");
        // the transposed copies Wcat_l^T of layers >= 1 are consecutive [pad16(wc_l)][Kp] blocks: k_r2 treats them as ONE
        // projection of h_pw columns
        for (int l = 1; l < p->h_L; ++l) {
            p->h_poff[l] = p->h_pw;
            if (ccsd_hl(*p, l).wcatT != ccsd_hl(*p, 1).wcatT + p->h_pw * ((p->K + 31) & ~31)) return pb.reject(CCSD_ERR_RUNTIME, "Wcat^T blocks not consecutive");
            p->h_pw += l == p->h_L - 1 ? ccsd_hl(*p, l).wc : pad16(ccsd_hl(*p, l).wc);
        }
    }
    p->a_fdim = p->a_nch_graph + p->a_nch_hodge;
    p->a_fin = pb.mlp(3, p->a_fdim, 2 * p->a_fdim, 1);
    pb.chainify(p->a_fin, CCSD_CHAIN_AFIN);
    pb.transposed(p->a_fin);
    return true;
}

// ScoreNetworkF (combinatorial complexes), and whether its general path reads zero-padded blocks behind the blob (f_blk)
static inline bool plan_fnet(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    p->f_blk = -1;
    if (!c->is_cc) return true;
    if (c->f_num_layers < 1 || c->f_num_layers > CCSD_MAXFL) return pb.reject(CCSD_ERR_UNSUPPORTED, "f_num_layers out of range");
    if (c->f_cnum < 1 || c->f_cnum > CCSD_MAXCN) return pb.reject(CCSD_ERR_UNSUPPORTED, "HIP path supports cnum in 1..4");
    p->f_L = c->f_num_layers; p->f_cnum = c->f_cnum; p->f_hmask = c->f_use_hodge_mask;
    int fch = c->f_cnum;
    bool narrow = true;        // every layer width <= 8
    for (int l = 0; l < p->f_L; ++l) {
        int cin, cout;
        ccsd_stack_io(l, p->f_L, c->f_cnum, c->f_c_hid, c->f_c_final, &cin, &cout);
        const MlpD& m = p->fl[l] = pb.mlp(c->f_num_linears, cin, c->f_nhid, cout);
        if (cin > CCSD_FWMAX || cout > CCSD_FWMAX || c->f_nhid > CCSD_FWMAX) return pb.reject(CCSD_ERR_UNSUPPORTED, "ScoreNetworkF layer wider than 32");
        narrow = narrow && m.in <= 8 && m.out <= 8 && (m.n == 1 || m.hid <= 8);
        fch += cout;
    }
    p->f_fdim = c->f_c_hid * (p->f_L - 1) + c->f_c_final + c->f_cnum;
    if (p->f_fdim != fch) return pb.reject(CCSD_ERR_INVALID, "ScoreNetworkF channel count inconsistent");
    p->f_fin = pb.mlp(c->f_num_layers_mlp, p->f_fdim, 2 * p->f_fdim, 1);
    if (p->f_fdim > CCSD_FWMAX || (c->f_num_layers_mlp > 1 && 2 * p->f_fdim > CCSD_FWMAX))
        return pb.reject(CCSD_ERR_UNSUPPORTED, "ScoreNetworkF final MLP wider than 32");
    p->f_affine = (c->f_num_linears == 1 && c->f_num_layers_mlp == 1) ? 1 : 0;
    // the general (non-affine) path with every layer width <= 8 and a single-Linear head: zero-padded [8][8] + [8] blocks (CCSD_HWBLK
    // floats per Linear) and the head's weights in 8-wide segments, appended to the device copy of the blob (ccsd_pack_fnet_blocks)
    if (!p->f_affine && p->f_fin.n == 1 && p->f_cnum <= 8 && narrow) p->f_blk = (pb.cur + 15) & ~15;
    return true;
}

// A plan k_xa has no code for (`need`: why) takes the tiled route, or fails with the reason the route does not serve it either.
// No k_xa layout: the plan's LDS fields stay zero.
static inline void plan_route_only(PlanD* p, PlanBuilder& pb, const char* lg_reason, const char* need) {
    if (lg_reason) { pb.fail(CCSD_ERR_UNSUPPORTED, std::string(need) + " the tiled graph-network route, which does not serve " + lg_reason); return; }
    pb.lg = 1;
    pb.route_copies(*p);
    p->ldn = round_ld(p->N);
    p->chan_rows = p->a_fdim;
}

// ---- k_xa's LDS layout.  What it needs to know of the networks: maxima over the AttentionLayers of both stacks, the hodge branch's scratch
struct XaNeeds {
    int fmaxA;                    // widest node-feature row
    int colmax, mchid, cinmax;    // Q | K | V columns, multi_channel's hidden width, input channels of a layer
    int pw_pair, pw_fin;          // widest hidden activation of the per-layer edge MLPs / of the final MLP
    bool pair_chained, fin_chained;   // ... which stay in registers when every such MLP is chained
    int hq_floats, h1m_floats;    // hodge branch: Q | K scratch, dense buffer of a layer that feeds another
    int hw_n;                     // ... most Linears of a mlp_attention
};
static inline XaNeeds xa_needs(const ccsd_config_t* c, const PlanD& p) {
    XaNeeds n = {};
    n.fmaxA = p.F > c->a_nhid ? p.F : c->a_nhid;
    n.pw_pair = 1; n.pair_chained = true;
    auto layer_max = [&](const AttnLayerD& a) {
        const int cols = 2 * a.adim + a.fout;
        if (cols > n.colmax) n.colmax = cols;
        if (a.mc.hid > n.mchid) n.mchid = a.mc.hid;
        if (a.cin > n.cinmax) n.cinmax = a.cin;
        if (a.mlp.n > 1 && a.mlp.hid > n.pw_pair) n.pw_pair = a.mlp.hid;
        n.pair_chained = n.pair_chained && a.mlp.chain != 0;
    };
    for (int l = 0; l < p.a_L; ++l) layer_max(p.al[l]);
    if (p.x_gmh) {
        for (int l = 0; l < p.x_depth; ++l) layer_max(p.gl[l]);
        if (c->x_nhid > n.fmaxA) n.fmaxA = c->x_nhid;
    }
    n.pw_fin = 2 * p.a_fdim;
    n.fin_chained = p.a_fin.chain != 0;
    n.hw_n = 1;
    for (int l = 0; l < p.h_L; ++l) {
        const HodgeLayerD& h = ccsd_hl(p, l);
        // (+1: the first layer's rows have an odd stride in k_xa -- bank-conflict-free reads in the dense pair loop)
        const int hq = h.cin * p.E * (2 * h.adim + (l == 0 ? 1 : 0)), h1m = l + 1 < p.h_L ? h.cout * p.E * p.E : 0;
        if (hq > n.hq_floats) n.hq_floats = hq;
        if (h1m > n.h1m_floats) n.h1m_floats = h1m;
        if (h.matt.n > n.hw_n) n.hw_n = h.matt.n;
    }
    return n;
}
static inline int xa_chunk_ld(int rows) { int r = (rows + 15) / 16 * 16; if (r % 32 == 0) r += 8; return r; }   // 2-way conflicts at worst
static inline int xa_carve(int& o, int v) { const int r = o; o += (v + 3) / 4 * 4; return r; }                // regions start on 16 bytes

// ... the hodge branch's regions, carved at o behind the attention stack's (o_att .. o_xnext up to o_xnext_end, then o_vcat).  The branch
// runs after the stack, whose regions are dead by then.  Returns the floats one row of HodgeBaselineLayer 0's chunk needs in the shared region
static inline int xa_layout_hodge(const XaNeeds& n, PlanD* q, int o_xnext_end, int& o) {
    const int E = q->E;
    auto carve = [&](int v) { return xa_carve(o, v); };
    // degree scratch of the dense hodge layers, three cases: (1) multi_channel's hidden layer; (2) two layers: a slot of its own when
    // layer 1's degrees do not fit there, or when the Q | K scratch reaches into it; (3) more than two: always its own, for the largest
    q->o_deg = q->o_vcat;
    if (q->h_L) {
        // the Q | K scratch re-uses [attention | node features | multi_channel hidden] when it fits
        const int deg1 = q->h_L > 1 ? q->hl[1].cin * E : 0;
        if (n.hq_floats <= o - q->o_att) {
            q->o_hq = q->o_att;
            if (q->h_L > 1 && (n.hq_floats > o_xnext_end - q->o_att || deg1 > n.mchid * q->ldn)) q->o_deg = carve(deg1);
        } else {
            q->o_hq = carve(n.hq_floats);
            if (q->h_L > 1 && deg1 > n.mchid * q->ldn) q->o_deg = carve(deg1);
        }
        q->o_hd = carve(q->a_nch_hodge * E + (q->h_L > 1 ? 2 * E : 0));   // + [s fl | b fl] of P_1's composition (k_xa)
        q->o_hw = carve((q->h_L > 2 ? q->h_L : 2) * n.hw_n * 72);
        q->hw_stride = n.hw_n * 72;
        if (q->h_L > 2) {
            int degmax = 0, wcmax = 0;
            for (int l = 1; l < q->h_L; ++l) {
                if (ccsd_hl(*q, l).cin * E > degmax) degmax = ccsd_hl(*q, l).cin * E;
                if (ccsd_hl(*q, l).wc > wcmax) wcmax = ccsd_hl(*q, l).wc;
            }
            q->o_deg = carve(degmax);
            q->o_h2m = carve(n.h1m_floats);
            q->o_hM = carve((q->h_L - 2) * E * E);
            q->o_hX = carve(2 * E * wcmax);
        }
    }
    if (!q->hb_L) return 0;
    // HodgeBaselineLayers: layer 0's hidden rows re-use the same regions when they fit
    const int g = q->hb[0].cin * E * q->hb[0].hid;
    q->o_hbg = (g <= o - q->o_att) ? q->o_att : carve(g);
    q->o_hbd = carve(q->hb_L > 1 ? q->hb[1].cin * E : 4);
    q->o_hbw = carve(2 * CCSD_MAXLIN * (CCSD_FW * CCSD_FW + CCSD_FW));
    q->o_hd = carve(q->a_nch_hodge * E);
    // per row of the chunk: the symmetrised block outputs (mlp_hodge's input), layer 0's output, the next layer's hidden row
    return q->hb_L > 1 ? q->hb[0].cin * E + q->hb[0].cout * (E + q->hb[1].hid) : 0;
}

// The layout (float offsets) of ONE candidate: `budget` floats of LDS, the channel stack [chan_rows][N*N] in LDS (gch = 0) or in the HBM
// workspace (1), attention channels in groups of cg.  Writes the regions into *q, a copy of the plan, and returns whether they fit the
// budget; cg, the chunk sizes, the shared region and xa_lds_floats are written only when they do.  Every aliasing rule k_xa relies on is here or in xa_layout_hodge.
static inline bool xa_layout(const XaNeeds& n, int budget, int gch, int cg, PlanD* q) {
    const int N = q->N, F = q->F, E = q->E, NN = N * N, NNpad = (NN + 15) / 16 * 16;
    int o = 0;
    auto carve = [&](int v) { return xa_carve(o, v); };
    q->chan_global = gch;
    q->o_flags = carve(N);
    q->o_x = carve(N * F);
    q->o_adj = carve(NN);
    q->o_an = carve(gch ? n.cinmax * N : cg * N > N ? cg * N : N);      // D^-1/2 per channel of the group (HBM stack: of the layer)
    q->o_edge = carve(E);
    const int phase0 = o;
    q->o_xcat = carve(q->x_fdim * q->ldn);                              // X-network phase ...
    // hidden activations of the head: in registers when it is chained (then h1 only receives the F outputs)
    q->o_h1 = carve(q->x_fin.chain ? (F > 4 ? F : 4) * q->ldn : 2 * q->x_fdim * q->ldn);
    q->o_h2 = carve(q->x_fin.chain ? 4 : 2 * q->x_fdim * q->ldn);
    const int xphase_end = o;
    q->x_lds_floats = xphase_end + 64;                                  // (an X-network-only launch; GMH: the whole layout, below)
    // ... aliased by the A-network phase -- unless ScoreNetworkX is GMH, which runs the attention-stack machinery itself: its regions stay clear
    if (!q->x_gmh) o = phase0;
    q->o_chan = gch ? 0 : carve(q->chan_rows * NN);
    q->o_att = carve(n.cinmax * NN);                                    // attention of every input channel
    q->o_xcur = carve(n.fmaxA * q->ldn);
    q->o_xnext = carve(n.fmaxA * q->ldn);
    const int o_after_xnext = o;
    q->o_vcat = carve(n.mchid * q->ldn);                                // hidden layer of multi_channel
    const int hb_rmin = xa_layout_hodge(n, q, o_after_xnext, o);
    if (xphase_end > o) o = xphase_end;
    // shared region R: GCN scratch of a channel group | hidden activations of the MLPs | dense hodge layer
    // [channel][node][Q | K | V] of a group (the GCN's x W intermediate lives in registers)
    int rmin = cg * N * n.colmax;
    if (N * q->x_nhid > rmin) rmin = N * q->x_nhid;
    if (n.h1m_floats > rmin) rmin = n.h1m_floats;
    if (NN > rmin) rmin = NN;                                           // raw output of the chained final MLP
    if (hb_rmin > rmin) rmin = hb_rmin;
    if (o + rmin > budget) return false;
    if (!n.fin_chained && o + 2 * n.pw_fin * 16 > budget) return false;
    // within the budget the largest chunks of pairs for the MLPs that are not chained
    int pch = 16, pchp = 16;
    while (!n.fin_chained && pch + 16 <= NNpad && o + 2 * n.pw_fin * xa_chunk_ld(pch + 16) <= budget) pch += 16;
    while (!n.pair_chained && pchp + 16 <= NNpad && o + 2 * n.pw_pair * xa_chunk_ld(pchp + 16) <= budget) pchp += 16;
    int r = rmin > 64 ? rmin : 64;
    if (!n.fin_chained && 2 * n.pw_fin * xa_chunk_ld(pch) > r) r = 2 * n.pw_fin * xa_chunk_ld(pch);
    if (!n.pair_chained && 2 * n.pw_pair * xa_chunk_ld(pchp) > r) r = 2 * n.pw_pair * xa_chunk_ld(pchp);
    q->cg = cg; q->pch = pch; q->ldp = xa_chunk_ld(pch); q->pchp = pchp; q->ldpp = xa_chunk_ld(pchp);
    q->o_c0 = carve(r);
    q->o_red = q->o_c0;                                                 // block reductions run when R is idle
    if (hb_rmin) { q->hb_rows = r / hb_rmin; if (q->hb_rows > E) q->hb_rows = E; }
    q->xa_lds_floats = o;
    if (q->x_gmh) q->x_lds_floats = o;
    return true;
}

// Searches k_xa's layout and settles the route where there is none.  Candidate LDS budgets: what leaves 4, 3, 2 workgroups and 1 on a CU
// (32 waves/CU hide the latency of the ~45 barrier-separated phases best).  The search starts at the budget that keeps
// ceil(batch / #CUs) workgroups co-resident per CU (batch_hint; unknown = 4 per CU, the qm9_CC B = 1024 case; CCSD_XA_PASS=<n> starts at
// candidate n) and grows.  Within a budget the channel stack in LDS is tried before the stack in the HBM workspace (L2-resident, one slab
// per graph -- large graphs, zinc250k: 46 channels x 38 x 38 = 266 KB; CCSD_XA_GCH=1 tries only that): with the residency the batch needs,
// more workgroups per CU buy nothing and the HBM stack costs.  Within either, the largest channel group first.  The first fit is taken.
#define CCSD_XA_NCAND 4
static const int CCSD_XA_BUDGETS[CCSD_XA_NCAND] = {40960, 53 * 1024, 79 * 1024, 152 * 1024};   // bytes
static inline void plan_xa_layout(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb, const char* lg_reason) {
    const int N = p->N, F = p->F;
    const XaNeeds n = xa_needs(c, *p);
    p->ldn = round_ld(N);
    p->chan_rows = p->a_fdim > p->g_nch ? p->a_fdim : p->g_nch;
    p->pw_pair = n.pw_pair;
    int need = c->batch_hint > 0 ? (c->batch_hint + 255) / 256 : 4;
    need = need < 1 ? 1 : need > 4 ? 4 : need;
    PlanD q = *p;
    bool fits = false;
    for (int pass = pb.xa_pass >= 0 ? pb.xa_pass : 4 - need; pass < CCSD_XA_NCAND && !fits; ++pass)
        for (int gch = pb.xa_gch; gch < 2 && !fits; ++gch)
            for (int cg = n.cinmax; cg >= 1 && !fits; --cg) {
                q = *p;
                fits = xa_layout(n, CCSD_XA_BUDGETS[pass] / 4, gch, cg, &q);
            }
    // (a plan no candidate fits keeps the regions of the last one tried, as it always did: chan_global still sizes its workspace)
    *p = q;
    int total = fits ? p->xa_lds_floats : -1;
    // ScoreNetworkX late (k_xa): one wave runs it in stages inside the A-network's MLP-chain intervals, where that wave has
    // no tile.  Needs: the plain networks, chained MLPs, two AttentionLayers, at most three 16-pair tiles (E <= 48), node
    // tiles of 16, and room for its own [x_fdim + max(F, 4)][ldn] + 16 floats inside the budget the layout already fits.
    if (fits && !p->x_gmh && !p->hb_L && !p->chan_global && p->x_fin.chain && p->a_fin.chain && p->a_L >= 2 && N <= 16 && p->E <= 48 &&
        p->al[0].mlp.chain && p->al[1].mlp.chain) {
        const int lx = (p->x_fdim + (F > 4 ? F : 4)) * p->ldn + 16;
        int cap = 160 * 1024 / 4;
        for (int b = CCSD_XA_NCAND - 1; b >= 0; --b) if (total * 4 <= CCSD_XA_BUDGETS[b]) cap = CCSD_XA_BUDGETS[b] / 4;
        if (total + lx <= cap) { p->x_late = 1; p->o_lx = total; total += lx; p->xa_lds_floats = total; }
    }
    if (pb.verbose)
        fprintf(stderr, "[ccsd] k_xa LDS %d B (cg=%d pch=%d/%d pchp=%d/%d, channel stack in %s)\n", total * 4, p->cg, p->pch, p->ldp, p->pchp, p->ldpp,
                p->chan_global ? "HBM" : "LDS");
    if (!fits || (size_t)total * 4 > 160 * 1024) {
        if (!lg_reason) pb.lg = 1;         // no k_xa layout: the tiled route serves the plan
        else pb.fail(CCSD_ERR_UNSUPPORTED, std::string("graph-network working set exceeds the 160 KB LDS of a CU, and the tiled graph-network route does not serve ") + lg_reason);
    }
}

// The route: the tiled graph-network kernels (ccsd_k_lg.h) when k_xa cannot place the plan or when forced; k_xa's layout otherwise
static inline void plan_route(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    const char* lg_reason = ccsd_lg_ineligible(c, p, pb.h_wide);
    // above 64 nodes k_xa's working set leaves one CU's LDS; its hodge branch is written for one or two HodgeBaselineLayers; its (and k_r2's)
    // per-thread small_mlp is 8 wide
    const char* need = c->N > CCSD_XA_MAXN ? "N > 64 needs" : p->hb_L > CCSD_MAXHL ? "more than 2 HodgeBaselineLayers need" :
                       pb.h_wide ? "hodge MLPs wider than 8 need" : nullptr;
    if (need) { plan_route_only(p, pb, lg_reason, need); return; }
    // A dense HodgeBaselineLayer beyond E = 255 -- the envelope k_xa's dense hodge layers are built and tested in (ccsd_plan_create
    // holds ScoreNetworkA_CC stacks to it; every shipped Base_CC geometry lies inside: E = 36 .. 190) -- takes the route where it is
    // eligible: one workgroup per complex would walk the E^2 pairs alone (grid_small_Base_CC: E = 1176, a 148 KB k_xa layout).  So does
    // a ScoreNetworkA_CC stack of two or more layers there: k_xa's pair table of the dense layer holds edge indices in bytes
    if ((p->hb_L > 1 || p->h_L > 1) && p->E > 255 && !lg_reason) pb.lg = 1;
    // (1 leaves combinatorial complexes on k_xa, as before the route served any of them: tests/golden/route_plans.json pins those plans)
    if (pb.lg_force && !lg_reason && (!c->is_cc || pb.lg_force >= 2)) pb.lg = 1;
    plan_xa_layout(c, p, pb, lg_reason);
    if (pb.lg) pb.route_copies(*p);
}

// Fills `p` (except the affine fold, which needs the weights) and pb's outputs; returns the blob size (0 where pb holds a failure).
static inline size_t ccsd_build_plan(const ccsd_config_t* c, PlanD* p, PlanBuilder& pb) {
    memset(p, 0, sizeof(*p));
    if (!plan_geometry(c, p, pb) || !plan_xnet(c, p, pb) || !plan_anet_graph(c, p, pb) || !plan_anet_hodge(c, p, pb) || !plan_fnet(c, p, pb)) return 0;
    const size_t nweights = (size_t)pb.cur;         // (the route reserves packed copies only)
    plan_route(c, p, pb);
    pb.npacked = (size_t)pb.pcur;
    return pb.status == CCSD_OK ? nweights : 0;
}

// ScoreNetworkF block layout behind the weight blob (PlanD::f_blk): Linear q of layer l at (l * CCSD_MAXLIN + q) * 72
// ([8][8] weights, row = output, + [8] biases); then the head: (CCSD_MAXFL + 1) segments of 8 weights (segment 0: the cnum
// input channels, segment l + 1: the outputs of layer l) + 8 floats whose first is the bias.
#define CCSD_FBLK_HEAD (CCSD_MAXFL * CCSD_MAXLIN * 72)
#define CCSD_FBLK_FLOATS (CCSD_FBLK_HEAD + (CCSD_MAXFL + 1) * 8 + 8)
static inline void ccsd_pack_fnet_blocks(const PlanD* p, const float* w, float* dst) {
    for (int i = 0; i < CCSD_FBLK_FLOATS; ++i) dst[i] = 0.f;
    int co0 = p->f_cnum;
    for (int i = 0; i < p->f_cnum; ++i) dst[CCSD_FBLK_HEAD + i] = w[p->f_fin.w[0] + i];
    for (int l = 0; l < p->f_L; ++l) {
        const MlpD& m = p->fl[l];
        for (int q = 0; q < m.n; ++q) {
            float* blk = dst + (l * CCSD_MAXLIN + q) * 72;
            const int ni = mlp_in(m, q), no = mlp_out(m, q);
            for (int o = 0; o < no; ++o) {
                for (int i = 0; i < ni; ++i) blk[o * 8 + i] = w[m.w[q] + o * ni + i];
                blk[64 + o] = w[m.b[q] + o];
            }
        }
        for (int i = 0; i < m.out; ++i) dst[CCSD_FBLK_HEAD + (l + 1) * 8 + i] = w[p->f_fin.w[0] + co0 + i];
        co0 += m.out;
    }
    dst[CCSD_FBLK_HEAD + (CCSD_MAXFL + 1) * 8] = w[p->f_fin.b[0]];
}

// Fold ScoreNetworkF into  score = mask * (alpha*F + beta*(H F) + gamma)  when every MLP in it is a
// single Linear (num_linears == 1 and num_layers_mlp == 1: true for every shipped CC checkpoint but
// ENZYMES).  The intermediate mask_rank2 factors are 0/1 and the final output is masked again, so
// the fold is exact in real arithmetic.
static inline void ccsd_fold_fnet(PlanD* p, const float* w) {
    if (!p->is_cc || !p->f_affine) return;
    const int fd = p->f_fdim, cn = p->f_cnum, nb = cn + 1;
    std::vector<double> A((size_t)fd * nb, 0.0);  // channel j = sum_i A[j][i] * H^i F  (i < cnum)  + A[j][cnum]
    for (int j = 0; j < cn; ++j) A[(size_t)j * nb + j] = 1.0;
    int ci0 = 0, co0 = cn;
    for (int l = 0; l < p->f_L; ++l) {
        const MlpD& m = p->fl[l];
        for (int oo = 0; oo < m.out; ++oo) {
            std::vector<double> acc(nb, 0.0);
            acc[cn] = (double)w[m.b[0] + oo];
            for (int i = 0; i < m.in; ++i)
                for (int t = 0; t < nb; ++t) acc[t] += (double)w[m.w[0] + oo * m.in + i] * A[(size_t)(ci0 + i) * nb + t];
            for (int t = 0; t < nb; ++t) A[(size_t)(co0 + oo) * nb + t] = acc[t];
        }
        ci0 = co0; co0 += m.out;
    }
    std::vector<double> r(nb, 0.0);
    r[cn] = (double)w[p->f_fin.b[0]];
    for (int j = 0; j < fd; ++j)
        for (int t = 0; t < nb; ++t) r[t] += (double)w[p->f_fin.w[0] + j] * A[(size_t)j * nb + t];
    p->f_alpha = (float)r[0]; p->f_beta = cn > 1 ? (float)r[1] : 0.f; p->f_gamma = (float)r[cn];
    for (int j = 0; j < CCSD_MAXCN; ++j) p->f_betas[j] = (j >= 1 && j < cn) ? (float)r[j] : 0.f;
}
#endif  // CCSD_DEVICE_ONLY
