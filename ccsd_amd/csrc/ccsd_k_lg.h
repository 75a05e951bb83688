// ccsd_k_lg.h -- the tiled graph-network path (k_lg_*): ScoreNetworkX + ScoreNetworkA for plans whose per-graph working set does not
// fit one CU's LDS (graph-only plans with N > 64, or k_xa's layout fails; CCSD_LARGE_GRAPH=1 forces it for any eligible graph-only
// plan), and for combinatorial complexes (N <= 64) without a k_xa layout (or under CCSD_LARGE_GRAPH=2, which forces every eligible
// plan): ScoreNetworkA_CC with 1 to 8 HodgeAdjAttentionLayers (two or more: E <= CCSD_LG_HD_MAXE, and always here beyond E = 255), and
// ScoreNetworkA_Base_CC with 1 to 8 HodgeBaselineLayers (more than two: always here).  ScoreNetworkA_CC plans whose hodge MLPs have a Linear
// wider than 8 (up to 16) are always here.
// Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// State lives in the HBM workspace (carve_ws, LgWs in ccsd_api.h) and every phase is a launch of its own that tiles each graph over
// many workgroups.  The decomposition of one forward (launch_lg):
//   ScoreNetworkX   k_lg_dis (D^-1/2 of adjX) ; per GCN layer: k_lg_xw (Y = D^-1/2 X W), k_lg_gcn (tanh(D^-1/2 A' Y + b) into the
//                   concatenation) ; k_lg_nmlp (final MLP per node, mask_x)
//   ScoreNetworkA   k_lg_pow (channel stack [A, A^2, ...]) ; ScoreNetworkA_CC, one hodge layer: k_lg_hodge1 (the hodge channels, behind the
//                   graph channels of the stack) ; two or more: k_lg_hd_qk0, per layer but the last k_lg_hd_dense + k_lg_hd_dis +
//                   k_lg_hd_conv, k_lg_hd_diag (the dense E x E layers tiled through the workspace; hodge MLPs wider than 8: k_lg_hodge1_w /
//                   k_lg_hd_diag_w, mlp_attention on the diagonal through the MFMA chain too) ; ScoreNetworkA_Base_CC: k_lg_hb_in, per layer but the last k_lg_hb_dense + k_lg_hb_hid,
//                   k_lg_hb_diag (the same channels from the HodgeBaselineLayers) ; per AttentionLayer: k_lg_dis, k_lg_xw (Q | K | V columns side by side),
//                   k_lg_gcn, k_lg_nmlp (multi_channel, mask_x, tanh), k_lg_att (head-mean tanh(Q K^T / sqrt(fout)), symmetrised),
//                   k_lg_edge (edge MLP on [att_c | adj_c] per entry, MFMA: mlp_chain_tile), k_lg_sym (out + out^T, mask_adjs) ;
//                   k_lg_fin (final MLP per entry, MFMA: mlp_chain_tile, + the adjacency epilogue, per-tile norm partials)
//   k_lg_epi        the node-feature epilogue and the per-sample norm reduction (fixed order, no atomics)
// Reference: attention.py:84-132, 270-304 (AttentionLayer), ScoreNetwork_A.py:505-541, ScoreNetwork_X.py:102-132, layers.py:134-158
// (DenseGCNConv, add_loop: the diagonal is SET to 1).  The oracle (oracle/ccsd_oracle.py: dense_gcn, attention, attention_layer,
// score_network_a, score_network_x) is the specification.
//
// Build: the definitions are compiled in ccsd_lg.hip (CCSD_LG_UNIT; k_lg_fin_w in ccsd_lgw.hip) and in the host emulation; ccsd_hip.hip sees the declarations.
// Every per-graph base is a 64-bit offset; offsets inside one graph stay below fdim * N^2 < 2^31 for N <= CCSD_LG_MAXN.
#pragma once
#include "ccsd_dev.h"
#include "ccsd_rank2_common.h"
#include "ccsd_k_xa.h"          // XaArgs

#define CCSD_LG_TB 256          // threads per workgroup of every k_lg_* kernel (CCSD_NTHREADS on the GPU)
#define CCSD_LG_FIN_ROWS 64     // entries per workgroup of k_lg_edge / k_lg_fin: one 16-entry MFMA tile per wave
#define CCSD_LG_GT 32           // k_lg_gcn output tile (rows x columns) and k-chunk
#define CCSD_LG_AT 16           // k_lg_att node tile
#define CCSD_LG_MAXAD 64        // widest attention dimension of the route (k_lg_att stages Q | K of two node tiles in LDS)

// node-MLP input gather (k_lg_nmlp): feature k of node i of sample b = src[b * bs + (k / per) * cs + i * rs + off + k % per]
struct LgGather {
    const float* src;
    long long bs;
    int cs, rs, off, per;
};

__global__ void k_lg_put(const float* __restrict__ src, int F, float* __restrict__ dst, int ldd, int rows);
__global__ void k_lg_pow(const float* __restrict__ adj, float* __restrict__ S, long long sstride, int N, int c);
__global__ void k_lg_hodge1(HodgeLayerD h, float rks, const float* __restrict__ w, const unsigned char* __restrict__ edges,
                            const float* __restrict__ P0, float* __restrict__ S, long long sstride, int ch0, int N, int E,
                            const float* __restrict__ flags);
// per-edge factors of P_1 = fl (s Q_1 + b u_1) when k_r2 delivered the raw Q_1, u_1 (XaArgs::p1_raw; k_xa's hodge_early): k_lg_hd_dis writes
// pc[b][0][e] = fl s[e], pc[b][1][e] = fl b, s = sum_c w_c a_c[e] over the first layer's linear mlp_value (pc == nullptr: nothing to do)
struct LgHdRaw {
    const float *w, *S, *flags;
    const unsigned char* edges;
    float* pc;
    long long sstride;
    int N, cin0, mw, mb;
};
__global__ void k_lg_hd_qk0(HodgeLayerD h, int nch, const float* __restrict__ w, const unsigned char* __restrict__ edges, const float* __restrict__ P0,
                            float* __restrict__ S, long long sstride, int ch0, int N, int E, float* __restrict__ QK, long long qstride);
__global__ void k_lg_hd_dense(HodgeLayerD h, MlpD matt, float rks, const float* __restrict__ wp, const unsigned char* __restrict__ edges,
                              const float* __restrict__ QK, long long qstride, float* __restrict__ Hout, long long hstride, float* __restrict__ S,
                              long long sstride, int ch0, int N, int E, const float* __restrict__ flags);
__global__ void k_lg_hd_dis(const float* __restrict__ Hin, long long hstride, int cin, int E, float* __restrict__ dis, LgHdRaw raw);
__global__ void k_lg_hd_conv(HodgeLayerD h, const float* __restrict__ w, const float* __restrict__ Hin, long long hstride, const float* __restrict__ dis,
                             const float* __restrict__ P, int ldp, const float* __restrict__ pc, const float* __restrict__ U, int E,
                             float* __restrict__ QK, long long qstride);
__global__ void k_lg_hd_diag(HodgeLayerD h, float rks, const float* __restrict__ w, const unsigned char* __restrict__ edges, const float* __restrict__ QK,
                             long long qstride, float* __restrict__ S, long long sstride, int ch0, int N, int E, const float* __restrict__ flags);
// ... of plans with hodge MLPs wider than 8 (Route::h_wide): mlp_attention on the diagonal through the MFMA chain, matt = PlanBuilder::hdm's copy
__global__ void k_lg_hodge1_w(HodgeLayerD h, MlpD matt, float rks, const float* __restrict__ w, const float* __restrict__ wp,
                              const unsigned char* __restrict__ edges, const float* __restrict__ P0, float* __restrict__ S, long long sstride, int ch0,
                              int N, int E, const float* __restrict__ flags);
__global__ void k_lg_hd_diag_w(HodgeLayerD h, MlpD matt, float rks, const float* __restrict__ wp, const unsigned char* __restrict__ edges,
                               const float* __restrict__ QK, long long qstride, float* __restrict__ S, long long sstride, int ch0, int N, int E,
                               const float* __restrict__ flags);
__global__ void k_lg_hb_in(HodgeBaseD h, int nch, const float* __restrict__ w, const unsigned char* __restrict__ edges, float* __restrict__ S,
                           long long sstride, int ch0, int N, int E, float* __restrict__ G, long long gstride);
__global__ void k_lg_hb_dense(HodgeBaseD h, const float* __restrict__ w, const float* __restrict__ wp, const unsigned char* __restrict__ edges,
                              const float* __restrict__ G, long long gstride, float* __restrict__ Hout, long long hstride, float* __restrict__ S,
                              long long sstride, int ch0, int N, int E, const float* __restrict__ flags);
__global__ void k_lg_hb_hid(HodgeBaseD h, const float* __restrict__ w, const float* __restrict__ wp, const float* __restrict__ Hin, long long hstride,
                            int E, float* __restrict__ G, long long gstride);
__global__ void k_lg_hb_diag(HodgeBaseD h, const float* __restrict__ w, const unsigned char* __restrict__ edges, const float* __restrict__ G,
                             long long gstride, float* __restrict__ S, long long sstride, int ch0, int N, int E, const float* __restrict__ flags);
__global__ void k_lg_dis(const float* __restrict__ S, long long sstride, int ci0, int cin, int N, float* __restrict__ dis);
__global__ void k_lg_xw(const float* __restrict__ X, long long xbs, int ldx, int fin, const float* __restrict__ W, int wcs, int ldy,
                        int cin, int N, const float* __restrict__ dis, float* __restrict__ Y);
__global__ void k_lg_gcn(const float* __restrict__ S, long long sstride, int ci0, const float* __restrict__ Y, const float* __restrict__ dis,
                         const float* __restrict__ bias, int bcs, int ldy, int cols, int cin, int N, float* __restrict__ out, long long obs,
                         int ocs, int ldo, int ooff, int act_tanh);
__global__ void k_lg_nmlp(MlpD m, const float* __restrict__ w, LgGather g, int N, const float* __restrict__ flags, int act_tanh,
                          float* __restrict__ out);
__global__ void k_lg_att(const float* __restrict__ QKV, int ldy, int adim, int nchunk, int dsplit, float rscale, float ratt, int cin, int N,
                         float* __restrict__ att);
__global__ void k_lg_edge(MlpD m, const float* __restrict__ wp, const float* __restrict__ att, float* __restrict__ S, long long sstride,
                          int ci0, int co0, int cin, int N);
__global__ void k_lg_sym(float* __restrict__ S, long long sstride, int co0, int cout, int N, const float* __restrict__ flags);
__global__ void k_lg_fin(MlpD m, const float* __restrict__ wp, const float* __restrict__ S, long long sstride, int N,
                         const float* __restrict__ flags, const float* __restrict__ adj, XaArgs xa, NoiseArgs na, float* __restrict__ part);
__global__ void k_lg_fin_w(MlpD m, const float* __restrict__ wp, const float* __restrict__ S, long long sstride, int N,
                           const float* __restrict__ flags, const float* __restrict__ adj, XaArgs xa, NoiseArgs na, float* __restrict__ part);
__global__ void k_lg_epi(const float* __restrict__ xnet, const float* __restrict__ x, const float* __restrict__ flags, XaArgs xa,
                         NoiseArgs na, const float* __restrict__ part, int ntiles, int N, int F);

// k_lg_hb_dense's LDS (floats / bytes): the hidden rows and the W2 rows of the tile's 16 + 16 edges per channel (odd row stride: the 16
// lanes along an edge index read 16 banks), their b2, and mlp_hodge's input [cin][256 pairs]
static inline __host__ __device__ int lg_hb_row_ld(int hid) { return hid | 1; }
static inline size_t lg_hb_dense_lds(const HodgeBaseD& h) { return ((size_t)4 * h.cin * 16 * lg_hb_row_ld(h.hid) + 32 * h.cin + 256 * h.cin) * 4; }
// k_lg_hd_dense's: the Q | K rows of the tile's 16 + 16 edges per channel (the same odd row stride) and mlp_attention's input [cin][256 pairs]
static inline size_t lg_hd_dense_lds(const HodgeLayerD& h) { return ((size_t)2 * h.cin * 16 * lg_hb_row_ld(2 * h.adim) + 256 * h.cin) * 4; }

#if defined(CCSD_LG_UNIT) || defined(CCSD_EMU)
// per-thread work items of a CCSD_LG_TB-sized tile: one per thread on the GPU, the whole tile in the emulation's one thread
#define LG_PT(tile) ((tile) / CCSD_NTHREADS)

// dst[r][0 .. F) = src[r][0 .. F) for the B * N node rows (ScoreNetworkX: x heads the concatenation of the layer outputs)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_put(const float* __restrict__ src, int F, float* __restrict__ dst, int ldd, int rows) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < (long long)rows * F; t += (long long)gridDim.x * blockDim.x) {
        const long long r = t / F;
        dst[r * ldd + (t - r * F)] = src[t];
    }
}

// S[b][c] = c == 0 ? adj[b] : S[b][c - 1] . adj[b]      (pow_tensor, graph_utils.py:285-292)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_pow(const float* __restrict__ adj, float* __restrict__ S, long long sstride, int N, int c) {
    const int b = blockIdx.y, NN = N * N;
    const float* A = adj + (size_t)b * NN;
    float* dst = S + (size_t)b * sstride + (size_t)c * NN;
    const float* prev = dst - NN;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < NN; t += gridDim.x * blockDim.x) {
        if (c == 0) { dst[t] = A[t]; continue; }
        const int i = t / N, j = t - i * N;
        const float* pr = prev + (size_t)i * N;
        float acc = 0.f;
        for (int k = 0; k < N; ++k) acc = fmaf(pr[k], A[(size_t)k * N + j], acc);
        dst[t] = acc;
    }
}

// dis[b][c][i] = rsqrt(max(1, rowsum(A'_c)[i])), A'_c = channel ci0 + c with its diagonal set to 1 (dense_gcn: add_loop)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_dis(const float* __restrict__ S, long long sstride, int ci0, int cin, int N, float* __restrict__ dis) {
    const int b = blockIdx.y, NN = N * N;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < cin * N; t += gridDim.x * blockDim.x) {
        const int c = t / N, i = t - c * N;
        const float* row = S + (size_t)b * sstride + (size_t)(ci0 + c) * NN + (size_t)i * N;
        float s = 0.f;
        for (int j = 0; j < N; ++j) s += j == i ? 1.f : row[j];
        dis[((size_t)b * cin + c) * N + i] = 1.0f / sqrtf(fmaxf(s, 1.f));
    }
}

// Y[b][c][i][col] = dis[b][c][i] * sum_k X[b][i][k] W_c[k][col]   (W_c = W + c * wcs, row stride ldy; zero-padded columns give zeros)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_xw(const float* __restrict__ X, long long xbs, int ldx, int fin, const float* __restrict__ W, int wcs,
                                                     int ldy, int cin, int N, const float* __restrict__ dis, float* __restrict__ Y) {
    const int b = blockIdx.y;
    const float* xb = X + (size_t)b * xbs;
    const int total = cin * N * ldy;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const int col = t % ldy, r = t / ldy, i = r % N, c = r / N;
        const float* xr = xb + (size_t)i * ldx;
        const float* wc = W + (size_t)c * wcs + col;
        float acc = 0.f;
        for (int k = 0; k < fin; ++k) acc = fmaf(xr[k], wc[(size_t)k * ldy], acc);
        Y[(size_t)b * total + t] = dis[((size_t)b * cin + c) * N + i] * acc;
    }
}

// out[b][c][i][ooff + col] = act(dis_i * sum_j A'_c[i][j] Y[b][c][j][col] + bias_c[col])    (the GCN's adjacency product, K = N)
// One CCSD_LG_GT x CCSD_LG_GT output tile per workgroup, A' and Y staged in LDS by k-chunks of CCSD_LG_GT.
// grid: (row tiles * column tiles, cin, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_gcn(const float* __restrict__ S, long long sstride, int ci0, const float* __restrict__ Y,
                                                      const float* __restrict__ dis, const float* __restrict__ bias, int bcs, int ldy, int cols,
                                                      int cin, int N, float* __restrict__ out, long long obs, int ocs, int ldo, int ooff,
                                                      int act_tanh) {
    constexpr int T = CCSD_LG_GT, PT = LG_PT(T * T);
    __shared__ float sA[T][T + 1];
    __shared__ float sY[T][T + 1];
    const int c = blockIdx.y, b = blockIdx.z, NN = N * N;
    const int ntc = (cols + T - 1) / T;
    const int i0 = (blockIdx.x / ntc) * T, c0 = (blockIdx.x % ntc) * T;
    const float* A = S + (size_t)b * sstride + (size_t)(ci0 + c) * NN;
    const float* Yc = Y + ((size_t)b * cin + c) * N * ldy;
    const int tid = threadIdx.x, nth = blockDim.x;
    float acc[PT];
    for (int u = 0; u < PT; ++u) acc[u] = 0.f;
    for (int j0 = 0; j0 < N; j0 += T) {
        for (int t = tid; t < T * T; t += nth) {
            const int r = t / T, q = t - r * T;
            const int i = i0 + r, j = j0 + q, jy = j0 + r, col = c0 + q;
            sA[r][q] = (i < N && j < N) ? (i == j ? 1.f : A[(size_t)i * N + j]) : 0.f;
            sY[r][q] = (jy < N && col < cols) ? Yc[(size_t)jy * ldy + col] : 0.f;
        }
        __syncthreads();
        for (int u = 0; u < PT; ++u) {
            const int t = tid + u * CCSD_NTHREADS, r = t / T, q = t - r * T;
            float a = acc[u];
            for (int k = 0; k < T; ++k) a = fmaf(sA[r][k], sY[k][q], a);
            acc[u] = a;
        }
        __syncthreads();
    }
    for (int u = 0; u < PT; ++u) {
        const int t = tid + u * CCSD_NTHREADS, r = t / T, q = t - r * T;
        const int i = i0 + r, col = c0 + q;
        if (i >= N || col >= cols) continue;
        float v = fmaf(dis[((size_t)b * cin + c) * N + i], acc[u], bias[(size_t)c * bcs + col]);
        if (act_tanh) v = tanh_f(v);
        out[(size_t)b * obs + (size_t)c * ocs + (size_t)i * ldo + ooff + col] = v;
    }
}

// A per-node MLP (layers.py:260-275, ELU between the linears) on 16 nodes per workgroup, activations in LDS:
// act_tanh = 1: out[b][i][o] = tanh(mask_x(mlp(.)))  (AttentionLayer's multi_channel, attention.py:292-293)
// act_tanh = 0: out[b][i][o] = mask_x(mlp(.))        (ScoreNetworkX's final MLP, ScoreNetwork_X.py:127-132)
// dynamic LDS: 16 * (m.in + 2 * max(hid, out)) floats.  grid: (ceil(N / 16), B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_nmlp(MlpD m, const float* __restrict__ w, LgGather g, int N, const float* __restrict__ flags,
                                                       int act_tanh, float* __restrict__ out) {
    CCSD_DYN_SMEM(sm);
    const int b = blockIdx.y, n0 = blockIdx.x * 16, tid = threadIdx.x, nth = blockDim.x;
    const int wmax = m.hid > m.out ? m.hid : m.out;
    float* h0 = sm;
    float* h1 = sm + 16 * (m.in > wmax ? m.in : wmax);
    const float* src = g.src + (size_t)b * g.bs;
    for (int t = tid; t < 16 * m.in; t += nth) {
        const int r = t / m.in, k = t - r * m.in, i = n0 + r;
        const int cc = k / g.per, o = k - cc * g.per;
        h0[t] = i < N ? src[(size_t)cc * g.cs + (size_t)i * g.rs + g.off + o] : 0.f;
    }
    __syncthreads();
    for (int l = 0; l < m.n; ++l) {
        const int in = mlp_in(m, l), on = mlp_out(m, l);
        const float* W = w + m.w[l];
        const float* bb = w + m.b[l];
        for (int t = tid; t < 16 * on; t += nth) {
            const int r = t / on, o = t - r * on;
            const float* xr = h0 + r * in;
            const float* wr = W + (size_t)o * in;
            float acc = 0.f;
            for (int k = 0; k < in; ++k) acc = fmaf(xr[k], wr[k], acc);
            acc += bb[o];
            h1[t] = l < m.n - 1 ? elu1(acc) : acc;
        }
        __syncthreads();
        float* tmp = h0; h0 = h1; h1 = tmp;
    }
    for (int t = tid; t < 16 * m.out; t += nth) {
        const int r = t / m.out, o = t - r * m.out, i = n0 + r;
        if (i >= N) continue;
        const float v = h0[t] * flags[(size_t)b * N + i];
        out[((size_t)b * N + i) * m.out + o] = act_tanh ? tanh_f(v) : v;
    }
}

// att[b][c][i][j] = (sum_h tanh(q_i^h . k_j^h * rscale) + sum_h tanh(q_j^h . k_i^h * rscale)) * 0.5 / heads
// (attention.py:111-130: head chunks, mean over heads, (A + A^T) / 2; the same expression as k_xa's).  Q | K are the first 2 adim
// columns of QKV [b][c][node][ldy].  One 16 x 16 tile of one channel per workgroup; grid: (tiles^2, cin, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_att(const float* __restrict__ QKV, int ldy, int adim, int nchunk, int dsplit, float rscale,
                                                      float ratt, int cin, int N, float* __restrict__ att) {
    constexpr int T = CCSD_LG_AT, PT = LG_PT(T * T);
    __shared__ float sI[T][2 * CCSD_LG_MAXAD + 1];
    __shared__ float sJ[T][2 * CCSD_LG_MAXAD + 1];
    const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, nth = blockDim.x;
    const int nt = (N + T - 1) / T, i0 = (blockIdx.x / nt) * T, j0 = (blockIdx.x % nt) * T;
    const float* Qc = QKV + ((size_t)b * cin + c) * N * ldy;
    const int w2 = 2 * adim;
    for (int t = tid; t < T * w2; t += nth) {
        const int r = t / w2, q = t - r * w2;
        sI[r][q] = i0 + r < N ? Qc[(size_t)(i0 + r) * ldy + q] : 0.f;
        sJ[r][q] = j0 + r < N ? Qc[(size_t)(j0 + r) * ldy + q] : 0.f;
    }
    __syncthreads();
    float* ab = att + ((size_t)b * cin + c) * N * N;
    for (int u = 0; u < PT; ++u) {
        const int t = tid + u * CCSD_NTHREADS, r = t / T, q = t - r * T;
        const int i = i0 + r, j = j0 + q;
        if (i >= N || j >= N) continue;
        const float s1 = attn_logits(&sI[r][0], &sJ[q][adim], nchunk, dsplit, rscale);
        const float s2 = attn_logits(&sJ[q][0], &sI[r][adim], nchunk, dsplit, rscale);
        ab[(size_t)i * N + j] = (s1 + s2) * ratt;
    }
}

// raw edge MLP (attention.py:295-300) of one AttentionLayer: S[b][co0 + o][i][j] = mlp([att_c(i, j) | adj_c(i, j)])_o, every ordered
// entry; k_lg_sym then forms out + out^T.  One 16-entry tile per wave (mlp_chain_tile, the 16-wide chain shape; the planner routes only
// plans whose edge MLPs are chained).  grid: (ceil(N^2 / 64), B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_edge(MlpD m, const float* __restrict__ wp, const float* __restrict__ att, float* __restrict__ S,
                                                       long long sstride, int ci0, int co0, int cin, int N) {
    const int b = blockIdx.y, NN = N * N;
    const float* X = att + (size_t)b * cin * NN;
    float* Sb = S + (size_t)b * sstride;
    const float* X2 = Sb + (size_t)ci0 * NN;
    float* dst = Sb + (size_t)co0 * NN;
    auto ident = [](int r) { return r; };
    auto epi = [&](int r, int f, float v) { dst[(size_t)f * NN + r] = v; };
#ifdef CCSD_EMU
    for (int wv = 0; wv < CCSD_LG_FIN_ROWS / 16; ++wv)
#else
    const int wv = wave_index();
#endif
    {
        const int p0 = blockIdx.x * CCSD_LG_FIN_ROWS + 16 * wv;
        if (p0 < NN) mlp_chain_tile<1, 1, 1>(m, wp, X, NN, X2, cin, p0, NN, ident, epi);
    }
}

// S[b][co0 + c] <- mask_adjs(T + T^T) in place: the work item of an unordered pair (i <= j) reads and writes both entries
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_sym(float* __restrict__ S, long long sstride, int co0, int cout, int N, const float* __restrict__ flags) {
    const int b = blockIdx.y, NN = N * N;
    const float* fl = flags + (size_t)b * N;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < (long long)cout * NN; t += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(t / NN), ij = (int)(t - (long long)c * NN), i = ij / N, j = ij - i * N;
        if (j < i) continue;
        float* T = S + (size_t)b * sstride + (size_t)(co0 + c) * NN;
        const float fm = fl[i] * fl[j];
        const float v = (T[(size_t)i * N + j] + T[(size_t)j * N + i]) * fm;
        T[(size_t)i * N + j] = v;
        T[(size_t)j * N + i] = v;
    }
}

// final MLP of ScoreNetworkA per entry (ScoreNetwork_A.py:530-541: fdim -> 2 fdim -> 2 fdim -> 1, ELU) on MFMA (mlp_chain_tile), then
// the no-diagonal and flag masks and k_xa's adjacency epilogue (same contract and expressions, ccsd_k_xa.h): SCORE ss * net; NORMS
// raw net + per-workgroup partials (net^2, z^2) to part[b][tile][2]; PRED mean = pa adj + pb net, out = mean + pc z.
// grid: (ceil(N^2 / 64), B)
// k_lg_fin: the shapes of CCSD_CHAIN_AFIN (m = PlanD::a_fin); k_lg_fin_w (ccsd_lgw.hip): the one shape of CCSD_CHAIN_AFIN_LG (57 to 64
// channels, m = PlanBuilder::afin_lg)
#define LG_FIN_KERNEL k_lg_fin
#define LG_FIN_CHAIN                                                                                \
    if (m.chain == 3) mlp_chain_tile<2, 4, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);           \
    else if (m.chain == 4) mlp_chain_tile<3, 5, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);      \
    else if (m.chain == 5) mlp_chain_tile<3, 6, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);      \
    else mlp_chain_tile<4, 7, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);
#include "ccsd_lg_fin.inc"
#undef LG_FIN_KERNEL
#undef LG_FIN_CHAIN
#ifdef CCSD_EMU          // (the product compiles k_lg_fin_w in a unit of its own, ccsd_lgw.hip)
#include "ccsd_lg_fin_w.inc"
#endif

// the node-feature epilogue (k_xa's: SCORE / NORMS / PRED on the masked net) and, in NORMS mode, norm2[b][4] in k_normsum's layout:
// |net_x|^2, |net_adj|^2 (k_lg_fin's tile partials, fixed order), |z_x|^2, |z_adj|^2.  One workgroup per sample.
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_epi(const float* __restrict__ xnet, const float* __restrict__ x, const float* __restrict__ flags,
                                                      XaArgs xa, NoiseArgs na, const float* __restrict__ part, int ntiles, int N, int F) {
    __shared__ float red[16 * 4];
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (xa.do_x) {
        for (int t = tid; t < N * F; t += nth) {
            const float fl = flags[(size_t)b * N + t / F];
            const size_t gi = (size_t)b * N * F + t;
            const float net = xnet[gi];                                  // (masked by k_lg_nmlp)
            if (xa.mode == MODE_SCORE) {
                xa.out_x[gi] = xa.ss_x * net;
            } else {
                const float z = raw_noise_x(na, b, t, N * F) * fl;       // gen_noise(sym=False)
                if (xa.mode == MODE_NORMS) {
                    xa.out_x[gi] = net;
                    v[0] = fmaf(net, net, v[0]);
                    v[2] = fmaf(z, z, v[2]);
                } else {
                    float mean;
                    const float nv = pred_update(xa.pa_x, xa.pb_x, xa.pc_x, x[gi], net, z, &mean);
                    if (xa.mean_x) xa.mean_x[gi] = mean;
                    xa.out_x[gi] = nv;
                }
            }
        }
    }
    if (xa.mode != MODE_NORMS) return;
    if (xa.do_a)
        for (int t = tid; t < ntiles; t += nth) {
            v[1] += part[((size_t)b * ntiles + t) * 2];
            v[3] += part[((size_t)b * ntiles + t) * 2 + 1];
        }
    block_sums<4>(v, red);
    if (tid == 0) {
        float* o = xa.norm2 + (size_t)b * 4;
        if (xa.do_x) { o[0] = v[0]; o[2] = v[2]; }
        if (xa.do_a) { o[1] = v[1]; o[3] = v[3]; }
    }
}
// ---- The hodge branch of ScoreNetworkA_CC (ScoreNetwork_A_CC.py:295-316; the oracle's score_network_a_cc), k_xa's with the same
// expressions.  adj_to_hodgedual makes the hodge adjacency of channel c diagonal with the upper triangle of the adjacency power c on it
// (a_c[e] = S[c][i][j], e = (i, j), i < j), DenseHCNConv on a diagonal matrix is a row scaling of the layer-0 projection P_0 = F Wcat_0
// ([B][E][wc], left by the rank-2 side), and hodgedual_to_adj reads only the diagonal of every layer's output.  The two pieces every
// stack is made of, stated once:

// the first layer's Q | K row of channel c of one edge: g a g P_0[e][block c] + b, g = rsqrt(max(1, a)) (no self-loop: dense_hcn)
CCSD_DEV void lg_hd_qk0_row(const HodgeLayerD& h, const float* __restrict__ w, const float* __restrict__ pr, int c, float a, float* q) {
    const int qw = 2 * h.adim;
    const float g = 1.0f / sqrtf(fmaxf(a, 1.f));
    for (int d = 0; d < qw; ++d) q[d] = fmaf(g * a * g, pr[c * qw + d], w[h.bcat + c * qw + d]);
}
// a layer's output on the diagonal, from the Q | K rows qrow(c) of one edge: head-mean logits -> mlp_attention (zero-padded blocks in
// LDS) -> mask -> tanh -> + transpose, into rows Ho[0 .. cout) of the stack at (i, j) and (j, i)
template <class QROW>
CCSD_DEV void lg_hd_diag_edge(const HodgeLayerD& h, float rks, const float* s_hw, QROW qrow, float fh, float* Ho, int NN, size_t ij, size_t ji) {
    float in[CCSD_SMALLW], out[CCSD_SMALLW];
#pragma unroll
    for (int c = 0; c < CCSD_SMALLW; ++c) {
        float sacc = 0.f;
        if (c < h.cin) {
            const float* q = qrow(c);
            sacc = attn_logits(q, q + h.adim, h.nchunk, h.dsplit, rks) * (1.0f / (float)h.nchunk);
        }
        in[c] = sacc;
    }
    small_mlp_lds<CCSD_SMALLW>(s_hw, h.matt.n, in, out);     // mlp_attention -> mask -> tanh -> + transpose
#pragma unroll
    for (int o = 0; o < CCSD_SMALLW; ++o)
        if (o < h.cout) {
            const float tv = tanh_f(out[o] * fh * fh);
            Ho[(size_t)o * NN + ij] = tv + tv;
            Ho[(size_t)o * NN + ji] = tv + tv;
        }
}

// ONE HodgeAdjAttentionLayer: everything is arithmetic per edge.  Written at (i, j) and (j, i) of the stack: rows ch0 .. ch0 + cin the
// hodge adjacency a_c itself, the next cout rows 2 tanh(fl^2 mlp_attention(head-mean logits)).  The work items behind the E edges are
// the N diagonal entries of those rows: zero (nothing is scattered there, and the workspace is not cleared).
// grid: (grid-stride over E + N, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hodge1(HodgeLayerD h, float rks, const float* __restrict__ w, const unsigned char* __restrict__ edges,
                                                         const float* __restrict__ P0, float* __restrict__ S, long long sstride, int ch0, int N,
                                                         int E, const float* __restrict__ flags) {
    __shared__ float s_hw[CCSD_MAXLIN * CCSD_HWBLK];                  // zero-padded mlp_attention weight blocks
    __shared__ float s_q[CCSD_LG_TB][2 * CCSD_LG_HAD + 1];            // the calling thread's Q | K row of one channel
    const int b = blockIdx.y, NN = N * N;
    stage_mlp_blocks(h.matt, w, s_hw, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
    float* Sb = S + (size_t)b * sstride;
    float* Hb = Sb + (size_t)ch0 * NN;
    const float* fl = flags + (size_t)b * N;
    float* q = &s_q[threadIdx.x][0];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < E + N; t += gridDim.x * blockDim.x) {
        if (t >= E) {
            const int i = t - E;
            for (int c = 0; c < h.cin + h.cout; ++c) Hb[(size_t)c * NN + (size_t)i * N + i] = 0.f;
            continue;
        }
        const int i = edges[2 * t], j = edges[2 * t + 1];
        const size_t ij = (size_t)i * N + j, ji = (size_t)j * N + i;
        const float* pr = P0 + ((size_t)b * E + t) * h.wc;
        auto qrow = [&](int c) {
            const float a = Sb[(size_t)c * NN + ij];
            lg_hd_qk0_row(h, w, pr, c, a, q);
            Hb[(size_t)c * NN + ij] = a;
            Hb[(size_t)c * NN + ji] = a;
            return (const float*)q;
        };
        lg_hd_diag_edge(h, rks, s_hw, qrow, fl[i] * fl[j], Hb + (size_t)h.cin * NN, NN, ij, ji);
    }
}

// ---- TWO OR MORE HodgeAdjAttentionLayers (hodge_attention.py:290-325; the oracle's hodge_adj_attention_layer), E <= CCSD_LG_HD_MAXE.
// Layer l sees the dense hodge adjacency channels H^l [cin][E][E] (H^0: the diagonal a_c) and the projection P_l = R_l Wcat_l of its
// rank-2 features ([B][E][wc_l], delivered by the rank-2 side: launch_lg):
//   dis_c[e] = rsqrt(max(1, sum_e' H_c[e][e']))                                        (k_lg_hd_dis; the diagonal counts as it is)
//   Q | K_c[e] = dis_c[e] sum_e' H_c[e][e'] dis_c[e'] P_l[e'][block c] + b            (k_lg_hd_conv; l = 0: k_lg_hd_qk0, per edge)
//   A_c[e][e'] = mean over heads of tanh(Q_h[e] . K_h[e'] / sqrt(K)), (A + A^T) / 2
//   H^(l+1) = 2 tanh(fh[e] fh[e'] mlp_attention(cat_c A_c)),  fh[e] = fl(i) fl(j)      (k_lg_hd_dense; A is symmetric: h + h^T = 2 h)
// The diagonal of every layer's output goes behind the graph channels of the stack, at (i, j) and (j, i); only the last layer's
// diagonal is ever read, so the last layer is evaluated there alone (k_lg_hd_diag).  The dense output lives in ONE workspace buffer
// [B][c_hid_h][E][E]: k_lg_hd_dis / k_lg_hd_conv (and k_hodge_value of the general stack) are all that read it, and the next layer's
// dense pass, which overwrites it, reads only the Q | K rows they left.  No atomics, fixed summation orders: launches repeat bit for bit.

// the input channels into the stack (rows ch0 .. ch0 + cin; zeros on the node diagonal of all nch hodge rows) and layer 0's Q | K rows
// QK[b][c][e][2 adim].  grid: (grid-stride over E + N, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hd_qk0(HodgeLayerD h, int nch, const float* __restrict__ w, const unsigned char* __restrict__ edges,
                                                         const float* __restrict__ P0, float* __restrict__ S, long long sstride, int ch0, int N,
                                                         int E, float* __restrict__ QK, long long qstride) {
    const int b = blockIdx.y, NN = N * N, qw = 2 * h.adim;
    float* Sb = S + (size_t)b * sstride;
    float* Hb = Sb + (size_t)ch0 * NN;
    float* Qb = QK + (size_t)b * qstride;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < E + N; t += gridDim.x * blockDim.x) {
        if (t >= E) {
            const int i = t - E;
            for (int c = 0; c < nch; ++c) Hb[(size_t)c * NN + (size_t)i * N + i] = 0.f;
            continue;
        }
        const int i = edges[2 * t], j = edges[2 * t + 1];
        const size_t ij = (size_t)i * N + j, ji = (size_t)j * N + i;
        const float* pr = P0 + ((size_t)b * E + t) * h.wc;
        for (int c = 0; c < h.cin; ++c) {
            const float a = Sb[(size_t)c * NN + ij];
            lg_hd_qk0_row(h, w, pr, c, a, Qb + ((size_t)c * E + t) * qw);
            Hb[(size_t)c * NN + ij] = a;
            Hb[(size_t)c * NN + ji] = a;
        }
    }
}

// upper-triangle tile t of an nt x nt grid of tiles, row-major -> row tile ty, column tile ty + dt
CCSD_DEV void lg_tri_tile(int t, int nt, int& ty, int& dt) {
    ty = 0;
    while (t >= nt - ty) { t -= nt - ty; ++ty; }
    dt = t;
}
// entry (e, f) of output channel o of a dense hodge layer, v = the channel mix before the mask: 2 tanh(fl(i) fl(j) fl(i') fl(j') v) into
// Hb [cout][E][E], mirrored (a tile on the diagonal computes both halves itself); the diagonal also into row o of Sb at (i, j) and (j, i)
CCSD_DEV void lg_dense_store(float v, int o, int e, int f, bool diag, int E, int N, const unsigned char* __restrict__ edges,
                             const float* __restrict__ fl, float* __restrict__ Hb, float* __restrict__ Sb) {
    if (e >= E || f >= E) return;
    const int i = edges[2 * e], j = edges[2 * e + 1], i2 = edges[2 * f], j2 = edges[2 * f + 1];
    const float fh = fl[i] * fl[j] * fl[i2] * fl[j2];
    const float tv = tanh_f(v * fh), val = tv + tv;
    float* Ho = Hb + (size_t)o * E * E;
    Ho[(size_t)e * E + f] = val;
    if (!diag) Ho[(size_t)f * E + e] = val;
    else if (e == f) {
        const int NN = N * N;
        Sb[(size_t)o * NN + (size_t)i * N + j] = val;
        Sb[(size_t)o * NN + (size_t)j * N + i] = val;
    }
}

// The dense output of a layer but the last from its Q | K rows.  One 16 x 16 tile (e, e') of the upper triangle per workgroup, mirrored
// on store (a tile on the diagonal computes both halves itself: the two orders of a pair add the same two logit sums, the result is
// symmetric bit for bit).  The rows of the tile's 16 + 16 edges of every channel are staged in LDS; the 256 pairs' symmetrised
// attentions (both orders of the head products, k_xa's expression) go to LDS, one pair per thread; mlp_attention then runs per 16-pair
// tile on MFMA (mlp_chain_tile, the 16-wide chain shape: matt = the layer's mlp_attention with its packed copies, PlanBuilder::hdm), four
// tiles per wave.  Ragged last tile: rows beyond E are staged from row E - 1 and never stored.
// dynamic LDS: lg_hd_dense_lds(h).  grid: (nt (nt + 1) / 2, B), nt = ceil(E / 16)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hd_dense(HodgeLayerD h, MlpD matt, float rks, const float* __restrict__ wp,
                                                           const unsigned char* __restrict__ edges, const float* __restrict__ QK, long long qstride,
                                                           float* __restrict__ Hout, long long hstride, float* __restrict__ S, long long sstride,
                                                           int ch0, int N, int E, const float* __restrict__ flags) {
    CCSD_DYN_SMEM(sm);
    const int b = blockIdx.y, tid = threadIdx.x, nth = blockDim.x, NN = N * N;
    int ty, dt;
    lg_tri_tile(blockIdx.x, (E + 15) / 16, ty, dt);
    const int e0 = 16 * ty, f0 = 16 * (ty + dt);
    const bool diag = dt == 0;
    const int cin = h.cin, qw = 2 * h.adim, ldq = lg_hb_row_ld(qw);
    float* s_q = sm;                             // [side][cin][16][ldq]: Q | K rows of the tile's row edges (side 0) / column edges (1)
    float* s_S = s_q + 2 * cin * 16 * ldq;       // [cin][256]: mlp_attention's input, pair u = 16 r + q
    const float* Qb = QK + (size_t)b * qstride;
    for (int u = tid; u < 2 * cin * 16 * qw; u += nth) {
        const int d = u % qw, v = u / qw, r = v & 15, sc = v >> 4, c = sc % cin, side = sc / cin;
        const int e = (side ? f0 : e0) + r, ec = e < E ? e : E - 1;
        s_q[(sc * 16 + r) * ldq + d] = Qb[((size_t)c * E + ec) * qw + d];
    }
    __syncthreads();
    const float rnc = 1.0f / (float)h.nchunk;
    for (int u = tid; u < 256; u += nth) {
        const int r = u >> 4, q = u & 15;
        for (int c = 0; c < cin; ++c) {
            const float* q1 = s_q + (c * 16 + r) * ldq;
            const float* q2 = s_q + ((cin + c) * 16 + q) * ldq;
            const float s1 = attn_logits(q1, q2 + h.adim, h.nchunk, h.dsplit, rks);
            const float s2 = attn_logits(q2, q1 + h.adim, h.nchunk, h.dsplit, rks);
            s_S[c * 256 + u] = (s1 * rnc + s2 * rnc) * 0.5f;
        }
    }
    __syncthreads();
    float* Hb = Hout + (size_t)b * hstride;
    float* Sb = S + (size_t)b * sstride + (size_t)ch0 * NN;
    const float* fl = flags + (size_t)b * N;
    auto ident = [](int r) { return r; };
    auto epi = [&](int u, int o, float v) { lg_dense_store(v, o, e0 + (u >> 4), f0 + (u & 15), diag, E, N, edges, fl, Hb, Sb); };
#ifdef CCSD_EMU
    for (int wv = 0; wv < CCSD_LG_TB / 64; ++wv)
#else
    const int wv = wave_index();
#endif
        for (int q4 = 0; q4 < 4; ++q4) mlp_chain_tile<1, 1, 1>(matt, wp, s_S, 256, s_S, matt.in, 16 * (4 * wv + q4), 256, ident, epi);
}

// dis[b][c][e] = rsqrt(max(1, sum_e' Hin[b][c][e][e'])) of a dense input (the matrix is symmetric bit for bit: the sum walks the column,
// consecutive threads read consecutive words), and, for the raw P_1 of the fused rank-2 family, its per-edge factors (LgHdRaw)
// grid: (grid-stride over cin E, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hd_dis(const float* __restrict__ Hin, long long hstride, int cin, int E, float* __restrict__ dis,
                                                         LgHdRaw raw) {
    const int b = blockIdx.y;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < cin * E; t += gridDim.x * blockDim.x) {
        const int c = t / E, e = t - c * E;
        const float* col = Hin + (size_t)b * hstride + (size_t)c * E * E + e;
        float s = 0.f;
        for (int e2 = 0; e2 < E; ++e2) s += col[(size_t)e2 * E];
        dis[((size_t)b * cin + c) * E + e] = 1.0f / sqrtf(fmaxf(s, 1.f));
    }
    if (!raw.pc) return;
    const int NN = raw.N * raw.N;
    const float mvb0 = raw.w[raw.mb];
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        const int i = raw.edges[2 * e], j = raw.edges[2 * e + 1];
        float sc = 0.f;
        for (int c = 0; c < raw.cin0; ++c) sc = fmaf(raw.w[raw.mw + c], raw.S[(size_t)b * raw.sstride + (size_t)c * NN + (size_t)i * raw.N + j], sc);
        const float fl = raw.flags[(size_t)b * raw.N + i] * raw.flags[(size_t)b * raw.N + j];
        raw.pc[((size_t)b * 2) * E + e] = fl * sc;
        raw.pc[((size_t)b * 2 + 1) * E + e] = fl * mvb0;
    }
}

// Q | K rows of a layer with dense input: QK[b][c][e][d] = dis_c[e] sum_e' Hin[b][c][e][e'] dis_c[e'] P[b][e'][c 2 adim + d] + b_c[d] -- an
// (E x E) . (E x 2 adim) product per channel, 2 adim <= 32 (CCSD_LG_HAD).  One 16-row tile per wave over the whole E and both 16-column
// tiles, v_mfma_f32_16x16x4_f32 in the permuted-k fragment order of the tiled GEMM kernels (frag_mma, row_load4: k_lg_hb_hid's form);
// dis[e'] is folded into the B operand, dis[e] and the bias are applied in the epilogue.  P: row stride ldp; pc != nullptr: P holds
// the raw factors Q_1 and U [B][ldp] the row u_1, P_1[e'] = pc[0][e'] Q_1[e'] + pc[1][e'] u_1 (k_xa's p1_compose).  Each row of Hin is
// read once: the pass is HBM-bound.  The ragged last row tile reads row E - 1 and stores nothing; the ragged k tail and the columns
// beyond 2 adim are zeros by guard, not by padding.
// grid: (ceil(ceil(E / 16) / 4), cin, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hd_conv(HodgeLayerD h, const float* __restrict__ w, const float* __restrict__ Hin, long long hstride,
                                                          const float* __restrict__ dis, const float* __restrict__ P, int ldp,
                                                          const float* __restrict__ pc, const float* __restrict__ U, int E,
                                                          float* __restrict__ QK, long long qstride) {
    const int c = blockIdx.y, b = blockIdx.z, qw = 2 * h.adim;
    const float* Hc = Hin + (size_t)b * hstride + (size_t)c * E * E;
    const float* dg = dis + ((size_t)b * h.cin + c) * E;
    const float* Pb = P + (size_t)b * E * ldp + c * qw;
    const float* pcb = pc ? pc + (size_t)b * 2 * E : nullptr;
    const float* Ub = pc ? U + (size_t)b * ldp + c * qw : nullptr;
    const float* bias = w + h.bcat + c * qw;
    float* Qc = QK + (size_t)b * qstride + (size_t)c * E * qw;
    // B operand: row k (< E), column d (< qw) of dis . P_l
    auto bval = [&](int k, int d) {
        const float pv = Pb[(size_t)k * ldp + d];
        return dg[k] * (pcb ? fmaf(pcb[k], pv, pcb[E + k] * Ub[d]) : pv);
    };
#ifdef CCSD_EMU
    for (int wv = 0; wv < CCSD_LG_TB / 64; ++wv) {
        const int m0 = 16 * (4 * blockIdx.x + wv);
        for (int e = m0; e < m0 + 16 && e < E; ++e)
            for (int d = 0; d < qw; ++d) {
                float acc = 0.f;
                for (int k = 0; k < E; ++k) acc = fmaf(Hc[(size_t)e * E + k], bval(k, d), acc);
                Qc[(size_t)e * qw + d] = fmaf(dg[e], acc, bias[d]);
            }
    }
#else
    const int m0 = 16 * (4 * blockIdx.x + wave_index());
    if (m0 >= E) return;
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const float* row = Hc + (size_t)(m0 + l15 < E ? m0 + l15 : E - 1) * E;
    const bool vec = (E & 3) == 0, two = qw > 16;
    const int d0 = l15 < qw ? l15 : qw - 1, d1 = 16 + l15 < qw ? 16 + l15 : qw - 1;
    const bool col0 = l15 < qw, col1 = 16 + l15 < qw;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < E; k0 += 16) {
        const int k = k0 + 4 * kq;
        float4 a, bq;
        row_load4(a, row, k, E, vec);
        const int ka = k < E ? k : E - 1, kb = k + 1 < E ? k + 1 : E - 1, kc = k + 2 < E ? k + 2 : E - 1, kd = k + 3 < E ? k + 3 : E - 1;
        bq.x = (col0 && k < E) ? bval(ka, d0) : 0.f;
        bq.y = (col0 && k + 1 < E) ? bval(kb, d0) : 0.f;
        bq.z = (col0 && k + 2 < E) ? bval(kc, d0) : 0.f;
        bq.w = (col0 && k + 3 < E) ? bval(kd, d0) : 0.f;
        frag_mma(acc0, a, bq);
        if (two) {
            bq.x = (col1 && k < E) ? bval(ka, d1) : 0.f;
            bq.y = (col1 && k + 1 < E) ? bval(kb, d1) : 0.f;
            bq.z = (col1 && k + 2 < E) ? bval(kc, d1) : 0.f;
            bq.w = (col1 && k + 3 < E) ? bval(kd, d1) : 0.f;
            frag_mma(acc1, a, bq);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = m0 + 4 * kq + r;
        if (e >= E) continue;
        if (col0) Qc[(size_t)e * qw + l15] = fmaf(dg[e], acc0[r], bias[l15]);
        if (two && col1) Qc[(size_t)e * qw + 16 + l15] = fmaf(dg[e], acc1[r], bias[16 + l15]);
    }
#endif
}

// The last layer, on its diagonal, from its Q | K rows: lg_hd_diag_edge into stack rows ch0 .. ch0 + cout.  grid: (grid-stride over E, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hd_diag(HodgeLayerD h, float rks, const float* __restrict__ w, const unsigned char* __restrict__ edges,
                                                          const float* __restrict__ QK, long long qstride, float* __restrict__ S, long long sstride,
                                                          int ch0, int N, int E, const float* __restrict__ flags) {
    __shared__ float s_hw[CCSD_MAXLIN * CCSD_HWBLK];
    const int b = blockIdx.y, NN = N * N, qw = 2 * h.adim;
    stage_mlp_blocks(h.matt, w, s_hw, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
    const float* Qb = QK + (size_t)b * qstride;
    float* Sb = S + (size_t)b * sstride + (size_t)ch0 * NN;
    const float* fl = flags + (size_t)b * N;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        const int i = edges[2 * e], j = edges[2 * e + 1];
        auto qrow = [&](int c) { return Qb + ((size_t)c * E + e) * qw; };
        lg_hd_diag_edge(h, rks, s_hw, qrow, fl[i] * fl[j], Sb, NN, (size_t)i * N + j, (size_t)j * N + i);
    }
}

// ---- Hodge MLPs wider than 8 (num_linears_h >= 2 with a hidden width of 9 .. 16; Route::h_wide).  lg_hd_diag_edge's per-thread MLP is 8
// wide -- at 16 its two register arrays would not fit beside the Q | K walk --, so mlp_attention on the diagonal runs as the dense pass
// runs it: the 16-wide MFMA chain (mlp_chain_tile<1, 1, 1>) on the packed copies of PlanBuilder::hdm, 16 edges per tile.  One pass of a
// workgroup takes CCSD_LG_TB consecutive edges from e0: every thread leaves the head-mean logits of its edge's channels in LDS
// (s_S [cin][CCSD_LG_TB], mlp_attention's input, feature-major), then each wave runs four tiles; the epilogue is lg_hd_diag_edge's (mask, 2 tanh,
// both orders of the node pair).  qrow(c, e): the Q | K row of channel c of edge e.  The same expressions as the narrow form but for the
// summation order inside the MLP (the chain's).
template <class QROW>
CCSD_DEV void lg_hd_diag_tiles(const HodgeLayerD& h, const MlpD& matt, float rks, const float* __restrict__ wp, float* s_S, int e0, int E, QROW qrow,
                               const unsigned char* __restrict__ edges, const float* __restrict__ fl, float* Ho, int N) {
    const int NN = N * N;
    const float rnc = 1.0f / (float)h.nchunk;
    for (int u = (int)threadIdx.x; u < CCSD_LG_TB; u += (int)blockDim.x) {
        const int e = e0 + u;
        if (e >= E) continue;                       // (a tile's rows beyond E are clamped to its last valid row by mlp_chain_tile)
        for (int c = 0; c < h.cin; ++c) {
            const float* q = qrow(c, e);
            s_S[c * CCSD_LG_TB + u] = attn_logits(q, q + h.adim, h.nchunk, h.dsplit, rks) * rnc;
        }
    }
    __syncthreads();
    const int rows = E - e0 < CCSD_LG_TB ? E - e0 : CCSD_LG_TB;
    auto ident = [](int r) { return r; };
    auto epi = [&](int u, int o, float v) {
        const int i = edges[2 * (e0 + u)], j = edges[2 * (e0 + u) + 1];
        const float fh = fl[i] * fl[j];
        const float tv = tanh_f(v * fh * fh);
        Ho[(size_t)o * NN + (size_t)i * N + j] = tv + tv;
        Ho[(size_t)o * NN + (size_t)j * N + i] = tv + tv;
    };
#ifdef CCSD_EMU
    for (int wv = 0; wv < CCSD_LG_TB / 64; ++wv)
#else
    const int wv = wave_index();
#endif
        for (int q4 = 0; q4 < 4; ++q4) {
            const int p0 = 16 * (4 * wv + q4);
            if (p0 < rows) mlp_chain_tile<1, 1, 1>(matt, wp, s_S, CCSD_LG_TB, s_S, matt.in, p0, rows, ident, epi);
        }
    __syncthreads();                                // (the next pass rewrites s_S)
}

// k_lg_hodge1 for such a plan (matt = hdm[0]).  grid: (grid-stride over E in passes of CCSD_LG_TB, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hodge1_w(HodgeLayerD h, MlpD matt, float rks, const float* __restrict__ w, const float* __restrict__ wp,
                                                           const unsigned char* __restrict__ edges, const float* __restrict__ P0, float* __restrict__ S,
                                                           long long sstride, int ch0, int N, int E, const float* __restrict__ flags) {
    __shared__ float s_S[CCSD_SMALLW * CCSD_LG_TB];
    __shared__ float s_q[CCSD_LG_TB][2 * CCSD_LG_HAD + 1];
    const int b = blockIdx.y, NN = N * N;
    float* Sb = S + (size_t)b * sstride;
    float* Hb = Sb + (size_t)ch0 * NN;
    const float* fl = flags + (size_t)b * N;
    float* q = &s_q[threadIdx.x][0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
        for (int c = 0; c < h.cin + h.cout; ++c) Hb[(size_t)c * NN + (size_t)i * N + i] = 0.f;
    auto qrow = [&](int c, int e) {
        const int i = edges[2 * e], j = edges[2 * e + 1];
        const size_t ij = (size_t)i * N + j, ji = (size_t)j * N + i;
        const float a = Sb[(size_t)c * NN + ij];
        lg_hd_qk0_row(h, w, P0 + ((size_t)b * E + e) * h.wc, c, a, q);
        Hb[(size_t)c * NN + ij] = a;
        Hb[(size_t)c * NN + ji] = a;
        return (const float*)q;
    };
    for (int e0 = blockIdx.x * CCSD_LG_TB; e0 < E; e0 += gridDim.x * CCSD_LG_TB)
        lg_hd_diag_tiles(h, matt, rks, wp, s_S, e0, E, qrow, edges, fl, Hb + (size_t)h.cin * NN, N);
}
// k_lg_hd_diag for such a plan (matt = hdm[h_L - 1]).  grid: (grid-stride over E in passes of CCSD_LG_TB, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hd_diag_w(HodgeLayerD h, MlpD matt, float rks, const float* __restrict__ wp,
                                                            const unsigned char* __restrict__ edges, const float* __restrict__ QK, long long qstride,
                                                            float* __restrict__ S, long long sstride, int ch0, int N, int E,
                                                            const float* __restrict__ flags) {
    __shared__ float s_S[CCSD_SMALLW * CCSD_LG_TB];
    const int b = blockIdx.y, qw = 2 * h.adim;
    const float* Qb = QK + (size_t)b * qstride;
    auto qrow = [&](int c, int e) { return Qb + ((size_t)c * E + e) * qw; };
    for (int e0 = blockIdx.x * CCSD_LG_TB; e0 < E; e0 += gridDim.x * CCSD_LG_TB)
        lg_hd_diag_tiles(h, matt, rks, wp, s_S, e0, E, qrow, edges, flags + (size_t)b * N, S + (size_t)b * sstride + (size_t)(ch0 * N) * N, N);
}


// ---- The hodge branch of ScoreNetworkA_Base_CC (ScoreNetwork_A_Base_CC.py:295-316; the oracle's score_network_a_base_cc): L
// HodgeBaselineLayers (hodge_layers.py:259-284, 381-416) on the E x E hodge adjacency channels, k_xa's HB block with the same
// expressions, the dense layers tiled through the workspace.  Per input channel c of a layer a BaselineBlock (weights
// W1[hid][E] b1[hid] W2[E][hid] b2[E]): g_c[e] = elu(W1 H_c[e] + b1) (hidden rows), T_c[e][e'] = tanh(W2[e'] . g_c[e] + b2[e']); mlp_hodge
// mixes the symmetrised channels (T_c + T_c^T) / 2 per (e, e'), then mask_hodge_adjs, tanh, + transpose.  The layers' rank-2 outputs
// never reach the score and are not evaluated; adj_to_hodgedual makes the first layer's input diagonal (a_c[e] on it: entry (i, j) of
// adjacency power c), and hodgedual_to_adj reads only the diagonal of every layer's output, so the last layer is evaluated there
// alone.  Stack rows ch0 ..: the a_c, then every layer's diagonal, at (i, j) and (j, i) of each edge, zero on the node diagonal.
// No atomics, fixed summation orders: launches repeat bit for bit.

// the input channels into the stack (rows ch0 .. ch0 + cin; zeros on the node diagonal of all nch hodge rows: nothing else writes
// there, and the workspace is not cleared) and the first layer's hidden rows G[b][c][e][h] = elu(W1_c[h][e] a_c[e] + b1_c[h])
// grid: (grid-stride over E + N, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hb_in(HodgeBaseD h, int nch, const float* __restrict__ w, const unsigned char* __restrict__ edges,
                                                        float* __restrict__ S, long long sstride, int ch0, int N, int E, float* __restrict__ G,
                                                        long long gstride) {
    const int b = blockIdx.y, NN = N * N, hid = h.hid;
    float* Sb = S + (size_t)b * sstride;
    float* Hb = Sb + (size_t)ch0 * NN;
    float* Gb = G + (size_t)b * gstride;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < E + N; t += gridDim.x * blockDim.x) {
        if (t >= E) {
            const int i = t - E;
            for (int c = 0; c < nch; ++c) Hb[(size_t)c * NN + (size_t)i * N + i] = 0.f;
            continue;
        }
        const int i = edges[2 * t], j = edges[2 * t + 1];
        const size_t ij = (size_t)i * N + j, ji = (size_t)j * N + i;
        for (int c = 0; c < h.cin; ++c) {
            const float* blk = w + h.blk_base + (size_t)c * h.blk_stride;
            const float a = Sb[(size_t)c * NN + ij];
            Hb[(size_t)c * NN + ij] = a;
            Hb[(size_t)c * NN + ji] = a;
            float* g = Gb + ((size_t)c * E + t) * hid;
            for (int hh = 0; hh < hid; ++hh) g[hh] = elu1(fmaf(blk[(size_t)hh * E + t], a, blk[(size_t)hid * E + hh]));
        }
    }
}

// The dense output of a layer but the last from its hidden rows: Hout[b][o][e][e'] = 2 tanh(fl(i) fl(j) fl(i') fl(j') mlp_hodge(S)_o),
// S_c = (T_c[e][e'] + T_c[e'][e]) / 2.  One 16 x 16 tile (e, e') of the upper triangle per workgroup, mirrored on store (a tile on the
// diagonal computes both halves itself: the two orders of a pair go through the same operations, the result is symmetric bit for
// bit).  The 256 pairs' block outputs go to LDS, one pair per thread; mlp_hodge then runs per 16-pair tile on MFMA (mlp_chain_tile,
// the 16-wide chain shape: the planner chains it for every dense layer), four tiles per wave.  The diagonal also goes to stack rows
// ch0 .. ch0 + cout.  Ragged last tile: rows beyond E are staged from row E - 1 and never stored.
// dynamic LDS: lg_hb_dense_lds(h).  grid: (nt (nt + 1) / 2, B), nt = ceil(E / 16)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hb_dense(HodgeBaseD h, const float* __restrict__ w, const float* __restrict__ wp,
                                                           const unsigned char* __restrict__ edges, const float* __restrict__ G, long long gstride,
                                                           float* __restrict__ Hout, long long hstride, float* __restrict__ S, long long sstride,
                                                           int ch0, int N, int E, const float* __restrict__ flags) {
    CCSD_DYN_SMEM(sm);
    const int b = blockIdx.y, tid = threadIdx.x, nth = blockDim.x, NN = N * N;
    int ty, t;                                   // upper-triangle tile -> (row tile ty, column tile ty + t)
    lg_tri_tile(blockIdx.x, (E + 15) / 16, ty, t);
    const int e0 = 16 * ty, f0 = 16 * (ty + t);
    const bool diag = t == 0;
    const int hid = h.hid, hp = lg_hb_row_ld(hid), cin = h.cin;
    float* s_g = sm;                             // [side][cin][16][hp]: hidden rows of the tile's row edges (side 0) / column edges (1)
    float* s_w = s_g + 2 * cin * 16 * hp;        // ... their rows of W2
    float* s_b = s_w + 2 * cin * 16 * hp;        // [side][cin][16]: their b2
    float* s_S = s_b + 2 * cin * 16;             // [cin][256]: mlp_hodge's input, pair u = 16 r + q
    const float* Gb = G + (size_t)b * gstride;
    for (int u = tid; u < 2 * cin * 16 * hid; u += nth) {
        const int hh = u % hid, v = u / hid, r = v & 15, sc = v >> 4, c = sc % cin, side = sc / cin;
        const int e = (side ? f0 : e0) + r, ec = e < E ? e : E - 1;
        const float* blk = w + h.blk_base + (size_t)c * h.blk_stride;
        s_g[(sc * 16 + r) * hp + hh] = Gb[((size_t)c * E + ec) * hid + hh];
        s_w[(sc * 16 + r) * hp + hh] = blk[(size_t)hid * E + hid + (size_t)ec * hid + hh];
    }
    for (int u = tid; u < 2 * cin * 16; u += nth) {
        const int r = u & 15, sc = u >> 4, c = sc % cin, side = sc / cin;
        const int e = (side ? f0 : e0) + r, ec = e < E ? e : E - 1;
        s_b[u] = w[h.blk_base + (size_t)c * h.blk_stride + 2 * (size_t)hid * E + hid + ec];
    }
    __syncthreads();
    for (int u = tid; u < 256; u += nth) {
        const int r = u >> 4, q = u & 15;
        for (int c = 0; c < cin; ++c) {
            const float* gr = s_g + (c * 16 + r) * hp;
            const float* wr = s_w + (c * 16 + r) * hp;
            const float* gq = s_g + ((cin + c) * 16 + q) * hp;
            const float* wq = s_w + ((cin + c) * 16 + q) * hp;
            float a1 = 0.f, a2 = 0.f;
            for (int hh = 0; hh < hid; ++hh) {
                a1 = fmaf(gr[hh], wq[hh], a1);       // W2[e'] . g[e]
                a2 = fmaf(gq[hh], wr[hh], a2);       // W2[e] . g[e']
            }
            const float t1 = tanh_f(a1 + s_b[(cin + c) * 16 + q]), t2 = tanh_f(a2 + s_b[c * 16 + r]);
            s_S[c * 256 + u] = (diag && r == q) ? t1 : (t1 + t2) * 0.5f;
        }
    }
    __syncthreads();
    float* Hb = Hout + (size_t)b * hstride;
    float* Sb = S + (size_t)b * sstride + (size_t)ch0 * NN;
    const float* fl = flags + (size_t)b * N;
    auto ident = [](int r) { return r; };
    auto epi = [&](int u, int o, float v) { lg_dense_store(v, o, e0 + (u >> 4), f0 + (u & 15), diag, E, N, edges, fl, Hb, Sb); };
#ifdef CCSD_EMU
    for (int wv = 0; wv < CCSD_LG_TB / 64; ++wv)
#else
    const int wv = wave_index();
#endif
        for (int q4 = 0; q4 < 4; ++q4) mlp_chain_tile<1, 1, 1>(h.mh, wp, s_S, 256, s_S, h.mh.in, 16 * (4 * wv + q4), 256, ident, epi);
}

// The hidden rows of a layer with dense input: G[b][c][e][h] = elu(sum_e' W1_c[h][e'] Hin[b][c][e][e'] + b1_c[h]) -- an (E x E) . (E x hid)
// product per channel, hid <= 16 (CCSD_LG_HBW).  One 16-row x 16-column v_mfma_f32_16x16x4_f32 tile per wave over the whole E, in the
// permuted-k fragment order of the tiled GEMM kernels (frag_mma, row_load4: k slot kq of step j of block t <-> e' = 16 t + 4 kq + j), B
// operand from the packed W1^T [E][hid] (HodgeBaseD::w1t).  Each row of Hin is read once: the pass is HBM-bound.  The ragged last row
// tile reads row E - 1 and stores nothing; the ragged k tail and the columns beyond hid are zeros by guard, not by padding.
// grid: (ceil(ceil(E / 16) / 4), cin, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hb_hid(HodgeBaseD h, const float* __restrict__ w, const float* __restrict__ wp,
                                                         const float* __restrict__ Hin, long long hstride, int E, float* __restrict__ G,
                                                         long long gstride) {
    const int c = blockIdx.y, b = blockIdx.z, hid = h.hid;
    const float* Hc = Hin + (size_t)b * hstride + (size_t)c * E * E;
    const float* b1 = w + h.blk_base + (size_t)c * h.blk_stride + (size_t)hid * E;
    const float* W1t = wp + h.w1t + (size_t)c * E * hid;
    float* Gc = G + (size_t)b * gstride + (size_t)c * E * hid;
#ifdef CCSD_EMU
    for (int wv = 0; wv < CCSD_LG_TB / 64; ++wv) {
        const int m0 = 16 * (4 * blockIdx.x + wv);
        for (int e = m0; e < m0 + 16 && e < E; ++e)
            for (int hh = 0; hh < hid; ++hh) {
                float acc = 0.f;
                for (int k = 0; k < E; ++k) acc = fmaf(Hc[(size_t)e * E + k], W1t[(size_t)k * hid + hh], acc);
                Gc[(size_t)e * hid + hh] = elu1(acc + b1[hh]);
            }
    }
#else
    const int m0 = 16 * (4 * blockIdx.x + wave_index());
    if (m0 >= E) return;
    const int lane = threadIdx.x & 63, l15 = lane & 15, kq = lane >> 4;
    const float* row = Hc + (size_t)(m0 + l15 < E ? m0 + l15 : E - 1) * E;
    const bool vec = (E & 3) == 0, col = l15 < hid;
    const float* wcol = W1t + (col ? l15 : 0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < E; k0 += 16) {
        const int k = k0 + 4 * kq;
        float4 a, bq;
        row_load4(a, row, k, E, vec);
        bq.x = (col && k < E) ? wcol[(size_t)(k < E ? k : E - 1) * hid] : 0.f;
        bq.y = (col && k + 1 < E) ? wcol[(size_t)(k + 1 < E ? k + 1 : E - 1) * hid] : 0.f;
        bq.z = (col && k + 2 < E) ? wcol[(size_t)(k + 2 < E ? k + 2 : E - 1) * hid] : 0.f;
        bq.w = (col && k + 3 < E) ? wcol[(size_t)(k + 3 < E ? k + 3 : E - 1) * hid] : 0.f;
        frag_mma(acc, a, bq);
    }
    if (col) {
        const float bb = b1[l15];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = m0 + 4 * kq + r;
            if (e < E) Gc[(size_t)e * hid + l15] = elu1(acc[r] + bb);
        }
    }
#endif
}

// The last layer, on its diagonal: d_c[e] = tanh(W2_c[e] . g_c[e] + b2_c[e]), mlp_hodge per edge (the per-thread MLP from zero-padded
// 16 x 16 blocks in LDS), mask, 2 tanh into stack rows ch0 .. ch0 + cout at (i, j) and (j, i).  grid: (grid-stride over E, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hb_diag(HodgeBaseD h, const float* __restrict__ w, const unsigned char* __restrict__ edges,
                                                          const float* __restrict__ G, long long gstride, float* __restrict__ S, long long sstride,
                                                          int ch0, int N, int E, const float* __restrict__ flags) {
    __shared__ float s_mh[CCSD_MAXLIN * (CCSD_FW * CCSD_FW + CCSD_FW)];
    const int b = blockIdx.y, NN = N * N, hid = h.hid;
    stage_mlp_blocks_w<CCSD_FW>(h.mh, w, s_mh);
    __syncthreads();
    const float* Gb = G + (size_t)b * gstride;
    float* Sb = S + (size_t)b * sstride + (size_t)ch0 * NN;
    const float* fl = flags + (size_t)b * N;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        float in[CCSD_FW], out[CCSD_FW];
#pragma unroll
        for (int c = 0; c < CCSD_FW; ++c) {
            float v = 0.f;
            if (c < h.cin) {
                const float* blk = w + h.blk_base + (size_t)c * h.blk_stride;
                const float* w2 = blk + (size_t)hid * E + hid + (size_t)e * hid;
                const float* g = Gb + ((size_t)c * E + e) * hid;
                float acc = 0.f;
                for (int hh = 0; hh < hid; ++hh) acc = fmaf(g[hh], w2[hh], acc);
                v = tanh_f(acc + blk[2 * (size_t)hid * E + hid + e]);
            }
            in[c] = v;
        }
        small_mlp_ldsw<CCSD_FW>(s_mh, h.mh.n, in, out);
        const int i = edges[2 * e], j = edges[2 * e + 1];
        const float fh = fl[i] * fl[j];
#pragma unroll
        for (int o = 0; o < CCSD_FW; ++o)
            if (o < h.cout) {
                const float tv = tanh_f(out[o] * fh * fh);
                Sb[(size_t)o * NN + (size_t)i * N + j] = tv + tv;
                Sb[(size_t)o * NN + (size_t)j * N + i] = tv + tv;
            }
    }
}
#undef LG_PT
#endif  // CCSD_LG_UNIT || CCSD_EMU
