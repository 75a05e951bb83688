// ccsd_k_lg.h -- the tiled graph-network path (k_lg_*): ScoreNetworkX + ScoreNetworkA for plans whose per-graph working set does not
// fit one CU's LDS (graph-only plans with N > 64, or k_xa's layout fails; CCSD_LARGE_GRAPH=1 forces it for any eligible graph-only
// plan), and ScoreNetworkA_CC with ONE hodge layer for combinatorial complexes (N <= 64) without a k_xa layout (or under
// CCSD_LARGE_GRAPH=2, which forces every eligible plan).
// Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// State lives in the HBM workspace (carve_ws, LgWs in ccsd_api.h) and every phase is a launch of its own that tiles each graph over
// many workgroups.  The decomposition of one forward (launch_lg):
//   ScoreNetworkX   k_lg_dis (D^-1/2 of adjX) ; per GCN layer: k_lg_xw (Y = D^-1/2 X W), k_lg_gcn (tanh(D^-1/2 A' Y + b) into the
//                   concatenation) ; k_lg_nmlp (final MLP per node, mask_x)
//   ScoreNetworkA   k_lg_pow (channel stack [A, A^2, ...]) ; ScoreNetworkA_CC: k_lg_hodge1 (the hodge channels, behind the graph
//                   channels of the stack) ; per AttentionLayer: k_lg_dis, k_lg_xw (Q | K | V columns side by side),
//                   k_lg_gcn, k_lg_nmlp (multi_channel, mask_x, tanh), k_lg_att (head-mean tanh(Q K^T / sqrt(fout)), symmetrised),
//                   k_lg_edge (edge MLP on [att_c | adj_c] per entry, MFMA: mlp_chain_tile), k_lg_sym (out + out^T, mask_adjs) ;
//                   k_lg_fin (final MLP per entry, MFMA: mlp_chain_tile, + the adjacency epilogue, per-tile norm partials)
//   k_lg_epi        the node-feature epilogue and the per-sample norm reduction (fixed order, no atomics)
// Reference: attention.py:84-132, 270-304 (AttentionLayer), ScoreNetwork_A.py:505-541, ScoreNetwork_X.py:102-132, layers.py:134-158
// (DenseGCNConv, add_loop: the diagonal is SET to 1).  The oracle (oracle/ccsd_oracle.py: dense_gcn, attention, attention_layer,
// score_network_a, score_network_x) is the specification.
//
// Build: the definitions are compiled in ccsd_lg.hip (CCSD_LG_UNIT) and in the host emulation; ccsd_hip.hip sees the declarations.
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
__global__ void k_lg_epi(const float* __restrict__ xnet, const float* __restrict__ x, const float* __restrict__ flags, XaArgs xa,
                         NoiseArgs na, const float* __restrict__ part, int ntiles, int N, int F);

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
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_fin(MlpD m, const float* __restrict__ wp, const float* __restrict__ S, long long sstride, int N,
                                                      const float* __restrict__ flags, const float* __restrict__ adj, XaArgs xa, NoiseArgs na,
                                                      float* __restrict__ part) {
    __shared__ float red[16 * 2];
    const int b = blockIdx.y, NN = N * N;
    const float* X = S + (size_t)b * sstride;
    const float* fl = flags + (size_t)b * N;
    float n2 = 0.f, z2 = 0.f;
    auto ident = [](int r) { return r; };
    auto epi = [&](int ij, int f, float v) {
        (void)f;
        const int i = ij / N, j = ij - i * N;
        const float fm = fl[i] * fl[j];
        const float net = (i == j) ? 0.f : v * fm;               // * no-diag mask, then mask_adjs
        const size_t gi = (size_t)b * NN + ij;
        if (xa.mode == MODE_SCORE) {
            xa.out_a[gi] = xa.ss_a * net;
        } else {
            const float z = raw_noise_adj(na, b, i, j, N) * fm;    // gen_noise(sym=True), graph_utils.py:173-175
            if (xa.mode == MODE_NORMS) {
                xa.out_a[gi] = net;
                n2 = fmaf(net, net, n2);
                z2 = fmaf(z, z, z2);
            } else {
                float mean;
                const float nv = pred_update(xa.pa_a, xa.pb_a, xa.pc_a, adj[gi], net, z, &mean);
                if (xa.mean_a) xa.mean_a[gi] = mean;
                xa.out_a[gi] = nv;
            }
        }
    };
#ifdef CCSD_EMU
    for (int wv = 0; wv < CCSD_LG_FIN_ROWS / 16; ++wv)
#else
    const int wv = wave_index();
#endif
    {
        const int p0 = blockIdx.x * CCSD_LG_FIN_ROWS + 16 * wv;
        if (p0 < NN) {
            if (m.chain == 3) mlp_chain_tile<2, 4, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);
            else if (m.chain == 4) mlp_chain_tile<3, 5, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);
            else if (m.chain == 5) mlp_chain_tile<3, 6, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);
            else mlp_chain_tile<4, 7, 1>(m, wp, X, NN, X, m.in, p0, NN, ident, epi);
        }
    }
    if (xa.mode == MODE_NORMS) {
        float t2[2] = {n2, z2};
        block_sums<2>(t2, red);
        if (threadIdx.x == 0) {
            float* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 2;
            o[0] = t2[0];
            o[1] = t2[1];
        }
    }
}

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
// The hodge branch of ScoreNetworkA_CC with ONE HodgeAdjAttentionLayer (ScoreNetwork_A_CC.py:295-316; the oracle's score_network_a_cc),
// k_xa's h_L == 1 branch with the same expressions.  adj_to_hodgedual makes the hodge adjacency of channel c diagonal with the upper
// triangle of the adjacency power c on it (a_c[e] = S[c][i][j], e = (i, j), i < j), DenseHCNConv on a diagonal matrix is a row scaling
// of the layer-0 projection P_0 = F Wcat_0 ([B][E][wc], left by the rank-2 side), and hodgedual_to_adj reads only the diagonal of the
// layer's output: everything is arithmetic per edge.  Written at (i, j) and (j, i) of the stack: rows ch0 .. ch0 + cin the hodge
// adjacency a_c itself, the next cout rows 2 tanh(fl^2 mlp_attention(head-mean logits)).  The work items behind the E edges are the N
// diagonal entries of those rows: zero (nothing is scattered there, and the workspace is not cleared).
// grid: (grid-stride over E + N, B)
__global__ __launch_bounds__(CCSD_LG_TB) void k_lg_hodge1(HodgeLayerD h, float rks, const float* __restrict__ w, const unsigned char* __restrict__ edges,
                                                         const float* __restrict__ P0, float* __restrict__ S, long long sstride, int ch0, int N,
                                                         int E, const float* __restrict__ flags) {
    __shared__ float s_hw[CCSD_MAXLIN * CCSD_HWBLK];                  // zero-padded mlp_attention weight blocks
    __shared__ float s_q[CCSD_LG_TB][2 * CCSD_LG_HAD + 1];            // the calling thread's Q | K row of one channel
    const int b = blockIdx.y, NN = N * N, qw = 2 * h.adim;
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
        float in[CCSD_SMALLW], out[CCSD_SMALLW];
#pragma unroll
        for (int c = 0; c < CCSD_SMALLW; ++c) {
            float sacc = 0.f;
            if (c < h.cin) {
                const float a = Sb[(size_t)c * NN + ij];
                const float g = 1.0f / sqrtf(fmaxf(a, 1.f));
                for (int d = 0; d < qw; ++d) q[d] = fmaf(g * a * g, pr[c * qw + d], w[h.bcat + c * qw + d]);
                sacc = attn_logits(q, q + h.adim, h.nchunk, h.dsplit, rks) * (1.0f / (float)h.nchunk);
                Hb[(size_t)c * NN + ij] = a;
                Hb[(size_t)c * NN + ji] = a;
            }
            in[c] = sacc;
        }
        small_mlp_lds<CCSD_SMALLW>(s_hw, h.matt.n, in, out);     // mlp_attention -> mask -> tanh -> + transpose
        const float fh = fl[i] * fl[j];
#pragma unroll
        for (int o = 0; o < CCSD_SMALLW; ++o)
            if (o < h.cout) {
                const float tv = tanh_f(out[o] * fh * fh);
                Hb[(size_t)(h.cin + o) * NN + ij] = tv + tv;
                Hb[(size_t)(h.cin + o) * NN + ji] = tv + tv;
            }
    }
}
#undef LG_PT
#endif  // CCSD_LG_UNIT || CCSD_EMU
