// ccsd_k_eval.h -- k_cluster_hist, k_mmd_prep, k_mmd_pairs, k_mmd_final: the evaluation of finished samples
// Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// After sampling the reference scores the samples against a held-out set with MMDs of per-graph histograms: eval_graph_list ->
// degree_stats / clustering_stats -> compute_mmd (evaluation/stats.py:36-310, evaluation/mmd.py:27-257) and eval_CC_list ->
// rank1_distrib_stats / rank2_distrib_stats (cc_utils.py:1208-1474).  ccsd_finish already gives the degree, edge-value and cell-size
// histograms; k_cluster_hist adds the clustering-coefficient histogram (clustering_worker, stats.py:206-220), and the three k_mmd_*
// kernels are compute_mmd itself.  The reference's EMD ground distance is toeplitz(range(L)) / distance_scaling (mmd.py:47-48), a line
// metric, on which the EMD of two pmfs of equal mass is sum |cdf_x - cdf_y| / distance_scaling: no linear program is solved.
// The MMD arithmetic is fp64 throughout, summed in a fixed order without floating-point atomics: a call is bit-reproducible.
#pragma once
#include "ccsd_dev.h"
#include "ccsd_k_finish.h"

// ---------------------------------------------------------------------------------------------
// k_cluster_hist: one workgroup per graph over adj (B, N, N) fp32, 2 <= N <= CCSD_FIN_MAXN, 1 <= bins <= CCSD_EVAL_MAXBINS
//   tri2 (B, N) int32            t2(i) = sum over neighbours j of |N(i) & N(j)|: twice the triangles through i, the numerator of
//                                nx.clustering (0 for isolated and masked slots)
//   cluster_hist (B, bins) int32 np.histogram(list(nx.clustering(G).values()), bins, range=(0, 1)) of G = adjs_to_graphs(adj_int)[b]
// Both nullable.  An edge i -- j is finish_quant(adj[i][j], thr) != 0 with j != i: the diagonal is ignored, raw samples, quantised
// samples and 0/1 data sets all pass through the one quantiser.  Only ROW i is read for node i, as k_finish_graph's degree does:
// a SYMMETRIC adjacency is the contract (finished samples and data sets are symmetric).
// Node rules of adjs_to_graphs (graph_utils.py:245-250): nodes of degree 0 are removed (not counted), nodes of degree 1 have c = 0
// (bin 0), a graph without any edge is replaced by one node (one count in bin 0).
// Binning is numpy's: c = (double)t2 / (double)(d (d - 1)) by IEEE division, bin = the largest i with edges[i] <= c, the last bin
// closed at 1; `edges` is the host's np.linspace(0, 1, bins + 1) (bins + 1 doubles, device).  Integer arithmetic such as
// floor(bins t2 / (d (d - 1))) is NOT the same function: ten of linspace's 101 edges are not the correctly rounded i / 100, and a node of
// degree 5 in 7 triangles (c = 0.7) belongs to bin 69.
//
// The rows are packed into bit masks in LDS (N rows of ceil(N / 64) 64-bit words: one ballot per 64 entries), so a pair (i, j) costs
// ceil(N / 64) and-popcounts.  A wave takes node i, its lanes the candidate neighbours j = lane, lane + 64, ...: row i is a broadcast
// read, row j an 8-byte read per lane at a stride of WS words.  ds_read_b64 banks by (address / 4) % 64 over each 32-lane half, so the
// stride in 8-byte words has to be odd: WS = W | 1 (36 KB at N = 512).
// ---------------------------------------------------------------------------------------------
#define CCSD_EVAL_MAXBINS 1024
#define CCSD_EVAL_MAXW ((CCSD_FIN_MAXN + 63) / 64)

// the bin of np.histogram(c, bins, range=(0, 1)) for 0 <= c <= 1: numpy's own estimate-and-correct over its linspace edges
CCSD_DEV int eval_cluster_bin(double c, const double* __restrict__ edges, int bins) {
    int i = (int)(c * (double)bins);
    if (i > bins - 1) i = bins - 1;
    while (i > 0 && c < edges[i]) --i;
    while (i < bins - 1 && c >= edges[i + 1]) ++i;
    return i;
}
CCSD_DEV double eval_cluster_coef(int t2, int d) { return d < 2 ? 0.0 : (double)t2 / (double)((long long)d * (d - 1)); }

__global__ void k_cluster_hist(const float* __restrict__ adj, int N, float thr, const double* __restrict__ edges, int bins,
                               int* __restrict__ tri2, int* __restrict__ cluster_hist) {
    const int b = blockIdx.x, W = (N + 63) >> 6, WS = W | 1;
    const float* Ab = adj + (size_t)b * N * N;
    __shared__ unsigned long long s_mask[CCSD_FIN_MAXN * (CCSD_EVAL_MAXW | 1)];
    __shared__ int s_hist[CCSD_EVAL_MAXBINS];
    __shared__ int s_nodes;
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int i = tid; i < bins; i += nth) s_hist[i] = 0;
    if (tid == 0) s_nodes = 0;
#ifdef CCSD_EMU
    for (int i = 0; i < N; ++i) {
        for (int w = 0; w < W; ++w) s_mask[i * WS + w] = 0;
        for (int j = 0; j < N; ++j)
            if (j != i && finish_quant(Ab[(size_t)i * N + j], thr) != 0) s_mask[i * WS + (j >> 6)] |= 1ull << (j & 63);
    }
    for (int i = 0; i < N; ++i) {
        int d = 0, t2 = 0;
        for (int w = 0; w < W; ++w) d += __builtin_popcountll(s_mask[i * WS + w]);
        for (int j = 0; j < N; ++j)
            if ((s_mask[i * WS + (j >> 6)] >> (j & 63)) & 1)
                for (int w = 0; w < W; ++w) t2 += __builtin_popcountll(s_mask[i * WS + w] & s_mask[j * WS + w]);
        if (tri2) tri2[(size_t)b * N + i] = t2;
        if (d > 0) {
            s_nodes += 1;
            s_hist[eval_cluster_bin(eval_cluster_coef(t2, d), edges, bins)] += 1;
        }
    }
#else
    const int wave = wave_index(), lane = tid & 63, nw = nth >> 6;
    // pass 1: row i -> W mask words, one ballot per 64 entries (the wave-uniform loop bound keeps every lane in the ballot)
    for (int i = wave; i < N; i += nw)
        for (int w = 0; w < W; ++w) {
            const int j = (w << 6) + lane;
            const bool on = j < N && j != i && finish_quant(Ab[(size_t)i * N + j], thr) != 0;
            const unsigned long long m = __ballot(on);
            if (lane == 0) s_mask[i * WS + w] = m;
        }
    __syncthreads();
    // pass 2: node i per wave, candidate neighbours j over the lanes
    for (int i = wave; i < N; i += nw) {
        int d = 0, t2 = 0;
        for (int w = 0; w < W; ++w) {
            const unsigned long long mi = s_mask[i * WS + w];           // (broadcast read)
            d += __popcll(mi);
            if ((mi >> lane) & 1) {
                const int j = (w << 6) + lane;                          // (< N: pass 1 sets no bit at or past N)
                for (int v = 0; v < W; ++v) t2 += __popcll(s_mask[i * WS + v] & s_mask[j * WS + v]);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t2 += __shfl_xor(t2, o, 64);
        if (lane == 0) {
            if (tri2) tri2[(size_t)b * N + i] = t2;
            if (d > 0) {
                atomicAdd(&s_nodes, 1);
                atomicAdd(&s_hist[eval_cluster_bin(eval_cluster_coef(t2, d), edges, bins)], 1);
            }
        }
    }
#endif
    __syncthreads();
    if (cluster_hist)
        for (int i = tid; i < bins; i += nth) cluster_hist[(size_t)b * bins + i] = s_hist[i] + (i == 0 && s_nodes == 0 ? 1 : 0);
}

// ---------------------------------------------------------------------------------------------
// compute_mmd (mmd.py:230-257): mmd = disc(s1, s1) + disc(s2, s2) - 2 disc(s1, s2), disc = the mean of k(x, y) over all pairs,
// k = exp(-dist^2 / (2 sigma^2)) with dist by kind:
//   EVAL_EMD  gaussian_emd (mmd.py:27-86)    sum |cdf_x - cdf_y| / distance_scaling        (rows are pmfs: is_hist only)
//   EVAL_TV   gaussian_tv  (mmd.py:111-131)  0.5 sum |x - y|
//   EVAL_L2   gaussian     (mmd.py:89-108)   sqrt(sum (x - y)^2)
// Rows shorter than L are zero padded, as process_tensor does (mmd.py:380-395): no distance changes.
// A row whose sum is zero stays un-normalised in compute_mmd (mmd.py:251-252).  For TV and L2 that is just a vector of zeros.  For the
// EMD the two masses then differ, and pyemd adds |mass_x - mass_y| times its documented default extra_mass_penalty =
// max(distance_matrix) = (max(len_x, len_y) - 1) / distance_scaling to a flow of zero: both rows zero -> 0, one row zero -> that
// penalty.  len is the length of the caller's ARRAY (emd() sizes its distance matrix by it, mmd.py:45-47).
// ---------------------------------------------------------------------------------------------
enum { EVAL_EMD = 0, EVAL_TV = 1, EVAL_L2 = 2 };
enum { EVAL_F_HIST = 1,      // is_hist: rows are normalised to pmfs (rows of sum zero stay as they are)
       EVAL_F_DEGREE = 2,    // rows are ccsd_finish's degree_hist: bin 0 (isolated and masked slots, which the reference's graphs do not
                             // have) is cleared, a row that is then empty becomes [1] (the one-node stand-in of adjs_to_graphs), and the
                             // row's length is its last non-zero bin + 1, as nx.degree_histogram trims it
       EVAL_F_F32PMF = 4 };  // the pmf is rounded to fp32 before it is widened: what compute_mmd does to the float32 histograms of
                             // rank1_distrib_worker / rank2_distrib_worker (cc_utils.py:1227, 1329)
#define CCSD_EVAL_TILE 64
#define CCSD_EVAL_KC 32

CCSD_DEV double eval_load(const void* h, int is_f64, size_t idx) {
    return is_f64 ? reinterpret_cast<const double*>(h)[idx] : (double)reinterpret_cast<const int*>(h)[idx];
}

// k_mmd_prep: one row per thread.  h (n, L) int32 or fp64 -> op (L, np) fp64, TRANSPOSED (np = n rounded up to the tile: the threads
// of rows n..np-1 write zeros, so the pair kernel stages whole tiles without a row mask, and the stores of a bin are contiguous over
// the threads), mass (np,) int32 0/1 and len (np,) int32.  The operand is the normalised cdf for EVAL_EMD, the pmf (EVAL_F_HIST) or the
// raw row otherwise.  lens (n,) int32, nullable: the caller's array lengths of a ragged set (default: L).  O(n L) next to the pair
// kernel's O(n^2 L).
__global__ void k_mmd_prep(const void* __restrict__ h, int is_f64, const int* __restrict__ lens, int n, int np, int L, int kind, int flags,
                           double* __restrict__ op, int* __restrict__ mass, int* __restrict__ len) {
#ifdef CCSD_EMU
    for (int row = (int)blockIdx.x * 256; row < (int)blockIdx.x * 256 + 256; ++row) {
#else
    {
        const int row = blockIdx.x * blockDim.x + threadIdx.x;
#endif
        if (row < np) {
            if (row >= n) {
                for (int k = 0; k < L; ++k) op[(size_t)k * np + row] = 0.0;
                mass[row] = 0;
                len[row] = 1;
            } else {
                const bool deg = (flags & EVAL_F_DEGREE) != 0;
                const int k0 = deg ? 1 : 0;
                double s = 0.0;
                int last = -1;
                for (int k = k0; k < L; ++k) {
                    const double v = eval_load(h, is_f64, (size_t)row * L + k);
                    s += v;
                    if (v != 0.0) last = k;
                }
                const bool stand_in = deg && last < 0;                 // no node of degree >= 1: the histogram [1]
                if (stand_in) s = 1.0;
                const bool norm = (flags & EVAL_F_HIST) && s != 0.0;
                double c = 0.0;
                for (int k = 0; k < L; ++k) {
                    double v = k < k0 ? 0.0 : eval_load(h, is_f64, (size_t)row * L + k);
                    if (stand_in && k == 0) v = 1.0;
                    if (norm) v = (flags & EVAL_F_F32PMF) ? (double)((float)v / (float)s) : v / s;
                    c += v;
                    op[(size_t)k * np + row] = kind == EVAL_EMD ? c : v;
                }
                mass[row] = s != 0.0 ? 1 : 0;
                len[row] = deg ? (last < 0 ? 1 : last + 1) : (lens ? lens[row] : L);
            }
        }
    }
}

CCSD_DEV double eval_kernel_value(double acc, int kind, double scale, double two_s2, int mx, int my, int lx, int ly) {
    double d;
    if (kind == EVAL_EMD) {
        if (mx != my) d = (double)((lx > ly ? lx : ly) - 1) / scale;
        else d = mx ? acc / scale : 0.0;
    } else if (kind == EVAL_TV) {
        d = acc / 2.0;
    } else {
        d = sqrt(acc);
    }
    return exp(-d * d / two_s2);                 // (two_s2 = 2 sigma sigma, mmd.py:86)
}

// k_mmd_pairs: sum of k(x_i, y_j) over one 64 x 64 tile of pairs per workgroup -> partial[blockIdx.y * gridDim.x + blockIdx.x].
// X (L, npx), Y (L, npy): k_mmd_prep's operands; grid (npy / 64, npx / 64), 256 threads.  Thread (ty, tx) = (tid / 16, tid % 16) owns the
// pairs (i0 + ty + 16 r, j0 + tx + 16 c), r, c = 0..3.  Both operand tiles are staged through LDS in chunks of CCSD_EVAL_KC bins as
// [bin][64 rows] (32 KB): a stage is 512 contiguous bytes per bin from global memory, and in the inner loop the 16 lanes of a tx group
// read 16 consecutive doubles of Y while the four ty values of a wave read four consecutive doubles of X (everything else is a
// broadcast) -- 8-byte reads without a bank conflict.  The last chunk is masked by k < L, the pad rows by i < nx, j < ny in the sum.
// symmetric != 0 (X is Y): tiles below the diagonal write 0, tiles above it count twice.
// The tile sum is a fixed shuffle tree, then the four waves in order: no atomics, the same bits every run.
__global__ void k_mmd_pairs(const double* __restrict__ X, const int* __restrict__ mass_x, const int* __restrict__ len_x, int nx, int npx,
                            const double* __restrict__ Y, const int* __restrict__ mass_y, const int* __restrict__ len_y, int ny, int npy,
                            int L, int kind, double scale, double two_s2, int symmetric, double* __restrict__ partial) {
    const int T = CCSD_EVAL_TILE;
    const int i0 = blockIdx.y * T, j0 = blockIdx.x * T;
    double* out = partial + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (symmetric && blockIdx.x < blockIdx.y) {
        if (threadIdx.x == 0) *out = 0.0;
        return;
    }
    const double weight = symmetric && blockIdx.x > blockIdx.y ? 2.0 : 1.0;
#ifdef CCSD_EMU
    double sum = 0.0;
    for (int i = i0; i < i0 + T && i < nx; ++i)
        for (int j = j0; j < j0 + T && j < ny; ++j) {
            double acc = 0.0;
            for (int k = 0; k < L; ++k) {
                const double df = X[(size_t)k * npx + i] - Y[(size_t)k * npy + j];
                acc += kind == EVAL_L2 ? df * df : fabs(df);
            }
            sum += eval_kernel_value(acc, kind, scale, two_s2, mass_x[i], mass_y[j], len_x[i], len_y[j]);
        }
    *out = weight * sum;
#else
    __shared__ double s_x[CCSD_EVAL_KC * CCSD_EVAL_TILE], s_y[CCSD_EVAL_KC * CCSD_EVAL_TILE];
    __shared__ double s_part[4];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int kb = 0; kb < L; kb += CCSD_EVAL_KC) {
        const int kc = L - kb < CCSD_EVAL_KC ? L - kb : CCSD_EVAL_KC;
        for (int e = tid; e < kc * T; e += 256) {                        // (i0 + 63 < npx, j0 + 63 < npy: whole tiles)
            const int k = e >> 6, r = e & 63;
            s_x[e] = X[(size_t)(kb + k) * npx + i0 + r];
            s_y[e] = Y[(size_t)(kb + k) * npy + j0 + r];
        }
        __syncthreads();
        if (kind == EVAL_L2) {
            for (int k = 0; k < kc; ++k) {
                double xv[4], yv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { xv[r] = s_x[k * T + ty + 16 * r]; yv[r] = s_y[k * T + tx + 16 * r]; }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) { const double df = xv[r] - yv[c]; acc[r][c] += df * df; }
            }
        } else {
            for (int k = 0; k < kc; ++k) {
                double xv[4], yv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { xv[r] = s_x[k * T + ty + 16 * r]; yv[r] = s_y[k * T + tx + 16 * r]; }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[r][c] += fabs(xv[r] - yv[c]);
            }
        }
        __syncthreads();
    }
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty + 16 * r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx + 16 * c;
            if (i < nx && j < ny) sum += eval_kernel_value(acc[r][c], kind, scale, two_s2, mass_x[i], mass_y[j], len_x[i], len_y[j]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) *out = weight * (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]);
#endif
}

// k_mmd_final: one workgroup.  partial = the tile sums of disc(1, 1) [c11], disc(2, 2) [c22], disc(1, 2) [c12], in this order.
// out[0..3] = disc(1, 1), disc(2, 2), disc(1, 2), mmd.  Thread t adds the partials t, t + nth, ... in order, thread 0 the nth thread
// sums in order: fixed for a given launch shape.
__global__ void k_mmd_final(const double* __restrict__ partial, int c11, int c22, int c12, double n1, double n2, double* __restrict__ out) {
    __shared__ double s_sum[3][256];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int cnt[3] = {c11, c22, c12};
    const double* p = partial;
    for (int q = 0; q < 3; ++q) {
        double s = 0.0;
        for (int i = tid; i < cnt[q]; i += nth) s += p[i];
        s_sum[q][tid] = s;
        p += cnt[q];
    }
    __syncthreads();
    if (tid == 0) {
        double d[3];
        for (int q = 0; q < 3; ++q) {
            double s = 0.0;
            for (int t = 0; t < nth; ++t) s += s_sum[q][t];
            d[q] = s;
        }
        d[0] /= n1 * n1;
        d[1] /= n2 * n2;
        d[2] /= n1 * n2;
        out[0] = d[0];
        out[1] = d[1];
        out[2] = d[2];
        out[3] = d[0] + d[1] - 2.0 * d[2];
    }
}
