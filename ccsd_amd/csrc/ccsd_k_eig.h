// ccsd_k_eig.h -- k_eigvalsh, k_norm_laplacian, k_hodge_laplacian: the spectral descriptors of finished samples
// Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// Two of the reference's scores are MMDs of eigenvalue spectra: spectral_worker (evaluation/stats.py:125-137: the 200-bin histogram
// of the eigenvalues of the normalised Laplacian of adjs_to_graphs(adj)[b]) and hodge_laplacian_spectrum_worker (cc_utils.py:994-1060:
// the eigenvalues of H = F F^T of the complex's rank-1 / rank-2 incidence matrix).  Both need the eigenvalues of many small dense
// symmetric matrices: k_eigvalsh.  k_norm_laplacian and k_hodge_laplacian build the matrices from what ccsd_finish already reads
// or writes (the adjacency with its quantiser, rank2_cell_bits).
//
// Every kernel here has ONE body: the loops run over `tid, tid + nth, ...` with barriers between the phases, so the host emulation
// (one thread per workgroup, barriers are no-ops) runs the same arithmetic in the same order as the device -- the rotation formula,
// the pairing order and the column-then-row application included.  Only FMA contraction differs between the two compilers.
#pragma once
#include "ccsd_dev.h"
#include "ccsd_k_finish.h"
#include "ccsd_k_eval.h"

#ifndef CCSD_EIG_MAXN
#define CCSD_EIG_MAXN 512           // the largest matrix k_eigvalsh takes (include/ccsd_hip.h states the same limit)
#endif
#define CCSD_EIG_LDS_MAXN 128       // up to here the matrix lives in LDS: 128 rows of 129 doubles = 129 KB of the CU's 160 KB
#define CCSD_EIG_MAX_SWEEPS 30      // compile-time bound of the sweep loop (a converging input ends in 5 to 9)
#ifndef CCSD_EIG_MAX_GRID           // workgroups (so workspace slabs) of the workspace-resident placement: one per CU.  The host emulation
#ifdef CCSD_EMU                     // walks with two, so that a batch of three already reuses a slab (its workgroups run one after the other)
#define CCSD_EIG_MAX_GRID 2
#else
#define CCSD_EIG_MAX_GRID 256
#endif
#endif
#define CCSD_EIG_THREADS 1024
// row stride in doubles, odd: a walk with one row per lane (the norms, the diagonal) then touches every LDS bank once (the rule
// ccsd_k_eval.h states for 8-byte reads); the workspace slabs use the same stride so the two placements share every index
CCSD_DEV int eig_ld(int nmax) { return nmax | 1; }

// The Jacobi rotation that annihilates a_pq (Rutishauser's form): t = tan(phi) is the smaller root of t^2 + 2 theta t - 1 = 0,
// theta = (a_qq - a_pp) / (2 a_pq).  theta is never squared when it is large (a_pq tiny against the diagonal gap: theta^2 overflows
// from |theta| = 2^512 on): there t = 1 / (2 theta), which is what the root rounds to anyway.  theta = +-inf gives t = 0.
CCSD_DEV void eig_rotation(double app, double aqq, double apq, double* c, double* s) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = fabs(theta);
    double t = at < 0x1p+500 ? 1.0 / (at + sqrt(at * at + 1.0)) : 0.5 / at;
    if (theta < 0.0) t = -t;
    const double cc = 1.0 / sqrt(t * t + 1.0);
    *c = cc;
    *s = t * cc;
}

// Round-robin (tournament) pairing of m players, m even: round r = 0..m-2, pair k = 0..m/2-1.  Player m - 1 stays, the others
// turn on a circle: every round is m / 2 disjoint pairs and the m - 1 rounds meet every pair once.  p < q.
CCSD_DEV void eig_pair(int m, int r, int k, int* p, int* q) {
    int a, b;
    if (k == 0) { a = m - 1; b = r; }
    else { a = (r + k) % (m - 1); b = (r + m - 1 - k) % (m - 1); }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// the bin of np.histogram(v, bins, range=(edges[0], edges[bins])) for edges[0] <= v <= edges[bins]: numpy's estimate-and-correct
// over its linspace edges, as eval_cluster_bin -- the largest i with edges[i] <= v, the last bin closed
CCSD_DEV int eig_bin(double v, const double* __restrict__ edges, int bins) {
    int i = (int)((v - edges[0]) / (edges[bins] - edges[0]) * (double)bins);
    if (i > bins - 1) i = bins - 1;
    if (i < 0) i = 0;
    while (i > 0 && v < edges[i]) --i;
    while (i < bins - 1 && v >= edges[i + 1]) ++i;
    return i;
}

// ---------------------------------------------------------------------------------------------
// k_eigvalsh: eigenvalues only of B symmetric fp64 matrices, parallel cyclic two-sided Jacobi, one workgroup per matrix at a time.
//   a        matrix b at a + b a_stride, row stride lda, order n_b = n_arr ? n_arr[b] : nmax (1 <= n_b <= nmax <= CCSD_EIG_MAXN); not modified
//   w   (B, nmax) fp64      the n_b eigenvalues ascending, the rest zero                       (nullable)
//   w32 (B, nmax) fp32      the same, rounded to fp32 once                                      (nullable)
//   sweeps (B,) int32       sweeps used (0 for a diagonal matrix), or -CCSD_EIG_MAX_SWEEPS if the cap ended the loop   (nullable)
//   hist (B, bins) int32    np.histogram(w, bins, range=(edges[0], edges[bins])) of the n_b eigenvalues, each CLAMPED to
//                           [0, edges[bins]] first (nullable; edges: bins + 1 doubles, bins <= CCSD_EVAL_MAXBINS).  The clamp is the one
//                           deliberate difference from spectral_worker: [0, 2] is the exact range of a normalised Laplacian's
//                           spectrum, a bipartite component has the eigenvalue 2 exactly, and LAPACK returns it as 2 - 2e-16, 2.0 or
//                           2 + 4e-16 depending on the graph -- np.histogram drops the last.  Here it always counts in the last bin.
// A sweep is m - 1 rounds (m = n_b rounded up to even: an odd order plays with a dummy index whose pairs are skipped); a round is
// m / 2 disjoint rotations in three phases with a barrier after each:
//   1. (c, s) per pair from a_pp, a_qq, a_pq (the upper triangle); a_pq == 0 is skipped
//   2. the columns p, q of every row:  a_ip' = c a_ip - s a_iq,  a_iq' = s a_ip + c a_iq     (lanes along the pairs k of one row: the
//      pairing puts (r + k) mod (m - 1) against (r - k) mod (m - 1), so consecutive pairs touch consecutive columns, one run upwards and
//      one downwards -- contiguous in LDS and in the workspace slab alike)
//   3. the rows p, q of every column, same form (lanes along j: contiguous); a_pq and a_qp are then SET to zero
// The sweep loop ends when off(A) <= n 2^-53 ||A||_F (rounding level: a bare 2^-52 ||A||_F is not reached when eigenvalues repeat),
// when a whole sweep applied no rotation, or at the cap; there is no data-dependent unbounded loop, and a NaN fails the `>` test
// and leaves at once.  The norms are summed row by row (one thread per row, ascending j) and then over the rows by thread 0: the
// same order for every launch shape.  The sorted output is a rank sort of the diagonal (ties by index).
//
// IN_LDS: the matrix is the dynamic LDS block (nmax <= CCSD_EIG_LDS_MAXN, grid = B).  Otherwise it is slab blockIdx.x of `slabs`
// (nmax (nmax | 1) doubles each, grid <= CCSD_EIG_MAX_GRID workgroups walking the batch): the slab is written and read by one
// workgroup only, between its own barriers, and is small enough to stay in L2 (2 MB at n = 512).  Every round reads and writes the
// whole matrix twice with a barrier between dependent passes; whether that placement is bound by L2 latency or by the barriers has
// not been measured with counters (DESIGN section 6 holds the times).
// Range: the two norms are sums of plain squares, so the stopping test needs ||A||_F^2 to be a normal fp64 number: entries between
// about 1e-150 and 1e+150 in magnitude (zeros aside).  Below, the squares underflow and the diagonal is returned unsolved with
// sweeps = 0; above, they overflow and the loop leaves at once likewise.  Scale such a matrix by a power of two first.
// ---------------------------------------------------------------------------------------------
template <bool IN_LDS>
__global__ __launch_bounds__(CCSD_EIG_THREADS) void k_eigvalsh(const double* __restrict__ a, int B, int nmax, long long a_stride, int lda,
                                                               const int* __restrict__ n_arr, double* slabs, double* __restrict__ w,
                                                               float* __restrict__ w32, int* __restrict__ sweeps,
                                                               const double* __restrict__ edges, int bins, int* __restrict__ hist) {
    CCSD_DYN_SMEM(sm);
    __shared__ double s_c[CCSD_EIG_MAXN / 2], s_s[CCSD_EIG_MAXN / 2];
    __shared__ double s_d[CCSD_EIG_MAXN], s_t[CCSD_EIG_MAXN];
    __shared__ double s_sum;
    __shared__ int s_p[CCSD_EIG_MAXN / 2], s_q[CCSD_EIG_MAXN / 2];
    __shared__ int s_hist[CCSD_EVAL_MAXBINS];
    __shared__ int s_rot;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int LD = eig_ld(nmax);
    double* S = IN_LDS ? reinterpret_cast<double*>(sm) : slabs + (size_t)blockIdx.x * nmax * LD;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        int n = n_arr ? n_arr[b] : nmax;
        n = n < 1 ? 1 : n > nmax ? nmax : n;
        const int m = (n + 1) & ~1, np = m >> 1;
        const double* Ab = a + (size_t)b * a_stride;
        __syncthreads();                                   // (the previous matrix's epilogue is done with the shared arrays)
        for (int idx = tid; idx < n * n; idx += nth) {
            const int i = idx / n, j = idx - i * n;
            S[i * LD + j] = Ab[(size_t)i * lda + j];
        }
        __syncthreads();
        // ||A||_F^2
        for (int i = tid; i < n; i += nth) {
            double r = 0.0;
            for (int j = 0; j < n; ++j) r += S[i * LD + j] * S[i * LD + j];
            s_t[i] = r;
        }
        __syncthreads();
        if (tid == 0) {
            double r = 0.0;
            for (int i = 0; i < n; ++i) r += s_t[i];
            s_sum = r;
        }
        __syncthreads();
        const double fro2 = s_sum;
        const double tol = (double)n * 0x1p-53;
        const double thr2 = tol * tol * fro2;
        int used = 0;
        bool capped = false;
        for (int sweep = 0;; ++sweep) {
            // off(A)^2
            __syncthreads();                               // (s_sum was read by everyone)
            for (int i = tid; i < n; i += nth) {
                double r = 0.0;
                for (int j = 0; j < n; ++j)
                    if (j != i) r += S[i * LD + j] * S[i * LD + j];
                s_t[i] = r;
            }
            __syncthreads();
            if (tid == 0) {
                double r = 0.0;
                for (int i = 0; i < n; ++i) r += s_t[i];
                s_sum = r;
                s_rot = 0;
            }
            __syncthreads();
            if (!(s_sum > thr2)) break;                    // converged (or not a number)
            if (sweep == CCSD_EIG_MAX_SWEEPS) { capped = true; break; }
            for (int r = 0; r < m - 1; ++r) {
                for (int k = tid; k < np; k += nth) {
                    int p, q;
                    eig_pair(m, r, k, &p, &q);
                    s_p[k] = -1;
                    if (q < n) {
                        const double apq = S[p * LD + q];
                        if (apq != 0.0) {
                            double c, s;
                            eig_rotation(S[p * LD + p], S[q * LD + q], apq, &c, &s);
                            s_p[k] = p; s_q[k] = q; s_c[k] = c; s_s[k] = s;
                            s_rot = 1;                     // (every writer stores the same value)
                        }
                    }
                }
                __syncthreads();
                for (int idx = tid; idx < np * n; idx += nth) {
                    const int i = idx / np, k = idx - i * np, p = s_p[k];
                    if (p < 0) continue;
                    const int q = s_q[k];
                    const double c = s_c[k], s = s_s[k], x = S[i * LD + p], y = S[i * LD + q];
                    S[i * LD + p] = c * x - s * y;
                    S[i * LD + q] = s * x + c * y;
                }
                __syncthreads();
                for (int idx = tid; idx < np * n; idx += nth) {
                    const int k = idx / n, j = idx - k * n, p = s_p[k];
                    if (p < 0) continue;
                    const int q = s_q[k];
                    const double c = s_c[k], s = s_s[k], x = S[p * LD + j], y = S[q * LD + j];
                    S[p * LD + j] = j == q ? 0.0 : c * x - s * y;
                    S[q * LD + j] = j == p ? 0.0 : s * x + c * y;
                }
                __syncthreads();
            }
            ++used;
            if (!s_rot) break;                             // (s_rot is next written after the barrier at the top of the loop)
        }
        // the diagonal, ascending
        for (int i = tid; i < n; i += nth) s_d[i] = S[i * LD + i];
        for (int i = tid; i < bins; i += nth) s_hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += nth) {
            const double v = s_d[i];
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += (s_d[j] < v || (s_d[j] == v && j < i)) ? 1 : 0;
            s_t[rank] = v;                                 // (a NaN collides with other ranks but stays below n)
            if (hist) {
                const double top = edges[bins];
                finish_inc(&s_hist[eig_bin(v < 0.0 ? 0.0 : v > top ? top : v, edges, bins)]);
            }
        }
        __syncthreads();
        for (int i = tid; i < nmax; i += nth) {
            const double v = i < n ? s_t[i] : 0.0;
            if (w) w[(size_t)b * nmax + i] = v;
            if (w32) w32[(size_t)b * nmax + i] = (float)v;
        }
        if (hist)
            for (int i = tid; i < bins; i += nth) hist[(size_t)b * bins + i] = s_hist[i];
        if (sweeps && tid == 0) sweeps[b] = capped ? -CCSD_EIG_MAX_SWEEPS : used;
    }
}

// ---------------------------------------------------------------------------------------------
// k_norm_laplacian: one workgroup per graph over adj (B, N, N) fp32, 2 <= N <= CCSD_FIN_MAXN
//   lap (B, N, N) fp64   the n_eff x n_eff matrix L = I - D^-1/2 A D^-1/2 of nx.normalized_laplacian_matrix(adjs_to_graphs(adj_int)[b]),
//                        row stride N, in the upper left corner (the rest is not written)
//   n_eff (B,) int32     its order
// The weights are the quantised values w_ij = finish_quant(adj[i][j], thr), j != i (0/1, or the bond orders 1..3 in mol mode, which
// nx.from_numpy_array keeps as edge weights); the diagonal is ignored (self loops are removed) and only ROW i is read for node i: a
// symmetric adjacency is the contract, as for k_cluster_hist.  d_i = sum_j w_ij; the nodes with d_i > 0 are compacted to the front
// in index order (isolated and masked nodes are removed), L_ij = delta_ij - w_ij / sqrt(d_i d_j) with IEEE sqrt and division.  A
// graph without any edge is replaced by one node: n_eff = 1, L = [0].
// ---------------------------------------------------------------------------------------------
__global__ void k_norm_laplacian(const float* __restrict__ adj, int N, float thr, double* __restrict__ lap, int* __restrict__ n_eff) {
    const int b = blockIdx.x;
    const float* Ab = adj + (size_t)b * N * N;
    double* Lb = lap + (size_t)b * N * N;
    __shared__ int s_deg[CCSD_FIN_MAXN], s_pos[CCSD_FIN_MAXN];
    __shared__ int s_n;
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int i = tid; i < N; i += nth) {
        int d = 0;
        for (int j = 0; j < N; ++j)
            if (j != i) d += finish_quant(Ab[(size_t)i * N + j], thr);
        s_deg[i] = d;
    }
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int i = 0; i < N; ++i) s_pos[i] = s_deg[i] > 0 ? c++ : -1;
        s_n = c;
    }
    __syncthreads();
    const int ne = s_n;
    if (ne == 0) {
        if (tid == 0) { Lb[0] = 0.0; n_eff[b] = 1; }
        return;
    }
    for (int idx = tid; idx < N * N; idx += nth) {
        const int i = idx / N, j = idx - i * N, pi = s_pos[i], pj = s_pos[j];
        if (pi < 0 || pj < 0) continue;
        const int wij = j != i ? finish_quant(Ab[idx], thr) : 0;
        Lb[(size_t)pi * N + pj] = (i == j ? 1.0 : 0.0) - (double)wij / sqrt((double)s_deg[i] * (double)s_deg[j]);
    }
    if (tid == 0) n_eff[b] = ne;
}

// ---------------------------------------------------------------------------------------------
// k_hodge_laplacian: one workgroup per complex -> H (B, E, E) fp64, E = N (N - 1) / 2 <= CCSD_EIG_MAXN (N <= 32), ZERO on entry
// H = F F^T of the incidence matrix CC_to_incidence_matrices gives back for cc_from_incidence(quantised sample) (cc_utils.py:
// 265-330, 199-262): F[e][k] = 1 iff cell k is present (bit k of cell_bits: some entry of column k of the quantised rank2 is set),
// both nodes of edge e lie in cell k, and edge e is in the quantised adjacency.  So H[e][e'] = the number of present cells that hold
// both edges, 0 unless both edges are in the graph: for every present cell, the edges of its C(d, 2) node pairs that are in the graph
// are listed and 1.0 is added at every ordered pair of the list, the diagonal included.  Sums of 1.0 in fp64 are exact integers
// whatever their order; within a cell every thread owns distinct entries and the cells are taken one after the other, so there is no
// atomic either: the result is bit-reproducible.
// Column k names its nodes as get_cells does (cc_utils.py:72-94): sizes d_min..d_max, itertools.combinations(range(N), d) order
// within a size -- unranked here per set bit (thread 0; absent cells cost nothing but the scan of the mask words).
// Edge (i, j), i < j, has the row index i (2 N - i - 1) / 2 + j - i - 1; the spectrum of H does not depend on the edge order.
// An edge is present when finish_quant(adj[i][j], thr) != 0, read from row i = the smaller index (symmetric adjacency).
// ---------------------------------------------------------------------------------------------
#define CCSD_EIG_HODGE_MAXN 32
CCSD_DEV long long eig_comb(int n, int k) {
    if (k < 0 || k > n) return 0;
    if (k > n - k) k = n - k;
    long long r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;       // (C(n - k + i, i) after step i: every division is exact)
    return r;
}
__global__ void k_hodge_laplacian(const float* __restrict__ adj, const unsigned long long* __restrict__ cell_bits, int N, int d_min,
                                  int d_max, int K, float thr, double* __restrict__ H) {
    const int b = blockIdx.x, W = (K + 63) >> 6, E = N * (N - 1) / 2;
    const float* Ab = adj + (size_t)b * N * N;
    double* Hb = H + (size_t)b * E * E;
    __shared__ int s_nodes[CCSD_EIG_HODGE_MAXN];
    __shared__ int s_e[CCSD_EIG_MAXN];
    __shared__ int s_dk;
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int wd = 0; wd < W; ++wd) {
        unsigned long long bw = cell_bits[(size_t)b * W + wd];       // (the same word in every thread: the loops below are uniform)
        while (bw) {
            const int k = (wd << 6) + __builtin_ctzll(bw);
            bw &= bw - 1;
            if (k >= K) break;
            __syncthreads();                                         // (the previous cell's pairs are done with s_e)
            if (tid == 0) {
                long long r = k;
                int d = d_min;
                for (; d < d_max; ++d) {
                    const long long cnt = eig_comb(N, d);
                    if (r < cnt) break;
                    r -= cnt;
                }
                int x = 0;
                for (int pos = 0; pos < d; ++pos)
                    for (;; ++x) {
                        const long long cnt = eig_comb(N - x - 1, d - pos - 1);
                        if (r < cnt || x >= N - (d - pos)) { s_nodes[pos] = x++; break; }      // (x stays a valid node whatever k)
                        r -= cnt;
                    }
                s_dk = d;
            }
            __syncthreads();
            const int d = s_dk, P = d * (d - 1) / 2;
            for (int idx = tid; idx < P; idx += nth) {               // pair idx = (u, v), u < v, of the cell's nodes
                int u = 0, rem = idx;
                while (rem >= d - 1 - u) { rem -= d - 1 - u; ++u; }
                const int i = s_nodes[u], j = s_nodes[u + 1 + rem];  // (i < j: the nodes ascend)
                s_e[idx] = finish_quant(Ab[(size_t)i * N + j], thr) != 0 ? i * (2 * N - i - 1) / 2 + j - i - 1 : -1;
            }
            __syncthreads();
            for (int idx = tid; idx < P * P; idx += nth) {
                const int ea = s_e[idx / P], eb = s_e[idx % P];
                if (ea >= 0 && eb >= 0) Hb[(size_t)ea * E + eb] += 1.0;
            }
        }
    }
}
