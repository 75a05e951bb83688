// ccsd_k_lift.h -- k_lift_paths, k_lift_cycles, k_lift_dense: graphs lifted to combinatorial complexes (rank-2 cells from paths or from a
// cycle basis).  Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// The reference turns graphs into complexes with convert_graphs_to_CCs (cc_utils.py:816-880): path_based_lift_CC (cc_utils.py:1692-1724)
// adds the node set of every path of `path_length` nodes that starts at a source node, cycles_lift_CC (cc_utils.py:1727-1754) the node set
// of every cycle of networkx.cycle_basis.  The kernels here give the result in the sparse form ccsd_finish writes and ccsd_hodge_spectrum
// reads: bit k of rank2_cell_bits = column k of the rank-2 incidence matrix holds a cell, with the per-complex counters beside it.
//
// The graph: nodes 0..N-1, N <= 64, so a row of the adjacency is ONE 64-bit mask.  Pair (i, j), i < j, is an edge when
// finish_quant(adj[i][j], thr) != 0, read from row i = the smaller index exactly as k_hodge_laplacian reads it; the diagonal and the lower
// triangle are never read.  Column k names its nodes as get_cells does (cc_utils.py:72-94): sizes d_min..d_max, within a size the order of
// itertools.combinations(range(N), d).
//
// path_based, path_length 3: {a, b, c} is a cell iff some node of the three is adjacent to the other two and one of those two is a source.
// cycles: networkx.cycle_basis(networkx.from_numpy_array(A)), restated in lift_cycle_walk below; each cycle reduced to its node set.
// Incidence (create_incidence_1_2, cc_utils.py:265-330): F[e][k] = 1 iff column k is a cell and edge e of the graph lies inside it.
#pragma once
#include "ccsd_dev.h"
#include "ccsd_k_finish.h"
#include "ccsd_k_eig.h"

#define CCSD_LIFT_MAXN 64
#define CCSD_LIFT_WPW 16                              // k_lift_paths: consecutive output words per wave
#define CCSD_LIFT_WPG (4 * CCSD_LIFT_WPW)            // ... and per workgroup (four waves)
#define CCSD_LIFT_DENSE_WPG 1024                      // k_lift_dense: words per workgroup

// the N mask rows of one graph -> LDS: a wave per row, one ballot per row (the emulation's one thread takes the entries in turn)
CCSD_DEV void lift_masks(const float* __restrict__ Ab, int N, float thr, unsigned long long* s_mask) {
#ifdef CCSD_EMU
    for (int i = 0; i < N; ++i) {
        unsigned long long m = 0;
        for (int j = 0; j < N; ++j)
            if (j != i && finish_quant(Ab[(size_t)(i < j ? i : j) * N + (i < j ? j : i)], thr) != 0) m |= 1ull << j;
        s_mask[i] = m;
    }
#else
    const int wave = wave_index(), lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    for (int i = wave; i < N; i += nw) {
        const int j = lane;
        const bool on = j < N && j != i && finish_quant(Ab[(size_t)(i < j ? i : j) * N + (i < j ? j : i)], thr) != 0;
        const unsigned long long m = __ballot(on);
        if (lane == 0) s_mask[i] = m;
    }
#endif
}

// entry r of itertools.combinations(range(N), 3), 0 <= r < C(N, 3)
CCSD_DEV void lift_unrank3(int N, int r, int& a, int& b, int& c) {
    a = 0;
    for (;;) {
        const int cnt = (N - a - 1) * (N - a - 2) / 2;
        if (r < cnt) break;
        r -= cnt;
        ++a;
    }
    b = a + 1;
    for (;;) {
        const int cnt = N - b - 1;
        if (r < cnt) break;
        r -= cnt;
        ++b;
    }
    c = b + 1 + r;
}
// s > 0 entries further in that order; the caller knows that the entry exists.  (a, b) is followed by N - 1 - b entries: one turn of the
// loop per run of c that the step crosses, about 3 s / N of them.
CCSD_DEV void lift_step3(int N, int s, int& a, int& b, int& c) {
    c += s;
    while (c >= N) {
        const int over = c - N;
        ++b;
        if (b >= N - 1) { ++a; b = a + 1; }
        c = b + 1 + over;
    }
}
// the path rule for {a, b, c}, a < b < c: 0 = no cell, otherwise the edges of the graph inside the cell (2 or 3)
CCSD_DEV int lift_path_cell(const unsigned long long* s_mask, unsigned long long sources, int a, int b, int c) {
    const unsigned long long ma = s_mask[a], mb = s_mask[b];
    const int ab = (int)((ma >> b) & 1), ac = (int)((ma >> c) & 1), bc = (int)((mb >> c) & 1);
    const int sa = (int)((sources >> a) & 1), sb = (int)((sources >> b) & 1), sc = (int)((sources >> c) & 1);
    const int cell = (ab & ac & (sb | sc)) | (ab & bc & (sa | sc)) | (ac & bc & (sa | sb));
    return cell ? ab + ac + bc : 0;
}
// One lane's walk over the words [w0, w1) of its wave: column 64 w + lane of word w, i.e. entry r = 64 w + lane - off3 of the size-3
// block (columns of the other sizes hold no path cell).  The first entry in range is unranked, every later one is a step of 64.
struct LiftLane {
    int r, a, b, c;
    bool have;
};
CCSD_DEV void lift_lane_start(LiftLane& s, int w0, int lane, int off3) { s.r = 64 * w0 + lane - off3; s.have = false; s.a = s.b = s.c = 0; }
CCSD_DEV int lift_lane_word(LiftLane& s, int N, int C3, const unsigned long long* s_mask, unsigned long long sources) {
    int ne = 0;
    if (s.r >= 0 && s.r < C3) {
        if (!s.have) { lift_unrank3(N, s.r, s.a, s.b, s.c); s.have = true; }
        ne = lift_path_cell(s_mask, sources, s.a, s.b, s.c);
    }
    if (s.have) {
        if (s.r + 64 < C3) lift_step3(N, 64, s.a, s.b, s.c);
        else s.have = false;                                             // (r only grows: never in range again)
    }
    s.r += 64;
    return ne;
}

// ---------------------------------------------------------------------------------------------
// k_lift_paths: grid (B, ceil(W / CCSD_LIFT_WPG)), 256 threads: a workgroup owns CCSD_LIFT_WPG consecutive words of one graph's bit row, each
// of its four waves CCSD_LIFT_WPW of them; lane l of a wave holds column 64 w + l and the ballot of the lanes IS word w.
//   bits (B, W) uint64        every word written (a plain store per word: no word has two owners), tail bits 0
//   cell_count (B,), cell_hist (B, nb) at bin3, nnz (B,)   ZERO on entry (ccsd_lift clears them on the stream): one atomicAdd each per
//                             workgroup; nullable
// off3 = the first column of size 3, C3 = C(N, 3).
// ---------------------------------------------------------------------------------------------
__global__ void k_lift_paths(const float* __restrict__ adj, int N, float thr, unsigned long long sources, int W, int off3, int C3, int nb,
                             int bin3, unsigned long long* __restrict__ bits, int* __restrict__ cell_count, int* __restrict__ cell_hist,
                             int* __restrict__ nnz) {
    const int b = blockIdx.x, wg0 = blockIdx.y * CCSD_LIFT_WPG;
    __shared__ unsigned long long s_mask[CCSD_LIFT_MAXN];
    __shared__ int s_cnt[2];
    lift_masks(adj + (size_t)b * N * N, N, thr, s_mask);
    for (int i = threadIdx.x; i < 2; i += blockDim.x) s_cnt[i] = 0;
    __syncthreads();
    unsigned long long* Bb = bits + (size_t)b * W;
#ifdef CCSD_EMU
    for (int wave = 0; wave < 4; ++wave) {
        const int w0 = wg0 + wave * CCSD_LIFT_WPW, w1 = w0 + CCSD_LIFT_WPW < W ? w0 + CCSD_LIFT_WPW : W;
        unsigned long long acc[CCSD_LIFT_WPW];
        for (int i = 0; i < CCSD_LIFT_WPW; ++i) acc[i] = 0;
        for (int lane = 0; lane < 64; ++lane) {
            LiftLane s;
            lift_lane_start(s, w0, lane, off3);
            for (int w = w0; w < w1; ++w) {
                const int ne = lift_lane_word(s, N, C3, s_mask, sources);
                if (ne) { acc[w - w0] |= 1ull << lane; s_cnt[0] += 1; s_cnt[1] += ne; }
            }
        }
        for (int w = w0; w < w1; ++w) Bb[w] = acc[w - w0];
    }
#else
    const int wave = wave_index(), lane = threadIdx.x & 63;
    const int w0 = wg0 + wave * CCSD_LIFT_WPW, w1 = w0 + CCSD_LIFT_WPW < W ? w0 + CCSD_LIFT_WPW : W;
    LiftLane s;
    lift_lane_start(s, w0, lane, off3);
    int cnt = 0, nz = 0;
    for (int w = w0; w < w1; ++w) {                                      // (wave-uniform bounds: every lane is in the ballot)
        const int ne = lift_lane_word(s, N, C3, s_mask, sources);
        const unsigned long long m = __ballot(ne != 0);
        nz += ne;
        if (lane == 0) {
            Bb[w] = m;
            cnt += __popcll(m);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_xor(nz, o, 64);
    if (lane == 0 && cnt) { atomicAdd(&s_cnt[0], cnt); atomicAdd(&s_cnt[1], nz); }
#endif
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt[0]) {
#ifdef CCSD_EMU
        if (cell_count) cell_count[b] += s_cnt[0];
        if (cell_hist) cell_hist[(size_t)b * nb + bin3] += s_cnt[0];
        if (nnz) nnz[b] += s_cnt[1];
#else
        if (cell_count) atomicAdd(&cell_count[b], s_cnt[0]);
        if (cell_hist) atomicAdd(&cell_hist[(size_t)b * nb + bin3], s_cnt[0]);
        if (nnz) atomicAdd(&nnz[b], s_cnt[1]);
#endif
    }
}

// column of a node set of size d (d_min <= d <= d_max) in get_cells' order: the columns of the smaller sizes, then the set's place among
// itertools.combinations(range(N), d) = C(N, d) - 1 - sum_i C(N - 1 - c_i, d - i) over its nodes c_0 < c_1 < ...
CCSD_DEV int lift_rank(const FinishTab& tab, int N, int d_min, int d, unsigned long long set) {
    long long r = eig_comb(N, d) - 1;
    for (int i = 0; set; ++i) {
        const int c = __builtin_ctzll(set);
        set &= set - 1;
        r -= eig_comb(N - 1 - c, d - i);
    }
    return (int)r + (d > d_min ? tab.end[d - d_min - 1] : 0);
}
// ... and back: the node set of column k < K, its size in *d
CCSD_DEV unsigned long long lift_unrank(const FinishTab& tab, int N, int d_min, int k, int* d_out) {
    const int bin = finish_bin(tab, k), d = d_min + bin;
    long long r = k - (bin ? tab.end[bin - 1] : 0);
    unsigned long long set = 0;
    if (d == 3) {
        int a, b, c;
        lift_unrank3(N, (int)r, a, b, c);
        set = (1ull << a) | (1ull << b) | (1ull << c);
    } else {
        int x = 0;
        for (int pos = 0; pos < d; ++pos)
            for (;; ++x) {
                const long long cnt = eig_comb(N - x - 1, d - pos - 1);
                if (r < cnt || x >= N - (d - pos)) { set |= 1ull << x++; break; }      // (x stays a valid node whatever k)
                r -= cnt;
            }
    }
    *d_out = d;
    return set;
}
// the edges of the graph inside a node set
CCSD_DEV int lift_edges_in(const unsigned long long* s_mask, unsigned long long set) {
    int t = 0;
    for (unsigned long long m = set; m; m &= m - 1) t += __builtin_popcountll(s_mask[__builtin_ctzll(m)] & set);
    return t >> 1;
}

// ---------------------------------------------------------------------------------------------
// k_lift_cycles: one wave per graph; the lanes build the mask rows, then lane 0 walks.  bits (B, W), cell_count, cell_hist (B, nb), nnz and
// dropped are ZERO on entry (ccsd_lift clears them on the stream); all but bits nullable.
// networkx.cycle_basis, restated: the components are taken in descending order of their highest node, which is the root.  A LIFO stack
// walk from the root with pred[root] = root, used[root] = {}: pop z, visit its neighbours in ascending order; a new neighbour n is pushed
// with pred[n] = z, used[n] = {z}; a known neighbour n outside used[z] closes the cycle n, z, pred[z], pred[pred[z]], ... up to and
// including the first node in used[n], and used[n] gains z.  Every node is pushed once: the stack holds N entries.  used[] are masks.
// A cycle of d nodes with d_min <= d <= d_max sets the bit of its node set; the lane tests the bit first, so a node set reached twice
// counts once in cell_count, cell_hist and nnz.  A cycle of any other size has no column: it counts in dropped[b].
// ---------------------------------------------------------------------------------------------
__global__ void k_lift_cycles(const float* __restrict__ adj, int N, float thr, FinishTab tab, int d_min, int d_max, int W,
                              unsigned long long* bits, int* __restrict__ cell_count, int* __restrict__ cell_hist, int* __restrict__ nnz,
                              int* __restrict__ dropped) {
    const int b = blockIdx.x;
    __shared__ unsigned long long s_mask[CCSD_LIFT_MAXN], s_used[CCSD_LIFT_MAXN];
    __shared__ int s_pred[CCSD_LIFT_MAXN], s_stack[CCSD_LIFT_MAXN];
    lift_masks(adj + (size_t)b * N * N, N, thr, s_mask);
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long* Bb = bits + (size_t)b * W;
    unsigned long long known = 0;
    int count = 0, total = 0, drop = 0;
    for (int root = N - 1; root >= 0; --root) {
        if ((known >> root) & 1) continue;
        int sp = 0;
        s_stack[sp++] = root;
        s_pred[root] = root;
        s_used[root] = 0;
        known |= 1ull << root;
        while (sp) {
            const int z = s_stack[--sp];
            const unsigned long long zused = s_used[z];
            for (unsigned long long nbrs = s_mask[z]; nbrs; nbrs &= nbrs - 1) {
                const int n = __builtin_ctzll(nbrs);
                if (!((known >> n) & 1)) {
                    s_pred[n] = z;
                    s_stack[sp++] = n;                                   // (sp < N: a node is pushed when it becomes known, once)
                    s_used[n] = 1ull << z;
                    known |= 1ull << n;
                } else if (!((zused >> n) & 1)) {
                    const unsigned long long pn = s_used[n];
                    unsigned long long cyc = (1ull << n) | (1ull << z);
                    int p = s_pred[z];
                    for (int steps = 0; steps < N && !((pn >> p) & 1); ++steps) { cyc |= 1ull << p; p = s_pred[p]; }      // (bounded whatever the masks)
                    cyc |= 1ull << p;
                    s_used[n] = pn | (1ull << z);
                    const int d = __builtin_popcountll(cyc);
                    if (d < d_min || d > d_max) { ++drop; continue; }
                    const int k = lift_rank(tab, N, d_min, d, cyc);
                    const unsigned long long old = Bb[k >> 6], bit = 1ull << (k & 63);
                    if (old & bit) continue;
                    Bb[k >> 6] = old | bit;
                    ++count;
                    total += lift_edges_in(s_mask, cyc);
                    if (cell_hist) cell_hist[(size_t)b * tab.nb + (d - d_min)] += 1;
                }
            }
        }
    }
    if (cell_count) cell_count[b] = count;
    if (nnz) nnz[b] = total;
    if (dropped) dropped[b] = drop;
}

// ---------------------------------------------------------------------------------------------
// k_lift_dense: the ones of rank2 (B, E, K) fp32, ZERO on entry (ccsd_lift clears it on the stream), driven from the finished bit words:
// grid (B, ceil(W / CCSD_LIFT_DENSE_WPG)), a thread per word; every set bit is unranked to its node set and 1.0 is stored at (e, k) for the
// edges e of the graph inside the set -- C(d, 2) stores or fewer per cell, nothing per absent cell.  Edge (i, j), i < j, is row
// i (2 N - i - 1) / 2 + j - i - 1, as in k_hodge_laplacian.
// ---------------------------------------------------------------------------------------------
__global__ void k_lift_dense(const float* __restrict__ adj, int N, float thr, FinishTab tab, int d_min, int K, int W,
                             const unsigned long long* __restrict__ bits, float* __restrict__ rank2) {
    const int b = blockIdx.x, w0 = blockIdx.y * CCSD_LIFT_DENSE_WPG, w1 = w0 + CCSD_LIFT_DENSE_WPG < W ? w0 + CCSD_LIFT_DENSE_WPG : W;
    __shared__ unsigned long long s_mask[CCSD_LIFT_MAXN];
    lift_masks(adj + (size_t)b * N * N, N, thr, s_mask);
    __syncthreads();
    const size_t E = (size_t)N * (N - 1) / 2;
    float* Rb = rank2 + (size_t)b * E * K;
    for (int w = w0 + threadIdx.x; w < w1; w += blockDim.x)
        for (unsigned long long word = bits[(size_t)b * W + w]; word; word &= word - 1) {
            const int k = (w << 6) + __builtin_ctzll(word);
            if (k >= K) break;
            int d;
            const unsigned long long set = lift_unrank(tab, N, d_min, k, &d);
            for (unsigned long long mi = set; mi; mi &= mi - 1) {
                const int i = __builtin_ctzll(mi);
                for (unsigned long long mj = s_mask[i] & mi & (mi - 1); mj; mj &= mj - 1) {      // the set's nodes j > i adjacent to i
                    const int j = __builtin_ctzll(mj);
                    Rb[(size_t)(i * (2 * N - i - 1) / 2 + j - i - 1) * K + k] = 1.0f;
                }
            }
        }
}
