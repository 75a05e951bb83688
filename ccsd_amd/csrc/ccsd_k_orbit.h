// ccsd_k_orbit.h -- k_orbit_counts: the 4-node graphlet orbit counts of finished samples (the "orbit" score of the evaluation)
// Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// The reference scores generic graphs with a third MMD, orbit_stats_all (evaluation/stats.py:382-435): per graph, the column sums of the
// per-node orbit counts that the external orca program prints for `node 4`, divided by the node count.  k_orbit_counts gives the same
// integers from the bit-mask rows k_cluster_hist already uses, by a closed form; no program is started and no equation system is solved.
//
// Orbit numbering (ORCA's), with the node's degree inside the graphlet:
//    0 edge               1 3-path end          2 3-path middle      3 triangle
//    4 4-path end         5 4-path inner        6 claw leaf          7 claw centre       8 4-cycle
//    9 paw pendant       10 paw triangle node without the tail      11 paw triangle node with the tail
//   12 diamond degree 2  13 diamond degree 3   14 K4
//
// Closed form.  d(u) = degree, c(u, w) = |N(u) & N(w)|, t(u) = triangles at u, s1(u) = sum over b in N(u) of d(b) - 1.  For a node v of
// degree d with t = t(v), H = the graph induced on N(v) (t edges, own degrees c(a, v)), out(a) = d(a) - 1 - c(a, v), all sums over
// a in N(v) unless stated:
//   T3   = sum over edges a < b of H of |N(v) & N(a) & N(b)|                     (three times the triangles of H)
//   EADJ = sum over edges a < b of H of c(a, b) - 1
//   SP   = sum over w != v of C(c(w, v), 2)   = sum over ALL pairs a < b of N(v) of c(a, b) - 1: a pair of N(v) with the common
//          neighbour w is a pair of N(v) & N(w); the common neighbour v itself is the - 1.  So the sum over NON-adjacent pairs is
//          SP - EADJ and needs no pair loop.
//   n3 = T3 / 3   n2 = sum C(c(a, v), 2) - 3 n3   n1 = t (d - 2) - 2 n2 - 3 n3   n0 = C(d, 3) - n1 - n2 - n3
//   (n_k = the 3-subsets of N(v) that induce k edges: with v they are the claws, paws, diamonds and K4s in which v touches all three)
//   o0 = d   o1 = s1(v) - 2 t   o2 = C(d, 2) - t   o3 = t   o7 = n0   o11 = n1   o13 = n2   o14 = n3
//   o12 = EADJ - 3 n3                                  o8 = (SP - EADJ) - n2
//   o10 = sum c(a, v) out(a) - 2 o12                   o5 = sum (d - 1 - c(a, v)) out(a) - 2 o8
//   o9  = sum t(a) - 2 t - 3 n3 - 2 o12                o6 = sum C(d(a) - 1, 2) - (sum t(a) - 2 t) - n2 - o10
//   o4  = sum (s1(a) - (d - 1)) - 2 t - 2 o9 - 2 o8 - o10 - 2 n2 - 4 o12 - 6 n3
// Each line counts walks or stars from v and removes the ones that close up into a denser graphlet.
//
// Arithmetic is integer and exact, in 64 bits from the per-neighbour terms on: at N = 512 a per-node count reaches C(511, 3) =
// 22 108 415 and a graph sum 11 319 508 480.  Integer sums do not depend on their order, so the graph sums are LDS atomics.
#pragma once
#include "ccsd_dev.h"
#include "ccsd_k_finish.h"
#include "ccsd_k_eval.h"

#define CCSD_NORBITS 15

// the sums of one node v that run over other nodes: every field is a plain sum, so lanes add their own and the wave adds the lanes
struct OrbitSums {
    long long c2, cout, dout, ta, cda2, s1a, eadj, t3, sp;
};
#define CCSD_ORBIT_NSUMS 9

CCSD_DEV int orbit_common(const unsigned long long* __restrict__ ru, const unsigned long long* __restrict__ rw, int W) {
    int c = 0;
    for (int x = 0; x < W; ++x) c += __builtin_popcountll(ru[x] & rw[x]);
    return c;
}

// the terms of neighbour a of v, and of the edges a -- b of H with b > a
CCSD_DEV void orbit_neighbour(OrbitSums& s, const unsigned long long* __restrict__ mask, int WS, int W, int v, int a, int dv,
                              const int* __restrict__ s_d, const int* __restrict__ s_t, const int* __restrict__ s_s1) {
    const unsigned long long* rv = mask + v * WS;
    const unsigned long long* ra = mask + a * WS;
    int c = 0;
    for (int u = 0; u < W; ++u) {
        const unsigned long long m = rv[u] & ra[u];
        c += __builtin_popcountll(m);
        // b > a only: every edge of H once
        unsigned long long mm = u < (a >> 6) ? 0ull : u == (a >> 6) ? m & ~((2ull << (a & 63)) - 1ull) : m;
        while (mm) {
            const int b = (u << 6) + __builtin_ctzll(mm);
            mm &= mm - 1;
            const unsigned long long* rb = mask + b * WS;
            int cab = 0, tri = 0;
            for (int x = 0; x < W; ++x) {
                const unsigned long long r = ra[x] & rb[x];
                cab += __builtin_popcountll(r);
                tri += __builtin_popcountll(r & rv[x]);
            }
            s.eadj += cab - 1;
            s.t3 += tri;
        }
    }
    const long long da1 = s_d[a] - 1, out = da1 - c;
    s.c2 += (long long)c * (c - 1) / 2;
    s.cout += c * out;
    s.dout += (dv - 1 - c) * out;
    s.ta += s_t[a];
    s.cda2 += da1 * (da1 - 1) / 2;
    s.s1a += s_s1[a] - (dv - 1);
}

// the term of any other node w of the graph: the pairs of N(v) that w joins
CCSD_DEV void orbit_other(OrbitSums& s, const unsigned long long* __restrict__ mask, int WS, int W, int v, int w) {
    const long long c = orbit_common(mask + v * WS, mask + w * WS, W);
    s.sp += c * (c - 1) / 2;
}

CCSD_DEV void orbit_finish(const OrbitSums& s, long long d, long long t, long long s1, long long* __restrict__ o) {
    const long long n3 = s.t3 / 3, n2 = s.c2 - 3 * n3, n1 = t * (d - 2) - 2 * n2 - 3 * n3, n0 = d * (d - 1) * (d - 2) / 6 - n1 - n2 - n3;
    const long long o12 = s.eadj - 3 * n3, o8 = (s.sp - s.eadj) - n2, o10 = s.cout - 2 * o12, o5 = s.dout - 2 * o8;
    const long long o9 = s.ta - 2 * t - 3 * n3 - 2 * o12, o6 = s.cda2 - (s.ta - 2 * t) - n2 - o10;
    o[0] = d;  o[1] = s1 - 2 * t;  o[2] = d * (d - 1) / 2 - t;  o[3] = t;
    o[4] = s.s1a - 2 * t - 2 * o9 - 2 * o8 - o10 - 2 * n2 - 4 * o12 - 6 * n3;
    o[5] = o5;  o[6] = o6;  o[7] = n0;  o[8] = o8;  o[9] = o9;  o[10] = o10;  o[11] = n1;  o[12] = o12;  o[13] = n2;  o[14] = n3;
}

// ---------------------------------------------------------------------------------------------
// k_orbit_counts: one workgroup per graph over adj (B, N, N) fp32, 2 <= N <= CCSD_FIN_MAXN
//   node_orbits (B, N, 15) int64   node_orbits[b][v][k] = the induced connected subgraphs on 2, 3 or 4 nodes in which v sits at orbit k
//                                  (zeros for isolated and masked slots): the rows of the non-isolated slots, in slot order, are what
//                                  `orca node 4` prints for adjs_to_graphs(adj_int)[b]
//   graph_orbits (B, 15) int64     the column sums over the nodes
//   orbit_nodes (B,) int32         nodes of degree > 0, or 1 for a graph without an edge: G.number_of_nodes() under adjs_to_graphs'
//                                  node rules (graph_utils.py:245-250), the same rule as k_cluster_hist's s_nodes
// All nullable.  The edge rule, the symmetric-adjacency contract and the LDS mask layout (stride WS = W | 1 words) are k_cluster_hist's.
// Three passes over the LDS-resident masks, a wave per node in each:
//   1  row i -> mask words by ballot, d(i)
//   2  t(i) and s1(i): lanes over the neighbours of i
//   3  the sums of OrbitSums: lanes over the neighbours a of v (orbit_neighbour: row a is an 8-byte read per lane at the odd stride; the
//      rows b of the pair loop are whatever neighbours the lanes hold, so those reads may share banks), then lanes over all nodes w
//      (orbit_other); a 64-bit shuffle tree; lane 0 finishes the node.
// The pair loop is the cost: sum over v of t(v) (2 W) and-popcounts, against N^2 W for everything else.
// ---------------------------------------------------------------------------------------------
__global__ void k_orbit_counts(const float* __restrict__ adj, int N, float thr, long long* __restrict__ node_orbits,
                               long long* __restrict__ graph_orbits, int* __restrict__ orbit_nodes) {
    const int b = blockIdx.x, W = (N + 63) >> 6, WS = W | 1;
    const float* Ab = adj + (size_t)b * N * N;
    __shared__ unsigned long long s_mask[CCSD_FIN_MAXN * (CCSD_EVAL_MAXW | 1)];
    __shared__ int s_d[CCSD_FIN_MAXN], s_t[CCSD_FIN_MAXN], s_s1[CCSD_FIN_MAXN];
    __shared__ unsigned long long s_graph[CCSD_NORBITS];
    __shared__ int s_nodes;
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int k = tid; k < CCSD_NORBITS; k += nth) s_graph[k] = 0;
    if (tid == 0) s_nodes = 0;
    long long* Ob = node_orbits ? node_orbits + (size_t)b * N * CCSD_NORBITS : nullptr;
#ifdef CCSD_EMU
    for (int i = 0; i < N; ++i) {
        int d = 0;
        for (int w = 0; w < W; ++w) s_mask[i * WS + w] = 0;
        for (int j = 0; j < N; ++j)
            if (j != i && finish_quant(Ab[(size_t)i * N + j], thr) != 0) s_mask[i * WS + (j >> 6)] |= 1ull << (j & 63), ++d;
        s_d[i] = d;
    }
    for (int i = 0; i < N; ++i) {
        int t2 = 0, s1 = 0;
        for (int j = 0; j < N; ++j)
            if ((s_mask[i * WS + (j >> 6)] >> (j & 63)) & 1) {
                t2 += orbit_common(s_mask + i * WS, s_mask + j * WS, W);
                s1 += s_d[j] - 1;
            }
        s_t[i] = t2 >> 1;
        s_s1[i] = s1;
    }
    for (int v = 0; v < N; ++v) {
        OrbitSums s = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        long long o[CCSD_NORBITS];
        const int d = s_d[v];
        for (int a = 0; a < N; ++a)
            if ((s_mask[v * WS + (a >> 6)] >> (a & 63)) & 1) orbit_neighbour(s, s_mask, WS, W, v, a, d, s_d, s_t, s_s1);
        for (int w = 0; w < N; ++w)
            if (w != v) orbit_other(s, s_mask, WS, W, v, w);
        orbit_finish(s, d, s_t[v], s_s1[v], o);
        for (int k = 0; k < CCSD_NORBITS; ++k) {
            if (Ob) Ob[(size_t)v * CCSD_NORBITS + k] = o[k];
            s_graph[k] += (unsigned long long)o[k];
        }
        if (d > 0) s_nodes += 1;
    }
#else
    const int wave = wave_index(), lane = tid & 63, nw = nth >> 6;
    // pass 1: row i -> W mask words, one ballot per 64 entries (the wave-uniform loop bound keeps every lane in the ballot); d(i)
    for (int i = wave; i < N; i += nw) {
        int d = 0;
        for (int w = 0; w < W; ++w) {
            const int j = (w << 6) + lane;
            const bool on = j < N && j != i && finish_quant(Ab[(size_t)i * N + j], thr) != 0;
            const unsigned long long m = __ballot(on);
            d += __popcll(m);
            if (lane == 0) s_mask[i * WS + w] = m;
        }
        if (lane == 0) s_d[i] = d;
    }
    __syncthreads();
    // pass 2: t(i), s1(i): node i per wave, its neighbours j over the lanes
    for (int i = wave; i < N; i += nw) {
        int t2 = 0, s1 = 0;
        for (int w = 0; w < W; ++w)
            if ((s_mask[i * WS + w] >> lane) & 1) {                         // (broadcast read)
                const int j = (w << 6) + lane;                              // (< N: pass 1 sets no bit at or past N)
                t2 += orbit_common(s_mask + i * WS, s_mask + j * WS, W);
                s1 += s_d[j] - 1;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            t2 += __shfl_xor(t2, o, 64);
            s1 += __shfl_xor(s1, o, 64);
        }
        if (lane == 0) {
            s_t[i] = t2 >> 1;
            s_s1[i] = s1;
        }
    }
    __syncthreads();
    // pass 3: the orbits of node v per wave
    for (int v = wave; v < N; v += nw) {
        OrbitSums s = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int d = s_d[v];
        for (int w = 0; w < W; ++w) {
            if ((s_mask[v * WS + w] >> lane) & 1) orbit_neighbour(s, s_mask, WS, W, v, (w << 6) + lane, d, s_d, s_t, s_s1);
            const int x = (w << 6) + lane;
            if (x < N && x != v && d > 1) orbit_other(s, s_mask, WS, W, v, x);      // (d < 2: N(v) holds no pair)
        }
        static_assert(sizeof(OrbitSums) == CCSD_ORBIT_NSUMS * sizeof(long long), "OrbitSums is its sums and nothing else");
        long long* f = reinterpret_cast<long long*>(&s);
#pragma unroll
        for (int q = 0; q < CCSD_ORBIT_NSUMS; ++q)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) f[q] += __shfl_xor(f[q], o, 64);
        if (lane == 0) {
            long long o[CCSD_NORBITS];
            orbit_finish(s, d, s_t[v], s_s1[v], o);
#pragma unroll
            for (int k = 0; k < CCSD_NORBITS; ++k) {
                if (Ob) Ob[(size_t)v * CCSD_NORBITS + k] = o[k];
                if (o[k]) atomicAdd(&s_graph[k], (unsigned long long)o[k]);
            }
            if (d > 0) atomicAdd(&s_nodes, 1);
        }
    }
#endif
    __syncthreads();
    if (graph_orbits)
        for (int k = tid; k < CCSD_NORBITS; k += nth) graph_orbits[(size_t)b * CCSD_NORBITS + k] = (long long)s_graph[k];
    if (orbit_nodes && tid == 0) orbit_nodes[b] = s_nodes > 0 ? s_nodes : 1;
}
