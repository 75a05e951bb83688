// ccsd_k_nspdk.h -- k_nspdk_features, k_nspdk_chunks, k_nspdk_dots, k_nspdk_final: the NSPDK feature vectors of finished samples and
// the linear-kernel MMD of two sets of them (the "nspdk" score of the evaluation)
// Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// The reference scores molecule runs with the neighbourhood subgraph pairwise distance kernel: eden.py's vectorize(graphs, complexity = 4,
// discrete = True) gives one L2-normalised sparse vector of 2^16 + 1 columns per graph, and compute_nspdk_mmd (mmd.py:352-377) the MMD of
// two sets under the linear kernel.  The vectoriser is a breadth-first search to depth 8 per node, Python's hash of tuples of integers,
// counting and two normalisations; with INTEGER node labels (hash(int) is the integer) it is deterministic and restated here exactly.
//
// Hash.  CPython >= 3.8 hashes a tuple of ints like xxHash: acc = P5; per element acc += lane P2, acc = rotl(acc, 31), acc *= P1; then
// acc += len ^ (P5 ^ 3527539); all ones -> 1546275796; read as signed 64-bit.  lane = hash(int) = sign(x) (|x| mod (2^61 - 1)), -1 -> -2.
// H(t, m) = (hash(t) & m) + 1; M32 = 2^32 - 1, M16 = 2^16 - 1.  H(., M32) reaches 2^32: hash values are kept in 64 bits.
//
// Per graph (N <= 64 node slots, a slot with a negative label holds no node; edges between present slots only, labelled with the
// quantised bond order in mol mode and 1 otherwise):
//   1  expanded graph: every edge is an edge-vertex of degree 2.  hl = (label & M16) + 1, vh = H((hl, degree), M32).  An edge-vertex's
//      vh depends on its label alone: three values.
//   2  per root r the BFS layers L_0 .. L_k, k <= 8, of the expanded graph: layer 2 j = the nodes at graph distance j, layer 2 j + 1 = the
//      edges whose nearer endpoint is at distance j; the layers end at the first empty one.
//   3  hs[i] = H(sorted vh of L_i, M32); run = 0xAAAAAAAA; run ^= hash((run, hs[i], i)); ngh[r][i] = (run & M32) + 1.
//   4  for every ordered pair (v, u) at graph distance dd <= 4 (u = v at 0) and every rr <= 4 with 2 rr < min(len ngh[v], len ngh[u]),
//      a = ngh[v][2 rr], b = ngh[u][2 rr]: the features H((min, max, 2 rr, 2 dd), M16) and H((b, 2 rr, 2 dd), M16) count + 1 in block (rr, dd).
//   5  each block is divided by its L2 norm; the blocks are merged by ASSIGNMENT in the order of their first use (v, then dd, then rr
//      ascending), so the block created last wins an index two blocks share; the merged vector is divided by its L2 norm.
//
// How k_nspdk_features does it, one workgroup per graph:
//   - rows are three 64-bit masks (one per edge label) by ballot; BFS layers are mask operations, a thread per root.
//   - no layer is sorted: the nodes are ranked by vh once per graph and a node layer is walked in that order; an edge layer is three
//     counts, fed to the hash in the order of the three edge vh values (the 1953 edges of K64's outer layer are 1953 hash steps).
//   - a block's <= 2 N^2 keys are written to LDS; the counts live in a 2^16-entry table of the workgroup in global memory, one
//     uint32 = (creation rank + 1) << 16 | count.  Blocks are taken in creation order, so "last wins" is an atomicMax that installs the
//     block's rank (and clears an older block's count), then an atomicAdd per key: INTEGER atomics, whose result does not depend on
//     their order.  The block's squared norm is the sum over its keys of the count of the key's index (= sum of count^2), an integer.
//   - an LDS bitmap of the occupied indices makes the last pass proportional to the non-zeros: 256 segments of 256 indices, each
//     summed in index order, the 256 partial sums added in segment order (a fixed order: identical bits from call to call); the rows
//     come out sorted by index and the table is left zero for the next graph.
#pragma once
#include "ccsd_dev.h"
#include "ccsd_k_finish.h"

#define CCSD_NSPDK_MAXN 64
#define CCSD_NSPDK_DEPTH 4                       // radius and distance limit ("complexity = 4")
#define CCSD_NSPDK_NL (CCSD_NSPDK_DEPTH + 1)     // node layers per root; radii; distances
#define CCSD_NSPDK_NBLK (CCSD_NSPDK_NL * CCSD_NSPDK_NL)
#define CCSD_NSPDK_COLS 65536                    // feature indices are 1 .. 65536 (column 0 of the 65537 is never used)
#define CCSD_NSPDK_NOKEY 0xFFFFFFFFu

typedef unsigned long long nspdk_u64;

#define NSPDK_P1 11400714785074694791ull
#define NSPDK_P2 14029467366897019727ull
#define NSPDK_P5 2870177450012600261ull

CCSD_DEV nspdk_u64 nspdk_step(nspdk_u64 acc, nspdk_u64 lane) {
    acc += lane * NSPDK_P2;
    acc = (acc << 31) | (acc >> 33);
    return acc * NSPDK_P1;
}
CCSD_DEV long long nspdk_fin(nspdk_u64 acc, nspdk_u64 len) {
    acc += len ^ (NSPDK_P5 ^ 3527539ull);
    return acc == ~0ull ? 1546275796ll : (long long)acc;
}
// hash(int) of a signed 64-bit value, as the unsigned lane
CCSD_DEV nspdk_u64 nspdk_ilane(long long x) {
    const nspdk_u64 MOD = (1ull << 61) - 1;
    const nspdk_u64 mag = x < 0 ? 0ull - (nspdk_u64)x : (nspdk_u64)x;
    nspdk_u64 m = (mag & MOD) + (mag >> 61);
    if (m >= MOD) m -= MOD;
    long long h = x < 0 ? -(long long)m : (long long)m;
    if (h == -1) h = -2;
    return (nspdk_u64)h;
}
CCSD_DEV long long nspdk_hash2(nspdk_u64 a, nspdk_u64 b) { return nspdk_fin(nspdk_step(nspdk_step(NSPDK_P5, a), b), 2); }
CCSD_DEV long long nspdk_hash3(nspdk_u64 a, nspdk_u64 b, nspdk_u64 c) {
    return nspdk_fin(nspdk_step(nspdk_step(nspdk_step(NSPDK_P5, a), b), c), 3);
}
CCSD_DEV long long nspdk_hash4(nspdk_u64 a, nspdk_u64 b, nspdk_u64 c, nspdk_u64 d) {
    return nspdk_fin(nspdk_step(nspdk_step(nspdk_step(nspdk_step(NSPDK_P5, a), b), c), d), 4);
}
CCSD_DEV nspdk_u64 nspdk_h32(long long h) { return ((nspdk_u64)h & 0xFFFFFFFFull) + 1ull; }

// integer atomics (the host emulation runs one thread per workgroup).  The table is read and written through the L2 only.
CCSD_DEV void nspdk_tab_max(unsigned* p, unsigned v) {
#ifdef CCSD_EMU
    if (*p < v) *p = v;
#else
    atomicMax(p, v);
#endif
}
CCSD_DEV void nspdk_tab_inc(unsigned* p) {
#ifdef CCSD_EMU
    *p += 1;
#else
    atomicAdd(p, 1u);
#endif
}
CCSD_DEV unsigned nspdk_tab_load(unsigned* p) {
#ifdef CCSD_EMU
    return *p;
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
CCSD_DEV void nspdk_tab_zero(unsigned* p) {
#ifdef CCSD_EMU
    *p = 0;
#else
    __hip_atomic_store(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
CCSD_DEV void nspdk_lds_or(unsigned* p, unsigned v) {
#ifdef CCSD_EMU
    *p |= v;
#else
    atomicOr(p, v);
#endif
}
CCSD_DEV void nspdk_lds_min(int* p, int v) {
#ifdef CCSD_EMU
    if (v < *p) *p = v;
#else
    atomicMin(p, v);
#endif
}
CCSD_DEV void nspdk_lds_add(nspdk_u64* p, nspdk_u64 v) {
#ifdef CCSD_EMU
    *p += v;
#else
    atomicAdd(p, v);
#endif
}
// Every table access of the workgroup before the barrier is performed before any after it.  The table belongs to this workgroup alone
// and every access to it is an atomic that the L2 performs, so the barrier's own workgroup-scope fence (each wave waits for its
// outstanding memory operations before it arrives) orders them.  A device-scope fence here writes back and invalidates caches at each of
// the 76 barriers of a graph.
CCSD_DEV void nspdk_sync() { __syncthreads(); }

// ---------------------------------------------------------------------------------------------
// k_nspdk_features: workgroup w takes the graphs w, w + gridDim.x, ... of adj (B, N, N) fp32, 1 <= N <= 64
//   labels (B, N) int32      node label per slot, negative = no node; NULL = every slot is a node with label 0
//   table                    gridDim.x x 65536 uint32, ZERO on entry and on exit
//   nnz (B,) int32           non-zeros of the row (0 for a graph without a node)
//   indices (B, cap) int32   ascending feature indices, 1 .. 65536
//   values (B, cap) fp64     cap >= min(65536, 10 N^2): two keys per (ordered pair within distance 4, radius)
// The edge rule (a non-zero quantised entry off the diagonal, finish_quant) and the symmetric-adjacency contract are k_cluster_hist's.
// ---------------------------------------------------------------------------------------------
__global__ void k_nspdk_features(const float* __restrict__ adj, const int* __restrict__ labels, int B, int N, float thr, int cap,
                                 unsigned* __restrict__ table, int* __restrict__ nnz, int* __restrict__ indices,
                                 double* __restrict__ values) {
    __shared__ nspdk_u64 s_m[3][CCSD_NSPDK_MAXN];                            // row i: the neighbours over an edge labelled l + 1
    __shared__ nspdk_u64 s_lay[CCSD_NSPDK_MAXN][CCSD_NSPDK_NL];              // root v: the nodes at distance j
    __shared__ nspdk_u64 s_ngh[CCSD_NSPDK_MAXN][CCSD_NSPDK_NL];              // root v: ngh[v][2 j]
    __shared__ nspdk_u64 s_vh[CCSD_NSPDK_MAXN];
    __shared__ int s_len[CCSD_NSPDK_MAXN], s_ord[CCSD_NSPDK_MAXN], s_lab[CCSD_NSPDK_MAXN];
    __shared__ int s_first[CCSD_NSPDK_NBLK], s_blk[CCSD_NSPDK_NBLK], s_nb, s_np;
    __shared__ nspdk_u64 s_norm2[CCSD_NSPDK_NBLK];
    __shared__ double s_inv[CCSD_NSPDK_NBLK];                                // sqrt of the block's squared norm
    __shared__ unsigned s_key[2 * CCSD_NSPDK_MAXN * CCSD_NSPDK_MAXN];        // index - 1 of the two keys of pair t = v N + u, or NOKEY
    __shared__ unsigned s_bits[CCSD_NSPDK_COLS / 32];                        // bit i: index i + 1 is occupied
    __shared__ int s_cnt[256];
    __shared__ double s_part[256];
    __shared__ double s_tot;
    const int tid = threadIdx.x, nth = blockDim.x;
    unsigned* T = table + (size_t)blockIdx.x * CCSD_NSPDK_COLS;
    for (int k = tid; k < CCSD_NSPDK_COLS / 32; k += nth) s_bits[k] = 0;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const float* Ab = adj + (size_t)b * N * N;
        // ---- labels, rows as masks ----
        for (int i = tid; i < N; i += nth) s_lab[i] = labels ? labels[(size_t)b * N + i] : 0;
        for (int k = tid; k < CCSD_NSPDK_NBLK; k += nth) { s_first[k] = CCSD_NSPDK_MAXN; s_norm2[k] = 0; }
        __syncthreads();
#ifdef CCSD_EMU
        for (int i = 0; i < N; ++i) {
            s_m[0][i] = s_m[1][i] = s_m[2][i] = 0;
            for (int j = 0; j < N; ++j) {
                const int q = (j != i && s_lab[i] >= 0 && s_lab[j] >= 0) ? finish_quant(Ab[(size_t)i * N + j], thr) : 0;
                if (q) s_m[q - 1][i] |= 1ull << j;
            }
        }
#else
        {
            const int wave = wave_index(), lane = tid & 63, nw = nth >> 6;
            for (int i = wave; i < N; i += nw) {                             // (wave-uniform bound: every lane takes part in the ballots)
                const int q = (lane < N && lane != i && s_lab[i] >= 0 && s_lab[lane] >= 0) ? finish_quant(Ab[(size_t)i * N + lane], thr) : 0;
                const nspdk_u64 m1 = __ballot(q == 1), m2 = __ballot(q == 2), m3 = __ballot(q == 3);
                if (lane == 0) { s_m[0][i] = m1; s_m[1][i] = m2; s_m[2][i] = m3; }
            }
        }
#endif
        __syncthreads();
        // ---- vh of the nodes ----
        for (int i = tid; i < N; i += nth) {
            const nspdk_u64 hl = ((nspdk_u64)s_lab[i] & 0xFFFFull) + 1ull;
            const int deg = __builtin_popcountll(s_m[0][i] | s_m[1][i] | s_m[2][i]);
            s_vh[i] = nspdk_h32(nspdk_hash2(hl, (nspdk_u64)deg));
        }
        __syncthreads();
        // ---- the present nodes in ascending order of vh (ties by slot: equal values are interchangeable) ----
        for (int i = tid; i < N; i += nth)
            if (s_lab[i] >= 0) {
                int r = 0;
                for (int j = 0; j < N; ++j)
                    if (s_lab[j] >= 0 && (s_vh[j] < s_vh[i] || (s_vh[j] == s_vh[i] && j < i))) ++r;
                s_ord[r] = i;
            }
        if (tid == 0) {
            int np = 0;
            for (int i = 0; i < N; ++i) np += s_lab[i] >= 0;
            s_np = np;
        }
        __syncthreads();
        // ---- BFS layers and neighbourhood hashes, a thread per root ----
        for (int v = tid; v < N; v += nth) {
            int nl = 0;
            for (int j = 0; j < CCSD_NSPDK_NL; ++j) s_lay[v][j] = 0;
            if (s_lab[v] >= 0) {
                // the three edge vh values in ascending order
                nspdk_u64 evh[3];
                int eo[3] = {0, 1, 2};
                for (int l = 0; l < 3; ++l) evh[l] = nspdk_h32(nspdk_hash2((nspdk_u64)(l + 2), 2ull));      // hl = (l + 1) + 1
                if (evh[eo[0]] > evh[eo[1]]) { const int x = eo[0]; eo[0] = eo[1]; eo[1] = x; }
                if (evh[eo[1]] > evh[eo[2]]) { const int x = eo[1]; eo[1] = eo[2]; eo[2] = x; }
                if (evh[eo[0]] > evh[eo[1]]) { const int x = eo[0]; eo[0] = eo[1]; eo[1] = x; }
                const int np = s_np;
                nspdk_u64 seen = 1ull << v, front = seen;
                long long run = 0xAAAAAAAAll;
                for (int j = 0; j < CCSD_NSPDK_NL; ++j) {
                    // layer 2 j: the nodes of `front`
                    s_lay[v][j] = front;
                    nspdk_u64 acc = NSPDK_P5;
                    for (int k = 0; k < np; ++k) {
                        const int i = s_ord[k];
                        if ((front >> i) & 1) acc = nspdk_step(acc, s_vh[i]);
                    }
                    nspdk_u64 hs = nspdk_h32(nspdk_fin(acc, (nspdk_u64)__builtin_popcountll(front)));
                    run ^= nspdk_hash3(nspdk_ilane(run), hs, (nspdk_u64)(2 * j));
                    s_ngh[v][j] = nspdk_h32(run);
                    nl = 2 * j + 1;
                    if (j == CCSD_NSPDK_NL - 1) break;
                    // layer 2 j + 1: the edges from `front` outwards or inside it (twice the count per label: an inner edge is met from both ends)
                    nspdk_u64 next = 0;
                    int c2[3] = {0, 0, 0};
                    for (nspdk_u64 f = front; f; f &= f - 1) {
                        const int i = __builtin_ctzll(f);
                        for (int l = 0; l < 3; ++l) {
                            const nspdk_u64 m = s_m[l][i];
                            next |= m;
                            c2[l] += 2 * __builtin_popcountll(m & ~seen) + __builtin_popcountll(m & front);
                        }
                    }
                    next &= ~seen;
                    const int ne = (c2[0] + c2[1] + c2[2]) >> 1;
                    if (ne == 0) break;
                    acc = NSPDK_P5;
                    for (int q = 0; q < 3; ++q) {
                        const nspdk_u64 e = evh[eo[q]];
                        for (int k = c2[eo[q]] >> 1; k > 0; --k) acc = nspdk_step(acc, e);
                    }
                    hs = nspdk_h32(nspdk_fin(acc, (nspdk_u64)ne));
                    run ^= nspdk_hash3(nspdk_ilane(run), hs, (nspdk_u64)(2 * j + 1));
                    nl = 2 * j + 2;
                    if (!next) break;
                    seen |= next;
                    front = next;
                }
            }
            s_len[v] = nl;
        }
        __syncthreads();
        // ---- the blocks in the order of their first use ----
        for (int v = tid; v < N; v += nth)
            for (int dd = 0; dd < CCSD_NSPDK_NL; ++dd) {
                int far = 0;
                for (nspdk_u64 f = s_lay[v][dd]; f; f &= f - 1) {
                    const int l = s_len[__builtin_ctzll(f)];
                    far = l > far ? l : far;
                }
                const int m = s_len[v] < far ? s_len[v] : far;
                for (int rr = 0; 2 * rr < m; ++rr) nspdk_lds_min(&s_first[rr * CCSD_NSPDK_NL + dd], v);
            }
        __syncthreads();
        if (tid == 0) {
            int nb = 0;
            for (int k = 0; k < CCSD_NSPDK_NBLK; ++k)
                if (s_first[k] < CCSD_NSPDK_MAXN) s_blk[nb++] = k;
            // creation order: (first v, dd, rr) ascending; block id k = rr NL + dd
            for (int x = 1; x < nb; ++x) {
                const int k = s_blk[x], key = (s_first[k] * CCSD_NSPDK_NL + k % CCSD_NSPDK_NL) * CCSD_NSPDK_NL + k / CCSD_NSPDK_NL;
                int y = x - 1;
                for (; y >= 0; --y) {
                    const int k2 = s_blk[y];
                    if ((s_first[k2] * CCSD_NSPDK_NL + k2 % CCSD_NSPDK_NL) * CCSD_NSPDK_NL + k2 / CCSD_NSPDK_NL < key) break;
                    s_blk[y + 1] = k2;
                }
                s_blk[y + 1] = k;
            }
            s_nb = nb;
        }
        __syncthreads();
        const int nb = s_nb;
        // ---- the blocks, one after the other ----
        for (int r = 0; r < nb; ++r) {
            const int rr = s_blk[r] / CCSD_NSPDK_NL, dd = s_blk[r] % CCSD_NSPDK_NL;
            // keys of the block; its rank is installed at their indices
            for (int t = tid; t < N * N; t += nth) {
                const int v = t / N, u = t - v * N;
                unsigned k0 = CCSD_NSPDK_NOKEY, k1 = CCSD_NSPDK_NOKEY;
                if (((s_lay[v][dd] >> u) & 1) && 2 * rr < s_len[v] && 2 * rr < s_len[u]) {
                    const nspdk_u64 a = s_ngh[v][rr], c = s_ngh[u][rr];
                    k0 = (unsigned)((nspdk_u64)nspdk_hash4(a < c ? a : c, a < c ? c : a, (nspdk_u64)(2 * rr), (nspdk_u64)(2 * dd)) & 0xFFFFull);
                    k1 = (unsigned)((nspdk_u64)nspdk_hash3(c, (nspdk_u64)(2 * rr), (nspdk_u64)(2 * dd)) & 0xFFFFull);
                    nspdk_tab_max(&T[k0], (unsigned)(r + 1) << 16);
                    nspdk_tab_max(&T[k1], (unsigned)(r + 1) << 16);
                    nspdk_lds_or(&s_bits[k0 >> 5], 1u << (k0 & 31));
                    nspdk_lds_or(&s_bits[k1 >> 5], 1u << (k1 & 31));
                }
                s_key[2 * t] = k0;
                s_key[2 * t + 1] = k1;
            }
            nspdk_sync();
            for (int t = tid; t < 2 * N * N; t += nth)
                if (s_key[t] != CCSD_NSPDK_NOKEY) nspdk_tab_inc(&T[s_key[t]]);
            nspdk_sync();
            // sum over the keys of the count at the key's index = sum over the block's indices of count^2
            nspdk_u64 sq = 0;
            for (int t = tid; t < 2 * N * N; t += nth)
                if (s_key[t] != CCSD_NSPDK_NOKEY) sq += nspdk_tab_load(&T[s_key[t]]) & 0xFFFFu;
            if (sq) nspdk_lds_add(&s_norm2[r], sq);
            nspdk_sync();                                                    // (the next block's atomicMax clears counts read here)
        }
        for (int r = tid; r < nb; r += nth) s_inv[r] = sqrt((double)s_norm2[r]);
        __syncthreads();
        // ---- merged vector: 256 segments of 256 indices; squared norm in a fixed order ----
        for (int q = tid; q < 256; q += nth) {
            int cnt = 0;
            double part = 0.0;
            for (int w = 0; w < 8; ++w)
                for (unsigned m = s_bits[8 * q + w]; m; m &= m - 1) {
                    const int i = 32 * (8 * q + w) + __builtin_ctz(m);
                    const unsigned e = nspdk_tab_load(&T[i]);
                    const double val = (double)(e & 0xFFFFu) / s_inv[(e >> 16) - 1];
                    part += val * val;
                    ++cnt;
                }
            s_cnt[q] = cnt;
            s_part[q] = part;
        }
        __syncthreads();
        if (tid == 0) {
            int off = 0;
            double tot = 0.0;
            for (int q = 0; q < 256; ++q) {
                const int c = s_cnt[q];
                s_cnt[q] = off;
                off += c;
                tot += s_part[q];
            }
            s_tot = sqrt(tot);
            nnz[b] = off < cap ? off : cap;                                  // (= off: see the guard of the writes below)
        }
        __syncthreads();
        const double tot = s_tot;
        for (int q = tid; q < 256; q += nth) {
            int pos = s_cnt[q];
            for (int w = 0; w < 8; ++w) {
                for (unsigned m = s_bits[8 * q + w]; m; m &= m - 1) {
                    const int i = 32 * (8 * q + w) + __builtin_ctz(m);
                    const unsigned e = nspdk_tab_load(&T[i]);
                    const double val = (double)(e & 0xFFFFu) / s_inv[(e >> 16) - 1];
                    if (pos < cap) {                                         // (always: cap >= the number of keys; nnz is clamped alike)
                        indices[(size_t)b * cap + pos] = i + 1;
                        values[(size_t)b * cap + pos] = val / tot;
                    }
                    ++pos;
                    nspdk_tab_zero(&T[i]);
                }
                s_bits[8 * q + w] = 0;
            }
        }
        nspdk_sync();
    }
}

// ---------------------------------------------------------------------------------------------
// The MMD of two sets of rows in CSR form (indptr (n + 1) int64, ascending indices 1 .. 65536, fp64 values) under the linear kernel:
// mean K(x, x') over all pairs = |mean x|^2, so   out = [ |mx|^2, |my|^2, mx . my, |mx|^2 + |my|^2 - 2 mx . my ]
// with mx the mean over ALL n1 rows of the first set and my the mean over the rows of the second set that hold a non-zero (a graph
// without a node has no row in the reference's predicted set, stats.py:452-454).
//   k_nspdk_chunks   cp[r][k] = the first position of row r with index >= 256 k + 1, k = 0 .. 256; counts the non-empty rows
//   k_nspdk_dots     workgroup k, thread t: column 256 k + t + 1 of both means, each summed over the rows in row order; then the three
//                    products summed over t in thread order: part[k][3]
//   k_nspdk_final    the 256 partials in workgroup order
// Every sum has one fixed order: identical bits from call to call.
// ---------------------------------------------------------------------------------------------
#define CCSD_NSPDK_CHUNKS 256
__global__ void k_nspdk_chunks(const long long* __restrict__ indptr, const int* __restrict__ indices, int n, long long* __restrict__ cp,
                               int* __restrict__ nonempty) {
    const long long total = (long long)n * (CCSD_NSPDK_CHUNKS + 1);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(t / (CCSD_NSPDK_CHUNKS + 1)), k = (int)(t - (long long)r * (CCSD_NSPDK_CHUNKS + 1));
        long long lo = indptr[r], hi = indptr[r + 1];
        if (k == 0 && hi > lo && nonempty) {
#ifdef CCSD_EMU
            *nonempty += 1;
#else
            atomicAdd(nonempty, 1);
#endif
        }
        const int want = 256 * k + 1;
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (indices[mid] < want) lo = mid + 1; else hi = mid;
        }
        cp[t] = lo;
    }
}

// the column's sum over the rows of one set, in row order
CCSD_DEV double nspdk_colsum(const int* __restrict__ indices, const double* __restrict__ values, const long long* __restrict__ cp, int n,
                             int k, int col) {
    double s = 0.0;
    for (int r = 0; r < n; ++r) {
        const long long p0 = cp[(size_t)r * (CCSD_NSPDK_CHUNKS + 1) + k], p1 = cp[(size_t)r * (CCSD_NSPDK_CHUNKS + 1) + k + 1];
        for (long long p = p0; p < p1; ++p)
            if (indices[p] == col) s += values[p];
    }
    return s;
}

__global__ void k_nspdk_dots(const int* __restrict__ ix, const double* __restrict__ vx, const long long* __restrict__ cpx, int n1,
                             const int* __restrict__ iy, const double* __restrict__ vy, const long long* __restrict__ cpy, int n2,
                             const int* __restrict__ nonempty2, double* __restrict__ part) {
    __shared__ double s_xx[256], s_yy[256], s_xy[256];
    const int k = blockIdx.x;
    const double d1 = (double)n1, d2 = (double)*nonempty2;
    for (int t = threadIdx.x; t < 256; t += blockDim.x) {
        const int col = 256 * k + t + 1;
        const double mx = nspdk_colsum(ix, vx, cpx, n1, k, col) / d1, my = nspdk_colsum(iy, vy, cpy, n2, k, col) / d2;
        s_xx[t] = mx * mx;
        s_yy[t] = my * my;
        s_xy[t] = mx * my;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, c = 0.0, e = 0.0;
        for (int t = 0; t < 256; ++t) { a += s_xx[t]; c += s_yy[t]; e += s_xy[t]; }
        part[3 * k] = a;
        part[3 * k + 1] = c;
        part[3 * k + 2] = e;
    }
}

__global__ void k_nspdk_final(const double* __restrict__ part, double* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double a = 0.0, c = 0.0, e = 0.0;
        for (int k = 0; k < CCSD_NSPDK_CHUNKS; ++k) { a += part[3 * k]; c += part[3 * k + 1]; e += part[3 * k + 2]; }
        out[0] = a;
        out[1] = c;
        out[2] = e;
        out[3] = a + c - 2.0 * e;
    }
}
