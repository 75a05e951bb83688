// ccsd_k_finish.h -- k_finish_rank2, k_finish_graph: the finish of a sampling run in one pass per tensor
// Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// After the last predictor step the harness quantises the samples (graph_utils.py:181-213), builds the sparse form of the rank-2
// incidence matrix (cc_utils.py:243-262) and -- new here -- reduces each complex to the integer descriptors the reference's
// evaluators histogram (degree_worker, stats.py:36; rank1_distrib_worker / rank2_distrib_worker, cc_utils.py:1208-1334).  Both
// kernels produce integers only; sums of integers do not depend on the order of the atomics, so the results are deterministic.
#pragma once
#include "ccsd_dev.h"

// quantize(t, thr) (thr >= 0; graph_utils.py:191) / quantize_mol (thr < 0; graph_utils.py:209-213): the expression of k_quantize
CCSD_DEV int finish_quant(float v, float thr) {
    if (thr >= 0.f) return v < thr ? 0 : 1;
    return v >= 2.5f ? 3 : v >= 1.5f ? 2 : v >= 0.5f ? 1 : 0;
}

// LDS counter increment (the host emulation runs one thread per workgroup)
CCSD_DEV void finish_inc(int* p) {
#ifdef CCSD_EMU
    *p += 1;
#else
    atomicAdd(p, 1);
#endif
}

// The K columns of rank2 enumerate the candidate cells by size (get_cells, cc_utils.py:72-76): the first C(N, d_min) columns have
// size d_min, the next C(N, d_min + 1) size d_min + 1, ...  end[i] = number of columns of size <= d_min + i (end[nb - 1] = K).
#define CCSD_FIN_MAXBINS 64
struct FinishTab {
    int nb;
    int end[CCSD_FIN_MAXBINS];
};
CCSD_DEV int finish_bin(const FinishTab& tab, int k) {
    int i = 0;
    while (i < tab.nb - 1 && k >= tab.end[i]) ++i;
    return i;
}

// ---------------------------------------------------------------------------------------------
// k_finish_rank2: ONE streaming read of rank2 (B, E, K) fp32 -> 4 bytes read and (with the dense output) 1 byte written per element
//   u8   (B, E, K) uint8     quantize(rank2, thr)                                (nullable)
//   bits (B, ceil(K/64))     bit k % 64 of word k / 64 = any_e(rank2[b][e][k] >= thr), as k_rank2_cells
//   cell_count (B,)          number of set bits, as k_rank2_cells
//   cell_hist (B, nb)        set bits per cell size (FinishTab)
//   nnz (B,)                 entries >= thr
// bits / cell_count / cell_hist / nnz are ZERO on entry (ccsd_finish clears them on the stream); each is nullable.
//
// grid (ceil(K / SLAB), B), 256 threads: a workgroup owns the columns [k0, k1) of one complex, its four waves take the rows
// e = wave, wave + 4, ... (the launch has exactly four waves).  K is a sum of binomials without any alignment, so rows start at arbitrary flat offsets: the lanes do NOT
// follow columns but the 16-byte groups of the WHOLE tensor (flat index 4 Q .. 4 Q + 3, 64-bit): lane j of a row piece takes group
// Q0 + j, Q0 = the group holding the piece's first element.  Every load is one aligned 16-byte load (1 KiB contiguous per wave) and every
// store one aligned dword of four quantised bytes (256 B contiguous per wave).  A group is STORED by the piece that holds its first
// element (exactly one piece does), whatever row, slab or complex its other three elements belong to; it is REDUCED element by element,
// only over the elements inside the piece.  SLAB = 252 makes the groups of a piece at most 64: one per lane.  Because a wave's rows are 4
// apart, the offset `sh` between its lanes' groups and the slab's columns is the same for all its rows (4 K = 0 mod 4): the column
// flags stay in four registers per lane and are merged through LDS once, after the rows.  Only the last group of the whole tensor can
// reach past its end (B E K not a multiple of 4): it is loaded and stored element by element.
// The slab's column flags go to `bits` with one 64-bit atomicOr per touched word (slabs are not word-aligned), the three counters with
// one atomicAdd each per workgroup.
// ---------------------------------------------------------------------------------------------
#define CCSD_FIN_SLAB 252
__global__ void k_finish_rank2(const float* __restrict__ rank2, int E, int K, float thr, FinishTab tab, long long n_total,
                               unsigned char* __restrict__ u8, unsigned long long* __restrict__ bits, int* __restrict__ cell_count,
                               int* __restrict__ cell_hist, int* __restrict__ nnz) {
    const int b = blockIdx.y, W = (K + 63) >> 6;
    const int k0 = blockIdx.x * CCSD_FIN_SLAB, k1 = k0 + CCSD_FIN_SLAB < K ? k0 + CCSD_FIN_SLAB : K, nc = k1 - k0;
    const long long cb = (long long)b * E * K;
#ifdef CCSD_EMU
    int count = 0, total = 0;
    for (int k = k0; k < k1; ++k) {
        bool any = false;
        for (int e = 0; e < E; ++e) {
            const float v = rank2[cb + (long long)e * K + k];
            if (u8) u8[cb + (long long)e * K + k] = (unsigned char)(v < thr ? 0 : 1);
            any = any || v >= thr;
            total += v >= thr;
        }
        if (any) {
            ++count;
            if (bits) bits[(size_t)b * W + (k >> 6)] |= 1ull << (k & 63);
            if (cell_hist) cell_hist[(size_t)b * tab.nb + finish_bin(tab, k)] += 1;
        }
    }
    if (cell_count) cell_count[b] += count;
    if (nnz) nnz[b] += total;
    (void)n_total; (void)nc;
#else
    __shared__ int s_any[CCSD_FIN_SLAB + 4];
    __shared__ int s_hist[CCSD_FIN_MAXBINS];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, wave = wave_index(), lane = tid & 63;
    for (int i = tid; i < CCSD_FIN_SLAB + 4; i += blockDim.x) s_any[i] = 0;
    if (tid < CCSD_FIN_MAXBINS) s_hist[tid] = 0;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    // this wave's rows: flat offset of the piece's first element, modulo 4, is the same for all of them
    const long long f_first = cb + (long long)wave * K + k0;
    const int sh = (int)(f_first & 3);
    const int c0 = 4 * lane - sh;                                  // column (relative to k0) of this lane's element 0
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0, mine = 0;
    const bool m0 = c0 >= 0 && c0 < nc, m1 = c0 + 1 >= 0 && c0 + 1 < nc, m2 = c0 + 2 >= 0 && c0 + 2 < nc, m3 = c0 + 3 >= 0 && c0 + 3 < nc;
    const bool active = c0 < nc;                                     // the group meets the piece (c0 + 3 >= 0 always)
    const bool owner = c0 >= 0 && active;                            // ... and starts inside it: this lane stores it
    if (active) {
#pragma unroll 4
        for (int e = wave; e < E; e += 4) {
            const long long fq = cb + (long long)e * K + k0 + c0;   // flat index of the group: a multiple of 4, >= 0 (c0 < 0 only when sh > 0)
            float v0, v1, v2, v3;
            const bool whole = fq + 3 < n_total;
            if (whole) {
                const float4 v4 = *reinterpret_cast<const float4*>(rank2 + fq);
                v0 = v4.x; v1 = v4.y; v2 = v4.z; v3 = v4.w;
            } else {                                                 // the tensor's last group, partly past its end (fq < n_total: m0 or a later mask holds)
                v0 = rank2[fq];
                v1 = fq + 1 < n_total ? rank2[fq + 1] : 0.f;
                v2 = fq + 2 < n_total ? rank2[fq + 2] : 0.f;
                v3 = 0.f;
            }
            const int g0 = m0 && v0 >= thr, g1 = m1 && v1 >= thr, g2 = m2 && v2 >= thr, g3 = m3 && v3 >= thr;
            a0 |= g0; a1 |= g1; a2 |= g2; a3 |= g3;
            mine += g0 + g1 + g2 + g3;
            if (u8 && owner) {
                const unsigned int q0 = v0 < thr ? 0u : 1u, q1 = v1 < thr ? 0u : 1u, q2 = v2 < thr ? 0u : 1u, q3 = v3 < thr ? 0u : 1u;
                if (whole) *reinterpret_cast<unsigned int*>(u8 + fq) = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
                else {
                    u8[fq] = (unsigned char)q0;
                    if (fq + 1 < n_total) u8[fq + 1] = (unsigned char)q1;
                    if (fq + 2 < n_total) u8[fq + 2] = (unsigned char)q2;
                }
            }
        }
        // (masks m* already confine the flags to this slab's columns; waves differ in sh, so the merge goes through LDS)
        if (a0) atomicOr(&s_any[c0], 1);
        if (a1) atomicOr(&s_any[c0 + 1], 1);
        if (a2) atomicOr(&s_any[c0 + 2], 1);
        if (a3) atomicOr(&s_any[c0 + 3], 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(&s_cnt[1], mine);
    __syncthreads();
    // columns k0 + tid: 64 per wave, one ballot per wave
    const int k = k0 + tid;
    const bool on = tid < nc && s_any[tid] != 0;
    const unsigned long long m = __ballot(on);
    if (m) {
        if (on && cell_hist) atomicAdd(&s_hist[finish_bin(tab, k)], 1);
        if (lane == 0) {
            atomicAdd(&s_cnt[0], __popcll(m));
            if (bits) {
                const int word = k >> 6, off = k & 63;              // lane 0's column: the ballot's bit 0
                atomicOr(&bits[(size_t)b * W + word], m << off);
                if (off && (m >> (64 - off))) atomicOr(&bits[(size_t)b * W + word + 1], m >> (64 - off));
            }
        }
    }
    __syncthreads();
    if (tid == 0 && cell_count && s_cnt[0]) atomicAdd(&cell_count[b], s_cnt[0]);
    if (tid == 1 && nnz && s_cnt[1]) atomicAdd(&nnz[b], s_cnt[1]);
    if (cell_hist && tid < tab.nb && s_hist[tid]) atomicAdd(&cell_hist[(size_t)b * tab.nb + tid], s_hist[tid]);
#endif
}

// ---------------------------------------------------------------------------------------------
// k_finish_graph: one workgroup per complex over x (B, N, F) and adj (B, N, N), 2 <= N <= CCSD_FIN_MAXN, F <= CCSD_FIN_MAXN
//   adj_int (B, N, N) int64   finish_quant(adj, thr): quantize (thr >= 0) or quantize_mol (thr < 0), as k_quantize
//   degree (B, N)             number of j != i with adj_int[i][j] != 0
//   degree_hist (B, N)        bin d = number of node slots i with degree d (bin 0: isolated and masked slots too); bins 1.. are
//                             nx.degree_histogram of adjs_to_graphs(quantize(adj)) (graph_utils.py:216-251, which drops isolated nodes)
//   edge_hist (B, 4)          pairs i < j by adj_int[i][j]
//   n_nodes (B,)              rows of x with a non-zero entry (cc_from_incidence's node rule, cc_utils.py:199-213)
//   x_hist (B, F)             nodes with x[i][f] > 0.5 (column sums of the xi of sampler.py:1222)
// Every output is nullable; x == NULL skips the x part, adj == NULL the adjacency part.  A wave takes a row of adj at a time (lanes
// along the row: coalesced loads, 8-byte stores), so N^2 never has to fit registers or LDS; the per-node counters live in LDS.
// ---------------------------------------------------------------------------------------------
#define CCSD_FIN_MAXN 512
__global__ void k_finish_graph(const float* __restrict__ x, const float* __restrict__ adj, int N, int F, float thr,
                               long long* __restrict__ adj_int, int* __restrict__ degree, int* __restrict__ degree_hist,
                               int* __restrict__ edge_hist, int* __restrict__ n_nodes, int* __restrict__ x_hist) {
    const int b = blockIdx.x;
    __shared__ int s_deg[CCSD_FIN_MAXN], s_dh[CCSD_FIN_MAXN], s_xh[CCSD_FIN_MAXN], s_row[CCSD_FIN_MAXN];
    __shared__ int s_eh[4], s_nn;
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int i = tid; i < CCSD_FIN_MAXN; i += nth) { s_deg[i] = 0; s_dh[i] = 0; s_xh[i] = 0; s_row[i] = 0; }
    for (int i = tid; i < 4; i += nth) s_eh[i] = 0;      // (loops, not `tid < 4`: the host emulation runs one thread per workgroup)
    if (tid == 0) s_nn = 0;
    __syncthreads();
    if (adj) {
        const float* Ab = adj + (size_t)b * N * N;
        long long* Qb = adj_int ? adj_int + (size_t)b * N * N : nullptr;
        int h0 = 0, h1 = 0, h2 = 0, h3 = 0;
#ifdef CCSD_EMU
        for (int i = 0; i < N; ++i) {
            int cnt = 0;
            for (int j = 0; j < N; ++j) {
                const int q = finish_quant(Ab[(size_t)i * N + j], thr);
                if (Qb) Qb[(size_t)i * N + j] = q;
                cnt += q != 0 && j != i;
                if (j > i) { h0 += q == 0; h1 += q == 1; h2 += q == 2; h3 += q == 3; }
            }
            s_deg[i] = cnt;
        }
        s_eh[0] = h0; s_eh[1] = h1; s_eh[2] = h2; s_eh[3] = h3;
#else
        const int wave = wave_index(), lane = tid & 63, nw = nth >> 6;
        for (int i = wave; i < N; i += nw) {
            int cnt = 0;
            for (int j = lane; j < N; j += 64) {
                const int q = finish_quant(Ab[(size_t)i * N + j], thr);
                if (Qb) Qb[(size_t)i * N + j] = q;
                cnt += q != 0 && j != i;
                if (j > i) { h0 += q == 0; h1 += q == 1; h2 += q == 2; h3 += q == 3; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
            if (lane == 0) s_deg[i] = cnt;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            h0 += __shfl_xor(h0, o, 64); h1 += __shfl_xor(h1, o, 64); h2 += __shfl_xor(h2, o, 64); h3 += __shfl_xor(h3, o, 64);
        }
        if (lane == 0) { atomicAdd(&s_eh[0], h0); atomicAdd(&s_eh[1], h1); atomicAdd(&s_eh[2], h2); atomicAdd(&s_eh[3], h3); }
#endif
    }
    if (x) {
        const float* Xb = x + (size_t)b * N * F;
        for (int idx = tid; idx < N * F; idx += nth) {
            const float v = Xb[idx];
            if (v > 0.5f) finish_inc(&s_xh[idx % F]);
            if (v != 0.f) s_row[idx / F] = 1;                      // (every writer stores the same value)
        }
    }
    __syncthreads();
    for (int i = tid; i < N; i += nth) {
        if (adj) finish_inc(&s_dh[s_deg[i]]);
        if (x && s_row[i]) finish_inc(&s_nn);
    }
    __syncthreads();
    if (adj) {
        for (int i = tid; i < N; i += nth) {
            if (degree) degree[(size_t)b * N + i] = s_deg[i];
            if (degree_hist) degree_hist[(size_t)b * N + i] = s_dh[i];
        }
        if (edge_hist)
            for (int i = tid; i < 4; i += nth) edge_hist[(size_t)b * 4 + i] = s_eh[i];
    }
    if (x) {
        if (x_hist)
            for (int f = tid; f < F; f += nth) x_hist[(size_t)b * F + f] = s_xh[f];
        if (n_nodes && tid == 0) n_nodes[b] = s_nn;
    }
}
