// ccsd_k_mol.h -- k_mol_correct, k_mol_check_labels: molecule post-processing (valency correction, largest fragment).
// Part of the kernel source of libccsd_hip.so (see ccsd_kernels.h for the map).
//
// For molecule runs the reference does not score the quantised samples as sampled: gen_mol (utils/mol_utils.py:191-229) passes every
// sample through construct_mol (:144-188, formal charges while the bonds are added), correct_mol (:256-300, over-valent bonds lowered)
// and valid_mol_can_with_seg (:303-326, the largest fragment).  k_mol_correct restates the three on integer bond orders, without rdkit:
// what rdkit decides there -- the largest permitted valence of an element, neutral or with charge +1 -- is the caller's table.
//
// The molecule: atom slots 0..N-1, N <= 64; slot i holds an atom when 0 <= labels[i] < L.  Pair (i, j), i < j, has the bond order
// finish_quant(adj[i][j], mol mode) = 0..3, read from row i = the smaller index, the convention of k_lift_* and k_hodge_laplacian; the
// diagonal and the lower triangle are never read.  For the symmetric adjacency a sampler produces this is the reference's
// adj[start, end], start > end.  A bond to a slot without an atom is ignored (the reference drops those slots before it adds a bond).
//
// Construction.  Bonds enter in the reference's order, ascending (larger index, smaller index): (1,0), (2,0), (2,1), (3,0), ...; each gets
// the next insertion number.  After every bond the first atom in slot order whose bond-order sum exceeds max_valence[label][charge] is
// looked up (check_valency reports rdkit's first over-valent atom); if it may take a charge (charge_base[label] > 0) and its sum is
// charge_base + 1, its charge becomes +1.  An earlier atom that stays over-valent masks every later one, as in the reference.
// no_correct = no atom is over-valent once all bonds are in.
// Correction.  While some atom is over-valent: the first such atom in slot order; among its bonds the one of highest order, on a tie the
// one of lowest insertion number (rdkit's per-atom bond order under Python's stable sort); its order drops by one.  A bond that reaches 0
// is gone; one that remains gets a fresh insertion number (the reference removes and re-adds it).  The total bond order falls with every
// pass, so the loop ends.
// Fragments.  The connected components of the corrected molecule over 64-bit row masks, in ascending order of their lowest slot; the one
// with the most atoms is kept, on a tie the first.  Every other atom is dropped: label -1, bonds 0, charge 0.
#pragma once
#include "ccsd_dev.h"
#include "ccsd_k_finish.h"

#define CCSD_MOL_MAXN 64
#define CCSD_MOL_MAXL 16
// per-label data of the call, by value: max_valence (L, 2) = [neutral, charge +1] and charge_base (L,)
struct MolTab {
    int L;
    int maxv[CCSD_MOL_MAXL][2];
    int cbase[CCSD_MOL_MAXL];
};
// LDS bytes of one molecule: the insertion numbers (N, N) uint16 -- below 2016 + 2 * 2016 whatever the molecule: a bond enters once and
// is re-added at most twice -- then the bond orders (N, N) uint8, both symmetric
static __host__ __device__ inline int mol_lds_bytes(int N) { return (N * N * 3 + 15) & ~15; }

// One wave per molecule, lane l = atom slot l.  The per-lane values are arrays of MOL_NL entries: one on the GPU (a register), 64 in the
// host emulation, whose single thread takes the lanes in turn; MOL_LANES(l) is the lane's own statement there and a loop over the 64
// lanes here.  Everything outside MOL_LANES is wave-uniform.
#ifdef CCSD_EMU
#define MOL_NL 64
#define MOL_LANES(l) for (int l = 0; l < 64; ++l)
#define MOL_AT(l) (l)
#else
#define MOL_NL 1
#define MOL_LANES(l) for (int l = (int)(threadIdx.x & 63), once_ = 1; once_; once_ = 0)
#define MOL_AT(l) 0
#endif
// the wave's LDS writes before its (other lanes') LDS reads
CCSD_DEV void mol_wave_sync() {
#ifndef CCSD_EMU
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#endif
}
// bit l = lane l's flag
CCSD_DEV unsigned long long mol_ballot(const int* flag) {
#ifdef CCSD_EMU
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l)
        if (flag[l]) m |= 1ull << l;
    return m;
#else
    return __ballot(flag[0] != 0);
#endif
}
// the largest key of the wave, as a wave-uniform value
CCSD_DEV int mol_max(const int* key) {
#ifdef CCSD_EMU
    int m = key[0];
    for (int l = 1; l < 64; ++l) m = key[l] > m ? key[l] : m;
    return m;
#else
    int m = key[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    return __builtin_amdgcn_readfirstlane(m);
#endif
}
struct MolAtoms {      // per lane: has an atom, bond-order sum, charge, the label's two maxima and charge base
    int on[MOL_NL], sum[MOL_NL], chg[MOL_NL], mv0[MOL_NL], mv1[MOL_NL], cb[MOL_NL];
};
// the first over-valent atom in slot order, -1 when there is none: one ballot
CCSD_DEV int mol_first_over(const MolAtoms& a) {
    int over[MOL_NL];
    MOL_LANES(l) over[MOL_AT(l)] = a.on[MOL_AT(l)] && a.sum[MOL_AT(l)] > (a.chg[MOL_AT(l)] ? a.mv1[MOL_AT(l)] : a.mv0[MOL_AT(l)]);
    const unsigned long long m = mol_ballot(over);
    return m ? __builtin_ctzll(m) : -1;
}

// ---------------------------------------------------------------------------------------------
// k_mol_correct: grid ceil(B / waves per workgroup), one molecule per wave, mol_lds_bytes(N) of dynamic LDS per wave; no workgroup barrier
// (a wave past the batch leaves at once).  adj (B, N, N) fp32, labels (B, N) int32 (negative or >= L: no atom).  Outputs, all written in
// full for every molecule, slots not compacted:
//   mol_adj (B, N, N) uint8     symmetric bond orders, zero diagonal          mol_labels (B, N) int32, mol_charge (B, N) int8
//   no_correct (B,) uint8       n_corrections (B,) int32: the decrements      n_fragments (B,) int32: after correction, before selection
//   atoms (B,) int32            the atoms kept
// largest_fragment = 0 keeps every fragment.
// ---------------------------------------------------------------------------------------------
__global__ void k_mol_correct(const float* __restrict__ adj, const int* __restrict__ labels, int B, int N, MolTab tab, int largest_fragment,
                              unsigned char* __restrict__ mol_adj, int* __restrict__ mol_labels, signed char* __restrict__ mol_charge,
                              unsigned char* __restrict__ no_correct, int* __restrict__ n_corrections, int* __restrict__ n_fragments,
                              int* __restrict__ atoms) {
    CCSD_DYN_SMEM(smem);
#ifdef CCSD_EMU
    const int wave = 0, b = (int)blockIdx.x;
#else
    const int wave = wave_index(), b = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
#endif
    if (b >= B) return;
    unsigned short* s_ins = (unsigned short*)((unsigned char*)smem + (size_t)wave * mol_lds_bytes(N));
    unsigned char* s_ord = (unsigned char*)(s_ins + N * N);
    const float* Ab = adj + (size_t)b * N * N;
    const int* Lb = labels + (size_t)b * N;
    const int NN = N * N;

    MolAtoms a;
    int lab[MOL_NL];
    MOL_LANES(l) {
        const int v = l < N ? Lb[l] : -1, ok = v >= 0 && v < tab.L;
        lab[MOL_AT(l)] = ok ? v : -1;
        a.on[MOL_AT(l)] = ok;
        a.sum[MOL_AT(l)] = a.chg[MOL_AT(l)] = 0;
        a.mv0[MOL_AT(l)] = ok ? tab.maxv[v][0] : 0;
        a.mv1[MOL_AT(l)] = ok ? tab.maxv[v][1] : 0;
        a.cb[MOL_AT(l)] = ok ? tab.cbase[v] : 0;
    }
    // the bond orders, both triangles from the upper one; a pair with a slot that holds no atom has order 0
    for (int base = 0; base < NN; base += 64)
        MOL_LANES(l) {
            const int idx = base + l;
            if (idx < NN) {
                const int i = idx / N, j = idx - i * N;
                if (i == j) s_ord[idx] = 0;
                if (i < j) {
                    const int li = Lb[i], lj = Lb[j];
                    const int q = li >= 0 && li < tab.L && lj >= 0 && lj < tab.L ? finish_quant(Ab[idx], -1.0f) : 0;
                    s_ord[idx] = (unsigned char)q;
                    s_ord[j * N + i] = (unsigned char)q;
                }
            }
        }
    mol_wave_sync();

    // construction
    int next = 0;                                                        // the next insertion number
    for (int s = 1; s < N; ++s) {
        int has[MOL_NL];
        MOL_LANES(l) has[MOL_AT(l)] = l < s && s_ord[s * N + l] != 0;
        for (unsigned long long m = mol_ballot(has); m; m &= m - 1) {
            const int e = __builtin_ctzll(m), o = s_ord[s * N + e];
            MOL_LANES(l) {
                if (l == e) s_ins[s * N + e] = s_ins[e * N + s] = (unsigned short)next;
                if (l == e || l == s) a.sum[MOL_AT(l)] += o;
            }
            ++next;
            const int f = mol_first_over(a);
            MOL_LANES(l)
                if (l == f && a.cb[MOL_AT(l)] > 0 && a.sum[MOL_AT(l)] == a.cb[MOL_AT(l)] + 1) a.chg[MOL_AT(l)] = 1;
        }
    }
    mol_wave_sync();
    int f = mol_first_over(a);
    const int clean = f < 0;

    // correction
    int ncorr = 0;
    while (f >= 0) {
        int key[MOL_NL];                                                 // order, then the earlier insertion, then (unique anyway) the slot
        MOL_LANES(l) {
            const int o = l < N ? s_ord[f * N + l] : 0;
            key[MOL_AT(l)] = o ? (o << 22) | ((0xFFFF - (int)s_ins[f * N + l]) << 6) | l : 0;
        }
        const int best = mol_max(key);
        if (!best) break;                                                // (an atom over-valent without a bond: a negative maximum, which ccsd_mol_correct refuses)
        const int j = best & 63, o = (best >> 22) - 1;
        MOL_LANES(l) {
            if (l == j) {
                s_ord[f * N + j] = s_ord[j * N + f] = (unsigned char)o;
                if (o) s_ins[f * N + j] = s_ins[j * N + f] = (unsigned short)next;
            }
            if (l == j || l == f) a.sum[MOL_AT(l)] -= 1;
        }
        if (o) ++next;
        ++ncorr;
        mol_wave_sync();
        f = mol_first_over(a);
    }

    // fragments: lane l keeps row l of the corrected molecule as a mask
    unsigned long long row[MOL_NL];
    MOL_LANES(l) row[MOL_AT(l)] = 0;
    for (int i = 0; i < N; ++i) {
        int has[MOL_NL];
        MOL_LANES(l) has[MOL_AT(l)] = l < N && s_ord[i * N + l] != 0;
        const unsigned long long m = mol_ballot(has);
        MOL_LANES(l)
            if (l == i) row[MOL_AT(l)] = m;
    }
    const unsigned long long present = mol_ballot(a.on);
    unsigned long long seen = 0, keep = 0;
    int nfrag = 0, kept = 0;
    while (present & ~seen) {
        unsigned long long comp = 1ull << __builtin_ctzll(present & ~seen);
        for (;;) {                                                       // one ballot per breadth-first layer
            int touch[MOL_NL];
            MOL_LANES(l) touch[MOL_AT(l)] = (row[MOL_AT(l)] & comp) != 0;
            const unsigned long long grown = comp | mol_ballot(touch);
            if (grown == comp) break;
            comp = grown;
        }
        seen |= comp;
        ++nfrag;
        const int cnt = __builtin_popcountll(comp);
        if (cnt > kept) { kept = cnt; keep = comp; }
    }
    if (!largest_fragment) { keep = present; kept = __builtin_popcountll(present); }

    // outputs
    MOL_LANES(l) {
        if (l < N) {
            const int in = (int)((keep >> l) & 1);
            mol_labels[(size_t)b * N + l] = in ? lab[MOL_AT(l)] : -1;
            mol_charge[(size_t)b * N + l] = (signed char)(in ? a.chg[MOL_AT(l)] : 0);
        }
        if (l == 0) {
            no_correct[b] = (unsigned char)clean;
            n_corrections[b] = ncorr;
            n_fragments[b] = nfrag;
            atoms[b] = kept;
        }
    }
    unsigned char* Ob = mol_adj + (size_t)b * NN;
    for (int base = 0; base < NN; base += 64)
        MOL_LANES(l) {
            const int idx = base + l;
            if (idx < NN) {
                const int i = idx / N, j = idx - i * N;
                Ob[idx] = ((keep >> i) & (keep >> j) & 1) ? s_ord[idx] : (unsigned char)0;
            }
        }
}

// flag[0] = 1 when a label is >= L (ZERO on entry); a grid-stride loop
__global__ void k_mol_check_labels(const int* __restrict__ labels, long long n, int L, int* __restrict__ flag) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        if (labels[i] >= L) *flag = 1;
}
