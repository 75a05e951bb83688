// Host probe of the device helpers behind the noise stream (TEST INFRASTRUCTURE ONLY -- see ccsd_amd/csrc/ccsd_rt.h): philox4,
// philox_normal4, FastDiv, the flat split of k_noise_norm / k_langevin_apply / k_ew1, and k_noise_norm itself, compiled from the
// kernel source for the host.  tests/test_probe.py drives it through ctypes.
// Build: g++ -O2 -DCCSD_EMU -fPIC -shared -I ccsd_amd/csrc tests/emu/ccsd_probe.cpp -o tests/emu/_build/libccsd_probe.so
#ifndef CCSD_EMU
#error "compile with -DCCSD_EMU"
#endif
#include "ccsd_dev.h"
#ifdef CCSD_PROBE_FASTDIV_SPLIT
// a kernel source from before flat_split (given with -I): the split as its three kernels state it
CCSD_DEV void flat_split(int t, int K, int& e, int& k) { FastDiv(K).divmod(t, e, k); }
#endif
#include "ccsd_k_update.h"

extern "C" {

void probe_philox4(long long n, const unsigned int* ctr, const unsigned int* key, unsigned int* out) {
    for (long long i = 0; i < n; ++i) philox4(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1], out + 4 * i);
}

// groups g[i] of sample b, draw `draw`: out[i][4]
void probe_philox_normal4(long long n, unsigned long long seed, unsigned int draw, long long b, const unsigned int* g, float* out) {
    for (long long i = 0; i < n; ++i) philox_normal4(seed, draw, b, g[i], out + 4 * i);
}

// FastDiv(d) over t0 <= t < t1: number of t whose (quotient, remainder) is not (t / d, t % d); *first = the first such t (or -1)
long long probe_fastdiv_errors(int d, long long t0, long long t1, long long* first) {
    const FastDiv fd(d);
    long long bad = 0;
    *first = -1;
    for (long long t = t0; t < t1; ++t) {
        int q, r;
        fd.divmod((int)t, q, r);
        if (q != (int)(t / d) || r != (int)(t % d)) {
            if (!bad) *first = t;
            ++bad;
        }
    }
    return bad;
}

// the split of the first element of every flat group of an (E, K) block, exhaustively: groups whose (e, k) is not
// (4 g / K, 4 g % K); low / high = how many of them have the quotient below / above.  fastdiv != 0: FastDiv(K) in its place.
// (t0, step) = (0, 4) visits every group; other values a slice or a stride of them (both multiples of 4).
long long probe_split_errors(int E, int K, int fastdiv, long long t0, long long step, long long* low, long long* high) {
    const long long EK = (long long)E * K;
    const FastDiv fd(K);
    long long bad = 0;
    *low = *high = 0;
    for (long long t = t0; t < EK; t += step) {
        int e, k;
        if (fastdiv) fd.divmod((int)t, e, k);
        else flat_split((int)t, K, e, k);
        const int we = (int)(t / K), wk = (int)(t % K);
        if (e != we || k != wk) {
            ++bad;
            if (e < we) ++*low;
            if (e > we) ++*high;
        }
    }
    return bad;
}

// k_noise_norm<0, 0> with all-ones draws on a batch of two complexes, complex `full` switched on entirely and the other one off
// entirely, mask tables laid out as the workspace lays them out ([B][Kp] then [B][Ep], rows padded with zeros to multiples of 4;
// a zeroed guard band on both sides keeps a wrong split's reads inside the allocation).  counts[b] = sum over the complex of
// (z mask)^2 = the number of entries that got mask 1: E K for the full complex, 0 for the empty one.
void probe_noise_norm_counts(int E, int K, int full, double* counts) {
    const int B = 2, Kp = (K + 3) & ~3, Ep = (E + 3) & ~3, guard = 64;
    const size_t EK = (size_t)E * K;
    std::vector<unsigned char> tab(guard + (size_t)B * (Kp + Ep) + guard, 0);
    unsigned char* mfr = tab.data() + guard;
    unsigned char* mfl = mfr + (size_t)B * Kp;
    for (int k = 0; k < K; ++k) mfr[(size_t)full * Kp + k] = 1;
    for (int e = 0; e < E; ++e) mfl[(size_t)full * Ep + e] = 1;
    std::vector<float> z(B * EK, 1.0f);
    NoiseArgs na{};
    na.zr = z.data();
    na.flat_r = 1;
    const int nchunk = (int)(((EK + 3) / 4 + CCSD_NN_CH - 1) / CCSD_NN_CH);
    std::vector<float> zpart((size_t)B * nchunk, -1.0f);
    float* zp = zpart.data();
    const MaskTab mt{mfr, mfl, Kp, Ep};
    CCSD_LAUNCH((k_noise_norm<0, 0>), dim3(nchunk, B), dim3(CCSD_NTHREADS), 0, nullptr, na, mt, E, K, zp);
    for (int b = 0; b < B; ++b) {
        double s = 0.0;
        for (int c = 0; c < nchunk; ++c) s += zpart[(size_t)b * nchunk + c];      // (each partial <= 16384: exact in fp32)
        counts[b] = s;
    }
}

}
