// ccsd_lg_fin.inc -- the body of k_lg_fin / k_lg_fin_w (ccsd_k_lg.h includes it once per kernel): LG_FIN_KERNEL = the kernel's name,
// LG_FIN_CHAIN = the mlp_chain_tile call(s) of its chain shapes on (m, wp, X, NN, p0, ident, epi).  One text, so that the two kernels cannot
// drift apart, and k_lg_fin's code does not depend on its sibling.
__global__ __launch_bounds__(CCSD_LG_TB) void LG_FIN_KERNEL(MlpD m, const float* __restrict__ wp, const float* __restrict__ S, long long sstride, int N,
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
            LG_FIN_CHAIN
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
