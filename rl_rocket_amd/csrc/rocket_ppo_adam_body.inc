// rocket_ppo_adam_body.inc — the body of rr_ppo_update's optimizer kernel, included as text inside
// the kernels that share it: adam_chain_kernel (rocket_ppo.inc) and ppo_opts_adam_kernel
// (ppo_opts/rocket_ppo_opts.hip, which obeys the control block before it and counts the step after
// it); bc_adam_kernel (bc/rocket_bc.hip) sets max_norm 0 and an empty nx; a2c_adam_kernel (a2c/rocket_a2c.hip,
// SB3's use_rms_prop=False) an empty nx. Text and not a function
// for rocket_ppo_finish_body.inc's reason. In scope where it is included: OBS, ACT and the kernel's
// arguments (A, normw, n_norm, max_norm, lr_p, beta1, beta2, w1, w2, eps, pack, nx, nbp). A block past
// nbp returns from inside it.
    if ((int)blockIdx.x >= nbp) {
        __shared__ double red[2][kAdamThreads / kWave];
        const int sub = threadIdx.x / 256, t = threadIdx.x % 256, b = (blockIdx.x - nbp) * 4 + sub;
        double s = 0.0, q = 0.0;
        ppo::adv_sums(nx.adv, nx.idx, nx.bs, (int64_t)b * 256 + t, s, q);
        s = ppo::wave_sum(s);
        q = ppo::wave_sum(q);
        const int w = threadIdx.x / kWave;
        if ((threadIdx.x & (kWave - 1)) == 0) {
            red[0][w] = s;
            red[1][w] = q;
        }
        __syncthreads();
        if (t == 0) {
            double ss = 0.0, qq = 0.0;
            for (int k = 0; k < 256 / kWave; ++k) {
                ss += red[0][sub * (256 / kWave) + k];
                qq += red[1][sub * (256 / kWave) + k];
            }
            nx.part[2 * b] = ss;
            nx.part[2 * b + 1] = qq;
        }
        return;
    }
    __shared__ float red[kAdamThreads / kWave];
    // Every wave holds elements of one tensor (wstart: sizes rounded up to a wave), so the tensor
    // and its pointers are scalar and the parameter scatter below branches per wave, not per lane.
    // The element's four loads go first, unmasked (a padding lane reads element 0): their round
    // trip overlaps the norm's.
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t wbase = (int64_t)blockIdx.x * kAdamThreads + (int64_t)wv * kWave;
    int t = 0;
    while (t + 1 < A.n && wbase >= A.wstart[t + 1]) ++t;
    const int64_t kw = wbase - A.wstart[t] + (threadIdx.x & (kWave - 1));
    const bool live = wbase < A.wstart[A.n] && kw < A.start[t + 1] - A.start[t];
    const int64_t k = live ? kw : 0;
    const float g0 = A.grad[t][k], m0 = A.exp_avg[t][k], v0 = A.exp_avg_sq[t][k], p0 = A.param[t][k];
    float part = 0.0f;
    for (int b = threadIdx.x; b < n_norm; b += kAdamThreads) part += normw[b];
    const float tot = block_sum<kAdamThreads>(part, red);
    const float step = normw[n_norm], lr = *lr_p;
    const float coef = max_norm > 0.0f ? fminf(max_norm / (sqrtf(tot) + 1e-6f), 1.0f) : 1.0f;
    const float bc1 = 1.0f - powf(beta1, step), bc2 = 1.0f - powf(beta2, step);
    const float sneg = -(1.0f / (bc1 / lr));
    const float d = sqrtf(bc2) * sneg, eos = 1.0f / (sneg / eps);
    if (live) {
        const float g = g0 * coef;
        A.grad[t][k] = g;
        const float mk = m0 + w1 * (g - m0);
        const float vk = v0 * beta2 + (w2 * g) * g;
        A.exp_avg[t][k] = mk;
        A.exp_avg_sq[t][k] = vk;
        const float pk = p0 + mk / (sqrtf(vk) / d + eos);
        A.param[t][k] = pk;
        pack_scatter<OBS, ACT>(pack, t, (int)k, pk);
    }
    if (blockIdx.x == 0 && threadIdx.x < A.n) *A.step[threadIdx.x] = step;
