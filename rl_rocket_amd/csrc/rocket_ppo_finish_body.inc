// rocket_ppo_finish_body.inc — the body of the learner's finish kernel, included as text inside the
// kernels that share it: ppo_finish_kernel (rocket_ppo.inc; CTL false) and ppo_opts_finish_kernel
// (ppo_opts/rocket_ppo_opts.hip; CTL true, `ca` its ppo::CtlArgs); bc_finish_kernel (bc/rocket_bc.hip;
// CTL false, stats null, nwg 0 for the value half) adds its own lines after it; a2c_finish_kernel
// (a2c/rocket_a2c.hip; CTL false, stats null) its statistics in a block row of its own. Text and not a function: taken
// through a call, even an inlined one, ppo_finish_kernel's machine code changed. In scope where it
// is included: OBS, ACT, CTL, ca and the kernel's arguments (part, nwg, bs, ent_coef, src, dst,
// stats, normw, step0).
// CTL (stats required): each statistic's thread also adds it to the control block's running sum,
// and the approx_kl thread takes the stop decision (ppo::Ctl).
    using PT = ppo::Part<OBS, ACT>;
    static_assert(kFinElems * kFinGroups == 256, "block shape");
    static_assert(kFinElems == kWave / 2, "the norm sum is a half-wave sum");
    __shared__ float red[kFinGroups][kFinElems];
    const int tw = blockIdx.y;
    const int l = threadIdx.x % kFinElems, grp = threadIdx.x / kFinElems;
    const int e = blockIdx.x * kFinElems + l;
    float s = 0.0f;
    if (e < PT::SIZE) {
        const float* p = part + (int64_t)tw * nwg * PT::SIZE + e;
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int w = grp;
        // four rounds' 16 loads in flight at once, then added in the rounds' order
        for (; w + 15 * kFinGroups < nwg; w += 16 * kFinGroups) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = p[(int64_t)(w + u * kFinGroups) * PT::SIZE];
            __builtin_amdgcn_sched_barrier(0);  // the scheduler otherwise waits for each load in turn
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] += v[4 * r + u];
        }
        for (; w + 3 * kFinGroups < nwg; w += 4 * kFinGroups)
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] += p[(int64_t)(w + u * kFinGroups) * PT::SIZE];
        for (; w < nwg; w += kFinGroups) a[0] += p[(int64_t)w * PT::SIZE];
        s = (a[0] + a[1]) + (a[2] + a[3]);
    }
    red[grp][l] = s;
    __syncthreads();
    if (grp != 0) return;
    float v = 0.0f;
#pragma unroll
    for (int g = 0; g < kFinGroups; ++g) v += red[g][l];
    float* out = nullptr;  // where element e's gradient goes (none: padding, statistics)
    float* const* G = dst.p + 4 * tw;  // W1 b1 W2 b2 of this tower
    if (e >= PT::SIZE) {
    } else if (e < PT::W1) {
        const int lane = e % 64, reg = (e / 64) % 16, blk = e / 1024;
        const int u2 = 32 * (blk >> 1) + ppo::drow(reg, lane >> 5), u1 = 32 * (blk & 1) + (lane & 31);
        out = &G[2][u2 * 64 + u1];
    } else if (e < PT::B2) {
        const int i = e - PT::W1, lane = i % 64, reg = (i / 64) % 16, m = i / 1024;
        const int u1 = 32 * m + ppo::drow(reg, lane >> 5), col = lane & 31;
        if (col < OBS) out = &G[0][u1 * OBS + col];
        else if (col == OBS) out = &G[1][u1];
    } else if (e < PT::HW) {
        out = &G[3][e - PT::B2];
    } else if (e < PT::HB) {
        const int i = e - PT::HW, a = i / 64, u = i % 64;
        if (tw == 0) out = &dst.p[8][a * 64 + u];
        else if (a == 0) out = &dst.p[10][u];
    } else if (e < PT::LS) {
        const int a = e - PT::HB;
        if (tw == 0 && a < ACT) out = &dst.p[9][a];
        else if (tw == 1 && a == 0) out = &dst.p[11][0];
    } else if (e < PT::ST) {
        const int a = e - PT::LS;
        if (tw == 0 && a < ACT) {
            out = &dst.p[12][a];
            v -= ent_coef;  // d(ent_coef * -sum(0.5 + 0.5 log 2 pi + log_std))
        }
    } else if (stats) {
        const int k = e - PT::ST;
        const float inv_b = 1.0f / (float)bs;
        if (tw == 0) {
            if (k == 0) stats[0] = v * inv_b;  // policy_loss
            if (k == 1) stats[3] = v * inv_b;  // clip_fraction
            if (k == 2) stats[4] = v * inv_b;  // approx_kl
            if (k == 3) {
                float ent = 0.0f;
                for (int a = 0; a < ACT; ++a) ent += 1.41893853320467274f + src.p[12][a];  // 0.5 + 0.5 log 2 pi
                stats[2] = ent;  // entropy (per sample; the loss term is -ent)
            }
        } else if (k == 0) {
            stats[1] = v * inv_b;  // value_loss
        }
        if constexpr (CTL) {
            float* c = ca.ctl;
            if (c && tw == 0) {
                if (k == 0) c[ppo::kSumPg] += stats[0];
                if (k == 1) c[ppo::kSumClip] += stats[3];
                if (k == 2) {
                    const float kl = stats[4];
                    c[ppo::kKlSum] = ca.epoch_start ? kl : c[ppo::kKlSum] + kl;
                    c[ppo::kKlCount] = ca.epoch_start ? 1.0f : c[ppo::kKlCount] + 1.0f;
                    c[ppo::kKlLast] = kl;
                    c[ppo::kEvals] += 1.0f;
                    if (ca.epoch_start) c[ppo::kEpochs] += 1.0f;
                    c[ppo::kDecide] = kl > ca.kl_limit ? 1.0f : 0.0f;
                }
                if (k == 3) c[ppo::kSumEnt] += stats[2];
            } else if (c && k == 0) {
                c[ppo::kSumVf] += stats[1];
            }
        }
    }
    if (out) *out = v;
    if (normw) {
        float g2 = out ? v * v : 0.0f;
#pragma unroll
        for (int o = kFinElems / 2; o >= 1; o >>= 1) g2 += __shfl_xor(g2, o);
        if (l == 0) {
            normw[tw * gridDim.x + blockIdx.x] = g2;
            if (tw == 0 && blockIdx.x == 0) normw[2 * gridDim.x] = *step0 + 1.0f;
        }
    }
