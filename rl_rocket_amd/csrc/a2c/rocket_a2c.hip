// rocket_a2c.hip — the nineteenth translation unit of librocket_hip.so: SB3's A2C on the device
// (rr_a2c_update), one A2C.train() for the MlpPolicy actor-critic with a diagonal Gaussian:
//   A    = advantages[idx], or (A - mean) / (std + 1e-8) with normalize_advantage
//   pg   = -mean(A log_prob(a))                      no ratio: the stored log-probs are never read
//   vf   = mean((ret - V)^2)                         F.mse_loss(returns, values)
//   ent  = -mean(entropy) = -sum(0.5 + 0.5 log 2 pi + log_std)
//   loss = pg + ent_coef ent + vf_coef vf
//   clip_grad_norm_, then RMSprop (SB3's RMSpropTFLike or torch.optim.RMSprop) or Adam (use_rms_prop=False).
// Four launches: the learner's prep (ppo_prep_body: advantage sums and packing), the gradient of both
// towers (the pi tower is ppo_grad_tower with LOSS 4, the vf tower the learner's unclipped one), the
// learner's finish body as text with a third row of blocks for the statistics, and the optimizer
// (a2c/rocket_rmsprop_body.inc, or the learner's Adam body with no next-minibatch blocks). Launched
// through rrc_launch_a2c with an A2cLaunch. Compiled with the collect translation unit's settings
// (build.py COLLECT_FLAGS), because the gradient kernel's loop is the learner's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_ppo.inc"

namespace {

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void a2c_prep_kernel(const float* __restrict__ adv, const int64_t* __restrict__ idx,
                                                       int64_t bs, double* __restrict__ part, PolSrc src,
                                                       float* __restrict__ pack)
{
    ppo_prep_body<OBS, ACT>(adv, idx, bs, part, src, pack);
}

template <int OBS, int ACT, bool NORM>
__global__ __launch_bounds__(ppo::kThreads) void a2c_grad_kernel(
    const float* __restrict__ obs, const float* __restrict__ act, const float* __restrict__ adv,
    const float* __restrict__ ret, const int64_t* __restrict__ idx, int64_t bs, float vf_coef,
    const double* __restrict__ adv_part, const float* __restrict__ pack, float* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
    if (blockIdx.y == 0)
        ppo_grad_tower<OBS, ACT, 0, false, NORM, 4>(lds, obs, act, nullptr, adv, ret, idx, bs, 0.0f, vf_coef, adv_part,
                                                    pack, part);
    else
        ppo_grad_tower<OBS, ACT, 1, false, true>(lds, obs, act, nullptr, adv, ret, idx, bs, 0.0f, vf_coef, adv_part,
                                                 pack, part);
}

// The statistics block (one block): the workgroups' -A logp and logp sums (pi rows) and squared-error sums
// (vf rows), thread = workgroup, each summed in a fixed order in fp64: butterflies within a wave, the four
// waves in order. stats = [policy_loss, value_loss, entropy, loss, mean log_prob, 0, 0, 0].
template <int OBS, int ACT>
__device__ __forceinline__ void a2c_stats_block(const float* __restrict__ part, int nwg, int64_t bs, float ent_coef,
                                                float vf_coef, const PolSrc& src, float* __restrict__ stats)
{
    using PT = ppo::Part<OBS, ACT>;
    __shared__ double sred[3][256 / kWave];
    static_assert(ppo::kMaxWG <= 256, "one workgroup's sums per thread");
    const bool own = (int)threadIdx.x < nwg;
    const int wg = own ? threadIdx.x : 0;
    const float* pi = part + (int64_t)wg * PT::SIZE + PT::ST;
    const float* vf = part + ((int64_t)nwg + wg) * PT::SIZE + PT::ST;
    const float pg0 = pi[0], lp0 = pi[1], se0 = vf[0];
    double s[3] = {own ? (double)pg0 : 0.0, own ? (double)lp0 : 0.0, own ? (double)se0 : 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        s[q] = ppo::wave_sum(s[q]);
        if ((threadIdx.x & (kWave - 1)) == 0) sred[q][threadIdx.x / kWave] = s[q];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot[3] = {};
    for (int q = 0; q < 3; ++q)
        for (int k = 0; k < 256 / kWave; ++k) tot[q] += sred[q][k];
    double ent = 0.0;
    for (int a = 0; a < ACT; ++a) ent += 1.41893853320467274 + (double)src.p[12][a];  // 0.5 + 0.5 log 2 pi
    const double pg = tot[0] / (double)bs, v = tot[2] / (double)bs;
    stats[0] = (float)pg;
    stats[1] = (float)v;
    stats[2] = (float)ent;
    stats[3] = (float)(pg - (double)ent_coef * ent + (double)vf_coef * v);
    stats[4] = (float)(tot[1] / (double)bs);
    stats[5] = stats[6] = stats[7] = 0.0f;
}

// grid (nfin, 2 or 3): blockIdx.y 0 the pi half, 1 the value half, 2 (one block) the statistics
template <int OBS, int ACT>
__global__ __launch_bounds__(256) void a2c_finish_kernel(const float* __restrict__ part, int nwg, int64_t bs,
                                                         float ent_coef, float vf_coef, PolSrc src, PolGrad dst,
                                                         float* __restrict__ a2c_stats, float* __restrict__ normw,
                                                         const float* __restrict__ step0)
{
    if (blockIdx.y == 2) {
        if (blockIdx.x == 0) a2c_stats_block<OBS, ACT>(part, nwg, bs, ent_coef, vf_coef, src, a2c_stats);
        return;
    }
    // the learner's statistics and control block are off; normw carries the clip's sums and the step count
    float* const stats = nullptr;
    constexpr bool CTL = false;
    const ppo::CtlArgs ca = {};
#include "rocket_ppo_finish_body.inc"
}

__global__ __launch_bounds__(kAdamThreads) void a2c_rmsprop_kernel(AdamList A, const float* __restrict__ normw, int n_norm,
                                                                   float max_norm, const float* __restrict__ lr_p,
                                                                   float alpha, float w, float eps, int eps_inside)
{
#include "rocket_rmsprop_body.inc"
}

// use_rms_prop=False: the learner's clip + Adam step; its repacked images are the next call's prep's to overwrite
template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void a2c_adam_kernel(AdamList A, const float* __restrict__ normw, int n_norm,
                                                                float max_norm, const float* __restrict__ lr_p,
                                                                float beta1, float beta2, float w1, float w2, float eps,
                                                                float* __restrict__ pack, int nbp)
{
    const AdvNext nx = {};  // no next-minibatch blocks: the grid is nbp
#include "rocket_ppo_adam_body.inc"
}

template <int OB, int A, bool NM>
int a2c_launch(const A2cLaunch& L, hipStream_t s)
{
    using PT = ppo::Part<OB, A>;
    using K = ppo::Pack<OB, A>;
    constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
    hipLaunchKernelGGL((a2c_prep_kernel<OB, A>), dim3(ppo::kAdvPart + (2 * K::SIZE + 255) / 256), dim3(256), 0, s,
                       L.advantages, L.idx, L.batch, L.adv_part, L.ps, L.pack);
    hipLaunchKernelGGL((a2c_grad_kernel<OB, A, NM>), dim3(L.nwg, 2), dim3(ppo::kThreads), 0, s, L.obs, L.actions,
                       L.advantages, L.returns, L.idx, L.batch, L.vf, (const double*)L.adv_part, (const float*)L.pack,
                       L.part);
    hipLaunchKernelGGL((a2c_finish_kernel<OB, A>), dim3(nfin, L.stats ? 3 : 2), dim3(256), 0, s, (const float*)L.part,
                       L.nwg, L.batch, L.ent, L.vf, L.ps, L.pg, L.stats, L.normw, (const float*)L.a.step[0]);
    if (L.optimizer == RR_A2C_ADAM)
        hipLaunchKernelGGL((a2c_adam_kernel<OB, A>), dim3(L.nbp), dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw,
                           2 * nfin, L.max_norm, L.lr, L.beta1, L.beta2, L.w1, L.w2, L.eps, L.pack, L.nbp);
    else
        hipLaunchKernelGGL(a2c_rmsprop_kernel, dim3(L.nbp), dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw,
                           2 * nfin, L.max_norm, L.lr, L.alpha, L.w1, L.eps, L.optimizer == RR_A2C_RMSPROP_TF ? 1 : 0);
    return (int)hipGetLastError();
}

}  // namespace

// rr_a2c_update's launches (declared in rocket_device.h); `launch` points to the A2cLaunch of the calling
// TU, which validated the arguments and carved the workspace.
extern "C" int rrc_launch_a2c(const void* launch, void* stream)
{
    const auto L = from_unit<A2cLaunch>(launch);
    hipStream_t s = (hipStream_t)stream;
    if (L.obs_dim == 14) return L.normalize ? a2c_launch<14, 3, true>(L, s) : a2c_launch<14, 3, false>(L, s);
    return L.normalize ? a2c_launch<7, 2, true>(L, s) : a2c_launch<7, 2, false>(L, s);
}
