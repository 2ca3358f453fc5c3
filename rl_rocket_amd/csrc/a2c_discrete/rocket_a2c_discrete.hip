// rocket_a2c_discrete.hip — the twentieth translation unit of librocket_hip.so: SB3's A2C on the device
// for the Categorical policy of the discrete 3DOF actions (rr_a2c_update_discrete), one A2C.train() behind
// a CategoricalDistribution over K = 2 .. 4 choices on the <7, 4> images:
//   A    = advantages[idx], or (A - mean) / (std + 1e-8) with normalize_advantage
//   lp   = logit_a - logsumexp(logits[:K])           no ratio: the stored log-probs are never read
//   H    = -sum_k p_k log p_k                        per sample: it depends on the state
//   pg   = -mean(A lp);  vf = mean((ret - V)^2);  ent = mean(H)
//   loss = pg - ent_coef ent + vf_coef vf
//   clip_grad_norm_, then RMSprop (SB3's RMSpropTFLike or torch.optim.RMSprop) or Adam (use_rms_prop=False).
// Four launches, each composed of what the other units have:
//   prep       ppo_prep_body's advantage sums; the packing blocks go through discrete_pack_value (zeros for
//              the heads >= K), as discrete/rocket_discrete.hip's do;
//   gradient   ppo_grad_tower<7, 4, 0, false, NORM, LOSS 5> (LOSS 2's softmax head and per-sample entropy
//              gradient with LOSS 4's d loss / d log_prob = -A / B) and the learner's unclipped vf tower;
//   finish     rocket_ppo_finish_body.inc as text over 12 tensors with the discrete unit's choice between
//              the gradient list and the sink for elements of heads >= K (ent_coef is 0 inside the body:
//              the entropy's gradient came with the head derivative), and a third row of blocks for the
//              statistics, as a2c/rocket_a2c.hip's;
//   optimizer  a2c/rocket_rmsprop_body.inc, or the learner's Adam body with no next-minibatch blocks and
//              the <7, 4> repack, over an AdamList of 12 tensors.
// No atomics. Launched through rrc_launch_a2c_discrete with an A2cDiscreteLaunch. Compiled with the collect
// translation unit's settings (build.py COLLECT_FLAGS), because the gradient kernel's loop is the learner's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_ppo.inc"

namespace {

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void a2cd_prep_kernel(const float* __restrict__ adv, const int64_t* __restrict__ idx,
                                                        int64_t bs, double* __restrict__ part, PolSrc src,
                                                        int n_choices, float* __restrict__ pack)
{
    using K = ppo::Pack<OBS, ACT>;
    if (blockIdx.x >= ppo::kAdvPart) {
        const int k = (blockIdx.x - ppo::kAdvPart) * 256 + threadIdx.x;
        if (k < 2 * K::SIZE) pack[k] = discrete_pack_value<OBS, ACT>(src, n_choices, k / K::SIZE, k % K::SIZE);
        return;
    }
    ppo_prep_body<OBS, ACT>(adv, idx, bs, part, src, pack);  // the advantage sums: these blocks pack nothing
}

template <int OBS, int ACT, bool NORM>
__global__ __launch_bounds__(ppo::kThreads) void a2cd_grad_kernel(
    const float* __restrict__ obs, const float* __restrict__ act, const float* __restrict__ adv,
    const float* __restrict__ ret, const int64_t* __restrict__ idx, int64_t bs, float ent_coef, float vf_coef,
    int n_choices, const double* __restrict__ adv_part, const float* __restrict__ pack, float* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
    if (blockIdx.y == 0)
        ppo_grad_tower<OBS, ACT, 0, false, NORM, 5>(lds, obs, act, nullptr, adv, ret, idx, bs, 0.0f, vf_coef, adv_part,
                                                    pack, part, nullptr, 0.0f, n_choices, ent_coef);
    else
        ppo_grad_tower<OBS, ACT, 1, false, true>(lds, obs, act, nullptr, adv, ret, idx, bs, 0.0f, vf_coef, adv_part,
                                                 pack, part);
}

// The statistics block (one block), a2c_stats_block with the entropy from the fourth per-sample sum: the
// workgroups' -A lp, lp and H sums (pi rows) and squared-error sums (vf rows), thread = workgroup, each summed
// in a fixed order in fp64: butterflies within a wave, the four waves in order.
// stats = [policy_loss, value_loss, mean H, loss, mean log_prob, 0, 0, 0].
template <int OBS, int ACT>
__device__ __forceinline__ void a2cd_stats_block(const float* __restrict__ part, int nwg, int64_t bs, float ent_coef,
                                                 float vf_coef, float* __restrict__ stats)
{
    using PT = ppo::Part<OBS, ACT>;
    __shared__ double sred[4][256 / kWave];
    static_assert(ppo::kMaxWG <= 256, "one workgroup's sums per thread");
    const bool own = (int)threadIdx.x < nwg;
    const int wg = own ? threadIdx.x : 0;
    const float* pi = part + (int64_t)wg * PT::SIZE + PT::ST;
    const float* vf = part + ((int64_t)nwg + wg) * PT::SIZE + PT::ST;
    const float pg0 = pi[0], lp0 = pi[1], h0 = pi[3], se0 = vf[0];
    double s[4] = {own ? (double)pg0 : 0.0, own ? (double)lp0 : 0.0, own ? (double)se0 : 0.0, own ? (double)h0 : 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        s[q] = ppo::wave_sum(s[q]);
        if ((threadIdx.x & (kWave - 1)) == 0) sred[q][threadIdx.x / kWave] = s[q];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot[4] = {};
    for (int q = 0; q < 4; ++q)
        for (int k = 0; k < 256 / kWave; ++k) tot[q] += sred[q][k];
    const double pg = tot[0] / (double)bs, v = tot[2] / (double)bs, ent = tot[3] / (double)bs;
    stats[0] = (float)pg;
    stats[1] = (float)v;
    stats[2] = (float)ent;
    stats[3] = (float)(pg - (double)ent_coef * ent + (double)vf_coef * v);
    stats[4] = (float)(tot[1] / (double)bs);
    stats[5] = stats[6] = stats[7] = 0.0f;
}

// grid (nfin, 2 or 3): blockIdx.y 0 the pi half, 1 the value half, 2 (one block) the statistics. Both lists'
// p[12] is four spare floats; dst_sink is dst_in with the action head's weight and bias gradients replaced
// by a [4][64] + [4] sink.
template <int OBS, int ACT>
__global__ __launch_bounds__(256) void a2cd_finish_kernel(const float* __restrict__ part, int nwg, int64_t bs,
                                                          int n_choices, float ent_coef_stats, float vf_coef,
                                                          PolSrc src, PolGrad dst_in, PolGrad dst_sink,
                                                          float* __restrict__ a2c_stats, float* __restrict__ normw,
                                                          const float* __restrict__ step0)
{
    if (blockIdx.y == 2) {
        if (blockIdx.x == 0) a2cd_stats_block<OBS, ACT>(part, nwg, bs, ent_coef_stats, vf_coef, a2c_stats);
        return;
    }
    // (the sink: see discrete_finish_kernel) an element of a head >= n_choices, a zero sum, goes to the sink
    // at the offsets the body computes, not past the [n_choices][64] weight and [n_choices] bias gradients
    using P = ppo::Part<OBS, ACT>;
    const int el = blockIdx.x * kFinElems + threadIdx.x % kFinElems;
    const bool spare = blockIdx.y == 0 && ((el >= P::HW + 64 * n_choices && el < P::HB) ||
                                           (el >= P::HB + n_choices && el < P::LS));
    const PolGrad& dst = spare ? dst_sink : dst_in;
    // the body's entropy lines are the Gaussian's: off. The learner's statistics and control block are off
    // too; normw carries the clip's sums and the step count
    constexpr float ent_coef = 0.0f;
    float* const stats = nullptr;
    constexpr bool CTL = false;
    const ppo::CtlArgs ca = {};
#include "rocket_ppo_finish_body.inc"
}

__global__ __launch_bounds__(kAdamThreads) void a2cd_rmsprop_kernel(AdamList A, const float* __restrict__ normw,
                                                                    int n_norm, float max_norm,
                                                                    const float* __restrict__ lr_p, float alpha, float w,
                                                                    float eps, int eps_inside)
{
#include "a2c/rocket_rmsprop_body.inc"
}

// use_rms_prop=False: the learner's clip + Adam step; its repacked <7, 4> images are the next call's prep's to
// overwrite (an element of a head >= K is no element of a tensor, so its zero stays)
template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void a2cd_adam_kernel(AdamList A, const float* __restrict__ normw, int n_norm,
                                                                 float max_norm, const float* __restrict__ lr_p,
                                                                 float beta1, float beta2, float w1, float w2, float eps,
                                                                 float* __restrict__ pack, int nbp)
{
    const AdvNext nx = {};  // no next-minibatch blocks: the grid is nbp
#include "rocket_ppo_adam_body.inc"
}

template <bool NM>
int a2cd_launch(const A2cDiscreteLaunch& D, hipStream_t s)
{
    constexpr int OB = 7, A = 4;
    const A2cLaunch& L = D.base;
    using PT = ppo::Part<OB, A>;
    using K = ppo::Pack<OB, A>;
    constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
    hipLaunchKernelGGL((a2cd_prep_kernel<OB, A>), dim3(ppo::kAdvPart + (2 * K::SIZE + 255) / 256), dim3(256), 0, s,
                       L.advantages, L.idx, L.batch, L.adv_part, L.ps, D.n_choices, L.pack);
    hipLaunchKernelGGL((a2cd_grad_kernel<OB, A, NM>), dim3(L.nwg, 2), dim3(ppo::kThreads), 0, s, L.obs, L.actions,
                       L.advantages, L.returns, L.idx, L.batch, L.ent, L.vf, D.n_choices, (const double*)L.adv_part,
                       (const float*)L.pack, L.part);
    PolGrad pg_sink = L.pg;
    pg_sink.p[8] = D.sink;
    pg_sink.p[9] = D.sink + 64 * A;
    hipLaunchKernelGGL((a2cd_finish_kernel<OB, A>), dim3(nfin, L.stats ? 3 : 2), dim3(256), 0, s, (const float*)L.part,
                       L.nwg, L.batch, D.n_choices, L.ent, L.vf, L.ps, L.pg, pg_sink, L.stats, L.normw,
                       (const float*)L.a.step[0]);
    if (L.optimizer == RR_A2C_ADAM)
        hipLaunchKernelGGL((a2cd_adam_kernel<OB, A>), dim3(L.nbp), dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw,
                           2 * nfin, L.max_norm, L.lr, L.beta1, L.beta2, L.w1, L.w2, L.eps, L.pack, L.nbp);
    else
        hipLaunchKernelGGL(a2cd_rmsprop_kernel, dim3(L.nbp), dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw,
                           2 * nfin, L.max_norm, L.lr, L.alpha, L.w1, L.eps, L.optimizer == RR_A2C_RMSPROP_TF ? 1 : 0);
    return (int)hipGetLastError();
}

}  // namespace

// rr_a2c_update_discrete's launches (declared in rocket_device.h); `launch` points to the A2cDiscreteLaunch
// of the calling TU, which validated the arguments and carved the workspace.
extern "C" int rrc_launch_a2c_discrete(const void* launch, void* stream)
{
    const auto D = from_unit<A2cDiscreteLaunch>(launch);
    hipStream_t s = (hipStream_t)stream;
    return D.base.normalize ? a2cd_launch<true>(D, s) : a2cd_launch<false>(D, s);
}
