// rocket_ppo_opts.hip — the seventh translation unit of librocket_hip.so: the PPO learner with the
// options of SB3's PPO.__init__ that rr_ppo_update fixes (rr_ppo_update_opts): clip_range_vf,
// normalize_advantage=False, target_kl, and the control block that carries the KL stop and the
// train() call's running statistics on the device. The four launches are rr_ppo_update's
// (rocket_ppo.inc: packing / advantage sums, gradient, finish, clip + Adam + repack), their bodies
// (functions, or text included into both kernels) compiled here with the options on, in kernels
// that first read the control block's stop word: a stopped epoch's graph replay costs its launches
// only. Launched through
// rrc_launch_learner_opts with a PpoOptsLaunch. Compiled with the collect translation unit's
// settings (build.py COLLECT_FLAGS), because the gradient kernel's loop is the learner's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_ppo.inc"

namespace {

// Who reads and writes which word of the control block: ppo::Ctl (rocket_ppo.inc).
__device__ __forceinline__ bool ctl_set(const float* ctl, int slot) { return ctl && ctl[slot] != 0.0f; }

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void ppo_opts_prep_kernel(const float* __restrict__ ctl, const float* __restrict__ adv,
                                                            const int64_t* __restrict__ idx, int64_t bs,
                                                            double* __restrict__ part, PolSrc src,
                                                            float* __restrict__ pack)
{
    if (ctl_set(ctl, ppo::kStop)) return;
    ppo_prep_body<OBS, ACT>(adv, idx, bs, part, src, pack);
}

template <int OBS, int ACT, bool VCLIP, bool NORM>
__global__ __launch_bounds__(ppo::kThreads) void ppo_opts_grad_kernel(
    const float* __restrict__ ctl, const float* __restrict__ obs, const float* __restrict__ act,
    const float* __restrict__ old_lp, const float* __restrict__ adv, const float* __restrict__ ret,
    const int64_t* __restrict__ idx, int64_t bs, float clip, float vf_coef, const double* __restrict__ adv_part,
    const float* __restrict__ pack, float* __restrict__ part, const float* __restrict__ old_val, float clip_vf)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
    if (ctl_set(ctl, ppo::kStop)) return;
    // the value clip touches the vf tower only, the advantages the pi tower only
    if (blockIdx.y == 0)
        ppo_grad_tower<OBS, ACT, 0, false, NORM>(lds, obs, act, old_lp, adv, ret, idx, bs, clip, vf_coef, adv_part, pack,
                                                 part);
    else
        ppo_grad_tower<OBS, ACT, 1, VCLIP, true>(lds, obs, act, old_lp, adv, ret, idx, bs, clip, vf_coef, adv_part, pack,
                                                 part, old_val, clip_vf);
}

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void ppo_opts_finish_kernel(ppo::CtlArgs ca, const float* __restrict__ part, int nwg,
                                                              int64_t bs, float ent_coef, PolSrc src, PolGrad dst,
                                                              float* __restrict__ stats, float* __restrict__ normw,
                                                              const float* __restrict__ step0)
{
    if (ctl_set(ca.ctl, ppo::kStop)) return;
    constexpr bool CTL = true;
#include "rocket_ppo_finish_body.inc"
}

// The optimizer launch obeys the finish launch's decision: with kDecide set nothing is stepped,
// repacked or summed, and block 0 commits the stop for every later launch.
template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void ppo_opts_adam_kernel(float* __restrict__ ctl, AdamList A,
                                                                     const float* __restrict__ normw, int n_norm,
                                                                     float max_norm, const float* __restrict__ lr_p,
                                                                     float beta1, float beta2, float w1, float w2,
                                                                     float eps, float* __restrict__ pack, AdvNext nx,
                                                                     int nbp)
{
    if (ctl_set(ctl, ppo::kDecide)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) ctl[ppo::kStop] = 1.0f;
        return;
    }
    // the step is counted ahead of the body, which a block past nbp leaves by a return
    if (ctl && blockIdx.x == 0 && threadIdx.x == 0) ctl[ppo::kSteps] += 1.0f;
#include "rocket_ppo_adam_body.inc"
}

}  // namespace

// rr_ppo_update_opts's launches (declared in rocket_device.h); `launch` points to the PpoOptsLaunch
// of the calling TU, which validated the arguments and carved the workspace.
extern "C" int rrc_launch_learner_opts(const void* launch, void* stream)
{
    const auto O = from_unit<PpoOptsLaunch>(launch);
    const PpoLaunch& L = O.base;
    hipStream_t s = (hipStream_t)stream;
    const float* ctl = O.ctl.ctl;
    auto run = [&](auto obs_c, auto act_c, auto vclip_c, auto norm_c) {
        constexpr int OB = decltype(obs_c)::value, A = decltype(act_c)::value;
        constexpr bool VC = decltype(vclip_c)::value != 0, NM = decltype(norm_c)::value != 0;
        using PT = ppo::Part<OB, A>;
        using K = ppo::Pack<OB, A>;
        constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
        if (!(L.flags & RR_PPO_CHAINED))
            hipLaunchKernelGGL((ppo_opts_prep_kernel<OB, A>), dim3(ppo::kAdvPart + (2 * K::SIZE + 255) / 256), dim3(256),
                               0, s, ctl, L.advantages, L.idx, L.batch, L.adv_part, L.ps, L.pack);
        hipLaunchKernelGGL((ppo_opts_grad_kernel<OB, A, VC, NM>), dim3(L.nwg, 2), dim3(ppo::kThreads), 0, s, ctl, L.obs,
                           L.actions, L.old_log_prob, L.advantages, L.returns, L.idx, L.batch, L.clip, L.vf,
                           (const double*)L.adv_part, (const float*)L.pack, L.part, O.old_values, O.clip_vf);
        hipLaunchKernelGGL((ppo_opts_finish_kernel<OB, A>), dim3(nfin, 2), dim3(256), 0, s, O.ctl, (const float*)L.part,
                           L.nwg, L.batch, L.ent, L.ps, L.pg, L.stats, L.normw, (const float*)L.a.step[0]);
        const AdvNext nx = {L.advantages, L.next_idx, L.next_idx ? L.next_batch : 0, L.adv_part};
        hipLaunchKernelGGL((ppo_opts_adam_kernel<OB, A>), dim3(L.nbp + (L.next_idx ? ppo::kAdvPart / 4 : 0)),
                           dim3(kAdamThreads), 0, s, O.ctl.ctl, L.a, (const float*)L.normw, 2 * nfin, L.max_norm, L.lr,
                           L.beta1, L.beta2, L.w1, L.w2, L.eps, L.pack, nx, L.nbp);
    };
    auto pick = [&](auto obs_c, auto act_c) {
        const bool vc = O.clip_vf > 0.0f;
        if (vc && O.normalize) run(obs_c, act_c, tag<1>{}, tag<1>{});
        else if (vc) run(obs_c, act_c, tag<1>{}, tag<0>{});
        else if (O.normalize) run(obs_c, act_c, tag<0>{}, tag<1>{});
        else run(obs_c, act_c, tag<0>{}, tag<0>{});
    };
    if (L.obs_dim == 14) pick(tag<14>{}, tag<3>{});
    else pick(tag<7>{}, tag<2>{});
    return (int)hipGetLastError();
}
