// rocket_ppo_discrete_opts.hip — the twelfth translation unit of librocket_hip.so: the Categorical
// policy's PPO learner with the options of SB3's PPO.__init__ that rr_ppo_update_discrete fixes
// (rr_ppo_update_discrete_opts): clip_range_vf, normalize_advantage=False, target_kl, and the control
// block that carries the KL stop and the train() call's running statistics on the device. The four
// launches are rr_ppo_update_discrete's (discrete/rocket_discrete.hip), composed as
// ppo_opts/rocket_ppo_opts.hip composes rr_ppo_update's:
//   prep       discrete_prep_kernel's body (the advantage sums, the packing with zeros for heads >= K)
//              behind the stop check;
//   gradient   ppo_grad_tower<7, 4, 0, false, NORM, LOSS 2> (the softmax head) and
//              ppo_grad_tower<7, 4, 1, VCLIP, true> (the value clip touches the vf tower only);
//   finish     rocket_ppo_finish_body.inc as discrete_finish_kernel includes it (CTL false for the
//              body: its control lines read the Gaussian entropy), the five statistics, and then the
//              body's control-block lines in the kernel's own tail, from the statistics just written;
//   optimizer  ppo_opts_adam_kernel's frame around rocket_ppo_adam_body.inc over the 12 tensors.
// Every kernel first reads the control block's stop word: a stopped epoch's graph replay costs its
// launches only. Launched through rrc_launch_discrete_opts with a DiscreteOptsLaunch. Compiled with
// the collect translation unit's settings (build.py COLLECT_FLAGS): the gradient kernel's loop is the
// learner's.
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
__global__ __launch_bounds__(256) void dopts_prep_kernel(const float* __restrict__ ctl, const float* __restrict__ adv,
                                                         const int64_t* __restrict__ idx, int64_t bs,
                                                         double* __restrict__ part, PolSrc src, int n_choices,
                                                         float* __restrict__ pack)
{
    using K = ppo::Pack<OBS, ACT>;
    if (ctl_set(ctl, ppo::kStop)) return;
    if (blockIdx.x >= ppo::kAdvPart) {
        const int k = (blockIdx.x - ppo::kAdvPart) * 256 + threadIdx.x;
        if (k < 2 * K::SIZE) pack[k] = discrete_pack_value<OBS, ACT>(src, n_choices, k / K::SIZE, k % K::SIZE);
        return;
    }
    ppo_prep_body<OBS, ACT>(adv, idx, bs, part, src, pack);  // the advantage sums: these blocks pack nothing
}

template <int OBS, int ACT, bool VCLIP, bool NORM>
__global__ __launch_bounds__(ppo::kThreads) void dopts_grad_kernel(
    const float* __restrict__ ctl, const float* __restrict__ obs, const float* __restrict__ act,
    const float* __restrict__ old_lp, const float* __restrict__ adv, const float* __restrict__ ret,
    const int64_t* __restrict__ idx, int64_t bs, float clip, float ent_coef, float vf_coef, int n_choices,
    const double* __restrict__ adv_part, const float* __restrict__ pack, float* __restrict__ part,
    const float* __restrict__ old_val, float clip_vf)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
    if (ctl_set(ctl, ppo::kStop)) return;
    // the value clip touches the vf tower only, the advantages the pi tower only
    if (blockIdx.y == 0)
        ppo_grad_tower<OBS, ACT, 0, false, NORM, 2>(lds, obs, act, old_lp, adv, ret, idx, bs, clip, vf_coef, adv_part,
                                                    pack, part, nullptr, 0.0f, n_choices, ent_coef);
    else
        ppo_grad_tower<OBS, ACT, 1, VCLIP, true>(lds, obs, act, old_lp, adv, ret, idx, bs, clip, vf_coef, adv_part, pack,
                                                 part, old_val, clip_vf);
}

// grid (nfin, 2). discrete_finish_kernel with the control block: the body runs with CTL false (its
// control lines take the entropy from log_std), and the tail below repeats them on this kernel's
// statistics. stats_out is never null here (the caller's, or eight floats of the workspace).
template <int OBS, int ACT>
__global__ __launch_bounds__(256) void dopts_finish_kernel(ppo::CtlArgs cb, const float* __restrict__ part, int nwg,
                                                           int64_t bs, int n_choices, PolSrc src, PolGrad dst_in,
                                                           PolGrad dst_sink, float* __restrict__ stats_out,
                                                           float* __restrict__ normw,
                                                           const float* __restrict__ step0)
{
    if (ctl_set(cb.ctl, ppo::kStop)) return;
    // (the sink, the entropy lines: see discrete_finish_kernel)
    using P = ppo::Part<OBS, ACT>;
    const int el = blockIdx.x * kFinElems + threadIdx.x % kFinElems;
    const bool spare = blockIdx.y == 0 && ((el >= P::HW + 64 * n_choices && el < P::HB) ||
                                           (el >= P::HB + n_choices && el < P::LS));
    const PolGrad& dst = spare ? dst_sink : dst_in;
    constexpr float ent_coef = 0.0f;
    float* const stats = nullptr;
    constexpr bool CTL = false;
    const ppo::CtlArgs ca = {};
#include "rocket_ppo_finish_body.inc"
    if (e >= PT::ST && e < PT::SIZE) {
        const int k = e - PT::ST;
        const float inv_b = 1.0f / (float)bs;
        const float f = v * inv_b;
        float* c = cb.ctl;
        // one thread per statistic: it writes the figure and adds it to the block's sum (one writer
        // per word per launch, as in the body's CTL lines)
        if (tw == 0) {
            if (k == 0) {
                stats_out[0] = f;  // policy_loss
                if (c) c[ppo::kSumPg] += f;
            }
            if (k == 1) {
                stats_out[3] = f;  // clip_fraction
                if (c) c[ppo::kSumClip] += f;
            }
            if (k == 2) {
                stats_out[4] = f;  // approx_kl
                if (c) {
                    c[ppo::kKlSum] = cb.epoch_start ? f : c[ppo::kKlSum] + f;
                    c[ppo::kKlCount] = cb.epoch_start ? 1.0f : c[ppo::kKlCount] + 1.0f;
                    c[ppo::kKlLast] = f;
                    c[ppo::kEvals] += 1.0f;
                    if (cb.epoch_start) c[ppo::kEpochs] += 1.0f;
                    c[ppo::kDecide] = f > cb.kl_limit ? 1.0f : 0.0f;
                }
            }
            if (k == 3) {
                stats_out[2] = f;  // entropy: the mean of H
                if (c) c[ppo::kSumEnt] += f;
            }
        } else if (k == 0) {
            stats_out[1] = f;  // value_loss
            if (c) c[ppo::kSumVf] += f;
        }
    }
}

// The optimizer launch obeys the finish launch's decision (ppo_opts_adam_kernel's frame): with
// kDecide set nothing is stepped, repacked or summed, and block 0 commits the stop. It also returns
// at a stop word that stands without the decision, so that kStop alone makes the whole call a no-op.
template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void dopts_adam_kernel(float* __restrict__ ctl, AdamList A,
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
    // a stop word the caller set by hand (kDecide clear, so no block of this launch writes kStop)
    if (ctl_set(ctl, ppo::kStop)) return;
    // the step is counted ahead of the body, which a block past nbp leaves by a return
    if (ctl && blockIdx.x == 0 && threadIdx.x == 0) ctl[ppo::kSteps] += 1.0f;
#include "rocket_ppo_adam_body.inc"
}

}  // namespace

// rr_ppo_update_discrete_opts's launches (declared in rocket_device.h); `launch` points to the
// DiscreteOptsLaunch of the calling TU, which validated the arguments and carved the workspace.
extern "C" int rrc_launch_discrete_opts(const void* launch, void* stream)
{
    const auto O = from_unit<DiscreteOptsLaunch>(launch);
    const DiscreteLaunch& D = O.base;
    const PpoLaunch& L = D.u;
    hipStream_t s = (hipStream_t)stream;
    const float* ctl = O.ctl.ctl;
    constexpr int OB = 7, A = 4;
    using PT = ppo::Part<OB, A>;
    using K = ppo::Pack<OB, A>;
    constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
    auto run = [&](auto vclip_c, auto norm_c) {
        constexpr bool VC = decltype(vclip_c)::value != 0, NM = decltype(norm_c)::value != 0;
        if (!(L.flags & RR_PPO_CHAINED))
            hipLaunchKernelGGL((dopts_prep_kernel<OB, A>), dim3(ppo::kAdvPart + (2 * K::SIZE + 255) / 256), dim3(256), 0,
                               s, ctl, L.advantages, L.idx, L.batch, L.adv_part, L.ps, D.n_choices, L.pack);
        hipLaunchKernelGGL((dopts_grad_kernel<OB, A, VC, NM>), dim3(L.nwg, 2), dim3(ppo::kThreads), 0, s, ctl, L.obs,
                           L.actions, L.old_log_prob, L.advantages, L.returns, L.idx, L.batch, L.clip, L.ent, L.vf,
                           D.n_choices, (const double*)L.adv_part, (const float*)L.pack, L.part, O.old_values,
                           O.clip_vf);
        PolGrad pg_sink = L.pg;
        pg_sink.p[8] = D.sink;
        pg_sink.p[9] = D.sink + 64 * A;
        hipLaunchKernelGGL((dopts_finish_kernel<OB, A>), dim3(nfin, 2), dim3(256), 0, s, O.ctl, (const float*)L.part,
                           L.nwg, L.batch, D.n_choices, L.ps, L.pg, pg_sink, L.stats, L.normw,
                           (const float*)L.a.step[0]);
        const AdvNext nx = {L.advantages, L.next_idx, L.next_idx ? L.next_batch : 0, L.adv_part};
        hipLaunchKernelGGL((dopts_adam_kernel<OB, A>), dim3(L.nbp + (L.next_idx ? ppo::kAdvPart / 4 : 0)),
                           dim3(kAdamThreads), 0, s, O.ctl.ctl, L.a, (const float*)L.normw, 2 * nfin, L.max_norm, L.lr,
                           L.beta1, L.beta2, L.w1, L.w2, L.eps, L.pack, nx, L.nbp);
    };
    const bool vc = O.clip_vf > 0.0f;
    if (vc && O.normalize) run(tag<1>{}, tag<1>{});
    else if (vc) run(tag<1>{}, tag<0>{});
    else if (O.normalize) run(tag<0>{}, tag<1>{});
    else run(tag<0>{}, tag<0>{});
    return (int)hipGetLastError();
}
