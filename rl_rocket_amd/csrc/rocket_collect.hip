// rocket_collect.hip — the third translation unit of librocket_hip.so: the rollout collect kernels
// (rollout_step_kernel<..., MULTI = true>, rocket_rollout.inc: rr_rollout_collect, launched through
// rrc_launch_collect), the evaluation kernels (eval_kernel, rocket_eval.inc: rr_policy_evaluate, the
// collect's loop without its value tower, launched through rrc_launch_eval) and the PPO learner's
// kernels (rocket_ppo.inc: rr_ppo_grad / rr_ppo_update / rr_clip_adam, launched through
// rrc_launch_learner). Each entry point takes the caller's launch record (rocket_device.h:
// EnvLaunch, PpoLaunch) as bytes; the env kernels' instantiation is picked by dispatch_env_prec.
// They are compiled with their own code-generation setting (rl_rocket_amd/build.py COLLECT_FLAGS:
// -amdgpu-mfma-vgpr-form, the MFMA accumulators in VGPRs) without touching the other kernels. In the
// AGPR form every tanh input of the policy towers first crosses back with a v_accvgpr_read (384 in
// the collect loop); in the VGPR form the loop issues 12 % fewer VALU instructions and the collect
// measured 5.5 % faster (profiles/r04/ab_vf/). The gradient kernel
// moves 1 082 -> 343 registers between the files and its minibatch measured 3 % faster, bitwise
// (profiles/r06/ppo_vf/). The same flag on the whole main TU would cost the per-step fp16x3
// rollout kernels their second wave per SIMD.
#include "rocket_device.h"
// layer-2 A fragments read a group ahead in this translation unit (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "rocket_eval.inc"
#include "rocket_ppo.inc"

namespace {

// rr_clip_adam's two launches (rocket_ppo.inc, at AdamList): the learner's only non-template
// kernels, so they are defined in the translation unit that compiles them.
// work[b] = sum of g^2 over block b's elements; work[gridDim.x] = the new step count
__global__ __launch_bounds__(kAdamThreads) void adam_norm_kernel(AdamList A, float* __restrict__ work)
{
    __shared__ float red[kAdamThreads / kWave];
    const int64_t e = (int64_t)blockIdx.x * kAdamThreads + threadIdx.x;
    float g = 0.0f;
    if (e < A.start[A.n]) {
        const int t = adam_tensor_of(A, e);
        g = A.grad[t][e - A.start[t]];
    }
    const float tot = block_sum<kAdamThreads>(g * g, red);
    if (threadIdx.x == 0) {
        work[blockIdx.x] = tot;
        if (blockIdx.x == 0) work[gridDim.x] = *A.step[0] + 1.0f;
    }
}

__global__ __launch_bounds__(kAdamThreads) void adam_step_kernel(AdamList A, const float* __restrict__ work,
                                                                 float max_norm, const float* __restrict__ lr_p,
                                                                 float beta1, float beta2, float w1, float w2, float eps)
{
    __shared__ float red[kAdamThreads / kWave];
    const int nb = gridDim.x;
    float part = 0.0f;
    for (int b = threadIdx.x; b < nb; b += kAdamThreads) part += work[b];
    const float tot = block_sum<kAdamThreads>(part, red);
    const float step = work[nb], lr = *lr_p;
    const float coef = max_norm > 0.0f ? fminf(max_norm / (sqrtf(tot) + 1e-6f), 1.0f) : 1.0f;
    const float bc1 = 1.0f - powf(beta1, step), bc2 = 1.0f - powf(beta2, step);
    const float sneg = -(1.0f / (bc1 / lr));
    const float d = sqrtf(bc2) * sneg, eos = 1.0f / (sneg / eps);
    const int64_t e = (int64_t)blockIdx.x * kAdamThreads + threadIdx.x;
    if (e < A.start[A.n]) {
        const int t = adam_tensor_of(A, e);
        const int64_t k = e - A.start[t];
        float *p = A.param[t], *gp = A.grad[t], *m = A.exp_avg[t], *v = A.exp_avg_sq[t];
        const float g = gp[k] * coef;
        gp[k] = g;
        const float mk = m[k] + w1 * (g - m[k]);
        const float vk = v[k] * beta2 + (w2 * g) * g;
        m[k] = mk;
        v[k] = vk;
        p[k] = p[k] + mk / (sqrtf(vk) / d + eos);
    }
    if (blockIdx.x == 0 && threadIdx.x < A.n) *A.step[threadIdx.x] = step;
}

}  // namespace

// the collect's entry point (declared in rocket_device.h): one rr_rollout_collect launch,
// rollout_step_kernel<MODEL, INTEG, PREC, MULTI = true, 2>. launch / io point to the EnvLaunch /
// RolloutIO of the calling TU.
extern "C" int rrc_launch_collect(const void* launch, const void* io)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<RolloutIO>(io);
    dispatch_env_prec(L.model, L.integ, L.prec, [&](auto m, auto i, auto pr) {
        hipLaunchKernelGGL((rollout_step_kernel<decltype(m)::value, decltype(i)::value, decltype(pr)::value, true, 2>),
                           dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream, L.state, L.n, L.mode,
                           p, b, o);
    });
    return (int)hipGetLastError();
}

// rr_policy_evaluate's launch (declared in rocket_device.h): eval_kernel<MODEL, INTEG, PREC>, the
// collect's grid and workgroup. launch / io point to the EnvLaunch / EvalIO of the calling TU.
extern "C" int rrc_launch_eval(const void* launch, const void* io)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    dispatch_env_prec(L.model, L.integ, L.prec, [&](auto m, auto i, auto pr) {
        hipLaunchKernelGGL((eval_kernel<decltype(m)::value, decltype(i)::value, decltype(pr)::value>), dim3(L.grid),
                           dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o);
    });
    return (int)hipGetLastError();
}

// the learner's launches (declared in rocket_device.h), for rr_ppo_grad / rr_ppo_update /
// rr_clip_adam, which validated the arguments and carved the workspace into `launch` (a PpoLaunch of
// the calling TU). Compiled here with the MFMA accumulators in VGPRs: the gradient kernel's loop
// then moves ~740 fewer registers between AGPRs and VGPRs per launch, bitwise the same gradients
// (profiles/r06/ppo_vf/)
extern "C" int rrc_launch_learner(const void* launch, void* stream)
{
    const auto L = from_unit<PpoLaunch>(launch);
    hipStream_t s = (hipStream_t)stream;
    if (L.op == 2) {
        const dim3 grid((unsigned)((L.a.start[L.a.n] + kAdamThreads - 1) / kAdamThreads));
        hipLaunchKernelGGL(adam_norm_kernel, grid, dim3(kAdamThreads), 0, s, L.a, L.work);
        hipLaunchKernelGGL(adam_step_kernel, grid, dim3(kAdamThreads), 0, s, L.a, L.work, L.max_norm, L.lr, L.beta1,
                           L.beta2, L.w1, L.w2, L.eps);
        return (int)hipGetLastError();
    }
    const bool update = L.op == 1;
    auto run = [&](auto obs_c, auto act_c) {
        constexpr int O = decltype(obs_c)::value, A = decltype(act_c)::value;
        using PT = ppo::Part<O, A>;
        using K = ppo::Pack<O, A>;
        constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
        if (!(update && (L.flags & RR_PPO_CHAINED)))
            hipLaunchKernelGGL((ppo_prep_kernel<O, A>), dim3(ppo::kAdvPart + (2 * K::SIZE + 255) / 256), dim3(256), 0, s,
                               L.advantages, L.idx, L.batch, L.adv_part, L.ps, L.pack);
        hipLaunchKernelGGL((ppo_grad_kernel<O, A>), dim3(L.nwg, 2), dim3(ppo::kThreads), 0, s, L.obs, L.actions,
                           L.old_log_prob, L.advantages, L.returns, L.idx, L.batch, L.clip, L.vf, L.adv_part, L.pack,
                           L.part);
        hipLaunchKernelGGL((ppo_finish_kernel<O, A>), dim3(nfin, 2), dim3(256), 0, s, L.part, L.nwg, L.batch, L.ent,
                           L.ps, L.pg, L.stats, update ? L.normw : nullptr,
                           update ? (const float*)L.a.step[0] : nullptr);
        if (update) {
            const AdvNext nx = {L.advantages, L.next_idx, L.next_idx ? L.next_batch : 0, L.adv_part};
            hipLaunchKernelGGL((adam_chain_kernel<O, A>), dim3(L.nbp + (L.next_idx ? ppo::kAdvPart / 4 : 0)),
                               dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw, 2 * nfin, L.max_norm, L.lr,
                               L.beta1, L.beta2, L.w1, L.w2, L.eps, L.pack, nx, L.nbp);
        }
    };
    if (L.obs_dim == 14) run(tag<14>{}, tag<3>{});
    else run(tag<7>{}, tag<2>{});
    return (int)hipGetLastError();
}
