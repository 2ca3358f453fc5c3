// rocket_eval_sampled.hip — the seventeenth translation unit of librocket_hip.so: the one-launch evaluation
// under the policy's SAMPLED action (rr_policy_evaluate_sampled; SB3 evaluate_policy(deterministic=False)).
//   eval_sampled_kernel<MODEL, INTEG, PREC>         eval_kernel's body (rocket_eval_body.inc, RR_EVAL_TRACE 0)
//              with RR_EVAL_SAMPLE: the action of step k is rollout_step_kernel's sample of step t = k (the key
//              from the seed words, the env's global id, *iter and t; Box-Muller on pol::normal2;
//              mean + exp(log_std) * eps, clipped), where eval_kernel takes the clipped mean.
//   eval_sampled_trace_kernel<MODEL, INTEG, PREC>   the same with eval_trace_kernel's five recording regions
//              (RR_EVAL_TRACE 1); the recorded action row is the clipped sample the env stepped with.
// The seed words and the iter pointer follow every argument of the deterministic kernels, so EvalTraceIO stays
// right after EvalIO, where trace_args() (rocket_eval.inc) reads it from the kernel-argument segment.
// Launched through rrc_launch_eval_sampled with the launch record of rrc_launch_eval (rocket_device.h:
// EnvLaunch), an EvalSample and, recording, an EvalTraceIO. Compiled with the collect translation unit's
// settings (build.py COLLECT_FLAGS, RR_POL_PREFETCH_A 1), because its loop is the collect's and eval_kernel's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their machine
// code (see eval_trace/rocket_eval_trace.hip), and so that it can be taken out whole.
#include "rocket_device.h"
// layer-2 A fragments read a group ahead, as in rocket_collect.hip (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "rocket_eval.inc"

namespace {

#define RR_EVAL_SAMPLE

// waves per SIMD the register allocation aims at: the 6DOF instantiations that do not fit two waves' 256
// registers (--resource-usage; DESIGN.md, "Sampled evaluation") are given one, as the exact kernels are
constexpr int sampled_waves(int model, int integ, int prec, bool trace)
{
    return model == 6 && (prec != 0 || (integ == RR_INT_RK4 && trace)) ? 1 : 2;
}

template <int MODEL, int INTEG, int PREC>
__global__ __launch_bounds__(rol::Shape<2>::kThreads)
__attribute__((amdgpu_waves_per_eu(sampled_waves(MODEL, INTEG, PREC, false)))) void eval_sampled_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const EvalIO io,
    uint32_t seed_lo, uint32_t seed_hi, const uint64_t* __restrict__ iter)
{
#define RR_EVAL_TRACE 0
#include "rocket_eval_body.inc"
#undef RR_EVAL_TRACE
}

template <int MODEL, int INTEG, int PREC>
__global__ __launch_bounds__(rol::Shape<2>::kThreads)
__attribute__((amdgpu_waves_per_eu(sampled_waves(MODEL, INTEG, PREC, true)))) void eval_sampled_trace_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const EvalIO io,
    const EvalTraceIO tr0, uint32_t seed_lo, uint32_t seed_hi, const uint64_t* __restrict__ iter)
{
#define RR_EVAL_TRACE 1
#include "rocket_eval_body.inc"
#undef RR_EVAL_TRACE
}

#undef RR_EVAL_SAMPLE

}  // namespace

// rr_policy_evaluate_sampled's launch (declared in rocket_device.h): eval_sampled_kernel<MODEL, INTEG, PREC> or,
// with trace != nullptr, eval_sampled_trace_kernel, eval_kernel's grid and workgroup, picked by
// dispatch_env_prec. launch / io / sample / trace point to the EnvLaunch / EvalIO / EvalSample / EvalTraceIO
// of the calling TU.
extern "C" int rrc_launch_eval_sampled(const void* launch, const void* io, const void* sample, const void* trace)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    const auto s = from_unit<EvalSample>(sample);
    dispatch_env_prec(L.model, L.integ, L.prec, [&](auto m, auto i, auto pr) {
        constexpr int M = decltype(m)::value, I = decltype(i)::value, PR = decltype(pr)::value;
        if (trace) {
            const auto t = from_unit<EvalTraceIO>(trace);
            hipLaunchKernelGGL((eval_sampled_trace_kernel<M, I, PR>), dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0,
                               (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o, t, s.seed_lo, s.seed_hi, s.iter);
        } else {
            hipLaunchKernelGGL((eval_sampled_kernel<M, I, PR>), dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0,
                               (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o, s.seed_lo, s.seed_hi, s.iter);
        }
    });
    return (int)hipGetLastError();
}
