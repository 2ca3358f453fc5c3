// rocket_eval_sampled_discrete.hip — the eighteenth translation unit of librocket_hip.so: the Categorical
// policy's one-launch evaluation under its SAMPLED action (rr_policy_evaluate_discrete_sampled).
//   eval_discrete_sampled_kernel<INTEG>         eval_discrete_kernel's body (rocket_eval_body.inc with
//              RR_DISCRETE_HEAD) with RR_EVAL_SAMPLE: the action of step k is rollout_discrete_kernel's sample
//              of step t = k (softmax over the first K logits, one uniform draw from the same key, the
//              inverse-CDF index, the table row by compares), where eval_discrete_kernel takes the argmax.
//   eval_discrete_sampled_trace_kernel<INTEG>   the same with the recording regions (RR_EVAL_TRACE 1) and the
//              choice plane of eval_discrete_trace_kernel, which here receives the sampled index.
// The seed words and the iter pointer follow every argument of the deterministic kernels, so EvalTraceIO stays
// right after EvalIO, where trace_args() (rocket_eval.inc) reads it from the kernel-argument segment.
// Fixed here, as in rollout_discrete/rocket_rollout_discrete.hip: the 3DOF env, fp32 towers, the image
// pol::Layout<7, 4, 0>. Launched through rrc_launch_eval_discrete_sampled with the launch record of
// rrc_launch_eval (rocket_device.h: EnvLaunch), a DiscHead, an EvalSample and, recording, an EvalTraceIO and
// the choice pointer. Compiled with the collect translation unit's settings (build.py COLLECT_FLAGS,
// RR_POL_PREFETCH_A 1).
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

// the choices' [gimbal, thrust] rows (eval_discrete_kernel's argument of the same name and layout)
struct DiscTable {
    float v[4][2];
};

#define RR_DISCRETE_HEAD
#define RR_EVAL_SAMPLE

template <int INTEG>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void eval_discrete_sampled_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const EvalIO io,
    int n_choices, const DiscTable tab, uint32_t seed_lo, uint32_t seed_hi, const uint64_t* __restrict__ iter)
{
    constexpr int MODEL = 3, PREC = 0;
#define RR_EVAL_TRACE 0
#include "rocket_eval_body.inc"
#undef RR_EVAL_TRACE
}

template <int INTEG>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void eval_discrete_sampled_trace_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const EvalIO io,
    const EvalTraceIO tr0, int n_choices, const DiscTable tab, int32_t* __restrict__ choice, uint32_t seed_lo,
    uint32_t seed_hi, const uint64_t* __restrict__ iter)
{
    constexpr int MODEL = 3, PREC = 0;
#define RR_EVAL_TRACE 1
#include "rocket_eval_body.inc"
#undef RR_EVAL_TRACE
}

#undef RR_EVAL_SAMPLE
#undef RR_DISCRETE_HEAD

}  // namespace

// rr_policy_evaluate_discrete_sampled's launch (declared in rocket_device.h): eval_discrete_sampled_kernel<INTEG>
// or, with trace != nullptr, eval_discrete_sampled_trace_kernel, the collect's grid and workgroup. launch / io /
// head / sample / trace point to the EnvLaunch / EvalIO / DiscHead / EvalSample / EvalTraceIO of the calling TU,
// which checked that the handle is a 3DOF one with an RK4 / Euler integrator; choice is the device plane
// [n_slots][n_episodes][steps] or nullptr.
extern "C" int rrc_launch_eval_discrete_sampled(const void* launch, const void* io, const void* head,
                                                const void* sample, const void* trace, void* choice)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    const auto h = from_unit<DiscHead>(head);
    const auto s = from_unit<EvalSample>(sample);
    DiscTable tab;
    std::memcpy(tab.v, h.table, sizeof(tab.v));
    dispatch_env(RR_MODEL_3DOF, L.integ, [&](auto, auto i) {
        constexpr int I = decltype(i)::value;
        if (trace) {
            const auto t = from_unit<EvalTraceIO>(trace);
            hipLaunchKernelGGL((eval_discrete_sampled_trace_kernel<I>), dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0,
                               (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o, t, h.n_choices, tab,
                               (int32_t*)choice, s.seed_lo, s.seed_hi, s.iter);
        } else {
            hipLaunchKernelGGL((eval_discrete_sampled_kernel<I>), dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0,
                               (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o, h.n_choices, tab, s.seed_lo,
                               s.seed_hi, s.iter);
        }
    });
    return (int)hipGetLastError();
}
