// rocket_rollout_discrete.hip — the eleventh translation unit of librocket_hip.so: the one-launch
// collect and the one-launch evaluation of the Categorical policy (the reference's DiscreteActions3DOF:
// Discrete(K) over a table of [gimbal, thrust] rows, K = 2 .. 4).
//   rollout_discrete_kernel<INTEG, MULTI>   rollout_step_kernel<3, INTEG, 0, MULTI, 2>'s body
//              (rocket_rollout_body.inc) with RR_DISCRETE_HEAD: the pi tower's four heads are logits,
//              the sample region is discrete_act_kernel's (discrete/rocket_discrete.hip: softmax over the
//              first K logits, one uniform draw from the same key, the inverse-CDF index, the table row by
//              compares) and buf_act holds the index, one float per sample. MULTI = true is
//              rr_rollout_collect_discrete (T steps, V(last obs) and the GAE scan in one launch), false
//              rr_rollout_step_discrete (one step per launch).
//   eval_discrete_kernel<INTEG>             eval_kernel<3, INTEG, 0>'s body (rocket_eval_body.inc) with
//              RR_DISCRETE_HEAD: the action is the table row of the largest of the first K logits, the
//              lowest index on a tie (rr_policy_evaluate_discrete).
// Fixed here: the 3DOF env (7 observations), fp32 towers, the image pol::Layout<7, 4, 0> of
// rr_policy_pack_discrete (heads >= K are zeros and stay out of the softmax and the argmax). The
// integrator is a template arm, picked by dispatch_env's integrator half. K and the table travel by
// value in the kernel arguments. Launched through rrc_launch_rollout_discrete / rrc_launch_eval_discrete
// with the launch record of rrc_launch_collect / rrc_launch_eval (rocket_device.h: EnvLaunch) and a
// DiscHead. Compiled with the collect translation unit's settings (build.py COLLECT_FLAGS,
// RR_POL_PREFETCH_A 1), because both loops are the collect's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
// layer-2 A fragments read a group ahead, as in rocket_collect.hip (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "rocket_eval.inc"

namespace {

// the choices' [gimbal, thrust] rows (discrete_act_kernel's argument of the same name and layout)
struct DiscTable {
    float v[4][2];
};

#define RR_DISCRETE_HEAD

template <int INTEG, bool MULTI>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void rollout_discrete_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const RolloutIO io,
    int n_choices, const DiscTable tab)
{
    constexpr int MODEL = 3, PREC = 0, NTW = 2;
#define RR_COLLECT_STATS 0
#include "rocket_rollout_body.inc"
#undef RR_COLLECT_STATS
}

template <int INTEG>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void eval_discrete_kernel(float* __restrict__ state,
                                                                                uint32_t n_envs, uint32_t mode,
                                                                                const KParams P, const Bufs B,
                                                                                const EvalIO io, int n_choices,
                                                                                const DiscTable tab)
{
    constexpr int MODEL = 3, PREC = 0;
#define RR_EVAL_TRACE 0
#include "rocket_eval_body.inc"
#undef RR_EVAL_TRACE
}

#undef RR_DISCRETE_HEAD

DiscTable table_of(const DiscHead& h)
{
    DiscTable tab;
    std::memcpy(tab.v, h.table, sizeof(tab.v));
    return tab;
}

}  // namespace

// rr_rollout_collect_discrete's (multi != 0) and rr_rollout_step_discrete's launch (declared in
// rocket_device.h): rollout_discrete_kernel<INTEG, MULTI> on rr_rollout_collect's grid and workgroup.
// launch / io / head point to the EnvLaunch / RolloutIO / DiscHead of the calling TU, which checked
// that the handle is a 3DOF one with an RK4 / Euler integrator.
extern "C" int rrc_launch_rollout_discrete(const void* launch, const void* io, const void* head, int multi)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<RolloutIO>(io);
    const auto h = from_unit<DiscHead>(head);
    const DiscTable tab = table_of(h);
    dispatch_env(RR_MODEL_3DOF, L.integ, [&](auto, auto i) {
        dispatch_flag(multi != 0, [&](auto mt) {
            hipLaunchKernelGGL((rollout_discrete_kernel<decltype(i)::value, decltype(mt)::value>), dim3(L.grid),
                               dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o,
                               h.n_choices, tab);
        });
    });
    return (int)hipGetLastError();
}

// rr_policy_evaluate_discrete's launch (declared in rocket_device.h): eval_discrete_kernel<INTEG>, the
// collect's grid and workgroup. launch / io / head point to the EnvLaunch / EvalIO / DiscHead of the
// calling TU.
extern "C" int rrc_launch_eval_discrete(const void* launch, const void* io, const void* head)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    const auto h = from_unit<DiscHead>(head);
    const DiscTable tab = table_of(h);
    dispatch_env(RR_MODEL_3DOF, L.integ, [&](auto, auto i) {
        hipLaunchKernelGGL((eval_discrete_kernel<decltype(i)::value>), dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0,
                           (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o, h.n_choices, tab);
    });
    return (int)hipGetLastError();
}
