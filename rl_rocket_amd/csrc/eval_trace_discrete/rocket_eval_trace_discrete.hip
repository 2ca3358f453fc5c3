// rocket_eval_trace_discrete.hip — the fourteenth translation unit of librocket_hip.so: the Categorical
// policy's one-launch evaluation that records whole episodes of chosen envs
// (rr_policy_evaluate_discrete_trace).
//   eval_discrete_trace_kernel<INTEG>   rocket_eval_body.inc with both of its regions: RR_DISCRETE_HEAD
//              (eval_discrete_kernel's argmax of the first K logits, the lowest index on a tie, and the table
//              row) and RR_EVAL_TRACE 1 (eval_trace_kernel's five recording regions), plus the one region
//              only this kernel sees: the head keeps the winner's index and the step's record stores it in
//              the choice plane beside the action row. The recorded action row is the table row the env
//              stepped with.
// EvalTraceIO travels as in eval_trace_kernel and sits right after EvalIO in the argument list, because
// trace_args() (rocket_eval.inc) reads it from the kernel-argument segment at that offset; K, the table
// and the choice pointer follow it.
// Fixed here, as in rollout_discrete/rocket_rollout_discrete.hip: the 3DOF env, fp32 towers, the image
// pol::Layout<7, 4, 0>. Launched through rrc_launch_eval_discrete_trace with the launch record of
// rrc_launch_eval (rocket_device.h: EnvLaunch), a DiscHead, an EvalTraceIO and the choice pointer.
// Compiled with the collect translation unit's settings (build.py COLLECT_FLAGS, RR_POL_PREFETCH_A 1).
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

template <int INTEG>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void eval_discrete_trace_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const EvalIO io,
    const EvalTraceIO tr0, int n_choices, const DiscTable tab, int32_t* __restrict__ choice)
{
    constexpr int MODEL = 3, PREC = 0;
#define RR_EVAL_TRACE 1
#include "rocket_eval_body.inc"
#undef RR_EVAL_TRACE
}

#undef RR_DISCRETE_HEAD

}  // namespace

// rr_policy_evaluate_discrete_trace's launch (declared in rocket_device.h): eval_discrete_trace_kernel<INTEG>,
// the collect's grid and workgroup. launch / io / head / trace point to the EnvLaunch / EvalIO / DiscHead /
// EvalTraceIO of the calling TU, which checked that the handle is a 3DOF one with an RK4 / Euler
// integrator; choice is the device plane [n_slots][n_episodes][steps] or nullptr.
extern "C" int rrc_launch_eval_discrete_trace(const void* launch, const void* io, const void* head, const void* trace,
                                              void* choice)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    const auto h = from_unit<DiscHead>(head);
    const auto t = from_unit<EvalTraceIO>(trace);
    DiscTable tab;
    std::memcpy(tab.v, h.table, sizeof(tab.v));
    dispatch_env(RR_MODEL_3DOF, L.integ, [&](auto, auto i) {
        hipLaunchKernelGGL((eval_discrete_trace_kernel<decltype(i)::value>), dim3(L.grid),
                           dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o, t,
                           h.n_choices, tab, (int32_t*)choice);
    });
    return (int)hipGetLastError();
}
