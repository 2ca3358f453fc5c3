// rocket_eval_trace.hip — the fourth translation unit of librocket_hip.so: the recording
// evaluation kernels (eval_trace_kernel, rocket_eval.inc: rr_policy_evaluate_trace, the body of
// eval_kernel, rocket_eval_body.inc, with the regions that write the histories of the envs with a
// trace slot), launched through
// rrc_launch_eval_trace with the launch record of rrc_launch_eval (rocket_device.h: EnvLaunch) and
// the same dispatcher. Compiled with the collect translation unit's settings (build.py
// COLLECT_FLAGS, RR_POL_PREFETCH_A 1), because its loop is the collect's and eval_kernel's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (tools/isa_diff.py): instantiated next to eval_kernel in rocket_collect.hip, the
// recording kernels changed how eight eval_kernel instantiations address LDS (the same addresses,
// split differently between register and immediate offset) although not one line of eval_kernel's
// source had changed. Which form the backend picks depends on what else the module holds; a module
// of their own takes the recording kernels out of that.
#include "rocket_device.h"
// layer-2 A fragments read a group ahead, as in rocket_collect.hip (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "rocket_eval.inc"

// rr_policy_evaluate_trace's launch (declared in rocket_device.h): eval_trace_kernel<MODEL, INTEG,
// PREC>, eval_kernel's grid and workgroup, picked by dispatch_env_prec. launch / io / trace point to
// the EnvLaunch / EvalIO / EvalTraceIO of the calling TU.
extern "C" int rrc_launch_eval_trace(const void* launch, const void* io, const void* trace)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    const auto t = from_unit<EvalTraceIO>(trace);
    dispatch_env_prec(L.model, L.integ, L.prec, [&](auto m, auto i, auto pr) {
        hipLaunchKernelGGL((eval_trace_kernel<decltype(m)::value, decltype(i)::value, decltype(pr)::value>),
                           dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream, L.state, L.n, L.mode,
                           p, b, o, t);
    });
    return (int)hipGetLastError();
}
