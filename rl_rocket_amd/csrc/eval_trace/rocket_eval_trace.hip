// rocket_eval_trace.hip — the fourth translation unit of librocket_hip.so: the recording
// evaluation kernels (eval_trace_kernel, rocket_eval.inc: rr_policy_evaluate_trace, the loop of
// eval_kernel that also writes the histories of the envs with a trace slot), launched through
// rrc_launch_eval_trace. Compiled with the collect translation unit's settings (build.py
// COLLECT_FLAGS, RR_POL_PREFETCH_A 1), because its loop is the collect's and eval_kernel's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (tools/isa_diff.py): instantiated next to eval_kernel in rocket_collect.hip, the
// recording kernels changed how eight eval_kernel instantiations address LDS (the same addresses,
// split differently between register and immediate offset) although not one line of eval_kernel's
// source had changed. Which form the backend picks depends on what else the module holds; a module
// of their own takes the recording kernels out of that.
#include <cstring>
#include <type_traits>

#include "rocket_device.h"
// layer-2 A fragments read a group ahead, as in rocket_collect.hip (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "rocket_eval.inc"

// rr_policy_evaluate_trace's launch (declared in rocket_device.h): eval_trace_kernel<MODEL, INTEG,
// PREC>, eval_kernel's grid and workgroup. io / trace point to the EvalIO / EvalTraceIO of the
// calling TU.
extern "C" int rrc_launch_eval_trace(int model, int integ, int prec, unsigned grid, float* state, uint32_t n,
                                     uint32_t mode, const void* kp, const void* bufs, const void* io,
                                     const void* trace, void* stream)
{
    KParams p;
    Bufs b;
    EvalIO o;
    EvalTraceIO t;
    std::memcpy(&p, kp, sizeof(KParams));
    std::memcpy(&b, bufs, sizeof(Bufs));
    std::memcpy(&o, io, sizeof(EvalIO));
    std::memcpy(&t, trace, sizeof(EvalTraceIO));
    hipStream_t s = (hipStream_t)stream;
#define RR_EVAL(M, I, PR)                                                                                    \
    hipLaunchKernelGGL((eval_trace_kernel<M, I, PR>), dim3(grid), dim3(rol::Shape<2>::kThreads), 0, s, state, n, \
                       mode, p, b, o, t)
#define RR_EVAL_P(M, I)                      \
    do {                                     \
        if (prec == 1) RR_EVAL(M, I, 1);     \
        else if (prec == 2) RR_EVAL(M, I, 2); \
        else RR_EVAL(M, I, 0);               \
    } while (0)
    const bool euler = integ == RR_INT_EULER;
    if (model == RR_MODEL_6DOF && !euler) RR_EVAL_P(6, RR_INT_RK4);
    else if (model == RR_MODEL_6DOF) RR_EVAL_P(6, RR_INT_EULER);
    else if (!euler) RR_EVAL_P(3, RR_INT_RK4);
    else RR_EVAL_P(3, RR_INT_EULER);
#undef RR_EVAL_P
#undef RR_EVAL
    return (int)hipGetLastError();
}
