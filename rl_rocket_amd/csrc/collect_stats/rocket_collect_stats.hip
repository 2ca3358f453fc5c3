// rocket_collect_stats.hip — the sixth translation unit of librocket_hip.so: the rollout collect
// that also accounts for the episodes it finishes (rollout_collect_stats_kernel and
// rollout_stats_reduce_kernel, rocket_collect_stats.inc: rr_rollout_collect_stats), launched through
// rrc_launch_collect_stats with the launch record of rrc_launch_collect (rocket_device.h: EnvLaunch)
// and the same dispatcher. Compiled with the collect translation unit's settings (build.py
// COLLECT_FLAGS, RR_POL_PREFETCH_A 1), because its loop is the collect's: both kernels include
// rocket_rollout_body.inc.
//
// Sharing the body's text does not make one module of the two: this stays a translation unit of its
// own so that the kernels which existed before it keep their machine code (see
// eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
// layer-2 A fragments read a group ahead, as in rocket_collect.hip (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "rocket_collect_stats.inc"

// rr_rollout_collect_stats's two launches (declared in rocket_device.h): the collect,
// rollout_collect_stats_kernel<MODEL, INTEG, PREC> on rr_rollout_collect's grid and workgroup, picked
// by dispatch_env_prec, then the one-workgroup reduction of the waves' rows on the same stream.
// launch / io / stats point to the EnvLaunch / RolloutIO / CollectStatsIO of the calling TU.
extern "C" int rrc_launch_collect_stats(const void* launch, const void* io, const void* stats)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<RolloutIO>(io);
    const auto s = from_unit<CollectStatsIO>(stats);
    dispatch_env_prec(L.model, L.integ, L.prec, [&](auto m, auto i, auto pr) {
        hipLaunchKernelGGL((rollout_collect_stats_kernel<decltype(m)::value, decltype(i)::value, decltype(pr)::value>),
                           dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream, L.state, L.n, L.mode,
                           p, b, o, s);
    });
    hipLaunchKernelGGL(rollout_stats_reduce_kernel, dim3(1), dim3(kRedThreads), 0, (hipStream_t)L.stream, s);
    return (int)hipGetLastError();
}
