// rocket_collect_stats_discrete.hip — the thirteenth translation unit of librocket_hip.so: the
// Categorical policy's one-launch collect that also accounts for the episodes it finishes
// (rr_rollout_collect_discrete_stats).
//   rollout_discrete_stats_kernel<INTEG>   rocket_rollout_body.inc with both of its independent regions:
//              RR_DISCRETE_HEAD (rollout_discrete_kernel<INTEG, true>'s softmax head, one uniform draw,
//              the table row; buf_act holds the index) and RR_COLLECT_STATS 1
//              (rollout_collect_stats_kernel's accounting: the lanes' LDS columns, the finished episode
//              inside the done branch, the sample sums of the GAE scan, the wave's butterfly and its row
//              of partials). The body's text is unchanged: the two regions never touch the same lines.
//   rollout_stats_reduce_kernel            this unit's copy of the one-workgroup reduction
//              (collect_stats/rocket_collect_stats.inc, included for it and for namespace rst), launched
//              right after on the same stream.
// Fixed here, as in rollout_discrete/rocket_rollout_discrete.hip: the 3DOF env, fp32 towers, the image
// pol::Layout<7, 4, 0>, MULTI and NTW 2. Launched through rrc_launch_collect_discrete_stats with the launch
// record of rrc_launch_collect (rocket_device.h: EnvLaunch), a DiscHead and a CollectStatsIO. Compiled
// with the collect translation unit's settings (build.py COLLECT_FLAGS, RR_POL_PREFETCH_A 1).
//
// It is a translation unit of its own so that the kernels which existed before it keep their machine
// code (see eval_trace/rocket_eval_trace.hip), and so that it can be taken out whole.
#include "rocket_device.h"
// layer-2 A fragments read a group ahead, as in rocket_collect.hip (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "collect_stats/rocket_collect_stats.inc"

namespace {

// the choices' [gimbal, thrust] rows (rollout_discrete_kernel's argument of the same name and layout)
struct DiscTable {
    float v[4][2];
};

#define RR_DISCRETE_HEAD

template <int INTEG>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void rollout_discrete_stats_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const RolloutIO io,
    int n_choices, const DiscTable tab, const CollectStatsIO sio)
{
    constexpr int MODEL = 3, PREC = 0, NTW = 2;
    constexpr bool MULTI = true;
#define RR_COLLECT_STATS 1
#include "rocket_rollout_body.inc"
#undef RR_COLLECT_STATS
}

#undef RR_DISCRETE_HEAD

}  // namespace

// rr_rollout_collect_discrete_stats's two launches (declared in rocket_device.h):
// rollout_discrete_stats_kernel<INTEG> on rr_rollout_collect's grid and workgroup, then the
// one-workgroup reduction of the waves' rows on the same stream. launch / io / head / stats point to the
// EnvLaunch / RolloutIO / DiscHead / CollectStatsIO of the calling TU, which checked that the handle is a
// 3DOF one with an RK4 / Euler integrator.
extern "C" int rrc_launch_collect_discrete_stats(const void* launch, const void* io, const void* head,
                                                 const void* stats)
{
    const auto L = from_unit<EnvLaunch>(launch);
    const auto p = from_unit<KParams>(L.kp);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<RolloutIO>(io);
    const auto h = from_unit<DiscHead>(head);
    const auto s = from_unit<CollectStatsIO>(stats);
    DiscTable tab;
    std::memcpy(tab.v, h.table, sizeof(tab.v));
    dispatch_env(RR_MODEL_3DOF, L.integ, [&](auto, auto i) {
        hipLaunchKernelGGL((rollout_discrete_stats_kernel<decltype(i)::value>), dim3(L.grid),
                           dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream, L.state, L.n, L.mode, p, b, o,
                           h.n_choices, tab, s);
    });
    hipLaunchKernelGGL(rollout_stats_reduce_kernel, dim3(1), dim3(kRedThreads), 0, (hipStream_t)L.stream, s);
    return (int)hipGetLastError();
}
