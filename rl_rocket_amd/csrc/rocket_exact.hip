// rocket_exact.hip — the second translation unit of librocket_hip.so: the exact-integrator
// kernels (step_exact_kernel, rocket_dopri5.inc) and nothing else, so that they can be compiled
// with their own scheduler setting (rl_rocket_amd/build.py: -amdgpu-schedule-metric-bias=100,
// register pressure first) without touching the fast kernels' code. With the fast kernels'
// scheduler the 6DOF exact kernel spilled 33 VGPRs to scratch at one wave per SIMD.
#include "rocket_device.h"
// Exact-integrator mode (RR_INT_DOPRI5): fp64 scipy RK45 restatement, compiled without FMA
// contraction so its roundings follow the reference's numpy arithmetic
#pragma clang fp contract(off)
#include "rocket_dopri5.inc"
#pragma clang fp contract(fast)

// the exact TU's only entry point (declared in rocket_device.h). launch / io point to the
// ExactLaunch / StepIO of the calling TU.
extern "C" int rrx_launch_exact(const void* launch, const void* io)
{
    const auto L = from_unit<ExactLaunch>(launch);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<StepIO>(io);
    // variant bit 0 = lean (6DOF above one wave per SIMD, the caller's choice): 256 registers, two
    // waves per SIMD hide each other's fp64 latency (147.6 vs 176.6 us at N = 524 288); otherwise the
    // in-loop dense output (no event re-derivation, no spills: 28.9 vs 32.1 us at 65 536,
    // profiles/r04/ab_lean/). Bit 1 = [NA][N] action planes (RR_FLAG_ACTION_SOA).
    auto run = [&](auto m, auto lean) {
        dispatch_flag(L.variant & 2, [&](auto soa) {
            hipLaunchKernelGGL((step_exact_kernel<decltype(m)::value, decltype(lean)::value, decltype(soa)::value>),
                               dim3(L.grid), dim3(kBlock), 0, (hipStream_t)L.stream,
                               static_cast<const XParams*>(L.xp), b, o, L.state64);
        });
    };
    if (L.model == RR_MODEL_6DOF && (L.variant & 1)) run(tag<6>{}, std::true_type{});
    else if (L.model == RR_MODEL_6DOF) run(tag<6>{}, std::false_type{});
    else run(tag<3>{}, std::false_type{});
    return (int)hipGetLastError();
}
