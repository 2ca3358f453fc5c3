// rocket_exact.hip — the second translation unit of librocket_hip.so: the exact-integrator
// kernels (step_exact_kernel, rocket_dopri5.inc) and nothing else, so that they can be compiled
// with their own scheduler setting (rl_rocket_amd/build.py: -amdgpu-schedule-metric-bias=100,
// register pressure first) without touching the fast kernels' code. With the fast kernels'
// scheduler the 6DOF exact kernel spilled 33 VGPRs to scratch at one wave per SIMD.
#include <cstring>

#include "rocket_device.h"
// Exact-integrator mode (RR_INT_DOPRI5): fp64 scipy RK45 restatement, compiled without FMA
// contraction so its roundings follow the reference's numpy arithmetic
#pragma clang fp contract(off)
#include "rocket_dopri5.inc"
#pragma clang fp contract(fast)

// the exact TU's only entry point (declared in rocket_device.h). bufs / io / xp point to the Bufs /
// StepIO / XParams of the calling TU.
extern "C" int rrx_launch_exact(int model, int variant, const void* xp, const void* bufs, const void* io,
                                double* state64, unsigned grid, void* stream)
{
    Bufs b;
    StepIO o;
    std::memcpy(&b, bufs, sizeof(Bufs));
    std::memcpy(&o, io, sizeof(StepIO));
    const XParams* x = static_cast<const XParams*>(xp);
    hipStream_t s = (hipStream_t)stream;
    // variant bit 0 = lean (6DOF above one wave per SIMD, the caller's choice): 256 registers, two
    // waves per SIMD hide each other's fp64 latency (147.6 vs 176.6 us at N = 524 288); otherwise the
    // in-loop dense output (no event re-derivation, no spills: 28.9 vs 32.1 us at 65 536,
    // profiles/r04/ab_lean/). Bit 1 = [NA][N] action planes (RR_FLAG_ACTION_SOA).
    const bool lean = variant & 1, soa = variant & 2;
#define RR_LAUNCH_X(M, L, A) \
    hipLaunchKernelGGL((step_exact_kernel<M, L, A>), dim3(grid), dim3(kBlock), 0, s, x, b, o, state64)
    if (model == RR_MODEL_6DOF && lean) {
        if (soa) RR_LAUNCH_X(6, true, true);
        else RR_LAUNCH_X(6, true, false);
    } else if (model == RR_MODEL_6DOF) {
        if (soa) RR_LAUNCH_X(6, false, true);
        else RR_LAUNCH_X(6, false, false);
    } else {
        if (soa) RR_LAUNCH_X(3, false, true);
        else RR_LAUNCH_X(3, false, false);
    }
#undef RR_LAUNCH_X
    return (int)hipGetLastError();
}
