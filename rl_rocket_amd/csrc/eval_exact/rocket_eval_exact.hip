// rocket_eval_exact.hip — the fifth translation unit of librocket_hip.so: deterministic policy
// evaluation under the exact integrator, whole episodes in ONE launch (rr_policy_evaluate_exact).
//
// eval_exact_kernel is eval_kernel's loop (rocket_eval.inc) with the env step replaced by
// step_exact_kernel's (rocket_dopri5.inc): lane = env, 64 envs per wave, 256 per workgroup, the
// packed policy and the auto-reset parameters staged once per workgroup; the fp64 state, v0, the
// counter word and the running return stay in registers from the first load to the last store.
// A loop iteration is one env step of the lanes still evaluating:
//   obs = float32(state64 / norm) (the exact mode's formula, not the fast kernels' state * inv_norm)
//   -> the pi tower and the action heads -> a = clip(mean, -1, 1) -> dp::make_ctl, dp::solve,
//   quaternion renormalisation / angle wrap, the float32 cast, dp::finish6 / finish3, the
//   TimeLimit -> ret += r
// with step_exact_kernel's statements in its order, so an episode is bitwise the one rr_policy_act
// + rr_step run where the policy's noise vanishes (tests/test_gpu_eval_exact.py). Where an episode
// ends the lane writes row [ep][i] of the output planes as eval_kernel does and auto-resets as
// step_exact_kernel does; a lane that has finished n_episodes is frozen in that post-reset state
// (it still feeds the wave's MFMAs). A wave leaves the loop when none of its lanes is evaluating or
// after max_steps iterations, both wave-uniform. Nothing is stored per step, and the waves of a
// launch never meet: each pays its own adaptive loops, not the slowest wave's of every step.
//
// One variant for every N: the in-loop dense output (solve<MODEL, false>), bitwise the lean
// variant rr_step picks at large N. One wave per SIMD: the 6DOF solver alone holds ~360 registers.
//
// It is a translation unit of its own so that every kernel which existed before it keeps its
// machine code (see eval_trace/rocket_eval_trace.hip), and because it needs both compile settings:
// the policy code outside `#pragma clang fp contract(off)` (as rocket_collect.hip), the solver and
// the kernel's own fp64 statements inside it (as rocket_exact.hip).
#include "rocket_device.h"
// layer-2 A fragments read a group ahead, as in rocket_collect.hip (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "rocket_eval.inc"
// the exact mode's roundings follow the reference's numpy arithmetic: no FMA contraction
#pragma clang fp contract(off)
#include "rocket_dopri5.inc"

namespace {

template <int MODEL, int PREC>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) __attribute__((amdgpu_waves_per_eu(1))) void eval_exact_kernel(
    const XParams* __restrict__ xp, const Bufs B, const EvalIO io, double* __restrict__ state64)
{
    const KParams& P = *B.kp;
    const XParams& X = *xp;
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT;
    constexpr int EPW = rol::Shape<2>::kEPW, NWV = rol::Shape<2>::kWaves;
    using L = pol::Layout<NS, NA, PREC>;
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float tile_all[NWV][EPW * NS];  // the post-call obs rows only
    __shared__ __attribute__((aligned(16))) rol::ResetParams<NS> rps;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t n = (uint32_t)B.n;
    const uint32_t wave_base = (blockIdx.x * NWV + wv) * EPW;
    // waves past n (last workgroup only) run on a clamped env, never evaluate and store nothing,
    // so every wave reaches the workgroup barrier below
    const bool live = wave_base < n;
    const uint32_t i0 = wave_base + lane;
    const bool valid = live && i0 < n;
    const uint32_t i_in = i0 < n ? i0 : n - 1;
    const uint32_t nvalid = !live ? 0u : ((n - wave_base) < (uint32_t)EPW ? (n - wave_base) : (uint32_t)EPW);

    // ---- loads (as step_exact_kernel: the fp64 planes are the state) ----
    float v0 = B.v0[i_in];
    uint32_t cw = B.counter[i_in];
    float ret = B.ep_ret[i_in];
    double y[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y[j] = state64[(size_t)j * n + i_in];
    pol::stage_params<NS, NA, PREC, rol::Shape<2>::kThreads>(io.params, sp);
    rol::stage_reset<NS>(B.kp, &rps);
    const int32_t n_ep = io.n_episodes;
    int32_t ep = 0;                  // episodes this env has completed
    float m0 = (float)y[NS - 1];     // float32 mass at the first state of the running episode
    float o[NS];
    auto observe = [&]() {
#pragma unroll
        for (int j = 0; j < NS; ++j)  // 6DOF: float32(state64 / n); 3DOF: float32(state32 / n), as step_exact_kernel
            o[j] = (float)((MODEL == 6 ? y[j] : (double)(float)y[j]) / X.norm[j]);
    };
    __syncthreads();  // packed policy and reset parameters staged

    for (uint64_t k = 0; k < io.max_steps; ++k) {
        const bool active = valid && ep < n_ep;
        if (__ballot(active) == 0) break;

        // ---- deterministic action: the pi tower's means, clipped (every lane: the MFMAs need the wave) ----
        observe();
        float value, mean[NA], a[NA];
        typename pol::XOp<PREC>::T x[2][L::KP1];
        rol::regs_x<NS, NA, PREC>(o, x);
        rol::policy_forward<NS, NA, PREC, 2, false>(sp, x, lane, value, mean);
#pragma unroll
        for (int j = 0; j < NA; ++j) a[j] = fminf(1.0f, fmaxf(-1.0f, mean[j]));

        if (active) {
            // ---- env step (step_exact_kernel) ----
            const uint32_t k_steps = cw & P.el_mask;
            // simulator clock: t_k = round(t_{k-1} + dt, 3) = rint(k * dt_milli) / 1000 (simulator.py:245)
            const double t0 = X.dt_milli > 0 ? (double)k_steps * X.dt_milli / 1000.0 : (double)k_steps * X.dt;
            float u[NA];
            const dp::XCtl c = dp::make_ctl<MODEL>(X, a, u);
            const int status = dp::solve<MODEL, false>(X, c, t0, y);
            // the env index re-derived after the adaptive loop, so that no address stays live across it
            uint32_t i = i_in;
            asm volatile("" : "+v"(i));
            if constexpr (MODEL == 6) {
                // _normalize_quaternion (simulator.py:250)
                const double nq = sqrt(y[6] * y[6] + y[7] * y[7] + y[8] * y[8] + y[9] * y[9]);
                y[6] /= nq;
                y[7] /= nq;
                y[8] /= nq;
                y[9] /= nq;
            } else {
                // _wrapTo2Pi (simulator.py:150-163)
                const double p2 = 2.0 * dp::kPi;
                y[2] = fmod(fmod(y[2], p2) + p2, p2);
            }
            float s[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) s[j] = (float)y[j];
            bool bv;
            double td[6];
            double rd = MODEL == 6 ? dp::finish6(X, s, u, v0, bv, td) : dp::finish3(X, s, u, v0, bv, td);
            if (P.flags & RR_FLAG_REWARD_ANNEALING)  // wrappers.py:72-86
                rd = td[3] + td[NT - 1] - X.xi * ((double)a[NA - 1] + 1.0);
            const float r = (float)rd;
            bool done = status != 0 || bv;
            bool trunc = false;
            int32_t el = min((int32_t)k_steps + 1, (int32_t)P.el_mask);  // saturated as CounterLayout::time_limit
            if (P.max_steps > 0 && el >= P.max_steps) {
                trunc = !done;
                done = true;
            }
            ret += r;

            if (done) {
                // ---- the episode's row (eval_kernel), then the auto-reset of step_exact_kernel ----
                const size_t row = (size_t)ep * n + i;
                if (io.ep_return) io.ep_return[row] = ret;
                if (io.ep_length) io.ep_length[row] = el;
                if (io.flags)
                    io.flags[row] = (uint8_t)((status > 0 ? RR_EVAL_EVENT : 0) | (bv ? RR_EVAL_BOUNDS : 0) |
                                              (trunc ? RR_EVAL_TRUNCATED : 0) | (status < 0 ? RR_EVAL_NONFINITE : 0) |
                                              ((float)td[NT - 1] != 0.0f ? RR_EVAL_LANDED : 0));
                if (io.used_mass) io.used_mass[row] = m0 - s[NS - 1];
                if (io.final_state) {
                    float* fs = io.final_state + (size_t)ep * NS * n + i;
#pragma unroll
                    for (int j = 0; j < NS; ++j) fs[(size_t)j * n] = s[j];
                }
                const uint32_t epn = (cw >> P.ep_shift) + 1u;
                ResetStream key = reset_stream(rps.seed_w, P.id_off + i, cw);  // cw is still this step's word
                sample_ic<MODEL>(rps, key, s, v0);
#pragma unroll
                for (int j = 0; j < NS; ++j) y[j] = (double)s[j];
                cw = epn << P.ep_shift;
                el = 0;
                ret = 0.0f;
                m0 = s[NS - 1];
                ++ep;
            }
            cw = (cw & ~P.el_mask) | ((uint32_t)el & P.el_mask);
        }
    }

    // ---- both state images, v0, counter word, running return; episodes completed ----
    if (valid) {
        uint32_t i = i_in;
        asm volatile("" : "+v"(i));
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            state64[(size_t)j * n + i] = y[j];
            B.state[(size_t)j * n + i] = (float)y[j];
        }
        B.v0[i] = v0;
        B.counter[i] = cw;
        B.ep_ret[i] = ret;
        io.episodes[i] = ep;
    }
    if (io.obs) {  // the post-call obs (of the fresh episode's first state where the env finished)
        observe();
        store_obs_tile<NS, EPW>(tile_all[wv], o, make_rsrc(io.obs, (uint64_t)NS * n * 4u), wave_base, lane, nvalid,
                                io.obs_vec_ok);
    }
}

}  // namespace
#pragma clang fp contract(fast)

// rr_policy_evaluate_exact's launch (declared in rocket_device.h): eval_exact_kernel<MODEL, PREC>,
// eval_kernel's grid and workgroup. launch / io point to the EvalExactLaunch / EvalIO of the
// calling TU.
extern "C" int rrx_launch_eval_exact(const void* launch, const void* io)
{
    const auto L = from_unit<EvalExactLaunch>(launch);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    auto run = [&](auto m) {
        dispatch_prec(L.prec, [&](auto pr) {
            hipLaunchKernelGGL((eval_exact_kernel<decltype(m)::value, decltype(pr)::value>), dim3(L.grid),
                               dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream,
                               static_cast<const XParams*>(L.xp), b, o, L.state64);
        });
    };
    if (L.model == RR_MODEL_6DOF) run(tag<6>{});
    else run(tag<3>{});
    return (int)hipGetLastError();
}
