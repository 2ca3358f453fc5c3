// rocket_eval_exact_discrete.hip — the sixteenth translation unit of librocket_hip.so: deterministic
// evaluation of the Categorical policy (the reference's DiscreteActions3DOF: Discrete(K) over a table of
// [gimbal, thrust] rows, K = 2 .. 4) under the exact integrator, whole episodes in ONE launch
// (rr_policy_evaluate_exact_discrete): the reference's sensitivity_test.py set-up, evaluate_policy on
// TimeLimit(DiscreteActions3DOF(RewardAnnealing(Rocket))) stepped by scipy RK45 + brentq.
//
// eval_exact_discrete_kernel is eval_exact_kernel<3, 0>'s loop (eval_exact/rocket_eval_exact.hip),
// statement for statement, with the Categorical head of rocket_eval_body.inc's RR_DISCRETE_HEAD region
// in the place of the Gaussian head's clipped means:
//   obs = float32(float32(state64) / norm) -> the pi tower and its NH = 4 heads, the logits -> the
//   action is the table row of the largest of the first n_choices logits, the lowest index on a tie
//   (torch.argmax; a zero-packed head >= n_choices never wins), NOT clipped -> dp::make_ctl,
//   dp::solve<3, false>, the angle wrap, the float32 cast, dp::finish3, the TimeLimit -> ret += r
// With RR_FLAG_REWARD_ANNEALING the annealed reward's thrust is the table row's thrust entry. The
// episode rows, the auto-reset draws, the final stores and the post-call obs tile are eval_exact_kernel's,
// so an episode is bitwise the one rr_policy_act_discrete + rr_step run where the sampled index is the
// argmax (tests/test_gpu_eval_exact_discrete.py).
//
// Fixed here: the 3DOF env (7 observations), fp32 towers, the image pol::Layout<7, 4, 0> of
// rr_policy_pack_discrete. K and the table travel by value in the kernel arguments, as in
// eval_discrete_kernel. One wave per SIMD as eval_exact_kernel<3, 0> has it; whether the 3DOF loop fits
// two has not been measured.
// Resource usage (python -m rl_rocket_amd.build --resource-usage, gfx950): 256 VGPRs, 60 AGPRs, 106 SGPRs
// (122 spilled to VGPR lanes), no scratch, 46 456 B of LDS per workgroup, one wave per SIMD;
// eval_exact_kernel<3, 0> has 256 / 58 / 106 (114), no scratch and 45 944 B (two fewer head columns).
//
// It is a translation unit of its own so that every kernel which existed before it keeps its machine
// code (see eval_trace/rocket_eval_trace.hip). Compiled in the library's link call with the collect
// unit's settings (build.py COLLECT_FLAGS), as eval_exact_trace/rocket_eval_exact_trace.hip is.
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

// the choices' [gimbal, thrust] rows (eval_discrete_kernel's argument of the same name and layout)
struct DiscTable {
    float v[4][2];
};

__global__ __launch_bounds__(rol::Shape<2>::kThreads) __attribute__((amdgpu_waves_per_eu(1))) void eval_exact_discrete_kernel(
    const XParams* __restrict__ xp, const Bufs B, const EvalIO io, double* __restrict__ state64, int n_choices,
    const DiscTable tab)
{
    constexpr int MODEL = 3, PREC = 0;
    const KParams& P = *B.kp;
    const XParams& X = *xp;
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT;
    constexpr int EPW = rol::Shape<2>::kEPW, NWV = rol::Shape<2>::kWaves;
    constexpr int NH = 4;  // heads of the packed image (rr_policy_pack_discrete): the logits
    static_assert(NS == 7 && NA == 2, "the table rows are [gimbal, thrust] of the 3DOF env");
    using L = pol::Layout<NS, NH, PREC>;
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
    pol::stage_params<NS, NH, PREC, rol::Shape<2>::kThreads>(io.params, sp);
    rol::stage_reset<NS>(B.kp, &rps);
    const int32_t n_ep = io.n_episodes;
    int32_t ep = 0;                  // episodes this env has completed
    float m0 = (float)y[NS - 1];     // float32 mass at the first state of the running episode
    float o[NS];
    auto observe = [&]() {
#pragma unroll
        for (int j = 0; j < NS; ++j)  // float32(state32 / n), as step_exact_kernel's 3DOF arm
            o[j] = (float)((double)(float)y[j] / X.norm[j]);
    };
    __syncthreads();  // packed policy and reset parameters staged

    for (uint64_t k = 0; k < io.max_steps; ++k) {
        const bool active = valid && ep < n_ep;
        if (__ballot(active) == 0) break;

        // ---- deterministic action: the most probable choice's table row (every lane: the MFMAs need the wave) ----
        observe();
        float value, mean[NH], a[NA];
        typename pol::XOp<PREC>::T x[2][L::KP1];
        rol::regs_x<NS, NH, PREC>(o, x);
        rol::policy_forward<NS, NH, PREC, 2, false>(sp, x, lane, value, mean);
        // the lowest q < n_choices with the largest logit (torch.argmax: on a tie the lowest index; a
        // zero-packed head >= n_choices never wins), then its table row by compares; no clip
        float zb = mean[0];
        a[0] = tab.v[0][0];
        a[1] = tab.v[0][1];
#pragma unroll
        for (int q = 1; q < NH; ++q)
            if (q < n_choices && mean[q] > zb) {
                zb = mean[q];
                a[0] = tab.v[q][0];
                a[1] = tab.v[q][1];
            }

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
            // _wrapTo2Pi (simulator.py:150-163)
            const double p2 = 2.0 * dp::kPi;
            y[2] = fmod(fmod(y[2], p2) + p2, p2);
            float s[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) s[j] = (float)y[j];
            bool bv;
            double td[6];
            double rd = dp::finish3(X, s, u, v0, bv, td);
            if (P.flags & RR_FLAG_REWARD_ANNEALING)  // wrappers.py:72-86; the thrust is the table row's
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

DiscTable table_of(const DiscHead& h)
{
    DiscTable tab;
    std::memcpy(tab.v, h.table, sizeof(tab.v));
    return tab;
}

}  // namespace
#pragma clang fp contract(fast)

// rr_policy_evaluate_exact_discrete's launch (declared in rocket_device.h): eval_exact_discrete_kernel on
// eval_exact_kernel's grid and workgroup. launch / io / head point to the EvalExactLaunch / EvalIO /
// DiscHead of the calling TU, which checked that the handle is a 3DOF RR_INT_DOPRI5 one and the
// precision fp32.
extern "C" int rrx_launch_eval_exact_discrete(const void* launch, const void* io, const void* head)
{
    const auto L = from_unit<EvalExactLaunch>(launch);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    const auto h = from_unit<DiscHead>(head);
    const DiscTable tab = table_of(h);
    hipLaunchKernelGGL(eval_exact_discrete_kernel, dim3(L.grid), dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream,
                       static_cast<const XParams*>(L.xp), b, o, L.state64, h.n_choices, tab);
    return (int)hipGetLastError();
}
