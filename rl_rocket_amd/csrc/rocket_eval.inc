// rocket_eval.inc — deterministic policy evaluation, whole episodes in ONE launch
// (rr_policy_evaluate): what SB3's EvalCallback / evaluate_policy(deterministic=True) computes on
// an EpisodeAnalyzer-wrapped env (reference main_6DOF.py:60-103, wrappers.py:189-235), for every
// env of the handle at once.
//
// The layout and every piece of arithmetic are rollout_step_kernel<..., MULTI = true, 2>'s
// (rocket_rollout.inc): lane = env, 64 envs per wave, 256 per workgroup, the packed policy and the
// auto-reset parameters staged once per workgroup, the env state, counter word and running return
// in registers from the first load to the last store. A loop iteration is one env step of the
// lanes still evaluating:
//   obs = state * inv_norm -> the pi tower and the action heads (no value tower, no noise, no
//   log-prob) -> a_env = clip(mean, -1, 1) -> env step, reward terms, TimeLimit -> ret += r
// with the same functions in the same order as the collect, so an episode is bitwise the one
// rr_rollout_step runs when the policy's noise vanishes (tests/test_gpu_eval.py).
// Where an episode ends the lane writes row [ep][i] of the output planes, draws its auto-reset
// from the reset stream (same key: seed words, env id, counter word) and starts the next episode;
// a lane that has finished n_episodes is frozen in that post-reset state: it still feeds the
// wave's MFMAs (its column is computed and dropped) but nothing of it changes any more. A wave
// leaves the loop when none of its lanes is evaluating or after max_steps iterations, both
// wave-uniform. Nothing is stored per step.

#pragma once

#include <type_traits>

#include "rocket_device.h"
#include "rocket_policy.inc"
#include "rocket_rollout.inc"

namespace {

struct EvalIO {
    const float* params;        // packed policy (rr_policy_layout / rr_policy_pack), 16-B aligned
    int32_t* episodes;          // [n] episodes completed
    float* ep_return;           // [n_episodes][n] planes, any may be nullptr
    int32_t* ep_length;
    uint8_t* flags;             // RR_EVAL_*
    float* used_mass;
    float* final_state;         // [n_episodes][NS][n]
    float* obs;                 // [n][NS] post-call obs or nullptr
    uint64_t max_steps;         // iterations of the step loop (>= 1)
    int32_t n_episodes;
    int32_t obs_vec_ok;
};
static_assert(std::is_trivially_copyable_v<EvalIO>, "EvalIO crosses TUs by memcpy (rrc_launch_eval)");

template <int MODEL, int INTEG, int PREC>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void eval_kernel(float* __restrict__ state, uint32_t n_envs,
                                                                       uint32_t mode, const KParams P, const Bufs B,
                                                                       const EvalIO io)
{
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT, EV = Dims<MODEL>::EV;
    constexpr int EPW = rol::Shape<2>::kEPW, NWV = rol::Shape<2>::kWaves;
    using L = pol::Layout<NS, NA, PREC>;
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float tile_all[NWV][EPW * NS];  // the post-call obs rows only
    __shared__ __attribute__((aligned(16))) rol::ResetParams<NS> rps;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t n = n_envs;
    const uint32_t wave_base = (blockIdx.x * NWV + wv) * EPW;
    // waves past n (last workgroup only) run on a clamped env, never evaluate and store nothing,
    // so every wave reaches the workgroup barrier below
    const bool live = wave_base < n;
    const uint32_t i = wave_base + lane;
    const bool valid = live && i < n;
    const uint32_t ic = i < n ? i : n - 1;
    const uint32_t vo = ic * 4u;
    const uint32_t plane = n * 4u;
    const uint32_t nvalid = !live ? 0u : ((n - wave_base) < (uint32_t)EPW ? (n - wave_base) : (uint32_t)EPW);
    const rsrc_t st_r = make_rsrc(state, (uint64_t)(NS + 3) * plane);
    const uint32_t v0_off = NS * plane, cw_off = (NS + 1) * plane, ret_off = (NS + 2) * plane;

    // ---- loads (as rollout_step_kernel; an auto-reset handle always keeps counter words) ----
    uint32_t cw = bld_u(st_r, vo, cw_off);
    float y0[NS], y1[NS], f0[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0[j] = bld_f(st_r, vo, j * plane);
    float v0 = bld_f(st_r, vo, v0_off);
    float ret = (mode & RR_FLAG_EPISODE_STATS) ? bld_f(st_r, vo, ret_off) : 0.0f;
    pol::stage_params<NS, NA, PREC, rol::Shape<2>::kThreads>(io.params, sp);
    rol::stage_reset<NS>(B.kp, &rps);
    const HotParams H = load_hot<NS>(P);
    const CounterLayout CL(P);
    const int32_t n_ep = io.n_episodes;
    int32_t ep = 0;            // episodes this env has completed
    float m0 = y0[NS - 1];     // mass at the first state of the running episode
    bool v0_new = false;
    float o[NS];
    __syncthreads();  // packed policy and reset parameters staged

    for (uint64_t k = 0; k < io.max_steps; ++k) {
        const bool active = valid && ep < n_ep;
        if (__ballot(active) == 0) break;

        // ---- deterministic action: the pi tower's means, clipped ----
        normalize_obs<NS>(y0, H.inv_norm, o);
        float value, mean[NA], a_env[NA];
        typename pol::XOp<PREC>::T x[2][L::KP1];
        rol::regs_x<NS, NA, PREC>(o, x);
        rol::policy_forward<NS, NA, PREC, 2, false>(sp, x, lane, value, mean);
#pragma unroll
        for (int a = 0; a < NA; ++a) a_env[a] = fminf(1.0f, fmaxf(-1.0f, mean[a]));

        if (active) {
            // ---- env step (rollout_step_kernel / step_kernel) ----
            const Ctl c = make_ctl<MODEL>(P, a_env);
            integrate<MODEL, INTEG>(P, c, y0, P.h, y1, f0);
            const float g0 = y0[EV], g1 = y1[EV];
            const bool event = (g0 <= 0.0f && g1 >= 0.0f) || (g0 >= 0.0f && g1 <= 0.0f);
            if (event) event_step<MODEL, INTEG>(P, c, y0, f0, y1);
            post_integrate<MODEL>(y1);
            bool bv;
            float tt[NT];
            const float r = reward_terms<MODEL>(H, y1, a_env, v0, bv, tt);
            const bool nf = nonfinite<NS>(y1);
            bool done = event || bv || nf, trunc;
            int32_t el = CL.time_limit(cw, done, trunc);
            ret += r;

            if (done) {
                // ---- the episode's row, then the auto-reset of the step kernels ----
                const size_t row = (size_t)ep * n + i;
                if (io.ep_return) io.ep_return[row] = ret;
                if (io.ep_length) io.ep_length[row] = el;
                if (io.flags)
                    io.flags[row] = (uint8_t)((event ? RR_EVAL_EVENT : 0) | (bv ? RR_EVAL_BOUNDS : 0) |
                                              (trunc ? RR_EVAL_TRUNCATED : 0) | (nf ? RR_EVAL_NONFINITE : 0) |
                                              (tt[NT - 1] != 0.0f ? RR_EVAL_LANDED : 0));
                if (io.used_mass) io.used_mass[row] = m0 - y1[NS - 1];
                if (io.final_state) {
                    float* fs = io.final_state + (size_t)ep * NS * n + i;
#pragma unroll
                    for (int j = 0; j < NS; ++j) fs[(size_t)j * n] = y1[j];
                }
                ResetStream key = reset_stream(rps.seed_w, P.id_off + i, cw);  // cw is still this step's word
                sample_ic<MODEL>(rps, key, y1, v0);
                v0_new = true;
                cw = CL.next_episode(cw);
                el = 0;
                ret = 0.0f;
                m0 = y1[NS - 1];
                ++ep;
            }
            cw = CL.with_elapsed(cw, el);
#pragma unroll
            for (int j = 0; j < NS; ++j) y0[j] = y1[j];
        }
    }

    // ---- env state, counter word, running return; episodes completed ----
    if (valid) {
#pragma unroll
        for (int j = 0; j < NS; ++j) bst_f(st_r, y0[j], vo, j * plane);
        if (v0_new) bst_f(st_r, v0, vo, v0_off);
        bst_u(st_r, cw, vo, cw_off);
        if (mode & RR_FLAG_EPISODE_STATS) bst_f(st_r, ret, vo, ret_off);
        io.episodes[i] = ep;
    }
    if (io.obs) {  // the post-call obs (of the fresh episode's first state where the env finished)
        normalize_obs<NS>(y0, H.inv_norm, o);
        store_obs_tile<NS, EPW>(tile_all[wv], o, make_rsrc(io.obs, (uint64_t)NS * plane), wave_base, lane, nvalid,
                                io.obs_vec_ok);
    }
}

}  // namespace
