// rocket_eval_exact_trace.hip — the fifteenth translation unit of librocket_hip.so: the one-launch
// evaluation under the exact integrator that also records whole episodes of chosen envs
// (rr_policy_evaluate_exact_trace).
//
// eval_exact_trace_kernel is eval_exact_kernel's loop (eval_exact/rocket_eval_exact.hip), statement for
// statement, plus the five recording regions of rocket_eval_body.inc: the slot's load, row 0 of episode
// 0, the step's record, row 0 of the next episode, and the length of an episode cut by max_steps. What
// is recorded for an env with a trace slot (rr_eval_trace, rocket_hip.h):
//   state row t + 1   s[j] = (float)y[j], the float32 cast of the fp64 state after the quaternion
//                     renormalisation / angle wrap and before any reset: the registers final_state
//                     is written from; row 0 is (float)y at the call, the auto-reset draw afterwards
//   action row t      the clipped mean a the solver stepped with
//   terms row t       (float)td[0 .. NT-1], the casts step_exact_kernel stores, then the reward r (with
//                     RR_FLAG_REWARD_ANNEALING the annealed one, the terms unchanged, as rr_step reports)
// The evaluation itself is eval_exact_kernel's: the same arithmetic in the same order, the same reset
// draws, the same rr_eval_out rows and handle state (tests/test_gpu_eval_exact_trace.py).
//
// The lane's slot and its step count live in two registers, not in the wave's obs tile as in
// rocket_eval_body.inc: this kernel runs one wave per SIMD (the 6DOF solver alone holds ~360 of the
// 512 registers), so two more do not cost a wave, and no instantiation uses scratch. The
// trace pointers are still read from the kernel-argument segment inside the branch only recording
// lanes take (trace_args<OFF>, rocket_eval.inc), so that they do not sit in SGPRs across dp::solve;
// the slot is made opaque after the adaptive loop like the env index, so that no trace address is
// formed ahead of it and stays live across it.
//
// It is a translation unit of its own so that every kernel which existed before it keeps its machine
// code (see eval_trace/rocket_eval_trace.hip), eval_exact_kernel included. Compiled in the library's
// link call with the collect unit's settings (build.py COLLECT_FLAGS); the exact units' scheduler
// bias changes instruction order, not arithmetic, and no register figure here.
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

// where tr0 sits in the kernel-argument segment: xp, B, io come before it (laid out like the members
// of a C struct, see kTraceArgOff)
constexpr size_t kExactTraceArgOff =
    karg_up(karg_up(karg_up(sizeof(const XParams*), alignof(Bufs)) + sizeof(Bufs), alignof(EvalIO)) + sizeof(EvalIO),
            alignof(EvalTraceIO));

template <int MODEL, int PREC>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) __attribute__((amdgpu_waves_per_eu(1))) void eval_exact_trace_kernel(
    const XParams* __restrict__ xp, const Bufs B, const EvalIO io, const EvalTraceIO tr0, double* __restrict__ state64)
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
    const uint32_t slot0 = (uint32_t)tr0.slot[i_in];  // the env's trace slot
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
    // ---- trace: a value outside [0, n_slots) records nothing (negative ones too: the compare is unsigned) ----
    const bool rec = valid && slot0 < (uint32_t)tr0.n_slots;
    uint32_t t_rec = 0;  // steps of the running episode taken in THIS call (the counter word's field may start above 0)
    // episodes ahead of (slot, ep) in the buffers; times rows per episode this may pass 2^32
    auto episode_index = [&](uint32_t slot) { return (uint64_t)slot * (uint32_t)n_ep + (uint32_t)ep; };
    if (rec) {  // row 0 of episode 0
        float s0[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) s0[j] = (float)y[j];
        trace_row<NS>(tr0.state + episode_index(slot0) * ((uint32_t)tr0.steps + 1u) * NS, s0);
    }
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
            // the env index and the trace slot re-derived after the adaptive loop, so that no address
            // stays live across it
            uint32_t i = i_in;
            asm volatile("" : "+v"(i));
            uint32_t slot = slot0;
            asm volatile("" : "+v"(slot));
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

            // ---- trace: the step's record (row t + 1 of the states: the un-reset s) ----
            if (rec) {
                const TraceArgs tr = trace_args<kExactTraceArgOff>();
                const uint32_t cap = tr.steps;
                const uint32_t t = t_rec;
                if (t < cap) {  // steps past the capacity are counted, not written
                    const uint64_t e = episode_index(slot);
                    trace_row<NS>(tr.state + (e * (cap + 1u) + t + 1u) * NS, s);
                    const uint64_t row = e * cap + t;
                    if (tr.action) trace_row<NA>(tr.action + row * NA, a);
                    if (tr.terms) {
                        float tt[NT];
#pragma unroll
                        for (int j = 0; j < NT; ++j) tt[j] = (float)td[j];
                        gfloat_t* tp = tr.terms + row * (NT + 1);
                        trace_row<NT>(tp, tt);
                        trace_row<1>(tp + NT, &r);
                    }
                }
                t_rec = done ? 0u : t + 1u;
                if (done) tr.length[(uint64_t)ep * tr.n_slots + slot] = (int32_t)(t + 1u);
            }

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
                // ---- trace: row 0 of the next episode is the auto-reset state ----
                if (rec && ep < n_ep) {
                    const TraceArgs tr = trace_args<kExactTraceArgOff>();
                    trace_row<NS>(tr.state + episode_index(slot) * (tr.steps + 1u) * NS, s);
                }
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
    // ---- trace: an episode cut by max_steps reports the steps it took so far ----
    if (rec && ep < n_ep) {
        const TraceArgs tr = trace_args<kExactTraceArgOff>();
        tr.length[(uint64_t)ep * tr.n_slots + slot0] = (int32_t)t_rec;
    }
    if (io.obs) {  // the post-call obs (of the fresh episode's first state where the env finished)
        observe();
        store_obs_tile<NS, EPW>(tile_all[wv], o, make_rsrc(io.obs, (uint64_t)NS * n * 4u), wave_base, lane, nvalid,
                                io.obs_vec_ok);
    }
}

}  // namespace
#pragma clang fp contract(fast)

// rr_policy_evaluate_exact_trace's launch (declared in rocket_device.h): eval_exact_trace_kernel<MODEL,
// PREC>, eval_exact_kernel's grid and workgroup. launch / io / trace point to the EvalExactLaunch /
// EvalIO / EvalTraceIO of the calling TU, which checked that the handle is an RR_INT_DOPRI5 one.
extern "C" int rrx_launch_eval_exact_trace(const void* launch, const void* io, const void* trace)
{
    const auto L = from_unit<EvalExactLaunch>(launch);
    const auto b = from_unit<Bufs>(L.bufs);
    const auto o = from_unit<EvalIO>(io);
    const auto t = from_unit<EvalTraceIO>(trace);
    auto run = [&](auto m) {
        dispatch_prec(L.prec, [&](auto pr) {
            hipLaunchKernelGGL((eval_exact_trace_kernel<decltype(m)::value, decltype(pr)::value>), dim3(L.grid),
                               dim3(rol::Shape<2>::kThreads), 0, (hipStream_t)L.stream,
                               static_cast<const XParams*>(L.xp), b, o, t, L.state64);
        });
    };
    if (L.model == RR_MODEL_6DOF) run(tag<6>{});
    else run(tag<3>{});
    return (int)hipGetLastError();
}
