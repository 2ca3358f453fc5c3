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
//
// eval_trace_kernel (second half of this file, rr_policy_evaluate_trace) is the same loop that also
// writes, for the envs the caller gives a trace slot, every step's state, action, reward terms and
// reward: the histories of the reference's EpisodeAnalyzer (wrappers.py:189-235).

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

// ---- rr_policy_evaluate_trace: the same evaluation, recording whole episodes of chosen envs ----
//
// eval_trace_kernel is eval_kernel's loop, statement for statement, plus the stores marked
// "trace" below. It is a second kernel and not a TRACE parameter of a shared body because
// eval_kernel must keep its machine code (tools/isa_diff.py): a body shared through a
// forceinlined __device__ template, with the LDS arrays declared in the body or in the wrappers,
// compiled every eval_kernel instantiation to different code. For the same reason it is
// instantiated in a translation unit of its own (eval_trace/rocket_eval_trace.hip), not next to
// eval_kernel in rocket_collect.hip. tests/test_gpu_eval_trace.py holds the two loops together:
// outputs and the handle's state must agree bit for bit.

// where the recorded envs' histories go (rr_eval_trace, rocket_hip.h). One contiguous block per
// slot, so an env writes whole rows of its own.
struct EvalTraceIO {
    const int32_t* slot;        // [n]: trace slot of env i in [0, n_slots), anything else = not recorded
    float* state;               // [n_slots][n_episodes][steps + 1][NS]
    float* action;              // [n_slots][n_episodes][steps][NA] or nullptr
    float* terms;               // [n_slots][n_episodes][steps][NT + 1] or nullptr
    int32_t* length;            // [n_episodes][n_slots]
    int32_t n_slots;
    int32_t steps;
};
static_assert(std::is_trivially_copyable_v<EvalTraceIO>, "EvalTraceIO crosses TUs by memcpy (rrc_launch_eval_trace)");

// Cache policy of the trace rows: 0 = the default policy, 1 = nontemporal stores (nt). The rows are
// written once, 28-56 B per lane at addresses a whole slot block apart, and nothing in the launch
// reads them back, which reads like a case for nt. Measured (tools/eval_trace_bench.py, N = K =
// 65 536, 6DOF, 0.54 GB of rows in one launch of 1.1 ms) it is the opposite: with the default policy
// the launch takes 39 us longer than the plain evaluation (inside the plain call's spread), with nt
// 1 480 us longer (367 GB/s): the partial-line nt stores go to memory one by one, the default ones
// merge in L2 and leave in whole lines (DESIGN.md, "Recording evaluation"). The other value stays
// buildable for that A/B (-DRR_TRACE_NT=1).
#ifndef RR_TRACE_NT
#define RR_TRACE_NT 0
#endif

// N consecutive floats of one lane's row. The backend merges them into 16- / 8-B global stores
// (which need 4-B alignment only).
template <int N, class P>
__device__ __forceinline__ void trace_row(P* __restrict__ p, const float* v)
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if constexpr (RR_TRACE_NT != 0) __builtin_nontemporal_store(v[j], p + j);
        else p[j] = v[j];
    }
}

// The trace arguments, read from the kernel-argument segment where they are used. Held as kernel
// parameters through the loop they are 12 more live SGPRs in a kernel that already parks 33 SGPRs
// in VGPR lanes: the 6DOF RK4 fp32 kernel then needed 260 registers (one wave per SIMD, where
// eval_kernel runs two) or, held to 256, spilled to scratch. Loaded inside the branch only
// recording waves take (scalar loads, cached), they are live only there. The empty asm makes the
// address opaque: loads from the argument segment are speculatable and would otherwise be hoisted
// back to the kernel's entry. kTraceArgOff is the offset of eval_trace_kernel's last parameter:
// the arguments are laid out like the members of a C struct (AMDGPU kernarg ABI).
// (pointers of the global address space: a pointer made from a loaded integer is otherwise generic
// and its stores become flat_store)
typedef __attribute__((address_space(1))) float gfloat_t;
typedef __attribute__((address_space(1))) int32_t gint32_t;
struct TraceArgs {
    gfloat_t* state;
    gfloat_t* action;
    gfloat_t* terms;
    gint32_t* length;
    uint32_t n_slots;
    uint32_t steps;
};
constexpr size_t karg_up(size_t off, size_t align) { return (off + align - 1) / align * align; }
constexpr size_t kTraceArgOff =
    karg_up(karg_up(karg_up(karg_up(sizeof(float*) + 2 * sizeof(uint32_t), alignof(KParams)) + sizeof(KParams),
                            alignof(Bufs)) + sizeof(Bufs), alignof(EvalIO)) + sizeof(EvalIO), alignof(EvalTraceIO));

__device__ __forceinline__ TraceArgs trace_args()
{
    typedef const __attribute__((address_space(4))) char* karg_t;
    karg_t k = (karg_t)__builtin_amdgcn_kernarg_segment_ptr() + kTraceArgOff;
    asm volatile("" : "+s"(k));
    auto ptr = [&](size_t off) { return *(const __attribute__((address_space(4))) uint64_t*)(k + off); };
    auto word = [&](size_t off) { return *(const __attribute__((address_space(4))) uint32_t*)(k + off); };
    TraceArgs t;
    t.state = (gfloat_t*)ptr(offsetof(EvalTraceIO, state));
    t.action = (gfloat_t*)ptr(offsetof(EvalTraceIO, action));
    t.terms = (gfloat_t*)ptr(offsetof(EvalTraceIO, terms));
    t.length = (gint32_t*)ptr(offsetof(EvalTraceIO, length));
    t.n_slots = word(offsetof(EvalTraceIO, n_slots));
    t.steps = word(offsetof(EvalTraceIO, steps));
    return t;
}

template <int MODEL, int INTEG, int PREC>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void eval_trace_kernel(float* __restrict__ state,
                                                                             uint32_t n_envs, uint32_t mode,
                                                                             const KParams P, const Bufs B,
                                                                             const EvalIO io, const EvalTraceIO tr0)
{
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT, EV = Dims<MODEL>::EV;
    constexpr int EPW = rol::Shape<2>::kEPW, NWV = rol::Shape<2>::kWaves;
    using L = pol::Layout<NS, NA, PREC>;
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float tile_all[NWV][EPW * NS];
    __shared__ __attribute__((aligned(16))) rol::ResetParams<NS> rps;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t n = n_envs;
    const uint32_t wave_base = (blockIdx.x * NWV + wv) * EPW;
    const bool live = wave_base < n;
    const uint32_t i = wave_base + lane;
    const bool valid = live && i < n;
    const uint32_t ic = i < n ? i : n - 1;
    const uint32_t vo = ic * 4u;
    const uint32_t plane = n * 4u;
    const uint32_t nvalid = !live ? 0u : ((n - wave_base) < (uint32_t)EPW ? (n - wave_base) : (uint32_t)EPW);
    const rsrc_t st_r = make_rsrc(state, (uint64_t)(NS + 3) * plane);
    const uint32_t v0_off = NS * plane, cw_off = (NS + 1) * plane, ret_off = (NS + 2) * plane;

    // ---- loads (eval_kernel's, and the env's trace slot) ----
    uint32_t cw = bld_u(st_r, vo, cw_off);
    float y0[NS], y1[NS], f0[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0[j] = bld_f(st_r, vo, j * plane);
    float v0 = bld_f(st_r, vo, v0_off);
    float ret = (mode & RR_FLAG_EPISODE_STATS) ? bld_f(st_r, vo, ret_off) : 0.0f;
    const uint32_t slot0 = bld_u(make_rsrc(tr0.slot, plane), vo, 0);  // trace
    pol::stage_params<NS, NA, PREC, rol::Shape<2>::kThreads>(io.params, sp);
    rol::stage_reset<NS>(B.kp, &rps);
    const HotParams H = load_hot<NS>(P);
    const CounterLayout CL(P);
    const int32_t n_ep = io.n_episodes;
    int32_t ep = 0;
    float m0 = y0[NS - 1];
    bool v0_new = false;
    float o[NS];
    // ---- trace: a recording lane carries only its mask bit; the 64-bit row index is formed where
    // a row is stored, inside the branch only recording lanes take ----
    // a value outside [0, n_slots) records nothing (negative ones too: the compare is unsigned)
    const bool rec = valid && slot0 < (uint32_t)tr0.n_slots;
    // Each lane's slot and step count live in LDS, not in registers: the 6DOF loop sits at the
    // 256-VGPR line of two waves per SIMD (eval_kernel<6, RK4, fp32>: 254), and two more values
    // live across the policy's MFMAs cost the second wave or spilled to scratch. They use the
    // wave's obs tile, which is idle until the loop has ended (words [0, 64) and [64, 128) of
    // >= 448), so the workgroup's LDS stays eval_kernel's. Only recording lanes touch these words,
    // in the branch that stores a row. volatile: a load hoisted out of the loop would put the
    // value back into a register.
    // lane_t: steps of the running episode taken in THIS call (the counter word's field may start above 0)
    static_assert(EPW * NS >= 2 * kWave, "the wave's obs tile holds lane_slot and lane_t");
    typedef volatile __attribute__((address_space(3))) uint32_t lds_word_t;
    lds_word_t* const lane_slot = (lds_word_t*)tile_all[wv];
    lds_word_t* const lane_t = lane_slot + kWave;
    lane_slot[lane] = slot0;
    lane_t[lane] = 0;
    // episodes ahead of (slot, ep) in the buffers; times rows per episode this may pass 2^32
    // this lane's word of lane_slot / lane_t, formed where it is used from values the loop keeps
    // anyway (the opaque asm keeps the LDS address from being hoisted into a register of its own)
    auto lane_word = [&]() {
        uint32_t w = lane;
        asm volatile("" : "+v"(w));
        return w;
    };
    auto episode_index = [&](uint32_t slot) { return (uint64_t)slot * (uint32_t)n_ep + (uint32_t)ep; };
    if (rec) trace_row<NS>(tr0.state + episode_index(slot0) * ((uint32_t)tr0.steps + 1u) * NS, y0);  // row 0 of episode 0
    __syncthreads();  // packed policy and reset parameters staged

    for (uint64_t k = 0; k < io.max_steps; ++k) {
        const bool active = valid && ep < n_ep;
        if (__ballot(active) == 0) break;

        normalize_obs<NS>(y0, H.inv_norm, o);
        float value, mean[NA], a_env[NA];
        typename pol::XOp<PREC>::T x[2][L::KP1];
        rol::regs_x<NS, NA, PREC>(o, x);
        rol::policy_forward<NS, NA, PREC, 2, false>(sp, x, lane, value, mean);
#pragma unroll
        for (int a = 0; a < NA; ++a) a_env[a] = fminf(1.0f, fmaxf(-1.0f, mean[a]));

        if (active) {
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

            // ---- trace: the step's record (row t + 1 of the states: the un-reset y1) ----
            if (rec) {
                const TraceArgs tr = trace_args();
                const uint32_t cap = tr.steps;
                const uint32_t lw = lane_word();
                const uint32_t slot = lane_slot[lw], t = lane_t[lw];
                if (t < cap) {  // steps past the capacity are counted, not written
                    const uint64_t e = episode_index(slot);
                    trace_row<NS>(tr.state + (e * (cap + 1u) + t + 1u) * NS, y1);
                    const uint64_t row = e * cap + t;
                    if (tr.action) trace_row<NA>(tr.action + row * NA, a_env);
                    if (tr.terms) {
                        gfloat_t* tp = tr.terms + row * (NT + 1);
                        trace_row<NT>(tp, tt);
                        trace_row<1>(tp + NT, &r);
                    }
                }
                lane_t[lw] = done ? 0u : t + 1u;
                if (done) tr.length[(uint64_t)ep * tr.n_slots + slot] = (int32_t)(t + 1u);
            }

            if (done) {
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
                ResetStream key = reset_stream(rps.seed_w, P.id_off + i, cw);
                sample_ic<MODEL>(rps, key, y1, v0);
                v0_new = true;
                cw = CL.next_episode(cw);
                el = 0;
                ret = 0.0f;
                m0 = y1[NS - 1];
                ++ep;
                // ---- trace: row 0 of the next episode is the auto-reset state ----
                if (rec && ep < n_ep) {
                    const TraceArgs tr = trace_args();
                    trace_row<NS>(tr.state + episode_index(lane_slot[lane_word()]) * (tr.steps + 1u) * NS, y1);
                }
            }
            cw = CL.with_elapsed(cw, el);
#pragma unroll
            for (int j = 0; j < NS; ++j) y0[j] = y1[j];
        }
    }

    if (valid) {
#pragma unroll
        for (int j = 0; j < NS; ++j) bst_f(st_r, y0[j], vo, j * plane);
        if (v0_new) bst_f(st_r, v0, vo, v0_off);
        bst_u(st_r, cw, vo, cw_off);
        if (mode & RR_FLAG_EPISODE_STATS) bst_f(st_r, ret, vo, ret_off);
        io.episodes[i] = ep;
    }
    // ---- trace: an episode cut by max_steps reports the steps it took so far ----
    if (rec && ep < n_ep) {
        const TraceArgs tr = trace_args();
        const uint32_t lw = lane_word();
        tr.length[(uint64_t)ep * tr.n_slots + lane_slot[lw]] = (int32_t)lane_t[lw];
    }
    if (io.obs) {
        normalize_obs<NS>(y0, H.inv_norm, o);
        store_obs_tile<NS, EPW>(tile_all[wv], o, make_rsrc(io.obs, (uint64_t)NS * plane), wave_base, lane, nvalid,
                                io.obs_vec_ok);
    }
}

}  // namespace
