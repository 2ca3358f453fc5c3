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
// reward: the histories of the reference's EpisodeAnalyzer (wrappers.py:189-235). Both kernels
// include one body, rocket_eval_body.inc.

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
#define RR_EVAL_TRACE 0
#include "rocket_eval_body.inc"
#undef RR_EVAL_TRACE
}

// ---- rr_policy_evaluate_trace: the same evaluation, recording whole episodes of chosen envs ----
//
// eval_trace_kernel is eval_kernel's body (rocket_eval_body.inc) with the regions that record
// (RR_EVAL_TRACE 1). The body is shared as text and not as a TRACE parameter of a function because
// eval_kernel must keep its machine code (tools/isa_diff.py): a body shared through a
// forceinlined __device__ template, with the LDS arrays declared in the body or in the wrappers,
// compiled every eval_kernel instantiation to different code. For the same reason it is
// instantiated in a translation unit of its own (eval_trace/rocket_eval_trace.hip), not next to
// eval_kernel in rocket_collect.hip. tests/test_gpu_eval_trace.py checks that recording changes
// nothing else: outputs and the handle's state must agree bit for bit.

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

// OFF: where the kernel's EvalTraceIO parameter sits (eval_exact_trace_kernel has another argument list)
template <size_t OFF = kTraceArgOff>
__device__ __forceinline__ TraceArgs trace_args()
{
    typedef const __attribute__((address_space(4))) char* karg_t;
    karg_t k = (karg_t)__builtin_amdgcn_kernarg_segment_ptr() + OFF;
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
#define RR_EVAL_TRACE 1
#include "rocket_eval_body.inc"
#undef RR_EVAL_TRACE
}

}  // namespace
