// rocket_collect_stats.inc — rr_rollout_collect_stats: the one-launch rollout collect that also
// accounts for the episodes it finishes (what SB3's Monitor / logger report as rollout/ep_rew_mean,
// rollout/ep_len_mean and train/explained_variance, reference main_6DOF.py:18-24, 62-69).
//
// rollout_collect_stats_kernel is the body of rollout_step_kernel<MODEL, INTEG, PREC, MULTI = true, 2>
// (rocket_rollout_body.inc) with the accounting regions (RR_COLLECT_STATS 1). The body is shared as
// text, not as a STATS parameter of a function, and the kernel sits in a translation unit of its own,
// because the collect kernels must keep their machine code (the reasons: rocket_eval.inc, at
// eval_trace_kernel). tests/test_gpu_collect_stats.py checks that the accounting changes nothing
// else: every rollout buffer, env output and the handle's state must be bitwise rr_rollout_collect's.
//
// Accounting. A lane that finishes an episode (done && valid, before the auto-reset clears ret / el)
// adds it to its own column of the workgroup's LDS block acc[word][thread]: seven 8-byte words per lane, read
// and written by that lane alone inside the done branch, so the step loop carries no register for
// them and waves without a done lane touch nothing. The GAE scan sums the lane's samples in
// registers. Every live wave then folds each slot over its 64 lanes by butterfly (one fixed balanced
// tree per slot: the same bits on every run, no atomics) and stores its 16-slot row, one 128-byte
// line, into partials[wave]. Lanes past n and dead waves add nothing: their
// columns keep the initial zeros / +-inf.
// rollout_stats_reduce_kernel (one workgroup, launched right after on the same stream) folds the
// rows in a fixed order into out[16] and, when given, into accum[16].

#pragma once

#include "rocket_device.h"
#include "rocket_policy.inc"
#include "rocket_rollout.inc"

namespace {

namespace rst {

constexpr int kSlots = RR_RSTAT_SLOTS;
static_assert(kSlots == 16 && kSlots * 8 == 128, "a wave's row is one 128-byte line");

// the per-lane 8-byte words of the LDS block (each [kThreads] wide: lane-contiguous ds_read_b64 /
// ds_write_b64, conflict-free). The counts sit in pairs, low | high << 32: a lane's count is at most
// n_steps and its length sum at most the TimeLimit's elapsed count it started with + n_steps (its
// episodes follow one another), both below 2^32, so a pair never carries
enum { Q_EP_LEN = 0, Q_LANDED_EVENT, Q_BOUNDS_TRUNC, Q_NONFIN, Q_MIN_MAX, Q_SUM, Q_SQ, Q_N };
__device__ __forceinline__ uint64_t pair(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
__device__ __forceinline__ uint64_t pair_f(float lo, float hi)
{
    return pair(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
}
__device__ __forceinline__ float lo_f(uint64_t q) { return __builtin_bit_cast(float, (uint32_t)q); }
__device__ __forceinline__ float hi_f(uint64_t q) { return __builtin_bit_cast(float, (uint32_t)(q >> 32)); }

// how slot s folds: 0 = int64 sum, 1 = fp64 sum, 2 = fp64 min, 3 = fp64 max
__host__ __device__ constexpr int slot_kind(int s)
{
    return s == RR_RSTAT_RET_MIN ? 2 : s == RR_RSTAT_RET_MAX ? 3 : (s >= RR_RSTAT_RET_SUM && s <= RR_RSTAT_D_SQ) ? 1 : 0;
}
// a op b on the 8-byte patterns of slot kind k. min / max skip a NaN (fmin / fmax), so a non-finite
// episode's NaN return leaves them alone; it does make the return sums NaN
__device__ __forceinline__ uint64_t fold(int k, uint64_t a, uint64_t b)
{
    const double x = __builtin_bit_cast(double, a), y = __builtin_bit_cast(double, b);
    const double r = k == 1 ? x + y : k == 2 ? fmin(x, y) : fmax(x, y);
    return k == 0 ? a + b : __builtin_bit_cast(uint64_t, r);
}
__device__ __forceinline__ uint64_t identity(int k)
{
    return k == 2 ? __builtin_bit_cast(uint64_t, (double)INFINITY) : k == 3 ? __builtin_bit_cast(uint64_t, -(double)INFINITY) : 0ull;
}

// the same fold with the kind known at compile time (the wave's butterfly: every lane holds all slots)
template <int K>
__device__ __forceinline__ uint64_t fold_c(uint64_t a, uint64_t b)
{
    if constexpr (K == 0) return a + b;
    const double x = __builtin_bit_cast(double, a), y = __builtin_bit_cast(double, b);
    return __builtin_bit_cast(uint64_t, K == 1 ? x + y : K == 2 ? fmin(x, y) : fmax(x, y));
}
// lane l's partner value, without LDS: lanes l and l ^ 32 / l ^ 16 through v_permlane32_swap /
// v_permlane16_swap of the value with itself (both partners then hold the pair as (lower lane's,
// upper lane's)), the four steps inside a row of 16 lanes through a DPP row rotate by 8, 4, 2, 1 (after
// the step before it the row's values repeat with that period, so the rotate pairs l with l ^ 8, ...)
template <int K, bool WIDE>
__device__ __forceinline__ uint64_t swap_fold(uint64_t v)
{
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    const auto rl = WIDE ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false)
                         : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto rh = WIDE ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false)
                         : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return fold_c<K>(pair((uint32_t)rl[0], (uint32_t)rh[0]), pair((uint32_t)rl[1], (uint32_t)rh[1]));
}
template <int K, int ROR>
__device__ __forceinline__ uint64_t row_fold(uint64_t v)
{
    constexpr int ctrl = 0x120 | ROR;  // DPP row_ror:ROR
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, 0xf, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, 0xf, 0xf, false);
    return fold_c<K>(v, pair(lo, hi));
}
// v[s] of every lane <- the fold of slot s over the wave's 64 lanes (all active): a butterfly, i.e.
// one fixed balanced tree per slot, so the same bits on every run
template <int S = 0>
__device__ __forceinline__ void wave_fold(uint64_t (&v)[kSlots - 1])
{
    if constexpr (S < kSlots - 1) {
        constexpr int K = slot_kind(S);
        v[S] = swap_fold<K, true>(v[S]);
        v[S] = swap_fold<K, false>(v[S]);
        v[S] = row_fold<K, 8>(v[S]);
        v[S] = row_fold<K, 4>(v[S]);
        v[S] = row_fold<K, 2>(v[S]);
        v[S] = row_fold<K, 1>(v[S]);
        wave_fold<S + 1>(v);
    }
}

}  // namespace rst

template <int MODEL, int INTEG, int PREC>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void rollout_collect_stats_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const RolloutIO io,
    const CollectStatsIO sio)
{
    constexpr bool MULTI = true;
    constexpr int NTW = 2;
#define RR_COLLECT_STATS 1
#include "rocket_rollout_body.inc"
#undef RR_COLLECT_STATS
}

// One workgroup, kRedGroups groups of kSlots lanes: lane s of group g folds slot s of the g-th
// contiguous share of the rows in row order; the groups' results then fold as a balanced tree over g
// (group g with group g + 32, + 16, ... + 1) into out[s] and, when given, into accum[s] (sums add,
// min / max fold; accum is never zeroed here). The order depends on the row count alone: the same
// bits on every run.
constexpr int kRedGroups = 64, kRedThreads = kRedGroups * rst::kSlots;
__global__ __launch_bounds__(kRedThreads) void rollout_stats_reduce_kernel(const CollectStatsIO sio)
{
    __shared__ uint64_t part[kRedGroups][rst::kSlots];
    const int s = (int)(threadIdx.x % rst::kSlots), g = (int)(threadIdx.x / rst::kSlots);
    const int kind = rst::slot_kind(s);
    const uint32_t per = (sio.rows + kRedGroups - 1) / kRedGroups;
    const uint32_t r_begin = (uint32_t)g * per, r_end = r_begin + per < sio.rows ? r_begin + per : sio.rows;
    const uint64_t old = sio.accum && g == 0 ? sio.accum[s] : 0ull;  // loaded beside the rows
    uint64_t a = rst::identity(kind);
    constexpr int kC = 16;  // rows loaded ahead of their fold
    for (uint32_t r0 = r_begin; r0 < r_end; r0 += kC) {
        uint64_t v[kC];
#pragma unroll
        for (int j = 0; j < kC; ++j)
            v[j] = r0 + j < r_end ? sio.partials[(size_t)(r0 + j) * rst::kSlots + s] : rst::identity(kind);
#pragma unroll
        for (int j = 0; j < kC; ++j) a = rst::fold(kind, a, v[j]);
    }
    part[g][s] = a;
    __syncthreads();
#pragma unroll
    for (int h = kRedGroups / 2; h >= 1; h >>= 1) {
        if (g < h) part[g][s] = rst::fold(kind, part[g][s], part[g + h][s]);
        __syncthreads();
    }
    if (g != 0) return;
    a = part[0][s];
    sio.out[s] = a;
    if (sio.accum) sio.accum[s] = rst::fold(kind, old, a);
}

}  // namespace
