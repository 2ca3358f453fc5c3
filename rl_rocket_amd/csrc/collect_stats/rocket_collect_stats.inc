// rocket_collect_stats.inc — rr_rollout_collect_stats: the one-launch rollout collect that also
// accounts for the episodes it finishes (what SB3's Monitor / logger report as rollout/ep_rew_mean,
// rollout/ep_len_mean and train/explained_variance, reference main_6DOF.py:18-24, 62-69).
//
// rollout_collect_stats_kernel is rollout_step_kernel<MODEL, INTEG, PREC, MULTI = true, 2>
// (rocket_rollout.inc), statement for statement, plus the lines marked "stats" below. It is a
// second kernel in a translation unit of its own, not a STATS parameter of a shared body, because the
// collect kernels must keep their machine code (the reasons: rocket_eval.inc, at eval_trace_kernel).
// tests/test_gpu_collect_stats.py holds the two loops together: every rollout buffer, env output and
// the handle's state must be bitwise rr_rollout_collect's.
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

// pol::gae_env (rocket_policy.inc), the same loads, FMAs and stores, which also sums over the env's
// samples y = (double)ret[t], d = y - (double)value[t]: SB3 explained_variance's inputs
__device__ __forceinline__ void gae_env_stats(int64_t T, int64_t n, int64_t e, const float* __restrict__ rewards,
                                              const float* __restrict__ values, const float* __restrict__ starts,
                                              float last_value, float last_done, double gamma, double lam,
                                              float* __restrict__ adv, float* __restrict__ ret, double (&s)[4])
{
    constexpr int kC = 16;
    const double gl = gamma * lam;
    double last = 0.0;
    double next_v = last_value, next_g = last_done != 0.0f ? 0.0 : gamma, next_gl = last_done != 0.0f ? 0.0 : gl;
    for (int64_t t1 = T; t1 > 0; t1 -= kC) {
        const int c = t1 < kC ? (int)t1 : kC;
        float rw[kC], vl[kC], st[kC];
#pragma unroll
        for (int j = 0; j < kC; ++j)
            if (j < c) {
                const int64_t k = (t1 - 1 - j) * n + e;
                rw[j] = rewards[k];
                vl[j] = values[k];
                st[j] = starts[k];
            }
#pragma unroll
        for (int j = 0; j < kC; ++j)
            if (j < c) {
                const int64_t k = (t1 - 1 - j) * n + e;
                const double v = vl[j];
                last = fma(next_gl, last, fma(next_g, next_v, (double)rw[j] - v));
                adv[k] = (float)last;
                const float rt = (float)(last + v);
                ret[k] = rt;
                next_v = v;
                next_g = st[j] != 0.0f ? 0.0 : gamma;
                next_gl = st[j] != 0.0f ? 0.0 : gl;
                const double y = (double)rt, d = y - v;  // stats
                s[0] += y;
                s[1] += y * y;
                s[2] += d;
                s[3] += d * d;
            }
    }
}

}  // namespace rst

template <int MODEL, int INTEG, int PREC>
__global__ __launch_bounds__(rol::Shape<2>::kThreads) void rollout_collect_stats_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const RolloutIO io,
    const CollectStatsIO sio)
{
    constexpr int NTW = 2;
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT, EV = Dims<MODEL>::EV;
    constexpr int EPW = rol::Shape<NTW>::kEPW, NWV = rol::Shape<NTW>::kWaves, NTH = rol::Shape<NTW>::kThreads;
    using L = pol::Layout<NS, NA, PREC>;
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float tile_all[NWV][EPW * NS];
    __shared__ __attribute__((aligned(16))) rol::ResetParams<NS> rps;
    __shared__ __attribute__((aligned(16))) uint64_t acc[rst::Q_N][NTH];  // stats: the lanes' episode sums
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t n = n_envs;
    const uint32_t wave_idx = blockIdx.x * NWV + wv;
    const uint32_t wave_base = wave_idx * EPW;
    float* tile = tile_all[wv];
    const bool live = wave_base < n;
    const uint32_t i = wave_base + (lane & (EPW - 1));
    const bool valid = live && i < n && lane < (uint32_t)EPW;
    const uint32_t ic = i < n ? i : n - 1;
    const uint32_t vo = ic * 4u;
    const uint32_t plane = n * 4u;
    const uint32_t nvalid = !live ? 0u : ((n - wave_base) < (uint32_t)EPW ? (n - wave_base) : (uint32_t)EPW);
    const bool use_counter = mode & kModeCounter;
    const rsrc_t st_r = make_rsrc(state, (uint64_t)(NS + 3) * plane);
    const uint32_t v0_off = NS * plane, cw_off = (NS + 1) * plane, ret_off = (NS + 2) * plane;
    const uint32_t T = io.T;

    // stats: this lane's column starts empty (only this lane reads or writes it before the end)
    const uint32_t tx = threadIdx.x;
#pragma unroll
    for (int w = 0; w < rst::Q_N; ++w) acc[w][tx] = 0ull;
    acc[rst::Q_MIN_MAX][tx] = rst::pair_f(INFINITY, -INFINITY);

    // ---- loads (as step_kernel) ----
    uint32_t cw = use_counter ? bld_u(st_r, vo, cw_off) : 0u;
    float y0[NS], y1[NS], f0[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0[j] = bld_f(st_r, vo, j * plane);
    float v0 = bld_f(st_r, vo, v0_off);
    float ret = (mode & RR_FLAG_EPISODE_STATS) ? bld_f(st_r, vo, ret_off) : 0.0f;
    bool start = io.done[ic] != 0;
    pol::stage_params<NS, NA, PREC, NTH>(io.params, sp);
    if (mode & RR_FLAG_AUTO_RESET) rol::stage_reset<NS>(B.kp, &rps);
    const HotParams H = load_hot<NS>(P);
    const CounterLayout CL(P);
    const uint64_t it = *io.iter;
    float o[NS];
    bool v0_new = false;

    for (uint32_t k = 0; k < T; ++k) {
        const bool last = k + 1 == T;
        const size_t so = (size_t)k * n;  // [T][n] slice of step k

        // ---- obs of step t: rollout buffer + MFMA operands ----
        normalize_obs<NS>(y0, H.inv_norm, o);
        if (k > 0) {  // the tile's readers of the previous step are done
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        const rsrc_t bobs_r = make_rsrc(io.buf_obs + so * NS, (uint64_t)NS * plane);
        rol::ObsRead<NS, EPW> obr;
        if constexpr (kPolPrefetchA) rol::obs_begin<NS, EPW>(tile, o, bobs_r, wave_base, lane, nvalid, io.buf_obs_vec_ok, obr);
        else store_obs_tile<NS, EPW>(tile, o, bobs_r, wave_base, lane, nvalid, io.buf_obs_vec_ok);
        if (k == 0) __syncthreads();  // packed policy and reset parameters staged (T is uniform)

        // ---- policy (rocket_policy.inc towers on two 32-env tiles; env = lane) ----
        float value, mean[NA];
        typename pol::XOp<PREC>::T x[NTW][L::KP1];
        rol::regs_x<NS, NA, PREC>(o, x);
        rol::policy_forward<NS, NA, PREC, NTW>(sp, x, lane, value, mean, [&](int p) {
            if constexpr (kPolPrefetchA)
                if (p == 1) rol::obs_end<NS, EPW>(obr, bobs_r, wave_base, lane);
        });
        // sample: the key and arithmetic of policy_act_kernel
        const uint32_t t = io.t + k;
        uint32_t key = mix32((uint32_t)(P.id_off + i) ^ io.seed_lo);
        key = mix32(key ^ (uint32_t)it ^ io.seed_hi);
        key = mix32(key ^ (uint32_t)(it >> 32) ^ (t * 0x9E3779B9u));
        float eps[NA];
#pragma unroll
        for (int a = 0; a < NA; a += 2) {
            const float2 z = pol::normal2(key + (uint32_t)a * 0x632BE5ABu);
            eps[a] = z.x;
            if (a + 1 < NA) eps[a + 1] = z.y;
        }
        float act[NA], a_env[NA], lp = 0.0f;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const float ls = sp[L::LS + a];
            act[a] = mean[a] + __builtin_amdgcn_exp2f(ls * 1.44269504088896341f) * eps[a];
            lp += -0.5f * eps[a] * eps[a] - ls - 0.918938533204672742f;
            a_env[a] = fminf(1.0f, fmaxf(-1.0f, act[a]));
        }

        // ---- env step (step_kernel) ----
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
        normalize_obs<NS>(y1, H.inv_norm, o);  // terminal obs where done

        // ---- timeout bootstrap from the terminal obs (waves holding a truncated env only) ----
        float rb = r;
        if (__ballot(trunc && valid)) {
            rol::put_rows<NS, NTW>(tile, o, lane);
            const float vt = rol::tile_value<NS, NA, PREC, NTW>(sp, tile, lane);
            rb = trunc ? fmaf(io.gamma, vt, r) : r;
        }

        // ---- done compaction, terminal rows, auto-reset (step_kernel) ----
        const bool dv = done && valid;
        const uint64_t m = __ballot(dv);
        if (last && lane == 0 && live) B.done_bits[wave_idx] = m;
        if (m) {
            if (dv) {
                float* tr = B.term_obs + (size_t)i * NS;
#pragma unroll
                for (int j = 0; j < NS; ++j) tr[j] = o[j];
                B.term_ret[i] = ret;
                B.term_len[i] = el;
                // stats: the finished episode into this lane's column
                acc[rst::Q_EP_LEN][tx] += rst::pair(1u, (uint32_t)el);
                acc[rst::Q_LANDED_EVENT][tx] += rst::pair(tt[NT - 1] != 0.0f, event);
                acc[rst::Q_BOUNDS_TRUNC][tx] += rst::pair(bv, trunc);
                acc[rst::Q_NONFIN][tx] += nf ? 1ull : 0ull;
                const uint64_t mm = acc[rst::Q_MIN_MAX][tx];
                acc[rst::Q_MIN_MAX][tx] = rst::pair_f(fminf(rst::lo_f(mm), ret), fmaxf(rst::hi_f(mm), ret));
                const double rd = (double)ret;
                acc[rst::Q_SUM][tx] = __builtin_bit_cast(uint64_t, __builtin_bit_cast(double, acc[rst::Q_SUM][tx]) + rd);
                acc[rst::Q_SQ][tx] = __builtin_bit_cast(uint64_t, __builtin_bit_cast(double, acc[rst::Q_SQ][tx]) + rd * rd);
            }
            if ((mode & RR_FLAG_AUTO_RESET) && dv) {
                ResetStream key = reset_stream(rps.seed_w, P.id_off + i, cw);
                sample_ic<MODEL>(rps, key, y1, v0);
                v0_new = true;
                cw = CL.next_episode(cw);
                normalize_obs<NS>(y1, H.inv_norm, o);
                el = 0;
                ret = 0.0f;
            }
        }
        cw = CL.with_elapsed(cw, el);

        // ---- rollout buffer slices of step k; env outputs of the last step ----
        if (valid) {
#pragma unroll
            for (int a = 0; a < NA; ++a) io.buf_act[(so + i) * NA + a] = act[a];
            io.buf_val[so + i] = value;
            io.buf_logp[so + i] = lp;
            io.buf_start[so + i] = start ? 1.0f : 0.0f;
            io.buf_rew[so + i] = rb;
            if (last) {
                io.reward[i] = r;
                io.done[i] = (uint8_t)done;
                if (io.truncated) io.truncated[i] = (uint8_t)trunc;
                if (io.terms) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) io.terms[(size_t)j * n + i] = tt[j];
                    io.terms[(size_t)NT * n + i] = bv ? 1.0f : 0.0f;
                    io.terms[(size_t)(NT + 1) * n + i] = event ? 1.0f : (nf ? -1.0f : 0.0f);  // solve_ivp status
                }
            }
        }
        start = done;
#pragma unroll
        for (int j = 0; j < NS; ++j) y0[j] = y1[j];
    }

    // ---- env state (the post-step, post-reset state of the last step) ----
    if (valid) {
#pragma unroll
        for (int j = 0; j < NS; ++j) bst_f(st_r, y0[j], vo, j * plane);
        if (v0_new) bst_f(st_r, v0, vo, v0_off);
        if (use_counter) bst_u(st_r, cw, vo, cw_off);
        if (mode & RR_FLAG_EPISODE_STATS) bst_f(st_r, ret, vo, ret_off);
    }
    if (io.obs) {  // post-step (post-reset) obs
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        store_obs_tile<NS, EPW>(tile, o, make_rsrc(io.obs, (uint64_t)NS * plane), wave_base, lane, nvalid,
                                  io.obs_vec_ok);
    }
    // ---- end of the rollout: V(last obs), the last-done flags and GAE of this env ----
    rol::put_rows<NS, NTW>(tile, o, lane);
    const float lv = rol::tile_value<NS, NA, PREC, NTW>(sp, tile, lane);
    double ss[4] = {0.0, 0.0, 0.0, 0.0};  // stats: sum y, y^2, d, d^2 of this env's samples
    if (valid) {
        const float ld = start ? 1.0f : 0.0f;
        if (io.last_value) io.last_value[i] = lv;
        if (io.last_done) io.last_done[i] = ld;
        if (io.last_start) io.last_start[i] = ld;
        rst::gae_env_stats(T, n, i, io.buf_rew, io.buf_val, io.buf_start, lv, ld, io.gamma64, io.lam, io.buf_adv,
                           io.buf_ret, ss);
    }

    // ---- stats: the wave's row. Every lane takes its column out of LDS (its own words: no barrier),
    // the wave folds the 15 accumulated slots by butterfly, lane s < 16 stores slot s ----
    if (live) {
        uint64_t v[rst::kSlots - 1];
        const uint64_t q0 = acc[rst::Q_EP_LEN][tx], q1 = acc[rst::Q_LANDED_EVENT][tx], q2 = acc[rst::Q_BOUNDS_TRUNC][tx];
        const uint64_t q4 = acc[rst::Q_MIN_MAX][tx];
        v[RR_RSTAT_EPISODES] = (uint32_t)q0;
        v[RR_RSTAT_LEN_SUM] = q0 >> 32;
        v[RR_RSTAT_LANDED] = (uint32_t)q1;
        v[RR_RSTAT_END_EVENT] = q1 >> 32;
        v[RR_RSTAT_END_BOUNDS] = (uint32_t)q2;
        v[RR_RSTAT_END_TRUNCATED] = q2 >> 32;
        v[RR_RSTAT_END_NONFINITE] = acc[rst::Q_NONFIN][tx];
        v[RR_RSTAT_RET_SUM] = acc[rst::Q_SUM][tx];
        v[RR_RSTAT_RET_SQ] = acc[rst::Q_SQ][tx];
        v[RR_RSTAT_RET_MIN] = __builtin_bit_cast(uint64_t, (double)rst::lo_f(q4));
        v[RR_RSTAT_RET_MAX] = __builtin_bit_cast(uint64_t, (double)rst::hi_f(q4));
#pragma unroll
        for (int q = 0; q < 4; ++q) v[RR_RSTAT_Y_SUM + q] = __builtin_bit_cast(uint64_t, ss[q]);
        rst::wave_fold(v);
        uint64_t mine = (uint64_t)T * nvalid;  // RR_RSTAT_SAMPLES
#pragma unroll
        for (int q = 0; q < rst::kSlots - 1; ++q) mine = lane == (uint32_t)q ? v[q] : mine;
        if (lane < (uint32_t)rst::kSlots) sio.partials[(size_t)wave_idx * rst::kSlots + lane] = mine;
    }
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
