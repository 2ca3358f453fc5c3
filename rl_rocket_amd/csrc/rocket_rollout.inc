// rocket_rollout.inc — one launch per PPO rollout step (rr_rollout_step; SURVEY.md §8f rank
// 2, BASELINE configs[4]): the SB3 MlpPolicy forward + Gaussian sample of rocket_policy.inc
// and the env step of step_kernel fused, so the action never leaves registers, the policy
// input is formed from the state planes already loaded for the step, and the timeout
// bootstrap reads the terminal observation from registers.
//
// It computes exactly what the two-launch sequence rr_policy_act + rr_step computes (same
// tower code, same noise key, same physics / reward / reset code, same fp32 expressions):
// tests/test_gpu_rollout.py requires the two rollouts to be bitwise equal.
//   policy input  obs = state * inv_norm (bitwise the obs buffer rr_reset / rr_step write)
//   action        a ~ N(mean, exp(log_std)) keyed on (seed, env id, *iter, t); env gets clip(a)
//   reward_t      r + gamma * V(terminal obs) where TimeLimit-truncated (SB3 1.6)
//   start_t       the done flag of the previous step (io.done before this step writes it)
// Layout: lane = env, 64 envs per wave = two 32-env MFMA column tiles; the wave's obs rows
// pass through an LDS tile [64][NS] for the coalesced buffer store, the layer-1 MFMA B operands
// are formed in registers (regs_x: one v_permlane32_swap per k pair); the packed policy
// (rr_policy_pack) and the auto-reset parameters are staged per workgroup.
//
// rr_rollout_collect (MULTI = true) runs all T steps of a rollout in ONE launch: every env's
// trajectory is independent, so a lane loops policy -> sample -> step over t = 0..T-1 with its
// state in registers (loaded and stored once per rollout, the policy staged once), writes the
// [T][n] buffer slices of every step, and ends with V(last obs), the last-done flags and the
// env's GAE scan (the code of rr_policy_bootstrap and rr_gae). Bitwise the same rollout as T
// rr_rollout_step launches + rr_policy_bootstrap + rr_gae (tests/test_gpu_rollout.py).

#pragma once

#include <type_traits>

#include "rocket_device.h"
#include "rocket_policy.inc"

namespace {

struct RolloutIO {
    const float* params;        // packed policy (rr_policy_layout / rr_policy_pack), 16-B aligned
    const uint64_t* iter;       // device rollout counter (noise key)
    float* buf_obs;             // [n][NS]   obs of step t (policy input)
    float* buf_act;             // [n][NA]   unclipped sample
    float* buf_val;             // [n]       V(obs)
    float* buf_logp;            // [n]
    float* buf_start;           // [n]       episode-start flag of step t
    float* buf_rew;             // [n]       reward with the timeout bootstrap
    float* obs;                 // [n][NS]   post-step obs (env output) or nullptr
    float* reward;              // [n]       raw env reward (env output)
    uint8_t* done;              // [n]       in: previous done flags; out: this step's
    uint8_t* truncated;         // [n] or nullptr
    float* terms;               // [NT + 2][n] or nullptr
    uint32_t seed_lo, seed_hi, t;
    float gamma;
    int32_t obs_vec_ok, buf_obs_vec_ok;
    // rr_rollout_collect only (MULTI): steps per launch and the end-of-rollout outputs
    uint32_t T;
    double gamma64, lam;        // GAE coefficients (the scan runs in fp64; gamma above is the bootstrap's)
    float* buf_adv;             // [T][n] or nullptr (no GAE)
    float* buf_ret;             // [T][n]
    float* last_value;          // [n] V(obs after the last step) or nullptr
    float* last_done;           // [n] float(done of the last step) or nullptr
    float* last_start;          // [n] same values (SB3 _last_episode_starts) or nullptr
};
static_assert(std::is_trivially_copyable_v<RolloutIO>, "RolloutIO crosses TUs by memcpy (rrc_launch_collect)");

namespace rol {
// NTW 32-env MFMA column tiles per wave: 2 = 64 envs per wave, 4 waves per workgroup (the
// default); 1 = 32 envs per wave (lanes 32..63 mirror lanes 0..31 and store nothing), 8 waves
// per workgroup, so two waves share a SIMD and one's MFMA chain can overlap the other's VALU
// work (measured slower: the env step's VALU work doubles). Either way 256 envs per workgroup.
template <int NTW> struct Shape {
    static constexpr int kEPW = 32 * NTW;
    static constexpr int kWaves = NTW == 2 ? 4 : 8;
    static constexpr int kThreads = kWaves * kWave;
};
constexpr int kEnvsPerBlock = 256;

// What the auto-reset draw reads (KParams' seed_w, ic_low, ic_span), staged into LDS at kernel
// start. Read from the device copy (B.kp) inside the step loop, they cost the done lanes' waves
// three dependent global round trips per step, the first also waiting (vmcnt) for the step's
// terminal-row stores to complete.
template <int NS> struct ResetParams {
    uint32_t seed_w[4];
    float ic_low[NS], ic_span[NS];
};
template <int NS>
__device__ __forceinline__ void stage_reset(const KParams* __restrict__ kp, ResetParams<NS>* rp)
{
    // thread t copies word t of ResetParams from its KParams field: one load per thread (three
    // divergent branches each waited out their own load)
    const uint32_t t = threadIdx.x;
    if (t < 4 + 2 * NS) {
        const uint32_t* src = t < 4 ? &kp->seed_w[t] : t < 4 + NS ? reinterpret_cast<const uint32_t*>(&kp->ic_low[t - 4])
                                                                  : reinterpret_cast<const uint32_t*>(&kp->ic_span[t - 4 - NS]);
        reinterpret_cast<uint32_t*>(rp)[t] = *src;
    }
}

// this wave's rows o[NS] into its LDS tile (the wave's previous readers of the tile are done)
template <int NS, int NTW>
__device__ __forceinline__ void put_rows(float* tile, const float* o, uint32_t lane)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < (uint32_t)Shape<NTW>::kEPW) {
#pragma unroll
        for (int j = 0; j < NS; ++j) tile[lane * NS + j] = o[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// V of the wave's tile rows, for the env of this lane
template <int NS, int NA, int PREC, int NTW>
__device__ __forceinline__ float tile_value(const float* sp, const float* tile, uint32_t lane)
{
    using L = pol::Layout<NS, NA, PREC>;
    typename pol::XOp<PREC>::T x[NTW][L::KP1];
    pol::load_x<NS, NA, PREC, NTW>(tile, lane, x);
    f32x16 h2[2][NTW];
    pol::tower<NS, NA, PREC, NTW>(sp + L::VF, x, lane, h2);
    const int half = lane >> 5;
    const float v0 = pol::head_dot<NTW>(sp + L::HV, h2, 0, half) + sp[L::VB];
    if constexpr (NTW == 1) return v0;
    const float v1 = pol::head_dot<NTW>(sp + L::HV, h2, NTW - 1, half) + sp[L::VB];
    return half ? v1 : v0;
}

// store_obs_tile in two halves, so the buffer stores of the step's obs rows can go out under the
// first tower's layer-1 MFMAs: obs_begin writes the rows into the wave's LDS tile and reads the tile
// back as 16-B lane-contiguous pieces (or, for a ragged / unaligned tile, stores it at once);
// obs_end issues the 16-B buffer stores of those pieces.
template <int NS, int EPW>
struct ObsRead {
    static constexpr int NV = EPW * NS / 4, NQ = (NV + kWave - 1) / kWave;
    u32x4 v[NQ];
    bool vec;
};
template <int NS, int EPW>
__device__ __forceinline__ void obs_begin(float* lds, const float* o, rsrc_t obs_r, uint32_t wave_base, int lane,
                                          uint32_t nvalid, bool vec_ok, ObsRead<NS, EPW>& r)
{
    if (lane >= EPW) {
    } else if constexpr (NS % 2 == 0) {
        float2* l2 = reinterpret_cast<float2*>(lds + lane * NS);
#pragma unroll
        for (int j = 0; j < NS / 2; ++j) l2[j] = make_float2(o[2 * j], o[2 * j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < NS; ++j) lds[lane * NS + j] = o[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    r.vec = vec_ok && nvalid == (uint32_t)EPW;
    if (r.vec) {
        const u32x4* src4 = reinterpret_cast<const u32x4*>(lds);
#pragma unroll
        for (int q = 0; q < ObsRead<NS, EPW>::NQ; ++q) {
            const int k = lane + q * kWave;
            if (ObsRead<NS, EPW>::NV % kWave == 0 || k < ObsRead<NS, EPW>::NV) r.v[q] = src4[k];
        }
    } else {
        const uint32_t sbase = wave_base * NS * 4u;
        const int tot = (int)nvalid * NS;
        for (int k = lane; k < tot; k += kWave) bst_f<kOutAux>(obs_r, lds[k], k * 4u, sbase);
    }
}
template <int NS, int EPW>
__device__ __forceinline__ void obs_end(const ObsRead<NS, EPW>& r, rsrc_t obs_r, uint32_t wave_base, int lane)
{
    if (!r.vec) return;
    const uint32_t sbase = wave_base * NS * 4u;
#pragma unroll
    for (int q = 0; q < ObsRead<NS, EPW>::NQ; ++q) {
        const int k = lane + q * kWave;
        if (ObsRead<NS, EPW>::NV % kWave == 0 || k < ObsRead<NS, EPW>::NV)
            __builtin_amdgcn_raw_buffer_store_b128(r.v[q], obs_r, (int)(k * 16u), (int)sbase, kOutAux);
    }
}

// The layer-1 B operands of the wave's two env tiles (NTW 2) from this lane's obs registers, no LDS:
// x[n][s] of lane l holds obs[env 32n + (l&31)][k] with k = 2s + (l>>5) (fp32) or 16s + 8(l>>5) + j
// (element j, bf16 / split fp16), so one v_permlane32_swap of the pair (obs[k0], obs[k1]) gives
// both tiles' operand: lanes 0-31 keep their own k0 and receive the partner's (lane + 32) k0 for
// tile 1, lanes 32-63 keep their own k1 and receive the partner's (lane - 32) k1 for tile 0.
// Bitwise the values pol::load_x reads back from the obs tile.
template <int NS, int NA, int PREC>
__device__ __forceinline__ void regs_x(const float* o, typename pol::XOp<PREC>::T (&x)[2][pol::Layout<NS, NA, PREC>::KP1])
{
    constexpr int KP1 = pol::Layout<NS, NA, PREC>::KP1;
    auto swap = [](float a, float b, float& t0, float& t1) {
        const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b),
                                                        false, false);
        t0 = __builtin_bit_cast(float, (uint32_t)r[0]);
        t1 = __builtin_bit_cast(float, (uint32_t)r[1]);
    };
#pragma unroll
    for (int s = 0; s < KP1; ++s) {
        if constexpr (PREC == 0) {
            swap(o[2 * s], 2 * s + 1 < NS ? o[2 * s + 1] : 0.0f, x[0][s], x[1][s]);
        } else {
            float v0[8], v1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k0 = 16 * s + j, k1 = 16 * s + 8 + j;
                swap(k0 < NS ? o[k0] : 0.0f, k1 < NS ? o[k1] : 0.0f, v0[j], v1[j]);
            }
            if constexpr (PREC == 2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v0[j] = pol::f16_operand(v0[j]);  // saturated as in pol::load_x
                    v1[j] = pol::f16_operand(v1[j]);
                }
                pol::split_f16(v0, x[0][s]);
                pol::split_f16(v1, x[1][s]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    x[0][s][j] = (__bf16)v0[j];
                    x[1][s][j] = (__bf16)v1[j];
                }
            }
        }
    }
}

// Both towers and their heads for the wave's envs (value, action means of this lane's env); stamp(p)
// is called at the stage boundaries p = 1..8 (1: after the value tower's layer-1 MFMAs). In the
// collect TU (kPolPrefetchA) each tower's head weights are read from LDS before its last tanh stage,
// so their latency runs under that stage's transcendentals instead of stalling the head's FMA chain
// at every read; the main TU's per-step kernels read them where used (the ~128 registers of early
// head weights would cost them their second wave per SIMD).
// VALUE = false (rr_policy_evaluate, rocket_eval.inc) runs the pi tower and the action heads only:
// `value` is then 0 and the stages p = 1..4 are not stamped.
struct NoStamp {
    __device__ __forceinline__ void operator()(int) const {}
};
template <int NS, int NA, int PREC, int NTW, bool VALUE = true, class ST = NoStamp>
__device__ __forceinline__ void policy_forward(const float* sp,
                                               const typename pol::XOp<PREC>::T (&x)[NTW][pol::Layout<NS, NA, PREC>::KP1],
                                               uint32_t lane, float& value, float (&mean)[NA], ST stamp = ST())
{
    using L = pol::Layout<NS, NA, PREC>;
    constexpr bool FOLD = PREC == 0 && kPolFoldTanh;
    const int half = lane >> 5;
    if constexpr (!kPolPrefetchA) {
        f32x16 h2[2][NTW];
        value = 0.0f;
        if constexpr (VALUE) {
            pol::tower<NS, NA, PREC, NTW>(sp + L::VF, x, lane, h2);
            stamp(1);
            const float va = pol::head_dot<NTW>(sp + L::HV, h2, 0, half) + sp[L::VB];
            const float vb = pol::head_dot<NTW>(sp + L::HV, h2, NTW - 1, half) + sp[L::VB];
            value = (NTW == 2 && half) ? vb : va;
        }
        pol::tower<NS, NA, PREC, NTW>(sp + L::PI, x, lane, h2);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const float ma = pol::head_dot<NTW>(sp + L::HA + a * 64, h2, 0, half) + sp[L::HB + a];
            const float mb = pol::head_dot<NTW>(sp + L::HA + a * 64, h2, NTW - 1, half) + sp[L::HB + a];
            mean[a] = (NTW == 2 && half) ? mb : ma;
        }
        return;
    }
    f32x16 h1[2][NTW], h2[2][NTW];
    value = 0.0f;
    if constexpr (VALUE) {
        pol::tower_l1<NS, NA, PREC, NTW>(sp + L::VF, x, lane, h1);
        stamp(1);
        pol::tower_act1<PREC, NTW, FOLD>(h1);
        stamp(2);
        pol::tower_l2<NS, NA, PREC, NTW>(sp + L::VF, h1, lane, h2);
        stamp(3);
        const pol::HeadW wv = pol::load_head(sp + L::HV, half);
        __builtin_amdgcn_sched_barrier(0);
        pol::tower_act2<PREC, NTW, FOLD>(h2);
        const float va = pol::head_dot_w<NTW>(wv, h2, 0) + sp[L::VB];
        const float vb = pol::head_dot_w<NTW>(wv, h2, NTW - 1) + sp[L::VB];
        value = (NTW == 2 && half) ? vb : va;
        stamp(4);
    }
    pol::tower_l1<NS, NA, PREC, NTW>(sp + L::PI, x, lane, h1);
    stamp(5);
    pol::tower_act1<PREC, NTW, FOLD>(h1);
    stamp(6);
    pol::tower_l2<NS, NA, PREC, NTW>(sp + L::PI, h1, lane, h2);
    stamp(7);
    pol::HeadW wa[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) wa[a] = pol::load_head(sp + L::HA + a * 64, half);
    __builtin_amdgcn_sched_barrier(0);
    pol::tower_act2<PREC, NTW, FOLD>(h2);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const float ma = pol::head_dot_w<NTW>(wa[a], h2, 0) + sp[L::HB + a];
        const float mb = pol::head_dot_w<NTW>(wa[a], h2, NTW - 1) + sp[L::HB + a];
        mean[a] = (NTW == 2 && half) ? mb : ma;
    }
    stamp(8);
}

}  // namespace rol

// Diagnostic builds only (RR_DIAG_STAMPS, rocket_stamps.h, tools/collect_stamps.py): per-wave
// s_memtime cycles of each phase of the collect, summed over the steps (RR_ST), written over
// io.last_value[wave's first 16 envs] at the end. Never in the shipped library.
//
// The kernel's body is rocket_rollout_body.inc, included as text: rollout_collect_stats_kernel
// (collect_stats/rocket_collect_stats.inc) is the same body with its accounting regions.

template <int MODEL, int INTEG, int PREC, bool MULTI, int NTW>
__global__ __launch_bounds__(rol::Shape<NTW>::kThreads) void rollout_step_kernel(
    float* __restrict__ state, uint32_t n_envs, uint32_t mode, const KParams P, const Bufs B, const RolloutIO io)
{
#define RR_COLLECT_STATS 0
#include "rocket_rollout_body.inc"
#undef RR_COLLECT_STATS
}

}  // namespace
