// rocket_hip.hip — MI355X (gfx950) kernels and C-ABI for the vectorized rocket env.
//
// One lane = one env. The per-env state lives in HBM as fp32 struct-of-arrays
// planes ([state_dim][N]); one launch of step_kernel does, for every env:
//   action denormalisation   (rocket_env.py:969-981 / :395-406)
//   RK4 integration of the rigid-body ODE over dt with the terminal ground event
//                            (simulator.py:227-294 / :55-130; the reference uses
//                             scipy RK45 + brentq on its dense output)
//   quaternion renormalisation / theta wrap (simulator.py:250 / :77)
//   bounds check, reward shaping, landing check, obs normalisation
//                            (rocket_env.py:690-719, 825-859, 963-1061 / :150-247, 431-476)
//   TimeLimit, auto-reset with an in-kernel RNG, done compaction by wave ballot
// with state kept in registers, the [N][state_dim] observation tile staged through
// LDS so that it leaves the CU as 16-byte coalesced stores.
//
// Element-wise ODE work: no contraction, so no MFMA. The roofline is HBM bytes
// (189 B per 6DOF env-step, 101 B per 3DOF env-step).

// This file is the main translation unit of librocket_hip.so: step_kernel, reset_kernel and the
// small kernels of the C-ABI's helpers, the per-step rollout and policy kernels (instantiated from
// rocket_policy.inc / rocket_rollout.inc), and the host side. The device code it shares with the
// other two (rocket_exact.hip: the exact-mode kernels; rocket_collect.hip: the rollout collect and
// PPO learner kernels) is rocket_device.h. It also builds into a loadable library on its own
// (the tools/ A/B variants): see the weak stand-ins below.

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rocket_device.h"
// On-device PPO rollout kernels (fused MlpPolicy forward on fp32 MFMA, bootstrap, GAE). One A
// fragment set in this translation unit (see rocket_policy.inc)
#define RR_POL_PREFETCH_A 0
#include "rocket_policy.inc"
#include "rocket_rollout.inc"
#include "rocket_eval.inc"
// PPO learner (loss + backward of the MlpPolicy on fp32 MFMA, clip + Adam): its types here, its
// kernels compiled in and launched from the collect TU (rrc_launch_learner)
#include "rocket_ppo.inc"

namespace {

// The workgroup barrier of the helper-wave kernels' entry. It orders LDS only (the flag clear before
// the helpers' publish): unlike __syncthreads() it carries no fence over global memory, so the
// loads issued before it stay in flight across it.
__device__ __forceinline__ void entry_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The step kernel: one env per lane, 64 envs per wave.
// HELP (N <= kHelpMaxN, about one main wave per SIMD): the auto-reset candidates of main
// wave k are drawn by helper wave WPB + k of the same workgroup (on the same SIMD) into
// cand[k] (row per lane: NS values, v0), published by cflag[k]. A lone wave issues one VALU op
// per 4 cycles and its SIMD can take one per 2 (MI355X_MICROARCH.md, 'vector-instruction ISSUE
// cost'), so the helper's ~190 instructions run beside the main wave's instead of before them
// (they need the counter word, which arrives with the state planes). Without HELP the main
// wave draws the candidate itself right after its counter word lands. Measured and rejected
// (round 2): a helper that also computes reward, obs and every caller-owned output while the
// main wave resets and stores the state (bitwise equal, 4.69 vs 4.31 us per step at N = 65536).
// ROWS (rr_step_rows): obs, reward and done leave as ONE row of NS + 2 fp32 per env
// (obs[NS], reward, done as 0 / 1) through the same LDS tile, e.g. straight into the send
// buffer of the multi-GPU all-gather (rl_rocket_amd.dist.ShardGather).
template <int MODEL, int INTEG, bool ASOA, bool HELP, int WPB, bool ROWS>
// amdgpu_waves_per_eu(4): <= 128 VGPRs keeps 4 waves per SIMD at large N
__global__ __launch_bounds__(HELP ? 2 * WPB * kWave : WPB * kWave) __attribute__((amdgpu_waves_per_eu(4))) void step_kernel(
    float* __restrict__ state, const float* __restrict__ action, uint32_t n_envs, uint32_t mode, const KParams P,
    const Bufs B, const StepIO io)
{
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT, EV = Dims<MODEL>::EV;
    constexpr int OW = ROWS ? NS + 2 : NS;  // floats per output row
    __shared__ __attribute__((aligned(16))) float lds[WPB][kWave * OW];
    constexpr int kCandRow = (NS + 1 + 3) / 4 * 4;
    __shared__ __attribute__((aligned(16))) float cand[HELP ? WPB : 1][HELP ? kWave * kCandRow : 1];
    __shared__ uint32_t cflag[WPB];
    const uint32_t lane = threadIdx.x & (kWave - 1);
    // wave index as an SGPR: derived from threadIdx it is a VGPR the compiler cannot prove
    // uniform, and every buffer store with a wave_base soffset became a waterfall loop
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t n = n_envs;
    RR_STAMPS_BEGIN(4);  // diagnostic builds only (rocket_stamps.h)
    RR_SUB_BEGIN(3);     // the done tail, in cycles after stamp 2: terminal rows issued, flag seen, candidate landed
    if constexpr (HELP) {
        if (wv >= (uint32_t)WPB) {
            // the helper role reads its parameters through the device copy (B.kp): kernel-argument
            // values it used were loaded in the kernel's entry block and kept live into the main
            // role, where SGPRs are the scarce resource
            const KParams& P = *B.kp;
            const uint32_t k = wv - WPB;  // the main wave this helper serves
            const uint32_t base = (blockIdx.x * WPB + k) * kWave;
            const uint32_t ih = min(base + lane, n - 1);
            // the counter word is in flight across the barrier (see the main role below)
            const uint32_t cwh = (base < n && (mode & kModeCounter)) ? at(B.counter, ih) : 0u;
            entry_barrier();
            if ((mode & RR_FLAG_AUTO_RESET) && base < n) {
                float s_[NS], v_;
                ResetStream key = reset_stream(P.seed_w, P.id_off + base + lane, cwh);
                sample_ic<MODEL>(P, key, s_, v_);
                float* row = &cand[k][lane * kCandRow];
#pragma unroll
                for (int j = 0; j < NS; ++j) row[j] = s_[j];
                row[NS] = v_;
            }
            __hip_atomic_store(&cflag[k], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            return;
        }
    }
    const uint32_t wave_idx = blockIdx.x * WPB + wv;
    const uint32_t wave_base = wave_idx * kWave;
    if constexpr (!HELP) {
        if (wave_base >= n) return;  // wave-uniform
        RR_STAMP(0);
    }
    const uint32_t i = wave_base + lane;
    const bool valid = i < n;
    const uint32_t ic = valid ? i : n - 1;
    const uint32_t vo = ic * 4u;           // per-lane byte offset in every fp32/u32 plane
    const uint32_t plane = n * 4u;         // bytes per plane
    const bool use_counter = mode & kModeCounter;
    // state planes, v0, counter and ep_ret are consecutive planes of ONE allocation
    // (rr_create), so a single descriptor (4 SGPRs) serves them all via soffset
    const rsrc_t st_r = make_rsrc(state, (uint64_t)(NS + 3) * plane);
    const uint32_t v0_off = NS * plane, cw_off = (NS + 1) * plane, ret_off = (NS + 2) * plane;
    constexpr int SA = HELP ? kStAuxHelp : kStAux;  // cache policy of the state-buffer stores

    // ---- all loads first (one memory round trip per wave); the counter word first, so the
    // reset candidate below is drawn while the state planes are still in flight ----
    uint32_t cw = use_counter ? bld_u(st_r, vo, cw_off) : 0u;
    float y0[NS], y1[NS], a[NA];
    load_action<NA, ASOA>(make_rsrc(action, (uint64_t)NA * plane), vo, plane, a);
#pragma unroll
    for (int j = 0; j < NS; ++j) y0[j] = bld_f(st_r, vo, j * plane);
    float v0 = bld_f(st_r, vo, v0_off);
    float ret = (mode & RR_FLAG_EPISODE_STATS) ? bld_f(st_r, vo, ret_off) : 0.0f;
    const HotParams H = load_hot<NS>(P);  // scalar loads overlap the HBM latency above
    const CounterLayout CL(P);
    // the kernel-argument lines holding the tail's pointers (outputs, terminal rows) are read
    // here, in the load shadow, so that the scalar reloads after the integration hit the
    // scalar cache instead of missing in the wave's critical tail (HELP kernels: without the
    // helpers' device parameter copy the SGPRs are short, 2-5 spills)
    if constexpr (HELP)
        asm volatile("" ::"s"(io.obs), "s"(io.reward), "s"(io.done), "s"(io.truncated), "s"(B.done_bits),
                     "s"(B.term_obs));
    // the SGPR -> VGPR copies of the pinned per-axis parameters issue here, in the shadow of
    // the state loads; left to the scheduler they landed after the load wait, inside the RK4
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HELP) {
        // HELP: the flag clear and the workgroup barrier (no helper may publish before the flag is
        // cleared) come after every load of this wave has been issued: the barrier waits until all
        // 2 * WPB waves of the workgroup have been dispatched, and that wait now passes inside the
        // load round trip instead of in front of it. The early exit stays behind the barrier, so
        // that every wave reaches it; an empty wave's loads above read env n - 1 (ic), in bounds.
        if (lane == 0) cflag[wv] = 0u;
        entry_barrier();
        if (wave_base >= n) return;  // wave-uniform
        RR_STAMP(0);
    }
    // SB3 auto-reset candidate of this step, keyed on (gid, counter word): ~190 VALU right
    // after the counter word lands, instead of in the done branch of the waves that finish
    // last. Used by done lanes only. (HELP: drawn by the helper wave instead.)
    float ic_s[NS], ic_v0 = 0.0f;
    if (!HELP && (mode & RR_FLAG_AUTO_RESET)) {
        ResetStream key = reset_stream(B.kp->seed_w, P.id_off + i, cw);
        sample_ic<MODEL>(P, key, ic_s, ic_v0);
    }

    RR_STAMP_AFTER(1, y0, NS);  // the state landed
    const bool event = physics_step<MODEL, INTEG>(P, a, y0, y1);
    const bool nf = nonfinite<NS>(y1);
    bool bv;
    float t[NT];
    const float r = reward_terms<MODEL>(H, y1, a, v0, bv, t);
    bool done = event || bv || nf, trunc;
    int32_t el = CL.time_limit(cw, done, trunc);
    ret += r;
    float o[NS];
    normalize_obs<NS>(y1, H.inv_norm, o);
    RR_STAMP(2);

    // Done compaction: one ballot per wave; lane 0 stores the wave's 64-bit done mask
    // (every wave writes its word each step, so no clearing and no atomics; the host
    // side expands the masks into the sorted index list, rr_fetch_done).
    const bool dv = done && valid;
    const uint64_t m = __ballot(dv);
    if (lane == 0) {
        // HELP: write-through like every other store of these kernels (kStAuxHelp): a 128-B line of
        // done words is written by waves of four XCDs, and left dirty in their L2s it is what the
        // end-of-kernel release has to find and write back even when no env is done
        if constexpr (HELP) __hip_atomic_store(&B.done_bits[wave_idx], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else B.done_bits[wave_idx] = m;
    }
    if (m) {
        // plain kernels past the MALL: the 4-B terminal return / length and the reset v0 leave as
        // whole lines, from every lane of a wave with a done lane (the others' values are not
        // read: terminal rows count at done indices only; their v0 is unchanged)
        if (dv) store_terminal<NS, HELP ? kStAuxHelp : kTermAuxLarge, HELP>(B, i, vo, plane, o, ret, el);
        RR_SUB_STAMP(0, 2);
        if constexpr (!HELP) {
            if ((mode & kModeWholeLines) ? valid : dv) {
                bst_f<0>(make_rsrc(B.term_ret, plane), ret, vo, 0);
                bst_u<0>(make_rsrc(B.term_len, plane), (uint32_t)el, vo, 0);
            }
        }
        if ((mode & RR_FLAG_AUTO_RESET) && dv) {
            if constexpr (HELP) {
                while (__hip_atomic_load(&cflag[wv], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u)
                    __builtin_amdgcn_s_sleep(1);
                RR_SUB_STAMP(1, 2);
                const float* row = &cand[wv][lane * kCandRow];
#pragma unroll
                for (int j = 0; j < NS; ++j) y1[j] = row[j];
                v0 = row[NS];
                RR_SUB_STAMP_AFTER(2, 2, y1, NS);
            } else {
#pragma unroll
                for (int j = 0; j < NS; ++j) y1[j] = ic_s[j];
                v0 = ic_v0;
            }
            if (HELP || !(mode & kModeWholeLines)) bst_f<SA>(st_r, v0, vo, v0_off);
            cw = CL.next_episode(cw);
            normalize_obs<NS>(y1, H.inv_norm, o);
            el = 0;
            ret = 0.0f;
        }
        if constexpr (!HELP) {
            if ((mode & kModeWholeLines) && (mode & RR_FLAG_AUTO_RESET) && valid) bst_f<SA>(st_r, v0, vo, v0_off);
        }
    }
    cw = CL.with_elapsed(cw, el);

    // HELP: the tail tests the mode word itself: `use_counter` kept from the entry as a lane mask
    // was live across the whole kernel and spilled (2 SGPRs) once the entry barrier moved
    uint32_t mode_t = mode;
    if constexpr (HELP) pin_s(mode_t);
    if (valid) {
#pragma unroll
        for (int j = 0; j < NS; ++j) bst_f<SA>(st_r, y1[j], vo, j * plane);
        if (HELP ? (mode_t & kModeCounter) != 0u : use_counter) bst_u<SA>(st_r, cw, vo, (NS + 1) * plane);
        if (mode & RR_FLAG_EPISODE_STATS) bst_f<SA>(st_r, ret, vo, (NS + 2) * plane);
        store_outputs<NT, !ROWS>(io, i, vo, plane, n, r, done, trunc, t, bv, event ? 1.0f : (nf ? -1.0f : 0.0f));
    }
    const uint32_t nvalid = (n - wave_base) < (uint32_t)kWave ? (n - wave_base) : (uint32_t)kWave;
    if constexpr (ROWS) {
        float ow[OW];
#pragma unroll
        for (int j = 0; j < NS; ++j) ow[j] = o[j];
        ow[NS] = r;
        ow[NS + 1] = done ? 1.0f : 0.0f;
        store_obs_tile<OW, kWave>(lds[wv], ow, make_rsrc(io.obs, (uint64_t)OW * plane), wave_base, lane, nvalid,
                                  io.obs_vec_ok);
    } else {
        store_obs_tile<NS, kWave>(lds[wv], o, make_rsrc(io.obs, (uint64_t)NS * plane), wave_base, lane, nvalid,
                                  io.obs_vec_ok);
    }
    // lanes 0..2: barrier / loads / compute cycles; 3: the tail (outputs issued); 4, 5: the wave's
    // s_memrealtime start / end (100 MHz, low 32 bits, bit patterns in the float slots); 6-8: the
    // done tail's sub-stamps (tools/step_stamps_steady.py)
    RR_STAMP(3);
    RR_STAMPS_WRITE(io.reward, i, lane, valid, true);
    RR_SUB_WRITE(io.reward, i, lane, valid, 6);
}

template <int MODEL>
__global__ __launch_bounds__(kBlock) void reset_kernel(const KParams P, const Bufs B, const uint8_t* mask,
                                                      float* obs, double* state64)
{
    constexpr int NS = Dims<MODEL>::NS;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B.n) return;
    const int64_t n = B.n;
    float s[NS], v0;
    if (mask == nullptr || mask[i]) {
        const uint32_t ep = (B.counter[i] >> P.ep_shift) + 1u;
        ResetStream key = reset_stream(B.kp->seed_w, P.id_off + i, B.counter[i]);
        sample_ic<MODEL>(P, key, s, v0);
#pragma unroll
        for (int j = 0; j < NS; ++j) B.state[(int64_t)j * n + i] = s[j];
        if (state64) {  // RR_INT_DOPRI5
#pragma unroll
            for (int j = 0; j < NS; ++j) state64[(int64_t)j * n + i] = (double)s[j];
        }
        B.v0[i] = v0;
        B.counter[i] = ep << P.ep_shift;
        B.ep_ret[i] = 0.0f;
    } else {
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j] = B.state[(int64_t)j * n + i];
    }
    if (obs) {
#pragma unroll
        for (int j = 0; j < NS; ++j) obs[i * NS + j] = s[j] * P.inv_norm[j];
    }
}

// counter words: clear the elapsed field, keep the episode field (rr_set_state without elapsed)
__global__ __launch_bounds__(kBlock) void clear_elapsed_kernel(uint32_t* counter, int64_t n, uint32_t el_mask)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) counter[i] &= ~el_mask;
}

// Compact the terminal rows of the (sorted) done list for one host copy.
__global__ __launch_bounds__(kBlock) void gather_done_kernel(const int32_t* idx, int64_t count, int ns,
                                                             const float* term_obs, const float* term_ret,
                                                             const int32_t* term_len, const uint8_t* trunc,
                                                             float* g_obs, float* g_ret, int32_t* g_len,
                                                             uint8_t* g_trunc)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const int64_t i = idx[k];
    for (int j = 0; j < ns; ++j) g_obs[k * ns + j] = term_obs[i * ns + j];
    g_ret[k] = term_ret[i];
    g_len[k] = term_len[i];
    if (trunc) g_trunc[k] = trunc[i];
}

// rr_copy_terminal: the terminal rows of the envs done at the last step (done_bits) into
// caller buffers (any may be null); rows of other envs are left untouched
__global__ __launch_bounds__(kBlock) void copy_done_rows_kernel(const uint64_t* done_bits, int64_t n, int ns,
                                                                const float* term_obs, const float* term_ret,
                                                                const int32_t* term_len, float* d_obs, float* d_ret,
                                                                int32_t* d_len)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !((done_bits[i / kWave] >> (i % kWave)) & 1ull)) return;
    if (d_obs)
        for (int j = 0; j < ns; ++j) d_obs[i * ns + j] = term_obs[i * ns + j];
    if (d_ret) d_ret[i] = term_ret[i];
    if (d_len) d_len[i] = term_len[i];
}

// SB3 RolloutBuffer.compute_returns_and_advantage on device: one thread per env scans t
// backwards. rewards/values/starts [T][n]; starts[t] = episode start flag of step t.
__global__ __launch_bounds__(kBlock) void gae_kernel(int64_t T, int64_t n, const float* __restrict__ rewards,
                                                     const float* __restrict__ values,
                                                     const float* __restrict__ starts,
                                                     const float* __restrict__ last_value,
                                                     const float* __restrict__ last_done, double gamma, double lam,
                                                     float* __restrict__ adv, float* __restrict__ ret)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    pol::gae_env(T, n, e, rewards, values, starts, last_value[e], last_done[e], gamma, lam, adv, ret);
}

// fp32 <-> fp64 state planes (rr_set_state / rr_set_state64 / rr_get_state64)
__global__ __launch_bounds__(kBlock) void widen_kernel(const float* src, double* dst, int64_t count)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < count) dst[k] = (double)src[k];
}

__global__ __launch_bounds__(kBlock) void narrow_kernel(const double* src, float* dst, int64_t count)
{
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < count) dst[k] = (float)src[k];
}

}  // namespace

// defined by the exact / collect / recording translation units (declared hidden in rocket_device.h);
// these weak stand-ins (a library built from this file alone, e.g. a tools/ A/B variant) make
// RR_INT_DOPRI5 steps, rr_rollout_collect(_stats), rr_policy_evaluate(_trace / _exact) and the learner fail loudly
// instead of failing to load
constexpr int kNoUnit = (int)hipErrorInvalidDeviceFunction;
extern "C" {
__attribute__((weak)) int rrx_launch_exact(const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrx_launch_eval_exact(const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrx_launch_eval_exact_trace(const void*, const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrx_launch_eval_exact_discrete(const void*, const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_collect(const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_eval(const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_eval_trace(const void*, const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_collect_stats(const void*, const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_learner(const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_learner_opts(const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_bc(const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_discrete(const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_bc_discrete(const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_a2c(const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_a2c_discrete(const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_rollout_discrete(const void*, const void*, const void*, int) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_eval_discrete(const void*, const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_discrete_opts(const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_collect_discrete_stats(const void*, const void*, const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_eval_discrete_trace(const void*, const void*, const void*, const void*, void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_eval_sampled(const void*, const void*, const void*, const void*) { return kNoUnit; }
__attribute__((weak)) int rrc_launch_eval_discrete_sampled(const void*, const void*, const void*, const void*, const void*, void*) { return kNoUnit; }
}

namespace {

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what)
{
    return fail(RR_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// What entry points with a twin share. `who` names the entry point in the error text, built only on a refusal.
int refuse(const char* who, const std::string& what) { return fail(RR_EINVAL, std::string(who) + ": " + what); }

float ceil_f(double d)   // smallest float >= d
{
    float f = (float)d;
    if ((double)f < d) f = std::nextafter(f, INFINITY);
    return f;
}
float floor_f(double d)  // largest float <= d
{
    float f = (float)d;
    if ((double)f > d) f = std::nextafter(f, -INFINITY);
    return f;
}

// one splitmix64 step (host side): the user seed never reaches a kernel's key unmixed
uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// 64-bit user seed -> the reset stream's four key words (splitmix64, host side)
void seed_words(uint64_t seed, uint32_t* w)
{
    const auto sm = splitmix64;
    const uint64_t a = sm(seed), b = sm(seed + 0x9E3779B97F4A7C15ull);
    w[0] = (uint32_t)a;
    w[1] = (uint32_t)(a >> 32);
    w[2] = (uint32_t)b;
    w[3] = (uint32_t)(b >> 32);
}

// bits of the elapsed field of the counter word: enough for max_episode_steps (TimeLimit
// 800 -> 10), 16 without a TimeLimit (elapsed then only counts Monitor's episode length)
int counter_bits(int32_t max_episode_steps)
{
    if (max_episode_steps <= 0) return 16;
    int b = 1;
    while (((int64_t)1 << b) <= (int64_t)max_episode_steps) ++b;
    return b;
}

KParams make_kparams(const rr_params& p)
{
    KParams k;
    std::memset(&k, 0, sizeof(k));
    const int ns = p.model == RR_MODEL_6DOF ? 14 : 7;
    k.max_steps = p.max_episode_steps;
    k.flags = p.flags;
    const int eb = counter_bits(p.max_episode_steps);
    k.el_mask = (1u << eb) - 1u;
    k.ep_shift = (uint32_t)eb;
    k.h = (float)p.dt;
    k.h2 = 0.5f * k.h;
    k.h6 = k.h / 6.0f;
    for (int j = 0; j < ns; ++j) {
        k.ic_low[j] = p.ic_low[j];
        k.ic_span[j] = p.ic_high[j] - p.ic_low[j];
        k.inv_norm[j] = (float)(1.0 / p.normalizer[j]);
    }
    // fp32 thresholds equivalent to the reference's float64 comparisons of float32 values
    for (int j = 0; j < 3; ++j) {
        if (p.model == RR_MODEL_6DOF) {  // inside <=> lo <= x <= hi
            k.blo[j] = ceil_f(p.bounds_low[j]);
            k.bhi[j] = floor_f(p.bounds_high[j]);
        } else {                         // out <=> x <= lo | x >= hi
            k.blo[j] = floor_f(p.bounds_low[j]);
            k.bhi[j] = ceil_f(p.bounds_high[j]);
        }
    }
    k.max_gimbal = (float)p.max_gimbal;
    k.half_thrust = (float)(0.5 * p.max_thrust);
    k.alfa = (float)p.alfa;
    k.beta = (float)p.beta;
    k.eta = (float)p.eta;
    k.gamma = (float)p.gamma;
    k.delta = (float)p.delta;
    k.kappa = (float)p.kappa;
    k.xi = (float)p.xi;
    k.waypoint = (float)p.waypoint;
    k.land_r2 = (float)((double)p.landing_radius * p.landing_radius);
    k.land_v2 = (float)((double)p.max_velocity * p.max_velocity);
    const double pi = 3.14159265358979323846;
    for (int ax = 0; ax < 3; ++ax) {
        const double L = p.att_limit[ax], M = p.land_att_limit[ax];
        // limits outside the angle's range make a test constant: |e| > L always holds for L < 0
        // (threshold 2 on axes 0 / 2: X < 2r for every r > 0, since |X| <= r; -1 on axis 1: |S| > -1;
        // the one exception, r == 0 exactly — the pitch singularity — reads false), and |e| < M
        // never holds for M <= 0 (X > 2r and |S| < -1 are never true)
        if (ax == 1) {  // b = asin(R02) in [-pi/2, pi/2]
            if (L >= pi / 2) k.att_never |= 1u << ax;
            else k.att_c[ax] = L < 0 ? -1.0f : (float)std::sin(L);
            if (M > pi / 2) k.land_always |= 1u << ax;
            else k.land_c[ax] = M <= 0 ? -1.0f : (float)std::sin(M);
        } else {        // a, c = atan2(.) in [-pi, pi]
            if (L >= pi) k.att_never |= 1u << ax;
            else k.att_c[ax] = L < 0 ? 2.0f : (float)std::cos(L);
            if (M > pi) k.land_always |= 1u << ax;
            else k.land_c[ax] = M <= 0 ? 2.0f : (float)std::cos(M);
        }
    }
    k.omega_lt = ceil_f(p.omega_lim[0]);
    k.zero_h = floor_f(1e-3);
    seed_words(42, k.seed_w);
    k.id_off = 0;
    return k;
}

XParams make_xparams(const rr_params& p)
{
    XParams x;
    std::memset(&x, 0, sizeof(x));
    x.dt = p.dt;
    const double ms = std::rint(p.dt * 1000.0);
    x.dt_milli = (ms > 0 && std::fabs(p.dt * 1000.0 - ms) < 1e-6) ? ms : 0.0;
    for (int j = 0; j < RR_MAX_STATE; ++j) x.norm[j] = p.normalizer[j];
    for (int j = 0; j < 3; ++j) {
        x.lo[j] = p.bounds_low[j];
        x.hi[j] = p.bounds_high[j];
        x.att_limit[j] = p.att_limit[j];
        x.land_att_limit[j] = p.land_att_limit[j];
        x.omega_lim[j] = p.omega_lim[j];
    }
    x.max_gimbal = p.max_gimbal;
    x.max_thrust = p.max_thrust;
    x.alfa = p.alfa;
    x.beta = p.beta;
    x.eta = p.eta;
    x.gamma = p.gamma;
    x.delta = p.delta;
    x.kappa = p.kappa;
    x.xi = p.xi;
    x.waypoint = p.waypoint;
    x.landing_radius = p.landing_radius;
    x.max_velocity = p.max_velocity;
    x.clamp_h0 = (p.flags & RR_FLAG_SCIPY_H0_CLAMP) ? 1 : 0;
    {
        const double pi = 3.14159265358979323846;
        for (int ax = 0; ax < 3; ++ax) {  // as make_kparams' float thresholds, in fp64
            const double L = p.att_limit[ax], M = p.land_att_limit[ax];
            // constant tests: |e| > L for L < 0 always, |e| < M for M <= 0 never (finish6)
            if (L < 0) x.att_always |= 1u << ax;
            if (M <= 0) x.land_never |= 1u << ax;
            if (ax == 1) {
                if (L >= pi / 2) x.att_never |= 1u << ax;
                else x.att_c[ax] = std::sin(L);
                if (M > pi / 2) x.land_always |= 1u << ax;
                else x.land_c[ax] = std::sin(M);
            } else {
                if (L >= pi) x.att_never |= 1u << ax;
                else x.att_c[ax] = std::cos(L);
                if (M > pi) x.land_always |= 1u << ax;
                else x.land_c[ax] = std::cos(M);
            }
        }
    }
    return x;
}

}  // namespace

struct rr_env {
    int device;
    rr_params p;
    KParams kp;
    XParams xp;
    int ns, na, nt;
    int64_t n, id_off;
    uint64_t steps;
    int64_t help_max_n;       // largest N stepped with helper waves (kHelpMaxN, RR_HELP_MAX_N env override)
    int64_t exact_lean_min_n; // 6DOF exact mode: lean kernel above this N (CUs x 256, RR_EXACT_LEAN_MIN_N)
    int64_t whole_line_min_n; // plain step kernels: whole-line done-path stores above this N (kWholeLineMinN,
                              // RR_WHOLE_LINE_MIN_N)
    float* state;
    float* v0;
    uint32_t* counter;
    float* ep_ret;
    uint64_t* done_bits;
    float* term_obs;
    float* term_ret;
    int32_t* term_len;
    double* state64;    // RR_INT_DOPRI5 only
    bool host_state;    // RR_FLAG_HOST_STATE: `state` (+ v0, counter, ep_ret planes) is pinned host memory
    KParams* d_kp;      // device copy of kp (Bufs.kp)
    XParams* d_xp;      // device copy of xp (RR_INT_DOPRI5: step_exact_kernel reads it where it uses it)
    int32_t* g_idx;     // rr_fetch_done scratch
    float* g_obs;
    float* g_ret;
    int32_t* g_len;
    uint8_t* g_trunc;   // rr_gather_rows scratch
    // the streams the handle's key-reading launches (step, reset, rollout kernels) were queued on,
    // most recent last (stored handles, compared only): rr_seed makes its key copy wait for the work
    // queued on each of them (seed_ev), and for the whole device past kSeedStreams distinct streams
    static constexpr int kSeedStreams = 8;
    void* streams[kSeedStreams];
    int n_streams;
    bool streams_overflow;
    hipEvent_t seed_ev;
};

namespace {

// note that a launch reading the reset-stream key went to `stream` (rr_seed orders its key copy after
// the work queued on every stream noted): a pointer compare per launch, no HIP call
inline void note_stream(rr_env* e, void* stream)
{
    if (e->n_streams > 0 && e->streams[e->n_streams - 1] == stream) return;
    for (int k = 0; k < e->n_streams; ++k)
        if (e->streams[k] == stream) {
            for (int j = k; j + 1 < e->n_streams; ++j) e->streams[j] = e->streams[j + 1];
            e->streams[e->n_streams - 1] = stream;
            return;
        }
    if (e->n_streams < rr_env::kSeedStreams) e->streams[e->n_streams++] = stream;
    else e->streams_overflow = true;
}

Bufs bufs_of(const rr_env* e)
{
    Bufs b;
    b.state = e->state;
    b.v0 = e->v0;
    b.counter = e->counter;
    b.ep_ret = e->ep_ret;
    b.done_bits = e->done_bits;
    b.term_obs = e->term_obs;
    b.term_ret = e->term_ret;
    b.term_len = e->term_len;
    b.n = e->n;
    b.kp = e->d_kp;
    return b;
}

// the kernels' mode word: the handle's flags, and kModeCounter where it keeps counter words (a
// TimeLimit, episode statistics or the auto-reset's episode count)
uint32_t mode_of(const rr_env* e)
{
    const bool counter = e->p.max_episode_steps > 0 || (e->p.flags & (RR_FLAG_EPISODE_STATS | RR_FLAG_AUTO_RESET));
    return e->p.flags | (counter ? kModeCounter : 0u);
}

// the launch record of a rollout / evaluation kernel over the handle's envs (rol::kEnvsPerBlock per
// workgroup); `b` = bufs_of(e), alive until the launch call returns
EnvLaunch env_launch(const rr_env* e, int prec, const Bufs* b, void* stream)
{
    const unsigned grid = (unsigned)((e->n + rol::kEnvsPerBlock - 1) / rol::kEnvsPerBlock);
    return {e->p.model, e->p.integrator, prec, grid, e->state, (uint32_t)e->n, mode_of(e), &e->kp, b, stream};
}

unsigned grid_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
int64_t n_words(int64_t n) { return (n + kWave - 1) / kWave; }

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace

extern "C" {

int rr_abi_version(void) { return RR_ABI_VERSION; }

const char* rr_last_error(void) { return g_err.c_str(); }

int rr_create(rr_env** out, const rr_params* p, int64_t n, int64_t env_id_offset, int device)
{
    if (!out || !p) return fail(RR_EINVAL, "rr_create: null argument");
    *out = nullptr;
    if (p->model != RR_MODEL_6DOF && p->model != RR_MODEL_3DOF)
        return fail(RR_EINVAL, "rr_create: model must be 3 or 6");
    if (p->integrator != RR_INT_RK4 && p->integrator != RR_INT_EULER && p->integrator != RR_INT_DOPRI5)
        return fail(RR_EINVAL, "rr_create: unknown integrator");
    const int64_t ns_ = p->model == RR_MODEL_6DOF ? 14 : 7;
    if (n <= 0 || n * (ns_ + 3) * 4 > (int64_t)0xFFFFFFFF)
        return fail(RR_EINVAL, "rr_create: n must be >= 1 and n*state_dim*4 must fit 32-bit buffer offsets");
    if (p->max_episode_steps < 0 || p->max_episode_steps > kMaxEpisodeSteps)
        return fail(RR_EINVAL, "rr_create: max_episode_steps must be in [0, 65535]");
    if (!(p->dt > 0.0)) return fail(RR_EINVAL, "rr_create: dt must be > 0");
    constexpr uint32_t kKnownFlags = RR_FLAG_AUTO_RESET | RR_FLAG_EPISODE_STATS | RR_FLAG_REWARD_ANNEALING |
                                     RR_FLAG_ACTION_SOA | RR_FLAG_SCIPY_H0_CLAMP | RR_FLAG_HOST_STATE;
    if (p->flags & ~kKnownFlags)  // the high bits carry the kernels' internal mode (kModeCounter, ...)
        return fail(RR_EINVAL, "rr_create: unknown flag bits");
    rr_env* e = new (std::nothrow) rr_env();
    if (!e) return fail(RR_ENOMEM, "rr_create: host allocation failed");
    e->device = device;
    e->p = *p;
    e->kp = make_kparams(*p);
    e->xp = make_xparams(*p);
    e->ns = p->model == RR_MODEL_6DOF ? 14 : 7;
    e->na = p->model == RR_MODEL_6DOF ? 3 : 2;
    e->nt = p->model == RR_MODEL_6DOF ? 5 : 6;
    e->n = n;
    e->id_off = env_id_offset;
    DeviceGuard g(device);
    {
        // test / A-B override of the helper-wave threshold: RR_HELP_MAX_N=<n> in the environment
        const char* hv = std::getenv("RR_HELP_MAX_N");
        e->help_max_n = hv ? std::strtoll(hv, nullptr, 10) : kHelpMaxN;
        // the exact mode's lean-kernel threshold: one env per lane of one wave per SIMD of THIS
        // device (a partitioned or smaller part has fewer CUs); RR_EXACT_LEAN_MIN_N overrides it
        // (tests run the lean kernel at small N)
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
            cus = (int)kExactLeanCUs;
        const char* lv = std::getenv("RR_EXACT_LEAN_MIN_N");
        e->exact_lean_min_n = lv ? std::strtoll(lv, nullptr, 10) : (int64_t)cus * 4 * kWave;
        // the plain kernels' whole-line done path (tests run it at small N with RR_WHOLE_LINE_MIN_N=0)
        const char* wv = std::getenv("RR_WHOLE_LINE_MIN_N");
        e->whole_line_min_n = wv ? std::strtoll(wv, nullptr, 10) : kWholeLineMinN;
    }
    struct A {
        void** ptr;
        size_t bytes;
    } allocs[] = {
        {(void**)&e->state, sizeof(float) * (e->ns + 3) * n},  // + v0, counter, ep_ret planes
        {(void**)&e->done_bits, sizeof(uint64_t) * n_words(n)},
        {(void**)&e->term_obs, sizeof(float) * e->ns * n},
        {(void**)&e->term_ret, sizeof(float) * n},        {(void**)&e->term_len, sizeof(int32_t) * n},
        {(void**)&e->g_idx, sizeof(int32_t) * n},         {(void**)&e->g_obs, sizeof(float) * e->ns * n},
        {(void**)&e->g_ret, sizeof(float) * n},           {(void**)&e->g_len, sizeof(int32_t) * n},
        {(void**)&e->g_trunc, sizeof(uint8_t) * n},
    };
    const bool exact = p->integrator == RR_INT_DOPRI5;
    e->host_state = (p->flags & RR_FLAG_HOST_STATE) != 0;
    for (auto& a : allocs) {
        if (e->host_state && a.ptr == (void**)&e->state) {
            // fine-grained (coherent) pinned host memory: the kernels' loads and stores go straight
            // to host memory, and the host reads the planes after a stream synchronise
            hipError_t err = hipHostMalloc(a.ptr, a.bytes, hipHostMallocCoherent | hipHostMallocMapped);
            if (err != hipSuccess) {
                *a.ptr = nullptr;
                rr_destroy(e);
                return hip_fail(err, "rr_create: hipHostMalloc (host state)");
            }
            std::memset(*a.ptr, 0, a.bytes);
            continue;
        }
        hipError_t err = hipMalloc(a.ptr, a.bytes);
        if (err != hipSuccess) {
            rr_destroy(e);
            return hip_fail(err, "rr_create: hipMalloc");
        }
        err = hipMemset(*a.ptr, 0, a.bytes);
        if (err != hipSuccess) {
            rr_destroy(e);
            return hip_fail(err, "rr_create: hipMemset");
        }
    }
    if (exact) {
        const size_t bytes = sizeof(double) * e->ns * n;
        hipError_t err = hipMalloc((void**)&e->state64, bytes);
        if (err == hipSuccess) err = hipMemset(e->state64, 0, bytes);
        if (err != hipSuccess) {
            rr_destroy(e);
            return hip_fail(err, "rr_create: hipMalloc (fp64 state)");
        }
    }
    e->v0 = e->state + (size_t)e->ns * n;
    e->counter = reinterpret_cast<uint32_t*>(e->state + (size_t)(e->ns + 1) * n);
    e->ep_ret = e->state + (size_t)(e->ns + 2) * n;
    e->kp.id_off = env_id_offset;
    {
        hipError_t err = hipMalloc((void**)&e->d_kp, sizeof(KParams));
        if (err == hipSuccess) err = hipEventCreateWithFlags(&e->seed_ev, hipEventDisableTiming);
        if (err == hipSuccess) err = hipMalloc((void**)&e->d_xp, sizeof(XParams));
        if (err == hipSuccess) err = hipMemcpy(e->d_xp, &e->xp, sizeof(XParams), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            rr_destroy(e);
            return hip_fail(err, "rr_create: hipMalloc (params)");
        }
    }
    int rc = rr_seed(e, 42, nullptr);
    if (rc == RR_OK) {
        hipError_t err = hipDeviceSynchronize();
        if (err != hipSuccess) rc = hip_fail(err, "rr_create: sync");
    }
    if (rc != RR_OK) {
        rr_destroy(e);
        return rc;
    }
    *out = e;
    return RR_OK;
}

int rr_destroy(rr_env* e)
{
    if (!e) return RR_OK;
    DeviceGuard g(e->device);
    if (e->host_state && e->state) {
        (void)hipHostFree(e->state);
        e->state = nullptr;
    }
    if (e->seed_ev) (void)hipEventDestroy(e->seed_ev);
    void* ptrs[] = {e->state, e->state64, e->d_kp, e->d_xp, e->done_bits,
                    e->term_obs, e->term_ret, e->term_len, e->g_idx, e->g_obs,  e->g_ret, e->g_len,
                    e->g_trunc};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    delete e;
    return RR_OK;
}

int64_t rr_num_envs(const rr_env* e) { return e ? e->n : -1; }
int rr_state_dim(const rr_env* e) { return e ? e->ns : -1; }
int rr_action_dim(const rr_env* e) { return e ? e->na : -1; }

int rr_seed(rr_env* e, uint64_t seed, void* stream)
{
    // The reset stream is counter-based and every kernel reads its key from the device copy of
    // the parameters (Bufs.kp), so the new key applies to every launch that runs after this call
    // — graph replays of launches captured before it included — whatever the batch size. The
    // copy is written in the order of `stream` (the handle's stream: every launch queued on it
    // before this call reads the old key) and the call returns once it has landed. Refused
    // while `stream` is being captured: the key is not a graph node (replays read the key
    // current when they run).
    if (!e) return fail(RR_EINVAL, "rr_seed: null handle");
    DeviceGuard g(e->device);
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipError_t err = hipStreamIsCapturing(s, &cs);
    if (err != hipSuccess) return hip_fail(err, "rr_seed: hipStreamIsCapturing");
    if (cs != hipStreamCaptureStatusNone)
        return fail(RR_EINVAL, "rr_seed: the stream is being captured into a graph (seed before capturing: "
                               "replays read the key current when they run)");
    // launches of this handle queued on OTHER streams may still read the key: the new key must not
    // land under them. The copy waits, on the device, for the work queued so far on
    // every stream the handle launched on (the per-handle event recorded there now); the usual
    // single-stream caller keeps the plain stream-ordered write. Past kSeedStreams distinct streams
    // the device is synchronised. A stream being captured has run nothing of the capture yet.
    // Graph replays are not launches of the handle: the caller orders them (header).
    // A noted stream the runtime no longer knows (destroyed since: its queued work still runs) is
    // covered by the same device synchronise.
    bool sync_device = e->streams_overflow;
    for (int k = 0; k < e->n_streams && !sync_device; ++k) {
        hipStream_t o = (hipStream_t)e->streams[k];
        if (o == s) continue;
        hipStreamCaptureStatus ocs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(o, &ocs) != hipSuccess) {
            (void)hipGetLastError();
            sync_device = true;
            break;
        }
        if (ocs != hipStreamCaptureStatusNone) continue;
        err = hipEventRecord(e->seed_ev, o);
        if (err == hipSuccess) err = hipStreamWaitEvent(s, e->seed_ev, 0);
        if (err != hipSuccess) return hip_fail(err, "rr_seed: order the key after the handle's other streams");
    }
    if (sync_device) {
        err = hipDeviceSynchronize();
        if (err != hipSuccess) return hip_fail(err, "rr_seed: synchronise the device");
    }
    e->n_streams = 0;  // everything queued so far is ordered before the key copy
    e->streams_overflow = false;
    seed_words(seed, e->kp.seed_w);
    err = hipMemcpyAsync(e->d_kp, &e->kp, sizeof(KParams), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);  // e->kp is pageable host memory: wait until it is read
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_seed: params upload");
}

int rr_reset(rr_env* e, const uint8_t* mask, float* obs, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_reset: null handle");
    const Bufs b = bufs_of(e);
    if (e->p.model == RR_MODEL_6DOF)
        hipLaunchKernelGGL(reset_kernel<6>, dim3(grid_of(e->n)), dim3(kBlock), 0, (hipStream_t)stream, e->kp, b,
                           mask, obs, e->state64);
    else
        hipLaunchKernelGGL(reset_kernel<3>, dim3(grid_of(e->n)), dim3(kBlock), 0, (hipStream_t)stream, e->kp, b,
                           mask, obs, e->state64);
    hipError_t err = hipGetLastError();
    note_stream(e, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_reset: launch");
}

}  // extern "C"

namespace {
// one step launch (rr_step / rr_step_repeat; arguments checked by the caller)
template <bool ROWS>
int launch_step(rr_env* e, const float* action, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
                float* terms, void* stream)
{
    StepIO io;
    io.action = action;
    io.obs = obs;
    io.reward = reward;
    io.done = done;
    io.truncated = truncated;
    io.terms = terms;
    io.obs_vec_ok = ((uintptr_t)obs & 15u) == 0;
    const Bufs b = bufs_of(e);
    hipStream_t s = (hipStream_t)stream;
    const bool soa = e->p.flags & RR_FLAG_ACTION_SOA;
    const dim3 grid(grid_of(e->n)), block(kBlock);
    if (e->p.integrator == RR_INT_DOPRI5) {
        // the exact kernels live in the second translation unit (rocket_exact.hip: compiled with a
        // register-pressure-first scheduler, no scratch spills)
        const bool lean = e->p.model == RR_MODEL_6DOF && e->n > e->exact_lean_min_n;
        const ExactLaunch L = {e->p.model, (lean ? 1 : 0) | (soa ? 2 : 0), grid.x, e->d_xp, &b, e->state64, stream};
        const hipError_t xe = (hipError_t)rrx_launch_exact(&L, &io);
        if (xe != hipSuccess) return hip_fail(xe, "rr_step: exact launch");
    } else {
        const uint32_t nn = (uint32_t)e->n;
        const uint32_t mode = mode_of(e) | (e->n > e->whole_line_min_n ? kModeWholeLines : 0u);
        // small N (at most ~2 main waves per SIMD): helper waves draw the reset candidates
        const bool help = (mode & RR_FLAG_AUTO_RESET) && e->n <= e->help_max_n;
        // up to 16 384 envs one main wave per workgroup (64 + 64 threads): the few workgroups
        // spread over 4x as many CUs (A/B at N = 4 096: -5 % 6DOF); above, 4 main waves
        const bool narrow = e->n <= kNarrowMaxN;
        dispatch_env(e->p.model, e->p.integrator, [&](auto m, auto i) {
            constexpr int M = decltype(m)::value, I = decltype(i)::value;
            auto launch = [&](auto a) {
                constexpr bool A = decltype(a)::value;
                if (help && narrow)
                    hipLaunchKernelGGL((step_kernel<M, I, A, true, 1, ROWS>), dim3((unsigned)n_words(e->n)),
                                       dim3(2 * kWave), 0, s, e->state, action, nn, mode, e->kp, b, io);
                else if (help)
                    hipLaunchKernelGGL((step_kernel<M, I, A, true, kWavesPerBlock, ROWS>), grid, dim3(2 * kBlock), 0, s,
                                       e->state, action, nn, mode, e->kp, b, io);
                else
                    hipLaunchKernelGGL((step_kernel<M, I, A, false, kWavesPerBlock, ROWS>), grid, block, 0, s, e->state,
                                       action, nn, mode, e->kp, b, io);
            };
            if constexpr (ROWS) launch(std::false_type{});  // row-major actions only (the multi-GPU gather path)
            else dispatch_flag(soa, launch);
        });
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return hip_fail(err, "rr_step: launch");
    e->steps++;
    note_stream(e, stream);
    return RR_OK;
}
}  // namespace

extern "C" {

int rr_step(rr_env* e, const float* action, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
            float* terms, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_step: null handle");
    if (!action || !obs || !reward || !done) return fail(RR_EINVAL, "rr_step: action/obs/reward/done required");
    return launch_step<false>(e, action, obs, reward, done, truncated, terms, stream);
}

int rr_step_rows(rr_env* e, const float* action, float* rows, uint8_t* truncated, float* terms, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_step_rows: null handle");
    if (!action || !rows) return fail(RR_EINVAL, "rr_step_rows: action/rows required");
    if (e->p.integrator == RR_INT_DOPRI5 || (e->p.flags & RR_FLAG_ACTION_SOA))
        return fail(RR_EINVAL, "rr_step_rows: RK4 / Euler envs with [N][action_dim] actions only");
    return launch_step<true>(e, action, rows, nullptr, nullptr, truncated, terms, stream);
}

int rr_step_repeat(rr_env* e, const float* actions, int64_t n_batches, int64_t n_steps, float* obs, float* reward,
                   uint8_t* done, uint8_t* truncated, float* terms, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_step_repeat: null handle");
    if (!actions || !obs || !reward || !done) return fail(RR_EINVAL, "rr_step_repeat: actions/obs/reward/done required");
    if (n_batches <= 0 || n_steps < 0) return fail(RR_EINVAL, "rr_step_repeat: n_batches must be >= 1, n_steps >= 0");
    const int64_t batch = e->n * e->na;
    int rc = RR_OK;
    for (int64_t t = 0; t < n_steps && rc == RR_OK; ++t)
        rc = launch_step<false>(e, actions + (t % n_batches) * batch, obs, reward, done, truncated, terms, stream);
    return rc;
}

namespace {

// v0 / counter / episode-return part shared by the fp32 and fp64 setters
hipError_t set_aux(rr_env* e, const float* v0, const int32_t* elapsed, hipStream_t s)
{
    hipError_t err = hipSuccess;
    if (v0) err = hipMemcpyAsync(e->v0, v0, sizeof(float) * e->n, hipMemcpyDefault, s);
    if (err == hipSuccess) {
        if (elapsed) {
            err = hipMemcpyAsync(e->counter, elapsed, sizeof(int32_t) * e->n, hipMemcpyDefault, s);
        } else {  // elapsed steps -> 0, the episode field (reset-stream key) is kept
            hipLaunchKernelGGL(clear_elapsed_kernel, dim3(grid_of(e->n)), dim3(kBlock), 0, s, e->counter, e->n,
                               e->kp.el_mask);
            err = hipGetLastError();
        }
    }
    if (err == hipSuccess) err = hipMemsetAsync(e->ep_ret, 0, sizeof(float) * e->n, s);
    return err;
}

hipError_t get_aux(rr_env* e, float* v0, int32_t* elapsed, hipStream_t s)
{
    hipError_t err = hipSuccess;
    if (v0) err = hipMemcpyAsync(v0, e->v0, sizeof(float) * e->n, hipMemcpyDefault, s);
    if (err == hipSuccess && elapsed)
        err = hipMemcpyAsync(elapsed, e->counter, sizeof(int32_t) * e->n, hipMemcpyDefault, s);
    return err;
}

hipError_t widen_async(const float* src, double* dst, int64_t count, hipStream_t s)
{
    hipLaunchKernelGGL(widen_kernel, dim3(grid_of(count)), dim3(kBlock), 0, s, src, dst, count);
    return hipGetLastError();
}

hipError_t narrow_async(const double* src, float* dst, int64_t count, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_of(count)), dim3(kBlock), 0, s, src, dst, count);
    return hipGetLastError();
}

}  // namespace

int rr_set_state(rr_env* e, const float* state_soa, const float* v0, const int32_t* elapsed, void* stream)
{
    if (!e || !state_soa) return fail(RR_EINVAL, "rr_set_state: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int64_t cnt = (int64_t)e->ns * e->n;
    hipError_t err = hipMemcpyAsync(e->state, state_soa, sizeof(float) * cnt, hipMemcpyDefault, s);
    if (err == hipSuccess && e->state64) err = widen_async(e->state, e->state64, cnt, s);
    if (err == hipSuccess) err = set_aux(e, v0, elapsed, s);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_set_state");
}

int rr_get_state(rr_env* e, float* state_soa, float* v0, int32_t* elapsed, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_get_state: null handle");
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipSuccess;
    if (state_soa)
        err = hipMemcpyAsync(state_soa, e->state, sizeof(float) * e->ns * e->n, hipMemcpyDefault, s);
    if (err == hipSuccess) err = get_aux(e, v0, elapsed, s);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_get_state");
}

int rr_set_state64(rr_env* e, const double* state_soa, const float* v0, const int32_t* elapsed, void* stream)
{
    if (!e || !state_soa) return fail(RR_EINVAL, "rr_set_state64: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int64_t cnt = (int64_t)e->ns * e->n;
    hipError_t err = hipSuccess;
    if (e->state64) {
        err = hipMemcpyAsync(e->state64, state_soa, sizeof(double) * cnt, hipMemcpyDefault, s);
        if (err == hipSuccess) err = narrow_async(e->state64, e->state, cnt, s);
    } else {
        err = narrow_async(state_soa, e->state, cnt, s);
    }
    if (err == hipSuccess) err = set_aux(e, v0, elapsed, s);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_set_state64");
}

int rr_get_state64(rr_env* e, double* state_soa, float* v0, int32_t* elapsed, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_get_state64: null handle");
    hipStream_t s = (hipStream_t)stream;
    const int64_t cnt = (int64_t)e->ns * e->n;
    hipError_t err = hipSuccess;
    if (state_soa) {
        if (e->state64)
            err = hipMemcpyAsync(state_soa, e->state64, sizeof(double) * cnt, hipMemcpyDefault, s);
        else
            err = widen_async(e->state, state_soa, cnt, s);
    }
    if (err == hipSuccess) err = get_aux(e, v0, elapsed, s);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_get_state64");
}

int rr_counter_bits(const rr_env* e) { return e ? (int)e->kp.ep_shift : RR_EINVAL; }

int rr_get_aux(rr_env* e, uint32_t* counter, float* ep_return, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_get_aux: null handle");
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipSuccess;
    if (counter) err = hipMemcpyAsync(counter, e->counter, sizeof(uint32_t) * e->n, hipMemcpyDefault, s);
    if (err == hipSuccess && ep_return)
        err = hipMemcpyAsync(ep_return, e->ep_ret, sizeof(float) * e->n, hipMemcpyDefault, s);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_get_aux");
}

int rr_set_aux(rr_env* e, const uint32_t* counter, const float* ep_return, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_set_aux: null handle");
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipSuccess;
    if (counter) err = hipMemcpyAsync(e->counter, counter, sizeof(uint32_t) * e->n, hipMemcpyDefault, s);
    if (err == hipSuccess && ep_return)
        err = hipMemcpyAsync(e->ep_ret, ep_return, sizeof(float) * e->n, hipMemcpyDefault, s);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_set_aux");
}

int rr_get_buffers(rr_env* e, rr_buffers* out)
{
    if (!e || !out) return fail(RR_EINVAL, "rr_get_buffers: null argument");
    out->state = e->state;
    out->v0 = e->v0;
    out->elapsed = (int32_t*)e->counter;
    out->ep_return = e->ep_ret;
    out->done_bits = e->done_bits;
    out->terminal_obs = e->term_obs;
    out->terminal_return = e->term_ret;
    out->terminal_len = e->term_len;
    return RR_OK;
}

int rr_host_alloc(void** out, int64_t bytes)
{
    if (!out || bytes <= 0) return fail(RR_EINVAL, "rr_host_alloc: null pointer or bytes <= 0");
    *out = nullptr;
    const hipError_t err = hipHostMalloc(out, (size_t)bytes, hipHostMallocCoherent | hipHostMallocMapped);
    if (err != hipSuccess) {
        *out = nullptr;
        return hip_fail(err, "rr_host_alloc");
    }
    std::memset(*out, 0, (size_t)bytes);
    return RR_OK;
}

int rr_host_free(void* p)
{
    if (!p) return RR_OK;
    const hipError_t err = hipHostFree(p);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_host_free");
}

}  // extern "C"

namespace {
// The rows of the env indices `hidx` (ascending) from the given [N][ns] / [N] sources into the
// caller's host arrays (at most `capacity` rows): one index upload, one gather kernel into the
// env's scratch, the copies, one synchronise. Returns the number of indices or an RR_E* code.
int64_t fetch_rows(rr_env* e, const std::vector<int32_t>& hidx, int64_t capacity, const float* src_obs,
                   const float* src_ret, const int32_t* src_len, const uint8_t* src_trunc, int32_t* idx,
                   float* term_obs, float* term_return, int32_t* term_len, uint8_t* trunc_out, hipStream_t s,
                   const char* what)
{
    const int64_t count = (int64_t)hidx.size();
    const int64_t m = std::min<int64_t>(count, capacity);
    if (m == 0) return count;
    if (idx) std::memcpy(idx, hidx.data(), sizeof(int32_t) * m);
    if (term_obs || term_return || term_len || trunc_out) {
        hipError_t err = hipMemcpyAsync(e->g_idx, hidx.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, s);
        if (err != hipSuccess) return hip_fail(err, what);
        hipLaunchKernelGGL(gather_done_kernel, dim3(grid_of(m)), dim3(kBlock), 0, s, e->g_idx, m, e->ns, src_obs,
                           src_ret, src_len, trunc_out ? src_trunc : nullptr, e->g_obs, e->g_ret, e->g_len, e->g_trunc);
        err = hipGetLastError();
        if (err == hipSuccess && term_obs)
            err = hipMemcpyAsync(term_obs, e->g_obs, sizeof(float) * e->ns * m, hipMemcpyDefault, s);
        if (err == hipSuccess && term_return)
            err = hipMemcpyAsync(term_return, e->g_ret, sizeof(float) * m, hipMemcpyDefault, s);
        if (err == hipSuccess && term_len)
            err = hipMemcpyAsync(term_len, e->g_len, sizeof(int32_t) * m, hipMemcpyDefault, s);
        if (err == hipSuccess && trunc_out)
            err = hipMemcpyAsync(trunc_out, e->g_trunc, sizeof(uint8_t) * m, hipMemcpyDefault, s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        if (err != hipSuccess) return hip_fail(err, what);
    }
    return count;
}
}  // namespace

extern "C" {

int64_t rr_fetch_done(rr_env* e, int64_t capacity, int32_t* idx, float* term_obs, float* term_return,
                      int32_t* term_len, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_fetch_done: null handle");
    if (capacity < 0) return fail(RR_EINVAL, "rr_fetch_done: negative capacity");
    if (e->steps == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nw = n_words(e->n);
    std::vector<uint64_t> bits(nw);
    hipError_t err = hipMemcpyAsync(bits.data(), e->done_bits, sizeof(uint64_t) * nw, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return hip_fail(err, "rr_fetch_done: done bits");
    std::vector<int32_t> hidx;
    for (int64_t w = 0; w < nw; ++w) {
        uint64_t m = bits[w];
        while (m) {
            const int b = __builtin_ctzll(m);
            hidx.push_back((int32_t)(w * kWave + b));
            m &= m - 1;
        }
    }
    return fetch_rows(e, hidx, capacity, e->term_obs, e->term_ret, e->term_len, nullptr, idx, term_obs, term_return,
                      term_len, nullptr, s, "rr_fetch_done: gather");
}

int64_t rr_gather_rows(rr_env* e, const uint8_t* done, const float* term_obs_src, const float* term_return_src,
                       const int32_t* term_len_src, const uint8_t* truncated_src, int64_t capacity, int32_t* idx,
                       float* term_obs, float* term_return, int32_t* term_len, uint8_t* truncated, void* stream)
{
    if (!e || !done) return fail(RR_EINVAL, "rr_gather_rows: null handle or done flags");
    if (capacity < 0) return fail(RR_EINVAL, "rr_gather_rows: negative capacity");
    if ((term_obs && !term_obs_src) || (term_return && !term_return_src) || (term_len && !term_len_src) ||
        (truncated && !truncated_src))
        return fail(RR_EINVAL, "rr_gather_rows: an output without its source");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = e->n;
    std::vector<uint64_t> flags((n + 7) / 8, 0);  // the u8 flags, read 8 at a time
    hipError_t err = hipMemcpyAsync(flags.data(), done, (size_t)n, hipMemcpyDefault, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return hip_fail(err, "rr_gather_rows: done flags");
    std::vector<int32_t> hidx;
    const uint8_t* f8 = reinterpret_cast<const uint8_t*>(flags.data());
    for (int64_t w = 0; w < (int64_t)flags.size(); ++w) {
        if (!flags[w]) continue;  // ~1 % of the envs finish per step: most words are zero
        for (int64_t i = 8 * w; i < std::min<int64_t>(8 * w + 8, n); ++i)
            if (f8[i]) hidx.push_back((int32_t)i);
    }
    return fetch_rows(e, hidx, capacity, term_obs_src, term_return_src, term_len_src, truncated_src, idx, term_obs,
                      term_return, term_len, truncated, s, "rr_gather_rows: gather");
}

int rr_copy_terminal(rr_env* e, float* term_obs, float* term_return, int32_t* term_len, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_copy_terminal: null handle");
    if (!term_obs && !term_return && !term_len) return RR_OK;
    if (e->steps == 0) return RR_OK;  // no step yet: no done rows
    // only the rows of the envs done at the last step (its done_bits): ~1 % of the rows in steady
    // state, so one pass reads N/8 bytes of masks instead of copying the whole [N][state_dim] buffer
    hipLaunchKernelGGL(copy_done_rows_kernel, dim3(grid_of(e->n)), dim3(kBlock), 0, (hipStream_t)stream,
                       e->done_bits, e->n, e->ns, e->term_obs, e->term_ret, e->term_len, term_obs, term_return,
                       term_len);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_copy_terminal");
}

// ---- on-device PPO rollout (rocket_policy.inc) ----

}  // extern "C"

// the policy kernels' PREC (0 / 1 / 2) of an RR_POLICY_* value, -1 of anything else
static int prec_of(int precision)
{
    return precision == RR_POLICY_FP32 ? 0 : precision == RR_POLICY_BF16 ? 1 : precision == RR_POLICY_FP16X3 ? 2 : -1;
}

// f(tag<OBS>, tag<ACT>, tag<PREC>) for a supported (obs_dim, act_dim, precision); false otherwise
template <class F>
static bool pol_dispatch(int obs_dim, int act_dim, int precision, F&& f)
{
    const int prec = prec_of(precision);
    if (prec < 0) return false;
    if (obs_dim == 14 && act_dim == 3) dispatch_prec(prec, [&](auto p) { f(tag<14>{}, tag<3>{}, p); });
    else if (obs_dim == 7 && act_dim == 2) dispatch_prec(prec, [&](auto p) { f(tag<7>{}, tag<2>{}, p); });
    else return false;
    return true;
}

// the checks every policy-driven env launch shares, after the caller's null checks: `params`
// 16-B aligned and a known precision. Returns the kernels' PREC, or fails with `w`'s prefix (< 0)
static int policy_prec(const std::string& w, const float* params, int precision)
{
    if (((uintptr_t)params & 15) != 0) return fail(RR_EINVAL, w + "params must be 16-B aligned");
    if (prec_of(precision) < 0)
        return fail(RR_EINVAL, w + "precision must be RR_POLICY_FP32, RR_POLICY_BF16 or RR_POLICY_FP16X3");
    return prec_of(precision);
}

#define RR_POL_UNSUPPORTED(fn) \
    fail(RR_EINVAL, fn ": supported (obs_dim, act_dim) are (14, 3) and (7, 2), precision RR_POLICY_FP32 / RR_POLICY_BF16 / RR_POLICY_FP16X3")

// rr_policy_layout's 12 offsets of a pol::Layout into `off` (if given); the image's size in floats
template <class LL>
static int layout_offsets(int64_t* off)
{
    const int64_t v[12] = {LL::L1A, LL::B1, LL::L2A, LL::B2, LL::TOWER, LL::PI,
                           LL::VF,  LL::HA, LL::HV,  LL::HB, LL::VB,    LL::LS};
    for (int k = 0; off && k < 12; ++k) off[k] = v[k];
    return LL::SIZE;
}

// The argument checks of rr_policy_act and rr_policy_act_discrete (`extra`: the latter's table)
static int act_args_ok(const char* who, const float* params, const void* extra, const float* obs, const uint64_t* iter,
                       const float* action_env, const float* action, const float* value, const float* log_prob,
                       int64_t n, const float* prev_term_obs, const uint8_t* prev_truncated, const float* prev_reward,
                       const float* reward_out, const uint8_t* done, const float* start_out)
{
    if (!params || !extra || !obs || !iter || !action_env || !action || !value || !log_prob || n <= 0)
        return refuse(who, "null argument or n <= 0");
    if (reward_out && (!prev_term_obs || !prev_truncated || !prev_reward))
        return refuse(who, "reward_out needs prev_term_obs, prev_truncated, prev_reward");
    if (start_out && !done) return refuse(who, "start_out needs done");
    if (((uintptr_t)params & 15) != 0) return refuse(who, "params must be 16-B aligned");
    return RR_OK;
}

// the noise key's seed words: splitmix64 of the user seed (raw seed words XORed into the key
// made seed 1 give env e the stream seed 0 gives env e ^ 1, and seed 2^32 that of iteration + 1)
static void act_seed_words(uint64_t seed, uint32_t& lo, uint32_t& hi)
{
    const uint64_t mixed = splitmix64(seed);
    lo = (uint32_t)mixed;
    hi = (uint32_t)(mixed >> 32);
}

// What the learner's host code knows of a policy shape: one tower's partial-gradient vector and packed image
// in floats (ppo::Part / ppo::Pack), how many tensors a call binds, and their sizes in rr_policy_pack order
struct LearnerShape {
    int obs_dim;
    int64_t part, pack;  // part == 0: not a supported shape
    int n;
    int64_t numel[13];
    int64_t fin() const { return (part + kFinElems - 1) / kFinElems; }  // the finish kernel's blocks per tower
};

// The image <O, A> with `rows` action-head rows, `n` tensors bound (here: no template inside extern "C")
template <int O, int A>
static LearnerShape shape_of(int64_t rows, int n)
{
    return {O, ppo::Part<O, A>::SIZE, ppo::Pack<O, A>::SIZE, n,
            {64 * O, 64, 64 * 64, 64, 64 * O, 64, 64 * 64, 64, 64 * rows, rows, 64, 1, rows}};
}

extern "C" {

int rr_policy_layout(int obs_dim, int act_dim, int precision, int64_t* off)
{
    int size = 0;
    const bool ok = pol_dispatch(obs_dim, act_dim, precision, [&](auto o, auto a, auto p) {
        size = layout_offsets<pol::Layout<decltype(o)::value, decltype(a)::value, decltype(p)::value>>(off);
    });
    return ok ? size : RR_POL_UNSUPPORTED("rr_policy_layout");
}

int rr_policy_pack(int obs_dim, int act_dim, int precision, const float* const* src, float* params, void* stream)
{
    if (!src || !params) return fail(RR_EINVAL, "rr_policy_pack: null argument");
    PolSrc ps;
    for (int k = 0; k < 13; ++k) {
        if (!src[k]) return fail(RR_EINVAL, "rr_policy_pack: null parameter tensor");
        ps.p[k] = src[k];
    }
    hipStream_t s = (hipStream_t)stream;
    const bool ok = pol_dispatch(obs_dim, act_dim, precision, [&](auto o, auto a, auto p) {
        constexpr int O = decltype(o)::value, A = decltype(a)::value, P = decltype(p)::value;
        hipLaunchKernelGGL((policy_pack_kernel<O, A, P>), dim3((pol::Layout<O, A, P>::SIZE + 255) / 256), dim3(256), 0,
                           s, ps, params);
    });
    if (!ok) return RR_POL_UNSUPPORTED("rr_policy_pack");
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_policy_pack: launch");
}

int rr_policy_act(const float* params, int obs_dim, int act_dim, int precision, int64_t n, int64_t env_id_offset,
                  const float* obs, uint64_t seed, const uint64_t* iter, int t, float* action_env, float* action,
                  float* value, float* log_prob, float* obs_copy, const float* prev_term_obs,
                  const uint8_t* prev_truncated, const float* prev_reward, float gamma, float* reward_out,
                  const uint8_t* done, float* start_out, void* stream)
{
    if (const int rc = act_args_ok("rr_policy_act", params, params, obs, iter, action_env, action, value, log_prob, n,
                                   prev_term_obs, prev_truncated, prev_reward, reward_out, done, start_out);
        rc != RR_OK)
        return rc;
    const dim3 grid((unsigned)((n + pol::kEnvsPerBlock - 1) / pol::kEnvsPerBlock)), block(pol::kThreads);
    hipStream_t s = (hipStream_t)stream;
    uint32_t lo, hi;
    act_seed_words(seed, lo, hi);
    const bool ok = pol_dispatch(obs_dim, act_dim, precision, [&](auto o, auto a, auto p) {
        hipLaunchKernelGGL((policy_act_kernel<decltype(o)::value, decltype(a)::value, decltype(p)::value>), grid,
                           block, 0, s, params, n, env_id_offset, obs, lo, hi, iter, (uint32_t)t, action_env, action,
                           value, log_prob, obs_copy, prev_term_obs, prev_truncated, prev_reward, gamma, reward_out,
                           done, start_out);
    });
    if (!ok) return RR_POL_UNSUPPORTED("rr_policy_act");
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_policy_act: launch");
}

int rr_policy_bootstrap(const float* params, int obs_dim, int act_dim, int precision, int64_t n,
                        const float* term_obs, const uint8_t* truncated, const float* reward, float gamma,
                        float* reward_out, const float* obs, float* value_out, void* stream)
{
    if (!params || n <= 0) return fail(RR_EINVAL, "rr_policy_bootstrap: null params or n <= 0");
    if (term_obs && (!truncated || !reward || !reward_out))
        return fail(RR_EINVAL, "rr_policy_bootstrap: term_obs needs truncated, reward, reward_out");
    if (!term_obs && !value_out) return fail(RR_EINVAL, "rr_policy_bootstrap: nothing to do");
    if (value_out && !obs) return fail(RR_EINVAL, "rr_policy_bootstrap: value_out needs obs");
    if (((uintptr_t)params & 15) != 0) return fail(RR_EINVAL, "rr_policy_bootstrap: params must be 16-B aligned");
    if (obs_dim == 7 && act_dim == 4) {  // the Categorical policy's image (rr_policy_pack_discrete): its unit's kernel
        if (precision != RR_POLICY_FP32)
            return fail(RR_EINVAL, "rr_policy_bootstrap: (obs_dim, act_dim) = (7, 4) is RR_POLICY_FP32 only");
        DiscreteLaunch D = {};
        D.op = kDiscBootstrap;
        D.params = params;
        D.n = n;
        D.prev_term_obs = term_obs;
        D.prev_trunc = truncated;
        D.prev_reward = reward;
        D.gamma = gamma;
        D.reward_out = reward_out;
        D.obs = obs;
        D.value_out = value_out;
        const hipError_t err = (hipError_t)rrc_launch_discrete(&D, stream);
        return err == hipSuccess ? RR_OK : hip_fail(err, "rr_policy_bootstrap: launch");
    }
    const dim3 grid((unsigned)((n + pol::kEnvsPerBlock - 1) / pol::kEnvsPerBlock)), block(pol::kThreads);
    hipStream_t s = (hipStream_t)stream;
    const bool ok = pol_dispatch(obs_dim, act_dim, precision, [&](auto o, auto a, auto p) {
        hipLaunchKernelGGL((policy_bootstrap_kernel<decltype(o)::value, decltype(a)::value, decltype(p)::value>),
                           grid, block, 0, s, params, n, term_obs, truncated, reward, gamma, reward_out, obs,
                           value_out);
    });
    if (!ok) return RR_POL_UNSUPPORTED("rr_policy_bootstrap");
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_policy_bootstrap: launch");
}

namespace {
int launch_rollout(rr_env* e, const char* who, bool multi, const float* params, int precision, uint64_t seed,
                   const uint64_t* iter, RolloutIO& io, void* stream, const CollectStatsIO* stats = nullptr,
                   const DiscHead* head = nullptr)
{
    const std::string w = std::string(who) + ": ";
    if (!params || !iter || !io.buf_obs || !io.buf_act || !io.buf_val || !io.buf_logp || !io.buf_start ||
        !io.buf_rew || !io.reward || !io.done)
        return fail(RR_EINVAL, w + "null argument");
    const int prec = policy_prec(w, params, precision);
    if (prec < 0) return prec;
    if (e->p.integrator == RR_INT_DOPRI5)
        return fail(RR_EINVAL, w + "RR_INT_DOPRI5 envs step through rr_policy_act + rr_step");
    io.params = params;
    io.iter = iter;
    const uint64_t mixed = splitmix64(seed);  // as rr_policy_act: the same noise key
    io.seed_lo = (uint32_t)mixed;
    io.seed_hi = (uint32_t)(mixed >> 32);
    io.obs_vec_ok = ((uintptr_t)io.obs & 15u) == 0;
    io.buf_obs_vec_ok = ((uintptr_t)io.buf_obs & 15u) == 0;
    const Bufs b = bufs_of(e);
    const EnvLaunch L = env_launch(e, prec, &b, stream);
    // 64 envs per wave (two 32-env MFMA column tiles). 32 envs per wave (rol::Shape<1>, two waves
    // per SIMD) measured 2-16 % slower at N = 65536 in round 2 and 4-8 % slower in round 4, with or
    // without the second wave's start staggered: the env step's VALU work doubles, and an fp32
    // MFMA holds its SIMD's vector issue, so one wave's MFMAs do not hide the other's VALU work
    // (tools/coissue_probe.hip, profiles/r04/coissue/).
    // The collect kernel (MULTI) lives in the third translation unit (rocket_collect.hip), compiled
    // with the MFMA accumulators in VGPRs (rl_rocket_amd/build.py COLLECT_FLAGS).
    hipError_t err = hipSuccess;
    if (head && stats) {  // rr_rollout_collect_discrete_stats (collect_stats_discrete/): two launches
        err = (hipError_t)rrc_launch_collect_discrete_stats(&L, &io, head, stats);
    } else if (head) {  // the Categorical head (rollout_discrete/rocket_rollout_discrete.hip): the collect or one step
        err = (hipError_t)rrc_launch_rollout_discrete(&L, &io, head, multi);
    } else if (multi && stats) {  // rr_rollout_collect_stats (collect_stats/rocket_collect_stats.hip): two launches
        err = (hipError_t)rrc_launch_collect_stats(&L, &io, stats);
    } else if (multi) {
        err = (hipError_t)rrc_launch_collect(&L, &io);
    } else {
        dispatch_env_prec(L.model, L.integ, L.prec, [&](auto m, auto i, auto p) {
            constexpr int M = decltype(m)::value, I = decltype(i)::value, P = decltype(p)::value;
            hipLaunchKernelGGL((rollout_step_kernel<M, I, P, false, 2>), dim3(L.grid), dim3(rol::Shape<2>::kThreads),
                               0, (hipStream_t)stream, e->state, L.n, L.mode, e->kp, b, io);
        });
        err = hipGetLastError();
    }
    if (err != hipSuccess) return hip_fail(err, (w + "launch").c_str());
    e->steps += io.T;
    note_stream(e, stream);
    return RR_OK;
}

// the RolloutIO fields rr_rollout_step and rr_rollout_collect both take from their caller (the
// per-step buffer slices and the env outputs); the rest zero
RolloutIO rollout_io(float* buf_obs, float* buf_action, float* buf_value, float* buf_log_prob, float* buf_start,
                     float* buf_reward, float* obs, float* reward, uint8_t* done, uint8_t* truncated, float* terms)
{
    RolloutIO io = {};
    io.buf_obs = buf_obs;
    io.buf_act = buf_action;
    io.buf_val = buf_value;
    io.buf_logp = buf_log_prob;
    io.buf_start = buf_start;
    io.buf_rew = buf_reward;
    io.obs = obs;
    io.reward = reward;
    io.done = done;
    io.truncated = truncated;
    io.terms = terms;
    return io;
}

// what a whole rollout in one launch adds to them (rr_rollout_collect, rr_rollout_collect_stats):
// the step count, the GAE coefficients and the end-of-rollout outputs
void collect_io(RolloutIO& io, int n_steps, double gamma, double gae_lambda, float* buf_advantage, float* buf_return,
                float* last_value, float* last_done, float* last_start)
{
    io.buf_adv = buf_advantage;
    io.buf_ret = buf_return;
    io.last_value = last_value;
    io.last_done = last_done;
    io.last_start = last_start;
    io.t = 0;
    io.T = (uint32_t)n_steps;
    io.gamma = (float)gamma;  // the timeout bootstrap, fp32 as rr_rollout_step's
    io.gamma64 = gamma;
    io.lam = gae_lambda;
}
}  // namespace

int rr_rollout_step(rr_env* e, const float* params, int precision, uint64_t seed, const uint64_t* iter, int t,
                    float gamma, float* buf_obs, float* buf_action, float* buf_value, float* buf_log_prob,
                    float* buf_start, float* buf_reward, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
                    float* terms, void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_rollout_step: null handle");
    RolloutIO io = rollout_io(buf_obs, buf_action, buf_value, buf_log_prob, buf_start, buf_reward, obs, reward, done,
                              truncated, terms);
    io.t = (uint32_t)t;
    io.gamma = gamma;
    io.T = 1;
    return launch_rollout(e, "rr_rollout_step", false, params, precision, seed, iter, io, stream);
}

int rr_rollout_collect(rr_env* e, const float* params, int precision, uint64_t seed, const uint64_t* iter,
                       int n_steps, double gamma, double gae_lambda, float* buf_obs, float* buf_action,
                       float* buf_value, float* buf_log_prob, float* buf_start, float* buf_reward,
                       float* buf_advantage, float* buf_return, float* last_value, float* last_done,
                       float* last_start, float* obs, float* reward, uint8_t* done, uint8_t* truncated, float* terms,
                       void* stream)
{
    if (!e) return fail(RR_EINVAL, "rr_rollout_collect: null handle");
    if (n_steps <= 0) return fail(RR_EINVAL, "rr_rollout_collect: n_steps must be positive");
    if ((buf_advantage == nullptr) != (buf_return == nullptr))
        return fail(RR_EINVAL, "rr_rollout_collect: buf_advantage and buf_return go together");
    RolloutIO io = rollout_io(buf_obs, buf_action, buf_value, buf_log_prob, buf_start, buf_reward, obs, reward, done,
                              truncated, terms);
    collect_io(io, n_steps, gamma, gae_lambda, buf_advantage, buf_return, last_value, last_done, last_start);
    return launch_rollout(e, "rr_rollout_collect", true, params, precision, seed, iter, io, stream);
}

int64_t rr_rollout_stats_rows(int64_t n) { return n <= 0 ? 0 : (n + kWave - 1) / kWave; }

int rr_rollout_collect_stats(rr_env* e, const float* params, int precision, uint64_t seed, const uint64_t* iter,
                             int n_steps, double gamma, double gae_lambda, float* buf_obs, float* buf_action,
                             float* buf_value, float* buf_log_prob, float* buf_start, float* buf_reward,
                             float* buf_advantage, float* buf_return, float* last_value, float* last_done,
                             float* last_start, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
                             float* terms, const rr_rollout_stats* stats, void* stream)
{
    const char* who = "rr_rollout_collect_stats";
    const std::string w = std::string(who) + ": ";
    if (!e) return fail(RR_EINVAL, w + "null handle");
    if (n_steps <= 0) return fail(RR_EINVAL, w + "n_steps must be positive");
    if (!stats || !stats->partials || !stats->out) return fail(RR_EINVAL, w + "stats, stats->partials and stats->out must not be null");
    if (((uintptr_t)stats->partials & 127) != 0) return fail(RR_EINVAL, w + "stats->partials must be 128-B aligned");
    if ((((uintptr_t)stats->out | (uintptr_t)stats->accum) & 7) != 0)
        return fail(RR_EINVAL, w + "stats->out and stats->accum must be 8-B aligned");
    if (!buf_advantage || !buf_return)
        return fail(RR_EINVAL, w + "buf_advantage and buf_return are required (the sample sums follow the GAE scan)");
    if (!(e->p.flags & RR_FLAG_EPISODE_STATS))
        return fail(RR_EINVAL, w + "the handle needs RR_FLAG_EPISODE_STATS (the running return crosses launches)");
    if (!(e->p.flags & RR_FLAG_AUTO_RESET))
        return fail(RR_EINVAL, w + "the handle needs RR_FLAG_AUTO_RESET (episodes follow one another)");
    RolloutIO io = rollout_io(buf_obs, buf_action, buf_value, buf_log_prob, buf_start, buf_reward, obs, reward, done,
                              truncated, terms);
    collect_io(io, n_steps, gamma, gae_lambda, buf_advantage, buf_return, last_value, last_done, last_start);
    const CollectStatsIO sio = {(uint64_t*)stats->partials, (uint64_t*)stats->out, (uint64_t*)stats->accum,
                                (uint32_t)rr_rollout_stats_rows(e->n)};
    return launch_rollout(e, who, true, params, precision, seed, iter, io, stream, &sio);
}

namespace {

// rr_policy_evaluate (trace == nullptr), rr_policy_evaluate_trace, rr_policy_evaluate_exact and
// rr_policy_evaluate_exact_trace (`exact`: the handle must be an RR_INT_DOPRI5 one, where the other two
// refuse it; with `traced` it records as rr_policy_evaluate_trace does): the argument checks, the
// kernel's EvalIO and the launch. `who` prefixes every message. `head`: the Categorical policy's calls
// (rr_policy_evaluate_discrete and, traced, rr_policy_evaluate_discrete_trace with its `choice` plane; with
// `exact` and not traced, rr_policy_evaluate_exact_discrete). `sample`: rr_policy_evaluate_sampled and
// rr_policy_evaluate_discrete_sampled (never with `exact`), whose kernels draw the action under that key.
int evaluate(rr_env* e, const char* who, const float* params, int precision, int n_episodes, int64_t max_steps,
             const rr_eval_out* out, bool traced, const rr_eval_trace* trace, float* obs, void* stream,
             bool exact = false, const DiscHead* head = nullptr, int32_t* choice = nullptr,
             const EvalSample* sample = nullptr)
{
    const std::string w = std::string(who) + ": ";
    if (!e) return fail(RR_EINVAL, w + "null handle");
    if (!params || !out || !out->episodes)
        return fail(RR_EINVAL, w + "params, out and out->episodes must not be null");
    const int prec = policy_prec(w, params, precision);
    if (prec < 0) return prec;
    // the trace's own checks come before anything reads the handle
    if (traced) {
        if (!trace) return fail(RR_EINVAL, w + "trace must not be null");
        if (!trace->slot || !trace->state || !trace->length)
            return fail(RR_EINVAL, w + "trace->slot, trace->state and trace->length must not be null");
        if (trace->n_slots < 1 || trace->steps < 1)
            return fail(RR_EINVAL, w + "trace->n_slots and trace->steps must be at least 1");
    }
    if (exact && e->p.integrator != RR_INT_DOPRI5)
        return fail(RR_EINVAL, w + (traced ? "RK4 / Euler envs are evaluated by rr_policy_evaluate_trace"
                                           : "RK4 / Euler envs are evaluated by rr_policy_evaluate"));
    if (!exact && e->p.integrator == RR_INT_DOPRI5)
        return fail(RR_EINVAL, w + "RR_INT_DOPRI5 envs are evaluated step by step (rr_step) or by "
                                   "rr_policy_evaluate_exact");
    if (!(e->p.flags & RR_FLAG_AUTO_RESET))
        return fail(RR_EINVAL, w + "the handle needs RR_FLAG_AUTO_RESET (episodes follow one another)");
    if (n_episodes < 1) return fail(RR_EINVAL, w + "n_episodes must be at least 1");
    if (max_steps <= 0) max_steps = (int64_t)n_episodes * e->p.max_episode_steps;
    if (max_steps <= 0) return fail(RR_EINVAL, w + "an env without a TimeLimit needs max_steps > 0");
    if (sample && max_steps > (int64_t)INT32_MAX)  // the key's t is rr_rollout_step's int
        return fail(RR_EINVAL, w + "max_steps (given or n_episodes * max_episode_steps) must not exceed 2^31 - 1");
    DeviceGuard g(e->device);
    EvalIO io = {};
    io.params = params;
    io.episodes = out->episodes;
    io.ep_return = out->ep_return;
    io.ep_length = out->ep_length;
    io.flags = out->flags;
    io.used_mass = out->used_mass;
    io.final_state = out->final_state;
    io.obs = obs;
    io.max_steps = (uint64_t)max_steps;
    io.n_episodes = n_episodes;
    io.obs_vec_ok = ((uintptr_t)obs & 15u) == 0;
    const Bufs b = bufs_of(e);
    const EnvLaunch L = env_launch(e, prec, &b, stream);  // an auto-reset handle: its mode has kModeCounter
    // the fast modes' kernels are compiled in the collect translation units (rocket_collect.hip,
    // eval_trace/), as the collect kernel they derive from
    hipError_t err;
    EvalTraceIO t = {};
    if (traced) {
        t.slot = trace->slot;
        t.state = trace->state;
        t.action = trace->action;
        t.terms = trace->terms;
        t.length = trace->length;
        t.n_slots = trace->n_slots;
        t.steps = trace->steps;
    }
    if (sample && head) {  // rr_policy_evaluate_discrete_sampled (eval_sampled_discrete/), plain or recording
        err = (hipError_t)rrc_launch_eval_discrete_sampled(&L, &io, head, sample, traced ? &t : nullptr, choice);
    } else if (sample) {  // rr_policy_evaluate_sampled (eval_sampled/), plain or recording
        err = (hipError_t)rrc_launch_eval_sampled(&L, &io, sample, traced ? &t : nullptr);
    } else if (head && exact && !traced) {
        // rr_policy_evaluate_exact_discrete: eval_exact_discrete_kernel (eval_exact_discrete/), eval_exact_kernel's launch
        const EvalExactLaunch X = {e->p.model, prec, L.grid, e->d_xp, &b, e->state64, stream};
        err = (hipError_t)rrx_launch_eval_exact_discrete(&X, &io, head);
    } else if (head && traced) {  // rr_policy_evaluate_discrete_trace (eval_trace_discrete/)
        err = (hipError_t)rrc_launch_eval_discrete_trace(&L, &io, head, &t, choice);
    } else if (head) {  // rr_policy_evaluate_discrete (rollout_discrete/rocket_rollout_discrete.hip)
        err = (hipError_t)rrc_launch_eval_discrete(&L, &io, head);
    } else if (exact) {
        // eval_exact_kernel (eval_exact/rocket_eval_exact.hip): eval_kernel's grid, one variant for every N;
        // traced: eval_exact_trace_kernel (eval_exact_trace/rocket_eval_exact_trace.hip), the same launch
        const EvalExactLaunch X = {e->p.model, prec, L.grid, e->d_xp, &b, e->state64, stream};
        err = (hipError_t)(traced ? rrx_launch_eval_exact_trace(&X, &io, &t) : rrx_launch_eval_exact(&X, &io));
    } else if (traced) {
        err = (hipError_t)rrc_launch_eval_trace(&L, &io, &t);
    } else {
        err = (hipError_t)rrc_launch_eval(&L, &io);
    }
    if (err != hipSuccess) return hip_fail(err, (w + "launch").c_str());
    note_stream(e, stream);
    return RR_OK;
}

}  // namespace

int rr_policy_evaluate(rr_env* e, const float* params, int precision, int n_episodes, int64_t max_steps,
                       const rr_eval_out* out, float* obs, void* stream)
{
    return evaluate(e, "rr_policy_evaluate", params, precision, n_episodes, max_steps, out, false, nullptr, obs, stream);
}

int rr_policy_evaluate_trace(rr_env* e, const float* params, int precision, int n_episodes, int64_t max_steps,
                             const rr_eval_out* out, const rr_eval_trace* trace, float* obs, void* stream)
{
    return evaluate(e, "rr_policy_evaluate_trace", params, precision, n_episodes, max_steps, out, true, trace, obs,
                    stream);
}

int rr_policy_evaluate_exact(rr_env* e, const float* params, int precision, int n_episodes, int64_t max_steps,
                             const rr_eval_out* out, float* obs, void* stream)
{
    return evaluate(e, "rr_policy_evaluate_exact", params, precision, n_episodes, max_steps, out, false, nullptr, obs,
                    stream, true);
}

int rr_policy_evaluate_exact_trace(rr_env* e, const float* params, int precision, int n_episodes, int64_t max_steps,
                                   const rr_eval_out* out, const rr_eval_trace* trace, float* obs, void* stream)
{
    return evaluate(e, "rr_policy_evaluate_exact_trace", params, precision, n_episodes, max_steps, out, true, trace,
                    obs, stream, true);
}

int rr_policy_evaluate_sampled(rr_env* e, const float* params, int precision, uint64_t seed, const uint64_t* iter,
                               int n_episodes, int64_t max_steps, const rr_eval_out* out, const rr_eval_trace* trace,
                               float* obs, void* stream)
{
    const char* who = "rr_policy_evaluate_sampled";
    if (!iter) return refuse(who, "iter must not be null");
    EvalSample S = {};
    act_seed_words(seed, S.seed_lo, S.seed_hi);  // as rr_rollout_step: the same noise key
    S.iter = iter;
    return evaluate(e, who, params, precision, n_episodes, max_steps, out, trace != nullptr, trace, obs, stream, false,
                    nullptr, nullptr, &S);
}

int rr_gae(int64_t T, int64_t n, const float* rewards, const float* values, const float* starts,
           const float* last_value, const float* last_done, double gamma, double lam, float* advantages,
           float* returns, void* stream)
{
    if (!rewards || !values || !starts || !last_value || !last_done || !advantages || !returns || T <= 0 || n <= 0)
        return fail(RR_EINVAL, "rr_gae: null argument or empty rollout");
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       T, n, rewards, values, starts, last_value, last_done, gamma, lam, advantages, returns);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_gae: launch");
}

namespace {
int64_t ppo_nwg(int64_t batch)
{
    const int64_t tiles = (batch + ppo::kTile - 1) / ppo::kTile;
    const int64_t w = (tiles + ppo::kWaves - 1) / ppo::kWaves;
    return w < 1 ? 1 : (w > ppo::kMaxWG ? ppo::kMaxWG : w);
}

LearnerShape gauss_shape(int obs_dim, int act_dim)
{
    if (obs_dim == 14 && act_dim == 3) return shape_of<14, 3>(3, 13);
    if (obs_dim == 7 && act_dim == 2) return shape_of<7, 2>(2, 13);
    return {};
}

// rr_ppo_workspace_size's layout: advantage partial sums | 2 packed tower images | 2 towers x nwg
// partial-gradient vectors (16-B aligned: Pack::SIZE % 4 == 0). What one rr_ppo_update call leaves
// for the next, chained one (the advantage sums, the packed images) sits ahead of the only section
// whose size follows the call's batch: a chained call with a shorter minibatch, and so fewer
// workgroups, finds both where the call before it wrote them.
void ppo_carve(PpoLaunch& L, const LearnerShape& sh, int64_t batch, void* workspace)
{
    L.obs_dim = sh.obs_dim;
    L.nwg = (int)ppo_nwg(batch);
    L.adv_part = (double*)workspace;
    L.pack = (float*)((char*)workspace + 2 * ppo::kAdvPart * sizeof(double));
    L.part = L.pack + 2 * sh.pack;
}

// The finish kernel's squared-gradient sums (two towers) and the step count, in floats, 16-B rows
int64_t norm_floats(const LearnerShape& sh) { return (2 * sh.fin() + 1 + 3) / 4 * 4; }

// rr_bc_update's and rr_bc_update_discrete's workspace: 2 packed tower images | the finish's per-block
// sums and the step count, 16-B rows | the Categorical policy's sink (sink_floats; 0 for the Gaussian) |
// nwg partial-gradient vectors. What a call leaves for the chained one (the images) sits ahead of the
// only section whose size follows the batch, as in ppo_carve.
int64_t bc_fixed_floats(const LearnerShape& sh) { return 2 * sh.pack + norm_floats(sh); }

// the two rr_bc_update*_workspace_size calls' bytes for a shape that passed
int64_t bc_bytes(const LearnerShape& sh, int64_t batch, int64_t sink_floats)
{
    int64_t floats = bc_fixed_floats(sh) + sink_floats + ppo_nwg(batch) * sh.part;
#if defined(RR_DIAG_STAMPS)
    // the shared gradient body writes its stamps past two towers' partial vectors: 16 floats per wave
    floats += ppo_nwg(batch) * (sh.part + ppo::kWaves * 16);
#endif
    return floats * (int64_t)sizeof(float);
}

// The minibatch check of every learner entry point (sized: a *_workspace_size call, `bytes` is required too)
static int learner_batch_ok(const char* who, int64_t batch, const int64_t* bytes, bool sized = true)
{
    if (batch < 2 || (sized && !bytes)) return refuse(who, sized ? "batch >= 2 and bytes required" : "batch >= 2 required");
    return RR_OK;
}

// The shape checks of the Gaussian policy's four *_workspace_size calls and of rr_bc_update
int learner_shape_ok(const char* who, const LearnerShape& sh, int64_t batch, const int64_t* bytes, bool sized = true)
{
    if (!sh.part) return refuse(who, "supported (obs_dim, act_dim) are (14, 3) and (7, 2)");
    return learner_batch_ok(who, batch, bytes, sized);
}

// rr_ppo_workspace_size's bytes for a shape that passed: ppo_carve's three sections
int64_t ppo_bytes(const LearnerShape& sh, int64_t batch)
{
    return (int64_t)(2 * ppo::kAdvPart * sizeof(double)) +
           2 * (ppo_nwg(batch) * sh.part + sh.pack) * (int64_t)sizeof(float);
}

// rr_ppo_update_workspace_size's: + the finish kernel's sums
int64_t ppo_update_bytes(const LearnerShape& sh, int64_t batch)
{
    return (ppo_bytes(sh, batch) + 15) / 16 * 16 + norm_floats(sh) * (int64_t)sizeof(float);
}

// The shape's sh.n policy tensors (rr_policy_pack order) into a launch record; false if one is null. With `a` also the
// optimizer launch's list: each tensor's Adam state and the prefix sums of the sizes (params are then writable)
bool bind_policy(PolSrc& ps, PolGrad& pg, AdamList* a, const LearnerShape& sh, const float* const* params,
                 float* const* grads, float* const* exp_avg = nullptr, float* const* exp_avg_sq = nullptr,
                 float* const* step = nullptr)
{
    if (a) a->n = sh.n;
    for (int k = 0; k < sh.n; ++k) {
        if (!params[k] || !grads[k] || (a && (!exp_avg[k] || !exp_avg_sq[k] || !step[k]))) return false;
        ps.p[k] = params[k];
        pg.p[k] = grads[k];
        if (!a) continue;
        a->param[k] = const_cast<float*>(params[k]);
        a->grad[k] = grads[k];
        a->exp_avg[k] = exp_avg[k];
        a->exp_avg_sq[k] = exp_avg_sq[k];
        a->step[k] = step[k];
        a->start[k + 1] = a->start[k] + sh.numel[k];
        a->wstart[k + 1] = a->wstart[k] + (sh.numel[k] + kWave - 1) / kWave * kWave;
    }
    return true;
}

// Adam's hyper-parameters into a PpoLaunch or a BcLaunch (a generic lambda: no template inside extern "C")
const auto set_adam = [](auto& L, const float* lr, double beta1, double beta2, float eps) {
    L.lr = lr;
    L.beta1 = (float)beta1;
    L.beta2 = (float)beta2;
    L.w1 = (float)(1.0 - beta1);
    L.w2 = (float)(1.0 - beta2);
    L.eps = eps;
};

// The workspace and flag checks of rr_ppo_update, rr_ppo_update_opts and rr_bc_update
int learner_ws_ok(const char* who, const void* workspace, int64_t bytes, int64_t need, uint32_t flags, uint32_t known_flags)
{
    if (!workspace) return refuse(who, "null argument");
    if (bytes < need) return refuse(who, std::string("workspace smaller than ") + who + "_workspace_size");
    if (((uintptr_t)workspace & 15) != 0) return refuse(who, "workspace must be 16-B aligned");
    if (flags & ~known_flags) return refuse(who, "unknown flag bits");
    return RR_OK;
}
}  // namespace

int rr_clip_adam_workspace_size(int64_t total_elements, int64_t* bytes)
{
    if (total_elements < 1 || !bytes) return fail(RR_EINVAL, "rr_clip_adam_workspace_size: total_elements >= 1");
    *bytes = ((total_elements + kAdamThreads - 1) / kAdamThreads + 1) * (int64_t)sizeof(float);
    return RR_OK;
}

int rr_clip_adam(int n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_grad_norm,
                 const float* lr, double beta1, double beta2, float eps, void* workspace, int64_t workspace_bytes,
                 void* stream)
{
    if (n_tensors < 1 || n_tensors > 16) return fail(RR_EINVAL, "rr_clip_adam: 1 .. 16 tensors");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !numel || !lr || !workspace)
        return fail(RR_EINVAL, "rr_clip_adam: null argument");
    AdamList a = {};
    a.n = n_tensors;
    for (int t = 0; t < n_tensors; ++t) {
        if (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t] || !step[t] || numel[t] < 1)
            return fail(RR_EINVAL, "rr_clip_adam: null or empty tensor");
        a.param[t] = params[t];
        a.grad[t] = grads[t];
        a.exp_avg[t] = exp_avg[t];
        a.exp_avg_sq[t] = exp_avg_sq[t];
        a.step[t] = step[t];
        a.start[t + 1] = a.start[t] + numel[t];
    }
    int64_t need = 0;
    rr_clip_adam_workspace_size(a.start[n_tensors], &need);
    if (workspace_bytes < need) return fail(RR_EINVAL, "rr_clip_adam: workspace smaller than rr_clip_adam_workspace_size");
    PpoLaunch L = {};
    L.op = 2;
    L.a = a;
    L.work = (float*)workspace;
    L.max_norm = max_grad_norm;
    set_adam(L, lr, beta1, beta2, eps);
    const hipError_t err = (hipError_t)rrc_launch_learner(&L, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_clip_adam: launch");
}

int rr_ppo_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes)
{
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    const int rc = learner_shape_ok("rr_ppo_workspace_size", sh, batch, bytes);
    if (rc == RR_OK) *bytes = ppo_bytes(sh, batch);
    return rc;
}

int rr_ppo_grad(int obs_dim, int act_dim, const float* const* params, float* const* grads, const float* obs,
                const float* actions, const float* old_log_prob, const float* advantages, const float* returns,
                const int64_t* idx, int64_t batch, float clip_range, float ent_coef, float vf_coef, float* stats,
                void* workspace, int64_t workspace_bytes, void* stream)
{
    int64_t need = 0;
    if (const int rc = rr_ppo_workspace_size(obs_dim, act_dim, batch, &need); rc != RR_OK) return rc;
    if (!params || !grads || !obs || !actions || !old_log_prob || !advantages || !returns || !idx || !workspace)
        return fail(RR_EINVAL, "rr_ppo_grad: null argument");
    if (workspace_bytes < need) return fail(RR_EINVAL, "rr_ppo_grad: workspace smaller than rr_ppo_workspace_size");
    if (((uintptr_t)workspace & 15) != 0) return fail(RR_EINVAL, "rr_ppo_grad: workspace must be 16-B aligned");
    if (!(clip_range >= 0.0f)) return fail(RR_EINVAL, "rr_ppo_grad: clip_range must be >= 0");
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    PpoLaunch L = {};
    L.op = 0;
    if (!bind_policy(L.ps, L.pg, nullptr, sh, params, grads))
        return fail(RR_EINVAL, "rr_ppo_grad: null parameter or gradient tensor");
    ppo_carve(L, sh, batch, workspace);
    L.obs = obs;
    L.actions = actions;
    L.old_log_prob = old_log_prob;
    L.advantages = advantages;
    L.returns = returns;
    L.idx = idx;
    L.batch = batch;
    L.clip = clip_range;
    L.ent = ent_coef;
    L.vf = vf_coef;
    L.stats = stats;
    const hipError_t err = (hipError_t)rrc_launch_learner(&L, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_ppo_grad: launch");
}

int rr_ppo_update_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes)
{
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    const int rc = learner_shape_ok("rr_ppo_update_workspace_size", sh, batch, bytes);
    if (rc == RR_OK) *bytes = ppo_update_bytes(sh, batch);
    return rc;
}

namespace {
// rr_ppo_update's argument checks and launch record, for it, rr_ppo_update_opts and rr_ppo_update_discrete
// (`who` names the entry point in the error text, known_flags its flag bits; ws_need its workspace size)
int ppo_update_record(const char* who, PpoLaunch& L, const LearnerShape& sh, float* const* params,
                      float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, float* const* step,
                      const float* obs, const float* actions, const float* old_log_prob, const float* advantages,
                      const float* returns, const int64_t* idx, int64_t batch, const int64_t* next_idx,
                      int64_t next_batch, float clip_range, float ent_coef, float vf_coef, float max_grad_norm,
                      const float* lr, double beta1, double beta2, float eps, float* stats, uint32_t flags,
                      uint32_t known_flags, void* workspace, int64_t workspace_bytes, int64_t ws_need)
{
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !obs || !actions || !old_log_prob || !advantages ||
        !returns || !idx || !lr)
        return refuse(who, "null argument");
    const int rc = learner_ws_ok(who, workspace, workspace_bytes, ws_need, flags, known_flags);
    if (rc != RR_OK) return rc;
    if (!(clip_range >= 0.0f)) return refuse(who, "clip_range must be >= 0");
    if (next_idx && !(next_batch >= 2 && next_batch <= batch)) return refuse(who, "next_batch must be in [2, batch]");
    L = {};
    L.op = 1;
    if (!bind_policy(L.ps, L.pg, &L.a, sh, params, grads, exp_avg, exp_avg_sq, step))
        return refuse(who, "null parameter, gradient or optimizer-state tensor");
    ppo_carve(L, sh, batch, workspace);
    L.normw = (float*)((char*)workspace + (ppo_bytes(sh, batch) + 15) / 16 * 16);
    L.nbp = (int)((L.a.wstart[sh.n] + kAdamThreads - 1) / kAdamThreads);
    L.obs = obs;
    L.actions = actions;
    L.old_log_prob = old_log_prob;
    L.advantages = advantages;
    L.returns = returns;
    L.idx = idx;
    L.next_idx = next_idx;
    L.batch = batch;
    L.next_batch = next_batch;
    L.clip = clip_range;
    L.ent = ent_coef;
    L.vf = vf_coef;
    L.max_norm = max_grad_norm;
    set_adam(L, lr, beta1, beta2, eps);
    L.stats = stats;
    L.flags = flags & RR_PPO_CHAINED;
    return RR_OK;
}

// The option checks of rr_ppo_update_opts and rr_ppo_update_discrete_opts and the options' fields of their
// launch records (a generic lambda: no template inside extern "C")
const auto ppo_options_record = [](const char* who, auto& O, const rr_ppo_options* options, const float* old_values,
                                   float* control, uint32_t flags) {
    if (!options) return refuse(who, "null options");
    // NaN fails both comparisons' complements: !(x >= 0) is true for NaN and for negatives
    if (!(options->clip_range_vf >= 0.0f)) return refuse(who, "clip_range_vf must be >= 0 (0: off)");
    if (!(options->target_kl >= 0.0f)) return refuse(who, "target_kl must be >= 0 (0: off)");
    if (options->clip_range_vf > 0.0f && !old_values) return refuse(who, "clip_range_vf needs old_values");
    if (options->target_kl > 0.0f && !control) return refuse(who, "target_kl needs a control block");
    if (options->train_stats && !control) return refuse(who, "train_stats needs a control block");
    if (((uintptr_t)control & 15) != 0) return refuse(who, "control block must be 16-B aligned");
    O.old_values = old_values;
    O.clip_vf = options->clip_range_vf;
    O.normalize = options->normalize_advantage != 0;
    O.ctl.ctl = control;
    O.ctl.kl_limit = options->target_kl > 0.0f ? 1.5f * options->target_kl : HUGE_VALF;
    O.ctl.epoch_start = (flags & RR_PPO_EPOCH_START) != 0;
    return (int)RR_OK;
};
}  // namespace

int rr_ppo_update(int obs_dim, int act_dim, float* const* params, float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, float* const* step, const float* obs, const float* actions,
                  const float* old_log_prob, const float* advantages, const float* returns, const int64_t* idx,
                  int64_t batch, const int64_t* next_idx, int64_t next_batch, float clip_range, float ent_coef,
                  float vf_coef, float max_grad_norm, const float* lr, double beta1, double beta2, float eps,
                  float* stats, uint32_t flags, void* workspace, int64_t workspace_bytes, void* stream)
{
    int64_t need = 0;
    if (const int rc = rr_ppo_update_workspace_size(obs_dim, act_dim, batch, &need); rc != RR_OK) return rc;
    PpoLaunch L;
    const int rc = ppo_update_record("rr_ppo_update", L, gauss_shape(obs_dim, act_dim), params, grads, exp_avg,
                                     exp_avg_sq, step, obs, actions, old_log_prob, advantages, returns, idx, batch,
                                     next_idx, next_batch, clip_range, ent_coef, vf_coef, max_grad_norm, lr, beta1, beta2,
                                     eps, stats, flags, RR_PPO_CHAINED, workspace, workspace_bytes, need);
    if (rc != RR_OK) return rc;
    const hipError_t err = (hipError_t)rrc_launch_learner(&L, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_ppo_update: launch");
}

static_assert(ppo::kStop == RR_PPO_CTL_STOP && ppo::kDecide == RR_PPO_CTL_DECIDE && ppo::kSteps == RR_PPO_CTL_STEPS &&
                  ppo::kEvals == RR_PPO_CTL_EVALS && ppo::kEpochs == RR_PPO_CTL_EPOCHS &&
                  ppo::kSumPg == RR_PPO_CTL_SUM_POLICY && ppo::kSumVf == RR_PPO_CTL_SUM_VALUE &&
                  ppo::kSumEnt == RR_PPO_CTL_SUM_ENTROPY && ppo::kSumClip == RR_PPO_CTL_SUM_CLIP &&
                  ppo::kKlSum == RR_PPO_CTL_KL_SUM && ppo::kKlCount == RR_PPO_CTL_KL_COUNT &&
                  ppo::kKlLast == RR_PPO_CTL_KL_LAST && ppo::kKlLast < RR_PPO_CTL_SLOTS,
              "the kernels' control-block slots are the header's");

int rr_ppo_update_opts_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes)
{
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    const int rc = learner_shape_ok("rr_ppo_update_opts_workspace_size", sh, batch, bytes);
    // + 8 floats: the call's statistics when the caller passes none (the control block sums them)
    if (rc == RR_OK) *bytes = ppo_update_bytes(sh, batch) + 32;
    return rc;
}

int rr_ppo_update_opts(int obs_dim, int act_dim, float* const* params, float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, float* const* step, const float* obs, const float* actions,
                       const float* old_log_prob, const float* advantages, const float* returns,
                       const float* old_values, const int64_t* idx, int64_t batch, const int64_t* next_idx,
                       int64_t next_batch, float clip_range, float ent_coef, float vf_coef, float max_grad_norm,
                       const float* lr, double beta1, double beta2, float eps, const rr_ppo_options* options,
                       float* control, float* stats, uint32_t flags, void* workspace, int64_t workspace_bytes,
                       void* stream)
{
    int64_t need = 0;
    if (const int rc = rr_ppo_update_opts_workspace_size(obs_dim, act_dim, batch, &need); rc != RR_OK) return rc;
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    PpoOptsLaunch O = {};
    const int rc = ppo_update_record("rr_ppo_update_opts", O.base, sh, params, grads, exp_avg, exp_avg_sq, step,
                                     obs, actions, old_log_prob, advantages, returns, idx, batch, next_idx, next_batch,
                                     clip_range, ent_coef, vf_coef, max_grad_norm, lr, beta1, beta2, eps, stats, flags,
                                     RR_PPO_CHAINED | RR_PPO_EPOCH_START, workspace, workspace_bytes, need);
    if (rc != RR_OK) return rc;
    if (const int rc2 = ppo_options_record("rr_ppo_update_opts", O, options, old_values, control, flags); rc2 != RR_OK)
        return rc2;
    if (!stats) O.base.stats = (float*)((char*)workspace + ppo_update_bytes(sh, batch));
    const hipError_t err = (hipError_t)rrc_launch_learner_opts(&O, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_ppo_update_opts: launch");
}

namespace {
// The argument checks and launch record of rr_bc_update and rr_bc_update_discrete, for a shape and batch that
// passed (`who` names the entry point in the error text; sink_floats is the Categorical policy's sink and
// log_std slot, 0 for the Gaussian)
static int bc_update_record(const char* who, BcLaunch& L, const LearnerShape& sh, int64_t sink_floats, float* const* params,
                     float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, float* const* step,
                     const float* obs, const float* actions, const int64_t* idx, int64_t batch, float ent_weight,
                     float l2_weight, const float* lr, double beta1, double beta2, float eps, float* stats,
                     uint32_t flags, void* workspace, int64_t workspace_bytes)
{
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step || !obs || !actions || !idx || !lr)
        return refuse(who, "null argument");
    const int rc = learner_ws_ok(who, workspace, workspace_bytes, bc_bytes(sh, batch, sink_floats), flags, RR_BC_CHAINED);
    if (rc != RR_OK) return rc;
    // NaN fails the comparison too
    if (!(ent_weight >= 0.0f)) return refuse(who, "ent_weight must be >= 0");
    if (!(l2_weight >= 0.0f)) return refuse(who, "l2_weight must be >= 0");
    L = {};
    if (!bind_policy(L.ps, L.pg, &L.a, sh, params, grads, exp_avg, exp_avg_sq, step))
        return refuse(who, "null parameter, gradient or optimizer-state tensor");
    L.obs_dim = sh.obs_dim;
    L.nwg = (int)ppo_nwg(batch);
    L.pack = (float*)workspace;
    L.normw = L.pack + 2 * sh.pack;
    L.sink = sink_floats ? L.pack + bc_fixed_floats(sh) : nullptr;
    L.part = L.pack + bc_fixed_floats(sh) + sink_floats;
    L.nbp = (int)((L.a.wstart[sh.n] + kAdamThreads - 1) / kAdamThreads);
    L.obs = obs;
    L.actions = actions;
    L.idx = idx;
    L.batch = batch;
    L.ent = ent_weight;
    L.l2 = l2_weight;
    set_adam(L, lr, beta1, beta2, eps);
    L.stats = stats;
    L.flags = flags;
    return RR_OK;
}
}  // namespace

int rr_bc_update_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes)
{
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    const int rc = learner_shape_ok("rr_bc_update_workspace_size", sh, batch, bytes);
    if (rc == RR_OK) *bytes = bc_bytes(sh, batch, 0);
    return rc;
}

int rr_bc_update(int obs_dim, int act_dim, float* const* params, float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, float* const* step, const float* obs, const float* actions,
                 const int64_t* idx, int64_t batch, float ent_weight, float l2_weight, const float* lr,
                 double beta1, double beta2, float eps, float* stats, uint32_t flags,
                 void* workspace, int64_t workspace_bytes, void* stream)
{
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    if (const int rc = learner_shape_ok("rr_bc_update", sh, batch, nullptr, false); rc != RR_OK) return rc;
    BcLaunch L;
    const int rc = bc_update_record("rr_bc_update", L, sh, 0, params, grads, exp_avg, exp_avg_sq, step, obs, actions, idx,
                                    batch, ent_weight, l2_weight, lr, beta1, beta2, eps, stats, flags, workspace,
                                    workspace_bytes);
    if (rc != RR_OK) return rc;
    const hipError_t err = (hipError_t)rrc_launch_bc(&L, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_bc_update: launch");
}

// ---- A2C (a2c/rocket_a2c.hip): the workspace is rr_ppo_update's (ppo_carve's sections and the finish's sums) ----
int rr_a2c_update_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes)
{
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    const int rc = learner_shape_ok("rr_a2c_update_workspace_size", sh, batch, bytes);
    if (rc == RR_OK) *bytes = ppo_update_bytes(sh, batch);
    return rc;
}

namespace {
// rr_a2c_update's and rr_a2c_update_discrete's checks after the shape's (nothing is launched before they
// pass) and the launch record over the shape's tensors; ws_need is the call's *_workspace_size, whose first
// ppo_update_bytes are carved here (the Categorical call's sink follows them).
int a2c_update_record(const char* who, A2cLaunch& L, const LearnerShape& sh, float* const* params, float* const* grads,
                      float* const* square_avg, float* const* exp_avg, float* const* step, const float* obs,
                      const float* actions, const float* advantages, const float* returns, const int64_t* idx,
                      int64_t batch, int normalize_advantage, float ent_coef, float vf_coef, float max_grad_norm,
                      int optimizer, const float* lr, double alpha_or_beta1, double beta2, float eps, float* stats,
                      void* workspace, int64_t workspace_bytes, int64_t ws_need)
{
    if (optimizer != RR_A2C_RMSPROP && optimizer != RR_A2C_RMSPROP_TF && optimizer != RR_A2C_ADAM)
        return refuse(who, "optimizer must be RR_A2C_RMSPROP, RR_A2C_RMSPROP_TF or RR_A2C_ADAM");
    const bool adam = optimizer == RR_A2C_ADAM;
    if (!params || !grads || !square_avg || (adam && !exp_avg) || !step || !obs || !actions || !advantages || !returns ||
        !idx || !lr)
        return refuse(who, "null argument");
    if (const int rc = learner_ws_ok(who, workspace, workspace_bytes, ws_need, 0, 0); rc != RR_OK) return rc;
    // NaN fails every comparison: !(x >= 0 && x < inf) is true for NaN, negatives and infinities
    if (!(ent_coef >= 0.0f && ent_coef < HUGE_VALF)) return refuse(who, "ent_coef must be finite and >= 0");
    if (!(vf_coef >= 0.0f && vf_coef < HUGE_VALF)) return refuse(who, "vf_coef must be finite and >= 0");
    if (!(max_grad_norm >= 0.0f && max_grad_norm < HUGE_VALF))
        return refuse(who, "max_grad_norm must be finite and >= 0 (0: no clip)");
    if (!(eps >= 0.0f && eps < HUGE_VALF)) return refuse(who, "eps must be finite and >= 0");
    if (!(alpha_or_beta1 >= 0.0 && alpha_or_beta1 < 1.0))
        return refuse(who, adam ? "beta1 must be in [0, 1)" : "alpha must be in [0, 1)");
    if (adam && !(beta2 >= 0.0 && beta2 < 1.0)) return refuse(who, "beta2 must be in [0, 1)");
    L = {};
    // RMSprop has no first moment: the list's exp_avg slots are bound to square_avg and never read
    if (!bind_policy(L.ps, L.pg, &L.a, sh, params, grads, adam ? exp_avg : square_avg, square_avg, step))
        return refuse(who, "null parameter, gradient or optimizer-state tensor");
    if (!adam)
        for (int k = 0; k < sh.n; ++k) L.a.exp_avg[k] = nullptr;
    L.obs_dim = sh.obs_dim;
    L.nwg = (int)ppo_nwg(batch);
    L.adv_part = (double*)workspace;
    L.pack = (float*)((char*)workspace + 2 * ppo::kAdvPart * sizeof(double));
    L.part = L.pack + 2 * sh.pack;
    L.normw = (float*)((char*)workspace + (ppo_bytes(sh, batch) + 15) / 16 * 16);
    L.nbp = (int)((L.a.wstart[sh.n] + kAdamThreads - 1) / kAdamThreads);
    L.obs = obs;
    L.actions = actions;
    L.advantages = advantages;
    L.returns = returns;
    L.idx = idx;
    L.batch = batch;
    L.normalize = normalize_advantage != 0;
    L.ent = ent_coef;
    L.vf = vf_coef;
    L.max_norm = max_grad_norm;
    L.optimizer = optimizer;
    L.lr = lr;
    L.eps = eps;
    if (adam) {
        set_adam(L, lr, alpha_or_beta1, beta2, eps);
    } else {
        L.alpha = (float)alpha_or_beta1;
        L.w1 = (float)(1.0 - alpha_or_beta1);
    }
    L.stats = stats;
    return RR_OK;
}
}  // namespace

int rr_a2c_update(int obs_dim, int act_dim, float* const* params, float* const* grads, float* const* square_avg,
                  float* const* exp_avg, float* const* step, const float* obs, const float* actions,
                  const float* advantages, const float* returns, const int64_t* idx, int64_t batch,
                  int normalize_advantage, float ent_coef, float vf_coef, float max_grad_norm, int optimizer,
                  const float* lr, double alpha_or_beta1, double beta2, float eps, float* stats,
                  void* workspace, int64_t workspace_bytes, void* stream)
{
    const char* who = "rr_a2c_update";
    const LearnerShape sh = gauss_shape(obs_dim, act_dim);
    if (const int rc = learner_shape_ok(who, sh, batch, nullptr, false); rc != RR_OK) return rc;
    A2cLaunch L;
    const int rc = a2c_update_record(who, L, sh, params, grads, square_avg, exp_avg, step, obs, actions, advantages,
                                     returns, idx, batch, normalize_advantage, ent_coef, vf_coef, max_grad_norm, optimizer,
                                     lr, alpha_or_beta1, beta2, eps, stats, workspace, workspace_bytes,
                                     ppo_update_bytes(sh, batch));
    if (rc != RR_OK) return rc;
    const hipError_t err = (hipError_t)rrc_launch_a2c(&L, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_a2c_update: launch");
}

// ---- the Categorical policy (discrete/rocket_discrete.hip): obs_dim 7, 2 .. 4 choices on <7, 4> images ----
namespace {
constexpr int64_t kDiscSink = 64 * 4 + 4 + 4;  // floats: heads >= n_choices' weight and bias sums, log_std's slot

int disc_shape_ok(const char* who, int obs_dim, int n_choices)
{
    if (obs_dim != 7) return refuse(who, "obs_dim must be 7 (the 3DOF env)");
    if (n_choices < 2 || n_choices > 4) return refuse(who, "n_choices must be in 2 .. 4");
    return RR_OK;
}

// learner_shape_ok for the Categorical policy's learner calls
static int disc_learner_ok(const char* who, int obs_dim, int n_choices, int64_t batch, const int64_t* bytes, bool sized = true)
{
    if (const int rc = disc_shape_ok(who, obs_dim, n_choices); rc != RR_OK) return rc;
    return learner_batch_ok(who, batch, bytes, sized);
}

// The <7, 4> image with n_choices action-head rows over the 12 tensors of a policy without a log_std
LearnerShape disc_shape(int n_choices) { return shape_of<7, 4>(n_choices, 12); }
}  // namespace

int rr_policy_layout_discrete(int obs_dim, int64_t* off)
{
    if (obs_dim != 7) return fail(RR_EINVAL, "rr_policy_layout_discrete: obs_dim must be 7 (the 3DOF env)");
    return layout_offsets<pol::Layout<7, 4, 0>>(off);
}

int rr_policy_pack_discrete(int obs_dim, int n_choices, const float* const* src, float* params, void* stream)
{
    if (const int rc = disc_shape_ok("rr_policy_pack_discrete", obs_dim, n_choices); rc != RR_OK) return rc;
    if (!src || !params) return fail(RR_EINVAL, "rr_policy_pack_discrete: null argument");
    DiscreteLaunch D = {};
    D.op = kDiscPack;
    D.n_choices = n_choices;
    for (int k = 0; k < 12; ++k) {
        if (!src[k]) return fail(RR_EINVAL, "rr_policy_pack_discrete: null parameter tensor");
        D.u.ps.p[k] = src[k];
    }
    D.u.pack = params;
    D.n = 1;
    const hipError_t err = (hipError_t)rrc_launch_discrete(&D, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_policy_pack_discrete: launch");
}

int rr_policy_act_discrete(const float* params, int obs_dim, int n_choices, const float* table, int precision,
                           int64_t n, int64_t env_id_offset, const float* obs, uint64_t seed, const uint64_t* iter,
                           int t, float* action_env, float* action, float* value, float* log_prob, float* obs_copy,
                           const float* prev_term_obs, const uint8_t* prev_truncated, const float* prev_reward,
                           float gamma, float* reward_out, const uint8_t* done, float* start_out, void* stream)
{
    const char* who = "rr_policy_act_discrete";
    if (const int rc = disc_shape_ok(who, obs_dim, n_choices); rc != RR_OK) return rc;
    if (precision != RR_POLICY_FP32) return refuse(who, "precision must be RR_POLICY_FP32");
    if (const int rc = act_args_ok(who, params, table, obs, iter, action_env, action, value, log_prob, n, prev_term_obs,
                                   prev_truncated, prev_reward, reward_out, done, start_out);
        rc != RR_OK)
        return rc;
    DiscreteLaunch D = {};
    D.op = kDiscAct;
    D.n_choices = n_choices;
    for (int k = 0; k < n_choices; ++k)
        for (int c = 0; c < 2; ++c) {
            if (!std::isfinite(table[2 * k + c])) return refuse(who, "table entries must be finite");
            D.table[k][c] = table[2 * k + c];
        }
    act_seed_words(seed, D.seed_lo, D.seed_hi);  // as rr_policy_act: the same noise key
    D.params = params;
    D.n = n;
    D.id_off = env_id_offset;
    D.obs = obs;
    D.iter = iter;
    D.t = (uint32_t)t;
    D.act_env = action_env;
    D.act = action;
    D.value = value;
    D.logp = log_prob;
    D.obs_copy = obs_copy;
    D.prev_term_obs = prev_term_obs;
    D.prev_trunc = prev_truncated;
    D.prev_reward = prev_reward;
    D.gamma = gamma;
    D.reward_out = reward_out;
    D.done = done;
    D.start_out = start_out;
    const hipError_t err = (hipError_t)rrc_launch_discrete(&D, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_policy_act_discrete: launch");
}

namespace {
// What rr_rollout_step_discrete, rr_rollout_collect_discrete and rr_policy_evaluate_discrete check besides
// their Gaussian twins' checks, before any HIP call. The arguments first, so that they are refused
// whatever the handle is, then the handle; `H` receives the kernels' head.
int disc_head_args(const char* who, const float* params, int n_choices, const float* table, int precision, DiscHead& H)
{
    if (precision != RR_POLICY_FP32) return refuse(who, "precision must be RR_POLICY_FP32");
    if (n_choices < 2 || n_choices > 4) return refuse(who, "n_choices must be in 2 .. 4");
    if (!table) return refuse(who, "table must not be null");
    H = {};
    H.n_choices = n_choices;
    for (int k = 0; k < n_choices; ++k)
        for (int c = 0; c < 2; ++c) {
            if (!std::isfinite(table[2 * k + c])) return refuse(who, "table entries must be finite");
            H.table[k][c] = table[2 * k + c];
        }
    if (!params) return refuse(who, "params must not be null");
    if (((uintptr_t)params & 15) != 0) return refuse(who, "params must be 16-B aligned");
    return RR_OK;
}
// `exact`: rr_policy_evaluate_exact_discrete, which takes the RR_INT_DOPRI5 handles the others refuse
int disc_handle_ok(const char* who, const rr_env* e, bool exact = false)
{
    if (!e) return refuse(who, "null handle");
    if (e->p.model != RR_MODEL_3DOF)
        return refuse(who, "a 6DOF handle is refused: the table rows are [gimbal, thrust] of the 3DOF env");
    if (exact && e->p.integrator != RR_INT_DOPRI5)
        return refuse(who, "RK4 / Euler envs are evaluated by rr_policy_evaluate_discrete");
    if (!exact && e->p.integrator == RR_INT_DOPRI5)
        return refuse(who, "RR_INT_DOPRI5 envs step through rr_policy_act_discrete + rr_step");
    return RR_OK;
}
int disc_rollout_bufs_ok(const char* who, const uint64_t* iter, const RolloutIO& io)
{
    if (!iter || !io.buf_obs || !io.buf_act || !io.buf_val || !io.buf_logp || !io.buf_start || !io.buf_rew ||
        !io.reward || !io.done)
        return refuse(who, "null argument");
    return RR_OK;
}
}  // namespace

int rr_rollout_step_discrete(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                             uint64_t seed, const uint64_t* iter, int t, float gamma, float* buf_obs,
                             float* buf_action, float* buf_value, float* buf_log_prob, float* buf_start,
                             float* buf_reward, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
                             float* terms, void* stream)
{
    const char* who = "rr_rollout_step_discrete";
    DiscHead H;
    if (const int rc = disc_head_args(who, params, n_choices, table, precision, H); rc != RR_OK) return rc;
    RolloutIO io = rollout_io(buf_obs, buf_action, buf_value, buf_log_prob, buf_start, buf_reward, obs, reward, done,
                              truncated, terms);
    if (const int rc = disc_rollout_bufs_ok(who, iter, io); rc != RR_OK) return rc;
    if (const int rc = disc_handle_ok(who, e); rc != RR_OK) return rc;
    io.t = (uint32_t)t;
    io.gamma = gamma;
    io.T = 1;
    return launch_rollout(e, who, false, params, precision, seed, iter, io, stream, nullptr, &H);
}

int rr_rollout_collect_discrete(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                uint64_t seed, const uint64_t* iter, int n_steps, double gamma, double gae_lambda,
                                float* buf_obs, float* buf_action, float* buf_value, float* buf_log_prob,
                                float* buf_start, float* buf_reward, float* buf_advantage, float* buf_return,
                                float* last_value, float* last_done, float* last_start, float* obs, float* reward,
                                uint8_t* done, uint8_t* truncated, float* terms, void* stream)
{
    const char* who = "rr_rollout_collect_discrete";
    DiscHead H;
    if (const int rc = disc_head_args(who, params, n_choices, table, precision, H); rc != RR_OK) return rc;
    if (n_steps <= 0) return refuse(who, "n_steps must be positive");
    if ((buf_advantage == nullptr) != (buf_return == nullptr))
        return refuse(who, "buf_advantage and buf_return go together");
    RolloutIO io = rollout_io(buf_obs, buf_action, buf_value, buf_log_prob, buf_start, buf_reward, obs, reward, done,
                              truncated, terms);
    if (const int rc = disc_rollout_bufs_ok(who, iter, io); rc != RR_OK) return rc;
    if (const int rc = disc_handle_ok(who, e); rc != RR_OK) return rc;
    collect_io(io, n_steps, gamma, gae_lambda, buf_advantage, buf_return, last_value, last_done, last_start);
    return launch_rollout(e, who, true, params, precision, seed, iter, io, stream, nullptr, &H);
}

int rr_policy_evaluate_discrete(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                int n_episodes, int64_t max_steps, const rr_eval_out* out, float* obs, void* stream)
{
    const char* who = "rr_policy_evaluate_discrete";
    DiscHead H;
    if (const int rc = disc_head_args(who, params, n_choices, table, precision, H); rc != RR_OK) return rc;
    if (!out || !out->episodes) return refuse(who, "params, out and out->episodes must not be null");
    if (n_episodes < 1) return refuse(who, "n_episodes must be at least 1");
    if (const int rc = disc_handle_ok(who, e); rc != RR_OK) return rc;
    return evaluate(e, who, params, precision, n_episodes, max_steps, out, false, nullptr, obs, stream, false, &H);
}

int rr_policy_evaluate_exact_discrete(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                      int n_episodes, int64_t max_steps, const rr_eval_out* out, float* obs,
                                      void* stream)
{
    // rr_policy_evaluate_discrete's refusals with the integrator's turned round; the arguments before the handle
    const char* who = "rr_policy_evaluate_exact_discrete";
    DiscHead H;
    if (const int rc = disc_head_args(who, params, n_choices, table, precision, H); rc != RR_OK) return rc;
    if (!out || !out->episodes) return refuse(who, "params, out and out->episodes must not be null");
    if (n_episodes < 1) return refuse(who, "n_episodes must be at least 1");
    if (const int rc = disc_handle_ok(who, e, true); rc != RR_OK) return rc;
    return evaluate(e, who, params, precision, n_episodes, max_steps, out, false, nullptr, obs, stream, true, &H);
}

int rr_rollout_collect_discrete_stats(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                      uint64_t seed, const uint64_t* iter, int n_steps, double gamma,
                                      double gae_lambda, float* buf_obs, float* buf_action, float* buf_value,
                                      float* buf_log_prob, float* buf_start, float* buf_reward, float* buf_advantage,
                                      float* buf_return, float* last_value, float* last_done, float* last_start,
                                      float* obs, float* reward, uint8_t* done, uint8_t* truncated, float* terms,
                                      const rr_rollout_stats* stats, void* stream)
{
    // rr_rollout_collect_discrete's refusals, then rr_rollout_collect_stats's; the arguments before the handle
    const char* who = "rr_rollout_collect_discrete_stats";
    DiscHead H;
    if (const int rc = disc_head_args(who, params, n_choices, table, precision, H); rc != RR_OK) return rc;
    if (n_steps <= 0) return refuse(who, "n_steps must be positive");
    if (!stats || !stats->partials || !stats->out)
        return refuse(who, "stats, stats->partials and stats->out must not be null");
    if (((uintptr_t)stats->partials & 127) != 0) return refuse(who, "stats->partials must be 128-B aligned");
    if ((((uintptr_t)stats->out | (uintptr_t)stats->accum) & 7) != 0)
        return refuse(who, "stats->out and stats->accum must be 8-B aligned");
    if (!buf_advantage || !buf_return)
        return refuse(who, "buf_advantage and buf_return are required (the sample sums follow the GAE scan)");
    RolloutIO io = rollout_io(buf_obs, buf_action, buf_value, buf_log_prob, buf_start, buf_reward, obs, reward, done,
                              truncated, terms);
    if (const int rc = disc_rollout_bufs_ok(who, iter, io); rc != RR_OK) return rc;
    if (const int rc = disc_handle_ok(who, e); rc != RR_OK) return rc;
    if (!(e->p.flags & RR_FLAG_EPISODE_STATS))
        return refuse(who, "the handle needs RR_FLAG_EPISODE_STATS (the running return crosses launches)");
    if (!(e->p.flags & RR_FLAG_AUTO_RESET))
        return refuse(who, "the handle needs RR_FLAG_AUTO_RESET (episodes follow one another)");
    collect_io(io, n_steps, gamma, gae_lambda, buf_advantage, buf_return, last_value, last_done, last_start);
    const CollectStatsIO sio = {(uint64_t*)stats->partials, (uint64_t*)stats->out, (uint64_t*)stats->accum,
                                (uint32_t)rr_rollout_stats_rows(e->n)};
    return launch_rollout(e, who, true, params, precision, seed, iter, io, stream, &sio, &H);
}

int rr_policy_evaluate_discrete_trace(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                      int n_episodes, int64_t max_steps, const rr_eval_out* out,
                                      const rr_eval_trace* trace, int32_t* choice, float* obs, void* stream)
{
    // rr_policy_evaluate_discrete's refusals, then rr_policy_evaluate_trace's; the arguments before the handle
    const char* who = "rr_policy_evaluate_discrete_trace";
    DiscHead H;
    if (const int rc = disc_head_args(who, params, n_choices, table, precision, H); rc != RR_OK) return rc;
    if (!out || !out->episodes) return refuse(who, "params, out and out->episodes must not be null");
    if (n_episodes < 1) return refuse(who, "n_episodes must be at least 1");
    if (!trace) return refuse(who, "trace must not be null");
    if (!trace->slot || !trace->state || !trace->length)
        return refuse(who, "trace->slot, trace->state and trace->length must not be null");
    if (trace->n_slots < 1 || trace->steps < 1) return refuse(who, "trace->n_slots and trace->steps must be at least 1");
    if (((uintptr_t)choice & 3) != 0) return refuse(who, "choice must be 4-B aligned");
    if (const int rc = disc_handle_ok(who, e); rc != RR_OK) return rc;
    return evaluate(e, who, params, precision, n_episodes, max_steps, out, true, trace, obs, stream, false, &H, choice);
}

int rr_policy_evaluate_discrete_sampled(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                        uint64_t seed, const uint64_t* iter, int n_episodes, int64_t max_steps,
                                        const rr_eval_out* out, const rr_eval_trace* trace, int32_t* choice, float* obs,
                                        void* stream)
{
    // rr_policy_evaluate_discrete's refusals, with a trace rr_policy_evaluate_discrete_trace's, and the key's; the
    // arguments before the handle
    const char* who = "rr_policy_evaluate_discrete_sampled";
    DiscHead H;
    if (const int rc = disc_head_args(who, params, n_choices, table, precision, H); rc != RR_OK) return rc;
    if (!iter) return refuse(who, "iter must not be null");
    if (!out || !out->episodes) return refuse(who, "params, out and out->episodes must not be null");
    if (n_episodes < 1) return refuse(who, "n_episodes must be at least 1");
    if (trace) {
        if (!trace->slot || !trace->state || !trace->length)
            return refuse(who, "trace->slot, trace->state and trace->length must not be null");
        if (trace->n_slots < 1 || trace->steps < 1)
            return refuse(who, "trace->n_slots and trace->steps must be at least 1");
        if (((uintptr_t)choice & 3) != 0) return refuse(who, "choice must be 4-B aligned");
    } else if (choice) {
        return refuse(who, "choice needs trace (the indices are recorded beside the action rows)");
    }
    if (const int rc = disc_handle_ok(who, e); rc != RR_OK) return rc;
    EvalSample S = {};
    act_seed_words(seed, S.seed_lo, S.seed_hi);  // as rr_rollout_step_discrete: the same noise key
    S.iter = iter;
    return evaluate(e, who, params, precision, n_episodes, max_steps, out, trace != nullptr, trace, obs, stream, false,
                    &H, choice, &S);
}

int rr_ppo_update_discrete_workspace_size(int obs_dim, int n_choices, int64_t batch, int64_t* bytes)
{
    const int rc = disc_learner_ok("rr_ppo_update_discrete_workspace_size", obs_dim, n_choices, batch, bytes);
    // rr_ppo_update's sections (ppo_carve, the finish's sums), then the sink
    if (rc == RR_OK) *bytes = ppo_update_bytes(disc_shape(n_choices), batch) + kDiscSink * (int64_t)sizeof(float);
    return rc;
}

int rr_ppo_update_discrete(int obs_dim, int n_choices, float* const* params, float* const* grads,
                           float* const* exp_avg, float* const* exp_avg_sq, float* const* step, const float* obs,
                           const float* actions, const float* old_log_prob, const float* advantages,
                           const float* returns, const int64_t* idx, int64_t batch, const int64_t* next_idx,
                           int64_t next_batch, float clip_range, float ent_coef, float vf_coef, float max_grad_norm,
                           const float* lr, double beta1, double beta2, float eps, float* stats, uint32_t flags,
                           void* workspace, int64_t workspace_bytes, void* stream)
{
    const char* who = "rr_ppo_update_discrete";
    if (const int rc = disc_learner_ok(who, obs_dim, n_choices, batch, nullptr, false); rc != RR_OK) return rc;
    const LearnerShape sh = disc_shape(n_choices);
    const int64_t sink_at = ppo_update_bytes(sh, batch);
    DiscreteLaunch D = {};
    D.op = kDiscUpdate;
    D.n_choices = n_choices;
    const int rc = ppo_update_record(who, D.u, sh, params, grads, exp_avg, exp_avg_sq, step, obs, actions, old_log_prob,
                                     advantages, returns, idx, batch, next_idx, next_batch, clip_range, ent_coef, vf_coef,
                                     max_grad_norm, lr, beta1, beta2, eps, stats, flags, RR_PPO_CHAINED, workspace,
                                     workspace_bytes, sink_at + kDiscSink * (int64_t)sizeof(float));
    if (rc != RR_OK) return rc;
    D.sink = (float*)((char*)workspace + sink_at);
    D.u.pg.p[12] = D.sink + 64 * 4 + 4;
    const hipError_t err = (hipError_t)rrc_launch_discrete(&D, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_ppo_update_discrete: launch");
}

int rr_ppo_update_discrete_opts_workspace_size(int obs_dim, int n_choices, int64_t batch, int64_t* bytes)
{
    const int rc = disc_learner_ok("rr_ppo_update_discrete_opts_workspace_size", obs_dim, n_choices, batch, bytes);
    // rr_ppo_update_discrete's sections, + 8 floats: the call's statistics when the caller passes none
    if (rc == RR_OK) *bytes = ppo_update_bytes(disc_shape(n_choices), batch) + kDiscSink * (int64_t)sizeof(float) + 32;
    return rc;
}

int rr_ppo_update_discrete_opts(int obs_dim, int n_choices, float* const* params, float* const* grads,
                                float* const* exp_avg, float* const* exp_avg_sq, float* const* step, const float* obs,
                                const float* actions, const float* old_log_prob, const float* advantages,
                                const float* returns, const float* old_values, const int64_t* idx, int64_t batch,
                                const int64_t* next_idx, int64_t next_batch, float clip_range, float ent_coef,
                                float vf_coef, float max_grad_norm, const float* lr, double beta1, double beta2,
                                float eps, const rr_ppo_options* options, float* control, float* stats, uint32_t flags,
                                void* workspace, int64_t workspace_bytes, void* stream)
{
    const char* who = "rr_ppo_update_discrete_opts";
    if (const int rc = disc_learner_ok(who, obs_dim, n_choices, batch, nullptr, false); rc != RR_OK) return rc;
    const LearnerShape sh = disc_shape(n_choices);
    const int64_t sink_at = ppo_update_bytes(sh, batch);
    const int64_t stats_at = sink_at + kDiscSink * (int64_t)sizeof(float);
    DiscreteOptsLaunch O = {};
    DiscreteLaunch& D = O.base;
    PpoLaunch u;  // ppo_update_record assigns the whole record
    const int rc = ppo_update_record(who, u, sh, params, grads, exp_avg, exp_avg_sq, step, obs, actions, old_log_prob,
                                     advantages, returns, idx, batch, next_idx, next_batch, clip_range, ent_coef, vf_coef,
                                     max_grad_norm, lr, beta1, beta2, eps, stats, flags,
                                     RR_PPO_CHAINED | RR_PPO_EPOCH_START, workspace, workspace_bytes, stats_at + 32);
    if (rc != RR_OK) return rc;
    if (const int rc2 = ppo_options_record(who, O, options, old_values, control, flags); rc2 != RR_OK) return rc2;
    D.op = kDiscUpdate;
    D.n_choices = n_choices;
    D.u = u;
    D.sink = (float*)((char*)workspace + sink_at);
    D.u.pg.p[12] = D.sink + 64 * 4 + 4;
    if (!stats) D.u.stats = (float*)((char*)workspace + stats_at);
    const hipError_t err = (hipError_t)rrc_launch_discrete_opts(&O, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_ppo_update_discrete_opts: launch");
}

int rr_bc_update_discrete_workspace_size(int obs_dim, int n_choices, int64_t batch, int64_t* bytes)
{
    const int rc = disc_learner_ok("rr_bc_update_discrete_workspace_size", obs_dim, n_choices, batch, bytes);
    if (rc == RR_OK) *bytes = bc_bytes(disc_shape(n_choices), batch, kDiscSink);
    return rc;
}

int rr_bc_update_discrete(int obs_dim, int n_choices, float* const* params, float* const* grads,
                          float* const* exp_avg, float* const* exp_avg_sq, float* const* step, const float* obs,
                          const float* actions, const int64_t* idx, int64_t batch, float ent_weight, float l2_weight,
                          const float* lr, double beta1, double beta2, float eps, float* stats, uint32_t flags,
                          void* workspace, int64_t workspace_bytes, void* stream)
{
    const char* who = "rr_bc_update_discrete";
    if (const int rc = disc_learner_ok(who, obs_dim, n_choices, batch, nullptr, false); rc != RR_OK) return rc;
    BcLaunch L;
    const int rc = bc_update_record(who, L, disc_shape(n_choices), kDiscSink, params, grads, exp_avg, exp_avg_sq, step,
                                    obs, actions, idx, batch, ent_weight, l2_weight, lr, beta1, beta2, eps, stats, flags,
                                    workspace, workspace_bytes);
    if (rc != RR_OK) return rc;
    L.n_choices = n_choices;
    L.pg.p[12] = L.sink + 64 * 4 + 4;  // log_std's slot of the finish body
    const hipError_t err = (hipError_t)rrc_launch_bc_discrete(&L, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_bc_update_discrete: launch");
}

// ---- A2C for the Categorical policy (a2c_discrete/rocket_a2c_discrete.hip): rr_a2c_update's record over the
// 12 tensors, rr_ppo_update_discrete's workspace (rr_ppo_update's sections, then the sink) ----
int rr_a2c_update_discrete_workspace_size(int obs_dim, int n_choices, int64_t batch, int64_t* bytes)
{
    const int rc = disc_learner_ok("rr_a2c_update_discrete_workspace_size", obs_dim, n_choices, batch, bytes);
    if (rc == RR_OK) *bytes = ppo_update_bytes(disc_shape(n_choices), batch) + kDiscSink * (int64_t)sizeof(float);
    return rc;
}

int rr_a2c_update_discrete(int obs_dim, int n_choices, float* const* params, float* const* grads,
                           float* const* square_avg, float* const* exp_avg, float* const* step, const float* obs,
                           const float* actions, const float* advantages, const float* returns, const int64_t* idx,
                           int64_t batch, int normalize_advantage, float ent_coef, float vf_coef, float max_grad_norm,
                           int optimizer, const float* lr, double alpha_or_beta1, double beta2, float eps, float* stats,
                           void* workspace, int64_t workspace_bytes, void* stream)
{
    const char* who = "rr_a2c_update_discrete";
    if (const int rc = disc_learner_ok(who, obs_dim, n_choices, batch, nullptr, false); rc != RR_OK) return rc;
    const LearnerShape sh = disc_shape(n_choices);
    const int64_t sink_at = ppo_update_bytes(sh, batch);
    A2cDiscreteLaunch D = {};
    const int rc = a2c_update_record(who, D.base, sh, params, grads, square_avg, exp_avg, step, obs, actions, advantages,
                                     returns, idx, batch, normalize_advantage, ent_coef, vf_coef, max_grad_norm, optimizer,
                                     lr, alpha_or_beta1, beta2, eps, stats, workspace, workspace_bytes,
                                     sink_at + kDiscSink * (int64_t)sizeof(float));
    if (rc != RR_OK) return rc;
    D.n_choices = n_choices;
    D.sink = (float*)((char*)workspace + sink_at);
    D.base.pg.p[12] = D.sink + 64 * 4 + 4;  // log_std's slot of the finish body
    const hipError_t err = (hipError_t)rrc_launch_a2c_discrete(&D, stream);
    return err == hipSuccess ? RR_OK : hip_fail(err, "rr_a2c_update_discrete: launch");
}

}  // extern "C"
