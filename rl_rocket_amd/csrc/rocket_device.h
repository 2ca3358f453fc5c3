// rocket_device.h — the device code shared by the five translation units of librocket_hip.so
// (rocket_hip.hip, rocket_exact.hip, rocket_collect.hip, eval_trace/rocket_eval_trace.hip,
// eval_exact/rocket_eval_exact.hip): the constants and the host-derived
// parameter blocks (KParams, XParams), the buffer / intrinsic wrappers, the reset stream, the
// RHS, integrators and ground event, reward and bounds, the obs tile store and the per-env
// loads / stores that every step kernel inlines (physics_step, store_terminal, store_outputs).
// Everything here is a template, a forceinline device function, a constant or a plain struct in
// the anonymous namespace: including it emits no kernel. At its end, host side: the variant
// dispatcher (dispatch_env / dispatch_env_prec: every launch site calls a generic lambda with
// compile-time tags for the handle's model, integrator and precision), the launch records
// (EnvLaunch, ExactLaunch, EvalExactLaunch) and the one declaration of each hidden entry point through
// which the main translation unit hands such a record to the other four.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "rocket_hip.h"
#include "rocket_stamps.h"

namespace {

// Newton iterations of the event root (2: -1.2 % per step, but the oracle-parity margin drops
// from 36x to 3x)
constexpr int kNewtonIters = 3;
// Cache-policy bits of the step kernel's buffer loads / stores (gfx950 CPol: 1 = sc0,
// 2 = nt, 16 = sc1); 0 = default policy. kStAux: library state planes (kernels above
// kHelpMaxN); kOutAux: caller-owned outputs.
constexpr int kLdAux = 0;
constexpr int kStAux = 0;
// state planes of the helper-wave step kernels (N <= kHelpMaxN): sc1 (device-scope write-through)
// where the whole batch's state is a few MB, so the end-of-kernel release has no dirty state
// lines to write back. A/B at N = 65536: direct launches 4.13-4.26 vs 4.34-4.55 us per step,
// hipGraph replays K = 20 4.39-4.41 vs 4.47-4.48, K = 2000 equal; at N = 524288 (plain kernel,
// default policy kept) it had cost 10-25 %. Round 8: the done path's stores of
// these kernels too (terminal rows, terminal return / length, the wave's done word), the last ones
// that left dirty lines: 4.62 -> 4.39 us per launch in steady state, 4.16 -> 4.05 fresh
// (DESIGN.md §3 'Round 8').
constexpr int kStAuxHelp = 16;
// caller-owned outputs (obs, reward, done, truncated): sc1 = device-scope write-through, the
// outputs leave L2 while the kernel runs instead of in the end-of-kernel writeback (A/B at
// N = 65536: 5.49 -> 5.18 us; the same bit on the state planes, which the next launch re-reads,
// is slower; nt loads +5 %).
constexpr int kOutAux = 16;
// terminal obs rows (the done lanes' scattered 56 B) of the plain kernels (N > kHelpMaxN): nt.
// Past the MALL, 4-B stores from a few lanes of a wave cost far more than their bytes (one
// partial line each): at 4M envs in steady state (~1.5 % of the envs done per step) the
// terminal rows took ~24 us and the reset v0 ~20 us of a 200 us step. The rows go nt
// (197.5 -> 182.4 us; sc1 200.5, sc1 | nt 200.2); the terminal return / length and v0 are stored
// by every lane of a wave with a done lane, as whole lines, past the MALL (kModeWholeLines; v0:
// 174.3 -> 157.3 us with the rows off; profiles/r04/phase/done_path_ab.txt)
constexpr int kTermAuxLarge = 2;
// largest N stepped with helper waves (step_kernel<..., HELP = true>); RR_HELP_MAX_N in the
// environment overrides it at rr_create (tests select the plain kernel at small N with it)
constexpr int64_t kHelpMaxN = 131072;
// largest N stepped with one main wave per workgroup (helper variant)
constexpr int64_t kNarrowMaxN = 16384;
// exact mode: the one-wave-per-SIMD 6DOF kernel runs up to (CUs x 4 SIMDs x 64 lanes) envs, one
// env per lane; above it the lean two-waves-per-SIMD kernel (rocket_dopri5.inc, solve LEAN). The
// CU count is the device's (rr_create); kExactLeanCUs is the fallback if the query fails
constexpr int64_t kExactLeanCUs = 256;
constexpr int kWave = 64;
constexpr int kBlock = 256;  // threads per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;

// ---------------------------------------------------------------------------
// Physical constants of the reference simulators.
//   6DOF: simulator.py:210-224 — g0 9.81, Isp 360, J = diag(75350.25, 6037675.13,
//         6037675.13), thrust hinge r_T_B = [-15, 0, 0], aero force identically 0.
//   3DOF: simulator.py:36-51, :100-126 — rho 1.225, Cd 0.3, Sref 10.5, alpha = 0
//         (normal force 0), I 6.04e6, lever x_T - x_CG = 30.
// ---------------------------------------------------------------------------
constexpr float kG0 = 9.81f;
constexpr double kIsp = 360.0;
constexpr double kJ1 = 75350.25, kJ2 = 6037675.13, kJ3 = 6037675.13;
constexpr double kRT = -15.0;
constexpr double kDrag3 = 0.5 * 1.225 * 0.3 * 10.5;  // A = Cd * (0.5 rho v^2) * Sref
constexpr double kLever3 = 40.0 - 10.0;               // x_T - x_CG
constexpr double kI3 = 6.04e6;
// folded into the device code as immediates
constexpr float kDmScale = (float)(-1.0 / (9.81 * kIsp));  // dm = T * kDmScale
constexpr float kJinv2 = (float)(1.0 / kJ2), kJinv3 = (float)(1.0 / kJ3);
constexpr float kJd1 = (float)(kJ1 - kJ3), kJd2 = (float)(kJ2 - kJ1);  // (w x Jw)_1 = kJd1 w1 w3, _2 = kJd2 w1 w2
constexpr float kRt = (float)(-kRT);  // tau = r_T_B x T_b = [0, 15 Tbz, -15 Tby]
static_assert(kJ2 == kJ3, "omega_1 is constant only for an axisymmetric body (J2 == J3)");
constexpr float kDrag3f = (float)kDrag3;
constexpr float kLeverOverI3 = (float)(kLever3 / kI3);
constexpr float kHalfPi = 1.57079632679489662f;
constexpr float kTwoPi = 6.28318530717958648f;

// Per-env counter word: TimeLimit steps in the low E bits, episodes started in the high
// 32 - E bits (keys the counter-based reset stream). E = bits of max_episode_steps (10 for the
// reference's TimeLimit 800: 2^22 episodes per env before the episode field wraps), 16 without
// a TimeLimit (KParams.el_mask / ep_shift, counter_bits()).
constexpr int32_t kMaxEpisodeSteps = 0xFFFF;
// step_kernel `mode` word: rr_params.flags plus "the counter word is live" and "the batch is
// past the MALL" (N > kWholeLineMinN: the done path's 4-B scalars leave as whole lines)
constexpr uint32_t kModeCounter = 0x80000000u;
constexpr uint32_t kModeWholeLines = 0x40000000u;
// ~200 B of state, action and outputs per env and step: above ~1M envs a step's working set
// passes the 256 MB MALL and partial lines become DRAM read-modify-writes (at 524 288, inside
// it, the whole-line stores measured 2-4 % slower; at 4 194 304 10 % faster). RR_WHOLE_LINE_MIN_N
// in the environment overrides it at rr_create (tests run the whole-line path at small N)
constexpr int64_t kWholeLineMinN = 1 << 20;

// Device-side constants, derived once on the host from rr_params (see make_kparams).
struct KParams {
    int32_t max_steps;
    uint32_t flags;
    float h, h2, h6;          // dt, dt/2, dt/6
    float ic_low[RR_MAX_STATE];
    float ic_span[RR_MAX_STATE];
    float inv_norm[RR_MAX_STATE];
    float blo[3], bhi[3];     // 6DOF: inclusive position box; 3DOF: x_lo(<=), x_hi(>=), z_hi(>=)
    float max_gimbal, half_thrust;
    float alfa, beta, eta, gamma, delta, kappa, xi;
    float waypoint, land_r2, land_v2;
    // attitude tests on the zyx Euler angles without inverse trig (make_kparams):
    //   |atan2(Y,X)| > L  <=>  X < r cos L ;  |asin(S)| > L  <=>  |S| > sin L
    float att_c[3];           // threshold per axis for "> limit"
    float land_c[3];          // threshold per axis for "< limit"
    uint32_t att_never;       // bit k: "|e_k| > limit" can never hold
    uint32_t land_always;     // bit k: "|e_k| < limit" always holds
    float omega_lt;           // |w| < omega_lim  (float threshold, reference 0.2)
    float zero_h;             // x <= 1e-3 as a float threshold
    uint32_t seed_w[4];       // reset stream key words (rr_seed)
    int64_t id_off;           // global id of env 0 (multi-GPU shards)
    // counter word: elapsed = cw & el_mask, episode = cw >> ep_shift. Last in the struct: placed
    // after `flags` they shifted the fields above and the kernel's kernarg scalar loads regrouped
    // (+2 % per step at N = 65536, A/B r02l)
    uint32_t el_mask, ep_shift;
};

// Host-derived fp64 constants of the exact mode (make_xparams; read by rocket_dopri5.inc).
struct XParams {
    double dt;
    double dt_milli;          // rint(dt * 1000) when dt has <= 3 decimals (clock exact), else 0
    double norm[RR_MAX_STATE];
    double lo[3], hi[3];      // bounds as rr_params
    double max_gimbal, max_thrust;
    double alfa, beta, eta, gamma, delta, kappa, xi;
    double waypoint, landing_radius, max_velocity;
    double att_limit[3], land_att_limit[3], omega_lim[3];
    int32_t clamp_h0;
    // the attitude tests without inverse trig (finish6; make_xparams): axes 0, 2 (atan2) cos of the
    // limit, axis 1 (asin) its sin; bit k of att_never / land_always: the test is constant
    double att_c[3], land_c[3];
    uint32_t att_never, land_always;
    uint32_t att_always, land_never;  // L < 0: |e| > L always; M <= 0: |e| < M never
};

// The parameters read after the integration (reward, bounds, obs). Copied out of the
// kernel arguments once at kernel start and pinned (pin_s) so the compiler cannot
// rematerialise them as scalar loads later: a lone wave per SIMD would otherwise stall
// on ~20 dependent s_load/s_waitcnt round trips inside the reward code (measured with
// per-wave s_memtime stamps in round 1: 2380 cycles for ~150 instructions).
struct HotParams {
    float inv_norm[RR_MAX_STATE];
    float blo[3], bhi[3];
    float half_thrust, alfa, beta, eta, gamma, delta, kappa, xi;
    float waypoint, land_r2, land_v2;
    float att_c[3], land_c[3];
    float omega_lt, zero_h;
    uint32_t att_never, land_always, flags;
};

template <class T>
__device__ __forceinline__ void pin_s(T& x)
{
    asm volatile("" : "+s"(x));
}

template <int NS>
__device__ __forceinline__ HotParams load_hot(const KParams& P)
{
    HotParams H;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        H.inv_norm[j] = P.inv_norm[j];
        asm volatile("" : "+v"(H.inv_norm[j]));
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        H.blo[j] = P.blo[j];
        H.bhi[j] = P.bhi[j];
        H.att_c[j] = P.att_c[j];
        H.land_c[j] = P.land_c[j];
        asm volatile("" : "+v"(H.blo[j]));
        asm volatile("" : "+v"(H.bhi[j]));
        asm volatile("" : "+v"(H.att_c[j]));
        asm volatile("" : "+v"(H.land_c[j]));
    }
#define RR_HOT(f) \
    H.f = P.f;    \
    pin_s(H.f)
    RR_HOT(half_thrust);
    RR_HOT(alfa);
    RR_HOT(beta);
    RR_HOT(eta);
    RR_HOT(gamma);
    RR_HOT(delta);
    RR_HOT(kappa);
    RR_HOT(xi);
    RR_HOT(waypoint);
    RR_HOT(land_r2);
    RR_HOT(land_v2);
    RR_HOT(omega_lt);
    RR_HOT(zero_h);
    RR_HOT(att_never);
    RR_HOT(land_always);
    RR_HOT(flags);
#undef RR_HOT
    return H;
}

struct Bufs {
    float* state;
    float* v0;
    uint32_t* counter;        // [N] counter word: elapsed in bits 0..E-1, episode above (E = KParams.ep_shift)
    float* ep_ret;
    uint64_t* done_bits;      // [ceil(N/64)] wave ballot of done lanes, one word per wave
    float* term_obs;
    float* term_ret;
    int32_t* term_len;
    int64_t n;
    const KParams* kp;        // device copy of the kernel's KParams: the helper waves read it (see step_kernel),
                              // and every kernel reads the reset-stream key seed_w from it, so rr_seed applies
                              // to every later launch, graph replays included
};

struct StepIO {
    const float* action;
    float* obs;
    float* reward;
    uint8_t* done;
    uint8_t* truncated;
    float* terms;
    int32_t obs_vec_ok;       // obs pointer 16-B aligned: LDS-staged float4 stores
};

__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }

// packed fp32 pairs (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 with op_sel swizzles)
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_swap(f2 a) { return __builtin_shufflevector(a, a, 1, 0); }
__device__ __forceinline__ f2 pk_lo(f2 a) { return __builtin_shufflevector(a, a, 0, 0); }
__device__ __forceinline__ f2 pk_hi(f2 a) { return __builtin_shufflevector(a, a, 1, 1); }
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 pk_his(f2 a, f2 b) { return __builtin_shufflevector(a, b, 1, 3); }  // (a.hi, b.hi)
__device__ __forceinline__ f2 pk_bc(float x) { return f2{x, x}; }


// Raw buffer access (SRSRC descriptor built from wave-uniform values): 32-bit per-lane
// voffset, per-plane offsets in soffset (SGPR) — no per-lane 64-bit address arithmetic.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, uint64_t bytes)
{
    const uint32_t nr = bytes >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)nr, 0x00020000);
}
__device__ __forceinline__ float bld_f(rsrc_t r, uint32_t voff, uint32_t soff)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, kLdAux));
}
__device__ __forceinline__ uint32_t bld_u(rsrc_t r, uint32_t voff, uint32_t soff)
{
    return __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, kLdAux);
}
template <int AUX = kStAux>
__device__ __forceinline__ void bst_f(rsrc_t r, float v, uint32_t voff, uint32_t soff)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)voff, (int)soff, AUX);
}
template <int AUX = kStAux>
__device__ __forceinline__ void bst_u(rsrc_t r, uint32_t v, uint32_t voff, uint32_t soff)
{
    __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)voff, (int)soff, AUX);
}
template <int AUX = kStAux>
__device__ __forceinline__ void bst_u8(rsrc_t r, uint8_t v, uint32_t voff)
{
    __builtin_amdgcn_raw_buffer_store_b8(v, r, (int)voff, 0, AUX);
}

// Element idx of a wave-uniform base pointer with a 32-bit byte offset: lowers to the
// saddr + voffset form of global_load/store (no per-lane 64-bit address arithmetic).
template <class T>
__device__ __forceinline__ T& at(T* base, uint32_t idx)
{
    return *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + (uint32_t)(idx * (uint32_t)sizeof(T)));
}
template <class T>
__device__ __forceinline__ const T& at(const T* base, uint32_t idx)
{
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (uint32_t)(idx * (uint32_t)sizeof(T)));
}
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }  // v_sqrt_f32, no IEEE fixup

// 1 - exp(-x) for x >= 0 without cancellation: Taylor series below 1/8 (truncation
// < 2e-9 relative), v_exp_f32 above (result >= 0.117, so its ulp error stays relative).
__device__ __forceinline__ float one_minus_exp_neg(float x)
{
    const float p = x * (1.0f - x * (0.5f - x * (1.0f / 6.0f - x * (1.0f / 24.0f - x * (1.0f / 120.0f)))));
    const float e = 1.0f - __builtin_amdgcn_exp2f(-x * 1.44269504088896341f);
    return x < 0.125f ? p : e;
}

// ---------------------------------------------------------------------------
// Reset stream: counter-based. The initial condition an env `gid` gets when its episode
// ends at counter word `cw` (episode | steps, unique per env and step) comes from a
// register-resident xorshift128 (Marsaglia 2003) whose four words are chained lowbias32
// mixes of (seed words, gid, cw): no per-env RNG state lives in HBM, the draw needs only
// the counter word (so the step kernel draws it while the state planes are in flight),
// and it is independent of how envs are sharded. After the mixes every draw is 6 full-rate
// shift/xor ops; the top 24 bits of each draw make one uniform (statistics:
// tests/test_gpu_envs.py::test_reset_distribution).
// ---------------------------------------------------------------------------

// 32-bit avalanche mix (lowbias32)
__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The Categorical sampler's index (discrete_act_kernel, rocket_rollout_body.inc, rocket_eval_body.inc): the
// number of q in 0 .. K - 2 whose running sum of ex / sum is <= u, where a step past choice q counts only
// while some weight beyond q is positive. ex holds the softmax weights exp(z - max), 0 for the heads
// >= n_choices, and sum their fp32 sum. u reaches 1 - 2^-24 and the fp32 running sum over the live choices
// can stop one to three ulps short of 1: without the second condition the index then walked past the last
// live choice into a trailing one whose weight had underflowed to 0. A row on which that did not happen keeps
// its index: every step up to a live choice has that choice's weight beyond it. Compares only, no branch and
// no data-dependent address.
template <int NH>
__device__ __forceinline__ int categorical_index(const float (&ex)[NH], float sum, float u, int n_choices)
{
    bool more[NH - 1];  // more[q]: some ex beyond q is positive
    bool m = false;
#pragma unroll
    for (int q = NH - 2; q >= 0; --q) {
        m = m | (ex[q + 1] > 0.0f);
        more[q] = m;
    }
    int index = 0;
    float cdf = 0.0f;
#pragma unroll
    for (int q = 0; q < NH - 1; ++q) {
        cdf += ex[q] / sum;
        index += ((q < n_choices - 1) & (cdf <= u) & more[q]) ? 1 : 0;
    }
    return index;
}

struct ResetStream {
    uint32_t x, y, z, w;
    // next uniform in [0, 1) with 24 random bits
    __device__ __forceinline__ float uniform()
    {
        const uint32_t t = x ^ (x << 11);
        x = y;
        y = z;
        z = w;
        w = w ^ (w >> 19) ^ t ^ (t >> 8);
        return (float)(w >> 8) * 0x1p-24f;
    }
};

__device__ __forceinline__ ResetStream reset_stream(const uint32_t* seed_w, int64_t gid, uint32_t cw)
{
    // every state word is a nonlinear function of (gid, cw): a word that depended on gid
    // alone would correlate the components of one env's successive initial conditions
    const uint32_t g = mix32(((uint32_t)gid + seed_w[0]) ^ (uint32_t)((uint64_t)gid >> 32));
    ResetStream r;
    r.x = mix32(g ^ (cw + seed_w[1]));
    r.y = mix32(r.x ^ seed_w[2]);
    r.z = mix32(r.y ^ seed_w[3]);
    r.w = mix32(r.z ^ seed_w[0]);
    return r;
}

template <int MODEL>
struct Dims;
template <>
struct Dims<6> {
    static constexpr int NS = 14, NA = 3, NT = 5, EV = 0;  // event on x (altitude)
};
template <>
struct Dims<3> {
    static constexpr int NS = 7, NA = 2, NT = 6, EV = 1;   // event on z (altitude)
};

// Controls, fixed over one env step.
struct Ctl {
    // 6DOF: body-frame thrust T_b = T [cy cz, sy cz, sz] (simulator.py:311-318, :350-357)
    float tbx, tby, tbz;
    float tau1, tau2;       // r_T_B x T_b (simulator.py:373-378), component 0 is 0
    // 3DOF
    float sd, cd, thrust, dom;
    float dm;               // -T/(g0 Isp)
};

template <int MODEL>
__device__ __forceinline__ Ctl make_ctl(const KParams& P, const float* a)
{
    Ctl c;
    if constexpr (MODEL == 6) {
        float dy = a[0] * P.max_gimbal, dz = a[1] * P.max_gimbal;
        float T = (a[2] + 1.0f) * P.half_thrust;
        float cy = __cosf(dy), sy = __sinf(dy), cz = __cosf(dz), sz = __sinf(dz);
        c.tbx = T * (cy * cz);
        c.tby = T * (sy * cz);
        c.tbz = T * sz;
        c.tau1 = (kRt * kJinv2) * c.tbz;   // J2^-1 tau_1
        c.tau2 = (-kRt * kJinv3) * c.tby;  // J3^-1 tau_2
        c.dm = T * kDmScale;
    } else {
        float d = a[0] * P.max_gimbal;
        float T = (a[1] + 1.0f) * P.half_thrust;
        c.sd = __sinf(d);
        c.cd = __cosf(d);
        c.thrust = T;
        c.dom = -(T * c.sd) * kLeverOverI3;
        c.dm = T * kDmScale;
    }
    return c;
}

// 6DOF RHS, simulator.py:259-294. R(q/|q|) T_b (scipy Rotation.from_quat normalises,
// simulator.py:346) is applied as a quaternion rotation of the UNnormalised q scaled by
// 1/|q|^2 (R is homogeneous of degree 2 in q):  |q|^2 R T_b = |q|^2 T_b + w t + u x t,
// t = 2 u x T_b; the division by |q|^2 folds into the division by the mass.
template <int MODEL>
__device__ __forceinline__ void rhs(const KParams& P, const Ctl& c, const float* s, float* d)
{
    if constexpr (MODEL == 6) {
        const float q0 = s[6], q1 = s[7], q2 = s[8], q3 = s[9];
        const float w1 = s[10], w2 = s[11], w3 = s[12];
        const float qq = q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3;
        const float tx = 2.0f * (q2 * c.tbz - q3 * c.tby);
        const float ty = 2.0f * (q3 * c.tbx - q1 * c.tbz);
        const float tz = 2.0f * (q1 * c.tby - q2 * c.tbx);
        const float Fx = qq * c.tbx + q0 * tx + (q2 * tz - q3 * ty);
        const float Fy = qq * c.tby + q0 * ty + (q3 * tx - q1 * tz);
        const float Fz = qq * c.tbz + q0 * tz + (q1 * ty - q2 * tx);
        const float sc = frcp(qq * s[13]);
        d[0] = s[3];
        d[1] = s[4];
        d[2] = s[5];
        d[3] = Fx * sc - kG0;
        d[4] = Fy * sc;
        d[5] = Fz * sc;
        // dq = 0.5 Omega(w) q with the unnormalised q (simulator.py:287, :362-370)
        const float h1 = 0.5f * w1, h2 = 0.5f * w2, h3 = 0.5f * w3;
        d[6] = -h1 * q1 - h2 * q2 - h3 * q3;
        d[7] = h1 * q0 + h3 * q2 - h2 * q3;
        d[8] = h2 * q0 - h3 * q1 + h1 * q3;
        d[9] = h3 * q0 + h2 * q1 - h1 * q2;
        // dw = J^-1 (tau - w x Jw) (simulator.py:288); J2 == J3 makes dw_1 = 0
        d[10] = 0.0f;
        d[11] = c.tau1 - (kJd1 * kJinv2) * (w1 * w3);
        d[12] = c.tau2 - (kJd2 * kJinv3) * (w1 * w2);
        d[13] = c.dm;
    } else {
        // 3DOF RHS, simulator.py:88-130 (N = 0; the z-drag uses cos(phi): reference quirk)
        const float th = s[2], vx = s[3], vz = s[4];
        float st = __sinf(th), ct = __cosf(th);
        float A = kDrag3f * (vx * vx + vz * vz);
        float cdt = c.cd * ct - c.sd * st;   // cos(delta + phi)
        float sdt = c.sd * ct + c.cd * st;   // sin(delta + phi)
        float im = frcp(s[6]);
        d[0] = vx;
        d[1] = vz;
        d[2] = s[5];
        d[3] = (c.thrust * cdt - A * ct) * im;
        d[4] = (c.thrust * sdt - A * ct) * im - kG0;
        d[5] = c.dom;
        d[6] = c.dm;
    }
}

// 6DOF RK4 specialised to the structure of the RHS (simulator.py:259-294): r and v never
// feed back (the aero force is identically zero, :359-360), so over one step they are
// quadratures of the stage accelerations a_s = R(q_s) T_b / m_s + g:
//   v1 = v0 + h/6 (a1 + 2 a2 + 2 a3 + a4),   r1 = r0 + h v0 + h^2/6 (a1 + a2 + a3)
// (the RK4 update itself, rearranged); m is linear in t (exact at every stage); w1 is
// constant (J2 == J3); q and (w2, w3) take the usual RK4 stages, carried as half-rates
// W = w/2 so dq = Omega(W) q needs no 0.5 factors. Same RK4 solution as the generic form
// (integrate) up to fp32 rounding. f0 = f(y0) for the event path.
// It runs on packed fp32 pairs (v_pk_fma_f32 / v_pk_mul_f32, two lanes'
// worth of fp32 per instruction): a lone wave issues one VALU instruction per 4 cycles
// whatever its width, so pairing the independent components of one env halves the issue
// cost of the quaternion and angular-rate algebra. Pairs: q = (q0,q1),(q2,q3);
// W = (W2,W3); a = (ax,ay), az. Each half rounds exactly like the scalar fma.

// o = y * inv_norm, two components per v_pk_mul_f32
template <int NS>
__device__ __forceinline__ void normalize_obs(const float* y, const float* inv_norm, float* o)
{
#pragma unroll
    for (int j = 0; j + 1 < NS; j += 2) {
        const f2 v = f2{y[j], y[j + 1]} * f2{inv_norm[j], inv_norm[j + 1]};
        o[j] = v.x;
        o[j + 1] = v.y;
    }
    if constexpr (NS % 2) o[NS - 1] = y[NS - 1] * inv_norm[NS - 1];
}

// Packed 6DOF RHS pieces for one step's controls: R(q) T_b / m + g as (ax, ay), az, and
// dq = Omega(W) q with W = w / 2 (pairs (q0,q1), (q2,q3); see rhs for the formulas).
struct Pk6 {
    f2 t2xy, tbxy, t2zn, t2yx, gxy;
    float t2z, tbz;
    __device__ __forceinline__ explicit Pk6(const Ctl& c)
    {
        t2xy = f2{2.0f * c.tbx, 2.0f * c.tby};
        t2z = 2.0f * c.tbz;
        tbxy = f2{c.tbx, c.tby};
        tbz = c.tbz;
        t2zn = f2{t2z, -t2z};
        t2yx = f2{-t2xy.y, t2xy.x};
        gxy = f2{-kG0, 0.0f};
    }
    __device__ __forceinline__ void accel(f2 q01, f2 q23, float m, f2& axy, float& az) const
    {
        const f2 sq = pk_fma(q01, q01, q23 * q23);
        const float qq = sq.x + sq.y;
        // t = 2 u x T_b, u = (q1, q2, q3), with qa = (q2, q1):
        //   (tx, ty) = qa (t2z, -t2z) + q3 (-t2y, t2x),   tz = q1 t2y - q2 t2x
        const f2 qa = __builtin_shufflevector(q23, q01, 0, 3);
        const f2 q3 = pk_hi(q23);
        const f2 txy = pk_fma(qa, t2zn, q3 * t2yx);
        const float tz = fmaf(q01.y, t2xy.y, -q23.x * t2xy.x);
        // F = |q|^2 T_b + q0 t + u x t;  (u x t)_xy = qa (tz, -tz) + q3 (-ty, tx)
        const f2 uxt = pk_fma(qa, f2{tz, -tz}, q3 * (pk_swap(txy) * f2{-1.0f, 1.0f}));
        const f2 Fxy = pk_fma(pk_bc(qq), tbxy, pk_fma(pk_lo(q01), txy, uxt));
        const float Fz = fmaf(qq, tbz, fmaf(q01.x, tz, fmaf(q01.y, txy.y, -q23.x * txy.x)));
        const float sc = frcp(qq * m);
        axy = pk_fma(Fxy, pk_bc(sc), gxy);
        az = Fz * sc;
    }
    // dq = Omega(W) q:
    //   (d0, d1) = (-W1, W1) (q1, q0) + (-W2, W3) (q2, q2) - (W3, W2) (q3, q3)
    //   (d2, d3) = (W2, W3) (q0, q0) + (-W3, W2) (q1, q1) + (W1, -W1) (q3, q2)
    static __device__ __forceinline__ void dq(f2 q01, f2 q23, float W1, f2 W, f2& d01, f2& d23)
    {
        const f2 w1a = {-W1, W1}, w1b = {W1, -W1};
        const f2 Wn = W * f2{-1.0f, 1.0f}, Ws = pk_swap(W), Wsn = Ws * f2{-1.0f, 1.0f};
        d01 = pk_fma(w1a, pk_swap(q01), pk_fma(Wn, pk_lo(q23), -(Ws * pk_hi(q23))));
        d23 = pk_fma(W, pk_lo(q01), pk_fma(Wsn, pk_hi(q01), w1b * pk_swap(q23)));
    }
};

// Full 6DOF RHS f(s) on the packed pieces (the ground-event path's f(y1)).
__device__ __forceinline__ void rhs6_pk(const Ctl& c, const float* s, float* d)
{
    const Pk6 k(c);
    f2 axy, d01, d23;
    float az;
    const f2 q01 = {s[6], s[7]}, q23 = {s[8], s[9]};
    k.accel(q01, q23, s[13], axy, az);
    const float W1 = 0.5f * s[10];
    const f2 W = {0.5f * s[11], 0.5f * s[12]};
    Pk6::dq(q01, q23, W1, W, d01, d23);
    const f2 A = {c.tau1, c.tau2};
    const f2 B = {(-kJd1 * kJinv2) * s[10], (-kJd2 * kJinv3) * s[10]};
    const f2 dw = pk_fma(B, f2{s[12], s[11]}, A);
    d[0] = s[3];
    d[1] = s[4];
    d[2] = s[5];
    d[3] = axy.x;
    d[4] = axy.y;
    d[5] = az;
    d[6] = d01.x;
    d[7] = d01.y;
    d[8] = d23.x;
    d[9] = d23.y;
    d[10] = 0.0f;
    d[11] = dw.x;
    d[12] = dw.y;
    d[13] = c.dm;
}

__device__ __forceinline__ void integrate6_rk4_pk(const KParams& P, const Ctl& c, const float* y0, float* y1,
                                                  float* f0)
{
    const float h = P.h, hh = P.h2, h6 = P.h6, hh6 = P.h * P.h6;
    const Pk6 k(c);
    auto accel = [&](f2 q01, f2 q23, float m, f2& axy, float& az) { k.accel(q01, q23, m, axy, az); };
    const float W1 = 0.5f * y0[10];
    // dW2 = A2 + B2 W3, dW3 = A3 + B3 W2 (half of dw = J^-1 (tau - w x Jw)): pair form
    // dW = A + B swap(W)
    const f2 A = {0.5f * c.tau1, 0.5f * c.tau2};
    const f2 B = {(-2.0f * kJd1 * kJinv2) * W1, (-2.0f * kJd2 * kJinv3) * W1};
    auto dq = [&](f2 q01, f2 q23, f2 W, f2& d01, f2& d23) { Pk6::dq(q01, q23, W1, W, d01, d23); };
    const f2 q01 = {y0[6], y0[7]}, q23 = {y0[8], y0[9]};
    const f2 W0 = {0.5f * y0[11], 0.5f * y0[12]};
    const float m0 = y0[13];
    const float mh = m0 + hh * c.dm, me = m0 + h * c.dm;
    const f2 hh2 = pk_bc(hh), h2 = pk_bc(h);
    f2 a1, a2, a3, a4, k101, k123, k201, k223, k301, k323, k401, k423, l1, l2, l3, l4;
    float a1z, a2z, a3z, a4z;
    // stage 1
    accel(q01, q23, m0, a1, a1z);
    dq(q01, q23, W0, k101, k123);
    l1 = pk_fma(B, pk_swap(W0), A);
    // stage 2
    f2 Ws = pk_fma(hh2, l1, W0);
    f2 qs01 = pk_fma(hh2, k101, q01), qs23 = pk_fma(hh2, k123, q23);
    accel(qs01, qs23, mh, a2, a2z);
    dq(qs01, qs23, Ws, k201, k223);
    l2 = pk_fma(B, pk_swap(Ws), A);
    // stage 3
    Ws = pk_fma(hh2, l2, W0);
    qs01 = pk_fma(hh2, k201, q01);
    qs23 = pk_fma(hh2, k223, q23);
    accel(qs01, qs23, mh, a3, a3z);
    dq(qs01, qs23, Ws, k301, k323);
    l3 = pk_fma(B, pk_swap(Ws), A);
    // stage 4
    Ws = pk_fma(h2, l3, W0);
    qs01 = pk_fma(h2, k301, q01);
    qs23 = pk_fma(h2, k323, q23);
    accel(qs01, qs23, me, a4, a4z);
    dq(qs01, qs23, Ws, k401, k423);
    l4 = pk_fma(B, pk_swap(Ws), A);
    // updates: v1 = v0 + h/6 (a1 + 2 a2 + 2 a3 + a4), r1 = r0 + h v0 + h^2/6 (a1 + a2 + a3)
    const f2 two = pk_bc(2.0f), h62 = pk_bc(h6), hh62 = pk_bc(hh6);
    const f2 v01 = {y0[3], y0[4]}, r01 = {y0[0], y0[1]};
    const f2 s23 = a2 + a3;
    const f2 v1 = pk_fma(h62, pk_fma(two, s23, a1 + a4), v01);
    const f2 r1 = pk_fma(hh62, a1 + s23, pk_fma(h2, v01, r01));
    const float s23z = a2z + a3z;
    y1[0] = r1.x;
    y1[1] = r1.y;
    y1[2] = (y0[2] + h * y0[5]) + hh6 * (a1z + s23z);
    y1[3] = v1.x;
    y1[4] = v1.y;
    y1[5] = y0[5] + h6 * (a1z + a4z + 2.0f * s23z);
    const f2 qe01 = pk_fma(h62, pk_fma(two, k201 + k301, k101 + k401), q01);
    const f2 qe23 = pk_fma(h62, pk_fma(two, k223 + k323, k123 + k423), q23);
    const f2 We = pk_fma(h62, pk_fma(two, l2 + l3, l1 + l4), W0);
    y1[6] = qe01.x;
    y1[7] = qe01.y;
    y1[8] = qe23.x;
    y1[9] = qe23.y;
    y1[10] = y0[10];
    y1[11] = 2.0f * We.x;
    y1[12] = 2.0f * We.y;
    y1[13] = me;
    f0[0] = y0[3];
    f0[1] = y0[4];
    f0[2] = y0[5];
    f0[3] = a1.x;
    f0[4] = a1.y;
    f0[5] = a1z;
    f0[6] = k101.x;
    f0[7] = k101.y;
    f0[8] = k123.x;
    f0[9] = k123.y;
    f0[10] = 0.0f;
    f0[11] = 2.0f * l1.x;
    f0[12] = 2.0f * l1.y;
    f0[13] = c.dm;
}

template <int MODEL, int INTEG>
__device__ __forceinline__ void integrate(const KParams& P, const Ctl& c, const float* y0, float h,
                                          float* y1, float* f0)
{
    constexpr int NS = Dims<MODEL>::NS;
    float k[NS], yt[NS];
    if constexpr (MODEL == 6 && INTEG == RR_INT_RK4) {
        integrate6_rk4_pk(P, c, y0, y1, f0);
        return;
    }
    if constexpr (INTEG == RR_INT_EULER) {
        rhs<MODEL>(P, c, y0, k);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            f0[j] = k[j];
            y1[j] = y0[j] + h * k[j];
        }
    } else {
        const float hh = 0.5f * h, h6 = h * (1.0f / 6.0f);
        float acc[NS];
        rhs<MODEL>(P, c, y0, k);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            f0[j] = k[j];
            acc[j] = k[j];
            yt[j] = y0[j] + hh * k[j];
        }
        rhs<MODEL>(P, c, yt, k);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            acc[j] += 2.0f * k[j];
            yt[j] = y0[j] + hh * k[j];
        }
        rhs<MODEL>(P, c, yt, k);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            acc[j] += 2.0f * k[j];
            yt[j] = y0[j] + h * k[j];
        }
        rhs<MODEL>(P, c, yt, k);
#pragma unroll
        for (int j = 0; j < NS; ++j) y1[j] = y0[j] + h6 * (acc[j] + k[j]);
    }
}

// Terminal ground event (solve_ivp events=..., terminal, direction 0; scipy
// ivp.find_active_events): sign change of the altitude between the step ends.
// The reference returns its RK45 dense output at the brentq root of the altitude
// (ivp.py handle_events, rk.py RkDenseOutput). Here the step's dense output is the
// cubic Hermite interpolant through (y0, f(y0)) and (y1, f(y1)) — 4th-order like the
// reference's — its altitude root is found by safeguarded Newton, and every state
// component is evaluated there. Explicit Euler (RR_INT_EULER) uses its own continuous extension,
// the line y0 + s h f(y0): root s = x0 / (x0 - x1) (oracle/rocket_oracle.c euler_step).
template <int MODEL, int INTEG>
__device__ __forceinline__ void event_step(const KParams& P, const Ctl& c, const float* y0, const float* f0,
                                           float* y1)
{
    constexpr int EV = Dims<MODEL>::EV;
    constexpr int NS = Dims<MODEL>::NS;
    const float x0 = y0[EV], x1 = y1[EV];
    if (x1 == 0.0f) return;  // root at the step end: state unchanged
    if constexpr (INTEG == RR_INT_EULER) {
        const float sh = (x0 * frcp(x0 - x1)) * P.h;
#pragma unroll
        for (int j = 0; j < NS; ++j) y1[j] = fmaf(sh, f0[j], y0[j]);
        return;
    }
    float f1[NS];
    if constexpr (MODEL == 6) rhs6_pk(c, y1, f1);
    else rhs<MODEL>(P, c, y1, f1);
    // straight-line code (one basic block with the RHS, so the scheduler interleaves the
    // two): x0 == 0 gives the secant guess 0 and H(0) == 0, so s stays 0 (y = y0, as the
    // reference's root at the step start)
    float s;
    {
        const float hv0 = P.h * f0[EV], hv1 = P.h * f1[EV];
        // the altitude's Hermite cubic in monomial form: H(s) = ((c3 s + c2) s + c1) s + c0
        const float dx = x1 - x0;
        const float c2 = 3.0f * dx - (2.0f * hv0 + hv1), c3 = (hv0 + hv1) - 2.0f * dx;
        const float d2 = 2.0f * c2, d3 = 3.0f * c3;
        const bool pos0 = x0 > 0.0f;
        float lo = 0.0f, hi = 1.0f;  // H(lo) has the sign of x0
        s = x0 * frcp(x0 - x1);
        // Newton from the secant guess, kept inside the closed sign bracket [lo, hi]
        // (bisection fallback). A converged iterate sits on a bracket end, so the test is
        // inclusive. Fixed 3 iterations, branch-free (quadratic convergence from the secant
        // guess; the parity tests cover touchdowns down to |v| ~ 1 m/s).
#pragma unroll
        for (int it = 0; it < kNewtonIters; ++it) {
            const float H = fmaf(fmaf(fmaf(c3, s, c2), s, hv0), s, x0);
            const float dH = fmaf(fmaf(d3, s, d2), s, hv0);
            const bool same = (H > 0.0f) == pos0;
            lo = same ? s : lo;
            hi = same ? hi : s;
            float sn = fmaf(-H, frcp(dH), s);
            sn = (sn >= lo && sn <= hi) ? sn : 0.5f * (lo + hi);
            s = (H == 0.0f) ? s : sn;
        }
    }
    // every component at the root: y = y0 + h01 (y1 - y0) + h10 f0 + h11 f1 (cubic Hermite)
    const float s2 = s * s, s3 = s2 * s;
    const float h01 = 3 * s2 - 2 * s3;
    const float h10 = P.h * (s3 - 2 * s2 + s), h11 = P.h * (s3 - s2);
    // two components per v_pk_fma_f32; w1 (6DOF) is constant over the step (J2 == J3) and the
    // mass is linear in t, so exact at the root
    const f2 H01 = {h01, h01}, H10 = {h10, h10}, H11 = {h11, h11};
    auto herm2 = [&](int j, int k) {
        const f2 a = {y0[j], y0[k]}, b = {y1[j], y1[k]};
        const f2 r = pk_fma(H11, f2{f1[j], f1[k]}, pk_fma(H10, f2{f0[j], f0[k]}, pk_fma(H01, b - a, a)));
        y1[j] = r.x;
        y1[k] = r.y;
    };
    herm2(0, 1);
    herm2(2, 3);
    herm2(4, 5);
    if constexpr (MODEL == 6) {
        herm2(6, 7);
        herm2(8, 9);
        herm2(11, 12);
    }
    y1[NS - 1] = fmaf(s * P.h, f0[NS - 1], y0[NS - 1]);
}

// After the step: _normalize_quaternion (simulator.py:250) / _wrapTo2Pi (simulator.py:150-163)
template <int MODEL>
__device__ __forceinline__ void post_integrate(float* y1)
{
    if constexpr (MODEL == 6) {
        // _normalize_quaternion (simulator.py:250)
        const f2 q01 = {y1[6], y1[7]}, q23 = {y1[8], y1[9]};
        const f2 sq = pk_fma(q01, q01, q23 * q23);
        const f2 rn = pk_bc(frsq(sq.x + sq.y));
        const f2 n01 = q01 * rn, n23 = q23 * rn;
        y1[6] = n01.x;
        y1[7] = n01.y;
        y1[8] = n23.x;
        y1[9] = n23.y;
    } else {
        // _wrapTo2Pi (simulator.py:150-163): fmod(fmod(theta, 2pi) + 2pi, 2pi)
        float th = fmodf(y1[2], kTwoPi) + kTwoPi;
        y1[2] = fmodf(th, kTwoPi);
    }
}

// A post-step state with a NaN / inf component ends the episode: the analogue of solve_ivp's
// status -1 (done = bool(status), simulator.py:236-241 -> rocket_env.py:702 / :158). scipy's RK45
// never returns on such a state (a NaN step size passes its `h_abs < min_step` test forever);
// the exact mode and the oracle stop it as TOO_SMALL_STEP (status -1), and here every
// component enters a sum of y_j * 0, which is +-0 for finite y_j and NaN otherwise (no
// overflow of finite values; 7 v_pk_fma_f32 for 6DOF). The terms plane reports status -1.
template <int NS>
__device__ __forceinline__ bool nonfinite(const float* y)
{
    f2 acc = pk_bc(0.0f);
#pragma unroll
    for (int j = 0; j + 1 < NS; j += 2) acc = pk_fma(f2{y[j], y[j + 1]}, pk_bc(0.0f), acc);
    float s = acc.x + acc.y;
    if constexpr (NS % 2) s = fmaf(y[NS - 1], 0.0f, s);
    return !(s == 0.0f);
}

// Sample one initial condition: gym Box.sample (uniform in [low, high], float32),
// then q <- q/|q| (rocket_env.py:672-673); v0 = |IC velocity| (rocket_env.py:989-991).
template <int MODEL, class IP>  // IP: KParams, or anything with its ic_low / ic_span (rol::ResetParams)
__device__ __forceinline__ void sample_ic(const IP& P, ResetStream& k, float* s, float& v0)
{
    constexpr int NS = Dims<MODEL>::NS;
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j] = fmaf(P.ic_span[j], k.uniform(), P.ic_low[j]);
    if constexpr (MODEL == 6) {
        const float rn = frsq(s[6] * s[6] + s[7] * s[7] + s[8] * s[8] + s[9] * s[9]);
        s[6] *= rn;
        s[7] *= rn;
        s[8] *= rn;
        s[9] *= rn;
        v0 = fsqrt(s[3] * s[3] + s[4] * s[4] + s[5] * s[5]);
    } else {
        v0 = fsqrt(s[3] * s[3] + s[4] * s[4]);
    }
}

// Bounds violation on the float32 post-step state: 6DOF Box(lo, hi, float32).contains(r)
// (rocket_env.py:1036-1038, inclusive); 3DOF _check_bounds (rocket_env.py:431-447).
struct BoxParams {
    float blo[3], bhi[3];
};

template <int MODEL, class BP>
__device__ __forceinline__ bool bounds_hit(const BP& P, const float* s)
{
    if constexpr (MODEL == 6) {
        const bool inside = (s[0] >= P.blo[0]) & (s[0] <= P.bhi[0]) & (s[1] >= P.blo[1]) & (s[1] <= P.bhi[1]) &
                            (s[2] >= P.blo[2]) & (s[2] <= P.bhi[2]);
        return !inside;
    } else {
        return (s[0] <= P.blo[0]) | (s[0] >= P.bhi[0]) | (s[1] >= P.bhi[1]);
    }
}

// Reward / done of the reference env on the float32 post-step state.
template <int MODEL>
__device__ __forceinline__ float reward_terms(const HotParams& P, const float* s, const float* a, float v0,
                                              bool& bounds_violation, float* t)
{
    // Branch-free on purpose: the comparisons combine with bitwise & / | and the waypoint
    // cases with selects, so a lone wave runs straight-line code (short-circuit && / ||
    // compiled to ~8 exec-mask branches here).
    if constexpr (MODEL == 6) {
        bounds_violation = bounds_hit<6>(P, s);
        // _compute_vtarg (rocket_env.py:986-1014)
        const bool above = s[0] > P.waypoint;
        const float rh0 = above ? s[0] - P.waypoint : s[0] + 1.0f;
        const float rh1 = above ? s[1] : 0.0f, rh2 = above ? s[2] : 0.0f;
        const float vh0 = s[3] + (above ? 2.0f : 1.0f);
        const float tau_inv = above ? 1.0f / 20.0f : 1.0f / 100.0f;
        float nrh = fsqrt(rh0 * rh0 + rh1 * rh1 + rh2 * rh2);
        float t_go = nrh * frsq(vh0 * vh0 + s[4] * s[4] + s[5] * s[5]);
        float f = (-v0 * frcp(fmaxf(1e-3f, nrh))) * one_minus_exp_neg(t_go * tau_inv);
        float e0 = s[3] - f * rh0, e1 = s[4] - f * rh1, e2 = s[5] - f * rh2;
        t[0] = P.alfa * fsqrt(e0 * e0 + e1 * e1 + e2 * e2);
        // thrust_penalty = beta * T (denormalised, float32)
        t[1] = P.beta * ((a[2] + 1.0f) * P.half_thrust);
        t[2] = P.eta;
        // zyx Euler angles of q (Rotation.as_euler("zyx"), rocket_env.py:852-855, 1047):
        //   a = atan2(-R01, R00), b = asin(R02), c = atan2(-R12, R22)
        const float w = s[6], x = s[7], y = s[8], z = s[9];
        float R00 = w * w + x * x - y * y - z * z;
        float mR01 = 2.0f * (z * w - x * y);
        float R02 = 2.0f * (x * z + y * w);
        float mR12 = 2.0f * (x * w - y * z);
        float R22 = w * w - x * x - y * y + z * z;
        float ra = fsqrt(R00 * R00 + mR01 * mR01);
        float rc = fsqrt(R22 * R22 + mR12 * mR12);
        // q was renormalised after the step (|q|^2 = 1 to fp32 rounding), so sin b = R02
        // without the division by |q|^2 (R00, R22 and the cos b radii are homogeneous)
        float sb = fabsf(R02);
        const bool att = (!(P.att_never & 1u) & (R00 < ra * P.att_c[0])) | (!(P.att_never & 2u) & (sb > P.att_c[1])) |
                         (!(P.att_never & 4u) & (R22 < rc * P.att_c[2]));
        t[3] = att ? P.gamma : 0.0f;
        // _check_landing (rocket_env.py:1040-1061); any() over angles and omega is the reference's
        const bool att_ok = (P.land_always != 0u) | (R00 > ra * P.land_c[0]) | (sb < P.land_c[1]) |
                            (R22 > rc * P.land_c[2]);
        const bool om_ok = (fabsf(s[10]) < P.omega_lt) | (fabsf(s[11]) < P.omega_lt) | (fabsf(s[12]) < P.omega_lt);
        float r2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
        float v2 = s[3] * s[3] + s[4] * s[4] + s[5] * s[5];
        const bool landing = (s[0] <= P.zero_h) & (v2 < P.land_v2) & (r2 < P.land_r2) & att_ok & om_ok;
        t[4] = landing ? P.kappa : 0.0f;
        if (P.flags & RR_FLAG_REWARD_ANNEALING) return t[3] + t[4] - P.xi * (a[2] + 1.0f);
        return t[0] + t[1] + t[2] + t[3] + t[4] + (bounds_violation ? -50.0f : 0.0f);
    } else {
        bounds_violation = bounds_hit<3>(P, s);
        // _compute_vtarg (rocket_env.py:219-247)
        const bool above = s[1] > P.waypoint;
        const float rh0 = above ? s[0] : 0.0f;
        const float rh1 = above ? s[1] - P.waypoint : s[1];
        const float vh1 = s[4] + (above ? 2.0f : 1.0f);
        const float tau_inv = above ? 1.0f / 20.0f : 1.0f / 100.0f;
        float nrh = fsqrt(rh0 * rh0 + rh1 * rh1);
        float nvh = fsqrt(s[3] * s[3] + vh1 * vh1);
        float t_go = nrh * frcp(nvh);
        float f = (-v0 * frcp(fmaxf(1e-3f, nrh))) * one_minus_exp_neg(t_go * tau_inv);
        float e0 = s[3] - f * rh0, e1 = s[4] - f * rh1;
        t[0] = P.alfa * fsqrt(e0 * e0 + e1 * e1);
        t[1] = P.beta * ((a[1] + 1.0f) * P.half_thrust);
        t[2] = P.eta;
        float zeta = fabsf(s[2] - kHalfPi);
        t[3] = zeta > kTwoPi ? P.gamma : 0.0f;
        t[4] = P.delta * fmaxf(0.0f, zeta - kHalfPi);
        // _check_landing (rocket_env.py:449-476)
        float r2 = s[0] * s[0] + s[1] * s[1];
        float v2 = s[3] * s[3] + s[4] * s[4];
        const bool landing = (s[1] <= P.zero_h) & (v2 < P.land_v2) & (r2 < P.land_r2) & (zeta < 0.2f) &
                             (fabsf(s[5]) < P.omega_lt);
        t[5] = landing ? P.kappa : 0.0f;
        if (P.flags & RR_FLAG_REWARD_ANNEALING) return t[3] + t[5] - P.xi * (a[1] + 1.0f);
        return t[0] + t[1] + t[2] + t[3] + t[4] + t[5] + (bounds_violation ? -50.0f : 0.0f);
    }
}

// Write this wave's [64][NS] observation tile through LDS as 16-B coalesced stores.
template <int NS, int EPW>
__device__ __forceinline__ void store_obs_tile(float* lds, const float* o, rsrc_t obs_r, uint32_t wave_base,
                                               int lane, uint32_t nvalid, bool vec_ok)
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
    const uint32_t sbase = wave_base * NS * 4u;  // byte offset of the tile (wave-uniform)
    if (vec_ok && nvalid == (uint32_t)EPW) {
        constexpr int NV = EPW * NS / 4;
        const u32x4* src4 = reinterpret_cast<const u32x4*>(lds);
#pragma unroll
        for (int q = 0; q < (NV + kWave - 1) / kWave; ++q) {
            const int k = lane + q * kWave;
            if (NV % kWave == 0 || k < NV)
                __builtin_amdgcn_raw_buffer_store_b128(src4[k], obs_r, (int)(k * 16u), (int)sbase, kOutAux);
        }
    } else {
        const int tot = (int)nvalid * NS;
        for (int k = lane; k < tot; k += kWave) bst_f<kOutAux>(obs_r, lds[k], k * 4u, sbase);
    }
}

// ---------------------------------------------------------------------------
// Step kernels. One launch = one env step of all N envs. Every HBM access goes through a
// buffer descriptor: the per-lane byte offset is one 32-bit VGPR (i*4), plane offsets are
// wave-uniform soffsets (NS*N*4 < 4 GiB, checked at rr_create). The leading four arguments
// are plain pointers / words so that the command processor preloads them into user SGPRs at
// wave launch (-mllvm -amdgpu-kernarg-preload-count, rl_rocket_amd/build.py): the first
// state loads then issue without waiting for scalar loads of the kernarg segment.
// `mode` = rr_params.flags | kModeCounter. ASOA: action layout [NA][N] (RR_FLAG_ACTION_SOA)
// as a template parameter (a runtime branch between the two layouts made the waitcnt pass
// stall the wave on the state loads before it issued the action load).
// ---------------------------------------------------------------------------

// the action row of env `vo / 4` ([N][NA] rows or [NA][N] planes)
template <int NA, bool ASOA>
__device__ __forceinline__ void load_action(rsrc_t act_r, uint32_t vo, uint32_t plane, float* a)
{
    if constexpr (ASOA) {
#pragma unroll
        for (int j = 0; j < NA; ++j) a[j] = bld_f(act_r, vo, j * plane);
    } else if constexpr (NA == 3) {
        const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(act_r, (int)((vo << 1) + vo), 0, kLdAux);  // 12 B rows
        a[0] = __uint_as_float(v.x);
        a[1] = __uint_as_float(v.y);
        a[2] = __uint_as_float(v.z);
    } else {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(act_r, (int)(vo << 1), 0, kLdAux);  // 8 B rows
        a[0] = __uint_as_float(v.x);
        a[1] = __uint_as_float(v.y);
    }
}

// Simulator*.step (simulator.py:227-257 / :55-80): integrator, terminal ground event,
// quaternion renormalisation / theta wrap. Returns the event flag (solve_ivp status 1).
template <int MODEL, int INTEG>
__device__ __forceinline__ bool physics_step(const KParams& P, const float* a, const float* y0, float* y1)
{
    constexpr int NS = Dims<MODEL>::NS, EV = Dims<MODEL>::EV;
    float f0[NS];
    const Ctl c = make_ctl<MODEL>(P, a);
    integrate<MODEL, INTEG>(P, c, y0, P.h, y1, f0);
    const float g0 = y0[EV], g1 = y1[EV];
    const bool event = (g0 <= 0.0f && g1 >= 0.0f) || (g0 >= 0.0f && g1 <= 0.0f);
    if (event) event_step<MODEL, INTEG>(P, c, y0, f0, y1);
    post_integrate<MODEL>(y1);
    return event;
}

// The counter-word layout and the TimeLimit, read from the kernel arguments once at kernel
// start and pinned in SGPRs (pin_s): read where they are used, after the integration, they
// were scalar loads with a wait in the tail of a lone wave (+2 % per step at N = 65536).
struct CounterLayout {
    uint32_t el_mask, ep_shift;
    int32_t max_steps;
    __device__ __forceinline__ explicit CounterLayout(const KParams& P)
        : el_mask(P.el_mask), ep_shift(P.ep_shift), max_steps(P.max_steps)
    {
        pin_s(el_mask);
        pin_s(ep_shift);
        pin_s(max_steps);
    }
    // gym TimeLimit (main_6DOF.py:21): elapsed += 1; at the limit done = True and
    // info["TimeLimit.truncated"] = not done. Returns the new elapsed count, saturated at el_mask
    // (>= max_steps): an env stepped on past its TimeLimit without a reset keeps reporting
    // done / truncated instead of wrapping into the episode field.
    __device__ __forceinline__ int32_t time_limit(uint32_t cw, bool& done, bool& trunc) const
    {
        const int32_t el = min((int32_t)(cw & el_mask) + 1, (int32_t)el_mask);
        trunc = false;
        if (max_steps > 0 && el >= max_steps) {
            trunc = !done;
            done = true;
        }
        return el;
    }
    // the counter word of a reset env: episode + 1, elapsed 0
    __device__ __forceinline__ uint32_t next_episode(uint32_t cw) const { return ((cw >> ep_shift) + 1u) << ep_shift; }
    // the elapsed field set to `el`
    __device__ __forceinline__ uint32_t with_elapsed(uint32_t cw, int32_t el) const
    {
        return (cw & ~el_mask) | ((uint32_t)el & el_mask);
    }
};

// terminal obs / return / length of a done env (info["terminal_observation"], Monitor):
// row i of [N][NS] as 16-B stores (rows are 4-B aligned; gfx950 buffer stores need only
// dword alignment), NS = 14 -> 3 x 16 B + 8 B, NS = 7 -> 16 B + 12 B. AUX: cache policy
template <int NS, int AUX, bool SCALARS = true>
__device__ __forceinline__ void store_terminal(const Bufs& B, uint32_t i, uint32_t vo, uint32_t plane, const float* o,
                                               float ret, int32_t el)
{
    const rsrc_t tr = make_rsrc(B.term_obs, (uint64_t)NS * plane);
    const uint32_t ro = NS == 14 ? (i << 6) - (i << 3) : i * (NS * 4u);  // i * 56 without v_mul_lo_u32
    auto u4 = [&](int j) {
        return u32x4{__float_as_uint(o[j]), __float_as_uint(o[j + 1]), __float_as_uint(o[j + 2]),
                     __float_as_uint(o[j + 3])};
    };
#pragma unroll
    for (int j = 0; j + 4 <= NS; j += 4) __builtin_amdgcn_raw_buffer_store_b128(u4(j), tr, (int)(ro + j * 4), 0, AUX);
    if constexpr (NS % 4 == 2)
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(o[NS - 2]), __float_as_uint(o[NS - 1])}, tr,
                                              (int)(ro + (NS - 2) * 4), 0, AUX);
    else if constexpr (NS % 4 == 3)
        __builtin_amdgcn_raw_buffer_store_b96(
            u32x3{__float_as_uint(o[NS - 3]), __float_as_uint(o[NS - 2]), __float_as_uint(o[NS - 1])}, tr,
            (int)(ro + (NS - 3) * 4), 0, AUX);
    if constexpr (SCALARS) {
        bst_f<AUX>(make_rsrc(B.term_ret, plane), ret, vo, 0);
        bst_u<AUX>(make_rsrc(B.term_len, plane), (uint32_t)el, vo, 0);
    }
}

// per-env step outputs owned by the caller: reward, done (unless they travel in the obs row),
// truncated, optional terms
template <int NT, bool REWARD_DONE = true>
__device__ __forceinline__ void store_outputs(const StepIO& io, uint32_t i, uint32_t vo, uint32_t plane, uint32_t n,
                                              float r, bool done, bool trunc, const float* t, bool bv, float status)
{
    if constexpr (REWARD_DONE) {
        bst_f<kOutAux>(make_rsrc(io.reward, plane), r, vo, 0);
        bst_u8<kOutAux>(make_rsrc(io.done, n), (uint8_t)done, i);
    }
    if (io.truncated) bst_u8<kOutAux>(make_rsrc(io.truncated, n), (uint8_t)trunc, i);
    if (io.terms) {
        const rsrc_t tr = make_rsrc(io.terms, (uint64_t)(NT + 2) * plane);
#pragma unroll
        for (int j = 0; j < NT; ++j) bst_f(tr, t[j], vo, j * plane);
        bst_f(tr, bv ? 1.0f : 0.0f, vo, NT * plane);           // info["bounds_violation"]
        bst_f(tr, status, vo, (NT + 1) * plane);  // solve_ivp status: 1 ground event, -1 non-finite state, 0
    }
}

// The structs below cross between translation units as bytes (void* + memcpy: a type of the
// anonymous namespace cannot appear in a cross-TU signature). Every TU gets them from this header,
// so the layouts agree; RolloutIO (rocket_rollout.inc) and PpoLaunch (rocket_ppo.inc) assert the
// same where they are defined.
static_assert(std::is_trivially_copyable_v<KParams>, "KParams crosses TUs by memcpy");
static_assert(std::is_trivially_copyable_v<XParams>, "XParams crosses TUs by memcpy");
static_assert(std::is_trivially_copyable_v<Bufs>, "Bufs crosses TUs by memcpy");
static_assert(std::is_trivially_copyable_v<StepIO>, "StepIO crosses TUs by memcpy");

}  // namespace

// Host side: the one place where a handle's runtime model / integrator / precision picks a kernel
// instantiation. A launch site passes a generic lambda and reads the template arguments off the
// compile-time tags it is called with; the arms keep the order in which the kernels were first
// instantiated (what else a device module holds, and in which order, can change its machine code).
template <int V>
using tag = std::integral_constant<int, V>;

// f(tag<PREC>): the policy kernels' PREC 0 (fp32) / 1 (bf16) / 2 (fp16x3)
template <class F>
inline void dispatch_prec(int prec, F&& f)
{
    if (prec == 1) f(tag<1>{});
    else if (prec == 2) f(tag<2>{});
    else f(tag<0>{});
}

// f(tag<MODEL>, tag<INTEG>) of an RK4 / Euler env
template <class F>
inline void dispatch_env(int model, int integ, F&& f)
{
    const bool euler = integ == RR_INT_EULER;
    if (model == RR_MODEL_6DOF && !euler) f(tag<6>{}, tag<RR_INT_RK4>{});
    else if (model == RR_MODEL_6DOF) f(tag<6>{}, tag<RR_INT_EULER>{});
    else if (!euler) f(tag<3>{}, tag<RR_INT_RK4>{});
    else f(tag<3>{}, tag<RR_INT_EULER>{});
}

// f(tag<MODEL>, tag<INTEG>, tag<PREC>)
template <class F>
inline void dispatch_env_prec(int model, int integ, int prec, F&& f)
{
    dispatch_env(model, integ, [&](auto m, auto i) { dispatch_prec(prec, [&](auto p) { f(m, i, p); }); });
}

// f(std::true_type) / f(std::false_type): a kernel's bool template argument
template <class F>
inline void dispatch_flag(bool v, F&& f)
{
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

namespace {

// What the hidden entry points below are handed besides the kernel's own IO struct: one launch of
// an env kernel of the collect units (rrc_launch_collect / _eval / _eval_trace) ...
struct EnvLaunch {
    int model, integ, prec;  // the dispatch_env_prec arm
    unsigned grid;
    float* state;
    uint32_t n, mode;
    const void *kp, *bufs;   // the caller's KParams / Bufs
    void* stream;
};
// ... and one of an exact-mode step (rrx_launch_exact). variant bit 0: the lean 6DOF kernel,
// bit 1: [NA][N] action planes
struct ExactLaunch {
    int model, variant;
    unsigned grid;
    const void* xp;          // XParams on the device
    const void* bufs;        // the caller's Bufs
    double* state64;
    void* stream;
};
// ... and one whole exact-mode evaluation (rrx_launch_eval_exact)
struct EvalExactLaunch {
    int model, prec;         // eval_exact_kernel<MODEL, PREC>
    unsigned grid;           // workgroups of rol::kEnvsPerBlock envs
    const void* xp;          // XParams on the device
    const void* bufs;        // the caller's Bufs
    double* state64;
    void* stream;
};
// ... and where rr_rollout_collect_stats's two kernels put the statistics (rr_rollout_stats,
// rocket_hip.h, plus the row count), beside the collect's EnvLaunch / RolloutIO
struct CollectStatsIO {
    uint64_t* partials;      // [rows][RR_RSTAT_SLOTS], 128-B aligned
    uint64_t* out;           // [RR_RSTAT_SLOTS]
    uint64_t* accum;         // [RR_RSTAT_SLOTS] or nullptr
    uint32_t rows;           // ceil(n / 64): the collect's live waves
};
static_assert(std::is_trivially_copyable_v<CollectStatsIO>, "CollectStatsIO crosses TUs by memcpy");
// ... and the Categorical head of rollout_discrete/rocket_rollout_discrete.hip's kernels, beside the
// collect's EnvLaunch / RolloutIO or the evaluation's EnvLaunch / EvalIO: the number of choices and
// their [gimbal, thrust] rows (rows >= n_choices are zeros and never read)
struct DiscHead {
    int n_choices;
    float table[4][2];
};
static_assert(std::is_trivially_copyable_v<DiscHead>, "DiscHead crosses TUs by memcpy");
// ... and the noise key of the sampled evaluations (eval_sampled/, eval_sampled_discrete/), beside the
// evaluation's EnvLaunch / EvalIO: the words of splitmix64(seed), as RolloutIO carries them, and the device
// iteration word the kernel reads once at entry
struct EvalSample {
    uint32_t seed_lo, seed_hi;
    const uint64_t* iter;
};
static_assert(std::is_trivially_copyable_v<EvalSample>, "EvalSample crosses TUs by memcpy");
static_assert(std::is_trivially_copyable_v<EvalExactLaunch>, "EvalExactLaunch crosses TUs by memcpy");
static_assert(std::is_trivially_copyable_v<EnvLaunch>, "EnvLaunch crosses TUs by memcpy");
static_assert(std::is_trivially_copyable_v<ExactLaunch>, "ExactLaunch crosses TUs by memcpy");

// a struct of the calling unit, taken over as bytes
template <class T>
inline T from_unit(const void* p)
{
    T v;
    std::memcpy(&v, p, sizeof(T));
    return v;
}

}  // namespace

// The hidden entry points (not part of the C-ABI) through which the main translation unit launches
// the kernels compiled in the others. Defined in rocket_exact.hip / rocket_collect.hip /
// eval_trace/rocket_eval_trace.hip (rrc_launch_eval_trace) / eval_exact/rocket_eval_exact.hip
// (rrx_launch_eval_exact) / collect_stats/rocket_collect_stats.hip (rrc_launch_collect_stats) /
// ppo_opts/rocket_ppo_opts.hip (rrc_launch_learner_opts, a PpoOptsLaunch); the
// main TU adds weak stand-ins, so that a library built from rocket_hip.hip alone still loads.
// launch points to the caller's ExactLaunch / EnvLaunch / EvalExactLaunch / PpoLaunch, io to its
// StepIO / RolloutIO / EvalIO, trace to its EvalTraceIO, stats to its CollectStatsIO.
extern "C" {
__attribute__((visibility("hidden"))) int rrx_launch_exact(const void* launch, const void* io);
__attribute__((visibility("hidden"))) int rrx_launch_eval_exact(const void* launch, const void* io);
// eval_exact_trace/rocket_eval_exact_trace.hip: the recording one-launch exact-mode evaluation; launch / io as
// rrx_launch_eval_exact, trace points to the caller's EvalTraceIO
__attribute__((visibility("hidden"))) int rrx_launch_eval_exact_trace(const void* launch, const void* io, const void* trace);
// eval_exact_discrete/rocket_eval_exact_discrete.hip: the Categorical policy's one-launch exact-mode evaluation;
// launch / io as rrx_launch_eval_exact, head points to the caller's DiscHead
__attribute__((visibility("hidden"))) int rrx_launch_eval_exact_discrete(const void* launch, const void* io, const void* head);
__attribute__((visibility("hidden"))) int rrc_launch_collect(const void* launch, const void* io);
__attribute__((visibility("hidden"))) int rrc_launch_eval(const void* launch, const void* io);
__attribute__((visibility("hidden"))) int rrc_launch_eval_trace(const void* launch, const void* io, const void* trace);
__attribute__((visibility("hidden"))) int rrc_launch_collect_stats(const void* launch, const void* io, const void* stats);
__attribute__((visibility("hidden"))) int rrc_launch_learner(const void* launch, void* stream);
__attribute__((visibility("hidden"))) int rrc_launch_learner_opts(const void* launch, void* stream);
// bc/rocket_bc.hip: rr_bc_update's launches, a BcLaunch
__attribute__((visibility("hidden"))) int rrc_launch_bc(const void* launch, void* stream);
// discrete/rocket_discrete.hip: the Categorical policy's launches, a DiscreteLaunch
__attribute__((visibility("hidden"))) int rrc_launch_discrete(const void* launch, void* stream);
// bc_discrete/rocket_bc_discrete.hip: rr_bc_update_discrete's launches, a BcLaunch with n_choices and a sink
__attribute__((visibility("hidden"))) int rrc_launch_bc_discrete(const void* launch, void* stream);
// a2c/rocket_a2c.hip: rr_a2c_update's launches, an A2cLaunch
__attribute__((visibility("hidden"))) int rrc_launch_a2c(const void* launch, void* stream);
// a2c_discrete/rocket_a2c_discrete.hip: rr_a2c_update_discrete's launches, an A2cDiscreteLaunch (rocket_ppo.inc,
// beside the A2cLaunch it extends)
__attribute__((visibility("hidden"))) int rrc_launch_a2c_discrete(const void* launch, void* stream);
// rollout_discrete/rocket_rollout_discrete.hip: the Categorical policy's one-launch collect (multi != 0),
// its per-step launch and its one-launch evaluation; head points to the caller's DiscHead
__attribute__((visibility("hidden"))) int rrc_launch_rollout_discrete(const void* launch, const void* io, const void* head,
                                                                      int multi);
__attribute__((visibility("hidden"))) int rrc_launch_eval_discrete(const void* launch, const void* io, const void* head);
// collect_stats_discrete/rocket_collect_stats_discrete.hip: the Categorical policy's one-launch collect with the
// episode statistics and their reduction; head / stats point to the caller's DiscHead / CollectStatsIO
__attribute__((visibility("hidden"))) int rrc_launch_collect_discrete_stats(const void* launch, const void* io,
                                                                            const void* head, const void* stats);
// eval_trace_discrete/rocket_eval_trace_discrete.hip: the Categorical policy's recording one-launch evaluation;
// trace points to the caller's EvalTraceIO, choice is the device plane of the winning indices or nullptr
__attribute__((visibility("hidden"))) int rrc_launch_eval_discrete_trace(const void* launch, const void* io,
                                                                         const void* head, const void* trace, void* choice);
// discrete_opts/rocket_ppo_discrete_opts.hip: rr_ppo_update_discrete_opts's launches, a DiscreteOptsLaunch
__attribute__((visibility("hidden"))) int rrc_launch_discrete_opts(const void* launch, void* stream);
// eval_sampled/rocket_eval_sampled.hip: the one-launch evaluation under the sampled action; launch / io as
// rrc_launch_eval, sample points to the caller's EvalSample, trace to its EvalTraceIO or is nullptr (plain)
__attribute__((visibility("hidden"))) int rrc_launch_eval_sampled(const void* launch, const void* io, const void* sample,
                                                                  const void* trace);
// eval_sampled_discrete/rocket_eval_sampled_discrete.hip: the Categorical policy's; head / choice as
// rrc_launch_eval_discrete_trace (choice only with a trace)
__attribute__((visibility("hidden"))) int rrc_launch_eval_discrete_sampled(const void* launch, const void* io,
                                                                           const void* head, const void* sample,
                                                                           const void* trace, void* choice);
}
