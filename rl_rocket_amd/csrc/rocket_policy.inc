// rocket_policy.inc — on-device PPO rollout kernels (SURVEY.md §8f rank 2, BASELINE
// configs[4]): the SB3 1.6 MlpPolicy actor-critic forward + Gaussian sample fused into one
// launch on fp32 MFMA, the timeout bootstrap, and GAE.
//
// Policy (stable_baselines3 ActorCriticPolicy defaults for PPO "MlpPolicy", the
// reference's sb3_config["policy_type"], configuration_file.py:41): separate pi / vf
// towers obs -> 64 -> 64 with tanh, action mean = Linear(64, act), value = Linear(64, 1),
// state-independent log_std. Sampling a = mean + exp(log_std) * eps, eps ~ N(0, 1);
// log_prob = sum(-eps^2 / 2 - log_std - log(2 pi) / 2); the env receives clip(a, -1, 1)
// (SB3 collect_rollouts clips to the Box action space).
//
// MFMA mapping (v_mfma_f32_32x32x2_f32, exact fp32 = an fmaf chain; lane l holds
// A[i = l&31][k = l>>5], B[k = l>>5][j = l&31]; D[i][j] in register reg of lane l with
// j = l&31, i = (reg&3) + 8(reg>>2) + 4(l>>5)): every layer computes Y^T = W^T X^T with
// M = hidden unit, N = env (32 envs per tile), so a layer's D tile is the next layer's B
// operand as it stands (register reg supplies the k pair i(reg, 0), i(reg, 1)) and the
// weights are packed on the host in that fragment order (rl_rocket_amd/rollout.py,
// pack_policy; offsets from rr_policy_layout). One wave = 64 envs = 2 N tiles; per tower
// 2 x KP1 x 2 + 2 x 2 x 32 x 2 MFMAs (156 for 14 observations). The packed parameters
// (~42 KB) are staged once per workgroup in LDS.
//
// bf16 variant (PREC = 1, rr_policy_* precision RR_POLICY_BF16; opt-in, not SB3-exact):
// v_mfma_f32_32x32x16_bf16 with fp32 accumulation. obs, W1, the layer-1 activations and W2
// are rounded to bf16 (RNE); biases, tanh, heads, log_std and sampling stay fp32. Lane l
// holds A[i = l&31][k = 8(l>>5) + j], B[k = 8(l>>5) + j][j' = l&31] in element j of its
// 8-element fragment; the D tile of layer 1 feeds layer 2 as B without lane movement:
// registers 8s..8s+7 of tile t form k-step (t, s), whose element j of lane half h is hidden
// unit 32t + 16s + 8(j>>2) + 4h + (j&3), and W2 is packed in that permuted k order.
// Per tower 2 x KP1 + 2 x 2 x 2 MFMAs (10 for 14 observations).

//
// split-fp16 variant (PREC = 2, RR_POLICY_FP16X3; fp32-accurate): v_mfma_f32_32x32x16_f16 with
// every operand v carried as two fp16 halves, v * 2^8 = hi + lo (hi = fp16(v 2^8), lo =
// fp16(v 2^8 - hi): 22 significant bits; the 2^8 keeps the low halves of O(1e-2) values out
// of the fp16 subnormals), and each k step as three MFMAs, lo_A hi_B + hi_A lo_B + hi_A hi_B
// (the lo lo term is 2^-22 of the product). Accumulators run at 2^16 scale (biases packed
// pre-scaled); the 2^-16 folds into the tanh's exponent constant. Same fragment layout as bf16,
// weights packed as [hi, lo] planes. Products carry ~2^-21 relative error against fp32's 2^-24,
// at 3 x 32 instead of 8 x 64 MFMA cycles per 16 k.
//
// The including translation unit defines RR_POL_PREFETCH_A (0 or 1, see kPolPrefetchA) first.
#pragma once

#include "rocket_device.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// layer-2 A fragments read a group ahead (a second register set) in the collect kernels' translation
// unit (rocket_collect.hip: MFMA accumulators in VGPRs, one wave per SIMD); the main translation
// unit's per-step rollout kernels keep one set: there the extra registers would cost the split-fp16
// kernel its second wave per SIMD (248 -> 268 registers). The translation unit chooses:
// rocket_hip.hip defines RR_POL_PREFETCH_A 0, rocket_collect.hip 1.
#ifndef RR_POL_PREFETCH_A
#error "define RR_POL_PREFETCH_A (0: one A fragment set, 1: read a group ahead) before including rocket_policy.inc"
#endif
constexpr bool kPolPrefetchA = RR_POL_PREFETCH_A;

// packed-f32 tanh (v_pk_mul/add/fma_f32 on register pairs) on the fp32 and bf16 towers (bit p set
// for precision p; the split-fp16 path has its own scaled tanh)
constexpr unsigned kPolPackedTanh = 3;

// Folded tanh on the fp32 towers of the rollout pack (rr_policy_pack, PREC 0). A hidden unit is
// tanh(x) = 1 - 2 r with r = 1 / (1 + 2^(2 x log2 e)). The packer folds the affine parts into
// the weights, so a tower carries r, not tanh(x), and a hidden unit costs exp2, add, rcp:
//   layer 1:  W1' = c W1, b1' = c b1                        (c = 2 log2 e: the accumulator is 2x log2 e)
//   layer 2:  W2' = -2c W2, b2' = c (b2 + sum_k W2[., k])    (W2 (1 - 2 r1) + b2, times c)
//   heads:    W' = -2 W, b' = b + sum_k W[., k]              (mean / value = W (1 - 2 r2) + b)
// (sums in fp64, one rounding). The per-value v_mul (the 2 log2 e scale) and v_fma (1 - 2 r) of
// the unfolded form leave the collect's VALU stream. The PPO learner (rocket_ppo.inc) packs its
// own unfolded image and runs the unfolded tanh. The fold is the only form of the fp32 rollout pack
// (the unfolded A/B build was removed in round 6 so that the host's reference packer,
// rl_rocket_amd.rollout.PolicyPack.pack_reference, and the device packer can never disagree).
constexpr bool kPolFoldTanh = true;

namespace pol {

constexpr int kH = 64;                                  // net_arch [64, 64]
constexpr int kNT = 1;                                  // env tiles per wave (32 envs, 2 waves per SIMD)
constexpr int kEPW = 32 * kNT;                          // envs per wave
constexpr int kWaves = kNT == 1 ? 8 : 4;                // waves per workgroup (2 / 1 per SIMD)
constexpr int kThreads = kWaves * kWave;
constexpr int kEnvsPerBlock = kWaves * kEPW;

// layer-1 B operand of one k step: one f32 (32x32x2) or 8 bf16 (32x32x16)
template <int PREC> struct XOp { using T = float; };
template <> struct XOp<1> { using T = bf16x8; };
struct F16Pair {
    f16x8 hi, lo;
};
template <> struct XOp<2> { using T = F16Pair; };

constexpr float kF16In = 256.0f;            // operand scale of the split-fp16 path (2^8)
constexpr float kF16Out = 1.0f / 65536.0f;  // accumulator scale back (2^-16)
constexpr float kF16Max = 65504.0f;         // largest finite fp16

// An obs component at the operand scale, saturated into fp16's finite range: past |obs| = 255.875
// (65504 / 2^8) the conversion of split_f16 gives hi = +-inf, lo = -+inf and every hidden unit
// inf - inf. The row is then evaluated at the obs clamped to +-255.875 (hi = +-65504, lo = 0: both
// halves come from the clamped value). One v_med3_f32, which returns min3 of its operands when one
// is NaN: a NaN component reads as -255.875 and +-inf as +-255.875 (every input gives finite
// outputs on this path; the fp32 and bf16 paths hand a NaN on). Values inside the range keep their
// bits.
__device__ __forceinline__ float f16_operand(float x) { return __builtin_amdgcn_fmed3f(kF16In * x, -kF16Max, kF16Max); }

// v = hi + lo (fp16 halves of v, element-wise; v already scaled). Both halves are converted with
// packed RNE conversions; lo = v - float(hi) has one rounding whichever instruction forms it.
__device__ __forceinline__ void split_f16(const float (&v)[8], F16Pair& out)
{
    typedef float f32x8 __attribute__((ext_vector_type(8)));
    const f32x8 vv = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
    out.hi = __builtin_convertvector(vv, f16x8);
    f32x8 d;
    typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));
    const u32x4_ hp = __builtin_bit_cast(u32x4_, out.hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a, b;
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(a) : "v"(hp[j]), "v"(v[2 * j]));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(b) : "v"(hp[j]), "v"(v[2 * j + 1]));
        d[2 * j] = a;
        d[2 * j + 1] = b;
    }
    out.lo = __builtin_convertvector(d, f16x8);
}

// Packed parameter layout (floats). Per tower (pi, then vf), fp32 (PREC 0):
//   L1A [2 m][KP1 s][64 lane]             W1[32m + (l&31)][2s + (l>>5)] (0 past obs_dim)
//   B1  [2 m][2 half][16 reg]             b1[32m + row(reg, half)]
//   L2A [2 m'][2 t][4 g][64 lane][4 r]    W2[32m' + (l&31)][32t + row(4g + r, l>>5)]
//   B2  [2 m'][2 half][16 reg]            b2[32m' + row(reg, half)]
// bf16 (PREC 1; 8 bf16 = 4 floats per lane and k step):
//   L1A [2 m][KP1 s][64 lane][8 j]        W1[32m + (l&31)][16s + 8(l>>5) + j] (0 past obs_dim)
//   L2A [2 m'][2 t][2 s][64 lane][8 j]    W2[32m' + (l&31)][32t + 16s + 8(j>>2) + 4(l>>5) + (j&3)]
// then HA [act][2 m'][2 half][16 reg] = W_action[a][32m' + row], HV [2][2][16] = W_value[0][...],
// HB [4] = b_action (padded), VB [4] = b_value, LS [4] = log_std.
// split fp16 (PREC 2): as bf16 with fp16 elements of W 2^8, each of L1A and L2A a [hi, lo]
// pair of planes; B1 / B2 hold b 2^16.
template <int OBS, int ACT, int PREC = 0>
struct Layout {
    static constexpr int KP1 = PREC ? (OBS + 15) / 16 : (OBS + 1) / 2;  // layer-1 k steps
    static constexpr int L1A = 0;
    static constexpr int L1PLANE = 2 * KP1 * 64 * (PREC ? 4 : 1);      // floats of one L1A plane
    static constexpr int B1 = L1A + L1PLANE * (PREC == 2 ? 2 : 1);
    static constexpr int L2A = B1 + 64;
    static constexpr int L2PLANE = PREC ? 2048 : 4096;
    static constexpr int B2 = L2A + L2PLANE * (PREC == 2 ? 2 : 1);
    static constexpr int TOWER = B2 + 64;
    static constexpr int PI = 0, VF = TOWER;
    static constexpr int HA = 2 * TOWER;
    static constexpr int HV = HA + ACT * 64;
    static constexpr int HB = HV + 64;
    static constexpr int VB = HB + 4;
    static constexpr int LS = VB + 4;
    static constexpr int SIZE = LS + 4;  // floats; multiple of 4
    static_assert(SIZE % 4 == 0, "16-B staging");
};

__device__ __forceinline__ float tanh_fast(float x)
{
    // 1 - 2 / (e^{2x} + 1): saturates to +-1 through inf / 0, abs error ~1e-7 near 0
    const float e = __builtin_amdgcn_exp2f(x * 2.88539008177792681f);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// tanh_fast of every register of a tile; PK: the mul / add / fma on register pairs
template <bool PK>
__device__ __forceinline__ void tanh_tile(f32x16& h)
{
    if constexpr (PK) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const f32x2 y = f32x2{h[r], h[r + 1]} * 2.88539008177792681f;
            const f32x2 d = f32x2{__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)} + 1.0f;
            const f32x2 t = 1.0f - 2.0f * f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
            h[r] = t.x;
            h[r + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = tanh_fast(h[r]);
    }
}

// folded tanh (kPolFoldTanh): the tile holds 2 x log2 e; leaves r = 1 / (1 + 2^acc) in place,
// stage by stage over the whole tile (each transcendental's result is consumed a stage later)
__device__ __forceinline__ void tanh_tile_folded(f32x16& h)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) h[r] = __builtin_amdgcn_exp2f(h[r]);
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const f32x2 d = f32x2{h[r], h[r + 1]} + 1.0f;
        h[r] = d.x;
        h[r + 1] = d.y;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) h[r] = __builtin_amdgcn_rcpf(h[r]);
}

// split-fp16 path: tanh of an accumulator at 2^16 scale, times OUT (2^8 for the next
// layer's operand, 1 for the heads): OUT (1 - 2 / (e^{2x} + 1)), x = acc 2^-16
template <bool TO_OPERAND>
__device__ __forceinline__ void tanh_tile_scaled(f32x16& h)
{
    constexpr float OUT = TO_OPERAND ? kF16In : 1.0f;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const f32x2 y = f32x2{h[r], h[r + 1]} * (2.88539008177792681f * kF16Out);
        const f32x2 d = f32x2{__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)} + 1.0f;
        const f32x2 t = OUT - (2.0f * OUT) * f32x2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
        h[r] = t.x;
        h[r + 1] = t.y;
    }
}

// accumulator tile initialised with the bias of its rows (D layout: b[row(reg, half)])
__device__ __forceinline__ f32x16 bias_tile(const float* __restrict__ b)
{
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = b[r];
    return c;
}

// One tower's two hidden layers for the wave's env tiles, in four stages (tower_l1 ->
// tower_act1 -> tower_l2 -> tower_act2 = tower) so a caller can interleave two towers' MFMA
// and VALU work; x[n][s] = B operands of layer 1 (fp32, lane l: obs[env 32n + (l&31)][2s +
// (l>>5)]; bf16: element j = obs[..][16s + 8(l>>5) + j]).
// Layer 1 MFMAs; the accumulators start at the bias: tanh(b + W x).
template <int OBS, int ACT, int PREC, int kNT = pol::kNT>
__device__ __forceinline__ void tower_l1(const float* __restrict__ P,
                                         const typename XOp<PREC>::T (&x)[kNT][Layout<OBS, ACT, PREC>::KP1],
                                         int lane, f32x16 (&h1)[2][kNT])
{
    using L = Layout<OBS, ACT, PREC>;
    constexpr int KP1 = L::KP1;
    const int half = lane >> 5;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const f32x16 b = bias_tile(P + L::B1 + (m * 2 + half) * 16);
#pragma unroll
        for (int n = 0; n < kNT; ++n) h1[m][n] = b;
    }
    // fp32: the A fragment of (s, m) read a step ahead in the collect TU (kPolPrefetchA, as layer 2)
    float a_next = PREC == 0 && kPolPrefetchA ? P[L::L1A + lane] : 0.0f;
#pragma unroll
    for (int s = 0; s < KP1; ++s)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if constexpr (PREC == 0) {
                float a;
                if constexpr (kPolPrefetchA) {
                    a = a_next;
                    const int q1 = s * 2 + m + 1;  // the next (s, m) in loop order
                    if (q1 < 2 * KP1) a_next = P[L::L1A + ((q1 & 1) * KP1 + (q1 >> 1)) * 64 + lane];
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    a = P[L::L1A + (m * KP1 + s) * 64 + lane];
                }
#pragma unroll
                for (int n = 0; n < kNT; ++n)
                    h1[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[n][s], h1[m][n], 0, 0, 0);
            } else if constexpr (PREC == 2) {
                const f16x8* A1 = reinterpret_cast<const f16x8*>(P + L::L1A);
                const f16x8 ahi = A1[(m * KP1 + s) * 64 + lane];
                const f16x8 alo = A1[L::L1PLANE / 4 + (m * KP1 + s) * 64 + lane];
#pragma unroll
                for (int n = 0; n < kNT; ++n)
                    h1[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, x[n][s].hi, h1[m][n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < kNT; ++n)
                    h1[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, x[n][s].lo, h1[m][n], 0, 0, 0);
#pragma unroll
                for (int n = 0; n < kNT; ++n)
                    h1[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, x[n][s].hi, h1[m][n], 0, 0, 0);
            } else {
                const bf16x8 a = reinterpret_cast<const bf16x8*>(P + L::L1A)[(m * KP1 + s) * 64 + lane];
#pragma unroll
                for (int n = 0; n < kNT; ++n)
                    h1[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, x[n][s], h1[m][n], 0, 0, 0);
            }
        }
}

// tanh of the layer-1 tiles (split-fp16: emitted at the next layer's operand scale; FOLD: the
// folded form of the rollout pack, kPolFoldTanh)
template <int PREC, int kNT = pol::kNT, bool FOLD = false>
__device__ __forceinline__ void tower_act1(f32x16 (&h1)[2][kNT])
{
    constexpr bool PK = (kPolPackedTanh >> PREC) & 1;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < kNT; ++n) {
            if constexpr (FOLD) tanh_tile_folded(h1[m][n]);
            else if constexpr (PREC == 2) tanh_tile_scaled<true>(h1[m][n]);
            else tanh_tile<PK>(h1[m][n]);
        }
}

// Layer 2 MFMAs on the post-tanh layer-1 tiles (bf16 / split-fp16: operands converted first)
template <int OBS, int ACT, int PREC, int kNT = pol::kNT>
__device__ __forceinline__ void tower_l2(const float* __restrict__ P, const f32x16 (&h1)[2][kNT], int lane,
                                         f32x16 (&h2)[2][kNT])
{
    using L = Layout<OBS, ACT, PREC>;
    const int half = lane >> 5;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const f32x16 b = bias_tile(P + L::B2 + (m * 2 + half) * 16);
#pragma unroll
        for (int n = 0; n < kNT; ++n) h2[m][n] = b;
    }
    if constexpr (PREC == 0) {
        // k groups (t, g) of 4 k steps; per group the A fragments (ds_read_b128, LDS order m, t, g)
        // of BOTH hidden-unit tiles m, so every k step issues the 2 x kNT accumulators' MFMAs in
        // turn: an f32 32x32x2 MFMA that accumulates onto the result of the MFMA issued two before
        // it waits out the first one's latency (measured 130 cycles per MFMA with m outermost, 67
        // with four accumulators in turn; tools/collect_stamps.py). Each accumulator still sums
        // its k steps in order (bitwise the m-outer result). Group tg + 1's fragments are read
        // before group tg's MFMAs in the collect TU (kPolPrefetchA), so their LDS latency runs
        // under the MFMAs instead of stalling the chain at every group.
        const float4* P4 = reinterpret_cast<const float4*>(P + L::L2A);
        float4 n0 = P4[lane], n1 = P4[8 * 64 + lane];
#pragma unroll
        for (int tg = 0; tg < 8; ++tg) {
            const int t = tg >> 2, g = tg & 3;
            const float4 a0 = kPolPrefetchA ? n0 : P4[tg * 64 + lane];
            const float4 a1 = kPolPrefetchA ? n1 : P4[(8 + tg) * 64 + lane];
            if (kPolPrefetchA && tg + 1 < 8) {
                n0 = P4[(tg + 1) * 64 + lane];
                n1 = P4[(8 + tg + 1) * 64 + lane];
            }
            if constexpr (kPolPrefetchA) __builtin_amdgcn_sched_barrier(0);
            const float av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < kNT; ++n)
                        h2[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][r], h1[t][n][4 * g + r], h2[m][n], 0, 0, 0);
        }
    } else if constexpr (PREC == 2) {
        F16Pair hb[2][kNT][2];  // k step (t, s): registers 8s..8s+7 of layer-1 tile t, split
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int n = 0; n < kNT; ++n)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = h1[t][n][8 * s + j];
                    split_f16(v, hb[t][n][s]);
                }
        const f16x8* A2 = reinterpret_cast<const f16x8*>(P + L::L2A);
        // groups (m, t, s) in LDS order, group q + 1's A halves read before group q's MFMAs (as PREC 0)
        f16x8 hi_next = A2[lane], lo_next = A2[L::L2PLANE / 4 + lane];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int m = q >> 2, t = (q >> 1) & 1, s = q & 1;
            const f16x8 ahi = kPolPrefetchA ? hi_next : A2[q * 64 + lane];
            const f16x8 alo = kPolPrefetchA ? lo_next : A2[L::L2PLANE / 4 + q * 64 + lane];
            if (kPolPrefetchA && q + 1 < 8) {
                hi_next = A2[(q + 1) * 64 + lane];
                lo_next = A2[L::L2PLANE / 4 + (q + 1) * 64 + lane];
            }
            if constexpr (kPolPrefetchA) __builtin_amdgcn_sched_barrier(0);
            // the three products of each env tile in turn (per accumulator in the same order)
#pragma unroll
            for (int n = 0; n < kNT; ++n)
                h2[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, hb[t][n][s].hi, h2[m][n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < kNT; ++n)
                h2[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, hb[t][n][s].lo, h2[m][n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < kNT; ++n)
                h2[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, hb[t][n][s].hi, h2[m][n], 0, 0, 0);
        }
    } else {
        bf16x8 hb[2][kNT][2];  // k step (t, s): registers 8s..8s+7 of layer-1 tile t, RNE to bf16
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int n = 0; n < kNT; ++n)
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 8; ++j) hb[t][n][s][j] = (__bf16)h1[t][n][8 * s + j];
        const bf16x8* A2 = reinterpret_cast<const bf16x8*>(P + L::L2A);
        bf16x8 a_next = A2[lane];  // prefetched a group ahead (as PREC 0)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int m = q >> 2, t = (q >> 1) & 1, s = q & 1;
            const bf16x8 a = kPolPrefetchA ? a_next : A2[q * 64 + lane];
            if (kPolPrefetchA && q + 1 < 8) a_next = A2[(q + 1) * 64 + lane];
            if constexpr (kPolPrefetchA) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < kNT; ++n)
                h2[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[t][n][s], h2[m][n], 0, 0, 0);
        }
    }
}

// tanh of the layer-2 tiles (split-fp16: back to scale 1 for the fp32 heads; FOLD as tower_act1)
template <int PREC, int kNT = pol::kNT, bool FOLD = false>
__device__ __forceinline__ void tower_act2(f32x16 (&h2)[2][kNT])
{
    constexpr bool PK = (kPolPackedTanh >> PREC) & 1;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < kNT; ++n) {
            if constexpr (FOLD) tanh_tile_folded(h2[m][n]);
            else if constexpr (PREC == 2) tanh_tile_scaled<false>(h2[m][n]);
            else tanh_tile<PK>(h2[m][n]);
        }
}

// Returns the layer-2 tiles of the rollout pack (rr_policy_pack): post-tanh (bf16 / split-fp16),
// or r2 with tanh = 1 - 2 r2 (fp32, folded: the heads' packed weights take the affine part).
template <int OBS, int ACT, int PREC, int kNT = pol::kNT>
__device__ __forceinline__ void tower(const float* __restrict__ P,
                                      const typename XOp<PREC>::T (&x)[kNT][Layout<OBS, ACT, PREC>::KP1], int lane,
                                      f32x16 (&h2)[2][kNT])
{
    constexpr bool FOLD = PREC == 0 && kPolFoldTanh;
    f32x16 h1[2][kNT];
    tower_l1<OBS, ACT, PREC, kNT>(P, x, lane, h1);
    tower_act1<PREC, kNT, FOLD>(h1);
    tower_l2<OBS, ACT, PREC, kNT>(P, h1, lane, h2);
    tower_act2<PREC, kNT, FOLD>(h2);
}

// w . h2 over the 64 hidden units of env tile n (each lane half holds 32 of them); the
// sum is valid in both halves, for env row l&31 of tile n
// sum of the even and the odd registers' products as two packed-fp32 chains (16 v_pk_fma_f32 instead
// of 32 v_fma_f32: adjacent registers of a tile and adjacent packed weights are register pairs)
// (load_head reads a head's weights for this lane half into registers; head_dot_w is the dot product
// on them, so a caller can issue the LDS reads early)
struct HeadW {
    f32x2 w[2][8];
};
__device__ __forceinline__ HeadW load_head(const float* __restrict__ w, int half)
{
    HeadW W;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int reg = 0; reg < 16; reg += 2) {
            const float* wp = w + (m * 2 + half) * 16 + reg;
            W.w[m][reg / 2] = f32x2{wp[0], wp[1]};
        }
    return W;
}
template <int kNT = pol::kNT>
__device__ __forceinline__ float head_dot_w(const HeadW& W, const f32x16 (&h2)[2][kNT], int n)
{
    f32x2 s = {0.0f, 0.0f};
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int reg = 0; reg < 16; reg += 2)
            s = __builtin_elementwise_fma(W.w[m][reg / 2], f32x2{h2[m][n][reg], h2[m][n][reg + 1]}, s);
    const float t = s.x + s.y;
    // (the other half's sum by ds_bpermute: its latency hides under the next head's FMAs; a
    // v_permlane32_swap instead costs ~3 VALU slots, which add to the step: r05r, no gain)
    return t + __shfl_xor(t, 32);
}
template <int kNT = pol::kNT>
__device__ __forceinline__ float head_dot(const float* __restrict__ w, const f32x16 (&h2)[2][kNT], int n, int half)
{
    return head_dot_w<kNT>(load_head(w, half), h2, n);
}

// env of lane l (one lane per env): tile = kNT == 2 ? l >> 5 : 0, row = l & 31; with one
// tile per wave lanes 32..63 mirror lanes 0..31 and do not write
__device__ __forceinline__ int lane_env(int lane) { return kNT == 2 ? lane : (lane & 31); }
__device__ __forceinline__ bool lane_writes(int lane) { return kNT == 2 || lane < 32; }
__device__ __forceinline__ int lane_tile(int lane) { return kNT == 2 ? (lane >> 5) : 0; }

// Stage the packed parameters into LDS (whole workgroup, 16-B loads).
template <int OBS, int ACT, int PREC, int NTHR = kThreads>
__device__ __forceinline__ void stage_params(const float* __restrict__ params, float* sp)
{
    using L = Layout<OBS, ACT, PREC>;
    const float4* g4 = reinterpret_cast<const float4*>(params);
    float4* s4 = reinterpret_cast<float4*>(sp);
    // every load issued before the first LDS write (one memory round trip): as a plain loop the
    // compiler waited for each 16-B load before its ds_write, ~11 dependent round trips per
    // workgroup at the start of every launch
    constexpr int NV = L::SIZE / 4, Q = (NV + NTHR - 1) / NTHR;
    float4 v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = (int)threadIdx.x + q * NTHR;
        v[q] = g4[k < NV ? k : NV - 1];  // clamped: an unconditional load keeps v in registers
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = (int)threadIdx.x + q * NTHR;
        if (k < NV) s4[k] = v[q];
    }
}

// Stage this wave's obs block [kEPW][OBS] into LDS (16-B coalesced; optionally copied to
// obs_copy on the way; rows past n are zero).
template <int OBS>
__device__ __forceinline__ void stage_obs(const float* __restrict__ obs, float* __restrict__ obs_copy, float* so,
                                          int64_t wave_env0, int64_t n)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t rows = n - wave_env0 < kEPW ? n - wave_env0 : kEPW;
    const int64_t tot = rows * OBS;  // floats of this wave's block
    const float* src = obs + wave_env0 * OBS;
    float* dst = obs_copy ? obs_copy + wave_env0 * OBS : nullptr;
    if (rows == kEPW && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        for (int k = lane; k < kEPW * OBS / 4; k += kWave) {
            const float4 v = reinterpret_cast<const float4*>(src)[k];
            reinterpret_cast<float4*>(so)[k] = v;
            if (dst) reinterpret_cast<float4*>(dst)[k] = v;
        }
    } else {
        for (int64_t k = lane; k < kEPW * OBS; k += kWave) {
            const float v = k < tot ? src[k] : 0.0f;
            so[k] = v;
            if (dst && k < tot) dst[k] = v;
        }
    }
}

template <int OBS, int ACT, int PREC, int kNT = pol::kNT>
__device__ __forceinline__ void load_x(const float* so, int lane,
                                       typename XOp<PREC>::T (&x)[kNT][Layout<OBS, ACT, PREC>::KP1])
{
    const int half = lane >> 5, r = lane & 31;
#pragma unroll
    for (int n = 0; n < kNT; ++n)
#pragma unroll
        for (int s = 0; s < Layout<OBS, ACT, PREC>::KP1; ++s) {
            if constexpr (PREC == 0) {
                const int k = 2 * s + half;
                x[n][s] = k < OBS ? so[(32 * n + r) * OBS + k] : 0.0f;
            } else if constexpr (PREC == 2) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * s + 8 * half + j;
                    v[j] = k < OBS ? f16_operand(so[(32 * n + r) * OBS + k]) : 0.0f;
                }
                split_f16(v, x[n][s]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * s + 8 * half + j;
                    x[n][s][j] = (__bf16)(k < OBS ? so[(32 * n + r) * OBS + k] : 0.0f);
                }
            }
        }
}

// standard normal from a 32-bit key (Box-Muller on two hashed uniforms)
__device__ __forceinline__ float2 normal2(uint32_t key)
{
    const uint32_t h1 = mix32(key), h2 = mix32(key ^ 0x68E31DA4u);
    const float u1 = ((float)(h1 >> 8) + 1.0f) * 0x1p-24f;  // (0, 1]
    const float u2 = (float)(h2 >> 8) * 0x1p-24f;
    const float r = __builtin_amdgcn_sqrtf(-2.0f * __logf(u1));
    float s, c;
    __sincosf(6.28318530717958648f * u2, &s, &c);
    return make_float2(r * c, r * s);
}

// V(obs) of the wave's staged block for the env of this lane (lane_env)
template <int OBS, int ACT, int PREC>
__device__ __forceinline__ float block_value(const float* sp, const float* so, int lane)
{
    using L = Layout<OBS, ACT, PREC>;
    typename XOp<PREC>::T x[kNT][L::KP1];
    load_x<OBS, ACT, PREC>(so, lane, x);
    const int half = lane >> 5;
    f32x16 h2[2][kNT];
    tower<OBS, ACT, PREC>(sp + L::VF, x, lane, h2);
    float v[kNT];
#pragma unroll
    for (int n = 0; n < kNT; ++n) v[n] = head_dot(sp + L::HV, h2, n, half) + sp[L::VB];
    return v[lane_tile(lane)];
}

// SB3 1.6 collect_rollouts timeout bootstrap for the wave's envs:
// reward_out = reward + gamma * V(term_obs) where truncated, else reward. The value tower
// runs only in waves that hold a truncated env (wave-uniform branch).
template <int OBS, int ACT, int PREC>
__device__ __forceinline__ void bootstrap_wave(const float* sp, float* so2, const float* __restrict__ term_obs,
                                               const uint8_t* __restrict__ truncated,
                                               const float* __restrict__ reward, float gamma,
                                               float* __restrict__ reward_out, int64_t env0, int64_t n, int lane)
{
    const int64_t e = env0 + lane_env(lane);
    const bool ok = e < n && lane_writes(lane);
    const bool tr = ok && truncated[e];
    const float r = ok ? reward[e] : 0.0f;
    float out = r;
    if (__ballot(tr)) {
        stage_obs<OBS>(term_obs, nullptr, so2, env0, n);
        const float v = block_value<OBS, ACT, PREC>(sp, so2, lane);
        out = tr ? fmaf(gamma, v, r) : r;
    }
    if (ok) reward_out[e] = out;
}

// SB3 1.6 RolloutBuffer.compute_returns_and_advantage for env e of a [T][n] rollout
// (rr_gae and the one-launch collect share it, so their results are bitwise equal). The scan
// runs in fp64 and rounds each stored advantage / return once: terminal rewards of +-60 take |A|
// past 128, where an fp32 scan's roundings add up to ~5e-5 over 16 steps (gamma, lambda as doubles
// for the same reason: 0.99f is 0.99 + 9.5e-9).
// STATS (the statistics collect, rocket_rollout_body.inc) also sums over the env's samples y =
// (double)ret[t], d = y - (double)value[t] into s: sum y, y^2, d, d^2, SB3 explained_variance's
// inputs. s is an array reference, not a pointer: a `double* s = nullptr` parameter changed the
// machine code of the kernels that take the sums. Without STATS s is not touched.
template <bool STATS>
__device__ __forceinline__ void gae_env_scan(int64_t T, int64_t n, int64_t e, const float* __restrict__ rewards,
                                             const float* __restrict__ values, const float* __restrict__ starts,
                                             float last_value, float last_done, double gamma, double lam,
                                             float* __restrict__ adv, float* __restrict__ ret, double (&s)[4])
{
    // backward over t in chunks of kC steps whose loads are all issued before the chunk's scan:
    // one memory round trip per chunk instead of one per step (the loads cannot move above the
    // previous step's adv / ret stores on their own; in the collect kernel they read back what the
    // step loop just wrote, so each was a full write-then-read round trip)
    constexpr int kC = 16;
    // the flags are exactly 0 / 1: (1 - start) as a select of the coefficient, two fp64 FMAs per step
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
                if constexpr (STATS) {
                    const double y = (double)rt, d = y - v;
                    s[0] += y;
                    s[1] += y * y;
                    s[2] += d;
                    s[3] += d * d;
                }
            }
    }
}
__device__ __forceinline__ void gae_env(int64_t T, int64_t n, int64_t e, const float* __restrict__ rewards,
                                        const float* __restrict__ values, const float* __restrict__ starts,
                                        float last_value, float last_done, double gamma, double lam,
                                        float* __restrict__ adv, float* __restrict__ ret)
{
    double none[4];  // never read or written
    gae_env_scan<false>(T, n, e, rewards, values, starts, last_value, last_done, gamma, lam, adv, ret, none);
}

}  // namespace pol

// One rollout step's policy work for N envs (rr_policy_act): forward + sample of step t;
// with reward_out != nullptr also the bootstrap of step t-1 (its env outputs are still in
// the env buffers) and the episode-start flags of step t (start_out = float(done)).
template <int OBS, int ACT, int PREC>
__global__ __launch_bounds__(pol::kThreads) void policy_act_kernel(
    const float* __restrict__ params, int64_t n, int64_t id_off, const float* __restrict__ obs, uint32_t seed_lo,
    uint32_t seed_hi, const uint64_t* __restrict__ iter, uint32_t t, float* __restrict__ act_env,
    float* __restrict__ act, float* __restrict__ value, float* __restrict__ logp, float* __restrict__ obs_copy,
    const float* __restrict__ prev_term_obs, const uint8_t* __restrict__ prev_trunc,
    const float* __restrict__ prev_reward, float gamma, float* __restrict__ reward_out,
    const uint8_t* __restrict__ done_flags, float* __restrict__ start_out)
{
    using L = pol::Layout<OBS, ACT, PREC>;
    constexpr int NT = pol::kNT;
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float so_all[pol::kWaves][pol::kEPW * OBS];
    __shared__ __attribute__((aligned(16))) float so2_all[pol::kWaves][pol::kEPW * OBS];
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int64_t env0 = ((int64_t)blockIdx.x * pol::kWaves + wv) * pol::kEPW;
    float* so = so_all[wv];
    const bool live = env0 < n;  // wave-uniform
    pol::stage_params<OBS, ACT, PREC>(params, sp);
    if (live) pol::stage_obs<OBS>(obs, obs_copy, so, env0, n);
    __syncthreads();
    if (!live) return;
    const int64_t e = env0 + pol::lane_env(lane);
    const bool ok = e < n && pol::lane_writes(lane);
    if (start_out && ok) start_out[e] = done_flags[e] ? 1.0f : 0.0f;
    if (reward_out)
        pol::bootstrap_wave<OBS, ACT, PREC>(sp, so2_all[wv], prev_term_obs, prev_trunc, prev_reward, gamma, reward_out,
                                      env0, n, lane);
    typename pol::XOp<PREC>::T x[NT][L::KP1];
    pol::load_x<OBS, ACT, PREC>(so, lane, x);
    const int half = lane >> 5;
    f32x16 h2[2][NT];
    // value tower
    pol::tower<OBS, ACT, PREC>(sp + L::VF, x, lane, h2);
    float v[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) v[nt] = pol::head_dot(sp + L::HV, h2, nt, half) + sp[L::VB];
    // action tower
    pol::tower<OBS, ACT, PREC>(sp + L::PI, x, lane, h2);
    float mean[NT][ACT];
#pragma unroll
    for (int a = 0; a < ACT; ++a)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) mean[nt][a] = pol::head_dot(sp + L::HA + a * 64, h2, nt, half) + sp[L::HB + a];
    // sample (one lane per env)
    const uint64_t it = *iter;
    uint32_t key = mix32((uint32_t)(id_off + e) ^ seed_lo);
    key = mix32(key ^ (uint32_t)it ^ seed_hi);
    key = mix32(key ^ (uint32_t)(it >> 32) ^ (t * 0x9E3779B9u));
    float eps[ACT];
#pragma unroll
    for (int a = 0; a < ACT; a += 2) {
        const float2 z = pol::normal2(key + (uint32_t)a * 0x632BE5ABu);
        eps[a] = z.x;
        if (a + 1 < ACT) eps[a + 1] = z.y;
    }
    const int tile = pol::lane_tile(lane);
    float lp = 0.0f;
    float* stage_out = so;  // the obs block is consumed: reuse it to stage the [kEPW][ACT] action rows
#pragma unroll
    for (int a = 0; a < ACT; ++a) {
        const float ls = sp[L::LS + a];
        const float s = mean[tile][a] + __builtin_amdgcn_exp2f(ls * 1.44269504088896341f) * eps[a];
        lp += -0.5f * eps[a] * eps[a] - ls - 0.918938533204672742f;  // log(2 pi) / 2
        if (pol::lane_writes(lane)) stage_out[pol::lane_env(lane) * ACT + a] = s;
    }
    if (ok) {
        value[e] = v[tile];
        logp[e] = lp;
    }
    // rows of this wave: raw sample and clipped action, [kEPW][ACT] floats each
    const int64_t rows = n - env0 < pol::kEPW ? n - env0 : pol::kEPW;
    for (int k = lane; k < rows * ACT; k += kWave) {
        const float s = stage_out[k];
        act[env0 * ACT + k] = s;
        act_env[env0 * ACT + k] = fminf(1.0f, fmaxf(-1.0f, s));
    }
}

// End of a rollout (rr_policy_bootstrap): the bootstrap of the last step
// (reward_out = reward + gamma * V(term_obs) where truncated) and, if value_out != nullptr,
// V(obs) of every env (SB3 compute_returns_and_advantage's last_values).
template <int OBS, int ACT, int PREC>
__global__ __launch_bounds__(pol::kThreads) void policy_bootstrap_kernel(
    const float* __restrict__ params, int64_t n, const float* __restrict__ term_obs,
    const uint8_t* __restrict__ truncated, const float* __restrict__ reward, float gamma,
    float* __restrict__ reward_out, const float* __restrict__ obs, float* __restrict__ value_out)
{
    using L = pol::Layout<OBS, ACT, PREC>;
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float so_all[pol::kWaves][pol::kEPW * OBS];
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int64_t env0 = ((int64_t)blockIdx.x * pol::kWaves + wv) * pol::kEPW;
    pol::stage_params<OBS, ACT, PREC>(params, sp);
    __syncthreads();
    if (env0 >= n) return;
    if (term_obs)
        pol::bootstrap_wave<OBS, ACT, PREC>(sp, so_all[wv], term_obs, truncated, reward, gamma, reward_out, env0, n,
                                            lane);
    if (value_out) {
        pol::stage_obs<OBS>(obs, nullptr, so_all[wv], env0, n);
        const float v = pol::block_value<OBS, ACT, PREC>(sp, so_all[wv], lane);
        const int64_t e = env0 + pol::lane_env(lane);
        if (e < n && pol::lane_writes(lane)) value_out[e] = v;
    }
}

// Pack an actor-critic's parameters (PyTorch nn.Linear layouts, [out][in] row-major) into
// the fragment-ordered buffer (rr_policy_pack): one thread per packed float.
struct PolSrc {
    const float* p[13];  // pi W1 b1 W2 b2, vf W1 b1 W2 b2, W_action b_action, W_value b_value, log_std
};

// bits of the bf16 nearest to v (RNE; v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t bf16_bits(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }

// split-fp16 weight halves of v 2^8 (RNE): part 0 = hi = fp16(v 2^8), part 1 = lo = fp16(v 2^8 - hi)
__device__ __forceinline__ uint32_t f16_split_bits(float v, int part)
{
    const float w = v * pol::kF16In;
    const _Float16 hi = (_Float16)w;
    return __builtin_bit_cast(uint16_t, part ? (_Float16)(w - (float)hi) : hi);
}

template <int OBS, int ACT, int PREC>
__global__ __launch_bounds__(256) void policy_pack_kernel(PolSrc src, float* __restrict__ dst)
{
    using L = pol::Layout<OBS, ACT, PREC>;
    constexpr int KP1 = L::KP1;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= L::SIZE) return;
    auto row = [](int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; };
    // folded fp32 tanh (kPolFoldTanh): c = 2 log2 e on the towers, -2 on the layer-2 and head
    // weights, the row sums of those weights into the next biases (fp64, one rounding)
    constexpr bool FOLD = PREC == 0 && kPolFoldTanh;
    constexpr double kC = 2.88539008177792681;
    auto rowsum = [](const float* W, int r, int cols) {
        double acc = 0.0;
        for (int q = 0; q < cols; ++q) acc += (double)W[r * cols + q];
        return acc;
    };
    float v = 0.0f;
    if (k < L::HA) {
        const int tw = k / L::TOWER, o = k % L::TOWER;
        const float* const* P = src.p + 4 * tw;  // W1 b1 W2 b2 of this tower
        if (o < L::B1 && PREC == 2) {  // plane p, elements 2q, 2q + 1 of the k-step fragment
            const int p = o / L::L1PLANE, oo = o % L::L1PLANE;
            const int q = oo % 4, lane = (oo / 4) % 64, s = (oo / 256) % KP1, m = oo / (256 * KP1);
            uint32_t bits = 0;
            for (int e = 0; e < 2; ++e) {
                const int kk = 16 * s + 8 * (lane >> 5) + 2 * q + e;
                bits |= f16_split_bits(kk < OBS ? P[0][(32 * m + (lane & 31)) * OBS + kk] : 0.0f, p) << (16 * e);
            }
            v = __builtin_bit_cast(float, bits);
        } else if (o < L::B1) {
            if constexpr (PREC == 0) {
                const int lane = o % 64, s = (o / 64) % KP1, m = o / (64 * KP1);
                const int kk = 2 * s + (lane >> 5);
                v = kk < OBS ? P[0][(32 * m + (lane & 31)) * OBS + kk] : 0.0f;
                if (FOLD) v = (float)(kC * (double)v);
            } else {  // elements 2q, 2q + 1 of lane's 8-element fragment of k step s
                const int q = o % 4, lane = (o / 4) % 64, s = (o / 256) % KP1, m = o / (256 * KP1);
                uint32_t bits = 0;
                for (int e = 0; e < 2; ++e) {
                    const int kk = 16 * s + 8 * (lane >> 5) + 2 * q + e;
                    bits |= bf16_bits(kk < OBS ? P[0][(32 * m + (lane & 31)) * OBS + kk] : 0.0f) << (16 * e);
                }
                v = __builtin_bit_cast(float, bits);
            }
        } else if (o < L::L2A) {
            const int i = o - L::B1, reg = i % 16, half = (i / 16) % 2, m = i / 32;
            v = P[1][32 * m + row(reg, half)] * (PREC == 2 ? 65536.0f : 1.0f);
            if (FOLD) v = (float)(kC * (double)P[1][32 * m + row(reg, half)]);
        } else if (o < L::B2) {
            const int i = o - L::L2A;
            if constexpr (PREC == 2) {
                const int p = i / L::L2PLANE, ii = i % L::L2PLANE;
                const int q = ii % 4, lane = (ii / 4) % 64, s = (ii / 256) % 2, t = (ii / 512) % 2, m = ii / 1024;
                uint32_t bits = 0;
                for (int e = 0; e < 2; ++e) {
                    const int j = 2 * q + e;
                    const int col = 32 * t + 16 * s + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
                    bits |= f16_split_bits(P[2][(32 * m + (lane & 31)) * 64 + col], p) << (16 * e);
                }
                v = __builtin_bit_cast(float, bits);
            } else if constexpr (PREC == 0) {
                const int r = i % 4, lane = (i / 4) % 64, g = (i / 256) % 4, t = (i / 1024) % 2, m = i / 2048;
                v = P[2][(32 * m + (lane & 31)) * 64 + 32 * t + row(4 * g + r, lane >> 5)];
                if (FOLD) v = (float)(-2.0 * kC * (double)v);
            } else {
                const int q = i % 4, lane = (i / 4) % 64, s = (i / 256) % 2, t = (i / 512) % 2, m = i / 1024;
                uint32_t bits = 0;
                for (int e = 0; e < 2; ++e) {
                    const int j = 2 * q + e;
                    const int col = 32 * t + 16 * s + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
                    bits |= bf16_bits(P[2][(32 * m + (lane & 31)) * 64 + col]) << (16 * e);
                }
                v = __builtin_bit_cast(float, bits);
            }
        } else {
            const int i = o - L::B2, reg = i % 16, half = (i / 16) % 2, m = i / 32;
            v = P[3][32 * m + row(reg, half)] * (PREC == 2 ? 65536.0f : 1.0f);
            if (FOLD) {
                const int rw = 32 * m + row(reg, half);
                v = (float)(kC * ((double)P[3][rw] + rowsum(P[2], rw, 64)));
            }
        }
    } else if (k < L::HV) {
        const int i = k - L::HA, reg = i % 16, half = (i / 16) % 2, m = (i / 32) % 2, a = i / 64;
        v = src.p[8][a * 64 + 32 * m + row(reg, half)];
        if (FOLD) v = -2.0f * v;
    } else if (k < L::HB) {
        const int i = k - L::HV, reg = i % 16, half = (i / 16) % 2, m = i / 32;
        v = src.p[10][32 * m + row(reg, half)];
        if (FOLD) v = -2.0f * v;
    } else if (k < L::VB) {
        const int a = k - L::HB;
        v = a < ACT ? src.p[9][a] : 0.0f;
        if (FOLD && a < ACT) v = (float)((double)src.p[9][a] + rowsum(src.p[8], a, 64));
    } else if (k < L::LS) {
        v = k == L::VB ? src.p[11][0] : 0.0f;
        if (FOLD && k == L::VB) v = (float)((double)src.p[11][0] + rowsum(src.p[10], 0, 64));
    } else {
        const int a = k - L::LS;
        v = a < ACT ? src.p[12][a] : 0.0f;
    }
    dst[k] = v;
}

}  // namespace
