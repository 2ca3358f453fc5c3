// rocket_ppo.inc — the PPO minibatch gradient on fp32 MFMA (rr_ppo_grad; SURVEY.md §8f rank 2,
// BASELINE configs[4]: the learner half of the on-device training loop).
//
// Computes, for one minibatch of a device rollout, the gradients that stable_baselines3 1.6
// PPO.train's loss.backward() produces for the MlpPolicy actor-critic (the reference trains
// PPO("MlpPolicy", ..., ent_coef=0.01), main_6DOF.py:62-69; SB3's defaults otherwise):
//   A   = (adv - mean(adv)) / (std(adv) + 1e-8)                      (normalize_advantage; mean and
//         std from fp64 sums, the mean subtracted as a float pair: no rounding of a large mean)
//   r   = exp(log_prob(a) - old_log_prob)
//   pg  = -mean(min(A r, A clamp(r, 1 - clip, 1 + clip)))
//   vf  = mean((ret - V)^2)                                         (clip_range_vf None)
//   ent = -mean(entropy) = -sum(0.5 + 0.5 log 2 pi + log_std)
//   loss = pg + ent_coef ent + vf_coef vf
// with PyTorch's backward conventions where they matter: torch.min splits the gradient of
// equal arguments in halves, clamp passes it on [lo, hi] inclusive, std is the unbiased one.
//
// Work split: the loss separates into a pi part (pi tower, action head, log_std) and a vf part
// (vf tower, value head), so blockIdx.y picks the tower and the two halves never talk. A wave
// takes 32-sample tiles (idx[32 t .. 32 t + 31], gathered from the rollout in HBM):
//   forward   h1 = tanh(W1 x + b1), h2 = tanh(W2 h1 + b2) — rocket_policy.inc's MFMA tower
//             (M = hidden unit, N = sample: the D tile of one layer is the next one's B);
//   heads     mean / V per sample (lane = sample), the loss derivatives dmean / dV per sample;
//   backward  dpre2 = (W_head^T dhead) (1 - h2^2) in the D layout; dh1 = W2^T dpre2 as MFMAs
//             whose A operand is W2 packed transposed (L2T) and whose B operand is dpre2 as it
//             stands; dpre1 = dh1 (1 - h1^2);
//   weights   dW2 += dpre2 h1^T and dW1|db1 += dpre1 [x, 1]^T are sums over samples, so the
//             sample index becomes the MFMA k: dpre2, h1, dpre1, x go through LDS as
//             [unit][sample] tiles (lane = unit, 16 consecutive samples per lane half = one
//             b128 read per 4 k steps) and accumulate in 6 32x32 tiles per wave over all its
//             tiles; db1 rides in the ones column of x (column OBS of the padded 32); db2 and the
//             head gradients are per-unit sums over the LDS tiles (lane = unit).
// Each workgroup sums its 4 waves' accumulators in LDS and writes one partial-gradient vector;
// ppo_finish_kernel sums the workgroups' vectors in a fixed order (deterministic, no atomics)
// and scatters them into the 13 PyTorch gradient tensors, adding the entropy term.
// Then clip_grad_norm_ + Adam: adam_norm_kernel + adam_step_kernel (rr_clip_adam), or, for a whole
// minibatch step in one call (rr_ppo_update), the finish also sums the squared gradients and
// adam_chain_kernel steps, repacks the towers and sums the next minibatch's statistics.
// The types and the kernel templates are here for both translation units that include this file;
// the kernels are instantiated and launched in the collect TU (rocket_collect.hip,
// rrc_launch_learner), which also defines adam_norm_kernel / adam_step_kernel.
// The kernels' bodies carry compile-time options that are all off in the kernels here: the
// value-function clip (VCLIP), raw advantages (NORM false) and the control block of
// rr_ppo_update_opts (CTL: stop word, running statistics). ppo_opts/rocket_ppo_opts.hip instantiates
// them with the options on, in kernels of its own: ppo_prep_body and ppo_grad_tower as functions,
// the finish and optimizer bodies as included text (rocket_ppo_finish_body.inc).
// bc/rocket_bc.hip (rr_bc_update, behaviour cloning) instantiates the pi tower with LOSS 1 and
// includes the same two bodies; discrete/rocket_discrete.hip (rr_ppo_update_discrete, the Categorical
// policy) the pi tower with LOSS 2 over <7, 4> and the same two bodies; bc_discrete/rocket_bc_discrete.hip
// (rr_bc_update_discrete, behaviour cloning of the Categorical policy) the pi tower with LOSS 3 over
// <7, 4>, LOSS 2's head with LOSS 1's derivative, and the same two bodies; a2c/rocket_a2c.hip (rr_a2c_update,
// SB3's A2C) the pi tower with LOSS 4, LOSS 0's Gaussian head with d loss / d log_prob = -A / B, beside the
// unclipped vf tower, the finish body and an optimizer body of its own (RMSprop) or the Adam one;
// a2c_discrete/rocket_a2c_discrete.hip (rr_a2c_update_discrete, A2C for the Categorical policy) the pi tower
// with LOSS 5 over <7, 4>, LOSS 2's head with LOSS 4's derivative, and the A2C unit's other pieces.
#pragma once

#include <type_traits>

#include "rocket_device.h"
#include "rocket_policy.inc"

namespace {

namespace ppo {

constexpr int kWaves = 4;  // one wave per SIMD: 6 accumulator tiles (96 registers) + the tower
constexpr int kThreads = kWaves * kWave;
constexpr int kTile = 32;     // samples per tile (the forward's N)
constexpr int kTS = 40;       // LDS stride of a [unit][sample] tile row (4 kTS = 32 mod 64 banks)
constexpr int kMaxWG = 128;   // workgroups per tower (4 tiles per wave at 65 536 samples)
// partial sums of the advantage statistics (ppo_prep_kernel blocks): one row per thread at the
// 65 536-row minibatch, so the gather's two dependent loads are one round trip each
constexpr int kAdvPart = 256;
static_assert(kAdvPart % kWave == 0 && kAdvPart % 4 == 0, "the gradient kernel's wave sum; adam_chain's blocks");

__device__ __forceinline__ int drow(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// the wave's own LDS writes visible to its other lanes
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS image of one tower's parameters: the forward tower in rocket_policy.inc's fragment order
// (pol::Layout offsets L1A, B1, L2A, B2), then W2 transposed for the backward, the head rows in
// the D order of head_dot, the head biases and log_std.
template <int OBS, int ACT>
struct Pack {
    using L = pol::Layout<OBS, ACT, 0>;
    static constexpr int L2T = L::TOWER;        // [2 m][2 t][4 g][64 lane][4 r] = W2[32t + row(4g + r, l>>5)][32m + (l&31)]
    static constexpr int HW = L2T + 4096;       // [ACT or 1][2 m][2 half][16 reg] = Whead[a][32m + row(reg, half)]
    static constexpr int HB = HW + 64 * ACT;    // 4: head biases
    static constexpr int LS = HB + 4;           // 4: log_std (pi)
    static constexpr int SIZE = LS + 4;
    static_assert(SIZE % 4 == 0, "16-B sections");
};

// Per-tower partial-gradient vector (floats); W2 / W1 in the accumulators' D order.
template <int OBS, int ACT>
struct Part {
    static constexpr int W2 = 0;                // [4 blk = 2 m2 + t1][16 reg][64 lane]: dW2[32 m2 + row(reg, l>>5)][32 t1 + (l&31)]
    static constexpr int W1 = 4096;             // [2 m][16 reg][64 lane]: [dW1 | db1][32 m + row(reg, l>>5)][col = l&31]
    static constexpr int B2 = 6144;             // [64 unit]
    static constexpr int HW = B2 + 64;          // [ACT][64 unit] (vf: row 0)
    static constexpr int HB = HW + 64 * ACT;    // [4]
    static constexpr int LS = HB + 4;           // [4] (pi)
    static constexpr int ST = LS + 4;           // pi: pg sum, clip count, approx-kl sum (LOSS 2: + entropy sum; LOSS 3: -logp, exp(logp), spare, entropy; LOSS 4: -A logp, logp; LOSS 5: -A logp, logp, spare, entropy); vf: squared-error sum
    static constexpr int SIZE = ST + 4;
    static_assert(SIZE % 4 == 0, "16-B rows");
};

template <int OBS, int ACT>
struct Lds {
    static constexpr int kPerWave = 2 * 64 * kTS + 32 * kTS + kTile * 4;  // T0, T1 [64][kTS], XT [32][kTS], DM [32][4]
    static constexpr int SIZE_TILES = Pack<OBS, ACT>::SIZE + kWaves * kPerWave;
    static constexpr int SIZE_RED = kWaves * Part<OBS, ACT>::SIZE;
    static constexpr int SIZE = SIZE_TILES > SIZE_RED ? SIZE_TILES : SIZE_RED;
    static_assert(SIZE * 4 <= 160 * 1024, "LDS budget");
};

// Element k of tower tw's packed image, from the PyTorch tensors.
template <int OBS, int ACT>
__device__ float pack_value(const PolSrc& src, int tw, int k)
{
    using L = pol::Layout<OBS, ACT, 0>;
    using K = Pack<OBS, ACT>;
    constexpr int KP1 = L::KP1;
    const float* W1 = src.p[4 * tw];
    const float* b1 = src.p[4 * tw + 1];
    const float* W2 = src.p[4 * tw + 2];
    const float* b2 = src.p[4 * tw + 3];
    const float* Wh = src.p[tw ? 10 : 8];
    const float* bh = src.p[tw ? 11 : 9];
    const int nh = tw ? 1 : ACT;
    {
        float v = 0.0f;
        if (k < L::B1) {
            const int lane = k % 64, s = (k / 64) % KP1, m = k / (64 * KP1);
            const int col = 2 * s + (lane >> 5);
            v = col < OBS ? W1[(32 * m + (lane & 31)) * OBS + col] : 0.0f;
        } else if (k < L::L2A) {
            const int i = k - L::B1, reg = i % 16, half = (i / 16) % 2, m = i / 32;
            v = b1[32 * m + drow(reg, half)];
        } else if (k < L::B2) {
            const int i = k - L::L2A, r = i % 4, lane = (i / 4) % 64, g = (i / 256) % 4, t = (i / 1024) % 2, m = i / 2048;
            v = W2[(32 * m + (lane & 31)) * 64 + 32 * t + drow(4 * g + r, lane >> 5)];
        } else if (k < L::TOWER) {
            const int i = k - L::B2, reg = i % 16, half = (i / 16) % 2, m = i / 32;
            v = b2[32 * m + drow(reg, half)];
        } else if (k < K::HW) {
            const int i = k - K::L2T, r = i % 4, lane = (i / 4) % 64, g = (i / 256) % 4, t = (i / 1024) % 2, m = i / 2048;
            v = W2[(32 * t + drow(4 * g + r, lane >> 5)) * 64 + 32 * m + (lane & 31)];
        } else if (k < K::HB) {
            const int i = k - K::HW, reg = i % 16, half = (i / 16) % 2, m = (i / 32) % 2, a = i / 64;
            v = a < nh ? Wh[a * 64 + 32 * m + drow(reg, half)] : 0.0f;
        } else if (k < K::LS) {
            const int a = k - K::HB;
            v = a < nh ? bh[a] : 0.0f;
        } else {
            const int a = k - K::LS;
            v = (!tw && a < ACT) ? src.p[12][a] : 0.0f;
        }
        return v;
    }
}

// One tile's gathered inputs (lane: sample j, obs columns 2k + half): x, and for pi the action,
// old log-prob and raw advantage, for vf the return (in av) and, under the value clip, the
// rollout's value (in olp).
template <int OBS, int ACT>
struct TileIn {
    float x[pol::Layout<OBS, ACT, 0>::KP1];
    float a[ACT];
    float olp, av;
};

// The control block of rr_ppo_update_opts (rocket_hip.h RR_PPO_CTL_*: these are its slots). Who
// writes what, so that no block reads a word another block of the same launch writes:
//   the finish launch  reads kStop; the thread that holds a statistic adds it to that statistic's
//                      sum, and the approx_kl one also counts the minibatch and the epoch and writes
//                      kDecide = (approx_kl > 1.5 target_kl);
//   the optimizer launch  reads kDecide: set, it steps nothing and block 0 commits kStop; clear,
//                      block 0 counts the step;
//   the packing and gradient launches  read kStop.
// kDecide stays set after a stop (the finish launches that would clear it return at kStop).
enum Ctl { kStop = 0, kDecide, kSteps, kEvals, kEpochs, kSumPg, kSumVf, kSumEnt, kSumClip, kKlSum, kKlCount, kKlLast };
struct CtlArgs {
    float* ctl;       // null: no control block
    float kl_limit;   // 1.5 target_kl, +inf without one
    int epoch_start;  // this call is an epoch's first minibatch
};

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One thread's share of the advantage statistics: adv[idx[i]] and its square summed over
// i = i0 + j kAdvPart 256 in increasing j, the index loads of four rows issued before their
// advantage loads (two memory round trips per four rows instead of eight)
__device__ __forceinline__ void adv_sums(const float* __restrict__ adv, const int64_t* __restrict__ idx, int64_t bs,
                                        int64_t i0, double& s, double& q)
{
    constexpr int64_t kStride = (int64_t)kAdvPart * 256;
    for (int64_t i = i0; i < bs; i += 4 * kStride) {
        int64_t ix[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ix[r] = i + r * kStride < bs ? idx[i + r * kStride] : -1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (ix[r] >= 0) {
                const double a = adv[ix[r]];
                s += a;
                q += a * a;
            }
        }
    }
}

}  // namespace ppo

// Before the gradient kernel, in one launch: blocks [0, kAdvPart) the partial sums (fp64) of
// adv[idx[i]] and its square for the minibatch statistics (block b: i = b * 256 + thread +
// multiples of kAdvPart * 256; part[2 b] = sum, part[2 b + 1] = sum of squares); the blocks after
// them the two towers' packed LDS images (pack[tower * Pack::SIZE + k], one element per thread),
// which every gradient workgroup then stages with 16-B loads.
// Element k of tower tw's learner image for the Categorical policy: ppo::pack_value, with zeros for the
// heads >= n_choices (the tensors have n_choices rows) and for log_std's slots (there is none)
template <int OBS, int ACT>
__device__ __forceinline__ float discrete_pack_value(const PolSrc& src, int n_choices, int tw, int k)
{
    using K = ppo::Pack<OBS, ACT>;
    if (k >= K::LS) return 0.0f;
    if (tw == 0 && k >= K::HW && k < K::HB && (k - K::HW) / 64 >= n_choices) return 0.0f;
    if (tw == 0 && k >= K::HB && k - K::HB >= n_choices) return 0.0f;
    return ppo::pack_value<OBS, ACT>(src, tw, k);
}

template <int OBS, int ACT>
__device__ __forceinline__ void ppo_prep_body(const float* __restrict__ adv, const int64_t* __restrict__ idx,
                                              int64_t bs, double* __restrict__ part, const PolSrc& src,
                                              float* __restrict__ pack)
{
    using K = ppo::Pack<OBS, ACT>;
    if (blockIdx.x >= ppo::kAdvPart) {
        const int k = (blockIdx.x - ppo::kAdvPart) * 256 + threadIdx.x;
        if (k < 2 * K::SIZE) pack[k] = ppo::pack_value<OBS, ACT>(src, k / K::SIZE, k % K::SIZE);
        return;
    }
    __shared__ double red[2][256 / kWave];
    double s = 0.0, q = 0.0;
    ppo::adv_sums(adv, idx, bs, (int64_t)blockIdx.x * 256 + threadIdx.x, s, q);
    s = ppo::wave_sum(s);
    q = ppo::wave_sum(q);
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red[0][w] = s;
        red[1][w] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ss = 0.0, qq = 0.0;
        for (int k = 0; k < 256 / kWave; ++k) {
            ss += red[0][k];
            qq += red[1][k];
        }
        part[2 * blockIdx.x] = ss;
        part[2 * blockIdx.x + 1] = qq;
    }
}

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void ppo_prep_kernel(const float* __restrict__ adv, const int64_t* __restrict__ idx,
                                                       int64_t bs, double* __restrict__ part, PolSrc src,
                                                       float* __restrict__ pack)
{
    ppo_prep_body<OBS, ACT>(adv, idx, bs, part, src, pack);
}

// One workgroup = 4 waves of one tower (blockIdx.y: 0 pi, 1 vf); writes the workgroup's partial
// gradient vector part[(tower * gridDim.x + blockIdx.x) * Part::SIZE ..]. The tower is a template
// parameter of the body (ppo_grad_tower<..., 0 / 1>): with it a runtime value, the two towers'
// gathers shared registers, and the hazard between one tower's in-flight load and the other's
// zero-initialised destination made every tile wait for its own gather (tools/ppo_stamps.py).
// VCLIP (SB3's clip_range_vf = clip_vf > 0): the vf tower gathers the rollout's value old_val[r]
// with the tile's other rows and its head computes
//   Vc = old + clamp(V - old, -clip_vf, clip_vf), value_loss = mean((ret - Vc)^2),
//   dV = vf_coef 2 (Vc - ret) / B where -clip_vf <= V - old <= clip_vf (torch's clamp passes the
//   gradient on the closed interval), else 0.
// NORM false (normalize_advantage=False): A = adv[idx], the minibatch statistics are not read.
// LOSS 1 (behaviour cloning, bc/rocket_bc.hip; pi tower, NORM false): loss = -mean(log_prob(a)), so
// d loss / d log_prob = -1 / B for every sample: no ratio, no clip; old_lp / adv are not read, and
// the three sums are -log_prob, exp(log_prob) and a spare.
// LOSS 2 (Categorical policy, discrete/rocket_discrete.hip; pi tower over <OBS, 4>): the heads are the
// logits of the first n_choices choices, act holds one float per row (the chosen index, compared
// against k, never used as an address), log_prob = logit_a - logsumexp. PPO's ratio lines are LOSS 0's.
// The entropy H = -sum_k p_k log p_k depends on the state, so its gradient is part of the head
// derivative here (ent_coef is an argument; the Gaussian kernels' finish adds theirs to log_std):
//   dz_k = dlp ((k == a) - p_k) + ent_coef / B p_k (log p_k + H),   0 for k >= n_choices;
// nothing goes to the log_std sums, and a fourth per-sample sum carries H.
// LOSS 3 (behaviour cloning of the Categorical policy, bc_discrete/rocket_bc_discrete.hip; pi tower over
// <OBS, 4>, NORM false): LOSS 2's softmax and entropy lines with LOSS 1's dlp = -1 / B and ent_coef the
// cloning loss's ent_weight:
//   dz_k = -(1 / B) ((k == a) - p_k) + ent_weight / B p_k (log p_k + H),   0 for k >= n_choices;
// no ratio, no clip; old_lp / adv are not read. The four sums are -log_prob, exp(log_prob), a spare and H.
// LOSS 4 (A2C, a2c/rocket_a2c.hip; pi tower): LOSS 0's Gaussian head under SB3 A2C.train's policy loss
// -mean(A log_prob), so d loss / d log_prob = -A / B with A the normalised advantage (NORM: LOSS 0's
// statistics and float-pair mean) or adv[idx] as it is. No ratio, no clip: adv is gathered, old_lp is not
// read (null is legal). The sums are -A log_prob (the policy loss times B), log_prob and a spare.
// LOSS 5 (A2C for the Categorical policy, a2c_discrete/rocket_a2c_discrete.hip; pi tower over <OBS, 4>):
// LOSS 2's softmax and entropy lines with LOSS 4's dlp = -A / B (A gathered, normalised under NORM) and
// ent_coef an argument:
//   dz_k = -(A / B) ((k == a) - p_k) + ent_coef / B p_k (log p_k + H),   0 for k >= n_choices;
// no ratio, no clip; old_lp is not read (null is legal). The four sums are -A log_prob, log_prob, a spare
// and H.
template <int OBS, int ACT, int TW, bool VCLIP = false, bool NORM = true, int LOSS = 0>
__device__ __forceinline__ void ppo_grad_tower(
    float* __restrict__ lds, const float* __restrict__ obs, const float* __restrict__ act,
    const float* __restrict__ old_lp, const float* __restrict__ adv, const float* __restrict__ ret,
    const int64_t* __restrict__ idx, int64_t bs, float clip, float vf_coef, const double* __restrict__ adv_part,
    const float* __restrict__ pack, float* __restrict__ part, const float* __restrict__ old_val = nullptr,
    float clip_vf = 0.0f, int n_choices = 0, float ent_coef = 0.0f)
{
    using L = pol::Layout<OBS, ACT, 0>;
    using K = ppo::Pack<OBS, ACT>;
    using PT = ppo::Part<OBS, ACT>;
    using LD = ppo::Lds<OBS, ACT>;
    constexpr int KP1 = L::KP1;
    constexpr int TS = ppo::kTS;
    constexpr int tw = TW;
    constexpr bool CAT = LOSS == 2 || LOSS == 3 || LOSS == 5;  // the softmax head
    constexpr bool CLONE = LOSS == 1 || LOSS == 3;             // d loss / d log_prob = -1 / B: no ratio
    constexpr bool A2C = LOSS == 4 || LOSS == 5;               // d loss / d log_prob = -A / B: no ratio
    const int lane = threadIdx.x & (kWave - 1), half = lane >> 5, j = lane & 31;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    float* sp = lds;
    float* T0 = lds + K::SIZE + wv * LD::kPerWave;  // [64 unit][kTS]
    float* T1 = T0 + 64 * TS;                       // [64 unit][kTS]
    float* XT = T1 + 64 * TS;                       // [32 col][kTS]: x^T, row OBS = 1, rows past it 0
    float* DM = XT + 32 * TS;                       // [32 sample][4]: the heads' output gradients
    // diagnostic builds only (rocket_stamps.h, tools/ppo_stamps.py): per-wave cycles of 12 phases
    RR_ACC_BEGIN(12);
    const int64_t ntiles = (bs + ppo::kTile - 1) / ppo::kTile;
    const int64_t stride = (int64_t)gridDim.x * ppo::kWaves;
    // Software pipeline over the wave's tiles (one wave per SIMD: nothing else hides a gather's
    // latency): the sample indices are loaded two tiles ahead, the gathered rows one tile ahead.
    // Unmasked loads throughout (a load under a branch, or whose value is selected against a
    // constant, is waited for right there): a padding sample (tile position >= bs) gathers the
    // minibatch's last sample and is masked where its row is used, a tile later. Its action /
    // log-prob / advantage / return reach no sum (its loss derivatives are zeroed by `valid`);
    // its x is zeroed at use.
    auto sample_of = [&](int64_t t) -> int64_t {
        const int64_t si = t * ppo::kTile + j;
        return idx[si < bs ? si : bs - 1];
    };
    auto gather = [&](int64_t r, ppo::TileIn<OBS, ACT>& in) {
#pragma unroll
        for (int k = 0; k < KP1; ++k) {
            const int col = 2 * k + half;
            in.x[k] = col < OBS ? obs[r * OBS + col] : 0.0f;
        }
        if (tw == 0) {
            if constexpr (CAT) {
                in.a[0] = act[r];  // the chosen index
            } else {
#pragma unroll
                for (int a = 0; a < ACT; ++a) in.a[a] = act[r * ACT + a];
            }
            if constexpr (A2C) {
                in.av = adv[r];
            } else if constexpr (!CLONE) {
                in.olp = old_lp[r];
                in.av = adv[r];
            }
        } else {
            in.av = ret[r];
            if constexpr (VCLIP) in.olp = old_val[r];  // with the tile's other rows: unmasked, one tile ahead
        }
    };
    // Issue order: the first tile's indices, the staging loads, then the first tile's rows (which
    // wait only for the indices), so the index -> row chain runs under the staging's latency.
    int64_t tile = (int64_t)blockIdx.x * ppo::kWaves + wv;
    ppo::TileIn<OBS, ACT> nxt;
    int64_t s_cur = sample_of(tile);
    int64_t s_nxt = sample_of(tile + stride);
    {  // stage this tower's packed image (ppo_prep_kernel): all loads first, then the LDS stores
        constexpr int N4 = K::SIZE / 4, IT = (N4 + ppo::kThreads - 1) / ppo::kThreads;
        const float4* g4 = reinterpret_cast<const float4*>(pack + tw * K::SIZE);
        float4 v[IT];
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int k = threadIdx.x + i * ppo::kThreads;
            v[i] = g4[k < N4 ? k : N4 - 1];
        }
        gather(s_cur, nxt);
        // no branches: a load under one is waited for at its end (lanes past N4 rewrite the last
        // element with its own value)
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int k = threadIdx.x + i * ppo::kThreads;
            reinterpret_cast<float4*>(sp)[k < N4 ? k : N4 - 1] = v[i];
        }
    }
    for (int k = lane; k < (32 - OBS) * TS; k += kWave) XT[OBS * TS + k] = k < TS ? 1.0f : 0.0f;
    // minibatch advantage statistics (pi): mean, unbiased std
    // (the mean as a float pair: rounded to one float, a mean of 50 over a std of 0.5 moves every A by ~3e-6)
    float a_mean = 0.0f, a_mean_lo = 0.0f, a_den = 1.0f;
    if (tw == 0 && NORM) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int j = lane; j < ppo::kAdvPart; j += kWave) {
            s += adv_part[2 * j];
            q += adv_part[2 * j + 1];
        }
        s = ppo::wave_sum(s);
        q = ppo::wave_sum(q);
        const double n = (double)bs, mean = s / n;
        const double var = (q - s * mean) / (n - 1.0);
        a_mean = (float)mean;
        a_mean_lo = (float)(mean - (double)a_mean);
        a_den = sqrtf((float)(var > 0.0 ? var : 0.0)) + 1e-8f;
    }
    __syncthreads();
    RR_ST(0);

    const float inv_b = 1.0f / (float)bs;
    const float lo = 1.0f - clip, hi = 1.0f + clip;
    f32x16 accW2[4], accW1[2];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) accW2[b][r] = 0.0f;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) accW1[b][r] = 0.0f;
    float hw_acc[ACT], hb_acc[ACT], ls_acc[ACT], b2_acc = 0.0f;
    float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f;
    [[maybe_unused]] float st3 = 0.0f;  // LOSS 2 / 3 / 5: the entropy sum
#pragma unroll
    for (int a = 0; a < ACT; ++a) hw_acc[a] = hb_acc[a] = ls_acc[a] = 0.0f;
    float ls[ACT], var[ACT];
#pragma unroll
    for (int a = 0; a < ACT; ++a) {
        ls[a] = sp[K::LS + a];
        const float sd = expf(ls[a]);
        var[a] = 2.0f * sd * sd;  // torch: (2 * std * std)
    }

    for (; tile < ntiles; tile += stride) {
        const ppo::TileIn<OBS, ACT> in = nxt;
        const bool valid = tile * ppo::kTile + j < bs;
        s_cur = s_nxt;
        gather(s_cur, nxt);  // past the last tile too: no branch (see sample_of)
        s_nxt = sample_of(tile + 2 * stride);
        // layer-1 B operand and x^T into LDS
        float x[1][KP1];
#pragma unroll
        for (int k = 0; k < KP1; ++k) {
            const int col = 2 * k + half;
            x[0][k] = valid ? in.x[k] : 0.0f;
            if (col < OBS) XT[col * TS + j] = x[0][k];
        }
        RR_ST(1);
        f32x16 h1[2][1], h2[2][1];
        pol::tower_l1<OBS, ACT, 0, 1>(sp, x, lane, h1);
        pol::tower_act1<0, 1>(h1);
        pol::tower_l2<OBS, ACT, 0, 1>(sp, h1, lane, h2);
        pol::tower_act2<0, 1>(h2);
        RR_ST(2);
        // heads and the per-sample loss derivatives (both lane halves hold sample j)
        float dh[ACT];
        if (tw == 0) {
            float A;
            if constexpr (CLONE) A = 0.0f;  // no advantages
            else if constexpr (NORM) A = valid ? ((in.av - a_mean) - a_mean_lo) / a_den : 0.0f;
            else A = valid ? in.av : 0.0f;
            float lp = 0.0f, d[ACT];
            [[maybe_unused]] float pr[ACT], lpk[ACT], H = 0.0f;
            if constexpr (CAT) {
                // softmax over the first n_choices logits: log p_k from the log of the sum, so that a
                // p_k that underflows to 0 leaves log p_k finite
                float z[ACT];
#pragma unroll
                for (int a = 0; a < ACT; ++a) z[a] = pol::head_dot<1>(sp + K::HW + a * 64, h2, 0, half) + sp[K::HB + a];
                float zm = z[0];
#pragma unroll
                for (int a = 1; a < ACT; ++a) zm = a < n_choices ? fmaxf(zm, z[a]) : zm;
                float sum = 0.0f;
#pragma unroll
                for (int a = 0; a < ACT; ++a) {
                    pr[a] = a < n_choices ? expf(z[a] - zm) : 0.0f;
                    sum += pr[a];
                }
                const float lse = logf(sum);
#pragma unroll
                for (int a = 0; a < ACT; ++a) {
                    lpk[a] = (z[a] - zm) - lse;
                    pr[a] = pr[a] / sum;
                    if (a < n_choices) {
                        if (in.a[0] == (float)a) lp = lpk[a];
                        if (pr[a] > 0.0f) H -= pr[a] * lpk[a];
                    }
                }
            } else {
#pragma unroll
                for (int a = 0; a < ACT; ++a) {
                    const float mean = pol::head_dot<1>(sp + K::HW + a * 64, h2, 0, half) + sp[K::HB + a];
                    d[a] = in.a[a] - mean;
                    lp += -(d[a] * d[a]) / var[a] - ls[a] - 0.918938533204672742f;
                }
            }
            // d loss / d lp; PPO's ratio terms are read again by its sums below
            float dlp, lr, r, u, c;
            if constexpr (CLONE) {
                dlp = valid ? -inv_b : 0.0f;
            } else if constexpr (A2C) {
                dlp = valid ? -inv_b * A : 0.0f;
            } else {
                lr = lp - in.olp;
                r = expf(lr);
                const float cr = fminf(fmaxf(r, lo), hi);
                u = A * r, c = A * cr;
                const float gu = u < c ? 1.0f : (u == c ? 0.5f : 0.0f);
                const float gc = c < u ? 1.0f : (u == c ? 0.5f : 0.0f);
                const float mask = (r >= lo && r <= hi) ? 1.0f : 0.0f;
                dlp = valid ? -inv_b * (A * gu + A * gc * mask) * r : 0.0f;
            }
            if constexpr (CAT) {
                // d lp / d z_k = (k == a) - p_k; d(-H) / d z_k = p_k (log p_k + H)
                const float ec = valid ? ent_coef * inv_b : 0.0f;
#pragma unroll
                for (int a = 0; a < ACT; ++a) {
                    const float hit = in.a[0] == (float)a ? 1.0f : 0.0f;
                    dh[a] = a < n_choices ? dlp * (hit - pr[a]) + ec * (pr[a] * (lpk[a] + H)) : 0.0f;
                    if (half == 0) hb_acc[a] += dh[a];
                }
            } else {
#pragma unroll
                for (int a = 0; a < ACT; ++a) {
                    // d lp / d mean = 2 d / (2 std^2); d lp / d log_std = d^2 / std^2 - 1
                    dh[a] = dlp * (2.0f * d[a] / var[a]);
                    if (half == 0) {
                        hb_acc[a] += dh[a];
                        ls_acc[a] += dlp * (2.0f * d[a] * d[a] / var[a] - 1.0f);
                    }
                }
            }
            if (half == 0 && valid) {
                if constexpr (CLONE) {
                    st0 -= lp;
                    st1 += expf(lp);
                    if constexpr (LOSS == 3) st3 += H;
                } else if constexpr (A2C) {
                    st0 -= A * lp;
                    st1 += lp;
                    if constexpr (LOSS == 5) st3 += H;
                } else {
                    st0 -= fminf(u, c);
                    st1 += fabsf(r - 1.0f) > clip ? 1.0f : 0.0f;
                    st2 += (r - 1.0f) - lr;
                    if constexpr (LOSS == 2) st3 += H;
                }
            }
        } else {
            const float v = pol::head_dot<1>(sp + K::HW, h2, 0, half) + sp[K::HB];
            const float R = in.av;
            if constexpr (VCLIP) {
                const float dv = v - in.olp;
                const float vc = in.olp + fminf(fmaxf(dv, -clip_vf), clip_vf);
                const bool pass = dv >= -clip_vf && dv <= clip_vf;
                dh[0] = valid && pass ? vf_coef * 2.0f * (vc - R) * inv_b : 0.0f;
                if (half == 0) {
                    hb_acc[0] += dh[0];
                    if (valid) st0 += (R - vc) * (R - vc);
                }
            } else {
                dh[0] = valid ? vf_coef * 2.0f * (v - R) * inv_b : 0.0f;
                if (half == 0) {
                    hb_acc[0] += dh[0];
                    if (valid) st0 += (R - v) * (R - v);
                }
            }
        }
        RR_ST(3);
        constexpr int NH = ACT;  // vf uses row 0
        const int nh = tw ? 1 : NH;
        // h2 -> T0 [unit][sample], dhead -> DM [sample][a]
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) T0[(32 * m + ppo::drow(reg, half)) * TS + j] = h2[m][0][reg];
        if (half == 0) {
#pragma unroll
            for (int a = 0; a < NH; ++a) DM[j * 4 + a] = a < nh ? dh[a] : 0.0f;
        }
        // dpre2 = (W_head^T dhead) (1 - h2^2), D layout: one head's row at a time, read as load_head's
        // 8-B pairs (per element the sum over a in the same order as a scalar loop)
        f32x16 dp2[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) dp2[m][reg] = 0.0f;
#pragma unroll
        for (int a = 0; a < NH; ++a) {
            if (a < nh) {
                const pol::HeadW W = pol::load_head(sp + K::HW + a * 64, half);
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg)
                        dp2[m][reg] = fmaf(dh[a], W.w[m][reg / 2][reg & 1], dp2[m][reg]);
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float y = h2[m][0][reg];
                dp2[m][reg] = dp2[m][reg] * (1.0f - y * y);
            }
        RR_ST(4);
        ppo::wave_sync();
        // head gradients: lane = hidden unit u, sum over the tile's samples
        {
            const float4* row = reinterpret_cast<const float4*>(T0 + lane * TS);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 hv = row[q];
                const float hs[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float4 dm = reinterpret_cast<const float4*>(DM)[4 * q + e];
                    const float dms[4] = {dm.x, dm.y, dm.z, dm.w};
#pragma unroll
                    for (int a = 0; a < NH; ++a) hw_acc[a] = fmaf(dms[a], hs[e], hw_acc[a]);
                }
            }
        }
        RR_ST(5);
        ppo::wave_sync();
        // dpre2 -> T0, h1 -> T1
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                T0[(32 * m + ppo::drow(reg, half)) * TS + j] = dp2[m][reg];
                T1[(32 * m + ppo::drow(reg, half)) * TS + j] = h1[m][0][reg];
            }
        RR_ST(6);
        // dh1 = W2^T dpre2 (A: L2T fragments; B: dpre2 tile t register 4g + r = k step)
        f32x16 dh1[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) dh1[m][r] = 0.0f;
        {
            const float4* P4 = reinterpret_cast<const float4*>(sp + K::L2T);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 a4 = P4[((m * 2 + t) * 4 + g) * 64 + lane];
                        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            dh1[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], dp2[t][4 * g + r], dh1[m], 0, 0, 0);
                    }
        }
        RR_ST(7);
        ppo::wave_sync();
        // db2 (lane = unit) and dW2 += dpre2 h1^T (k = sample 16 half + step)
        {
            const float4* row = reinterpret_cast<const float4*>(T0 + lane * TS);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 v = row[q];
                b2_acc += (v.x + v.y) + (v.z + v.w);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 av[2], bv[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                av[m] = reinterpret_cast<const float4*>(T0 + (32 * m + j) * TS + 16 * half)[q];
                bv[m] = reinterpret_cast<const float4*>(T1 + (32 * m + j) * TS + 16 * half)[q];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                    for (int t1 = 0; t1 < 2; ++t1)
                        accW2[m2 * 2 + t1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m2][e], bv[t1][e],
                                                                                  accW2[m2 * 2 + t1], 0, 0, 0);
        }
        RR_ST(8);
        // dpre1 = dh1 (1 - h1^2) -> T0 (its dpre2 reads are done)
        ppo::wave_sync();
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const float y = h1[m][0][reg];
                T0[(32 * m + ppo::drow(reg, half)) * TS + j] = dh1[m][reg] * (1.0f - y * y);
            }
        RR_ST(9);
        ppo::wave_sync();
        // [dW1 | db1] += dpre1 [x, 1]^T
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 av[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) av[m] = reinterpret_cast<const float4*>(T0 + (32 * m + j) * TS + 16 * half)[q];
            const float4 bv = reinterpret_cast<const float4*>(XT + j * TS + 16 * half)[q];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int m = 0; m < 2; ++m) accW1[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][e], bv[e], accW1[m], 0, 0, 0);
        }
        RR_ST(10);
        ppo::wave_sync();  // the next tile overwrites T0 / T1 / XT / DM
    }

    // per-lane sums across the wave
#pragma unroll
    for (int a = 0; a < ACT; ++a) {
        hb_acc[a] = ppo::wave_sum(hb_acc[a]);
        ls_acc[a] = ppo::wave_sum(ls_acc[a]);
    }
    st0 = ppo::wave_sum(st0);
    st1 = ppo::wave_sum(st1);
    st2 = ppo::wave_sum(st2);
    if constexpr (CAT) st3 = ppo::wave_sum(st3);
    __syncthreads();  // every wave is done with its tiles: LDS becomes the reduction buffer
    float* red = lds + wv * PT::SIZE;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[PT::W2 + (b * 16 + r) * 64 + lane] = accW2[b][r];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[PT::W1 + (b * 16 + r) * 64 + lane] = accW1[b][r];
    red[PT::B2 + lane] = b2_acc;
#pragma unroll
    for (int a = 0; a < ACT; ++a) red[PT::HW + a * 64 + lane] = hw_acc[a];
    if (lane < 4) {
        float hb = 0.0f, l = 0.0f;
#pragma unroll
        for (int a = 0; a < ACT; ++a)
            if (lane == a) {
                hb = hb_acc[a];
                l = ls_acc[a];
            }
        red[PT::HB + lane] = hb;
        red[PT::LS + lane] = l;
        red[PT::ST + lane] = lane == 0 ? st0 : lane == 1 ? st1 : lane == 2 ? st2 : (CAT ? st3 : 0.0f);
    }
    __syncthreads();
    // the four waves' vectors summed as 16-B rows (PT::SIZE % 4 == 0: every row 16-B aligned)
    constexpr int N4 = PT::SIZE / 4;
    const float4* l4 = reinterpret_cast<const float4*>(lds);
    float4* o4 = reinterpret_cast<float4*>(part + ((int64_t)tw * gridDim.x + blockIdx.x) * PT::SIZE);
    for (int k = threadIdx.x; k < N4; k += ppo::kThreads) {
        const float4 a = l4[k], b = l4[N4 + k], c = l4[2 * N4 + k], d = l4[3 * N4 + k];
        o4[k] = make_float4((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y), (a.z + b.z) + (c.z + d.z),
                            (a.w + b.w) + (c.w + d.w));
    }
    RR_ST(11);
    // (diagnostic builds) past the partial vectors: 16 floats per wave, in a workspace the caller enlarged
    RR_ACC_WRITE(part + 2 * (int64_t)gridDim.x * PT::SIZE,
                 (((int64_t)tw * gridDim.x + blockIdx.x) * ppo::kWaves + wv) * 16, (uint32_t)lane, true);
}

template <int OBS, int ACT>
__global__ __launch_bounds__(ppo::kThreads) void ppo_grad_kernel(
    const float* __restrict__ obs, const float* __restrict__ act, const float* __restrict__ old_lp,
    const float* __restrict__ adv, const float* __restrict__ ret, const int64_t* __restrict__ idx, int64_t bs,
    float clip, float vf_coef, const double* __restrict__ adv_part, const float* __restrict__ pack,
    float* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
    if (blockIdx.y == 0)
        ppo_grad_tower<OBS, ACT, 0>(lds, obs, act, old_lp, adv, ret, idx, bs, clip, vf_coef, adv_part, pack, part);
    else
        ppo_grad_tower<OBS, ACT, 1>(lds, obs, act, old_lp, adv, ret, idx, bs, clip, vf_coef, adv_part, pack, part);
}

struct PolGrad {
    float* p[13];  // same order as PolSrc
};

// Sum the workgroups' partial vectors (fixed order) and scatter into the PyTorch gradient
// tensors. Block: kFinElems consecutive elements x kFinGroups groups of partial rows (each thread
// sums nwg / kFinGroups rows, four loads in flight); element e of tower tw = blockIdx.y.
// normw (rr_ppo_update): also the block's sum of the squared gradient elements it stores, at
// normw[tw * gridDim.x + blockIdx.x], and the optimizer's next step count (*step0 + 1) after the
// 2 * gridDim.x sums — the clip's norm without a pass of its own over the gradients.
constexpr int kFinElems = 32, kFinGroups = 8;

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void ppo_finish_kernel(const float* __restrict__ part, int nwg, int64_t bs,
                                                         float ent_coef, PolSrc src, PolGrad dst,
                                                         float* __restrict__ stats, float* __restrict__ normw,
                                                         const float* __restrict__ step0)
{
    constexpr bool CTL = false;
    const ppo::CtlArgs ca = {};
#include "rocket_ppo_finish_body.inc"
}

// clip_grad_norm_ + Adam step over a list of tensors (rr_clip_adam): the optimizer half of a
// PPO minibatch (~10.6 k parameters), after rr_ppo_grad. Follows PyTorch's
// torch.nn.utils.clip_grad_norm_ (coef = max_norm / (||g|| + 1e-6), clamped to 1, grads scaled in
// place) and torch.optim.Adam(capturable=True)'s multi-tensor step (weight_decay 0, no amsgrad):
//   step += 1; m = lerp(m, g, 1 - beta1); v = v beta2 + (1 - beta2) g g;
//   s = -1 / ((1 - beta1^step) / lr); p += m / (sqrt(v) / (sqrt(1 - beta2^step) s) + 1 / (s / eps))
// with the optimizer's own state tensors (exp_avg, exp_avg_sq, per-tensor step) updated in place.
// Two launches over the concatenated elements, kAdamThreads per block: adam_norm_kernel writes
// each block's sum of squared gradients (and block 0 the new step count), adam_step_kernel sums
// those, scales, steps and (block 0) stores the step count into every tensor's step. No block
// writes what another block of the same launch reads.
struct AdamList {
    float* param[16];
    float* grad[16];
    float* exp_avg[16];
    float* exp_avg_sq[16];
    float* step[16];
    int64_t start[17];   // prefix sums of the tensors' sizes
    int64_t wstart[17];  // the same with every size rounded up to a wave (adam_chain_kernel's element order)
    int n;
};

constexpr int kAdamThreads = 1024;

__device__ __forceinline__ int adam_tensor_of(const AdamList& A, int64_t e)
{
    int t = 0;
    while (t + 1 < A.n && e >= A.start[t + 1]) ++t;
    return t;
}

template <int NT>
__device__ __forceinline__ float block_sum(float v, float* red)
{
    v = ppo::wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int k = 0; k < NT / kWave; ++k) tot += red[k];
    return tot;
}

// rr_ppo_update's optimizer launch: the clip + Adam step of adam_step_kernel over the 13 policy
// tensors in rr_ppo_grad's order, with the squared-gradient sums and the step count from
// ppo_finish_kernel (normw[0 .. n_norm), normw[n_norm]); each updated parameter also goes to its
// slots of the packed tower images (ppo::pack_value's inverse), so the next minibatch's gradient
// launch needs no packing pass. Blocks from nbp on: the next minibatch's advantage partial sums,
// ppo_prep_kernel's blocking exactly (four of its 256-thread blocks per block: bitwise its sums).
struct AdvNext {
    const float* adv;
    const int64_t* idx;  // null: no next minibatch
    int64_t bs;
    double* part;
};

// One learner call's launches as the C-ABI entry points (main TU: arguments validated, workspace
// carved) hand them to the collect TU, where the learner's kernels are compiled with the MFMA
// accumulators in VGPRs (rocket_collect.hip)
struct PpoLaunch {
    PolSrc ps;
    PolGrad pg;
    AdamList a;  // rr_ppo_update / rr_clip_adam
    const float *obs, *actions, *old_log_prob, *advantages, *returns, *lr;
    const int64_t *idx, *next_idx;
    int64_t batch, next_batch;
    float clip, ent, vf, max_norm, beta1, beta2, w1, w2, eps;
    float* stats;
    double* adv_part;
    float *part, *pack, *normw, *work;
    int obs_dim, nwg, nbp, op;  // op: 0 rr_ppo_grad, 1 rr_ppo_update, 2 rr_clip_adam
    uint32_t flags;
};
static_assert(std::is_trivially_copyable_v<PpoLaunch>, "PpoLaunch crosses TUs by memcpy (rrc_launch_learner)");

// rr_ppo_update_opts's launches (ppo_opts/rocket_ppo_opts.hip, rrc_launch_learner_opts): an
// rr_ppo_update launch record (op 1) and the options
struct PpoOptsLaunch {
    PpoLaunch base;
    const float* old_values;  // the value clip's rollout values (clip_vf > 0)
    float clip_vf;            // <= 0: off
    int normalize;            // normalize_advantage
    ppo::CtlArgs ctl;
};
static_assert(std::is_trivially_copyable_v<PpoOptsLaunch>, "PpoOptsLaunch crosses TUs by memcpy");

// rr_bc_update's and rr_bc_update_discrete's launches (rocket_bc.inc; rrc_launch_bc, rrc_launch_bc_discrete):
// pack the pi image, the pi tower's gradient on nwg workgroups, the finish over both halves and the
// statistics, Adam with the repack. For the Categorical policy the record is over 12 tensors, pg.p[12] is
// four spare floats of the workspace and `sink` 260 more (where the finish puts the zero sums of heads >=
// n_choices); for the Gaussian n_choices is 0 and sink null.
struct BcLaunch {
    PolSrc ps;
    PolGrad pg;
    AdamList a;
    const float *obs, *actions, *lr;
    const int64_t* idx;
    int64_t batch;
    float ent, l2, beta1, beta2, w1, w2, eps;
    float* stats;  // 8 floats (RR_BC_STAT_*) or null
    float *part, *pack, *normw;
    int obs_dim, nwg, nbp;
    uint32_t flags;
    int n_choices;
    float* sink;
};
static_assert(std::is_trivially_copyable_v<BcLaunch>, "BcLaunch crosses TUs by memcpy");

// rr_a2c_update's launches (a2c/rocket_a2c.hip, rrc_launch_a2c): the advantage sums and the packing, the
// gradient of both towers on nwg workgroups each, the finish, the optimizer. a.exp_avg_sq holds the
// optimizer's second-moment tensors (RMSprop's square_avg, Adam's exp_avg_sq); a.exp_avg is Adam's only.
struct A2cLaunch {
    PolSrc ps;
    PolGrad pg;
    AdamList a;
    const float *obs, *actions, *advantages, *returns, *lr;
    const int64_t* idx;
    int64_t batch;
    float ent, vf, max_norm, alpha, beta1, beta2, w1, w2, eps;
    float* stats;  // 8 floats or null
    double* adv_part;
    float *part, *pack, *normw;
    int obs_dim, nwg, nbp, normalize;
    int optimizer;  // RR_A2C_RMSPROP / RR_A2C_RMSPROP_TF / RR_A2C_ADAM
};
static_assert(std::is_trivially_copyable_v<A2cLaunch>, "A2cLaunch crosses TUs by memcpy");

// rr_a2c_update_discrete's launches (a2c_discrete/rocket_a2c_discrete.hip, rrc_launch_a2c_discrete): an
// rr_a2c_update launch record over 12 tensors whose pg.p[12] is four spare floats of the workspace, the
// number of choices, and `sink`, 260 more floats (where the finish puts the zero sums of heads >= n_choices)
struct A2cDiscreteLaunch {
    A2cLaunch base;
    int n_choices;
    float* sink;
};
static_assert(std::is_trivially_copyable_v<A2cDiscreteLaunch>, "A2cDiscreteLaunch crosses TUs by memcpy");

// What the main TU hands to discrete/rocket_discrete.hip (rrc_launch_discrete), by `op`:
//   kDiscAct        rr_policy_act_discrete: one discrete_act_kernel launch
//   kDiscUpdate     rr_ppo_update_discrete: `u`, an rr_ppo_update record (op 1) over 12 tensors whose
//                   pg.p[12] is four spare floats of the workspace, and `sink`, 260 more (where the
//                   finish puts the zero sums of heads >= n_choices)
//   kDiscPack       rr_policy_pack_discrete: the rollout image of pol::Layout<7, 4, 0>
//   kDiscBootstrap  rr_policy_bootstrap at (7, 4): policy_bootstrap_kernel<7, 4, 0>
enum { kDiscAct = 0, kDiscUpdate, kDiscPack, kDiscBootstrap };
struct DiscreteLaunch {
    int op, n_choices;
    float table[4][2];  // act: the choices' [gimbal, thrust] rows
    PpoLaunch u;        // update; pack: u.ps, u.pack
    float* sink;        // update
    // act / bootstrap
    const float *params, *obs, *prev_term_obs, *prev_reward;
    const uint8_t *prev_trunc, *done;
    const uint64_t* iter;
    float *act_env, *act, *value, *logp, *obs_copy, *reward_out, *start_out, *value_out;
    int64_t n, id_off;
    uint32_t seed_lo, seed_hi, t;
    float gamma;
};
static_assert(std::is_trivially_copyable_v<DiscreteLaunch>, "DiscreteLaunch crosses TUs by memcpy");

// rr_ppo_update_discrete_opts's launches (discrete_opts/rocket_ppo_discrete_opts.hip,
// rrc_launch_discrete_opts): an rr_ppo_update_discrete launch record (kDiscUpdate) and the options,
// as PpoOptsLaunch extends PpoLaunch; base.u.stats is never null (the caller's, or workspace floats)
struct DiscreteOptsLaunch {
    DiscreteLaunch base;
    const float* old_values;  // the value clip's rollout values (clip_vf > 0)
    float clip_vf;            // <= 0: off
    int normalize;            // normalize_advantage
    ppo::CtlArgs ctl;
};
static_assert(std::is_trivially_copyable_v<DiscreteOptsLaunch>, "DiscreteOptsLaunch crosses TUs by memcpy");

// Element k of policy tensor t (rr_ppo_grad order) into the packed images (two towers of Pack::SIZE).
template <int OBS, int ACT>
__device__ __forceinline__ void pack_scatter(float* __restrict__ pack, int t, int k, float v)
{
    using L = pol::Layout<OBS, ACT, 0>;
    using K = ppo::Pack<OBS, ACT>;
    constexpr int KP1 = L::KP1;
    // inverse of drow: unit r of a 32-unit half -> (reg, half) of the D layout
    auto dslot = [](int r) { return (r & 3) + 4 * (r >> 3) + 16 * ((r >> 2) & 1); };  // reg + 16 half
    const int tw = t < 8 ? t / 4 : (t == 10 || t == 11 ? 1 : 0);
    float* P = pack + tw * K::SIZE;
    switch (t < 8 ? t % 4 : t) {
    case 0: {  // W1 [64][OBS]
        const int u = k / OBS, c = k % OBS;
        P[((u >> 5) * KP1 + (c >> 1)) * 64 + (c & 1) * 32 + (u & 31)] = v;
        break;
    }
    case 1:  // b1
        P[L::B1 + 32 * (k >> 5) + dslot(k & 31)] = v;
        break;
    case 2: {  // W2 [64 out][64 in]: the forward fragments and the transposed copy
        const int a = k / 64, b = k % 64;
        const int rb = b & 31, ra = a & 31;
        P[L::L2A + (rb & 3) + 4 * (((rb >> 2) & 1) * 32 + ra) + 256 * (rb >> 3) + 1024 * (b >> 5) + 2048 * (a >> 5)] = v;
        P[K::L2T + (ra & 3) + 4 * (((ra >> 2) & 1) * 32 + rb) + 256 * (ra >> 3) + 1024 * (a >> 5) + 2048 * (b >> 5)] = v;
        break;
    }
    case 3:  // b2
        P[L::B2 + 32 * (k >> 5) + dslot(k & 31)] = v;
        break;
    case 8:
    case 10: {  // head rows [ACT or 1][64]
        const int a = k / 64, u = k % 64;
        P[K::HW + 64 * a + 32 * (u >> 5) + dslot(u & 31)] = v;
        break;
    }
    case 9:
    case 11:  // head biases
        P[K::HB + k] = v;
        break;
    default:  // 12: log_std (pi)
        P[K::LS + k] = v;
        break;
    }
}

template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void adam_chain_kernel(AdamList A, const float* __restrict__ normw, int n_norm,
                                                                  float max_norm, const float* __restrict__ lr_p,
                                                                  float beta1, float beta2, float w1, float w2, float eps,
                                                                  float* __restrict__ pack, AdvNext nx, int nbp)
{
#include "rocket_ppo_adam_body.inc"
}

}  // namespace
