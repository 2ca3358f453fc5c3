// rocket_discrete.hip — the ninth translation unit of librocket_hip.so: the Categorical policy of the
// reference's DiscreteActions3DOF (wrappers.py:24-35: Discrete(K) over a table of [gimbal, thrust]
// rows) on the device. With that wrapper SB3 builds an MlpPolicy whose action head is K logits and
// which has no log_std (CategoricalDistribution). The towers are the Gaussian policy's; pol::Layout,
// ppo::Pack and ppo::Part are instantiated at <7, 4> and the choices K = 2 .. 4 are a runtime count:
// heads k >= K are packed as zeros, stay out of the softmax and receive no gradient.
//   act        discrete_act_kernel: policy_act_kernel's frame (staging, the bootstrap of step t - 1, the
//              episode-start flags, value tower, pi tower, one lane per env) with a softmax head and
//              one uniform draw per env from policy_act_kernel's key (rr_policy_act_discrete);
//   learner    rr_ppo_update_discrete, rr_ppo_update's four launches (three chained):
//     prep       ppo_prep_body's advantage sums; the packing blocks zero the heads >= K;
//     gradient   ppo_grad_tower<7, 4, 0, false, true, LOSS 2> (the softmax head, the entropy's
//                gradient per sample) and the value tower as it is;
//     finish     rocket_ppo_finish_body.inc as text over 12 tensors: log_std's slot of the body is
//                four spare floats (its sums are zero, and nothing is subtracted: ent_coef is 0
//                there), elements of heads >= K go to a sink instead of past the [K][64] tensors,
//                and the entropy statistic is the mean of the fourth per-sample sum;
//     optimizer  rocket_ppo_adam_body.inc as text over 12 tensors, repacking the <7, 4> images;
//   pack       discrete_policy_pack_kernel: the rollout image (folded tanh) from the 12 tensors;
//   bootstrap  policy_bootstrap_kernel<7, 4, 0> for rr_policy_bootstrap at (7, 4).
// Launched through rrc_launch_discrete with a DiscreteLaunch. Compiled with the collect translation
// unit's settings (build.py COLLECT_FLAGS): the gradient kernel's loop is the learner's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_ppo.inc"

namespace {

struct DiscTable {
    float v[4][2];
};

template <int OBS, int NL>
__global__ __launch_bounds__(pol::kThreads) void discrete_act_kernel(
    const float* __restrict__ params, int64_t n, int64_t id_off, const float* __restrict__ obs, uint32_t seed_lo,
    uint32_t seed_hi, const uint64_t* __restrict__ iter, uint32_t t, int n_choices, DiscTable tab,
    float* __restrict__ act_env, float* __restrict__ act, float* __restrict__ value, float* __restrict__ logp,
    float* __restrict__ obs_copy, const float* __restrict__ prev_term_obs, const uint8_t* __restrict__ prev_trunc,
    const float* __restrict__ prev_reward, float gamma, float* __restrict__ reward_out,
    const uint8_t* __restrict__ done_flags, float* __restrict__ start_out)
{
    using L = pol::Layout<OBS, NL, 0>;
    static_assert(pol::kNT == 1, "one env tile per wave");
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float so_all[pol::kWaves][pol::kEPW * OBS];
    __shared__ __attribute__((aligned(16))) float so2_all[pol::kWaves][pol::kEPW * OBS];
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int64_t env0 = ((int64_t)blockIdx.x * pol::kWaves + wv) * pol::kEPW;
    float* so = so_all[wv];
    const bool live = env0 < n;  // wave-uniform
    pol::stage_params<OBS, NL, 0>(params, sp);
    if (live) pol::stage_obs<OBS>(obs, obs_copy, so, env0, n);
    __syncthreads();
    if (!live) return;
    const int64_t e = env0 + pol::lane_env(lane);
    const bool ok = e < n && pol::lane_writes(lane);
    if (start_out && ok) start_out[e] = done_flags[e] ? 1.0f : 0.0f;
    if (reward_out)
        pol::bootstrap_wave<OBS, NL, 0>(sp, so2_all[wv], prev_term_obs, prev_trunc, prev_reward, gamma, reward_out, env0,
                                        n, lane);
    float x[1][L::KP1];
    pol::load_x<OBS, NL, 0>(so, lane, x);
    const int half = lane >> 5;
    f32x16 h2[2][1];
    // value tower
    pol::tower<OBS, NL, 0>(sp + L::VF, x, lane, h2);
    const float v = pol::head_dot(sp + L::HV, h2, 0, half) + sp[L::VB];
    // action tower: the logits
    pol::tower<OBS, NL, 0>(sp + L::PI, x, lane, h2);
    float z[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) z[k] = pol::head_dot(sp + L::HA + k * 64, h2, 0, half) + sp[L::HB + k];
    // softmax over the first n_choices logits; log p_k from the log of the sum (a p_k that underflows
    // to 0 leaves log p_k finite)
    float zm = z[0];
#pragma unroll
    for (int k = 1; k < NL; ++k) zm = k < n_choices ? fmaxf(zm, z[k]) : zm;
    float ex[NL], sum = 0.0f;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        ex[k] = k < n_choices ? expf(z[k] - zm) : 0.0f;
        sum += ex[k];
    }
    const float lse = logf(sum);
    // one uniform per env: policy_act_kernel's key
    const uint64_t it = *iter;
    uint32_t key = mix32((uint32_t)(id_off + e) ^ seed_lo);
    key = mix32(key ^ (uint32_t)it ^ seed_hi);
    key = mix32(key ^ (uint32_t)(it >> 32) ^ (t * 0x9E3779B9u));
    const float u = (float)(mix32(key) >> 8) * 0x1p-24f;  // [0, 1)
    // index = the number of k in 0 .. K - 2 whose running sum p_0 + .. + p_k is <= u and which have a
    // positive weight beyond them: a choice whose weight underflowed to 0 is never drawn
    const int index = categorical_index(ex, sum, u, n_choices);
    // the chosen logit and the table row by compares: no data-dependent address
    float za = z[0], a0 = tab.v[0][0], a1 = tab.v[0][1];
#pragma unroll
    for (int k = 1; k < NL; ++k)
        if (index == k) {
            za = z[k];
            a0 = tab.v[k][0];
            a1 = tab.v[k][1];
        }
    if (ok) {
        value[e] = v;
        logp[e] = (za - zm) - lse;
        act[e] = (float)index;
        act_env[2 * e] = a0;
        act_env[2 * e + 1] = a1;
    }
}

// The rollout image pol::Layout<OBS, 4, 0> (policy_pack_kernel's fp32 form: the folded tanh) from the
// 12 tensors of the Categorical policy, W_action [K][64] and b_action [K]: heads >= K are zeros.
template <int OBS>
__global__ __launch_bounds__(256) void discrete_policy_pack_kernel(PolSrc src, int n_choices, float* __restrict__ dst)
{
    static_assert(kPolFoldTanh, "the only form of the fp32 rollout pack");
    using L = pol::Layout<OBS, 4, 0>;
    constexpr int KP1 = L::KP1;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= L::SIZE) return;
    constexpr double kC = 2.88539008177792681;  // 2 log2 e
    auto rowsum = [](const float* W, int r, int cols) {
        double acc = 0.0;
        for (int q = 0; q < cols; ++q) acc += (double)W[r * cols + q];
        return acc;
    };
    float v = 0.0f;
    if (k < L::HA) {
        const int tw = k / L::TOWER, o = k % L::TOWER;
        const float* const* P = src.p + 4 * tw;  // W1 b1 W2 b2 of this tower
        if (o < L::B1) {
            const int lane = o % 64, s = (o / 64) % KP1, m = o / (64 * KP1);
            const int kk = 2 * s + (lane >> 5);
            v = kk < OBS ? (float)(kC * (double)P[0][(32 * m + (lane & 31)) * OBS + kk]) : 0.0f;
        } else if (o < L::L2A) {
            const int i = o - L::B1, reg = i % 16, half = (i / 16) % 2, m = i / 32;
            v = (float)(kC * (double)P[1][32 * m + ppo::drow(reg, half)]);
        } else if (o < L::B2) {
            const int i = o - L::L2A;
            const int r = i % 4, lane = (i / 4) % 64, g = (i / 256) % 4, t = (i / 1024) % 2, m = i / 2048;
            v = (float)(-2.0 * kC * (double)P[2][(32 * m + (lane & 31)) * 64 + 32 * t + ppo::drow(4 * g + r, lane >> 5)]);
        } else {
            const int i = o - L::B2, reg = i % 16, half = (i / 16) % 2, m = i / 32;
            const int rw = 32 * m + ppo::drow(reg, half);
            v = (float)(kC * ((double)P[3][rw] + rowsum(P[2], rw, 64)));
        }
    } else if (k < L::HV) {
        const int i = k - L::HA, reg = i % 16, half = (i / 16) % 2, m = (i / 32) % 2, a = i / 64;
        v = a < n_choices ? -2.0f * src.p[8][a * 64 + 32 * m + ppo::drow(reg, half)] : 0.0f;
    } else if (k < L::HB) {
        const int i = k - L::HV, reg = i % 16, half = (i / 16) % 2, m = i / 32;
        v = -2.0f * src.p[10][32 * m + ppo::drow(reg, half)];
    } else if (k < L::VB) {
        const int a = k - L::HB;
        v = a < n_choices ? (float)((double)src.p[9][a] + rowsum(src.p[8], a, 64)) : 0.0f;
    } else if (k == L::VB) {
        v = (float)((double)src.p[11][0] + rowsum(src.p[10], 0, 64));
    }
    dst[k] = v;
}

// (discrete_pack_value, element k of a tower's learner image with zeros for the heads >= n_choices, is in
// rocket_ppo.inc: bc_discrete/rocket_bc_discrete.hip packs with it too)
template <int OBS, int ACT>
__global__ __launch_bounds__(256) void discrete_prep_kernel(const float* __restrict__ adv,
                                                            const int64_t* __restrict__ idx, int64_t bs,
                                                            double* __restrict__ part, PolSrc src, int n_choices,
                                                            float* __restrict__ pack)
{
    using K = ppo::Pack<OBS, ACT>;
    if (blockIdx.x >= ppo::kAdvPart) {
        const int k = (blockIdx.x - ppo::kAdvPart) * 256 + threadIdx.x;
        if (k < 2 * K::SIZE) pack[k] = discrete_pack_value<OBS, ACT>(src, n_choices, k / K::SIZE, k % K::SIZE);
        return;
    }
    ppo_prep_body<OBS, ACT>(adv, idx, bs, part, src, pack);  // the advantage sums: these blocks pack nothing
}

template <int OBS, int ACT>
__global__ __launch_bounds__(ppo::kThreads) void discrete_grad_kernel(
    const float* __restrict__ obs, const float* __restrict__ act, const float* __restrict__ old_lp,
    const float* __restrict__ adv, const float* __restrict__ ret, const int64_t* __restrict__ idx, int64_t bs,
    float clip, float ent_coef, float vf_coef, int n_choices, const double* __restrict__ adv_part,
    const float* __restrict__ pack, float* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
    if (blockIdx.y == 0)
        ppo_grad_tower<OBS, ACT, 0, false, true, 2>(lds, obs, act, old_lp, adv, ret, idx, bs, clip, vf_coef, adv_part,
                                                    pack, part, nullptr, 0.0f, n_choices, ent_coef);
    else
        ppo_grad_tower<OBS, ACT, 1>(lds, obs, act, old_lp, adv, ret, idx, bs, clip, vf_coef, adv_part, pack, part);
}

// grid (nfin, 2). Both lists' p[12] is four spare floats; dst_sink is dst_in with the action head's
// weight and bias gradients replaced by a [4][64] + [4] sink.
template <int OBS, int ACT>
__global__ __launch_bounds__(256) void discrete_finish_kernel(const float* __restrict__ part, int nwg, int64_t bs,
                                                              int n_choices, PolSrc src, PolGrad dst_in,
                                                              PolGrad dst_sink, float* __restrict__ stats_out,
                                                              float* __restrict__ normw,
                                                              const float* __restrict__ step0)
{
    // An element of a head >= n_choices (a zero sum) must not land past the [n_choices][64] weight and
    // [n_choices] bias gradients: the thread that holds one writes it to the sink, at the offsets the
    // body computes (a choice between the two argument lists: a modified copy would live in scratch).
    using P = ppo::Part<OBS, ACT>;
    const int el = blockIdx.x * kFinElems + threadIdx.x % kFinElems;
    const bool spare = blockIdx.y == 0 && ((el >= P::HW + 64 * n_choices && el < P::HB) ||
                                           (el >= P::HB + n_choices && el < P::LS));
    const PolGrad& dst = spare ? dst_sink : dst_in;
    // The body's entropy lines are the Gaussian's (-ent_coef on log_std, the statistic from log_std):
    // off here. The entropy's gradient came with the head derivative.
    constexpr float ent_coef = 0.0f;
    float* const stats = nullptr;
    constexpr bool CTL = false;
    const ppo::CtlArgs ca = {};
#include "rocket_ppo_finish_body.inc"
    if (stats_out && e >= PT::ST && e < PT::SIZE) {
        const int k = e - PT::ST;
        const float inv_b = 1.0f / (float)bs;
        if (tw == 0) {
            if (k == 0) stats_out[0] = v * inv_b;  // policy_loss
            if (k == 1) stats_out[3] = v * inv_b;  // clip_fraction
            if (k == 2) stats_out[4] = v * inv_b;  // approx_kl
            if (k == 3) stats_out[2] = v * inv_b;  // entropy: the mean of H
        } else if (k == 0) {
            stats_out[1] = v * inv_b;  // value_loss
        }
    }
}

template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void discrete_adam_kernel(AdamList A, const float* __restrict__ normw,
                                                                     int n_norm, float max_norm,
                                                                     const float* __restrict__ lr_p, float beta1,
                                                                     float beta2, float w1, float w2, float eps,
                                                                     float* __restrict__ pack, AdvNext nx, int nbp)
{
#include "rocket_ppo_adam_body.inc"
}

}  // namespace

// The launches of rr_policy_act_discrete, rr_ppo_update_discrete, rr_policy_pack_discrete and of
// rr_policy_bootstrap at (7, 4) (declared in rocket_device.h); `launch` points to the DiscreteLaunch of
// the calling TU, which validated the arguments and carved the workspace.
extern "C" int rrc_launch_discrete(const void* launch, void* stream)
{
    const auto D = from_unit<DiscreteLaunch>(launch);
    hipStream_t s = (hipStream_t)stream;
    constexpr int O = 7, A = 4;
    const dim3 pgrid((unsigned)((D.n + pol::kEnvsPerBlock - 1) / pol::kEnvsPerBlock)), pblock(pol::kThreads);
    if (D.op == kDiscAct) {
        DiscTable tab;
        std::memcpy(tab.v, D.table, sizeof(tab.v));
        hipLaunchKernelGGL((discrete_act_kernel<O, A>), pgrid, pblock, 0, s, D.params, D.n, D.id_off, D.obs, D.seed_lo,
                           D.seed_hi, D.iter, D.t, D.n_choices, tab, D.act_env, D.act, D.value, D.logp, D.obs_copy,
                           D.prev_term_obs, D.prev_trunc, D.prev_reward, D.gamma, D.reward_out, D.done, D.start_out);
    } else if (D.op == kDiscBootstrap) {
        hipLaunchKernelGGL((policy_bootstrap_kernel<O, A, 0>), pgrid, pblock, 0, s, D.params, D.n, D.prev_term_obs,
                           D.prev_trunc, D.prev_reward, D.gamma, D.reward_out, D.obs, D.value_out);
    } else if (D.op == kDiscPack) {
        hipLaunchKernelGGL((discrete_policy_pack_kernel<O>), dim3((pol::Layout<O, A, 0>::SIZE + 255) / 256), dim3(256),
                           0, s, D.u.ps, D.n_choices, D.u.pack);
    } else {
        const PpoLaunch& L = D.u;
        using PT = ppo::Part<O, A>;
        using K = ppo::Pack<O, A>;
        constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
        if (!(L.flags & RR_PPO_CHAINED))
            hipLaunchKernelGGL((discrete_prep_kernel<O, A>), dim3(ppo::kAdvPart + (2 * K::SIZE + 255) / 256), dim3(256),
                               0, s, L.advantages, L.idx, L.batch, L.adv_part, L.ps, D.n_choices, L.pack);
        hipLaunchKernelGGL((discrete_grad_kernel<O, A>), dim3(L.nwg, 2), dim3(ppo::kThreads), 0, s, L.obs, L.actions,
                           L.old_log_prob, L.advantages, L.returns, L.idx, L.batch, L.clip, L.ent, L.vf, D.n_choices,
                           (const double*)L.adv_part, (const float*)L.pack, L.part);
        PolGrad pg_sink = L.pg;
        pg_sink.p[8] = D.sink;
        pg_sink.p[9] = D.sink + 64 * A;
        hipLaunchKernelGGL((discrete_finish_kernel<O, A>), dim3(nfin, 2), dim3(256), 0, s, (const float*)L.part, L.nwg,
                           L.batch, D.n_choices, L.ps, L.pg, pg_sink, L.stats, L.normw, (const float*)L.a.step[0]);
        const AdvNext nx = {L.advantages, L.next_idx, L.next_idx ? L.next_batch : 0, L.adv_part};
        hipLaunchKernelGGL((discrete_adam_kernel<O, A>), dim3(L.nbp + (L.next_idx ? ppo::kAdvPart / 4 : 0)),
                           dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw, 2 * nfin, L.max_norm, L.lr, L.beta1,
                           L.beta2, L.w1, L.w2, L.eps, L.pack, nx, L.nbp);
    }
    return (int)hipGetLastError();
}
