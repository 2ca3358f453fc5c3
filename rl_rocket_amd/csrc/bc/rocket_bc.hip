// rocket_bc.hip — the eighth translation unit of librocket_hip.so: behaviour cloning on the device
// (rr_bc_update), what imitation's bc.BC does per minibatch for SB3's MlpPolicy with a diagonal
// Gaussian:
//   logp_i  = sum_a (-(a_ia - mean_ia)^2 / (2 std_a^2) - log_std_a - 0.5 log 2 pi)
//   loss    = -mean_i logp_i - ent_weight entropy + l2_weight 0.5 sum_{all 13 tensors} w^2
//   Adam (capturable, no clip) over the 13 tensors.
// It is the learner's pipeline (rocket_ppo.inc) with another head derivative and no value half:
//   packing   the pi tower's LDS image (ppo::pack_value), skipped by a chained call;
//   gradient  ppo_grad_tower<OBS, ACT, 0, false, false, LOSS 1> on a grid of (nwg, 1): the pi tower's
//             forward, backward and weight gradients as they are, d loss / d logp = -1 / B;
//   finish    rocket_ppo_finish_body.inc as text: the fixed-order sum of the workgroups' partial
//             vectors scattered into the gradient tensors, -ent_weight per log_std element. The
//             value half (blockIdx.y 1) runs it over zero partial rows, so its tensors are written as
//             zeros. After it every element adds l2_weight w. A third row of blocks (blockIdx.y 2)
//             sums the statistics: the workgroups' -logp and exp(logp) sums and all w^2, each in a
//             fixed order;
//   optimizer rocket_ppo_adam_body.inc as text with max_norm 0 (its "no clip" branch) and no
//             next-minibatch blocks; it repacks both tower images for the chained call.
// Launched through rrc_launch_bc with a BcLaunch. Compiled with the collect translation unit's
// settings (build.py COLLECT_FLAGS), because the gradient kernel's loop is the learner's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_ppo.inc"

namespace {

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void bc_pack_kernel(PolSrc src, float* __restrict__ pack)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < ppo::Pack<OBS, ACT>::SIZE) pack[k] = ppo::pack_value<OBS, ACT>(src, 0, k);
}

template <int OBS, int ACT>
__global__ __launch_bounds__(ppo::kThreads) void bc_grad_kernel(const float* __restrict__ obs,
                                                                const float* __restrict__ act,
                                                                const int64_t* __restrict__ idx, int64_t bs,
                                                                const float* __restrict__ pack,
                                                                float* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
    ppo_grad_tower<OBS, ACT, 0, false, false, 1>(lds, obs, act, nullptr, nullptr, nullptr, idx, bs, 0.0f, 0.0f, nullptr,
                                                 pack, part);
}

// elements of policy tensor t (rr_ppo_grad's order)
template <int OBS, int ACT>
__device__ __forceinline__ constexpr int bc_numel(int t)
{
    return t == 0 || t == 4 ? 64 * OBS
           : t == 2 || t == 6 ? 64 * 64
           : t == 8 ? 64 * ACT
           : t == 9 || t == 12 ? ACT
           : t == 11 ? 1
                     : 64;
}

// The statistics block: one fixed-order sum each of the workgroups' -logp and exp(logp) partial sums
// (thread = workgroup) and of every parameter's square (thread k: elements k, k + 256, ... of each
// tensor in turn), in fp64; the wave sums are butterflies, the four waves are added in order.
template <int OBS, int ACT>
__device__ __forceinline__ void bc_stats_block(const float* __restrict__ part, int nwg, int64_t bs, float ent_w,
                                               float l2_w, const PolSrc& src, float* __restrict__ stats)
{
    using PT = ppo::Part<OBS, ACT>;
    __shared__ double sred[3][256 / kWave];
    static_assert(ppo::kMaxWG <= 256, "one workgroup's sums per thread");
    // Every load first, unmasked (a padding lane reads element 0 and is masked at use), then the
    // sums: one memory round trip for the block instead of one per tensor and 256 elements. After
    // unrolling, a tensor's rounds (elements / 256, rounded up; at most kRounds) are constants.
    constexpr int kRounds = 16;
    static_assert(64 * 64 <= kRounds * 256 && 64 * OBS <= kRounds * 256, "the largest tensors");
    const int wg = (int)threadIdx.x < nwg ? threadIdx.x : 0;
    const float nl0 = part[(int64_t)wg * PT::SIZE + PT::ST], pr0 = part[(int64_t)wg * PT::SIZE + PT::ST + 1];
    float v[13][kRounds];
#pragma unroll
    for (int t = 0; t < 13; ++t)
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const int n = bc_numel<OBS, ACT>(t), k = threadIdx.x + 256 * i;
            if (256 * i < n) v[t][i] = src.p[t][k < n ? k : 0];
        }
    __builtin_amdgcn_sched_barrier(0);  // the scheduler otherwise waits for each load in turn
    double nl = (int)threadIdx.x < nwg ? (double)nl0 : 0.0, pr = (int)threadIdx.x < nwg ? (double)pr0 : 0.0, l2 = 0.0;
#pragma unroll
    for (int t = 0; t < 13; ++t)
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const int n = bc_numel<OBS, ACT>(t), k = threadIdx.x + 256 * i;
            if (256 * i < n) l2 += k < n ? (double)v[t][i] * (double)v[t][i] : 0.0;
        }
    nl = ppo::wave_sum(nl);
    pr = ppo::wave_sum(pr);
    l2 = ppo::wave_sum(l2);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sred[0][threadIdx.x / kWave] = nl;
        sred[1][threadIdx.x / kWave] = pr;
        sred[2][threadIdx.x / kWave] = l2;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < 3; ++q)
        for (int k = 0; k < 256 / kWave; ++k) s[q] += sred[q][k];
    double ent = 0.0;
    for (int a = 0; a < ACT; ++a) ent += 1.41893853320467274 + (double)src.p[12][a];  // 0.5 + 0.5 log 2 pi
    const double neglogp = s[0] / (double)bs, ent_loss = -(double)ent_w * ent;
    const double l2_norm = 0.5 * s[2], l2_loss = (double)l2_w * l2_norm;
    stats[RR_BC_STAT_NEGLOGP] = (float)neglogp;
    stats[RR_BC_STAT_ENTROPY] = (float)ent;
    stats[RR_BC_STAT_ENT_LOSS] = (float)ent_loss;
    stats[RR_BC_STAT_PROB_TRUE_ACT] = (float)(s[1] / (double)bs);
    stats[RR_BC_STAT_L2_NORM] = (float)l2_norm;
    stats[RR_BC_STAT_L2_LOSS] = (float)l2_loss;
    stats[RR_BC_STAT_LOSS] = (float)(neglogp + ent_loss + l2_loss);
    stats[RR_BC_STAT_SLOTS - 1] = 0.0f;
}

// grid (nfin, 2 or 3): blockIdx.y 0 the pi half, 1 the value half, 2 (one block) the statistics
template <int OBS, int ACT>
__global__ __launch_bounds__(256) void bc_finish_kernel(const float* __restrict__ part, int nwg_pi, int64_t bs,
                                                        float ent_coef, float l2_w, PolSrc src, PolGrad dst,
                                                        float* __restrict__ bc_stats, float* __restrict__ normw,
                                                        const float* __restrict__ step0)
{
    if (blockIdx.y == 2) {
        if (blockIdx.x == 0) bc_stats_block<OBS, ACT>(part, nwg_pi, bs, ent_coef, l2_w, src, bc_stats);
        return;
    }
    // the value half has no partial rows: the body's sums run over none and it stores zeros.
    // The learner's statistics and control block are off; normw carries the step count to the optimizer.
    const int nwg = blockIdx.y == 0 ? nwg_pi : 0;
    float* const stats = nullptr;
    constexpr bool CTL = false;
    const ppo::CtlArgs ca = {};
#include "rocket_ppo_finish_body.inc"
    // + l2_weight w: the parameter beside the gradient element `out` (equal offsets in tensor t)
    if (out && l2_w != 0.0f) {
        const float* w = nullptr;
#pragma unroll
        for (int t = 0; t < 13; ++t) {
            const int64_t o = out - dst.p[t];
            if (o >= 0 && o < bc_numel<OBS, ACT>(t)) w = src.p[t] + o;
        }
        if (w) *out = v + l2_w * *w;
    }
}

template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void bc_adam_kernel(AdamList A, const float* __restrict__ normw, int n_norm,
                                                               const float* __restrict__ lr_p, float beta1, float beta2,
                                                               float w1, float w2, float eps, float* __restrict__ pack,
                                                               int nbp)
{
    constexpr float max_norm = 0.0f;  // no clip
    const AdvNext nx = {};            // no next-minibatch blocks: the grid is nbp
#include "rocket_ppo_adam_body.inc"
}

}  // namespace

// rr_bc_update's launches (declared in rocket_device.h); `launch` points to the BcLaunch of the
// calling TU, which validated the arguments and carved the workspace.
extern "C" int rrc_launch_bc(const void* launch, void* stream)
{
    const auto L = from_unit<BcLaunch>(launch);
    hipStream_t s = (hipStream_t)stream;
    auto run = [&](auto obs_c, auto act_c) {
        constexpr int OB = decltype(obs_c)::value, A = decltype(act_c)::value;
        using PT = ppo::Part<OB, A>;
        using K = ppo::Pack<OB, A>;
        constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
        if (!(L.flags & RR_BC_CHAINED))
            hipLaunchKernelGGL((bc_pack_kernel<OB, A>), dim3((K::SIZE + 255) / 256), dim3(256), 0, s, L.ps, L.pack);
        hipLaunchKernelGGL((bc_grad_kernel<OB, A>), dim3(L.nwg, 1), dim3(ppo::kThreads), 0, s, L.obs, L.actions, L.idx,
                           L.batch, (const float*)L.pack, L.part);
        hipLaunchKernelGGL((bc_finish_kernel<OB, A>), dim3(nfin, L.stats ? 3 : 2), dim3(256), 0, s, (const float*)L.part,
                           L.nwg, L.batch, L.ent, L.l2, L.ps, L.pg, L.stats, L.normw, (const float*)L.a.step[0]);
        hipLaunchKernelGGL((bc_adam_kernel<OB, A>), dim3(L.nbp), dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw,
                           2 * nfin, L.lr, L.beta1, L.beta2, L.w1, L.w2, L.eps, L.pack, L.nbp);
    };
    if (L.obs_dim == 14) run(tag<14>{}, tag<3>{});
    else run(tag<7>{}, tag<2>{});
    return (int)hipGetLastError();
}
