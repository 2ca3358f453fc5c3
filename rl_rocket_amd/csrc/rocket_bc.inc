// rocket_bc.inc — the behaviour-cloning kernels and their launch sequence, included as text by the two
// units that compile them: bc/rocket_bc.hip (RR_BC_DISCRETE 0: the diagonal Gaussian, rr_bc_update,
// kernels bc_*) and bc_discrete/rocket_bc_discrete.hip (RR_BC_DISCRETE 1: the Categorical policy over
// the <7, 4> images with a runtime number of choices, rr_bc_update_discrete, kernels bcd_*). The unit
// sets the symbol, includes rocket_device.h, rocket_policy.inc and rocket_ppo.inc ahead of this file and
// defines its hidden entry point around bc_launch. Regions that differ are `#if` regions, so each
// kernel sees the token stream it had on its own (DESIGN.md §8 "One behaviour-cloning kernel text").
//
// It is the learner's pipeline (rocket_ppo.inc) with another head derivative and no value half:
//   packing   the pi tower's LDS image (ppo::pack_value; discrete_pack_value with zeros for heads >= K
//             and for log_std's slots), skipped by a chained call;
//   gradient  ppo_grad_tower<OBS, ACT, 0, false, false, LOSS> on a grid of (nwg, 1): the pi tower's
//             forward, backward and weight gradients as they are, d loss / d logp = -1 / B. LOSS 1 is
//             the Gaussian head; LOSS 3 is LOSS 2's softmax head and per-sample entropy gradient (the
//             demonstrated index is compared against k, never used as an address);
//   finish    rocket_ppo_finish_body.inc as text: the fixed-order sum of the workgroups' partial
//             vectors scattered into the gradient tensors. The Gaussian's entropy gradient is the
//             body's -ent_weight per log_std element; the Categorical's came with the head derivative
//             (ent_coef 0 inside the body), and its elements of heads >= K and of log_std's slots go to
//             a sink, as in discrete_finish_kernel. The value half (blockIdx.y 1) runs the body over
//             zero partial rows, so its tensors are written as zeros. After it every element that has
//             a parameter adds l2_weight w. A third row of blocks (blockIdx.y 2) sums the statistics:
//             the workgroups' -logp, exp(logp) (and H) sums and all w^2 at the tensors' real sizes,
//             each in a fixed order;
//   optimizer rocket_ppo_adam_body.inc as text with max_norm 0 (its "no clip" branch) and no
//             next-minibatch blocks; it repacks both tower images for the chained call.
#if RR_BC_DISCRETE
#define RR_BC_K(name) bcd_##name
#else
#define RR_BC_K(name) bc_##name
#endif

namespace {

#if RR_BC_DISCRETE
constexpr int kBcTensors = 12, kBcSums = 4;  // no log_std; -logp, exp(logp), H, w^2
#else
constexpr int kBcTensors = 13, kBcSums = 3;
#endif

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void RR_BC_K(pack_kernel)(PolSrc src,
#if RR_BC_DISCRETE
                                                            int n_choices,
#endif
                                                            float* __restrict__ pack)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
#if RR_BC_DISCRETE
    if (k < ppo::Pack<OBS, ACT>::SIZE) pack[k] = discrete_pack_value<OBS, ACT>(src, n_choices, 0, k);
#else
    if (k < ppo::Pack<OBS, ACT>::SIZE) pack[k] = ppo::pack_value<OBS, ACT>(src, 0, k);
#endif
}

template <int OBS, int ACT>
__global__ __launch_bounds__(ppo::kThreads) void RR_BC_K(grad_kernel)(const float* __restrict__ obs,
                                                                      const float* __restrict__ act,
                                                                      const int64_t* __restrict__ idx, int64_t bs,
#if RR_BC_DISCRETE
                                                                      float ent_w, int n_choices,
#endif
                                                                      const float* __restrict__ pack,
                                                                      float* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
#if RR_BC_DISCRETE
    ppo_grad_tower<OBS, ACT, 0, false, false, 3>(lds, obs, act, nullptr, nullptr, nullptr, idx, bs, 0.0f, 0.0f, nullptr,
                                                 pack, part, nullptr, 0.0f, n_choices, ent_w);
#else
    ppo_grad_tower<OBS, ACT, 0, false, false, 1>(lds, obs, act, nullptr, nullptr, nullptr, idx, bs, 0.0f, 0.0f, nullptr,
                                                 pack, part);
#endif
}

// elements of policy tensor t (rr_ppo_grad's order; the Categorical's 12 are its first 12) with `heads`
// action-head rows: ACT, or the Categorical's K choices
template <int OBS>
__device__ __forceinline__ constexpr int bc_numel(int t, int heads)
{
    return t == 0 || t == 4 ? 64 * OBS
           : t == 2 || t == 6 ? 64 * 64
           : t == 8 ? 64 * heads
           : t == 9 || t == 12 ? heads
           : t == 11 ? 1
                     : 64;
}

// The statistics block: one fixed-order sum each of the workgroups' -logp, exp(logp) (and H) partial
// sums (thread = workgroup) and of every parameter's square (thread k: elements k, k + 256, ... of each
// tensor in turn), in fp64; the wave sums are butterflies, the four waves are added in order. The
// Categorical's head tensors are read at their real sizes [K][64] and [K]: their rounds are those of
// ACT rows, the elements past K rows masked.
template <int OBS, int ACT>
__device__ __forceinline__ void RR_BC_K(stats_block)(const float* __restrict__ part, int nwg, int64_t bs,
#if RR_BC_DISCRETE
                                                     int n_choices,
#endif
                                                     float ent_w, float l2_w, const PolSrc& src,
                                                     float* __restrict__ stats)
{
#if !RR_BC_DISCRETE
    constexpr int n_choices = ACT;  // every head row is real
#endif
    using PT = ppo::Part<OBS, ACT>;
    __shared__ double sred[kBcSums][256 / kWave];
    static_assert(ppo::kMaxWG <= 256, "one workgroup's sums per thread");
    // Every load first, unmasked (a padding lane reads element 0 and is masked at use), then the
    // sums: one memory round trip for the block instead of one per tensor and 256 elements. After
    // unrolling, a tensor's rounds (elements / 256, rounded up; at most kRounds) are constants.
    constexpr int kRounds = 16;
    static_assert(64 * 64 <= kRounds * 256 && 64 * OBS <= kRounds * 256 && (!RR_BC_DISCRETE || 64 * ACT <= 256),
                  "the largest tensors");
    const int wg = (int)threadIdx.x < nwg ? threadIdx.x : 0;
#if RR_BC_DISCRETE
    const float* row = part + (int64_t)wg * PT::SIZE + PT::ST;
    const float nl0 = row[0], pr0 = row[1], en0 = row[3];
#else
    const float nl0 = part[(int64_t)wg * PT::SIZE + PT::ST], pr0 = part[(int64_t)wg * PT::SIZE + PT::ST + 1];
#endif
    float v[kBcTensors][kRounds];
#pragma unroll
    for (int t = 0; t < kBcTensors; ++t)
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
#if RR_BC_DISCRETE
            const int cap = bc_numel<OBS>(t, ACT), n = bc_numel<OBS>(t, n_choices), k = threadIdx.x + 256 * i;
#else
            const int n = bc_numel<OBS>(t, ACT), cap = n, k = threadIdx.x + 256 * i;
#endif
            if (256 * i < cap) v[t][i] = src.p[t][k < n ? k : 0];
        }
    __builtin_amdgcn_sched_barrier(0);  // the scheduler otherwise waits for each load in turn
    const bool own = (int)threadIdx.x < nwg;
#if RR_BC_DISCRETE
    double nl = own ? (double)nl0 : 0.0, pr = own ? (double)pr0 : 0.0, en = own ? (double)en0 : 0.0, l2 = 0.0;
#else
    double nl = own ? (double)nl0 : 0.0, pr = own ? (double)pr0 : 0.0, l2 = 0.0;
#endif
#pragma unroll
    for (int t = 0; t < kBcTensors; ++t)
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
#if RR_BC_DISCRETE
            const int cap = bc_numel<OBS>(t, ACT), n = bc_numel<OBS>(t, n_choices), k = threadIdx.x + 256 * i;
#else
            const int n = bc_numel<OBS>(t, ACT), cap = n, k = threadIdx.x + 256 * i;
#endif
            if (256 * i < cap) l2 += k < n ? (double)v[t][i] * (double)v[t][i] : 0.0;
        }
    nl = ppo::wave_sum(nl);
    pr = ppo::wave_sum(pr);
#if RR_BC_DISCRETE
    en = ppo::wave_sum(en);
#endif
    l2 = ppo::wave_sum(l2);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sred[0][threadIdx.x / kWave] = nl;
        sred[1][threadIdx.x / kWave] = pr;
#if RR_BC_DISCRETE
        sred[2][threadIdx.x / kWave] = en;
#endif
        sred[kBcSums - 1][threadIdx.x / kWave] = l2;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[kBcSums] = {};
    for (int q = 0; q < kBcSums; ++q)
        for (int k = 0; k < 256 / kWave; ++k) s[q] += sred[q][k];
#if RR_BC_DISCRETE
    const double neglogp = s[0] / (double)bs, ent = s[2] / (double)bs, ent_loss = -(double)ent_w * ent;
#else
    double ent = 0.0;
    for (int a = 0; a < ACT; ++a) ent += 1.41893853320467274 + (double)src.p[12][a];  // 0.5 + 0.5 log 2 pi
    const double neglogp = s[0] / (double)bs, ent_loss = -(double)ent_w * ent;
#endif
    const double l2_norm = 0.5 * s[kBcSums - 1], l2_loss = (double)l2_w * l2_norm;
    stats[RR_BC_STAT_NEGLOGP] = (float)neglogp;
    stats[RR_BC_STAT_ENTROPY] = (float)ent;
    stats[RR_BC_STAT_ENT_LOSS] = (float)ent_loss;
    stats[RR_BC_STAT_PROB_TRUE_ACT] = (float)(s[1] / (double)bs);
    stats[RR_BC_STAT_L2_NORM] = (float)l2_norm;
    stats[RR_BC_STAT_L2_LOSS] = (float)l2_loss;
    stats[RR_BC_STAT_LOSS] = (float)(neglogp + ent_loss + l2_loss);
    stats[RR_BC_STAT_SLOTS - 1] = 0.0f;
}

// grid (nfin, 2 or 3): blockIdx.y 0 the pi half, 1 the value half, 2 (one block) the statistics. The
// Categorical's lists have four spare floats as p[12]; its dst_sink is dst_in with the action head's
// weight and bias gradients replaced by a [4][64] + [4] sink (discrete_finish_kernel's arrangement).
template <int OBS, int ACT>
__global__ __launch_bounds__(256) void RR_BC_K(finish_kernel)(const float* __restrict__ part, int nwg_pi, int64_t bs,
#if RR_BC_DISCRETE
                                                              int n_choices, float ent_w, float l2_w, PolSrc src,
                                                              PolGrad dst_in, PolGrad dst_sink,
#else
                                                              float ent_coef, float l2_w, PolSrc src, PolGrad dst,
#endif
                                                              float* __restrict__ bc_stats, float* __restrict__ normw,
                                                              const float* __restrict__ step0)
{
    if (blockIdx.y == 2) {
#if RR_BC_DISCRETE
        if (blockIdx.x == 0) bcd_stats_block<OBS, ACT>(part, nwg_pi, bs, n_choices, ent_w, l2_w, src, bc_stats);
#else
        if (blockIdx.x == 0) bc_stats_block<OBS, ACT>(part, nwg_pi, bs, ent_coef, l2_w, src, bc_stats);
#endif
        return;
    }
#if RR_BC_DISCRETE
    // An element of a head >= n_choices (a zero sum) must not land past the [n_choices][64] weight and
    // [n_choices] bias gradients: the thread that holds one writes it to the sink.
    using P = ppo::Part<OBS, ACT>;
    const int el = blockIdx.x * kFinElems + threadIdx.x % kFinElems;
    const bool spare = blockIdx.y == 0 && ((el >= P::HW + 64 * n_choices && el < P::HB) ||
                                           (el >= P::HB + n_choices && el < P::LS));
    const PolGrad& dst = spare ? dst_sink : dst_in;
    constexpr float ent_coef = 0.0f;  // the body's entropy lines are the Gaussian's: off
#else
    constexpr int n_choices = ACT;  // every head row is real
    const PolGrad& dst_in = dst;
#endif
    // the value half has no partial rows: the body's sums run over none and it stores zeros.
    // The learner's statistics and control block are off; normw carries the step count to the optimizer.
    const int nwg = blockIdx.y == 0 ? nwg_pi : 0;
    float* const stats = nullptr;
    constexpr bool CTL = false;
    const ppo::CtlArgs ca = {};
#include "rocket_ppo_finish_body.inc"
    // + l2_weight w: the parameter beside the gradient element `out` (equal offsets in tensor t, at the
    // tensors' real sizes). A Categorical element in the sink or in log_std's spare slot has no parameter.
#if RR_BC_DISCRETE
    if (out && !spare && e < PT::LS && l2_w != 0.0f) {
#else
    if (out && l2_w != 0.0f) {
#endif
        const float* w = nullptr;
#pragma unroll
        for (int t = 0; t < kBcTensors; ++t) {
            const int64_t o = out - dst_in.p[t];
            if (o >= 0 && o < bc_numel<OBS>(t, n_choices)) w = src.p[t] + o;
        }
        if (w) *out = v + l2_w * *w;
    }
}

template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void RR_BC_K(adam_kernel)(AdamList A, const float* __restrict__ normw,
                                                                     int n_norm, const float* __restrict__ lr_p,
                                                                     float beta1, float beta2, float w1, float w2,
                                                                     float eps, float* __restrict__ pack, int nbp)
{
    constexpr float max_norm = 0.0f;  // no clip
    const AdvNext nx = {};            // no next-minibatch blocks: the grid is nbp
#include "rocket_ppo_adam_body.inc"
}

// The call's launches at one shape, from the BcLaunch of the main unit, which validated the arguments
// and carved the workspace.
template <int OB, int A>
int bc_launch(const BcLaunch& L, hipStream_t s)
{
    using PT = ppo::Part<OB, A>;
    using K = ppo::Pack<OB, A>;
    constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
    if (!(L.flags & RR_BC_CHAINED))
        hipLaunchKernelGGL((RR_BC_K(pack_kernel)<OB, A>), dim3((K::SIZE + 255) / 256), dim3(256), 0, s, L.ps,
#if RR_BC_DISCRETE
                           L.n_choices,
#endif
                           L.pack);
    hipLaunchKernelGGL((RR_BC_K(grad_kernel)<OB, A>), dim3(L.nwg, 1), dim3(ppo::kThreads), 0, s, L.obs, L.actions, L.idx,
                       L.batch,
#if RR_BC_DISCRETE
                       L.ent, L.n_choices,
#endif
                       (const float*)L.pack, L.part);
#if RR_BC_DISCRETE
    PolGrad pg_sink = L.pg;
    pg_sink.p[8] = L.sink;
    pg_sink.p[9] = L.sink + 64 * A;
#endif
    hipLaunchKernelGGL((RR_BC_K(finish_kernel)<OB, A>), dim3(nfin, L.stats ? 3 : 2), dim3(256), 0, s,
                       (const float*)L.part, L.nwg, L.batch,
#if RR_BC_DISCRETE
                       L.n_choices, L.ent, L.l2, L.ps, L.pg, pg_sink,
#else
                       L.ent, L.l2, L.ps, L.pg,
#endif
                       L.stats, L.normw, (const float*)L.a.step[0]);
    hipLaunchKernelGGL((RR_BC_K(adam_kernel)<OB, A>), dim3(L.nbp), dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw,
                       2 * nfin, L.lr, L.beta1, L.beta2, L.w1, L.w2, L.eps, L.pack, L.nbp);
    return (int)hipGetLastError();
}

}  // namespace
