// rocket_bc_discrete.hip — the tenth translation unit of librocket_hip.so: behaviour cloning of the
// Categorical policy on the device (rr_bc_update_discrete), what imitation's bc.BC does per minibatch
// for SB3's MlpPolicy over Discrete(K) (the reference's keyboard demonstrations are indices into
// DiscreteActions3DOF's table):
//   log p_ik = z_ik - logsumexp_k z_ik,  logp_i = log p_{i, a_i},  H_i = -sum_k p_ik log p_ik
//   loss     = -mean_i logp_i - ent_weight mean_i H_i + l2_weight 0.5 sum_{all 12 tensors} w^2
//   Adam (capturable, no clip) over the 12 tensors.
// It is bc/rocket_bc.hip's pipeline over discrete/rocket_discrete.hip's <7, 4> images, the choices
// K = 2 .. 4 a runtime count:
//   packing   the pi tower's LDS image with zeros for heads >= K and for log_std's slots
//             (discrete_pack_value), skipped by a chained call;
//   gradient  ppo_grad_tower<7, 4, 0, false, false, LOSS 3> on a grid of (nwg, 1): LOSS 2's softmax head
//             and per-sample entropy gradient with LOSS 1's d loss / d logp = -1 / B. The demonstrated
//             index is compared against k, never used as an address;
//   finish    rocket_ppo_finish_body.inc as text over 12 tensors (ent_coef 0 inside the body: the
//             entropy's gradient came with the head derivative). The value half (blockIdx.y 1) runs it
//             over zero partial rows. Elements of heads >= K and log_std's slots go to a sink, as in
//             discrete_finish_kernel; every other element then adds l2_weight w (a sink element reads
//             no w: the head tensors have K rows). A third row of blocks (blockIdx.y 2) sums the
//             statistics: the workgroups' -logp, exp(logp) and H sums and all w^2 at the tensors' real
//             sizes, each in a fixed order;
//   optimizer rocket_ppo_adam_body.inc as text with max_norm 0 and no next-minibatch blocks; it repacks
//             the <7, 4> images for the chained call.
// Launched through rrc_launch_bc_discrete with a BcDiscreteLaunch. Compiled with the collect translation
// unit's settings (build.py COLLECT_FLAGS), because the gradient kernel's loop is the learner's.
//
// It is a translation unit of its own so that the kernels which existed before it keep their
// machine code (see eval_trace/rocket_eval_trace.hip).
#include "rocket_device.h"
#define RR_POL_PREFETCH_A 1
#include "rocket_policy.inc"
#include "rocket_ppo.inc"

namespace {

template <int OBS, int ACT>
__global__ __launch_bounds__(256) void bcd_pack_kernel(PolSrc src, int n_choices, float* __restrict__ pack)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < ppo::Pack<OBS, ACT>::SIZE) pack[k] = discrete_pack_value<OBS, ACT>(src, n_choices, 0, k);
}

template <int OBS, int ACT>
__global__ __launch_bounds__(ppo::kThreads) void bcd_grad_kernel(const float* __restrict__ obs,
                                                                 const float* __restrict__ act,
                                                                 const int64_t* __restrict__ idx, int64_t bs,
                                                                 float ent_w, int n_choices,
                                                                 const float* __restrict__ pack,
                                                                 float* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lds[ppo::Lds<OBS, ACT>::SIZE];
    ppo_grad_tower<OBS, ACT, 0, false, false, 3>(lds, obs, act, nullptr, nullptr, nullptr, idx, bs, 0.0f, 0.0f, nullptr,
                                                 pack, part, nullptr, 0.0f, n_choices, ent_w);
}

// elements of tensor t of the Categorical policy's 12 (rr_ppo_update_discrete's order) with K choices
template <int OBS>
__device__ __forceinline__ int bcd_numel(int t, int n_choices)
{
    return t == 0 || t == 4 ? 64 * OBS
           : t == 2 || t == 6 ? 64 * 64
           : t == 8 ? 64 * n_choices
           : t == 9 ? n_choices
           : t == 11 ? 1
                     : 64;
}

// The statistics block: bc_stats_block's fixed-order fp64 sums (thread = workgroup for the -logp,
// exp(logp) and H partial sums; thread k: elements k, k + 256, ... of each tensor in turn for w^2); the
// wave sums are butterflies, the four waves are added in order. The head tensors are read at their real
// sizes [K][64] and [K]: their rounds are those of four rows, the elements past K rows masked.
template <int OBS, int ACT>
__device__ __forceinline__ void bcd_stats_block(const float* __restrict__ part, int nwg, int64_t bs, int n_choices,
                                                float ent_w, float l2_w, const PolSrc& src, float* __restrict__ stats)
{
    using PT = ppo::Part<OBS, ACT>;
    __shared__ double sred[4][256 / kWave];
    static_assert(ppo::kMaxWG <= 256, "one workgroup's sums per thread");
    constexpr int kRounds = 16;
    static_assert(64 * 64 <= kRounds * 256 && 64 * OBS <= kRounds * 256 && 64 * ACT <= 256, "the largest tensors");
    const int wg = (int)threadIdx.x < nwg ? threadIdx.x : 0;
    const float* row = part + (int64_t)wg * PT::SIZE + PT::ST;
    const float nl0 = row[0], pr0 = row[1], en0 = row[3];
    float v[12][kRounds];
#pragma unroll
    for (int t = 0; t < 12; ++t)
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const int cap = bcd_numel<OBS>(t, ACT), n = bcd_numel<OBS>(t, n_choices), k = threadIdx.x + 256 * i;
            if (256 * i < cap) v[t][i] = src.p[t][k < n ? k : 0];
        }
    __builtin_amdgcn_sched_barrier(0);  // the scheduler otherwise waits for each load in turn
    const bool own = (int)threadIdx.x < nwg;
    double nl = own ? (double)nl0 : 0.0, pr = own ? (double)pr0 : 0.0, en = own ? (double)en0 : 0.0, l2 = 0.0;
#pragma unroll
    for (int t = 0; t < 12; ++t)
#pragma unroll
        for (int i = 0; i < kRounds; ++i) {
            const int cap = bcd_numel<OBS>(t, ACT), n = bcd_numel<OBS>(t, n_choices), k = threadIdx.x + 256 * i;
            if (256 * i < cap) l2 += k < n ? (double)v[t][i] * (double)v[t][i] : 0.0;
        }
    nl = ppo::wave_sum(nl);
    pr = ppo::wave_sum(pr);
    en = ppo::wave_sum(en);
    l2 = ppo::wave_sum(l2);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sred[0][threadIdx.x / kWave] = nl;
        sred[1][threadIdx.x / kWave] = pr;
        sred[2][threadIdx.x / kWave] = en;
        sred[3][threadIdx.x / kWave] = l2;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < 4; ++q)
        for (int k = 0; k < 256 / kWave; ++k) s[q] += sred[q][k];
    const double neglogp = s[0] / (double)bs, ent = s[2] / (double)bs, ent_loss = -(double)ent_w * ent;
    const double l2_norm = 0.5 * s[3], l2_loss = (double)l2_w * l2_norm;
    stats[RR_BC_STAT_NEGLOGP] = (float)neglogp;
    stats[RR_BC_STAT_ENTROPY] = (float)ent;
    stats[RR_BC_STAT_ENT_LOSS] = (float)ent_loss;
    stats[RR_BC_STAT_PROB_TRUE_ACT] = (float)(s[1] / (double)bs);
    stats[RR_BC_STAT_L2_NORM] = (float)l2_norm;
    stats[RR_BC_STAT_L2_LOSS] = (float)l2_loss;
    stats[RR_BC_STAT_LOSS] = (float)(neglogp + ent_loss + l2_loss);
    stats[RR_BC_STAT_SLOTS - 1] = 0.0f;
}

// grid (nfin, 2 or 3): blockIdx.y 0 the pi half, 1 the value half, 2 (one block) the statistics. Both
// lists' p[12] is four spare floats; dst_sink is dst_in with the action head's weight and bias gradients
// replaced by a [4][64] + [4] sink (discrete_finish_kernel's arrangement).
template <int OBS, int ACT>
__global__ __launch_bounds__(256) void bcd_finish_kernel(const float* __restrict__ part, int nwg_pi, int64_t bs,
                                                         int n_choices, float ent_w, float l2_w, PolSrc src,
                                                         PolGrad dst_in, PolGrad dst_sink,
                                                         float* __restrict__ bc_stats, float* __restrict__ normw,
                                                         const float* __restrict__ step0)
{
    if (blockIdx.y == 2) {
        if (blockIdx.x == 0) bcd_stats_block<OBS, ACT>(part, nwg_pi, bs, n_choices, ent_w, l2_w, src, bc_stats);
        return;
    }
    // An element of a head >= n_choices (a zero sum) must not land past the [n_choices][64] weight and
    // [n_choices] bias gradients: the thread that holds one writes it to the sink.
    using P = ppo::Part<OBS, ACT>;
    const int el = blockIdx.x * kFinElems + threadIdx.x % kFinElems;
    const bool spare = blockIdx.y == 0 && ((el >= P::HW + 64 * n_choices && el < P::HB) ||
                                           (el >= P::HB + n_choices && el < P::LS));
    const PolGrad& dst = spare ? dst_sink : dst_in;
    // the value half has no partial rows: the body's sums run over none and it stores zeros. The body's
    // entropy lines are the Gaussian's: off. The learner's statistics and control block are off; normw
    // carries the step count to the optimizer.
    const int nwg = blockIdx.y == 0 ? nwg_pi : 0;
    constexpr float ent_coef = 0.0f;
    float* const stats = nullptr;
    constexpr bool CTL = false;
    const ppo::CtlArgs ca = {};
#include "rocket_ppo_finish_body.inc"
    // + l2_weight w: the parameter beside the gradient element `out` (equal offsets in tensor t, at the
    // tensors' real sizes). An element in the sink or in log_std's spare slot has no parameter.
    if (out && !spare && e < PT::LS && l2_w != 0.0f) {
        const float* w = nullptr;
#pragma unroll
        for (int t = 0; t < 12; ++t) {
            const int64_t o = out - dst_in.p[t];
            if (o >= 0 && o < bcd_numel<OBS>(t, n_choices)) w = src.p[t] + o;
        }
        if (w) *out = v + l2_w * *w;
    }
}

template <int OBS, int ACT>
__global__ __launch_bounds__(kAdamThreads) void bcd_adam_kernel(AdamList A, const float* __restrict__ normw, int n_norm,
                                                                const float* __restrict__ lr_p, float beta1, float beta2,
                                                                float w1, float w2, float eps, float* __restrict__ pack,
                                                                int nbp)
{
    constexpr float max_norm = 0.0f;  // no clip
    const AdvNext nx = {};            // no next-minibatch blocks: the grid is nbp
#include "rocket_ppo_adam_body.inc"
}

}  // namespace

// rr_bc_update_discrete's launches (declared in rocket_device.h); `launch` points to the BcDiscreteLaunch
// of the calling TU, which validated the arguments and carved the workspace.
extern "C" int rrc_launch_bc_discrete(const void* launch, void* stream)
{
    const auto D = from_unit<BcDiscreteLaunch>(launch);
    const BcLaunch& L = D.b;
    hipStream_t s = (hipStream_t)stream;
    constexpr int O = 7, A = 4;
    using PT = ppo::Part<O, A>;
    using K = ppo::Pack<O, A>;
    constexpr int nfin = (PT::SIZE + kFinElems - 1) / kFinElems;
    if (!(L.flags & RR_BC_CHAINED))
        hipLaunchKernelGGL((bcd_pack_kernel<O, A>), dim3((K::SIZE + 255) / 256), dim3(256), 0, s, L.ps, D.n_choices,
                           L.pack);
    hipLaunchKernelGGL((bcd_grad_kernel<O, A>), dim3(L.nwg, 1), dim3(ppo::kThreads), 0, s, L.obs, L.actions, L.idx,
                       L.batch, L.ent, D.n_choices, (const float*)L.pack, L.part);
    PolGrad pg_sink = L.pg;
    pg_sink.p[8] = D.sink;
    pg_sink.p[9] = D.sink + 64 * A;
    hipLaunchKernelGGL((bcd_finish_kernel<O, A>), dim3(nfin, L.stats ? 3 : 2), dim3(256), 0, s, (const float*)L.part,
                       L.nwg, L.batch, D.n_choices, L.ent, L.l2, L.ps, L.pg, pg_sink, L.stats, L.normw,
                       (const float*)L.a.step[0]);
    hipLaunchKernelGGL((bcd_adam_kernel<O, A>), dim3(L.nbp), dim3(kAdamThreads), 0, s, L.a, (const float*)L.normw,
                       2 * nfin, L.lr, L.beta1, L.beta2, L.w1, L.w2, L.eps, L.pack, L.nbp);
    return (int)hipGetLastError();
}
