/*
 * rocket_hip.h — C-ABI of librocket_hip.so, the MI355X-native vectorized
 * rocket-landing env step (gfx950 HIP kernels).
 *
 * The reference has no native boundary: its hot path is the Python gym 0.21
 * Env API (reference my_environment/envs/rocket_env.py). Each entry point below
 * replaces one reference interface, batched over N independent envs that live in
 * HBM in struct-of-arrays fp32 layout:
 *
 *   rr_create      <- Rocket6DOF.__init__ rocket_env.py:511-663 / Rocket.__init__ :27-135
 *                     (kwargs lowered to rr_params on the host, rl_rocket_amd/params.py)
 *   rr_reset       <- Rocket6DOF.reset rocket_env.py:665-688 / Rocket.reset :137-148
 *                     (+ seed(): rocket_env.py:1063-1065 / :478-480)
 *   rr_step        <- Rocket6DOF.step rocket_env.py:690-719 (+ Simulator6DOF.step/RHS
 *                     simulator.py:227-378) / Rocket.step :150-175 (+ simulator.py:55-130),
 *                     fused with gym TimeLimit (main_6DOF.py:21), the SB3 vec-env auto-reset
 *                     and, optionally, RewardAnnealing (wrappers.py:68-86)
 *   rr_set_state / rr_get_state
 *                  <- direct access to Simulator*.state / .t used by the reference's
 *                     callers (env.SIM, rocket_env.py:686, :694; used here for parity
 *                     injection and checkpoint/restore)
 *   rr_fetch_done / rr_copy_terminal / rr_get_buffers
 *                  <- info["terminal_observation"] / Monitor episode stats for done envs
 *                     (SB3 DummyVecEnv / Monitor, main_6DOF.py:18-24)
 *
 * Conventions
 *   - All data pointers are DEVICE pointers (e.g. torch.Tensor.data_ptr()) on the
 *     handle's device, or pinned host memory from rr_host_alloc (zero-copy: the kernels read
 *     and write it directly), owned by the caller unless stated otherwise.
 *   - Every call is asynchronous on the given hipStream_t (pass as void*; NULL = the
 *     default stream). Apart from rr_fetch_done (documented as synchronising), no call
 *     synchronises, allocates or frees after rr_create, so rr_step / rr_reset can be
 *     captured into a hipGraph.
 *   - Return value: 0 on success, < 0 on error (RR_E*); rr_last_error() returns a
 *     thread-local message. No exception or abort crosses the ABI.
 *   - A handle is not thread-safe; use one handle per stream / GPU.
 */
#ifndef ROCKET_HIP_H
#define ROCKET_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 14: rr_policy_evaluate. rr_policy_evaluate_trace / rr_eval_trace joined ABI 14 later as a pure
 * addition (no existing declaration changed), so the number did not move: a caller that needs the
 * recording entry point looks the symbol up. */
#define RR_ABI_VERSION 14

/* error codes */
#define RR_OK 0
#define RR_EINVAL -1   /* bad argument */
#define RR_EHIP -2     /* HIP runtime error */
#define RR_ENOMEM -3   /* allocation failed */

/* models */
#define RR_MODEL_3DOF 3
#define RR_MODEL_6DOF 6

/* integrators. RK4 is the fast parity mode (fp32 state; matches the reference's
 * adaptive RK45 + terminal ground event to <= 1e-5 floored-relative).
 * EULER is a declared NON-parity speed mode (BASELINE config "3DOF Euler").
 * DOPRI5 is the exact mode: fp64 state and the reference's own integrator
 * (scipy RK45: select_initial_step, DOPRI5 tableau, RMS error controller, dense-output
 * brentq ground event; simulator.py:230-241 / :58-69), per-env adaptive, with the
 * simulator clock t (round(t + dt, 3), simulator.py:245) kept as elapsed_steps * dt. */
#define RR_INT_RK4 0
#define RR_INT_EULER 1
#define RR_INT_DOPRI5 2

/* rr_params.flags */
#define RR_FLAG_AUTO_RESET 0x1        /* reset done envs inside rr_step (SB3 vec-env semantics) */
#define RR_FLAG_EPISODE_STATS 0x2     /* keep per-env episode return (Monitor) */
#define RR_FLAG_REWARD_ANNEALING 0x4  /* reward = attitude + goal - xi*(a_thrust+1)  (wrappers.py:72-86) */
#define RR_FLAG_ACTION_SOA 0x8        /* action laid out [n_act][N] instead of [N][n_act] */
#define RR_FLAG_SCIPY_H0_CLAMP 0x10   /* DOPRI5: scipy >= 1.12 select_initial_step (clamp h0 to
                                         the interval); default = scipy 1.7 (requirements.txt:73) */
#define RR_FLAG_HOST_STATE 0x20       /* the state planes (+ v0, counter words, episode returns) live in
                                         pinned, GPU-coherent host memory instead of HBM: after the
                                         stream is synchronised the host reads them through
                                         rr_get_buffers with no copy. For small N — the single-env gym
                                         shims (rocket_env.py:690-719 called once per env step), whose
                                         step is then one launch + one synchronise with the action and
                                         outputs in rr_host_alloc memory */

#define RR_MAX_STATE 14

/* Per-config constants. Lowered on the host from the reference env kwargs
 * (rl_rocket_amd/params.py restates rocket_env.py:51-123 / :557-658). Values the
 * reference holds as Python floats are double here; the fp32 kernels round them once
 * at rr_create (bounds with the rounding direction that keeps each comparison exact). */
typedef struct rr_params {
    int32_t model;               /* RR_MODEL_3DOF | RR_MODEL_6DOF */
    int32_t integrator;          /* RR_INT_* */
    int32_t max_episode_steps;   /* gym TimeLimit; 0 = none */
    uint32_t flags;              /* RR_FLAG_* */
    double dt;                   /* timestep [s] */
    float ic_low[RR_MAX_STATE];  /* init_space Box low  (float32, rocket_env.py:564-567) */
    float ic_high[RR_MAX_STATE]; /* init_space Box high */
    double normalizer[RR_MAX_STATE]; /* state_normalizer, float64 (rocket_env.py:592-612 / :76-94) */
    double bounds_low[3];        /* 6DOF: position Box low (float32 values, inclusive);
                                    3DOF: [-x_bound, -, -] (x <= -x_bound is out) */
    double bounds_high[3];       /* 6DOF: position Box high; 3DOF: [x_bound, z_bound, -] (>= is out) */
    double max_gimbal;           /* rad */
    double max_thrust;           /* N */
    double alfa, beta, eta, gamma, delta, kappa, xi; /* reward_coeff */
    double waypoint, landing_radius, max_velocity;
    double att_limit[3];         /* trajectory_limits["attitude_limit"] (zyx) */
    double land_att_limit[3];    /* landing_params["landing_attitude_limit"] */
    double omega_lim[3];         /* 0.2 hard-coded in the reference (rocket_env.py:656) */
} rr_params;

/* Library-owned device buffers, valid until rr_destroy. done_bits / terminal_* refer
 * to the MOST RECENT rr_step on the handle (overwritten by the next step). */
typedef struct rr_buffers {
    float* state;          /* [state_dim][N] fp32 SoA */
    float* v0;             /* [N] ||IC velocity|| of the episode (rocket_env.py:989-991) */
    int32_t* elapsed;      /* [N] counter word: TimeLimit steps in bits 0..E-1, episode in bits E..31,
                              E = rr_counter_bits() */
    float* ep_return;      /* [N] running episode return (RR_FLAG_EPISODE_STATS) */
    uint64_t* done_bits;   /* [ceil(N/64)] wave-ballot done masks: bit b of word w <=> env 64w+b done */
    float* terminal_obs;   /* [N][state_dim] final obs of env i, valid where done[i] */
    float* terminal_return;/* [N] episode return of env i, valid where done[i] */
    int32_t* terminal_len; /* [N] episode length of env i, valid where done[i] */
} rr_buffers;

typedef struct rr_env rr_env;

int rr_abi_version(void);
const char* rr_last_error(void);

/* Allocate N envs on `device`. env_id_offset = global id of env 0 (multi-GPU shards
 * use rank*N so every env has its own RNG stream). Envs start un-initialised: call
 * rr_reset before the first rr_step. 1 <= N and N * (state_dim + 3) * 4 <= 2^32 - 1 (the
 * kernels address each plane / row block with 32-bit buffer offsets): at most 63 161 283
 * 6DOF or 107 374 182 3DOF envs per handle, else RR_EINVAL; larger batches are several
 * handles (shards). */
int rr_create(rr_env** out, const rr_params* p, int64_t n, int64_t env_id_offset, int device);
int rr_destroy(rr_env* e);
int64_t rr_num_envs(const rr_env* e);
int rr_state_dim(const rr_env* e);
int rr_action_dim(const rr_env* e);

/* Set the key of the reset stream. Resets are counter-based: when env `gid` ends an episode
 * with counter word `cw` (episode number | elapsed steps), its next initial condition comes
 * from a register-resident xorshift128 whose four words are chained lowbias32 mixes of
 * (the seed's four key words — splitmix64 of `seed` on the host — , gid, cw): deterministic,
 * independent of how envs are sharded over GPUs, and free of per-env RNG state in HBM. The
 * episode field has 32 - rr_counter_bits() bits (22 under the reference's TimeLimit 800), so
 * one env's keys do not repeat for 2^22 episodes. Stream-ordered host call: the key is written
 * in the order of `stream` (launches queued on it before the call read the old key) and the
 * call returns once it has landed (it synchronises `stream`, nothing else); it applies to every
 * launch that runs after it, including replays of hipGraphs captured before it, at every N.
 * Launches of the handle (step / reset / rollout) queued on OTHER streams since the last rr_seed
 * are waited for on the device: the key copy waits on a per-handle event recorded on each of
 * those streams (up to 8 distinct streams; past that, or when one of them no longer exists, the
 * call synchronises the device), so no launch still queued there reads a half-written key, and
 * nothing else on the device is waited for. NOT tracked: replays of hipGraphs (they are not
 * launches of the handle) — the caller orders a replay queued on another stream before the seed
 * (seed on the replay's stream, or synchronise it first).
 * RR_EINVAL while `stream` is being captured into a graph. */
int rr_seed(rr_env* e, uint64_t seed, void* stream);
/* Sample a fresh initial condition for every env where mask[i] != 0 (all when mask is
 * NULL), write the normalised obs [N][state_dim] (obs may be NULL). */
int rr_reset(rr_env* e, const uint8_t* mask, float* obs, void* stream);

/* One env step for all N envs.
 *   action    [N][action_dim] fp32 normalised in [-1,1] (not clipped, like the reference)
 *   obs       [N][state_dim] fp32 out (post-reset obs for done envs under AUTO_RESET)
 *   reward    [N] fp32 out
 *   done      [N] u8 out (ground event | bounds violation | non-finite state | TimeLimit)
 *   truncated [N] u8 out or NULL (TimeLimit.truncated)
 *   terms     [n_terms + 2][N] fp32 out or NULL: info["rewards_dict"] (6DOF 5 terms:
 *             velocity_tracking, thrust_penalty, eta, attitude_constraint, rew_goal;
 *             3DOF 6 terms: ..., attitude_hint, rew_goal), then two planes:
 *             info["bounds_violation"] (0 / 1) and the solve_ivp status: 1 = ground event,
 *             -1 = failure (a post-step state with a NaN / inf component: done, like the
 *             reference's done = bool(status), rocket_env.py:702 / :158), 0 otherwise */
int rr_step(rr_env* e, const float* action, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
            float* terms, void* stream);

/* rr_step with obs, reward and done packed as one fp32 row per env: rows [N][state_dim + 2]
 * = (obs[state_dim], reward, done ? 1 : 0), bitwise the values rr_step writes. One 16-B
 * coalesced tile store per wave, and the row block is exactly the send buffer of the
 * multi-GPU all-gather (rl_rocket_amd.dist.ShardGather), so no copy kernels
 * sit between the step and the collective. truncated / terms as rr_step. RK4 / Euler envs
 * with [N][action_dim] actions. */
int rr_step_rows(rr_env* e, const float* action, float* rows, uint8_t* truncated, float* terms, void* stream);

/* n_steps consecutive rr_step launches on `stream`, step t taking action batch t % n_batches
 * of `actions` ([n_batches][N][action_dim], or [n_batches][action_dim][N] planes with
 * RR_FLAG_ACTION_SOA) — open-loop action sequences already resident on the device (e.g. a
 * benchmark or a replayed plan) without one host call per step. Outputs as rr_step, of the
 * last step. */
int rr_step_repeat(rr_env* e, const float* actions, int64_t n_batches, int64_t n_steps, float* obs, float* reward,
                   uint8_t* done, uint8_t* truncated, float* terms, void* stream);
/* Overwrite / read the per-env state (parity injection, checkpoint / restore).
 * state_soa [state_dim][N] fp32; v0 [N] or NULL (kept on set / skipped on get);
 * elapsed [N] or NULL is the per-env counter word: TimeLimit steps in bits 0..E-1, episodes
 * started in bits E..31 (keys the reset stream), E = rr_counter_bits(e); a plain step count
 * below 2^E is a valid word (episode 0; larger counts would spill into the episode field: the
 * Python layer rejects them). On set, NULL clears the steps and keeps the episode field. The
 * elapsed field saturates at 2^E - 1 (>= max_episode_steps): an env stepped on past its
 * TimeLimit without a reset keeps reporting done / truncated; its Monitor length and, under
 * RR_INT_DOPRI5, its clock t = steps * dt stop there.
 * rr_set_state* zero the Monitor running return (an injected state starts a new segment);
 * rr_get_aux / rr_set_aux round-trip the raw counter words and the running return for a
 * checkpoint. */
int rr_set_state(rr_env* e, const float* state_soa, const float* v0, const int32_t* elapsed, void* stream);
int rr_get_state(rr_env* e, float* state_soa, float* v0, int32_t* elapsed, void* stream);
/* Same with an fp64 state [state_dim][N]. Under RR_INT_DOPRI5 this is the state the
 * integrator carries (the reference's float64 SIM.state); otherwise it is converted
 * to / from the fp32 planes. In DOPRI5 mode elapsed also sets the clock: t = steps*dt. */
int rr_set_state64(rr_env* e, const double* state_soa, const float* v0, const int32_t* elapsed, void* stream);
int rr_get_state64(rr_env* e, double* state_soa, float* v0, int32_t* elapsed, void* stream);
/* Bits E of the elapsed-steps field of the counter word (16 without a TimeLimit). */
int rr_counter_bits(const rr_env* e);
/* Raw counter words [N] and Monitor running returns [N] (either may be NULL). */
int rr_get_aux(rr_env* e, uint32_t* counter, float* ep_return, void* stream);
int rr_set_aux(rr_env* e, const uint32_t* counter, const float* ep_return, void* stream);

/* Pointers to the library-owned buffers (done list of the last step, etc.). */
int rr_get_buffers(rr_env* e, rr_buffers* out);

/* Pinned, GPU-coherent (fine-grained) host memory that the kernels read and write directly:
 * zero-copy step inputs / outputs for small N (the single-env gym shims pass the action and
 * every output of rr_step in it, so a step needs no copy command). Host-only, synchronous;
 * free with rr_host_free. */
int rr_host_alloc(void** out, int64_t bytes);
int rr_host_free(void* p);

/* Host-side retrieval of the last step's done list (SB3 infos: terminal_observation,
 * Monitor episode stats). SYNCHRONISES `stream`. Writes at most `capacity` rows into
 * the HOST arrays (any may be NULL): idx [capacity], term_obs [capacity][state_dim],
 * term_return [capacity], term_len [capacity]; rows are in ascending env order.
 * Returns the number of done envs (>= 0) or an RR_E* code. */
int64_t rr_fetch_done(rr_env* e, int64_t capacity, int32_t* idx, float* term_obs, float* term_return,
                      int32_t* term_len, void* stream);

/* rr_fetch_done for caller-owned per-step snapshots (SB3 infos of a device-output vec env, built
 * after later steps have run): the env indices where done[i] != 0 ([N] u8, device), ascending,
 * and their rows of the given sources — term_obs_src [N][state_dim] f32, term_return_src [N] f32,
 * term_len_src [N] i32, truncated_src [N] u8 (device; e.g. the rows rr_copy_terminal wrote) — into
 * the host arrays idx / term_obs / term_return / term_len / truncated (at most `capacity` rows,
 * any may be NULL; an output needs its source). SYNCHRONISES `stream`. Returns the number of done
 * envs or an RR_E* code. */
int64_t rr_gather_rows(rr_env* e, const uint8_t* done, const float* term_obs_src, const float* term_return_src,
                       const int32_t* term_len_src, const uint8_t* truncated_src, int64_t capacity, int32_t* idx,
                       float* term_obs, float* term_return, int32_t* term_len, uint8_t* truncated, void* stream);

/* Device-to-device copy of the terminal rows of the envs done at the last step (their final
 * obs row [state_dim], episode return, episode length) into the same rows of the caller's
 * [N][state_dim] / [N] / [N] buffers; rows of envs not done are left untouched. Any destination
 * may be NULL. One kernel that reads the last step's done masks. Asynchronous. */
int rr_copy_terminal(rr_env* e, float* term_obs, float* term_return, int32_t* term_len, void* stream);

/* ---- On-device PPO rollouts (BASELINE configs[4]) ----
 * Replace the per-step host work of stable_baselines3 1.6 OnPolicyAlgorithm.collect_rollouts
 * + RolloutBuffer (the reference trains PPO("MlpPolicy", ...), main_6DOF.py:62-69) for
 * an on-device rollout: the MlpPolicy actor-critic (separate pi / vf towers, net_arch
 * [64, 64], tanh, state-independent log_std) runs as one fp32 MFMA launch per step.
 * Supported (obs_dim, act_dim): (14, 3) 6DOF, (7, 2) 3DOF.
 * precision: RR_POLICY_FP32 (default; v_mfma_f32_32x32x2_f32, exact fp32 products. The pack
 * holds the tanh FOLDED into the weights: tanh(x) = 1 - 2 r, r = 1 / (1 + 2^(2 x log2 e)), with
 * W1' = c W1, b1' = c b1, W2' = -2c W2, b2' = c (b2 + row sums of W2), heads W' = -2 W and
 * b' = b + row sums of W (c = 2 log2 e; each folded value computed in fp64 and rounded once to
 * fp32), so a hidden unit is v_exp_f32 + add + v_rcp_f32. The SB3 policy's numbers to a few fp32
 * ulps of each weight and hidden unit: values / means within ~1e-5 of the fp32 MlpPolicy
 * (tests/test_gpu_rollout.py). The PPO learner (rr_ppo_grad) packs and runs the UNfolded tanh,
 * so the rollout's log_prob / value and the learner's recomputation on the same parameters agree
 * to rounding, not bit for bit: at epoch 0 the ratio is 1 and approx_kl 0 only to ~1e-6 / ~1e-12
 * (tests/test_gpu_ppo.py::test_rollout_and_learner_forwards_agree)) or RR_POLICY_BF16 (opt-in; v_mfma_f32_32x32x16_bf16
 * with fp32 accumulation: obs, the tower weights and the first hidden layer rounded to
 * bf16, everything else fp32) or RR_POLICY_FP16X3 (v_mfma_f32_32x32x16_f16 on operands split
 * into two fp16 halves, three MFMAs per k step: ~2^-21 relative products, fp32-level
 * results at ~5x the fp32 MFMA rate). A packed buffer is specific to its precision. */
#define RR_POLICY_FP32 0
#define RR_POLICY_BF16 1
#define RR_POLICY_FP16X3 2

/* Packed parameter buffer for rr_policy_*: returns its size in floats (or RR_EINVAL) and,
 * if off != NULL, the 12 section offsets {L1A, B1, L2A, B2, TOWER, PI, VF, HA, HV, HB, VB,
 * LS} (fragment-ordered layout, rl_rocket_amd/csrc/rocket_policy.inc; filled on the device
 * by rl_rocket_amd.rollout.pack_policy). Host-only. */
int rr_policy_layout(int obs_dim, int act_dim, int precision, int64_t* off);

/* Fill the packed buffer (device, rr_policy_layout floats) from the 13 device fp32 tensors
 * of the actor-critic in PyTorch nn.Linear layouts ([out][in] row-major), src[] being a
 * HOST array of device pointers: pi {W1 [64][obs], b1, W2 [64][64], b2}, vf {W1, b1, W2,
 * b2}, W_action [act][64], b_action, W_value [1][64], b_value, log_std [act]. One launch. */
int rr_policy_pack(int obs_dim, int act_dim, int precision, const float* const* src, float* params, void* stream);

/* One rollout step's policy work (SB3 ActorCriticPolicy.forward + clip, plus the previous
 * step's bookkeeping of collect_rollouts) in one launch:
 *   obs [n][obs_dim] -> action_env [n][act_dim] (clip to [-1, 1], the rr_step input),
 *   action [n][act_dim] (unclipped sample), value [n], log_prob [n], obs_copy [n][obs_dim]
 *   (or NULL; the rollout buffer's obs[t]). The normal draws are counter-based on
 *   (seed, env_id_offset + i, *iter, t): `iter` is a device uint64 the caller advances once
 *   per rollout, so graph replays draw new noise. params 16-B aligned.
 *   The noise key (32-bit arithmetic; mix32 = lowbias32; restated in tests/rollout_ref.py and
 *   pinned element by element by tests/test_gpu_rollout_replay.py):
 *     s   = splitmix64(seed)   one step on the host, as rr_seed's key words, so that the
 *                              streams of two user seeds share nothing (raw seed words XORed
 *                              into the key gave seed 1 the streams of seed 0 with envs e, e ^ 1
 *                              swapped, and seed 2^32 those of seed 0 one iteration on)
 *     key = mix32((uint32)(env_id_offset + i) ^ (uint32)s)
 *     key = mix32(key ^ (uint32)*iter ^ (uint32)(s >> 32))
 *     key = mix32(key ^ (uint32)(*iter >> 32) ^ t * 0x9E3779B9)
 *   and for each pair of action components a = 0, 2, ..: k = key + a * 0x632BE5AB,
 *     h1 = mix32(k), h2 = mix32(k ^ 0x68E31DA4), u1 = ((h1 >> 8) + 1) 2^-24 in (0, 1],
 *     u2 = (h2 >> 8) 2^-24, (eps[a], eps[a + 1]) = sqrt(-2 ln u1) (cos, sin)(2 pi u2).
 *   If reward_out != NULL: reward_out[i] = prev_reward[i] + gamma * V(prev_term_obs[i])
 *   where prev_truncated[i] (the timeout bootstrap of step t-1; rr_step's outputs and
 *   rr_get_buffers' terminal_obs). If start_out != NULL: start_out[i] = done[i] (episode
 *   start flags of step t).
 *   Input domain and accuracy (every rr_policy_* / rr_rollout_* call; pinned at these edges by
 *   tests/test_gpu_policy_edges.py against float64): any obs is accepted. RR_POLICY_FP32 and
 *   RR_POLICY_BF16 hand a NaN component on to the row's value, mean and log_prob. RR_POLICY_FP16X3
 *   converts obs * 2^8 to fp16 and saturates it at fp16's largest finite value: a component past
 *   |obs| = 255.875 (65504 / 2^8) is read as +-255.875, so every finite obs gives finite outputs
 *   (before this saturation such a row's outputs were all NaN). The saturating instruction returns
 *   its smallest operand for a NaN, so on this path a NaN component is read as -255.875 and +-inf as
 *   +-255.875: rows with non-finite obs give finite outputs there and must be recognised by the
 *   caller (rr_step ends such an env's episode on its own state check). The worst-case error of
 *   value and mean grows linearly with |obs| (the layer-1 term (obs_dim + 2) u |W1| |obs|, u = 2^-24
 *   for fp32 and 2^-21 for fp16x3); measured against float64 on an SB3-initialised policy perturbed by
 *   0.3 N(0, 1): 1.3e-6 (value) / 1.5e-6 (mean) at obs ~ N(0, 1) and 5.3e-6 / 9.9e-6 at obs uniform
 *   in +-90 (the envs' own worst case) for fp16x3, 2.7e-6 / 4.8e-6 and 3.2e-6 / 8.0e-6 for fp32; with
 *   the tower weights 8 times larger 1.2e-4 / 1.4e-4 (fp16x3) and 3.5e-5 / 1.5e-4 (fp32) at +-90. */
int rr_policy_act(const float* params, int obs_dim, int act_dim, int precision, int64_t n, int64_t env_id_offset,
                  const float* obs, uint64_t seed, const uint64_t* iter, int t, float* action_env, float* action,
                  float* value, float* log_prob, float* obs_copy, const float* prev_term_obs,
                  const uint8_t* prev_truncated, const float* prev_reward, float gamma, float* reward_out,
                  const uint8_t* done, float* start_out, void* stream);

/* End of a rollout: reward_out[i] = reward[i] + gamma * V(term_obs[i]) where truncated[i]
 * (TimeLimit.truncated), else reward[i] (skipped when term_obs == NULL); and, if
 * value_out != NULL, value_out[i] = V(obs[i]). */
int rr_policy_bootstrap(const float* params, int obs_dim, int act_dim, int precision, int64_t n,
                        const float* term_obs, const uint8_t* truncated, const float* reward, float gamma,
                        float* reward_out, const float* obs, float* value_out, void* stream);

/* One rollout step in ONE launch: rr_policy_act (without its previous-step bookkeeping) and
 * rr_step fused. For every env i of e: obs = state * normalizer^-1 (the obs rr_step /
 * rr_reset last produced) -> buf_obs [n][obs_dim]; a ~ N(mean, exp(log_std)) with the noise
 * key of rr_policy_act (splitmix64(seed), env_id_offset + i, *iter, t: the same draws,
 * whatever the sharding) -> buf_action [n][act_dim] (unclipped),
 * buf_value, buf_log_prob; the env steps with clip(a, -1, 1) (auto-reset, TimeLimit, terminal
 * rows as rr_step); buf_reward[i] = reward + gamma * V(terminal obs) where truncated;
 * buf_start[i] = done[i] as passed in (the previous step's done flags, updated in place to
 * this step's). reward / done (required), truncated / terms (optional) are rr_step's env
 * outputs; obs (optional, NULL to skip) receives the post-step obs. Bitwise the same results
 * as rr_policy_act + rr_step. RK4 / Euler envs (not RR_INT_DOPRI5). */
int rr_rollout_step(rr_env* e, const float* params, int precision, uint64_t seed, const uint64_t* iter, int t,
                    float gamma, float* buf_obs, float* buf_action, float* buf_value, float* buf_log_prob,
                    float* buf_start, float* buf_reward, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
                    float* terms, void* stream);

/* A whole PPO rollout in ONE launch (replaces SB3 OnPolicyAlgorithm.collect_rollouts +
 * RolloutBuffer.compute_returns_and_advantage, stable_baselines3 1.6 on_policy_algorithm.py /
 * buffers.py, driving the reference's env through main_6DOF.py:60-103). Steps t = 0..n_steps-1
 * are exactly rr_rollout_step(t) — same noise key (seed, env id, *iter, t), same env step,
 * bootstrap and buffer writes, now into the [t] slices of [n_steps][n] buffers — with the env
 * state kept in registers between steps; then last_value[i] = V(post-step obs) (as
 * rr_policy_bootstrap), last_done[i] = last_start[i] = float(done[i]) and, when
 * buf_advantage / buf_return are given, the GAE scan of rr_gae(gamma, gae_lambda) (fp64; the
 * timeout bootstrap uses (float)gamma as rr_rollout_step does). Env outputs
 * (obs, reward, done, truncated, terms) are those of the last step. last_* / obs / truncated /
 * terms may be NULL. Bitwise the same results as n_steps rr_rollout_step launches +
 * rr_policy_bootstrap + rr_gae. RK4 / Euler envs. */
int rr_rollout_collect(rr_env* e, const float* params, int precision, uint64_t seed, const uint64_t* iter,
                       int n_steps, double gamma, double gae_lambda, float* buf_obs, float* buf_action,
                       float* buf_value, float* buf_log_prob, float* buf_start, float* buf_reward,
                       float* buf_advantage, float* buf_return, float* last_value, float* last_done,
                       float* last_start, float* obs, float* reward, uint8_t* done, uint8_t* truncated, float* terms,
                       void* stream);

/* ---- Training-time episode statistics from the collect (ABI 14, added without a version bump: two
 * new symbols and a new struct, nothing existing changes) ----
 * Replaces what SB3 logs from Monitor-wrapped envs every iteration (reference main_6DOF.py:18-24,
 * 62-69: rollout/ep_rew_mean, rollout/ep_len_mean, train/explained_variance).
 * rr_rollout_collect_stats IS rr_rollout_collect (same arguments, same arithmetic in the same order:
 * the rollout buffers, the env outputs and the handle's state are left bit for bit the same) and, in
 * the same launch, accounts for every episode an env finishes in it, whichever step it ends on and
 * however many one env finishes, and for the rollout's samples after the GAE scan. A second launch
 * on the same stream folds the per-wave rows (`partials`) into `out`, 16 slots of 8 bytes:
 *   EPISODES .. NONFINITE  int64: episodes finished, the sum of their lengths (the TimeLimit's
 *                          elapsed count, as rr_copy_terminal's ep_len), and how many landed (the
 *                          rule of RR_EVAL_LANDED), ended on the ground event, by a bounds violation,
 *                          by the TimeLimit, on a non-finite state (an episode can set several)
 *   RET_SUM, RET_SQ        fp64: sum of the episodes' returns (the fp32 running return of
 *                          rr_copy_terminal's ep_return, widened) and of their squares
 *   RET_MIN, RET_MAX       fp64: their extremes, +inf / -inf without an episode. fmin / fmax: a NaN
 *                          return (a non-finite episode) is skipped here and makes the two sums NaN
 *   Y_SUM .. D_SQ          fp64 over the n_steps * n samples: sums of y, y^2, d, d^2 with
 *                          y = buf_return[t][i], d = y - buf_value[t][i] (SB3 explained_variance =
 *                          1 - Var(d) / Var(y))
 *   SAMPLES                int64: n_steps * n
 * Every fold runs in a fixed order (lanes, then waves): no atomics, the same bits on every run.
 * When `accum` is given the call also folds `out` into it (sums add, min / max fold) and never
 * zeroes it: the caller starts a window with zeros and +inf / -inf in RET_MIN / RET_MAX.
 * RR_EINVAL: everything rr_rollout_collect refuses; stats, partials or out NULL; partials not
 * 128-B aligned, out or accum not 8-B aligned; buf_advantage NULL (Y_SUM .. SAMPLES need the scan);
 * a handle without RR_FLAG_EPISODE_STATS (the running return is then not carried across launches: an
 * episode spanning two collects would report a short return) or without RR_FLAG_AUTO_RESET.
 * Two launches, asynchronous on `stream`, capturable in a hipGraph, no allocation. */
enum {
    RR_RSTAT_EPISODES = 0,  /* int64 */
    RR_RSTAT_LEN_SUM,       /* int64 */
    RR_RSTAT_LANDED,        /* int64 */
    RR_RSTAT_END_EVENT,     /* int64 */
    RR_RSTAT_END_BOUNDS,    /* int64 */
    RR_RSTAT_END_TRUNCATED, /* int64 */
    RR_RSTAT_END_NONFINITE, /* int64 */
    RR_RSTAT_RET_SUM,       /* fp64 */
    RR_RSTAT_RET_SQ,        /* fp64 */
    RR_RSTAT_RET_MIN,       /* fp64 */
    RR_RSTAT_RET_MAX,       /* fp64 */
    RR_RSTAT_Y_SUM,         /* fp64 */
    RR_RSTAT_Y_SQ,          /* fp64 */
    RR_RSTAT_D_SUM,         /* fp64 */
    RR_RSTAT_D_SQ,          /* fp64 */
    RR_RSTAT_SAMPLES,       /* int64 */
    RR_RSTAT_SLOTS          /* 16: a block is 128 bytes */
};

typedef struct rr_rollout_stats {
    void* partials;   /* device, 128-B aligned, rr_rollout_stats_rows(n) * 128 bytes of scratch */
    void* out;        /* device [16] x 8 bytes: this collect's totals, RR_RSTAT_* slots */
    void* accum;      /* device [16] x 8 bytes or NULL: running totals, folded into, never zeroed by the call */
} rr_rollout_stats;

/* rows of `partials` for n envs: one per 64 envs, rounded up (<= 0 for n <= 0) */
int64_t rr_rollout_stats_rows(int64_t n);

int rr_rollout_collect_stats(rr_env* e, const float* params, int precision, uint64_t seed, const uint64_t* iter,
                             int n_steps, double gamma, double gae_lambda, float* buf_obs, float* buf_action,
                             float* buf_value, float* buf_log_prob, float* buf_start, float* buf_reward,
                             float* buf_advantage, float* buf_return, float* last_value, float* last_done,
                             float* last_start, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
                             float* terms, const rr_rollout_stats* stats, void* stream);

/* ---- On-device deterministic policy evaluation (ABI 14) ----
 * Replaces stable_baselines3 EvalCallback / evaluate_policy(deterministic=True) on an
 * EpisodeAnalyzer-wrapped env (reference main_6DOF.py:60-103: EvalCallback(eval_env, n_eval_episodes=5,
 * deterministic=True); wrappers.py:189-235: ep_statistic/landing_success, ep_statistic/used_mass,
 * final_errors/<state name>): every env of the handle runs n_episodes whole episodes under the
 * policy's MEAN action in ONE launch. A step is rr_rollout_step's with the noise removed: obs =
 * state * normalizer^-1, the pi tower and action heads of the packed policy (no value tower, no
 * sampling), the env steps with clip(mean, -1, 1), reward, TimeLimit and auto-reset (the reset
 * stream's draw for the env's counter word) as rr_step; the env state, counter word and running
 * return stay in registers between steps and nothing is written per step. Bitwise the episodes
 * rr_rollout_step runs where exp(log_std) * noise is absorbed by the mean (tests/test_gpu_eval.py).
 *   - Episode 0 of env i starts from the handle's CURRENT state (reset first for whole episodes;
 *     its return continues the running Monitor return under RR_FLAG_EPISODE_STATS, else starts at
 *     0, and its used mass counts from the state at the call).
 *   - When env i ends an episode (done or TimeLimit) row [ep][i] of the given planes is written;
 *     after its n_episodes-th it rests at the first state of a fresh episode: elapsed 0, episode
 *     number advanced by n_episodes, running return 0.
 *   - max_steps caps the steps of every env (<= 0: n_episodes * max_episode_steps, which always
 *     suffices); rows of episodes not completed by then are left untouched, episodes[i] counts the
 *     completed ones and the env rests mid-episode, exactly as after that many steps.
 *   - obs (or NULL) receives the post-call observation of every env.
 * The done list of the handle (rr_fetch_done / rr_copy_terminal / rr_get_buffers' done_bits and
 * terminal_*) is NOT touched: it still refers to the last rr_step / rollout launch.
 * RR_EINVAL: a handle without RR_FLAG_AUTO_RESET, RR_INT_DOPRI5, n_episodes < 1, no TimeLimit and
 * max_steps <= 0 (nothing bounds the launch), out or out->episodes NULL, params NULL or not 16-B
 * aligned, a precision that is not RR_POLICY_*. Asynchronous on `stream`, capturable in a hipGraph,
 * ordered for rr_seed like the handle's other launches. */
#define RR_EVAL_EVENT     0x01  /* ended on the ground event (solve_ivp status 1) */
#define RR_EVAL_BOUNDS    0x02  /* bounds violation */
#define RR_EVAL_TRUNCATED 0x04  /* TimeLimit */
#define RR_EVAL_NONFINITE 0x08  /* status -1 */
#define RR_EVAL_LANDED    0x10  /* the terminal step's rew_goal term != 0 (ep_statistic/landing_success) */

typedef struct rr_eval_out {      /* device pointers; planes are [n_episodes][n]; any but `episodes` may be NULL */
    int32_t* episodes;            /* [n] episodes completed by env i (<= n_episodes) */
    float*   ep_return;           /* sum of raw env rewards, fp32, step order */
    int32_t* ep_length;
    uint8_t* flags;               /* RR_EVAL_* */
    float*   used_mass;           /* mass at the episode's first state - mass at its terminal state */
    float*   final_state;         /* [n_episodes][state_dim][n]: the terminal (pre-reset) state, un-normalised */
} rr_eval_out;

int rr_policy_evaluate(rr_env* e, const float* params, int precision, int n_episodes, int64_t max_steps,
                       const rr_eval_out* out, float* obs /* [n][state_dim] or NULL */, void* stream);

/* ---- Recording evaluation: whole episodes of chosen envs (ABI 14, added without a version bump:
 * a new symbol and a new struct, nothing existing changes) ----
 * Replaces the per-episode histories the reference keeps while an EpisodeAnalyzer-wrapped env is
 * evaluated (wrappers.py:189-235: info["rewards_dict"] of every step, ep_history/states, /actions,
 * /vtarg, /rewards and the two 3D trajectory figures, all read from SIM.states / SIM.actions) and
 * the reward terms of rocket_env.py:1016-1034 (rewards_dict), for the envs the caller chooses.
 * rr_policy_evaluate_trace IS rr_policy_evaluate (same arithmetic in the same order, same reset
 * draws, same rr_eval_out rows, same state left in the handle) and additionally, for every env i
 * with slot[i] = s in [0, n_slots) and every step t = 0, 1, ... it takes in episode k < n_episodes:
 *   state [s][k][t + 1][:]  the un-normalised state after the step, BEFORE any reset (SIM.states);
 *                           row 0 is the state the episode starts from (k = 0: the state at the
 *                           call; k > 0: the auto-reset draw)
 *   action[s][k][t][:]      the clipped mean action the env stepped with
 *   terms [s][k][t][:]      the step's reward terms (rr_buffers terms order) followed by its reward
 *   length[k][s]            the steps episode k took in this call, written when it ends; an episode
 *                           cut by max_steps gets its partial count when the launch ends
 * t counts the steps of THIS call (not the TimeLimit's elapsed field: the handle may be
 * mid-episode). Steps at t >= steps are not written but still counted in length, so length > steps
 * marks a clipped record. Rows past an episode's length, rows of episodes never started and every
 * row of a slot no env maps to are left untouched. slot values outside [0, n_slots) (-1 by
 * convention) record nothing; two envs must not share a slot.
 * RR_EINVAL: as rr_policy_evaluate, and trace, trace->slot, trace->state or trace->length NULL,
 * n_slots < 1, steps < 1. Asynchronous, capturable, no allocation. */
typedef struct rr_eval_trace {
    const int32_t* slot;   /* device [n]: trace slot of env i in [0, n_slots), anything else = not recorded */
    int32_t n_slots;       /* K >= 1 */
    int32_t steps;         /* S >= 1: recorded steps per episode (capacity) */
    float* state;          /* [n_slots][n_episodes][steps + 1][state_dim] */
    float* action;         /* [n_slots][n_episodes][steps][action_dim] or NULL */
    float* terms;          /* [n_slots][n_episodes][steps][n_terms + 1] or NULL */
    int32_t* length;       /* [n_episodes][n_slots] */
} rr_eval_trace;

int rr_policy_evaluate_trace(rr_env* e, const float* params, int precision, int n_episodes, int64_t max_steps,
                             const rr_eval_out* out, const rr_eval_trace* trace, float* obs, void* stream);

/* ---- Evaluation under the exact integrator in ONE launch (ABI 14, added without a version bump: a
 * new symbol, nothing existing changes) ----
 * rr_policy_evaluate for RR_INT_DOPRI5 handles: the landing-success and final-error figures of the
 * reference's EvalCallback, computed by the reference's own integrator (scipy RK45 with the brentq
 * ground event, fp64, per env). A step is rr_policy_act's mean action followed by rr_step's exact
 * step: obs = float32(state64 / normalizer) (6DOF; 3DOF: of the float32 state, as rr_step writes it),
 * the pi tower and action heads, clip(mean, -1, 1), the adaptive solve, reward, TimeLimit and
 * auto-reset; the fp64 state, v0, counter word and running return stay in registers between steps.
 * Bitwise the episodes rr_policy_act + rr_step run where exp(log_std) * noise is absorbed by the
 * mean (tests/test_gpu_eval_exact.py), whichever kernel variant rr_step picks for the handle's N.
 * Rows, max_steps, obs, the untouched done list, asynchrony and capture are rr_policy_evaluate's;
 * flags: RR_EVAL_EVENT / RR_EVAL_NONFINITE are solve_ivp's status 1 / -1. The running return is the
 * handle's (rr_step keeps it whatever RR_FLAG_EPISODE_STATS says); the call leaves state64, the
 * float32 state planes, v0, the counter words and the running returns as that many rr_step calls.
 * RR_EINVAL: as rr_policy_evaluate, except that the handle must be an RR_INT_DOPRI5 one (RK4 / Euler
 * handles go to rr_policy_evaluate). */
int rr_policy_evaluate_exact(rr_env* e, const float* params, int precision, int n_episodes, int64_t max_steps,
                             const rr_eval_out* out, float* obs /* [n][state_dim] or NULL */, void* stream);

/* ---- Recording whole episodes in the one-launch exact-mode evaluation (ABI 14, added without a
 * version bump: a new symbol, nothing existing changes) ----
 * What the reference's make_eval_env computes: Monitor(RecordVideo(EpisodeAnalyzer(TimeLimit(env))))
 * under a deterministic policy, stepped by the reference's own integrator, with the EpisodeAnalyzer's
 * histories of the envs the caller chooses. rr_policy_evaluate_exact_trace IS rr_policy_evaluate_exact
 * (same arithmetic in the same order, same reset draws, same rr_eval_out rows, the same state64,
 * float32 planes, v0, counter words and running returns left in the handle) and additionally writes
 * the records of rr_policy_evaluate_trace into the same rr_eval_trace, by the contract stated there
 * (slots, t counted from this call, capacity clipping, partial lengths, untouched rows, 64-bit row
 * indices). In this mode, for step t of episode k of the env with slot s:
 *   state [s][k][t + 1][:]  float32 of the fp64 state after the quaternion renormalisation (3DOF:
 *                           the angle wrap) and before any reset: the values final_state holds for
 *                           the episode's last step; row 0 is float32(state64) at the call (k = 0)
 *                           or the auto-reset draw (k > 0)
 *   action[s][k][t][:]      the clipped mean action the solver stepped with
 *   terms [s][k][t][:]      the float32 reward terms rr_step stores, followed by the reward (with
 *                           RR_FLAG_REWARD_ANNEALING the annealed reward, the terms unchanged)
 * RR_EINVAL: as rr_policy_evaluate_exact (RK4 / Euler handles go to rr_policy_evaluate_trace), and
 * trace, trace->slot, trace->state or trace->length NULL, n_slots < 1, steps < 1. Asynchronous,
 * capturable, no allocation. */
int rr_policy_evaluate_exact_trace(rr_env* e, const float* params, int precision, int n_episodes,
                                   int64_t max_steps, const rr_eval_out* out, const rr_eval_trace* trace,
                                   float* obs, void* stream);

/* RolloutBuffer.compute_returns_and_advantage: rewards / values / starts [T][n] (starts[t]
 * = episode-start flag of step t), last_value / last_done [n] -> advantages, returns [T][n].
 * The backward scan runs in fp64 (gamma, lam doubles since ABI 13) and each stored value is
 * rounded to fp32 once: within half an fp32 ulp of the fp64 scan of the same inputs, where an
 * fp32 scan is ~5e-5 off at |A| ~ 150 (tests/test_gpu_rollout_replay.py). */
int rr_gae(int64_t T, int64_t n, const float* rewards, const float* values, const float* starts,
           const float* last_value, const float* last_done, double gamma, double lam, float* advantages,
           float* returns, void* stream);

/* ---- PPO minibatch gradient (the learner half of configs[4]) ----
 * Replaces the loss + loss.backward() of stable_baselines3 1.6 PPO.train for the MlpPolicy
 * actor-critic the reference trains (PPO("MlpPolicy", env, ..., ent_coef=0.01),
 * main_6DOF.py:62-69; SB3 defaults otherwise): for the minibatch idx[0 .. batch) of a device
 * rollout (obs [*][obs_dim], actions [*][act_dim], old_log_prob, advantages, returns [*]),
 *   A = (adv - mean) / (std + 1e-8) (unbiased std), r = exp(log_prob - old_log_prob),
 *   loss = -mean(min(A r, A clamp(r, 1 - clip_range, 1 + clip_range)))
 *          + ent_coef * -sum(0.5 + 0.5 log(2 pi) + log_std) + vf_coef * mean((returns - V)^2),
 * the gradient of loss with respect to the 13 parameter tensors (params / grads: HOST arrays of
 * device fp32 pointers in rr_policy_pack's order and PyTorch layouts) is WRITTEN to grads (not
 * accumulated). stats (device, 5 floats, or NULL): policy_loss, value_loss, entropy,
 * clip_fraction, approx_kl (SB3's logged quantities). Deterministic (fixed-order sums, no
 * atomics); fp32 MFMA, so the gradients equal PyTorch's autograd ones to fp32 summation-order
 * rounding. Three launches on `stream`, capturable in a graph. Supported (obs_dim, act_dim):
 * (14, 3), (7, 2); batch >= 2. workspace: device, 16-B aligned, rr_ppo_workspace_size bytes. */
int rr_ppo_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes);
int rr_ppo_grad(int obs_dim, int act_dim, const float* const* params, float* const* grads, const float* obs,
                const float* actions, const float* old_log_prob, const float* advantages, const float* returns,
                const int64_t* idx, int64_t batch, float clip_range, float ent_coef, float vf_coef, float* stats,
                void* workspace, int64_t workspace_bytes, void* stream);

/* torch.nn.utils.clip_grad_norm_(max_grad_norm) + one torch.optim.Adam(capturable=True) step
 * (weight_decay 0, no amsgrad / maximize) over n_tensors (<= 16) fp32 device tensors, in two
 * launches: the rest of SB3 PPO.train's minibatch step after rr_ppo_grad. grads are scaled in
 * place by min(1, max_grad_norm / (||grads|| + 1e-6)) (no clip when max_grad_norm <= 0);
 * exp_avg / exp_avg_sq / step are the optimizer's state tensors (optimizer.state[p]: "exp_avg",
 * "exp_avg_sq", and the device float "step", incremented), updated in place with PyTorch's
 * capturable multi-tensor formulas; lr is a DEVICE float, read at run time (a learning-rate
 * schedule can change it between graph replays). Arrays are host arrays of device pointers;
 * numel[] host. workspace: device, rr_clip_adam_workspace_size(sum of numel) bytes. */
int rr_clip_adam_workspace_size(int64_t total_elements, int64_t* bytes);
int rr_clip_adam(int n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_grad_norm,
                 const float* lr, double beta1, double beta2, float eps, void* workspace, int64_t workspace_bytes,
                 void* stream);

/* One whole PPO minibatch step: rr_ppo_grad followed by rr_clip_adam over the same 13 tensors
 * (rr_ppo_grad's order; exp_avg / exp_avg_sq / step as rr_clip_adam's), replacing SB3 1.6
 * PPO.train's loss.backward(), clip_grad_norm_ and optimizer.step() for one minibatch
 * (main_6DOF.py:62-69) without a multi-GPU all_reduce between them. It takes three launches
 * where the two calls take five:
 *   - the gradient finish also sums the squared gradients for the clip;
 *   - the optimizer step also refreshes the packed tower images of the gradient launch;
 *   - with next_idx (next_batch rows, 2 <= next_batch <= batch) the optimizer launch also sums
 *     the NEXT minibatch's advantage statistics.
 * A call with flags & RR_PPO_CHAINED skips the packing / statistics launch and uses what the
 * previous rr_ppo_update on the same workspace left there. That previous call must have been
 * given next_idx = this idx, next_batch = this batch, and nothing else may have written the
 * parameters since. Its batch may be smaller than the previous call's (a short last minibatch):
 * what is handed over sits at workspace offsets that do not depend on batch, on a workspace sized
 * for the largest batch. Without the flag the call packs from the parameters itself (four launches).
 * Arithmetic as the two calls, except that the clip's norm sums the squares in the finish's
 * order. workspace: device, 16-B aligned, rr_ppo_update_workspace_size bytes; lr a device float. */
#define RR_PPO_CHAINED 0x1u
int rr_ppo_update_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes);
int rr_ppo_update(int obs_dim, int act_dim, float* const* params, float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, float* const* step, const float* obs, const float* actions,
                  const float* old_log_prob, const float* advantages, const float* returns, const int64_t* idx,
                  int64_t batch, const int64_t* next_idx, int64_t next_batch, float clip_range, float ent_coef,
                  float vf_coef, float max_grad_norm, const float* lr, double beta1, double beta2, float eps,
                  float* stats, uint32_t flags, void* workspace, int64_t workspace_bytes, void* stream);

/* rr_ppo_update with the options of SB3 1.6's PPO.__init__ that it fixes, and PPO.train's early stop
 * and logging carried on the device: what replaces, per minibatch of PPO.train,
 *   values_pred = old_values + clamp(values - old_values, -clip_range_vf, clip_range_vf)
 *                                                         (clip_range_vf > 0; value_loss uses values_pred),
 *   `if self.normalize_advantage`                         (0: the loss takes advantages[idx] as they are),
 *   `if self.target_kl is not None and approx_kl_div > 1.5 * self.target_kl: continue_training = False;
 *    break`, and with it `if not continue_training: break` of the epoch loop,
 *   the appends to pg_losses / value_losses / entropy_losses / clip_fractions / approx_kl_divs that
 *   train() averages into train/policy_gradient_loss, value_loss, entropy_loss, clip_fraction, approx_kl.
 * Arguments as rr_ppo_update's, plus old_values [*] (the rollout's values, gathered by idx; required
 * with clip_range_vf > 0, else may be NULL), options (host), control (device, RR_PPO_CTL_SLOTS
 * floats, 16-B aligned, or NULL without target_kl and train_stats) and the flag RR_PPO_EPOCH_START
 * (this call is an epoch's first minibatch: the approx_kl mean restarts, the epoch count advances).
 * stats may be NULL.
 *
 * The control block is the caller's: zero it (hipMemsetAsync) before the first minibatch of a
 * train() call. While RR_PPO_CTL_STOP is 0 every call evaluates its minibatch, adds its loss figures
 * to the running sums and counts it (RR_PPO_CTL_EVALS). If its approx_kl > 1.5 target_kl the call
 * applies no optimizer step: parameters, exp_avg, exp_avg_sq and step stay as they were (grads are
 * unspecified), and RR_PPO_CTL_STOP becomes 1. Otherwise it steps and counts the step
 * (RR_PPO_CTL_STEPS). With RR_PPO_CTL_STOP set every call is a no-op for parameters, optimizer
 * state, stats, the workspace and the block itself (its kernels read the word and return), so the
 * rest of a captured epoch, and the epochs after it, cost their launches only. SB3's figures:
 * train/approx_kl = KL_SUM / KL_COUNT (the last, possibly partial, epoch), the others SUM_* / EVALS
 * (train/entropy_loss = -SUM_ENTROPY / EVALS), the epoch train() stopped in = EPOCHS - 1.
 *
 * With clip_range_vf = 0, target_kl = 0 and normalize_advantage = 1 the call computes bitwise what
 * rr_ppo_update computes, chained or not. Four launches (three chained) on `stream`, capturable in a
 * graph; deterministic: every sum in a fixed order, every word of the block with one writer per
 * launch. RR_EINVAL before any launch for what rr_ppo_update refuses and for: NaN or negative
 * clip_range_vf / target_kl, clip_range_vf > 0 without old_values, target_kl > 0 or train_stats
 * without control, unknown flag bits. workspace: rr_ppo_update_opts_workspace_size bytes. */
#define RR_PPO_EPOCH_START 0x2u
enum {
    RR_PPO_CTL_STOP = 0,     /* 1 after the minibatch whose approx_kl passed 1.5 target_kl */
    RR_PPO_CTL_DECIDE,       /* the last evaluated minibatch's decision (the optimizer launch reads it) */
    RR_PPO_CTL_STEPS,        /* optimizer steps applied */
    RR_PPO_CTL_EVALS,        /* minibatches evaluated */
    RR_PPO_CTL_EPOCHS,       /* epochs begun (calls with RR_PPO_EPOCH_START evaluated) */
    RR_PPO_CTL_SUM_POLICY,   /* sums over the evaluated minibatches: policy_loss */
    RR_PPO_CTL_SUM_VALUE,    /* value_loss */
    RR_PPO_CTL_SUM_ENTROPY,  /* entropy */
    RR_PPO_CTL_SUM_CLIP,     /* clip_fraction */
    RR_PPO_CTL_KL_SUM,       /* approx_kl summed over the current epoch's minibatches */
    RR_PPO_CTL_KL_COUNT,     /* and their number */
    RR_PPO_CTL_KL_LAST,      /* the last evaluated minibatch's approx_kl */
    RR_PPO_CTL_SLOTS = 16    /* floats: a block is 64 bytes */
};
typedef struct rr_ppo_options {
    float clip_range_vf;          /* 0: no value clip (negative or NaN is refused) */
    float target_kl;              /* 0: no KL stop */
    int32_t normalize_advantage;  /* SB3's default: 1 */
    int32_t train_stats;          /* 1: the caller reads the running sums (needs control) */
} rr_ppo_options;
int rr_ppo_update_opts_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes);
int rr_ppo_update_opts(int obs_dim, int act_dim, float* const* params, float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, float* const* step, const float* obs, const float* actions,
                       const float* old_log_prob, const float* advantages, const float* returns,
                       const float* old_values, const int64_t* idx, int64_t batch, const int64_t* next_idx,
                       int64_t next_batch, float clip_range, float ent_coef, float vf_coef, float max_grad_norm,
                       const float* lr, double beta1, double beta2, float eps, const rr_ppo_options* options,
                       float* control, float* stats, uint32_t flags, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* One behaviour-cloning minibatch step on demonstrations obs [M][obs_dim], actions [M][act_dim]
 * (fp32, device), rows idx[0 .. batch): what imitation's bc.BC does per minibatch for SB3's
 * MlpPolicy with a diagonal Gaussian, loss.backward() and Adam's step, without gradient clipping:
 *   logp_i  = sum_a (-(actions_ia - mean_ia)^2 / (2 std_a^2) - log_std_a - 0.5 log 2 pi)
 *   neglogp = -mean_i logp_i,   entropy = sum_a (0.5 + 0.5 log 2 pi + log_std_a)
 *   l2_norm = 0.5 * sum over all 13 tensors of sum(w^2)
 *   loss    = neglogp - ent_weight entropy + l2_weight l2_norm,   prob_true_act = mean_i exp(logp_i)
 * The value tower and head receive the gradient l2_weight w only (zeros at l2_weight 0, written, and
 * all 13 step tensors advance, as torch.optim.Adam does). Arrays, pointer conventions and the tensor
 * order are rr_ppo_update's; stats is a device block of RR_BC_STAT_SLOTS floats or NULL.
 * A call packs the pi tower's image, computes the gradient, finishes and runs Adam, which also
 * refreshes the packed images: four launches. With flags & RR_BC_CHAINED the packing launch is
 * skipped and the image the previous rr_bc_update left in the same workspace is used (nothing else
 * may have written the parameters since; the batch may be smaller than the previous call's, on a
 * workspace sized for the largest). Capturable in a graph; deterministic (fixed-order sums, no
 * atomics); lr is a device float. RR_EINVAL before any launch for unsupported dimensions,
 * batch < 2, a null argument or tensor, a workspace too small or not 16-B aligned, NaN or negative
 * ent_weight / l2_weight, unknown flag bits. workspace: rr_bc_update_workspace_size bytes. */
#define RR_BC_CHAINED 0x1u
enum {
    RR_BC_STAT_NEGLOGP = 0,
    RR_BC_STAT_ENTROPY,
    RR_BC_STAT_ENT_LOSS,       /* -ent_weight entropy */
    RR_BC_STAT_PROB_TRUE_ACT,
    RR_BC_STAT_L2_NORM,
    RR_BC_STAT_L2_LOSS,        /* l2_weight l2_norm */
    RR_BC_STAT_LOSS,
    RR_BC_STAT_SLOTS = 8       /* floats */
};
int rr_bc_update_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes);
int rr_bc_update(int obs_dim, int act_dim, float* const* params, float* const* grads, float* const* exp_avg,
                 float* const* exp_avg_sq, float* const* step, const float* obs, const float* actions,
                 const int64_t* idx, int64_t batch, float ent_weight, float l2_weight, const float* lr,
                 double beta1, double beta2, float eps, float* stats, uint32_t flags,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* One A2C update on a device rollout, rows idx[0 .. batch): stable_baselines3 A2C.train() for the
 * MlpPolicy actor-critic with a diagonal Gaussian, loss.backward(), clip_grad_norm_ and the optimizer's
 * step:
 *   A    = advantages[idx], or with normalize_advantage != 0 (A - mean(A)) / (std(A) + 1e-8)
 *   policy_loss = -mean(A log_prob(actions)),   value_loss = mean((returns - V)^2)
 *   entropy     = sum_a (0.5 + 0.5 log 2 pi + log_std_a)
 *   loss        = policy_loss - ent_coef entropy + vf_coef value_loss
 * There is no probability ratio: the rollout's stored log-probs are not an argument. Arrays, pointer
 * conventions and the 13 tensors' order are rr_ppo_update's. `optimizer` chooses the step, on the
 * optimizer's own state tensors:
 *   RR_A2C_RMSPROP     torch.optim.RMSprop      sq = alpha sq + (1 - alpha) g g; p -= lr g / (sqrt(sq) + eps)
 *   RR_A2C_RMSPROP_TF  SB3's RMSpropTFLike      the same sq;                    p -= lr g / sqrt(sq + eps)
 *   RR_A2C_ADAM        torch.optim.Adam(capturable=True), rr_ppo_update's step (use_rms_prop=False)
 * square_avg holds RMSprop's square_avg tensors or Adam's exp_avg_sq; exp_avg is Adam's and NULL
 * otherwise; alpha_or_beta1 is RMSprop's alpha or Adam's beta1, beta2 is Adam's only. No momentum, not
 * centered, no weight decay. max_grad_norm 0 is no clip; the clipped gradients are left in grads, and
 * every step tensor (a device float each) counts the call. lr is a device float.
 * stats is a device block of RR_A2C_STAT_SLOTS floats or NULL: [policy_loss, value_loss, entropy, loss,
 * mean log_prob, 0, 0, 0]. One call is four launches (advantage sums and packing, gradient, finish,
 * optimizer). Capturable in a graph; deterministic (fixed-order sums, no atomics). RR_EINVAL before any
 * launch for unsupported dimensions, batch < 2, a null argument or tensor, an unknown optimizer, NaN,
 * infinite or negative ent_coef / vf_coef / max_grad_norm / eps, alpha_or_beta1 or beta2 outside [0, 1),
 * a workspace too small or not 16-B aligned. workspace: rr_a2c_update_workspace_size bytes. */
enum { RR_A2C_RMSPROP = 0, RR_A2C_RMSPROP_TF = 1, RR_A2C_ADAM = 2 };
enum {
    RR_A2C_STAT_POLICY_LOSS = 0,
    RR_A2C_STAT_VALUE_LOSS,
    RR_A2C_STAT_ENTROPY,
    RR_A2C_STAT_LOSS,
    RR_A2C_STAT_LOG_PROB,      /* mean log_prob(actions) */
    RR_A2C_STAT_SLOTS = 8      /* floats */
};
int rr_a2c_update_workspace_size(int obs_dim, int act_dim, int64_t batch, int64_t* bytes);
int rr_a2c_update(int obs_dim, int act_dim, float* const* params, float* const* grads, float* const* square_avg,
                  float* const* exp_avg, float* const* step, const float* obs, const float* actions,
                  const float* advantages, const float* returns, const int64_t* idx, int64_t batch,
                  int normalize_advantage, float ent_coef, float vf_coef, float max_grad_norm, int optimizer,
                  const float* lr, double alpha_or_beta1, double beta2, float eps, float* stats,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* ---- Discrete 3DOF actions: the Categorical policy --------------------------------------------------
 * The reference's DiscreteActions3DOF (wrappers.py:24-35) turns the 3DOF env's [gimbal, thrust]
 * action into Discrete(K) through a table of K rows; behind it SB3 builds an MlpPolicy with the same
 * 64x64 towers, an action head of K logits and no log_std (stable_baselines3
 * CategoricalDistribution: log_prob = logit_a - logsumexp(logits), entropy = -sum_k p_k log p_k,
 * mode = argmax). obs_dim is 7, n_choices K is 2 .. 4. The policy has 12 tensors, rr_policy_pack's
 * order without log_std: pi {W1, b1, W2, b2}, vf {W1, b1, W2, b2}, W_action [K][64], b_action [K],
 * W_value [1][64], b_value. Kernels and packed images are those of a 4-head policy (the <7, 4>
 * instantiation of the layouts); heads k >= K are packed as zeros, stay out of the softmax and
 * receive no gradient. fp32 towers only.
 *
 * Packing: _discrete twins of rr_policy_layout / rr_policy_pack, because the source list has 12
 * tensors and the head tensors K rows; rr_policy_layout / rr_policy_pack and their instantiations are
 * untouched. rr_policy_layout_discrete returns the size in floats and the same 12 offsets (LS is
 * four unused floats). rr_policy_bootstrap is reused: it accepts (obs_dim, act_dim) = (7, 4) with
 * RR_POLICY_FP32 for an image packed by rr_policy_pack_discrete. */
int rr_policy_layout_discrete(int obs_dim, int64_t* off);
int rr_policy_pack_discrete(int obs_dim, int n_choices, const float* const* src, float* params, void* stream);

/* rr_policy_act for this policy, one launch: value [n] and, per env i,
 *   z_k = logit k (k < K), m = max z, p_k = exp(z_k - m) / sum, log p_k = (z_k - m) - log(sum)
 *   u = (mix32(key) >> 8) 2^-24 in [0, 1), key being rr_policy_act's three mix32 rounds over
 *       (env_id_offset + i, splitmix64(seed), *iter, t)
 *   index = the number of k in 0 .. K - 2 with p_0 + .. + p_k <= u (fp32 running sum): inverse-CDF
 *           sampling, always in 0 .. K - 1
 *   action [n] = index as a float (SB3's [n_steps, n_envs, 1] buffer), log_prob [n] = log p_index,
 *   action_env [n][2] = table[index] (the rr_step input).
 * table is a HOST array [n_choices][2] of finite floats, copied into the launch. The other arguments,
 * the previous step's bootstrap (reward_out) and the episode-start flags (start_out) are
 * rr_policy_act's. RR_EINVAL before any launch for obs_dim != 7, n_choices outside 2 .. 4, a
 * precision other than RR_POLICY_FP32, a non-finite table entry and what rr_policy_act refuses. */
int rr_policy_act_discrete(const float* params, int obs_dim, int n_choices, const float* table, int precision,
                           int64_t n, int64_t env_id_offset, const float* obs, uint64_t seed, const uint64_t* iter,
                           int t, float* action_env, float* action, float* value, float* log_prob, float* obs_copy,
                           const float* prev_term_obs, const uint8_t* prev_truncated, const float* prev_reward,
                           float gamma, float* reward_out, const uint8_t* done, float* start_out, void* stream);

/* rr_ppo_update for this policy: SB3 1.6 PPO.train's minibatch step with a Categorical distribution.
 * Arguments are rr_ppo_update's with n_choices for act_dim; the five tensor lists have 12 entries
 * (the order above); actions is [rows], the chosen index as a float. The loss is rr_ppo_grad's with
 *   log_prob = log p_a,   entropy = mean_i H_i,  H = -sum_k p_k log p_k (0 for a term whose p_k is 0)
 * so the entropy bonus is state dependent and its gradient is part of each sample's logit gradient
 *   d loss / d z_k = dlp ((k == a) - p_k) + ent_coef / B p_k (log p_k + H).
 * stats[5] as rr_ppo_grad's, stats[2] the mean entropy. RR_PPO_CHAINED, next_idx, the workspace rules,
 * the clip and Adam arithmetic are rr_ppo_update's: four launches, three chained; capturable;
 * deterministic (fixed-order sums, no atomics). RR_EINVAL before any launch for obs_dim != 7,
 * n_choices outside 2 .. 4, batch < 2 and what rr_ppo_update refuses.
 * workspace: rr_ppo_update_discrete_workspace_size bytes. */
int rr_ppo_update_discrete_workspace_size(int obs_dim, int n_choices, int64_t batch, int64_t* bytes);
int rr_ppo_update_discrete(int obs_dim, int n_choices, float* const* params, float* const* grads,
                           float* const* exp_avg, float* const* exp_avg_sq, float* const* step, const float* obs,
                           const float* actions, const float* old_log_prob, const float* advantages,
                           const float* returns, const int64_t* idx, int64_t batch, const int64_t* next_idx,
                           int64_t next_batch, float clip_range, float ent_coef, float vf_coef, float max_grad_norm,
                           const float* lr, double beta1, double beta2, float eps, float* stats, uint32_t flags,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* rr_ppo_update_opts for this policy: rr_ppo_update_discrete with SB3's clip_range_vf,
 * normalize_advantage and target_kl, and PPO.train's early stop and logging carried on the device.
 * Arguments are rr_ppo_update_discrete's, plus rr_ppo_update_opts's in its places: old_values [*]
 * after returns (the rollout's values, gathered by idx; required with clip_range_vf > 0, else may be
 * NULL), options (host) and control (device, RR_PPO_CTL_SLOTS floats, 16-B aligned, or NULL without
 * target_kl and train_stats) ahead of stats, and the flag RR_PPO_EPOCH_START. stats may be NULL.
 * The loss is rr_ppo_update_discrete's (log_prob = log p_a, the state-dependent entropy with its
 * gradient in each sample's logit gradient) with rr_ppo_update_opts's three replacements: the value
 * clip on the vf tower, raw advantages[idx] with normalize_advantage 0, and the stop at
 * approx_kl > 1.5 target_kl. The control block is the caller's and means what it means there:
 * RR_PPO_CTL_SUM_ENTROPY sums the minibatches' mean entropies (stats[2]), a stopping minibatch takes
 * no optimizer step and sets RR_PPO_CTL_STOP, and with RR_PPO_CTL_STOP set every call is a no-op for
 * parameters, optimizer state, stats, the workspace and the block itself (each kernel reads the word
 * at entry and returns).
 *
 * With clip_range_vf = 0, target_kl = 0 and normalize_advantage = 1 the call computes bitwise what
 * rr_ppo_update_discrete computes, chained or not, with or without a control block. Four launches
 * (three chained) on `stream`, capturable in a graph; deterministic: every sum in a fixed order,
 * every word of the block with one writer per launch. RR_EINVAL before any launch for what
 * rr_ppo_update_discrete refuses and for: NaN or negative clip_range_vf / target_kl,
 * clip_range_vf > 0 without old_values, target_kl > 0 or train_stats without control, a control
 * pointer that is not 16-B aligned, unknown flag bits, NULL options.
 * workspace: rr_ppo_update_discrete_opts_workspace_size bytes. */
int rr_ppo_update_discrete_opts_workspace_size(int obs_dim, int n_choices, int64_t batch, int64_t* bytes);
int rr_ppo_update_discrete_opts(int obs_dim, int n_choices, float* const* params, float* const* grads,
                                float* const* exp_avg, float* const* exp_avg_sq, float* const* step, const float* obs,
                                const float* actions, const float* old_log_prob, const float* advantages,
                                const float* returns, const float* old_values, const int64_t* idx, int64_t batch,
                                const int64_t* next_idx, int64_t next_batch, float clip_range, float ent_coef,
                                float vf_coef, float max_grad_norm, const float* lr, double beta1, double beta2,
                                float eps, const rr_ppo_options* options, float* control, float* stats, uint32_t flags,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* rr_bc_update for this policy: one behaviour-cloning minibatch step on demonstrations obs [M][7] and
 * actions [M], the demonstrated index as a float (what rr_policy_act_discrete writes and what the
 * reference's RecordTrajectoryCallback records behind DiscreteActions3DOF), rows idx[0 .. batch):
 * imitation's BehaviorCloningLossCalculator on SB3's CategoricalDistribution, loss.backward() and Adam's
 * step, without gradient clipping:
 *   log p_ik = z_ik - logsumexp_k z_ik,   logp_i = log p_{i, a_i}
 *   H_i      = -sum_k p_ik log p_ik       (0 for a term whose p_ik is 0)
 *   neglogp  = -mean_i logp_i,   entropy = mean_i H_i,   prob_true_act = mean_i exp(logp_i)
 *   l2_norm  = 0.5 * sum over all 12 tensors of sum(w^2)
 *   loss     = neglogp - ent_weight entropy + l2_weight l2_norm
 *   d loss / d z_ik = -(1 / B) ((k == a_i) - p_ik) + ent_weight / B p_ik (log p_ik + H_i)
 * The value tower and head receive the gradient l2_weight w only (zeros at l2_weight 0, written), and all
 * 12 step tensors advance. The five tensor lists have 12 entries, in rr_ppo_update_discrete's order;
 * stats is a device block of RR_BC_STAT_SLOTS floats (the slots above) or NULL. Four launches, three with
 * flags & RR_BC_CHAINED (rr_bc_update's rule: the previous rr_bc_update_discrete on the same workspace
 * was the last writer of the parameters). Capturable in a graph; deterministic (fixed-order sums, no
 * atomics); lr is a device float.
 * actions MUST hold integers in [0, n_choices): the call cannot check device data. It guarantees only
 * that no address depends on them (an index is compared against k, never used as an offset); a row whose
 * value names no choice contributes log p = 0 and a gradient that clones nothing.
 * RR_EINVAL before any launch for obs_dim != 7, n_choices outside 2 .. 4, batch < 2, a null argument or
 * tensor, a workspace too small or not 16-B aligned, NaN or negative ent_weight / l2_weight, unknown flag
 * bits. workspace: rr_bc_update_discrete_workspace_size bytes. */
int rr_bc_update_discrete_workspace_size(int obs_dim, int n_choices, int64_t batch, int64_t* bytes);
int rr_bc_update_discrete(int obs_dim, int n_choices, float* const* params, float* const* grads,
                          float* const* exp_avg, float* const* exp_avg_sq, float* const* step, const float* obs,
                          const float* actions, const int64_t* idx, int64_t batch, float ent_weight, float l2_weight,
                          const float* lr, double beta1, double beta2, float eps, float* stats, uint32_t flags,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* One A2C update of this policy (a pure addition to ABI 14), rr_a2c_update for the Categorical policy: rows
 * idx[0 .. batch) of a device rollout whose actions are [M], the chosen index as a float (what
 * rr_policy_act_discrete and the one-launch collect write); stable_baselines3 A2C.train() behind a
 * CategoricalDistribution, loss.backward(), clip_grad_norm_ and the optimizer's step:
 *   A    = advantages[idx], or with normalize_advantage != 0 (A - mean(A)) / (std(A) + 1e-8)
 *   lp_i = z_{i, a_i} - logsumexp_k z_ik          over the first n_choices logits
 *   H_i  = -sum_k p_ik log p_ik                   (0 for a term whose p_ik is 0)
 *   policy_loss = -mean(A lp),   value_loss = mean((returns - V)^2),   entropy = mean(H)
 *   loss        = policy_loss - ent_coef entropy + vf_coef value_loss
 *   d loss / d z_ik = -(A_i / B) ((k == a_i) - p_ik) + ent_coef / B p_ik (log p_ik + H_i),  0 for k >= n_choices
 * There is no probability ratio: the rollout's stored log-probs are not an argument. The five tensor lists
 * have 12 entries, in rr_ppo_update_discrete's order; `optimizer`, square_avg, exp_avg (NULL unless
 * RR_A2C_ADAM), step, alpha_or_beta1, beta2, eps, max_grad_norm (0: no clip) and lr (a device float) are
 * rr_a2c_update's, and all 12 step tensors count the call. stats is a device block of RR_A2C_STAT_SLOTS
 * floats or NULL: [policy_loss, value_loss, mean H, loss, mean lp, 0, 0, 0] (the RR_A2C_STAT_* slots).
 * One call is four launches (advantage sums and packing, gradient, finish, optimizer). Capturable in a
 * graph; deterministic (fixed-order sums, no atomics). The workspace holds the call's intermediates and a
 * sink of [4][64] + [4] floats for the heads >= n_choices; no state is read from it: its contents before
 * the call do not matter.
 * actions MUST hold integers in [0, n_choices): the call cannot check device data. It guarantees only
 * that no address depends on them (an index is compared against k, never used as an offset).
 * RR_EINVAL before any launch for obs_dim != 7, n_choices outside 2 .. 4, batch < 2, a null argument or
 * tensor, an unknown optimizer, NaN, infinite or negative ent_coef / vf_coef / max_grad_norm / eps,
 * alpha_or_beta1 or beta2 outside [0, 1), a workspace too small or not 16-B aligned. workspace:
 * rr_a2c_update_discrete_workspace_size bytes. */
int rr_a2c_update_discrete_workspace_size(int obs_dim, int n_choices, int64_t batch, int64_t* bytes);
int rr_a2c_update_discrete(int obs_dim, int n_choices, float* const* params, float* const* grads,
                           float* const* square_avg, float* const* exp_avg, float* const* step, const float* obs,
                           const float* actions, const float* advantages, const float* returns, const int64_t* idx,
                           int64_t batch, int normalize_advantage, float ent_coef, float vf_coef, float max_grad_norm,
                           int optimizer, const float* lr, double alpha_or_beta1, double beta2, float eps,
                           float* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* The one-launch collect, its per-step form and the one-launch evaluation for this policy (pure
 * additions to ABI 14: a caller that needs them looks the symbols up). The handle is a 3DOF one with
 * an RK4 or Euler integrator, params an image of rr_policy_pack_discrete (16-B aligned), precision
 * RR_POLICY_FP32, n_choices K in 2 .. 4 and table a HOST array [K][2] of finite floats, copied into the
 * launch (rows past K are not read), as for rr_policy_act_discrete.
 *
 * rr_rollout_step_discrete / rr_rollout_collect_discrete are rr_rollout_step / rr_rollout_collect with
 * the sample of rr_policy_act_discrete in place of the Gaussian one: the same key, one uniform draw,
 * the inverse-CDF index; buf_action is [n] / [n_steps][n], ONE float per sample holding the index,
 * buf_log_prob is log p_index and the env steps with table[index]. Everything else (env step, reward
 * terms, TimeLimit, the timeout bootstrap, terminal rows, auto-reset, V(last obs), the fp64 GAE scan,
 * the optional arguments, asynchrony and capture) is rr_rollout_step's / rr_rollout_collect's. Bitwise
 * the rollout of n_steps x (rr_policy_act_discrete + rr_step) + rr_policy_bootstrap(7, 4) + rr_gae
 * (tests/test_gpu_rollout_discrete.py).
 *
 * rr_policy_evaluate_discrete is rr_policy_evaluate with the action table[argmax_k<K z_k], the lowest
 * index on a tie (SB3's deterministic prediction behind DiscreteActions3DOF); rows, max_steps, obs,
 * asynchrony and capture are rr_policy_evaluate's.
 *
 * RR_EINVAL before any HIP call, with a message that starts with the function's name: a NULL handle
 * or required buffer, a 6DOF handle, an RR_INT_DOPRI5 handle, a precision other than RR_POLICY_FP32,
 * n_choices outside 2 .. 4, a NULL table or a non-finite entry in its first n_choices rows, params not
 * 16-B aligned, and what rr_rollout_collect (n_steps <= 0, buf_advantage without buf_return) /
 * rr_policy_evaluate (no RR_FLAG_AUTO_RESET, n_episodes < 1, no TimeLimit with max_steps 0, out or
 * out->episodes NULL) refuse. */
int rr_rollout_step_discrete(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                             uint64_t seed, const uint64_t* iter, int t, float gamma, float* buf_obs,
                             float* buf_action, float* buf_value, float* buf_log_prob, float* buf_start,
                             float* buf_reward, float* obs, float* reward, uint8_t* done, uint8_t* truncated,
                             float* terms, void* stream);
int rr_rollout_collect_discrete(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                uint64_t seed, const uint64_t* iter, int n_steps, double gamma, double gae_lambda,
                                float* buf_obs, float* buf_action, float* buf_value, float* buf_log_prob,
                                float* buf_start, float* buf_reward, float* buf_advantage, float* buf_return,
                                float* last_value, float* last_done, float* last_start, float* obs, float* reward,
                                uint8_t* done, uint8_t* truncated, float* terms, void* stream);
int rr_policy_evaluate_discrete(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                int n_episodes, int64_t max_steps, const rr_eval_out* out, float* obs, void* stream);

/* The same two one-launch calls with the collect statistics and with recorded episodes (pure additions
 * to ABI 14). Handle, params, n_choices, table and precision are as above.
 *
 * rr_rollout_collect_discrete_stats is rr_rollout_collect_discrete that also fills `stats` as
 * rr_rollout_collect_stats does: the same slots, the same rows of partials (rr_rollout_stats_rows), the
 * same fixed-order reduction launched after it on the same stream, `accum` folded when given. The
 * rollout buffers, env outputs and the handle's state are bitwise rr_rollout_collect_discrete's
 * (tests/test_gpu_collect_stats_discrete.py). RR_EINVAL before any HIP call for what
 * rr_rollout_collect_discrete refuses and for what rr_rollout_collect_stats refuses: stats,
 * stats->partials or stats->out NULL, partials not 128-B aligned, out / accum not 8-B aligned,
 * buf_advantage or buf_return NULL, a handle without RR_FLAG_EPISODE_STATS or RR_FLAG_AUTO_RESET. The
 * argument checks come before the handle is read.
 *
 * rr_policy_evaluate_discrete_trace is rr_policy_evaluate_discrete that also records the envs with a
 * trace slot as rr_policy_evaluate_trace does (rr_eval_trace is unchanged: state rows, action rows,
 * terms, length; the recorded action row is the table row the env stepped with). choice, device memory
 * [n_slots][n_episodes][steps] int32 or NULL, receives the index of that row, k in [0, n_choices),
 * written where the action row is written (t < steps; rows past an episode's length are not touched).
 * Outputs, the state left and obs are bitwise rr_policy_evaluate_discrete's
 * (tests/test_gpu_eval_trace_discrete.py). RR_EINVAL before any HIP call for what
 * rr_policy_evaluate_discrete refuses and for what rr_policy_evaluate_trace refuses: trace,
 * trace->slot, trace->state or trace->length NULL, trace->n_slots or trace->steps below 1; and for a
 * choice that is not 4-B aligned. */
int rr_rollout_collect_discrete_stats(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                      uint64_t seed, const uint64_t* iter, int n_steps, double gamma,
                                      double gae_lambda, float* buf_obs, float* buf_action, float* buf_value,
                                      float* buf_log_prob, float* buf_start, float* buf_reward, float* buf_advantage,
                                      float* buf_return, float* last_value, float* last_done, float* last_start,
                                      float* obs, float* reward, uint8_t* done, uint8_t* truncated, float* terms,
                                      const rr_rollout_stats* stats, void* stream);
int rr_policy_evaluate_discrete_trace(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                      int n_episodes, int64_t max_steps, const rr_eval_out* out,
                                      const rr_eval_trace* trace, int32_t* choice, float* obs, void* stream);

/* ---- The Categorical policy's evaluation under the exact integrator in ONE launch (a pure addition
 * to ABI 14: a new symbol, nothing existing changes) ----
 * The reference's sensitivity_test.py set-up: evaluate_policy on
 * TimeLimit(DiscreteActions3DOF(RewardAnnealing(Rocket))), a deterministic Discrete(K) policy stepped by
 * the reference's own integrator (scipy RK45 with the brentq ground event). The argument list is
 * rr_policy_evaluate_discrete's, the semantics are rr_policy_evaluate_exact's: a step is
 * obs = float32(float32(state64) / normalizer), the pi tower and its logits, the action
 * table[argmax_k<K z_k] (the lowest index on a tie, NOT clipped), the adaptive solve, reward (with
 * RR_FLAG_REWARD_ANNEALING the annealed one, its thrust the table row's), TimeLimit and auto-reset; the
 * fp64 state, v0, counter word and running return stay in registers between steps. Where the softmax is
 * saturated so that the sampled index is the argmax, the call writes bitwise the episodes
 * rr_policy_act_discrete + rr_step run (tests/test_gpu_eval_exact_discrete.py), and it leaves state64,
 * the float32 state planes, v0, the counter words and the running returns as that many rr_step calls.
 * Rows, flags, max_steps, obs, the untouched done list are rr_policy_evaluate_exact's. Asynchronous,
 * capturable, no allocation.
 * RR_EINVAL before any HIP call, with a message that starts with the function's name: everything
 * rr_policy_evaluate_discrete refuses (a NULL handle / params / out / out->episodes, a 6DOF handle, a
 * precision other than RR_POLICY_FP32, n_choices outside 2 .. 4, a NULL table or a non-finite entry in
 * its first n_choices rows, params not 16-B aligned, no RR_FLAG_AUTO_RESET, n_episodes < 1, no TimeLimit
 * with max_steps 0), except that the handle must be an RR_INT_DOPRI5 one (RK4 / Euler handles go to
 * rr_policy_evaluate_discrete). The argument checks come before the handle is read. */
int rr_policy_evaluate_exact_discrete(rr_env* e, const float* params, int n_choices, const float* table,
                                      int precision, int n_episodes, int64_t max_steps, const rr_eval_out* out,
                                      float* obs, void* stream);

/* ---- Sampled-action evaluation in ONE launch (pure additions to ABI 14: two new symbols, nothing
 * existing changes) ----
 * Replaces stable_baselines3 evaluate_policy(model, env, deterministic=False): whole episodes of the
 * STOCHASTIC policy, the one PPO optimises, for every env of the handle at once.
 * rr_policy_evaluate_sampled is rr_policy_evaluate (trace NULL) or rr_policy_evaluate_trace (trace given),
 * and rr_policy_evaluate_discrete_sampled is rr_policy_evaluate_discrete or
 * rr_policy_evaluate_discrete_trace, in every respect but the action: the rr_eval_out rows, the max_steps
 * rule, the state the handle is left in, the untouched done list, the trace layout with its t < steps
 * rule, obs, asynchrony, capture, no allocation.
 * The action of step k of the call (k = 0, 1, ...: the loop index, whatever the env's elapsed field is)
 * is the one rr_rollout_step(..., seed, iter, t = k, ...) / rr_rollout_step_discrete draws: the key from
 * splitmix64(seed), the env's global id (env_id_offset + i), *iter (read once at kernel entry) and t = k;
 *   Gaussian:     act = mean + exp(log_std) * eps (Box-Muller), the env steps with clip(act, -1, 1);
 *   Categorical:  softmax over the first n_choices of the four logits, u = (mix32(key) >> 8) * 2^-24, the
 *                 inverse-CDF index, the env steps with table[index] (not clipped).
 * No value tower and no log-prob. An env's draws depend on nothing but its own global id, so shards with
 * env_id_offset draw what the unsharded handle draws; an env that has finished n_episodes draws nothing
 * any more (its column of the MFMAs is computed and dropped). An episode is therefore bit for bit the one
 * rr_rollout_step / rr_rollout_step_discrete runs with the same (seed, *iter) and t counted from the call
 * (tests/test_gpu_eval_sampled.py). The caller advances *iter between calls (as between collects) for
 * fresh noise.
 * Recorded (trace given): action[s][k][t][:] is the CLIPPED sample the env stepped with (the unclipped
 * sample is not recorded), for the Categorical call the table row; choice (or NULL; needs trace) receives
 * the sampled index.
 * RR_EINVAL before any launch: everything the deterministic twin refuses (RR_INT_DOPRI5 handles, for the
 * Categorical call a 6DOF handle and a precision other than RR_POLICY_FP32, ...), iter NULL, an effective
 * max_steps (given, or n_episodes * max_episode_steps) above 2^31 - 1 (t is an int in rr_rollout_step),
 * choice given without trace. */
int rr_policy_evaluate_sampled(rr_env* e, const float* params, int precision, uint64_t seed, const uint64_t* iter,
                               int n_episodes, int64_t max_steps, const rr_eval_out* out,
                               const rr_eval_trace* trace /* or NULL */, float* obs, void* stream);
int rr_policy_evaluate_discrete_sampled(rr_env* e, const float* params, int n_choices, const float* table, int precision,
                                        uint64_t seed, const uint64_t* iter, int n_episodes, int64_t max_steps,
                                        const rr_eval_out* out, const rr_eval_trace* trace /* or NULL */,
                                        int32_t* choice /* or NULL; needs trace */, float* obs, void* stream);

#ifdef __cplusplus
}
#endif
#endif
