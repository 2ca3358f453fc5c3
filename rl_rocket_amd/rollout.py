"""On-device PPO rollouts: policy inference, env step and rollout buffer all in HBM.

SURVEY.md §8(f) rank 2 / BASELINE.json configs[4]: stock SB3 1.6 copies every observation
batch to a NumPy ``RolloutBuffer`` on the host; here the PyTorch policy consumes the obs
tensor the step kernel wrote, the sampled actions go straight back into ``rr_step``, and
the buffer, GAE and the PPO update stay on the GPU. One ``collect`` (n_steps × [policy
forward + sample + env step + buffer writes]) can be captured into a hipGraph.

Actions are clipped to the Box [-1, 1] before the env step, as SB3 does.
Timeouts are bootstrapped like SB3 1.6 ``collect_rollouts``:
reward += gamma * V(terminal_obs) where TimeLimit truncated the episode.

This module holds the collector, ``DeviceRollout``, and is the import surface of what works on its
buffers: the policy and its packer (``policy.py``), the PPO learner (``learner.py``), the evaluator
(``evaluate.py``), behaviour cloning (``bc.py``) and A2C (``a2c.py``, ``a2c_discrete.py``) are re-exported below, the same objects.
"""
import torch

from .a2c import A2CUpdate, GraphedA2C, RMSpropTFLike, a2c_update  # noqa: F401
from .a2c_discrete import A2CUpdateDiscrete, GraphedA2CDiscrete, a2c_update_discrete  # noqa: F401
from .bc import BCUpdate, Demonstrations, bc_train  # noqa: F401
from .evaluate import (EVAL_BOUNDS, EVAL_EVENT, EVAL_LANDED, EVAL_NONFINITE, EVAL_TRUNCATED,  # noqa: F401
                       EpisodeRecord, EvalResult, EvalTrace, PolicyEvaluator, evaluate_policy)
from .learner import (ClipAdam, GraphedPPOUpdate, PPOGrad, PPOUpdate, PPOUpdateDiscrete,  # noqa: F401
                      _allreduce_grads, _epoch_perms, _old_values, _ppo_options, _train_stats, clip_adam_supported,
                      ppo_update)
from .policy import (DISCRETE_TABLE_3DOF, FOLD_C, POLICY_PRECISIONS, MlpActorCritic,  # noqa: F401
                     MlpCategoricalActorCritic, PolicyPack, _Linear, _LinearFn, _policy_tensors, _rowsum,
                     fused_discrete_supported, fused_grad_supported)


class DeviceRollout:
    """Collects ``n_steps`` transitions from a ``RocketBatch`` (auto-reset, TimeLimit)
    into device tensors [n_steps, N, ...] and computes GAE on device.

    ``fused=True`` (default for an ``MlpActorCritic`` with 64x64 towers): per step one
    fp32-MFMA HIP launch for policy forward + sampling + buffer writes (``rr_policy_act``),
    the fused env step, one launch for the timeout bootstrap (``rr_policy_bootstrap``);
    GAE in one launch (``rr_gae``). ``fused=False``: the same algorithm in PyTorch ops.
    ``one_launch=True`` (default where possible: fused, RK4 / Euler env) collapses the whole
    ``collect`` to ONE launch (``rr_rollout_collect``: every env runs policy, sample, env step,
    bootstrap and buffer writes for all ``n_steps`` with its state in registers, then V(last
    obs) and its GAE scan); ``per_step=True`` keeps one launch per step (``rr_rollout_step``)
    + bootstrap + GAE launches. All three paths produce bitwise the same rollout.
    ``policy_dtype="fp16x3"`` (fused only) runs the towers on fp16 MFMA with every operand
    split into fp16 hi + lo halves and three MFMAs per k step: fp32-level results (values
    within ~3e-6 of the PyTorch fp32 policy at obs of O(1), as the fp32 path; ~1e-5 at the envs'
    largest obs of +-90; obs components past +-255.875, the fp16 operand range, are read as
    +-255.875: INTEGRATION.md) at 1.44x the collection rate.
    ``policy_dtype="bf16"`` (fused only, opt-in) runs the towers on bf16 MFMA with fp32
    accumulation: actions / values / log-probs then differ from the fp32 policy by the bf16
    rounding of obs, weights and the first hidden layer (the stored log-probs are those of
    the bf16 mean; PPO's first-epoch ratio starts within ~1e-3 of 1 instead of at 1).
    ``stats=True`` (one-launch path only, a batch with ``episode_stats=True`` and auto-reset) makes
    ``collect`` account for every episode the rollout finishes and for the samples' explained
    variance in the same launch (``rr_rollout_collect_stats``; the rollout itself is bitwise
    unchanged): ``ro.stats.last()`` / ``ro.stats.window()`` return SB3's ``rollout/*`` figures and
    ``train/explained_variance`` (``rollout_stats.RolloutStats``).

    A ``MlpCategoricalActorCritic`` (the reference's ``DiscreteActions3DOF`` stack, 3DOF batches
    only): ``actions`` is [n_steps, N, 1], the chosen index as a float (SB3's buffer for a
    ``Discrete`` space), and the env steps with the policy's table row. The default fused path is the
    two-launch one (``rr_policy_act_discrete`` + the env step, then ``rr_policy_bootstrap`` and
    ``rr_gae``). ``one_launch=True`` is opt-in for it: the whole ``collect`` in ONE launch
    (``rr_rollout_collect_discrete``: the collect kernel's loop with a softmax head, one uniform draw
    per sample and the table row), and with ``per_step=True`` one ``rr_rollout_step_discrete`` per
    step, then ``rr_policy_bootstrap`` and ``rr_gae``; both give bitwise the two-launch rollout. They
    need a batch on a CUDA device, an RK4 / Euler integrator, 64x64 towers and 2 .. 4 choices.
    ``one_launch`` stays False by default here (unlike the Gaussian policy's) until a later change
    flips it. ``stats=True`` with ``one_launch=True`` (and not ``per_step``) is
    ``rr_rollout_collect_discrete_stats``: the same launch with the Gaussian policy's accounting, ``ro.stats``
    the same ``RolloutStats``, the rollout bitwise ``rr_rollout_collect_discrete``'s; ``stats=True`` without
    ``one_launch=True`` or with ``per_step=True`` raises, as does a batch without ``episode_stats=True`` and
    ``auto_reset=True``. A ``policy_dtype`` other than "fp32" raises. ``fused=False`` samples with
    ``torch.multinomial`` on ``generator``."""

    def __init__(self, batch, policy, n_steps=16, gamma=0.99, gae_lambda=0.95, generator=None, fused=None,
                 seed=0, policy_dtype="fp32", one_launch=None, per_step=False, stats=False):
        self.env, self.policy = batch, policy
        self.n_steps, self.gamma, self.lam = n_steps, gamma, gae_lambda
        n, ns, na = batch.num_envs, batch.state_dim, batch.action_dim
        self.discrete = isinstance(policy, MlpCategoricalActorCritic)
        if self.discrete:  # refused before anything touches the device
            if ns != 7 or na != 2:
                raise ValueError("a Categorical policy drives the 3DOF env (its table rows are [gimbal, thrust]): "
                                 "a 6DOF batch is refused")
            if policy_dtype != "fp32":
                raise ValueError("policy_dtype=%r is not available for a Categorical policy: it collects on fp32 "
                                 "towers" % policy_dtype)
            if stats:  # rr_rollout_collect_discrete_stats: the one-launch collect only, on a real batch
                if not hasattr(batch, "params"):
                    raise ValueError("stats=True needs a RocketBatch (its params hold the integrator and the "
                                     "episode_stats / auto_reset flags)")
                if not one_launch or per_step:
                    raise ValueError("stats=True for a Categorical policy needs one_launch=True without per_step=True "
                                     "(rr_rollout_collect_discrete_stats); its default collect is the two-launch one")
            opt = "one_launch=True" if one_launch else "per_step=True" if per_step and one_launch is None else None
            if opt:  # the opt-in launches of the discrete-rollout unit
                if torch.device(batch.device).type != "cuda":
                    raise ValueError("%s for a Categorical policy needs a batch on a CUDA device "
                                     "(rr_rollout_collect_discrete / rr_rollout_step_discrete)" % opt)
                if fused is not None and not fused:
                    raise ValueError("%s needs the fused policy (fused=False collects in PyTorch ops)" % opt)
                if int(batch.params.integrator) == 2:  # RR_INT_DOPRI5
                    raise ValueError("%s is not available on an integrator=\"dopri5\" batch: a Categorical policy "
                                     "collects there with two launches per step" % opt)
                fused = True
            if fused and not fused_discrete_supported(policy, ns):
                raise ValueError("the fused Categorical path needs 64x64 towers and 2 .. 4 choices")
            if fused is None:
                fused = fused_discrete_supported(policy, ns)
            one_launch = bool(opt)
        dev = batch.device
        f = dict(device=dev, dtype=torch.float32)
        self.obs = torch.zeros((n_steps, n, ns), **f)
        self.actions = torch.zeros((n_steps, n, 1 if self.discrete else na), **f)
        self.rewards = torch.zeros((n_steps, n), **f)
        self.starts = torch.zeros((n_steps, n), **f)   # SB3 episode_starts
        self.values = torch.zeros((n_steps, n), **f)
        self.log_probs = torch.zeros((n_steps, n), **f)
        self.advantages = torch.zeros((n_steps, n), **f)
        self.returns = torch.zeros((n_steps, n), **f)
        self.last_obs = batch.reset().clone()
        self.last_start = torch.ones((n,), **f)
        self.last_value = torch.zeros((n,), **f)
        self.last_done = torch.zeros((n,), **f)
        self.gen = generator
        self._clipped = torch.zeros((n, na), **f)
        self._tobs = torch.zeros((n, ns), **f)
        self._r = torch.zeros((n,), **f)
        if fused is None:
            fused = isinstance(policy, MlpActorCritic) and policy.hidden == (64, 64) and (ns, na) in ((14, 3), (7, 2))
        self.fused = bool(fused)
        if policy_dtype not in POLICY_PRECISIONS:
            raise ValueError("policy_dtype must be one of %s" % sorted(POLICY_PRECISIONS))
        if policy_dtype != "fp32" and not self.fused:
            raise ValueError("policy_dtype=%r needs the fused HIP policy path" % policy_dtype)
        self.policy_dtype = policy_dtype
        dopri = self.fused and int(batch.params.integrator) == 2  # RR_INT_DOPRI5: two-launch path
        if one_launch is None:
            one_launch = self.fused and not dopri
        if one_launch and (not self.fused or dopri):
            raise ValueError("one_launch needs the fused policy and an RK4 / Euler env")
        self.one_launch = bool(one_launch)
        self.per_step = bool(per_step) or not self.one_launch  # one_launch + not per_step: rr_rollout_collect
        self.stats = None
        if stats:
            from . import _lib

            if not self.one_launch or self.per_step:
                raise ValueError("stats=True needs the one-launch collect (fused policy, RK4 / Euler env, not per_step)")
            flags = int(batch.params.flags)
            if not flags & _lib.RR_FLAG_EPISODE_STATS or not flags & _lib.RR_FLAG_AUTO_RESET:
                raise ValueError("stats=True needs a batch created with episode_stats=True and auto_reset=True")
        if self.fused:
            from . import _lib

            self._lib = _lib.load()
            self._pack = PolicyPack(policy, ns, policy.n_choices if self.discrete else na, dev, precision=policy_dtype)
            self.iter = torch.zeros((1,), dtype=torch.int64, device=dev)  # advanced by every collect (graph-safe)
            self.seed = int(seed) & (2 ** 64 - 1)
            self._ones = torch.ones((n,), dtype=torch.uint8, device=dev)
            self._zeros = torch.zeros((n,), **f)
            import ctypes

            from .batch import _ptr

            self._c, self._p = ctypes, _ptr
            # the two-launch path's act call (its symbol, the arguments between params and the precision)
            # and rr_policy_bootstrap's act_dim
            self._act, self._act_shape, self._boot_na = "rr_policy_act", (ns, na), na
            # the one-launch and per-step calls, and what they take between params and the precision
            self._collect, self._step, self._head = "rr_rollout_collect", "rr_rollout_step", ()
            self._collect_stats = "rr_rollout_collect_stats"
            if self.discrete:  # the host table the discrete calls copy into their launch; the 4-head image's (7, 4)
                table = (ctypes.c_float * (2 * policy.n_choices))(*policy.table.reshape(-1).tolist())
                self._act, self._act_shape, self._boot_na = "rr_policy_act_discrete", (ns, policy.n_choices, table), 4
                self._collect, self._step = "rr_rollout_collect_discrete", "rr_rollout_step_discrete"
                self._collect_stats = "rr_rollout_collect_discrete_stats"
                self._head = (policy.n_choices, table)
            bufs = _lib.RrBuffers()
            _lib.check(self._lib.rr_get_buffers(batch._h, ctypes.byref(bufs)), "rr_get_buffers")
            self._term_obs = ctypes.c_void_p(bufs.terminal_obs)
            batch.done.fill_(1)  # SB3: _last_episode_starts = ones before the first rollout
            if stats:
                from .rollout_stats import RolloutStats

                self.stats = RolloutStats(n, dev, self._lib)

    @torch.no_grad()
    def collect(self):
        if self.fused:
            return self._collect_fused()
        env, pol = self.env, self.policy
        for t in range(self.n_steps):
            obs = self.last_obs
            mean, value = pol(obs)
            if self.discrete:  # mean holds the logits; the env takes the table row of the drawn index
                act = torch.multinomial(torch.softmax(mean, dim=-1), 1, generator=self.gen).to(mean.dtype)
            else:
                noise = torch.randn(mean.shape, device=mean.device, generator=self.gen)
                act = mean + pol.log_std.exp() * noise
            self.obs[t].copy_(obs)
            self.actions[t].copy_(act)
            self.values[t].copy_(value)
            self.log_probs[t].copy_(pol.log_prob(mean, act))
            self.starts[t].copy_(self.last_start)
            if self.discrete:
                self._clipped.copy_(pol.continuous(act[:, 0]))
            else:
                torch.clamp(act, -1.0, 1.0, out=self._clipped)
            nobs, rew, done, trunc = env.step(self._clipped)
            # SB3 1.6: bootstrap timeouts with the value of the terminal observation
            env.copy_terminal(out=(self._tobs, None, None))
            # a select, as the fused kernels: terminal rows of envs that are not done are stale
            # (possibly non-finite), and NaN * 0 would leak into the reward
            torch.where(trunc.bool(), torch.addcmul(rew, pol.value(self._tobs), trunc.float(), value=self.gamma),
                        rew, out=self._r)
            self.rewards[t].copy_(self._r)
            self.last_obs.copy_(nobs)
            self.last_start.copy_(done.float())
        self.last_value.copy_(pol.value(self.last_obs))
        self.last_done.copy_(self.last_start)
        self._gae()

    def _collect_fused(self):
        """one_launch: the whole rollout + GAE in one rr_rollout_collect launch, or (per_step)
        one rr_rollout_step per step (the env's obs buffer is written on the last step only),
        then V(last obs); their _discrete twins for a Categorical policy. Otherwise two launches per step: rr_policy_act
        (forward + sample of step t, bootstrap of step t-1, episode-start flags) and the
        fused env step; obs are read in place from the env's output buffer."""
        env, lib, c, p = self.env, self._lib, self._c, self._p
        from . import _lib

        n, ns, na = env.num_envs, env.state_dim, self._boot_na
        params = p(self._pack.pack())
        stream = c.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        it, obs, done = p(self.iter), p(env.obs), p(env.done)
        prec = self._pack.prec
        if self.stats is not None:
            st = self.stats.struct()
            _lib.check(getattr(lib, self._collect_stats)(env._h, params, *self._head, prec, self.seed, it, self.n_steps,
                                                         self.gamma, self.lam, p(self.obs), p(self.actions),
                                                         p(self.values), p(self.log_probs), p(self.starts),
                                                         p(self.rewards), p(self.advantages), p(self.returns),
                                                         p(self.last_value), p(self.last_done), p(self.last_start),
                                                         obs, p(env.reward), done, p(env.truncated), p(env.terms),
                                                         c.byref(st), stream), self._collect_stats)
            self.iter.add_(1)
            return
        if self.one_launch and not self.per_step:
            _lib.check(getattr(lib, self._collect)(env._h, params, *self._head, prec, self.seed, it, self.n_steps,
                                                   self.gamma, self.lam, p(self.obs), p(self.actions), p(self.values),
                                                   p(self.log_probs), p(self.starts), p(self.rewards),
                                                   p(self.advantages), p(self.returns), p(self.last_value),
                                                   p(self.last_done), p(self.last_start), obs, p(env.reward), done,
                                                   p(env.truncated), p(env.terms), stream), self._collect)
            self.iter.add_(1)
            return
        if self.one_launch:
            T, step = self.n_steps, getattr(lib, self._step)
            for t in range(T):
                _lib.check(step(env._h, params, *self._head, prec, self.seed, it, t, self.gamma, p(self.obs[t]),
                                p(self.actions[t]), p(self.values[t]), p(self.log_probs[t]), p(self.starts[t]),
                                p(self.rewards[t]), obs if t == T - 1 else None, p(env.reward), done,
                                p(env.truncated), p(env.terms), stream), self._step)
            _lib.check(lib.rr_policy_bootstrap(params, ns, na, prec, n, None, None, None, self.gamma, None, obs,
                                               p(self.last_value), stream), "rr_policy_bootstrap")
            self._finish(stream)
            return
        act = getattr(lib, self._act)
        for t in range(self.n_steps):
            prev = t > 0
            carry = (self._term_obs if prev else None, p(env.truncated) if prev else None,
                     p(env.reward) if prev else None, self.gamma, p(self.rewards[t - 1]) if prev else None, done,
                     p(self.starts[t]), stream)
            out = (p(self._clipped), p(self.actions[t]), p(self.values[t]), p(self.log_probs[t]), p(self.obs[t]))
            _lib.check(act(params, *self._act_shape, prec, n, env.env_id_offset, obs, self.seed, it, t, *out, *carry),
                       self._act)
            env.step(self._clipped)
        _lib.check(lib.rr_policy_bootstrap(params, ns, na, prec, n, self._term_obs, p(env.truncated), p(env.reward),
                                           self.gamma, p(self.rewards[self.n_steps - 1]), obs, p(self.last_value),
                                           stream), "rr_policy_bootstrap")
        self._finish(stream)

    def _finish(self, stream):
        """last_done / last_start from the env's done flags, GAE (rr_gae), advance the
        noise counter."""
        from . import _lib

        env, lib, p = self.env, self._lib, self._p
        n = env.num_envs
        self.last_done.copy_(env.done)
        self.last_start.copy_(env.done)
        _lib.check(lib.rr_gae(self.n_steps, n, p(self.rewards), p(self.values), p(self.starts), p(self.last_value),
                              p(self.last_done), self.gamma, self.lam, p(self.advantages), p(self.returns), stream),
                   "rr_gae")
        self.iter.add_(1)

    def _gae(self):
        """SB3 RolloutBuffer.compute_returns_and_advantage, on device. The scan runs in float64
        and each stored value is rounded once, as rr_gae's (an fp32 scan is ~5e-5 off at |A| ~ 150)."""
        rewards, values, starts = self.rewards.double(), self.values.double(), self.starts.double()
        last_gae = torch.zeros_like(self.last_value, dtype=torch.float64)
        for t in reversed(range(self.n_steps)):
            if t == self.n_steps - 1:
                nonterminal = 1.0 - self.last_done.double()
                next_values = self.last_value.double()
            else:
                nonterminal = 1.0 - starts[t + 1]
                next_values = values[t + 1]
            delta = rewards[t] + self.gamma * next_values * nonterminal - values[t]
            last_gae = delta + self.gamma * self.lam * nonterminal * last_gae
            self.advantages[t].copy_(last_gae)
            self.returns[t].copy_(last_gae + values[t])
