"""Policy evaluation on the device (SB3 EvalCallback / evaluate_policy + EpisodeAnalyzer): under the most
likely action or, with ``deterministic=False``, under the sampled one."""
import torch

from ._lib import (RR_EVAL_BOUNDS as EVAL_BOUNDS, RR_EVAL_EVENT as EVAL_EVENT, RR_EVAL_LANDED as EVAL_LANDED,
                   RR_EVAL_NONFINITE as EVAL_NONFINITE, RR_EVAL_TRUNCATED as EVAL_TRUNCATED)
from .eval_trace import EpisodeRecord, EvalTrace  # noqa: F401
from .policy import (POLICY_PRECISIONS, MlpActorCritic, MlpCategoricalActorCritic, PolicyPack,
                     fused_discrete_supported, fused_grad_supported)


class EvalResult:
    """The per-episode outputs of one evaluation, as tensors on the evaluator's device (views of
    its buffers: the next ``run()`` overwrites them): ``episodes`` [n] (episodes env i completed),
    ``ep_return`` / ``ep_length`` / ``flags`` / ``used_mass`` [n_episodes, n] and ``final_state``
    [n_episodes, state_dim, n] (the terminal state, un-normalised). Row [k, i] is valid where
    ``k < episodes[i]``; ``finished()`` is that mask. ``trace`` is the ``EvalTrace`` of the envs the
    evaluator records (``PolicyEvaluator(record=...)``), else None."""

    def __init__(self, episodes, ep_return, ep_length, flags, used_mass, final_state, state_names, trace=None):
        self.episodes, self.ep_return, self.ep_length, self.flags = episodes, ep_return, ep_length, flags
        self.used_mass, self.final_state, self.state_names = used_mass, final_state, list(state_names)
        self.trace = trace

    def finished(self):
        k = torch.arange(self.ep_return.shape[0], device=self.episodes.device)
        return k[:, None] < self.episodes[None, :]

    def stats(self):
        """One synchronise (a single device-to-host copy). SB3 ``evaluate_policy``'s
        ``mean_reward`` / ``std_reward`` (population std) and ``mean_ep_length``; the reference
        EpisodeAnalyzer's ``ep_statistic/landing_success`` (here the rate of episodes whose last
        step paid the landing reward), ``ep_statistic/used_mass`` and ``final_errors/<state name>``
        (mean |terminal state|, wrappers.py:210-224); the counts of each way an episode ended
        (``n_event`` / ``n_bounds`` / ``n_truncated`` / ``n_nonfinite``), ``episodes`` and
        ``unfinished`` (rows not completed within max_steps, excluded from every mean)."""
        m = self.finished()
        w = m.double()
        cnt = w.sum()
        ret = torch.where(m, self.ep_return.double(), torch.zeros_like(w))
        mean = ret.sum() / cnt
        var = (torch.where(m, (self.ep_return.double() - mean) ** 2, torch.zeros_like(w))).sum() / cnt
        fl = torch.where(m, self.flags.to(torch.int64), torch.zeros_like(m, dtype=torch.int64))
        fe = torch.where(m[:, None, :], self.final_state.double().abs(), torch.zeros_like(w)[:, None, :])
        vals = [mean, var.sqrt(),
                torch.where(m, self.ep_length.double(), torch.zeros_like(w)).sum() / cnt,
                (fl & EVAL_LANDED).ne(0).double().sum() / cnt,
                torch.where(m, self.used_mass.double(), torch.zeros_like(w)).sum() / cnt]
        vals += [(fl & bit).ne(0).double().sum() for bit in (EVAL_EVENT, EVAL_BOUNDS, EVAL_TRUNCATED, EVAL_NONFINITE)]
        vals += [cnt, m.numel() - cnt]
        host = torch.cat([torch.stack(vals), fe.sum(dim=(0, 2)) / cnt]).cpu().tolist()
        out = dict(zip(("mean_reward", "std_reward", "mean_ep_length", "ep_statistic/landing_success",
                        "ep_statistic/used_mass"), host[:5]))
        for k, v in zip(("n_event", "n_bounds", "n_truncated", "n_nonfinite", "episodes", "unfinished"), host[5:11]):
            out[k] = int(v)
        for name, v in zip(self.state_names, host[11:]):
            out["final_errors/" + name] = v
        return out


class PolicyEvaluator:
    """Deterministic evaluation of ``policy`` on every env of a ``RocketBatch`` (auto-reset, with
    a TimeLimit or ``max_steps``): each env runs ``n_episodes`` episodes under the policy's mean
    action, starting from the batch's CURRENT state (reset first for whole episodes), and rests at
    the first state of a fresh episode afterwards. ``run()`` launches and returns an ``EvalResult``
    without synchronising; ``batch.obs`` holds the post-call observation.

    ``fused=True`` (default for an ``MlpActorCritic`` with 64x64 towers on an RK4 / Euler env): ONE
    launch (``rr_policy_evaluate``: the collect kernel's step loop with only the pi tower, state in
    registers, nothing stored per step), capturable in a graph. On an ``integrator="dopri5"`` batch
    ``fused=True`` must be asked for and is ``rr_policy_evaluate_exact``: the same loop around the exact
    solver, one launch where the step-by-step path takes two exact steps and a dozen small launches
    per iteration, bit for bit the episodes of ``rr_policy_act`` + ``rr_step`` (``record=`` with it
    raises unless ``record_in_launch=True`` asks for the recording launch, below).
    ``fused=False`` (any policy whose
    ``policy(obs)[0]`` is the action mean, and the default for ``integrator="dopri5"``): the same algorithm in
    PyTorch ops, one ``batch.step`` per iteration for ``max_steps`` iterations; the un-reset terminal
    state and the reward terms of each step come from a shadow batch without auto-reset stepped
    from the same state, and envs that have finished are put back after every step.
    ``max_steps`` (default ``n_episodes * max_episode_steps``) caps the steps of each env; episodes
    not completed by then leave their rows untouched (``EvalResult.episodes`` counts).

    ``record`` (a sequence or tensor of env indices local to the batch, unique, any order) records
    whole episodes of those envs: ``EvalResult.trace`` is then an ``EvalTrace`` with, per recorded
    env and episode, the un-normalised state before the episode's first step and after every step,
    the clipped mean actions, the reward terms and rewards, and the episode's length; its
    ``episode(env_id, k)`` gives the dataframes and figures of the reference's ``EpisodeAnalyzer``.
    The fused path does it in the same single launch (``rr_policy_evaluate_trace``); the evaluation
    itself is bit for bit the unrecorded one. ``record_steps`` is the recorded steps per episode
    (default ``max_episode_steps``; required without a TimeLimit): longer episodes are clipped, their
    ``length`` still counts every step. An episode's step count starts at the call, and the v_targ
    history takes v_0 from the first recorded state: reset first, as for whole episodes.
    ``record=None`` is the plain evaluation (``rr_policy_evaluate``).

    ``record_in_launch=True`` (default None: everything above as it is) records on an
    ``integrator="dopri5"`` batch in the one launch as well (``rr_policy_evaluate_exact_trace``): the
    reference's ``make_eval_env`` set-up, a deterministic policy stepped by the exact integrator with the
    ``EpisodeAnalyzer``'s histories, hundreds of launches cheaper than ``fused=False, record=``. It needs
    ``record``, ``fused=True``, a CUDA batch and the 64x64 ``MlpActorCritic``, with any ``policy_dtype``.
    The recorded state rows are the float32 casts of the fp64 state, the terms those ``rr_step`` stores.
    On a fused RK4 / Euler batch recording already happens in the launch and the keyword changes
    nothing; with ``fused=False``, and for a Categorical policy on a dopri5 batch (recorded step by
    step only), it raises.

    A ``MlpCategoricalActorCritic`` (discrete 3DOF actions) takes the action
    ``policy.continuous(policy.mode(logits))``, SB3's deterministic prediction behind
    ``DiscreteActions3DOF``. By default it runs through the step-by-step path (``fused=False``, chosen
    automatically; the default stays there until a later change flips it). ``fused=True`` is opt-in:
    ONE launch (``rr_policy_evaluate_discrete``: the evaluation kernel's loop with the argmax of the
    logits, the lowest index on a tie, and the table row), on a CUDA batch with an RK4 / Euler
    integrator, 64x64 towers and 2 .. 4 choices. On an ``integrator="dopri5"`` batch ``fused=True`` is
    ``rr_policy_evaluate_exact_discrete``: the same head in the exact evaluation's loop, the reference's
    ``sensitivity_test.py`` set-up (``evaluate_policy`` on ``TimeLimit(DiscreteActions3DOF(RewardAnnealing(
    Rocket)))`` under scipy RK45 + brentq) in one launch, bit for bit the episodes of
    ``rr_policy_act_discrete`` + ``rr_step`` where the sampled index is the argmax; ``record=`` with it
    raises (recording stays on the step-by-step path there). Where two logits lie within the fp32 towers'
    error of each other the two paths may pick different rows. On an RK4 / Euler batch ``record=`` records
    on either path: with
    ``fused=True`` in the same single launch (``rr_policy_evaluate_discrete_trace``), otherwise in the
    step-by-step loop; the recorded action rows are the table rows the env stepped with, and
    ``EvalTrace.choice`` [K, ne, S] (int32) holds their indices, from which ``Demonstrations.from_trace``
    builds the ``[M, 1]`` index demonstrations of ``rr_bc_update_discrete``. A ``policy_dtype`` other than
    "fp32" raises for it.

    ``deterministic=False`` (default True: everything above, "the clipped mean action, always") evaluates
    the STOCHASTIC policy, SB3's ``evaluate_policy(model, env, deterministic=False)``: the action of step
    ``k`` of the call is the sample ``rr_rollout_step`` / ``rr_rollout_step_discrete`` draws at ``t = k``
    under ``(seed, iter)`` (``mean + exp(log_std) * eps`` clipped to [-1, 1]; for a Categorical policy the
    inverse-CDF index of one uniform draw and its table row), so an episode is bit for bit the one the
    per-step rollout runs. ``run()`` is ONE launch (``rr_policy_evaluate_sampled``, for a Categorical policy
    ``rr_policy_evaluate_discrete_sampled``), with ``record=`` the same launch recording; the recorded
    action rows are then the CLIPPED samples the env stepped with (the table rows, ``choice`` the sampled
    indices), never the unclipped sample. The evaluator owns ``self.seed`` (from ``seed``) and ``self.iter``,
    an int64 ``[1]`` device tensor that ``run()`` advances by one in stream order, exactly as
    ``DeviceRollout.iter``: a captured ``run()`` draws fresh noise at every replay, and two evaluators with
    equal ``(seed, iter)`` on twin batches produce equal bits. A Gaussian policy resolves ``fused=None`` as
    above and takes every ``policy_dtype``; a Categorical one needs ``fused=True`` and fp32. It raises
    ``ValueError`` with ``fused=False``, a ``fused=None`` that resolves to the step-by-step path (a policy
    that is not 64x64, an ``integrator="dopri5"`` batch), ``fused=True`` on a dopri5 batch, a CPU batch and
    ``record_in_launch=True``: the step-by-step path and the exact integrator are out of scope for it."""

    def __init__(self, batch, policy, n_episodes=5, max_steps=None, policy_dtype="fp32", fused=None, record=None,
                 record_steps=None, record_in_launch=None, deterministic=True, seed=0):
        from . import _lib
        from .params import STATE_NAMES_3DOF, STATE_NAMES_6DOF

        self.env, self.policy = batch, policy
        n, ns, na = batch.num_envs, batch.state_dim, batch.action_dim
        self._discrete = isinstance(policy, MlpCategoricalActorCritic)
        self.deterministic = bool(deterministic)
        if not self.deterministic:  # the refusals of the sampled evaluation: the batch's params and device only
            scope = ("deterministic=False is the one-launch sampled evaluation (rr_policy_evaluate_sampled): the "
                     "step-by-step path and the exact integrator are out of scope for it")
            if record_in_launch:
                raise ValueError("deterministic=False with record_in_launch=True is not available; " + scope)
            if fused is not None and not fused:
                raise ValueError("deterministic=False with fused=False is not available; " + scope)
            if torch.device(batch.device).type != "cuda":
                raise ValueError("deterministic=False needs a batch on a CUDA device; " + scope)
            if int(batch.params.integrator) == _lib.RR_INT_DOPRI5:
                raise ValueError("deterministic=False on an integrator=\"dopri5\" batch is not available; " + scope)
            if self._discrete and not fused:
                raise ValueError("deterministic=False for a Categorical policy needs fused=True, as its other "
                                 "launches; " + scope)
            if not self._discrete and not fused_grad_supported(policy, ns, na):
                raise ValueError("deterministic=False needs an MlpActorCritic with 64x64 towers (this policy takes "
                                 "the step-by-step path); " + scope)
        if record_in_launch:  # the refusals that need nothing of the batch but its integrator
            if record is None:
                raise ValueError("record_in_launch=True needs record")
            if fused is not None and not fused:
                raise ValueError("record_in_launch=True needs fused=True (fused=False records step by step)")
            if self._discrete and hasattr(batch, "params") and int(batch.params.integrator) == _lib.RR_INT_DOPRI5:
                raise ValueError("record_in_launch=True is not available for a Categorical policy on an "
                                 "integrator=\"dopri5\" batch: it is evaluated step by step there")
        if self._discrete:
            if ns != 7 or na != 2:
                raise ValueError("a Categorical policy drives the 3DOF env (its table rows are [gimbal, thrust])")
            if record is not None and not hasattr(batch, "params"):
                raise ValueError("record= needs a RocketBatch (its params hold the integrator and the TimeLimit)")
            if policy_dtype != "fp32" and policy_dtype in POLICY_PRECISIONS:
                raise ValueError("policy_dtype=%r is not available for a Categorical policy: it is evaluated on "
                                 "fp32 towers" % policy_dtype)
            if fused:  # the opt-in launch of the discrete-rollout unit
                if torch.device(batch.device).type != "cuda":
                    raise ValueError("fused=True for a Categorical policy needs a batch on a CUDA device "
                                     "(rr_policy_evaluate_discrete / rr_policy_evaluate_exact_discrete)")
                if not fused_discrete_supported(policy, ns):
                    raise ValueError("fused=True needs a Categorical policy with 64x64 towers and 2 .. 4 choices")
                if int(batch.params.integrator) == _lib.RR_INT_DOPRI5 and record is not None:
                    raise ValueError("fused=True with record= is not available for a Categorical policy on an "
                                     "integrator=\"dopri5\" batch: it is recorded step by step there")
            fused = bool(fused)
        dev = batch.device
        p = batch.params
        if not p.flags & _lib.RR_FLAG_AUTO_RESET:
            raise ValueError("PolicyEvaluator needs a RocketBatch with auto_reset=True")
        self.n_episodes = int(n_episodes)
        if self.n_episodes < 1:
            raise ValueError("n_episodes must be at least 1")
        self.max_steps = int(max_steps) if max_steps else self.n_episodes * int(p.max_episode_steps)
        if self.max_steps <= 0:
            raise ValueError("an env without a TimeLimit needs max_steps")
        dopri = int(p.integrator) == _lib.RR_INT_DOPRI5
        if fused is None:  # an exact-mode batch keeps the step-by-step path unless asked (fused=True)
            fused = fused_grad_supported(policy, ns, na) and not dopri
        if fused and not self._discrete and not fused_grad_supported(policy, ns, na):
            raise ValueError("fused evaluation needs an MlpActorCritic with 64x64 towers")
        if record_in_launch and not fused:  # fused=None resolved to the step-by-step path (a dopri5 batch)
            raise ValueError("record_in_launch=True needs fused=True (fused=False records step by step)")
        if fused and dopri and record is not None and not record_in_launch:
            raise ValueError("record= on an integrator=\"dopri5\" batch needs fused=False, or "
                             "record_in_launch=True for the recording one-launch exact evaluation")
        if fused and dopri and record_in_launch and torch.device(batch.device).type != "cuda":
            raise ValueError("record_in_launch=True needs a batch on a CUDA device (rr_policy_evaluate_exact_trace)")
        self.fused = bool(fused)
        self._exact = self.fused and dopri
        if policy_dtype not in POLICY_PRECISIONS:
            raise ValueError("policy_dtype must be one of %s" % sorted(POLICY_PRECISIONS))
        if policy_dtype != "fp32" and not self.fused:
            raise ValueError("policy_dtype=%r needs the fused HIP policy path" % policy_dtype)
        self.policy_dtype = policy_dtype
        ne = self.n_episodes
        self.episodes = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.ep_return = torch.zeros((ne, n), dtype=torch.float32, device=dev)
        self.ep_length = torch.zeros((ne, n), dtype=torch.int32, device=dev)
        self.flags = torch.zeros((ne, n), dtype=torch.uint8, device=dev)
        self.used_mass = torch.zeros((ne, n), dtype=torch.float32, device=dev)
        self.final_state = torch.zeros((ne, ns, n), dtype=torch.float32, device=dev)
        self.trace = self._make_trace(record, record_steps)
        self.result = EvalResult(self.episodes, self.ep_return, self.ep_length, self.flags, self.used_mass,
                                 self.final_state, STATE_NAMES_6DOF if batch.model == 6 else STATE_NAMES_3DOF,
                                 trace=self.trace)
        self._lib = _lib.load()
        if not self.deterministic:  # the noise key of run(): advanced in stream order, as DeviceRollout.iter
            self.seed = int(seed) & (2 ** 64 - 1)
            self.iter = torch.zeros((1,), dtype=torch.int64, device=dev)
        if self.fused:
            self._pack = PolicyPack(policy, ns, policy.n_choices if self._discrete else na, dev, precision=policy_dtype)
            if self._discrete:  # the host table the call copies into its launch
                import ctypes

                self._table = (ctypes.c_float * (2 * policy.n_choices))(*policy.table.reshape(-1).tolist())
            self._out = _lib.RrEvalOut(*[t.data_ptr() for t in (self.episodes, self.ep_return, self.ep_length,
                                                                 self.flags, self.used_mass, self.final_state)])
            if self.trace is not None:
                tr = self.trace
                self._trace_io = _lib.RrEvalTrace(self._slot.data_ptr(), tr.state.shape[0], tr.steps,
                                                  tr.state.data_ptr(), tr.action.data_ptr(), tr.terms.data_ptr(),
                                                  tr.length.data_ptr())
                self._choice = tr.choice.data_ptr() if tr.choice is not None else None
            return
        from .batch import RocketBatch
        from .params import INTEGRATORS

        integ = {v: k for k, v in INTEGRATORS.items()}
        self._dopri = dopri
        self._stats = bool(p.flags & _lib.RR_FLAG_EPISODE_STATS)
        # the same env without auto-reset, TimeLimit or Monitor: stepped from the batch's pre-step
        # state, it leaves the un-reset terminal state and the reward terms of the step
        self._shadow = RocketBatch(n, model=batch.model, device=dev, max_episode_steps=0, auto_reset=False,
                                   episode_stats=False, reward_annealing=bool(p.flags & _lib.RR_FLAG_REWARD_ANNEALING),
                                   integrator=integ[int(p.integrator)], env_id_offset=batch.env_id_offset,
                                   compute_terms=True, scipy_h0_clamp=bool(p.flags & _lib.RR_FLAG_SCIPY_H0_CLAMP),
                                   **batch.cfg.kwargs)
        self._none = torch.zeros((n,), dtype=torch.uint8, device=dev)
        self._tlen = torch.zeros((n,), dtype=torch.int32, device=dev)

    def _make_trace(self, record, record_steps):
        """The slot plane ([n] int32: the trace slot of env i, -1 = not recorded) and the trace
        buffers of ``record``, allocated once; None without ``record``."""
        if record is None:
            if record_steps is not None:
                raise ValueError("record_steps needs record")
            return None
        env = self.env
        n, dev = env.num_envs, env.device
        ids = torch.as_tensor(record).reshape(-1).to(torch.int64).cpu()
        if ids.numel() < 1:
            raise ValueError("record must name at least one env")
        if int(ids.min()) < 0 or int(ids.max()) >= n:
            raise ValueError("record holds an env index outside [0, %d)" % n)
        if ids.unique().numel() != ids.numel():
            raise ValueError("record holds an env index twice")
        steps = int(record_steps) if record_steps else int(env.params.max_episode_steps)
        if steps < 1:
            raise ValueError("an env without a TimeLimit needs record_steps")
        k, ne = ids.numel(), self.n_episodes
        slot = torch.full((n,), -1, dtype=torch.int32)
        slot[ids] = torch.arange(k, dtype=torch.int32)
        self._slot = slot.to(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        return EvalTrace(env.cfg, torch.zeros((k, ne, steps + 1, env.state_dim), **f32),
                         torch.zeros((k, ne, steps, env.action_dim), **f32),
                         torch.zeros((k, ne, steps, env.n_terms + 1), **f32),
                         torch.zeros((ne, k), dtype=torch.int32, device=dev), ids.to(dev), episodes=self.episodes,
                         choice=torch.zeros((k, ne, steps), dtype=torch.int32, device=dev)
                         if getattr(self, "_discrete", False) else None)  # a Categorical policy's indices

    @torch.no_grad()
    def run(self):
        if not self.fused:
            return self._run_unfused()
        import ctypes

        from . import _lib
        from .batch import _ptr

        env = self.env
        stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        if not self.deterministic:  # one launch of the sampled call, then the iteration word moves on
            trace = ctypes.byref(self._trace_io) if self.trace is not None else None
            if self._discrete:
                _lib.check(self._lib.rr_policy_evaluate_discrete_sampled(
                    env._h, _ptr(self._pack.pack()), self.policy.n_choices, self._table, self._pack.prec, self.seed,
                    _ptr(self.iter), self.n_episodes, self.max_steps, ctypes.byref(self._out), trace,
                    self._choice if self.trace is not None else None, _ptr(env.obs), stream),
                    "rr_policy_evaluate_discrete_sampled")
            else:
                _lib.check(self._lib.rr_policy_evaluate_sampled(
                    env._h, _ptr(self._pack.pack()), self._pack.prec, self.seed, _ptr(self.iter), self.n_episodes,
                    self.max_steps, ctypes.byref(self._out), trace, _ptr(env.obs), stream),
                    "rr_policy_evaluate_sampled")
            self.iter.add_(1)
            return self.result
        if self.trace is not None and self._discrete:
            _lib.check(self._lib.rr_policy_evaluate_discrete_trace(
                env._h, _ptr(self._pack.pack()), self.policy.n_choices, self._table, self._pack.prec, self.n_episodes,
                self.max_steps, ctypes.byref(self._out), ctypes.byref(self._trace_io), self._choice, _ptr(env.obs),
                stream), "rr_policy_evaluate_discrete_trace")
            return self.result
        if self.trace is not None:
            call, name = ((self._lib.rr_policy_evaluate_exact_trace, "rr_policy_evaluate_exact_trace") if self._exact
                          else (self._lib.rr_policy_evaluate_trace, "rr_policy_evaluate_trace"))
            _lib.check(call(env._h, _ptr(self._pack.pack()), self._pack.prec, self.n_episodes, self.max_steps,
                            ctypes.byref(self._out), ctypes.byref(self._trace_io), _ptr(env.obs), stream), name)
            return self.result
        if self._discrete:
            call, name = ((self._lib.rr_policy_evaluate_exact_discrete, "rr_policy_evaluate_exact_discrete")
                          if self._exact else (self._lib.rr_policy_evaluate_discrete, "rr_policy_evaluate_discrete"))
            _lib.check(call(env._h, _ptr(self._pack.pack()), self.policy.n_choices, self._table, self._pack.prec,
                            self.n_episodes, self.max_steps, ctypes.byref(self._out), _ptr(env.obs), stream), name)
            return self.result
        call, name = ((self._lib.rr_policy_evaluate_exact, "rr_policy_evaluate_exact") if self._exact else
                      (self._lib.rr_policy_evaluate, "rr_policy_evaluate"))
        _lib.check(call(env._h, _ptr(self._pack.pack()), self._pack.prec, self.n_episodes, self.max_steps,
                        ctypes.byref(self._out), _ptr(env.obs), stream), name)
        return self.result

    # -- fused=False: the kernel's algorithm in PyTorch ops ---------------------------------------------------
    def _snap(self, env):
        import ctypes

        from . import _lib
        from .batch import _ptr

        st, v0, _ = env.get_state64() if self._dopri else env.get_state()
        cw = torch.empty((env.num_envs,), dtype=torch.int32, device=env.device)
        ret = torch.empty((env.num_envs,), dtype=torch.float32, device=env.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        _lib.check(self._lib.rr_get_aux(env._h, _ptr(cw), _ptr(ret), stream), "rr_get_aux")
        return st, v0, cw, ret

    def _put(self, env, st, v0, cw, ret):
        import ctypes

        from . import _lib
        from .batch import _ptr

        (env.set_state64 if self._dopri else env.set_state)(st, v0=v0, elapsed=cw)
        self._keep = (cw, ret)
        stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        _lib.check(self._lib.rr_set_aux(env._h, _ptr(cw), _ptr(ret), stream), "rr_set_aux")

    def _mean(self, obs):
        pol = self.policy
        if isinstance(pol, (MlpActorCritic, MlpCategoricalActorCritic)):
            return pol.action_net(pol.pi_net(obs))  # the pi tower only
        return pol(obs)[0]

    def _run_unfused(self):
        env, sh, ne = self.env, self._shadow, self.n_episodes
        n, nt = env.num_envs, env.n_terms
        el_mask = (1 << env.counter_bits) - 1

        def put_row(plane, ep, mask, val):  # plane[ep[i], ..., i] = val[..., i] where mask[i]
            idx = ep.clamp(max=ne - 1).long().expand(val.shape)[None]
            plane.scatter_(0, idx, torch.where(mask, val, plane.gather(0, idx)[0])[None])

        obs = env.reset(mask=self._none)  # no env is reset: the obs of the current state
        pre = self._snap(env)
        ep = torch.zeros_like(self.episodes)
        tr = self.trace
        if tr is not None:  # the kernel's records of the recorded envs, same rows, same tensors
            ids, cap = tr.env_ids, tr.steps
            ks = torch.arange(ids.numel(), device=ids.device)
            t_rec = torch.zeros_like(ids)  # steps of the running episode taken in this call
            tr.state[ks, 0, 0] = pre[0].float()[:, ids].T
        ret = pre[3].clone() if self._stats else torch.zeros_like(pre[3])
        m0 = pre[0][-1].float()
        for _ in range(self.max_steps):
            active = ep < ne
            if self._discrete:  # the table row of the most probable choice
                idx = self.policy.mode(self._mean(obs))
                act = self.policy.continuous(idx)
            else:
                act = torch.clamp(self._mean(obs), -1.0, 1.0)
            (sh.set_state64 if self._dopri else sh.set_state)(pre[0], v0=pre[1], elapsed=pre[2] & el_mask)
            sh.step(act)
            y1 = (sh.get_state64() if self._dopri else sh.get_state())[0].float()
            terms = sh.terms
            obs, rew, done, trunc = env.step(act)
            env.copy_terminal(out=(None, None, self._tlen))
            post = self._snap(env)
            ret = torch.where(active, ret + rew, ret)
            end = active & done.bool()
            status = terms[nt + 1]
            fl = ((status > 0) * EVAL_EVENT + (terms[nt] > 0) * EVAL_BOUNDS + trunc.bool() * EVAL_TRUNCATED
                  + (status < 0) * EVAL_NONFINITE + (terms[nt - 1] != 0) * EVAL_LANDED).to(torch.uint8)
            put_row(self.ep_return, ep, end, ret)
            put_row(self.ep_length, ep, end, self._tlen)
            put_row(self.flags, ep, end, fl)
            put_row(self.used_mass, ep, end, m0 - y1[-1])
            put_row(self.final_state, ep, end, y1)
            if tr is not None:
                act_r, end_r, ep_r = active[ids], end[ids], ep[ids].long()
                w = act_r & (t_rec < cap)  # steps past the capacity are counted, not written
                kw, ew, tw = ks[w], ep_r[w], t_rec[w]
                tr.state[kw, ew, tw + 1] = y1[:, ids].T[w]
                tr.action[kw, ew, tw] = act[ids][w]
                if tr.choice is not None:
                    tr.choice[kw, ew, tw] = idx[ids][w].to(torch.int32)
                tr.terms[kw, ew, tw] = torch.cat([terms[:nt, ids].T, rew[ids, None]], dim=1)[w]
                t_rec = t_rec + act_r.to(t_rec.dtype)
                tr.length[ep_r[end_r], ks[end_r]] = t_rec[end_r].to(torch.int32)
                t_rec = torch.where(end_r, torch.zeros_like(t_rec), t_rec)
                nxt = end_r & (ep_r + 1 < ne)  # row 0 of the next episode: the auto-reset state
                tr.state[ks[nxt], ep_r[nxt] + 1, 0] = post[0].float()[:, ids].T[nxt]
            ret = torch.where(end, torch.zeros_like(ret), ret)
            m0 = torch.where(end, post[0][-1].float(), m0)
            ep = ep + end.to(ep.dtype)
            # envs that had finished before this step stay where they were
            pre = tuple(torch.where(active, b, a) for a, b in zip(pre, post))
            self._put(env, *pre)
        self.episodes.copy_(ep)
        if tr is not None:  # episodes cut by max_steps: the steps they took so far
            cut = ep[ids] < ne
            tr.length[ep[ids].long()[cut], ks[cut]] = t_rec[cut].to(torch.int32)
        env.reset(mask=self._none)  # env.obs of the final state
        return self.result


def evaluate_policy(policy, batch, n_eval_episodes=5, return_episode_rewards=False, **kw):
    """SB3 ``evaluate_policy(model, env, n_eval_episodes, deterministic=True)`` on a ``RocketBatch``, or with
    ``deterministic=False, seed=...`` SB3's ``evaluate_policy(..., deterministic=False)`` (the sampled actions
    of ``PolicyEvaluator(deterministic=False)``, one launch):
    resets every env, runs a ``PolicyEvaluator`` (``**kw``: max_steps, policy_dtype, fused, record,
    record_in_launch, deterministic, seed, ...) and returns ``(mean_reward, std_reward)`` or, with ``return_episode_rewards``, ``(episode_rewards,
    episode_lengths)`` as lists over the finished episodes.

    ``n_eval_episodes`` is PER ENV here: every env runs that many episodes, N * n_eval_episodes in
    all. SB3 splits a total over the envs of a vec env, which would leave all but n_eval_episodes of
    thousands of envs idle."""
    batch.reset()
    res = PolicyEvaluator(batch, policy, n_episodes=n_eval_episodes, **kw).run()
    if return_episode_rewards:
        m = res.finished().cpu()
        return res.ep_return.cpu()[m].tolist(), res.ep_length.cpu()[m].tolist()
    s = res.stats()
    return s["mean_reward"], s["std_reward"]
