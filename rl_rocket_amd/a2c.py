"""A2C on a ``DeviceRollout``'s buffers: SB3's other on-policy algorithm, one gradient pass over a short
rollout (the reference's ``main.py`` imports ``A2C`` beside ``PPO``).

``RMSpropTFLike`` is SB3's default A2C optimizer as a ``torch.optim.Optimizer``; ``A2CUpdate`` is one
``A2C.train()`` as ONE library call (``rr_a2c_update``: the PPO learner's towers with the A2C head
derivative, the fixed-order finish, ``clip_grad_norm_`` and the optimizer's step: four launches);
``a2c_update`` is that call where it applies and the same loss in PyTorch autograd elsewhere;
``GraphedA2C`` captures ``ro.collect()`` followed by the update into one hipGraph, so a whole A2C
iteration is one replay with no host work.

The loss is SB3 1.6 ``A2C.train``'s for the ``MlpPolicy`` actor-critic with a diagonal Gaussian:

    A           = advantages, or (A - mean(A)) / (std(A) + 1e-8) with normalize_advantage
    policy_loss = -mean(A * log_prob(actions))
    value_loss  = F.mse_loss(returns, values)
    entropy     = sum_a (0.5 + 0.5 log 2 pi + log_std_a)
    loss        = policy_loss + ent_coef * -entropy + vf_coef * value_loss

then ``clip_grad_norm_(max_grad_norm)`` and ``optimizer.step()``. There is no probability ratio, so the
rollout's stored log-probs are never read: a rollout of any ``policy_dtype`` goes through the same call
(the learner is fp32).

A ``MlpCategoricalActorCritic`` is refused by the three classes here: its fused call has names of its own,
``a2c_discrete.A2CUpdateDiscrete``, ``a2c_update_discrete`` and ``GraphedA2CDiscrete``
(``rr_a2c_update_discrete``), which share this module's optimizer checks, state binding and graph capture.
"""
import ctypes

import torch

from . import _lib
from .learner import _check_params, _stream, _workspace
from .policy import MlpCategoricalActorCritic, _policy_tensors, fused_grad_supported

STAT_NAMES = ("policy_loss", "value_loss", "entropy", "loss", "log_prob")  # RR_A2C_STAT_*


class RMSpropTFLike(torch.optim.Optimizer):
    """``stable_baselines3.common.sb2_compat.rmsprop_tf_like.RMSpropTFLike`` without momentum, centering and
    weight decay (A2C's defaults): TensorFlow's RMSprop, which differs from ``torch.optim.RMSprop`` in two
    places. ``square_avg`` starts at ones, not zeros, and ``eps`` is added inside the square root:

        square_avg = alpha * square_avg + (1 - alpha) * g * g
        p         -= lr * g / sqrt(square_avg + eps)

    State per tensor: ``square_avg`` and ``step``, a float32 scalar on the parameter's device (what a
    capturable torch optimizer keeps). ``step()`` is PyTorch ops only and reads nothing back: it can be
    captured into a graph (``lr`` is then the value at capture)."""

    def __init__(self, params, lr=7e-4, alpha=0.99, eps=1e-5):
        if not 0.0 <= lr < float("inf"):
            raise ValueError("lr must be a finite number >= 0, not %r" % (lr,))
        if not 0.0 <= alpha < 1.0:
            raise ValueError("alpha must be in [0, 1), not %r" % (alpha,))
        if not 0.0 <= eps < float("inf"):
            raise ValueError("eps must be a finite number >= 0, not %r" % (eps,))
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps))

    def init_state(self, p):
        """The state of parameter ``p``, created as the first ``step()`` would if absent."""
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["square_avg"] = torch.ones_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, alpha, eps = group["lr"], group["alpha"], group["eps"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st, g = self.init_state(p), p.grad
                st["step"] += 1
                st["square_avg"].mul_(alpha).addcmul_(g, g, value=1 - alpha)
                p.addcdiv_(g, (st["square_avg"] + eps).sqrt(), value=-lr)
        return loss


def _optimizer_kind(optimizer, params):
    """(RR_A2C_* constant, None) for an optimizer ``rr_a2c_update`` steps, else (None, the reason). The
    optimizer's own options are judged before the tensors' device."""
    kinds = {RMSpropTFLike: _lib.RR_A2C_RMSPROP_TF, torch.optim.RMSprop: _lib.RR_A2C_RMSPROP,
             torch.optim.Adam: _lib.RR_A2C_ADAM}
    if type(optimizer) not in kinds:
        return None, ("the optimizer must be an RMSpropTFLike, a torch.optim.RMSprop or a torch.optim.Adam, not %s"
                      % type(optimizer).__name__)
    if len(optimizer.param_groups) != 1:
        return None, "the optimizer must have one parameter group"
    g = optimizer.param_groups[0]
    if {id(p) for p in g["params"]} != {id(p) for p in params} or len(params) > 16:
        return None, "the optimizer must be over exactly the policy's parameters"
    if type(optimizer) is torch.optim.RMSprop and (g.get("momentum", 0) != 0 or g.get("centered", False)
                                                   or g.get("weight_decay", 0) != 0):
        return None, "a torch.optim.RMSprop with momentum, centered or weight decay is not supported"
    if type(optimizer) is torch.optim.Adam and (g.get("amsgrad", False) or g.get("weight_decay", 0) != 0
                                                or torch.is_tensor(g["betas"][0])):
        return None, "a torch.optim.Adam with amsgrad, weight decay or tensor betas is not supported"
    if type(optimizer) is not RMSpropTFLike and (g.get("maximize", False) or not g.get("capturable", False)):
        return None, ("a %s must be capturable (its step count on the device) and not maximize"
                      % type(optimizer).__name__)
    if not all(p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda for p in params):
        return None, "the parameters must be contiguous fp32 tensors on the GPU, not CPU tensors"
    return kinds[type(optimizer)], None


def _coefficients(ent_coef, vf_coef, max_grad_norm):
    out = []
    for name, v in (("ent_coef", ent_coef), ("vf_coef", vf_coef),
                    ("max_grad_norm", 0.0 if max_grad_norm is None else max_grad_norm)):
        v = float(v)
        if not 0.0 <= v < float("inf"):
            raise ValueError("%s must be a finite number >= 0, not %r" % (name, v))
        out.append(v)
    return out


def _fused_reason(policy, optimizer, ro):
    """Why ``rr_a2c_update`` does not take this policy, optimizer and rollout; None if it does."""
    if isinstance(policy, MlpCategoricalActorCritic):
        return ("the fused A2C call takes the Gaussian MlpActorCritic; the Categorical A2C call is a follow-up "
                "(a2c_update(fused=False) runs its loss through autograd); it now exists under names of its own: "
                "a2c_discrete.A2CUpdateDiscrete, a2c_update_discrete and GraphedA2CDiscrete")
    if not fused_grad_supported(policy, ro.env.state_dim, ro.env.action_dim):
        return "the fused A2C call needs an MlpActorCritic with 64x64 towers and (obs, act) in ((14, 3), (7, 2))"
    reason = _optimizer_kind(optimizer, list(policy.parameters()))[1]
    if reason is None and not ro.obs.is_cuda:
        reason = "the fused A2C call needs a rollout on the GPU, not CPU tensors"
    return reason


def _check_rows(idx, n, dev):
    """``A2CUpdate.__call__``'s ``idx``: a contiguous 1-D int64 tensor of 2 .. ``n`` rows on ``dev``."""
    if (not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() != 1 or not 2 <= idx.numel() <= n
            or not idx.is_contiguous() or idx.device != dev):
        raise ValueError("idx must be None or a contiguous int64 device tensor of 2 .. n_steps * num_envs rows")


class A2CUpdate:
    """One ``A2C.train()`` as ONE library call (``rr_a2c_update``): the module's loss and its backward on
    fp32 MFMA, ``clip_grad_norm_`` and the optimizer's step on the optimizer's own state tensors. Four
    launches.

    ``optimizer`` is an ``RMSpropTFLike`` (SB3's default), a ``torch.optim.RMSprop(capturable=True)`` without
    momentum / centered / weight decay, or a capturable ``torch.optim.Adam`` (SB3's ``use_rms_prop=False``),
    over exactly the policy's parameters. It stays the source of truth: its ``square_avg`` (``exp_avg``,
    ``exp_avg_sq``) and ``step`` tensors are created here, as its first step would, if absent, and are
    updated in place. The gradient and state tensors must be kept (the library holds their addresses).

    ``__call__(idx=None)``: ``None`` is the whole rollout (SB3's ``rollout_buffer.get(batch_size=None)``);
    otherwise a contiguous int64 device tensor of 2 .. ``n_steps * num_envs`` rows of the flattened rollout.
    It writes ``p.grad`` (after the clip), steps the 13 parameters and returns ``stats`` (device, 8 floats:
    ``STAT_NAMES``). Stream-ordered and graph-capturable. ``lr`` is read from a device scalar that eager
    calls refresh from ``param_groups[0]["lr"]``; ``sync_lr()`` before replays of a captured graph.
    Reads ``ro.advantages`` and ``ro.returns`` and never ``ro.log_probs``. A Categorical policy is refused:
    ``a2c_discrete.A2CUpdateDiscrete`` is this class for it."""

    _call = "rr_a2c_update"  # A2CUpdateDiscrete: rr_a2c_update_discrete

    def __init__(self, policy, optimizer, ro, normalize_advantage=False, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5):
        self.ent_coef, self.vf_coef, self.max_norm = _coefficients(ent_coef, vf_coef, max_grad_norm)
        reason = _fused_reason(policy, optimizer, ro)
        if reason is not None:
            raise ValueError("A2CUpdate: " + reason)
        self._bind(policy, optimizer, ro, normalize_advantage, ro.env.action_dim, ro.env.action_dim)

    def _bind(self, policy, optimizer, ro, normalize_advantage, na, act_cols):
        """What the constructor does once the policy, optimizer and rollout have passed: the call's shape is
        ``(state_dim, na)`` and a row of ``ro.actions`` has ``act_cols`` floats."""
        self.normalize = bool(normalize_advantage)
        self.policy, self.opt = policy, optimizer
        self.kind = _optimizer_kind(optimizer, list(policy.parameters()))[0]
        ns = ro.env.state_dim
        n = ro.n_steps * ro.env.num_envs
        if n < 2:
            raise ValueError("%s needs a rollout of at least 2 rows" % type(self).__name__)
        self._lib = _lib.load()
        self.ns, self.na, self.n = ns, na, n
        dev = ro.obs.device
        self.data = [ro.obs.reshape(n, ns), ro.actions.reshape(n, act_cols), ro.advantages.reshape(n),
                     ro.returns.reshape(n)]
        for t in self.data:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("rollout tensors must be contiguous fp32")
        self.params = _policy_tensors(policy)
        _check_params(self._call, self.params, dev, "rollout")
        self._bind_state()
        self.ws, self._nbytes = _workspace(self._lib, self._call + "_workspace_size", dev, ns, na, n)
        self.stats = torch.zeros(_lib.RR_A2C_STAT_SLOTS, dtype=torch.float32, device=dev)
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sync_lr()
        self._all = torch.arange(n, dtype=torch.int64, device=dev)
        self.n_updates = 0

    def _bind_state(self):
        """The optimizer's own state tensors and the call's five pointer arrays (params, grads, square_avg
        or exp_avg_sq, exp_avg or NULL, step)."""
        opt, adam = self.opt, self.kind == _lib.RR_A2C_ADAM
        second = "exp_avg_sq" if adam else "square_avg"
        for p in self.params:
            st = opt.state[p]
            if not st:
                if type(opt) is RMSpropTFLike:
                    opt.init_state(p)
                else:  # what torch's first step creates for a capturable optimizer
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    if adam:
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st[second] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not torch.is_tensor(st["step"]) or not st["step"].is_cuda or st["step"].dtype != torch.float32:
                raise ValueError("%s needs the optimizer's device float32 step tensors" % type(self).__name__)
        self._tensors = [(p, p.grad, opt.state[p][second], opt.state[p]["exp_avg"] if adam else None,
                          opt.state[p]["step"]) for p in self.params]
        P = ctypes.c_void_p * len(self.params)
        self._ptrs = [P(*[t[k].data_ptr() for t in self._tensors]) if self._tensors[0][k] is not None else None
                      for k in range(5)]

    def sync_lr(self):
        self.lr.fill_(float(self.opt.param_groups[0]["lr"]))

    def _opt_args(self):
        """Before a call: refuses replaced tensors, refreshes ``lr`` unless capturing; returns the call's
        (optimizer, lr, alpha_or_beta1, beta2, eps)."""
        adam = self.kind == _lib.RR_A2C_ADAM
        second = "exp_avg_sq" if adam else "square_avg"
        for p, g, sq, m, s in self._tensors:
            st = self.opt.state[p]
            if p.grad is not g or st[second] is not sq or st["step"] is not s or (adam and st["exp_avg"] is not m):
                raise RuntimeError("a gradient or optimizer state tensor was replaced; %s holds their addresses"
                                   % type(self).__name__)
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        grp = self.opt.param_groups[0]
        a, b2 = grp["betas"] if adam else (grp["alpha"], 0.0)
        return self.kind, self.lr.data_ptr(), float(a), float(b2), float(grp["eps"])

    def __call__(self, idx=None):
        if idx is None:
            idx = self._all
        else:
            _check_rows(idx, self.n, self.ws.device)
        kind, lr, a, b2, eps = self._opt_args()
        _lib.check(getattr(self._lib, self._call)(self.ns, self.na, *self._ptrs, *[t.data_ptr() for t in self.data],
                                                  idx.data_ptr(), idx.numel(), int(self.normalize), self.ent_coef,
                                                  self.vf_coef, self.max_norm, kind, lr, a, b2, eps,
                                                  self.stats.data_ptr(), self.ws.data_ptr(), self._nbytes,
                                                  _stream(self.ws.device)), self._call)
        self.n_updates += 1
        return self.stats

    def last_stats(self):
        """The last call's five figures as a dict (one copy, which waits for the stream)."""
        return dict(zip(STAT_NAMES, self.stats.tolist()))

    def train_stats(self):
        """SB3 ``A2C.train``'s log figures for the last call (one copy of the statistics and one of
        ``log_std``, which wait for the stream)."""
        st = self.stats.tolist()
        return {"train/policy_loss": st[0], "train/value_loss": st[1], "train/entropy_loss": -st[2],
                "train/std": float(self.policy.log_std.detach().exp().mean()), "train/n_updates": self.n_updates}


def _a2c_loss(policy, obs, act, adv, ret, normalize_advantage, ent_coef, vf_coef):
    """SB3 1.6 ``A2C.train``'s loss in PyTorch ops on the whole rollout, with its figures (tensors)."""
    mean, value = policy(obs)
    lp = policy.log_prob(mean, act)
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg = -(adv * lp).mean()
    vf = torch.nn.functional.mse_loss(ret, value)
    if isinstance(policy, MlpCategoricalActorCritic):  # state dependent: from the logits (`mean` holds them)
        ent = policy.entropy(mean).mean()
    else:
        ent = policy.entropy(obs.shape[0]).mean()
    loss = pg + ent_coef * -ent + vf_coef * vf
    return loss, (pg, vf, ent, loss, lp.mean())


def a2c_update(policy, optimizer, ro, normalize_advantage=False, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
               fused=None):
    """One SB3 ``A2C.train()`` on the device-resident rollout: one gradient step on all
    ``n_steps * num_envs`` rows. Returns the five figures (``STAT_NAMES``) as a dict of floats.

    ``fused=None`` takes ``A2CUpdate`` (``rr_a2c_update``) where it applies: an ``MlpActorCritic`` with
    64x64 towers, a rollout on the GPU, and an ``RMSpropTFLike``, a plain capturable
    ``torch.optim.RMSprop`` or a capturable ``torch.optim.Adam`` over its parameters. Otherwise, and with
    ``fused=False``, the same loss runs through PyTorch autograd, then ``clip_grad_norm_`` and
    ``optimizer.step()``: the path for CPU tensors, any other policy (``policy(obs)`` gives ``(mean,
    value)``; ``log_prob``; ``entropy``), a Categorical one included, and any other optimizer.
    ``fused=True`` where the call does not apply raises and names the reason. A loop should hold an
    ``A2CUpdate`` (or a ``GraphedA2C``) instead: this function builds one per call."""
    ent_coef, vf_coef, max_norm = _coefficients(ent_coef, vf_coef, max_grad_norm)
    reason = _fused_reason(policy, optimizer, ro)
    if fused is None:
        fused = reason is None
    if fused and reason is not None:
        raise ValueError("a2c_update(fused=True): " + reason)
    if fused:
        step = A2CUpdate(policy, optimizer, ro, normalize_advantage, ent_coef, vf_coef, max_grad_norm)
        step()
        return step.last_stats()
    n = ro.n_steps * ro.env.num_envs
    loss, figures = _a2c_loss(policy, ro.obs.reshape(n, -1), ro.actions.reshape(n, -1), ro.advantages.reshape(n),
                              ro.returns.reshape(n), normalize_advantage, ent_coef, vf_coef)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    if max_norm > 0.0:
        torch.nn.utils.clip_grad_norm_(policy.parameters(), max_norm)
    optimizer.step()
    return {k: float(v.detach()) for k, v in zip(STAT_NAMES, figures)}


class GraphedA2C:
    """A whole A2C iteration, ``ro.collect()`` followed by ``A2CUpdate`` on all its rows, captured ONCE on
    one stream into one hipGraph; ``step()`` replays it. The graph is a linear chain (the policy's packing,
    the one-launch collect, its iteration counter, and the update's four launches), and a replay needs no
    host work: ``lr`` is read from a device scalar that ``step()`` refreshes from ``param_groups[0]["lr"]``.

    Needs the one-launch collect (``DeviceRollout`` with the fused policy on an RK4 / Euler batch, not
    ``per_step``) and what ``A2CUpdate`` needs. The warm-up iteration the capture requires runs on a side
    stream on the real env, rollout, parameters and optimizer state, and is undone in place (the env through
    its ``checkpoint()`` / ``restore()`` and its output buffers), so the first ``step()`` starts where an
    eager ``ro.collect(); update()`` would and computes the same bits. ``update`` is the ``A2CUpdate``;
    ``train_stats()`` is its. A Categorical policy is refused: ``a2c_discrete.GraphedA2CDiscrete`` is this
    class for it."""

    def __init__(self, policy, optimizer, ro, normalize_advantage=False, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5):
        _coefficients(ent_coef, vf_coef, max_grad_norm)
        reason = _fused_reason(policy, optimizer, ro)
        if reason is not None:
            raise ValueError("GraphedA2C: " + reason)
        if not (getattr(ro, "fused", False) and getattr(ro, "one_launch", False)) or getattr(ro, "per_step", True):
            raise ValueError("GraphedA2C needs the one-launch collect (fused policy, RK4 / Euler env, not per_step)")
        self._capture(ro, A2CUpdate(policy, optimizer, ro, normalize_advantage, ent_coef, vf_coef, max_grad_norm))

    def _capture(self, ro, update):
        """The warm-up iteration, the put-back and the capture of ``ro.collect(); update()``."""
        optimizer = update.opt
        self.ro = ro
        self.update = update
        env, dev = ro.env, ro.obs.device
        # what one iteration writes and the next one reads, to put back after the warm-up
        torch.cuda.synchronize(dev)
        ck = {k: v.clone() for k, v in env.checkpoint().items()}
        keep = [t for t in (env.obs, env.reward, env.done, env.truncated, env.terms, ro.iter, ro.last_value,
                            ro.last_done, ro.last_start) if torch.is_tensor(t)]
        for p in self.update.params:
            keep += [p, p.grad] + [v for v in optimizer.state[p].values() if torch.is_tensor(v)]
        if getattr(ro, "stats", None) is not None:
            keep += [ro.stats.out, ro.stats.accum]
        saved = [t.detach().clone() for t in keep]
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._iteration()
        torch.cuda.current_stream(dev).wait_stream(side)

        def put_back():
            with torch.no_grad():
                env.restore(ck)
                for t, v in zip(keep, saved):
                    t.copy_(v)

        put_back()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.stats = self._iteration()
        put_back()  # the capture ran nothing; the eager side of it counted a call
        self.update.n_updates = 0
        torch.cuda.synchronize(dev)

    def _iteration(self):
        self.ro.collect()
        return self.update()

    def step(self):
        """One iteration: the replay. Returns the update's ``stats`` tensor (device)."""
        self.update.sync_lr()
        self.graph.replay()
        self.update.n_updates += 1
        return self.stats

    def train_stats(self):
        return self.update.train_stats()
