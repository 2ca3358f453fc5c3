"""The PPO learner on a ``DeviceRollout``'s buffers: SB3 1.6 ``PPO.train`` in PyTorch ops
(``ppo_update``), its loss + backward and its clip + Adam step as HIP launches (``PPOGrad``,
``ClipAdam``), the whole minibatch step as one library call (``PPOUpdate``) and an epoch of steps
captured into a hipGraph (``GraphedPPOUpdate``). ``_AdamState`` is the binding of the 13 policy
tensors and a capturable Adam's state that the fused calls share with ``bc.BCUpdate``.
``PPOUpdate`` serves both distributions: for a ``MlpCategoricalActorCritic`` its constructor chooses
``rr_ppo_update_discrete`` (``rr_ppo_update_discrete_opts`` with an option or ``train_stats``),
``(ns, n_choices)`` as the shape, the actions as ``[n]`` indices and the policy's 12 tensors;
``__call__`` is the same. ``PPOUpdateDiscrete`` is that path under its own name. ``ppo_update`` and
``GraphedPPOUpdate`` share their refusals (``_refuse_options``) and build the whole-minibatch step
through ``_whole_step``.
"""
import ctypes

import torch

from . import _lib
from .policy import MlpCategoricalActorCritic, _policy_tensors, fused_discrete_supported, fused_grad_supported


def _check_params(who, params, dev, whose):
    """Contiguous fp32 parameters on ``dev``, ``whose`` device it is; ``.grad`` allocated where
    absent (the library call ``who`` is given its address and overwrites it)."""
    for p in params:
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
            raise ValueError("%s needs contiguous fp32 parameters on the %s device" % (who, whose))
        if p.grad is None:
            p.grad = torch.zeros_like(p)


def _check_idx(t, bs, dev, flat=False, what="idx must be a contiguous int64 device tensor"):
    if (t.dtype != torch.int64 or (flat and t.dim() != 1) or not 2 <= t.numel() <= bs or not t.is_contiguous()
            or t.device != dev):
        raise ValueError(what + " of 2 .. batch_size rows")


def _workspace(lib, size, dev, *shape):
    """(workspace tensor, its byte count) as the library's ``size`` symbol asks for ``shape``."""
    nbytes = ctypes.c_int64()
    _lib.check(getattr(lib, size)(*shape, ctypes.byref(nbytes)), size)
    return torch.empty((nbytes.value + 15) // 16 * 4, dtype=torch.float32, device=dev), nbytes.value


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _AdamState:
    """What ``ClipAdam``, ``PPOUpdate`` and ``BCUpdate`` share: the ``(param, grad, exp_avg,
    exp_avg_sq, step)`` tensors of a capturable ``torch.optim.Adam`` and their five pointer arrays
    (``_params_w`` / ``_dst`` / ``_m`` / ``_v`` / ``_s``), and the ``lr`` device scalar. The
    optimizer stays the source of truth: its state tensors are created here, as Adam's first step
    would, if absent, and are updated in place by the calls."""

    def _bind_adam(self, optimizer, params):
        self.opt, who = optimizer, type(self).__name__
        dev = params[0].device
        for p in params:
            st = optimizer.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not st["step"].is_cuda or st["step"].dtype != torch.float32:
                raise ValueError("%s needs the capturable Adam's device float32 step tensors" % who)
        self._tensors = [(p, p.grad, optimizer.state[p]["exp_avg"], optimizer.state[p]["exp_avg_sq"],
                          optimizer.state[p]["step"]) for p in params]
        P = ctypes.c_void_p * len(params)
        self._ptrs = [P(*[t[k].data_ptr() for t in self._tensors]) for k in range(5)]
        self._params_w, self._dst, self._m, self._v, self._s = self._ptrs
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sync_lr()

    def sync_lr(self):
        self.lr.fill_(float(self.opt.param_groups[0]["lr"]))

    def _adam_args(self):
        """Before a call: refuses replaced tensors, refreshes ``lr`` unless capturing; returns the
        call's (lr, beta1, beta2, eps)."""
        for p, g, m, v, s in self._tensors:
            st = self.opt.state[p]
            if p.grad is not g or st["exp_avg"] is not m or st["exp_avg_sq"] is not v or st["step"] is not s:
                raise RuntimeError("a gradient or Adam state tensor was replaced; %s holds their addresses"
                                   % type(self).__name__)
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        grp = self.opt.param_groups[0]
        b1, b2 = grp["betas"]
        return self.lr.data_ptr(), float(b1), float(b2), float(grp["eps"])


def _allreduce_grads(params, group):
    """Average the gradients of `params` over the ranks of `group` with ONE all_reduce of a
    flat buffer (the 64x64 MlpPolicy is ~10.6 k parameters: a single 42 KB message per
    minibatch, RCCL over xGMI with the "nccl" backend)."""
    import torch.distributed as dist

    grads = [p.grad for p in params if p.grad is not None]
    flat = torch.cat([g.reshape(-1) for g in grads])
    if flat.is_cuda and dist.get_backend(group) == "gloo":  # CPU rehearsal of the N > 1 path
        host = flat.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        flat.copy_(host)
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat /= dist.get_world_size(group)
    k = 0
    for g in grads:
        g.copy_(flat[k:k + g.numel()].view_as(g))
        k += g.numel()


class PPOGrad:
    """The PPO minibatch loss + backward as ONE HIP pipeline (``rr_ppo_grad``: fp32 MFMA forward
    and backward of both towers over the gathered minibatch, fixed-order workgroup sums).

    ``__call__(idx)`` WRITES ``p.grad`` of the policy's 13 parameters (allocated here once and
    kept: the library holds their addresses, so do not set them to None — use
    ``zero_grad(set_to_none=False)`` or none at all, the call overwrites) for the minibatch
    ``idx`` (int64 device tensor of 2 .. ``batch_size`` rows of the flattened rollout) and fills
    ``stats`` = [policy_loss, value_loss, entropy, clip_fraction, approx_kl]. Same loss as
    ``ppo_update`` (SB3 1.6 PPO.train); gradients equal autograd's to fp32 rounding
    (``tests/test_gpu_ppo.py``). Stream-ordered on the current stream; graph-capturable."""

    def __init__(self, policy, ro, batch_size, clip_range=0.2, ent_coef=0.01, vf_coef=0.5):
        ns, na = ro.env.state_dim, ro.env.action_dim
        if not fused_grad_supported(policy, ns, na):
            raise ValueError("PPOGrad needs an MlpActorCritic with 64x64 towers and (obs, act) in ((14, 3), (7, 2))")
        dev = self._bind_rollout("rr_ppo_grad", policy, ro, batch_size, (ns, na), (na,), clip_range, ent_coef, vf_coef)
        self.ws, self._nbytes = _workspace(self._lib, "rr_ppo_workspace_size", dev, ns, na, self.bs)
        self._src = (ctypes.c_void_p * 13)(*[p.data_ptr() for p in self.params])
        self._grads = [p.grad for p in self.params]
        self._dst = (ctypes.c_void_p * 13)(*[g.data_ptr() for g in self._grads])

    def _bind_rollout(self, who, policy, ro, batch_size, shape, act_shape, clip_range, ent_coef, vf_coef):
        """What a learner call reads, for the library call ``who``: its shape arguments (``ns`` / ``na``), the
        flattened rollout (actions as ``[n, *act_shape]``: ``[n, na]``, or ``[n]`` for indices), the policy's
        tensors, the coefficients and ``stats``. Returns the rollout's device."""
        n = ro.n_steps * ro.env.num_envs
        if not 2 <= batch_size <= n:
            raise ValueError("batch_size must be in [2, n_steps * num_envs]")
        self._lib = _lib.load()
        (self.ns, self.na), self.bs = shape, int(batch_size)
        self.coef = (float(clip_range), float(ent_coef), float(vf_coef))
        dev = ro.obs.device
        self.data = [ro.obs.reshape(n, self.ns), ro.actions.reshape(n, *act_shape), ro.log_probs.reshape(n),
                     ro.advantages.reshape(n), ro.returns.reshape(n)]
        for t in self.data:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("rollout tensors must be contiguous fp32")
        self.params = _policy_tensors(policy)
        _check_params(who, self.params, dev, "rollout")
        self.stats = torch.zeros(5, dtype=torch.float32, device=dev)
        return dev

    def __call__(self, idx):
        _check_idx(idx, self.bs, self.ws.device)
        for p, g in zip(self.params, self._grads):
            if p.grad is not g:
                raise RuntimeError("a parameter's .grad was replaced; PPOGrad writes into the tensors it allocated")
        clip, ent, vf = self.coef
        o, a, lp, adv, ret = self.data
        _lib.check(self._lib.rr_ppo_grad(self.ns, self.na, self._src, self._dst, o.data_ptr(), a.data_ptr(),
                                         lp.data_ptr(), adv.data_ptr(), ret.data_ptr(), idx.data_ptr(), idx.numel(),
                                         clip, ent, vf, self.stats.data_ptr(), self.ws.data_ptr(), self._nbytes,
                                         _stream(self.ws.device)), "rr_ppo_grad")
        return self.stats


def clip_adam_supported(optimizer, params):
    if type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
        return False
    g = optimizer.param_groups[0]
    if {id(p) for p in g["params"]} != {id(p) for p in params} or len(params) > 16:
        return False
    return (g.get("capturable", False) and not g.get("amsgrad", False) and not g.get("maximize", False)
            and g.get("weight_decay", 0) == 0 and not torch.is_tensor(g["betas"][0])
            and all(p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda for p in params))


class ClipAdam(_AdamState):
    """``clip_grad_norm_(params, max_grad_norm)`` + ``optimizer.step()`` for a
    ``torch.optim.Adam(capturable=True)`` in two launches (``rr_clip_adam``), on the optimizer's own
    state tensors (created here, as Adam's first step would, if absent), so the optimizer object
    stays the source of truth (state_dict, later eager steps). The learning rate is read from a
    device scalar that ``__call__`` refreshes from ``param_groups[0]["lr"]`` when called eagerly;
    inside a captured graph call ``sync_lr()`` before replays (GraphedPPOUpdate.update does)."""

    def __init__(self, optimizer, params, max_grad_norm):
        if not clip_adam_supported(optimizer, params):
            raise ValueError("ClipAdam needs a capturable torch.optim.Adam over exactly these fp32 CUDA parameters "
                             "(one group, no weight decay / amsgrad / maximize, <= 16 tensors)")
        self.params = list(params)
        self.max_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
        for p in self.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        self._bind_adam(optimizer, self.params)
        self._numel = (ctypes.c_int64 * len(self.params))(*[p.numel() for p in self.params])
        self._lib = _lib.load()
        self._ws, self._nbytes = _workspace(self._lib, "rr_clip_adam_workspace_size", self.lr.device,
                                            sum(p.numel() for p in self.params))

    def __call__(self):
        _lib.check(self._lib.rr_clip_adam(len(self.params), *self._ptrs, self._numel, self.max_norm,
                                          *self._adam_args(), self._ws.data_ptr(), self._nbytes,
                                          _stream(self.lr.device)), "rr_clip_adam")


def _ppo_options(clip_range_vf, normalize_advantage, target_kl):
    """SB3's three PPO.__init__ options as (clip_range_vf or 0.0, bool, target_kl or 0.0); None
    switches the first and the last off, a number must be finite and > 0."""
    out = []
    for name, v in (("clip_range_vf", clip_range_vf), ("target_kl", target_kl)):
        if v is None:
            out.append(0.0)
            continue
        v = float(v)
        if not (0.0 < v < float("inf")):
            raise ValueError("%s must be None or a finite number > 0, not %r" % (name, v))
        out.append(v)
    return out[0], bool(normalize_advantage), out[1]


def _old_values(ro, n):
    v = getattr(ro, "values", None)
    if v is None:
        raise ValueError("clip_range_vf needs the rollout's values (ro.values)")
    v = v.reshape(n)
    if not v.is_contiguous() or v.dtype != torch.float32:
        raise ValueError("rollout tensors must be contiguous fp32")
    return v


def _train_stats(ctl):
    """SB3 PPO.train's log means from a control block read to the host (rocket_hip.h RR_PPO_CTL_*)."""
    L = _lib
    n = max(ctl[L.RR_PPO_CTL_EVALS], 1.0)
    stopped = ctl[L.RR_PPO_CTL_STOP] != 0.0
    return {"train/policy_gradient_loss": ctl[L.RR_PPO_CTL_SUM_POLICY] / n,
            "train/value_loss": ctl[L.RR_PPO_CTL_SUM_VALUE] / n,
            "train/entropy_loss": -ctl[L.RR_PPO_CTL_SUM_ENTROPY] / n,
            "train/clip_fraction": ctl[L.RR_PPO_CTL_SUM_CLIP] / n,
            "train/approx_kl": ctl[L.RR_PPO_CTL_KL_SUM] / max(ctl[L.RR_PPO_CTL_KL_COUNT], 1.0),
            "train/n_minibatches": int(ctl[L.RR_PPO_CTL_STEPS]),
            "train/n_evaluated": int(ctl[L.RR_PPO_CTL_EVALS]),
            "train/early_stop": bool(stopped),
            "train/stop_epoch": int(ctl[L.RR_PPO_CTL_EPOCHS]) - 1 if stopped else None}


_DISCRETE_FUSED = ("the fused Categorical learner (rr_ppo_update_discrete, rr_ppo_update_discrete_opts) is the "
                   "one-replica call with a capturable torch.optim.Adam: %s needs fused=False (the autograd path "
                   "takes it)")


def _discrete_fused_ok(group, one_call, cvf, norm, tkl, train_stats=False):
    """Refuses what ``fused=True`` does not take for a Categorical policy, before any device work: a
    ``group``, and an optimizer that is no capturable CUDA Adam over the policy's parameters (named by
    the option that asked for the fused call, if there is one)."""
    if group is not None:
        raise ValueError(_DISCRETE_FUSED % "group=")
    if not one_call:
        what = ("clip_range_vf" if cvf else "normalize_advantage=False" if not norm else "target_kl" if tkl
                else "train_stats" if train_stats else None)
        raise ValueError(_DISCRETE_FUSED % ("%s with another optimizer" % what if what else "another optimizer"))


class PPOUpdate(PPOGrad, _AdamState):
    """A whole PPO minibatch step — ``PPOGrad`` then ``ClipAdam``'s clip + Adam step on the same 13
    tensors — as ONE library call (``rr_ppo_update``). Without a gradient all_reduce between the
    two halves, the clip's norm is summed by the gradient finish. The optimizer launch also repacks
    the towers for the next call and sums the next minibatch's advantage statistics. A chain of
    minibatches therefore takes three launches each instead of five; the first takes four.

    ``__call__(idx, next_idx=None, chained=False)``:
      * ``chained=True`` says that the previous call on this object was given ``next_idx=idx`` and
        that nothing else has written the parameters since.
      * The optimizer is the source of truth, as with ``ClipAdam``: its exp_avg / exp_avg_sq /
        step tensors are updated in place.
      * ``lr`` is read from a device scalar. ``sync_lr()`` refreshes it, and eager calls do so
        themselves.

    SB3's ``clip_range_vf``, ``normalize_advantage=False`` and ``target_kl`` (None / True / None:
    today's ``rr_ppo_update`` calls, unchanged), or ``train_stats=True``, take the same step through
    ``rr_ppo_update_opts`` (``rr_ppo_update_discrete_opts`` for a Categorical policy). That call
    carries a control block on the device (``self.ctl``):
      * ``reset()`` clears it; call it before the first minibatch of a ``train()``-like pass and pass
        ``epoch_start=True`` with every epoch's first minibatch.
      * With ``target_kl``, the minibatch whose ``approx_kl > 1.5 target_kl`` takes no optimizer
        step, and every later call is a no-op until ``reset()``. That is SB3's ``break``, without a
        host read.
      * ``train_stats()`` reads the block (one copy, which waits for the stream) and returns SB3's
        ``train/*`` means over the pass."""

    _categorical = False  # PPOUpdateDiscrete: a Categorical policy only

    def __init__(self, policy, optimizer, ro, batch_size, clip_range=0.2, ent_coef=0.01, vf_coef=0.5,
                 max_grad_norm=0.5, clip_range_vf=None, normalize_advantage=True, target_kl=None, train_stats=False):
        who = type(self).__name__
        cvf, norm, tkl = _ppo_options(clip_range_vf, normalize_advantage, target_kl)
        self.opts = (_lib.RrPpoOptions(cvf, tkl, int(norm), int(bool(train_stats)))
                     if cvf or tkl or not norm or train_stats else None)
        if not clip_adam_supported(optimizer, list(policy.parameters())):
            raise ValueError("%s needs a capturable torch.optim.Adam over the policy's parameters "
                             "(one group, no weight decay / amsgrad / maximize)" % who)
        if self._categorical or isinstance(policy, MlpCategoricalActorCritic):
            # what differs: the calls, (ns, n_choices) as their shape, the actions as [n] indices
            ns = ro.env.state_dim
            if not fused_discrete_supported(policy, ns):
                raise ValueError("%s needs an MlpCategoricalActorCritic with 64x64 towers and 2 .. 4 "
                                 "choices on a 3DOF rollout" % who)
            self._call = "rr_ppo_update_discrete" if self.opts is None else "rr_ppo_update_discrete_opts"
            dev = self._bind_rollout(self._call, policy, ro, batch_size, (ns, policy.n_choices), (), clip_range,
                                     ent_coef, vf_coef)
        else:
            self._call = "rr_ppo_update" if self.opts is None else "rr_ppo_update_opts"
            super().__init__(policy, ro, batch_size, clip_range, ent_coef, vf_coef)
            dev = self.ws.device
        self.max_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
        self._bind_adam(optimizer, self.params)
        self.ws, self._nbytes = _workspace(self._lib, self._call + "_workspace_size", dev, self.ns, self.na, self.bs)
        self._next = None
        self.ctl = self.old_values = None
        if self.opts is not None:
            self.ctl = torch.zeros(_lib.RR_PPO_CTL_SLOTS, dtype=torch.float32, device=dev)
            if cvf:
                self.old_values = _old_values(ro, self.data[0].shape[0])
        # the call's leading arguments, the same every time: the shape, the five pointer arrays, the rollout
        # (rr_ppo_update_opts, rr_ppo_update_discrete_opts: old_values after it)
        self._head = [self.ns, self.na, *self._ptrs, *[t.data_ptr() for t in self.data]]
        if self.opts is not None:
            self._head.append(None if self.old_values is None else self.old_values.data_ptr())

    def reset(self):
        """Clear the control block (stream-ordered, no wait): a new ``train()`` pass begins."""
        if self.ctl is None:
            raise ValueError("this PPOUpdate has no control block (no option and no train_stats)")
        self.ctl.zero_()

    def train_stats(self):
        if self.ctl is None:
            raise ValueError("train_stats() needs PPOUpdate(train_stats=True) or one of the options")
        return _train_stats(self.ctl.tolist())

    def __call__(self, idx, next_idx=None, chained=False, epoch_start=False):
        if epoch_start and self.opts is None:
            raise ValueError("epoch_start belongs to the control block (no option and no train_stats here)")
        for t in (idx,) if next_idx is None else (idx, next_idx):
            _check_idx(t, self.bs, self.ws.device, False, "idx / next_idx must be contiguous int64 device tensors")
        if next_idx is not None and next_idx.numel() > idx.numel():
            raise ValueError("next_idx may not be longer than idx")
        if chained and self._next != (idx.data_ptr(), idx.numel()):
            raise ValueError("chained=True needs the previous call on this %s to have had next_idx=idx"
                             % type(self).__name__)
        nxt = None if next_idx is None else (next_idx.data_ptr(), next_idx.numel())
        step = [idx.data_ptr(), idx.numel(), *(nxt or (None, 0)), *self.coef, self.max_norm, *self._adam_args()]
        flags = _lib.RR_PPO_CHAINED if chained else 0
        if self.opts is not None:  # rr_ppo_update's arguments with the options' among them
            step += [ctypes.byref(self.opts), self.ctl.data_ptr()]
            flags |= _lib.RR_PPO_EPOCH_START if epoch_start else 0
        _lib.check(getattr(self._lib, self._call)(*self._head, *step, self.stats.data_ptr(), flags, self.ws.data_ptr(),
                                                  self._nbytes, _stream(self.ws.device)), self._call)
        self._next = nxt  # (address, rows) of this call's next_idx: what chained=True may follow
        return self.stats


class PPOUpdateDiscrete(PPOUpdate):
    """``PPOUpdate`` for a ``MlpCategoricalActorCritic`` on a 3DOF rollout, under the name and with the
    constructor it had as a class of its own: one PPO minibatch step with a Categorical distribution as
    ONE library call (``rr_ppo_update_discrete``: the learner's towers with a softmax head, the
    entropy's gradient per sample, clip + Adam over the policy's 12 tensors). ``stats[2]`` is the
    minibatch's mean entropy. ``clip_range_vf``, ``normalize_advantage=False``, ``target_kl`` and
    ``train_stats=True`` are ``PPOUpdate``'s (``rr_ppo_update_discrete_opts``, with the control block,
    ``reset()``, ``train_stats()`` and ``epoch_start=``); without them ``opts`` is None and the call is
    ``rr_ppo_update_discrete``."""

    _categorical = True

    def __init__(self, policy, optimizer, ro, batch_size, clip_range=0.2, ent_coef=0.01, vf_coef=0.5,
                 max_grad_norm=0.5, clip_range_vf=None, normalize_advantage=True, target_kl=None, train_stats=False):
        super().__init__(policy, optimizer, ro, batch_size, clip_range, ent_coef, vf_coef, max_grad_norm,
                         clip_range_vf, normalize_advantage, target_kl, train_stats)


def _whole_step(policy, optimizer, ro, batch_size, *coef_and_options):
    """The chained whole-minibatch call of the one-replica path (clip_range, ent_coef, vf_coef,
    max_grad_norm, then ``PPOUpdate``'s options): ``PPOUpdateDiscrete`` for a Categorical policy."""
    if isinstance(policy, MlpCategoricalActorCritic):
        return PPOUpdateDiscrete(policy, optimizer, ro, batch_size, *coef_and_options)
    return PPOUpdate(policy, optimizer, ro, batch_size, *coef_and_options)


def _refuse_options(policy, optimizer, group, fused, cvf, norm, tkl, train_stats=False, graphed=False):
    """What ``ppo_update`` and ``GraphedPPOUpdate`` (``graphed``) refuse, before any device work. Returns
    whether the step is the one-call path: fused, one replica, a capturable Adam."""
    one_call = bool(fused) and group is None and clip_adam_supported(optimizer, list(policy.parameters()))
    if fused and isinstance(policy, MlpCategoricalActorCritic):
        _discrete_fused_ok(group, one_call, cvf, norm, tkl, train_stats)
    if tkl and group is not None:
        raise ValueError("target_kl with a group is not supported: the ranks would stop at different minibatches")
    if graphed and not one_call and (train_stats or tkl or (fused and (cvf or not norm))):
        raise ValueError("clip_range_vf / normalize_advantage=False on the fused path, target_kl and train_stats "
                         "need the fused one-replica update with a capturable torch.optim.Adam "
                         "(rr_ppo_update_opts); fused=False takes clip_range_vf and normalize_advantage only")
    if not graphed and fused and not one_call and (cvf or tkl or not norm):
        raise ValueError("fused=True takes clip_range_vf / normalize_advantage=False / target_kl only on the "
                         "one-replica path with a capturable torch.optim.Adam (rr_ppo_update_opts), not with a "
                         "group or another optimizer")
    return one_call


def _loss_stats(st):
    """A call's first three statistics under ``ppo_update``'s keys."""
    return {"policy_loss": st[0], "value_loss": st[1], "entropy": st[2]}


def _epoch_perms(n, n_epochs, dev, generator=None):
    """The epochs' permutations for the fused updates, each later one drawn on a side stream
    while the caller runs the previous epoch on the current stream (torch's randperm at 1 M rows
    is a ~0.25 ms chain of small sort launches). Same draws, same order, same generator as a
    sequential loop of torch.randperm calls; each yielded tensor is ready on the current stream."""
    if n_epochs <= 0:
        return
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    nxt = torch.randperm(n, device=dev, generator=generator)
    for e in range(n_epochs):
        perm, ready = nxt, None
        if e + 1 < n_epochs:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                nxt = torch.randperm(n, device=dev, generator=generator)
                ready = side.record_event()
        yield perm
        if ready is not None:
            main.wait_event(ready)
            nxt.record_stream(main)  # drawn on the side stream, read on this one


def _ppo_loss(policy, obs, act, old_lp, adv, ret, old_v, n_rows, clip_range, ent_coef, vf_coef, cvf, norm):
    """SB3 1.6 PPO.train's minibatch loss in PyTorch ops on the gathered rows (``old_v`` is read with
    ``cvf`` only): the loss, its three detached figures, and the log-probs and ratio the callers
    take the KL and the clip fraction from."""
    mean, value = policy(obs)
    lp = policy.log_prob(mean, act)
    if norm:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old_lp)
    pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    if cvf:
        value = old_v + torch.clamp(value - old_v, -cvf, cvf)
    vf = torch.nn.functional.mse_loss(ret, value)
    if isinstance(policy, MlpCategoricalActorCritic):  # state dependent: from the logits (`mean` holds them)
        ent = -policy.entropy(mean).mean()
    else:
        ent = -policy.entropy(n_rows).mean()
    loss = pg + ent_coef * ent + vf_coef * vf
    return loss, {"policy_loss": pg.detach(), "value_loss": vf.detach(), "entropy": -ent.detach()}, lp, ratio


def ppo_update(policy, optimizer, ro, n_epochs=10, batch_size=65536, clip_range=0.2, ent_coef=0.01,
               vf_coef=0.5, max_grad_norm=0.5, generator=None, group=None, fused=False, clip_range_vf=None,
               normalize_advantage=True, target_kl=None):
    """SB3 1.6 PPO.train on the device-resident rollout (advantage normalisation per
    minibatch, clipped surrogate, unclipped value loss, entropy bonus, grad-norm clip).
    ent_coef 0.01 as main_6DOF.py:68.

    Multi-GPU (one policy replica per GPU): with a torch.distributed `group`
    every rank collects from its own env shard and updates on its own rollout; the
    minibatch gradients are averaged over the ranks (one all_reduce) before the grad-norm
    clip and the optimizer step, so replicas that start equal stay equal. Ranks must run
    the same number of minibatches (equal shard sizes); advantages are normalised per
    rank's minibatch.

    ``fused=True``: the loss + backward of every minibatch is ``PPOGrad`` (one HIP pipeline)
    instead of PyTorch autograd, and for a capturable Adam the clip + optimizer step is
    ``ClipAdam`` (one launch) on the optimizer's own state; the all_reduce is unchanged.

    ``clip_range_vf`` / ``normalize_advantage`` / ``target_kl`` are SB3's (None / True / None: its
    defaults, and this function's behaviour without them). The autograd path implements all three,
    ``target_kl`` with SB3's ``break``. ``fused=True`` takes them on the one-replica path with a
    capturable Adam (``PPOUpdate``: ``rr_ppo_update_opts``, the stop carried on the device) and
    refuses them elsewhere. ``target_kl`` with a ``group`` is refused everywhere: every rank would
    decide on its own minibatch's KL.

    A ``MlpCategoricalActorCritic`` (discrete 3DOF actions): the autograd path takes everything above,
    with the entropy from the logits. ``fused=True`` is ``PPOUpdateDiscrete``
    (``rr_ppo_update_discrete``, chained) and needs a capturable Adam and no ``group``;
    ``clip_range_vf``, ``normalize_advantage=False`` and ``target_kl`` put it on
    ``rr_ppo_update_discrete_opts``, the stop carried on the device as for the Gaussian policy."""
    n = ro.n_steps * ro.env.num_envs
    cvf, norm, tkl = _ppo_options(clip_range_vf, normalize_advantage, target_kl)
    one_call = _refuse_options(policy, optimizer, group, fused, cvf, norm, tkl)
    if fused:
        perms = _epoch_perms(n, n_epochs, ro.obs.device, generator)
        if n % min(batch_size, n) == 1:
            # checked before the first minibatch: a 1-row remainder cannot be normalised (PPOGrad
            # refuses it) and failing there would leave the epoch's earlier Adam steps applied
            raise ValueError("n_steps * num_envs = %d leaves a 1-row last minibatch at batch_size %d (rr_ppo_grad "
                             "needs >= 2 rows); choose another batch_size" % (n, batch_size))
        params = list(policy.parameters())
        stats = None
        if one_call:
            # the whole minibatch step in one call, chained: each call sums the next one's statistics
            step = _whole_step(policy, optimizer, ro, min(batch_size, n), clip_range, ent_coef, vf_coef, max_grad_norm,
                               clip_range_vf, normalize_advantage, target_kl)
            kw = {}
            for perm in perms:
                for s in range(0, n, step.bs):
                    nxt = perm[s + step.bs:s + 2 * step.bs] if s + step.bs < n else None
                    if step.opts is not None:
                        kw = dict(epoch_start=s == 0)
                    stats = step(perm[s:s + step.bs], nxt, chained=s > 0, **kw)
            return {} if stats is None else _loss_stats(stats.tolist())
        grad = PPOGrad(policy, ro, min(batch_size, n), clip_range, ent_coef, vf_coef)
        adam = ClipAdam(optimizer, params, max_grad_norm) if clip_adam_supported(optimizer, params) else None
        for perm in perms:
            for s in range(0, n, grad.bs):
                stats = grad(perm[s:s + grad.bs])
                if group is not None:
                    _allreduce_grads(params, group)
                if adam is not None:
                    adam()
                else:
                    torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
                    optimizer.step()
        return {} if stats is None else _loss_stats(stats.tolist())
    obs = ro.obs.reshape(n, -1)
    act = ro.actions.reshape(n, -1)
    old_lp = ro.log_probs.reshape(n)
    adv_all = ro.advantages.reshape(n)
    ret = ro.returns.reshape(n)
    old_v = ro.values.reshape(n) if cvf else None
    stats = {}
    stop = False
    for _ in range(n_epochs):
        if stop:
            break
        perm = torch.randperm(n, device=obs.device, generator=generator)
        for s in range(0, n, batch_size):
            idx = perm[s:s + batch_size]
            old = old_lp[idx]
            loss, stats, lp, _ = _ppo_loss(policy, obs[idx], act[idx], old, adv_all[idx], ret[idx],
                                           old_v[idx] if cvf else None, len(idx), clip_range, ent_coef, vf_coef, cvf, norm)
            if tkl:
                with torch.no_grad():
                    log_ratio = lp - old
                    kl = float(((torch.exp(log_ratio) - 1) - log_ratio).mean())
                if kl > 1.5 * tkl:  # SB3: the minibatch's losses are logged, its step is not taken
                    stop = True
                    break
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            if group is not None:
                _allreduce_grads(list(policy.parameters()), group)
            torch.nn.utils.clip_grad_norm_(policy.parameters(), max_grad_norm)
            optimizer.step()
    return {k: float(v) for k, v in stats.items()}


class GraphedPPOUpdate:
    """``ppo_update``'s minibatch step — gather, forward, clipped-surrogate / value / entropy
    loss, backward, (multi-GPU gradient all_reduce), grad-norm clip, Adam step — captured ONCE
    into a hipGraph — one graph per EPOCH: the minibatch steps of one pass over the rollout,
    each reading its rows from a static permutation buffer that ``update`` refills with
    ``torch.randperm`` before every replay (no per-minibatch index copy or graph launch).

    ``fused`` (default: wherever ``PPOGrad`` supports the policy) takes the loss + backward from
    ``PPOGrad`` (rr_ppo_grad: one fp32-MFMA HIP pipeline) instead of PyTorch autograd, whose
    tall-skinny GEMMs over the 65 536-row minibatch run far below the GPU's rate (the weight
    gradient dW = g^T x alone ~190 us per layer: profiles/r03/r03i); the gradients then
    match the eager update's to fp32 rounding instead of bitwise. ``fused=False`` captures the
    PyTorch ops themselves (bitwise the eager ``ppo_update``).

    Needs an optimizer created with ``capturable=True`` (``torch.optim.Adam(..., capturable=True)``:
    its step count lives on the device) and ``n_steps * num_envs`` divisible by ``batch_size``.
    The warm-up steps the capture requires run on the real parameters and are undone (parameters
    and optimizer state restored in place), so the first ``update`` starts from the same state
    as the eager ``ppo_update`` would, and computes the same minibatch steps (``fused=False``: same
    kernels, same order; ``tests/test_gpu_rollout.py``). Multi-GPU: ``group`` must be an RCCL ("nccl") group —
    the all_reduce is captured with the rest.

    ``clip_range_vf`` / ``normalize_advantage`` / ``target_kl`` / ``train_stats`` (SB3's defaults and
    False: exactly the calls described above) put the fused one-replica path on
    ``rr_ppo_update_opts`` (``PPOUpdate``; ``rr_ppo_update_discrete_opts`` for a Categorical policy).
    ``update`` then clears the control block, every epoch's
    first minibatch is captured with the epoch-start flag, and a KL stop needs no host decision: the
    epochs after it replay as no-ops, and ``update`` still never waits for the device on their
    account. ``train_stats()`` returns SB3's ``train/*`` means over the last ``update`` with one
    copy. ``fused=False`` captures ``clip_range_vf`` and ``normalize_advantage`` as PyTorch ops and
    refuses ``target_kl`` (a ``break`` cannot be captured); the split multi-GPU path refuses all.

    A ``MlpCategoricalActorCritic``: ``fused`` defaults to True where ``PPOUpdateDiscrete`` applies
    (one replica, capturable Adam, SB3's defaults) and captures its chained calls. An option or
    ``train_stats`` keeps that default off the fused path; ``fused=True`` takes them
    (``rr_ppo_update_discrete_opts``: the control block, the KL stop and ``train_stats()`` as above).
    ``group`` raises with ``fused=True`` and is captured as PyTorch ops with ``fused=False``."""

    def __init__(self, policy, optimizer, ro, batch_size=65536, clip_range=0.2, ent_coef=0.01, vf_coef=0.5,
                 max_grad_norm=0.5, group=None, fused=None, clip_range_vf=None, normalize_advantage=True,
                 target_kl=None, train_stats=False):
        if not all(g.get("capturable", False) for g in optimizer.param_groups):
            raise ValueError("GraphedPPOUpdate needs an optimizer with capturable=True")
        cvf, norm, tkl = _ppo_options(clip_range_vf, normalize_advantage, target_kl)
        self._opt = (cvf, norm, tkl)
        if fused is None and isinstance(policy, MlpCategoricalActorCritic):
            fused = (fused_discrete_supported(policy, ro.env.state_dim) and group is None
                     and not (cvf or tkl or not norm or train_stats)
                     and clip_adam_supported(optimizer, list(policy.parameters())))
        if fused is None:
            fused = fused_grad_supported(policy, ro.env.state_dim, ro.env.action_dim)
        self.fused = bool(fused)
        one_call = _refuse_options(policy, optimizer, group, self.fused, cvf, norm, tkl, train_stats, graphed=True)
        n = ro.n_steps * ro.env.num_envs
        if n % batch_size:
            raise ValueError("n_steps * num_envs (%d) must be a multiple of batch_size (%d)" % (n, batch_size))
        if group is not None:
            import torch.distributed as dist
            if dist.get_backend(group) != "nccl":
                raise ValueError("a captured gradient all_reduce needs the nccl (RCCL) backend")
        self.policy, self.optimizer, self.ro, self.group = policy, optimizer, ro, group
        self.n, self.bs = n, batch_size
        dev = ro.obs.device
        self.obs = ro.obs.reshape(n, -1)
        self.act = ro.actions.reshape(n, -1)
        self.old_lp = ro.log_probs.reshape(n)
        self.adv_all = ro.advantages.reshape(n)
        self.ret = ro.returns.reshape(n)
        self.coef = (clip_range, ent_coef, vf_coef, max_grad_norm)
        self.perm = torch.arange(n, device=dev)  # refilled per epoch; minibatch k = perm[k bs : (k + 1) bs]
        self._perm_bufs = self._perm_stream = None  # update(): the next epoch's permutation, drawn aside
        self._first = None  # prepare(): the event of the next update's first draw
        self.n_mb = n // batch_size
        params = list(policy.parameters())
        # state to restore after the warm-up steps (in place: the graph keeps these tensors)
        saved_p = [p.detach().clone() for p in params]
        saved_s = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in optimizer.state[p].items()}
                   for p in params if p in optimizer.state}
        # static gradient buffers (allocated outside the graph): the captured step copies
        # torch.autograd.grad's results into them, so no accumulation into .grad is captured. The
        # policy's Linear layers must take their bias gradient as a GEMM (_LinearFn): a column sum
        # after a GEMM in the same graph is wrong from the second replay on (profiles/r03/r03i/probe_graph_reduce.txt)
        self.params = params
        for p in params:
            p.grad = torch.zeros_like(p)
        self.old_v = _old_values(ro, n) if cvf and not self.fused else None
        # fused, one replica, capturable Adam: the chained whole-minibatch call (rr_ppo_update, or
        # rr_ppo_update_opts with an option or train_stats)
        self._update = (_whole_step(policy, optimizer, ro, batch_size, clip_range, ent_coef, vf_coef, max_grad_norm,
                                    clip_range_vf, normalize_advantage, target_kl, train_stats) if one_call else None)
        self._grad = (PPOGrad(policy, ro, batch_size, clip_range, ent_coef, vf_coef)
                      if self.fused and self._update is None else None)
        self._adam = (ClipAdam(optimizer, params, max_grad_norm)
                      if self._grad is not None and clip_adam_supported(optimizer, params) else None)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for k in range(3):
                self._step(self._mb(k % self.n_mb), k % self.n_mb)
        torch.cuda.current_stream(dev).wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for k in range(self.n_mb):
                self.stats = self._step(self._mb(k), k)
        with torch.no_grad():
            for p, v in zip(params, saved_p):
                p.copy_(v)
            for p in params:
                st = optimizer.state.get(p)
                if not st:
                    continue
                old = saved_s.get(id(p))
                for k, v in st.items():
                    if torch.is_tensor(v):
                        if old is not None and k in old:
                            v.copy_(old[k])
                        else:
                            v.zero_()  # state the warm-up created: back to a fresh optimizer's
        if self._update is not None and self._update.opts is not None:
            self._update.reset()  # what the warm-up and the capture's eager side counted
        torch.cuda.synchronize(dev)

    def _mb(self, k):
        return self.perm[k * self.bs:(k + 1) * self.bs]

    def _step(self, i, k=0):
        clip_range, ent_coef, vf_coef, max_grad_norm = self.coef
        pol = self.policy
        if self.fused:
            if self._update is not None:
                kw = dict(epoch_start=k == 0) if self._update.opts is not None else {}
                st = self._update(i, self._mb(k + 1) if k + 1 < self.n_mb else None, chained=k > 0, **kw)
            else:
                st = self._grad(i)
                if self.group is not None:
                    _allreduce_grads(self.params, self.group)
                if self._adam is not None:
                    self._adam()
                else:
                    torch.nn.utils.clip_grad_norm_(self.params, max_grad_norm)
                    self.optimizer.step()
            self._more = (st[3], st[4])
            return _loss_stats(st)
        cvf, norm, _ = self._opt
        old = self.old_lp[i]
        loss, stats, lp, ratio = _ppo_loss(pol, self.obs[i], self.act[i], old, self.adv_all[i], self.ret[i],
                                           self.old_v[i] if cvf else None, self.bs, clip_range, ent_coef, vf_coef,
                                           cvf, norm)
        for p, g in zip(self.params, torch.autograd.grad(loss, self.params)):
            p.grad.copy_(g)
        if self.group is not None:
            _allreduce_grads(self.params, self.group)
        torch.nn.utils.clip_grad_norm_(pol.parameters(), max_grad_norm)
        self.optimizer.step()
        with torch.no_grad():  # SB3 1.6 PPO.train's clip_fraction and approx_kl, as rr_ppo_grad's stats[3:5]
            log_ratio = lp - old
            self._more = ((torch.abs(ratio - 1) > clip_range).float().mean(), ((ratio - 1) - log_ratio).mean())
        return stats

    def last_stats(self):
        """The last minibatch step's five figures as ``train/*`` keys: ``update``'s three and the
        ``clip_fraction`` / ``approx_kl`` the step computes beside them. One iteration's log dict is
        ``ro.stats.last() | upd.last_stats()``."""
        out = {"train/" + k: float(v) for k, v in self.stats.items()}
        out["train/clip_fraction"], out["train/approx_kl"] = (float(v) for v in self._more)
        return out

    def train_stats(self):
        """SB3 PPO.train's log figures over the last ``update``, from the control block with one copy:
        ``train/policy_gradient_loss``, ``train/value_loss``, ``train/entropy_loss``,
        ``train/clip_fraction`` (means over every evaluated minibatch), ``train/approx_kl`` (mean
        over the last, possibly partial, epoch), ``train/n_minibatches`` (optimizer steps applied),
        ``train/n_evaluated``, ``train/early_stop`` and ``train/stop_epoch`` (None without a stop)."""
        if self._update is None or self._update.opts is None:
            raise ValueError("train_stats() needs GraphedPPOUpdate(train_stats=True) or one of the options on the "
                             "fused one-replica path")
        return self._update.train_stats()

    def _perm_streams(self):
        dev = self.obs.device
        if self._perm_bufs is None:
            self._perm_bufs = (torch.empty_like(self.perm), torch.empty_like(self.perm))
            self._perm_stream = torch.cuda.Stream(dev)
        return torch.cuda.current_stream(dev), self._perm_bufs, self._perm_stream

    def prepare(self, generator=None):
        """Draw the next ``update``'s first-epoch permutation now, on the side stream: called
        before the rollout collect, the draw runs beside it instead of ahead of the first
        epoch. It is the draw ``update`` would make first; pass ``update`` the same generator
        and draw nothing else from it in between."""
        main, bufs, side = self._perm_streams()
        side.wait_stream(main)  # the previous update's readers of bufs[0] are done
        with torch.cuda.stream(side):
            torch.randperm(self.n, out=bufs[0], generator=generator)
            self._first = side.record_event()

    def update(self, n_epochs=10, generator=None):
        """n_epochs passes over the rollout in shuffled minibatches (ppo_update's order:
        one torch.randperm per epoch).

        Each later epoch's permutation is drawn on a side stream while the previous epoch's graph
        replays: torch's randperm is a ~0.25 ms chain of small sort launches at 1 M rows, and the
        learner's kernels leave most of each SIMD's wave slots free. The draws are issued in the
        same order from the same generator, so the permutations are the sequential loop's. After
        ``prepare`` the first epoch uses the permutation drawn there."""
        for o in (self._adam, self._update):
            if o is not None:
                o.sync_lr()  # the graph reads lr from the device: follow param_groups[0]["lr"]
        if self._update is not None and self._update.opts is not None:
            self._update.reset()  # a new train() pass: stop state and running sums cleared, stream-ordered
        main, bufs, side = self._perm_streams()
        ready, self._first = self._first, None
        if ready is None:  # no prepare(): the first epoch's draw in line
            torch.randperm(self.n, out=bufs[0], generator=generator)
        for e in range(n_epochs):
            cur = bufs[e % 2]
            if ready is not None:
                main.wait_event(ready)
            self.perm.copy_(cur)
            if e + 1 < n_epochs:
                side.wait_stream(main)  # the other buffer's last reader (the previous copy) is done
                with torch.cuda.stream(side):
                    torch.randperm(self.n, out=bufs[(e + 1) % 2], generator=generator)
                    ready = side.record_event()
            self.graph.replay()
        return {k: float(v) for k, v in self.stats.items()}
