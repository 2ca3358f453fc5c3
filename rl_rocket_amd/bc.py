"""Behaviour cloning on the device: pre-training a policy on recorded ``(obs, action)`` pairs, what
the reference's ``imitationKickstarter.train()`` does with ``imitation``'s ``bc.BC`` before PPO takes
over (my_environment/utils/imitation_kickstarter.py).

``Demonstrations`` holds the pairs as device tensors (from arrays, from a ``DeviceRollout``, or from
the episodes a recording ``PolicyEvaluator`` kept); ``BCUpdate`` is one minibatch step as one library
call (``rr_bc_update``: the PPO learner's pi tower with the behaviour-cloning head derivative, the
fixed-order finish, Adam); ``bc_train`` runs epochs of it, or of the same loss in PyTorch autograd
for a policy or an optimizer the fused call does not take.

The loss is ``imitation``'s ``BehaviorCloningLossCalculator`` for a diagonal Gaussian policy:

    logp_i  = sum_a (-(acts_ia - mean_ia)^2 / (2 std_a^2) - log_std_a - 0.5 log 2 pi)
    neglogp = -mean_i logp_i
    entropy = sum_a (0.5 + 0.5 log 2 pi + log_std_a)
    l2_norm = 0.5 * sum over all parameter tensors of sum(w^2)
    loss    = neglogp - ent_weight * entropy + l2_weight * l2_norm
    prob_true_act = mean_i exp(logp_i)

and for a ``MlpCategoricalActorCritic`` (the discrete 3DOF actions: the reference's keyboard demonstrations
are indices into ``DiscreteActions3DOF``'s table) the same calculator on SB3's ``CategoricalDistribution``:

    log p_ik = z_ik - logsumexp_k z_ik      logp_i = log p_{i, a_i}
    H_i      = -sum_k p_ik log p_ik         (a term whose p_ik is 0 counts 0)
    neglogp  = -mean_i logp_i               entropy = mean_i H_i
    l2_norm  = 0.5 * sum over the 12 tensors of sum(w^2)
    loss     = neglogp - ent_weight * entropy + l2_weight * l2_norm

There ``acts`` is ``[M, 1]`` float32 holding the indices (the form of SB3's buffer and of
``DeviceRollout.actions``), ``BCUpdate`` calls ``rr_bc_update_discrete`` on the policy's 12 tensors, and the
indices are checked once (``_check_indices``) before anything indexes with them.
"""
import math

import numpy as np
import torch

from . import _lib
from .learner import (_AdamState, _allreduce_grads, _check_idx, _check_params, _epoch_perms, _stream, _workspace,
                      clip_adam_supported)
from .policy import MlpCategoricalActorCritic, _policy_tensors, fused_discrete_supported, fused_grad_supported

STAT_NAMES = ("neglogp", "entropy", "ent_loss", "prob_true_act", "l2_norm", "l2_loss", "loss")  # RR_BC_STAT_*


class Demonstrations:
    """``obs`` [M, ns] and ``acts`` [M, na]: contiguous float32 tensors on one device, row i a
    normalised observation and the normalised action taken on it. For a Categorical policy ``acts`` is
    [M, 1] and holds the chosen index as a float (``from_arrays`` on an integer array gives it, and
    ``from_rollout`` on a Categorical collect is a view of the collect's buffers)."""

    def __init__(self, obs, acts):
        if obs.dim() != 2 or acts.dim() != 2 or obs.shape[0] != acts.shape[0]:
            raise ValueError("obs [M, ns] and acts [M, na] must have the same number of rows")
        for t in (obs, acts):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("demonstrations must be contiguous float32 tensors")
        if obs.device != acts.device:
            raise ValueError("obs and acts must be on the same device")
        self.obs, self.acts = obs, acts

    def __len__(self):
        return self.obs.shape[0]

    @property
    def device(self):
        return self.obs.device

    @classmethod
    def from_arrays(cls, obs, acts, device):
        """From array-likes (numpy, lists, tensors), converted to float32 on ``device``."""
        def conv(x):
            if not torch.is_tensor(x):
                x = torch.as_tensor(np.asarray(x, dtype=np.float32))
            x = x.to(device=device, dtype=torch.float32)
            return x.reshape(x.shape[0], -1).contiguous()

        return cls(conv(obs), conv(acts))

    @classmethod
    def from_rollout(cls, ro):
        """The collect's ``obs`` [T, N, ns] / ``actions`` [T, N, na] buffers, flattened to T * N rows
        (views: the next collect overwrites them)."""
        n = ro.obs.shape[0] * ro.obs.shape[1]
        return cls(ro.obs.reshape(n, ro.obs.shape[-1]), ro.actions.reshape(n, ro.actions.shape[-1]))

    @classmethod
    def from_trace(cls, trace, batch, episodes="finished"):
        """The steps of the episodes an ``EvalTrace`` recorded (``PolicyEvaluator(record=...)``).

        For every recorded slot and every FINISHED, UNCLIPPED episode of it, the steps
        ``t < length``: ``obs`` is the recorded state row ``t`` times the float32 reciprocal
        normaliser of ``batch`` (``float32(1 / state_normalizer)``, what the handle's kernels
        multiply by), so on an RK4 / Euler batch it is bitwise the observation the policy was given;
        ``acts`` is the recorded action, the clipped mean the env stepped with. A trace with a ``choice``
        plane (a Categorical policy's) gives ``acts`` [M, 1], the chosen indices as floats: what ``BCUpdate``
        and ``bc_train`` take for an ``MlpCategoricalActorCritic``. A trace recorded with
        ``PolicyEvaluator(deterministic=False)`` gives the clipped samples (the sampled indices): a teacher
        that explores, over the states its noise reaches.

        Row order: slot-major (the order of ``record=``), then episode, then step. Episodes cut by
        ``max_steps`` (partial) and episodes longer than the recording capacity (clipped) are left
        out whole. Built with a mask on the trace's device: no host loop over steps."""
        if episodes != "finished":
            raise ValueError("episodes must be \"finished\" (partial and clipped episodes are not demonstrations)")
        dev = trace.action.device
        k, ne, cap = trace.action.shape[:3]
        length = trace.length.to(torch.int64).T  # [K, ne]
        if trace.episodes is None:
            done = torch.full((k,), ne, dtype=torch.int64, device=dev)
        else:
            done = torch.as_tensor(trace.episodes, device=dev)[torch.as_tensor(trace.env_ids, device=dev).long()].long()
        ok = (torch.arange(ne, device=dev)[None, :] < done[:, None]) & (length <= cap)
        mask = ok[:, :, None] & (torch.arange(cap, device=dev)[None, None, :] < length[:, :, None])
        inv = torch.tensor((1.0 / np.asarray(batch.cfg.state_normalizer, dtype=np.float64)).astype(np.float32),
                           device=dev)[:trace.state.shape[-1]]
        obs = trace.state[:, :, :cap][mask] * inv
        if getattr(trace, "choice", None) is not None:
            return cls(obs.contiguous(), trace.choice[mask].to(torch.float32).reshape(-1, 1).contiguous())
        return cls(obs.contiguous(), trace.action[mask].contiguous())


def _check_indices(acts, n_choices):
    """One reduction on ``acts``' device: every demonstrated action of a Categorical policy is an integer
    in ``[0, n_choices)`` in an ``[M, 1]`` tensor, or ``ValueError``. Nothing may index with them before this
    (an index out of range in a ``gather`` on the GPU is a device-side assert), and the fused call, which
    cannot check device data, is only given indices that passed."""
    if acts.dim() != 2 or acts.shape[1] != 1:
        raise ValueError("a Categorical policy's demonstrations are acts [M, 1] holding the chosen index, not %s"
                         % (tuple(acts.shape),))
    if not bool(((acts == acts.floor()) & (acts >= 0) & (acts < n_choices)).all()):  # NaN fails the first
        raise ValueError("a Categorical policy's demonstrated actions must be integers in [0, %d)" % n_choices)


def _bc_loss(policy, obs, acts, ent_weight, l2_weight):
    """The loss of the module's head in PyTorch ops, with its seven figures (tensors). A Categorical
    policy's ``acts`` have passed ``_check_indices``."""
    if isinstance(policy, MlpCategoricalActorCritic):
        logits = policy(obs)[0]
        logp = policy.log_prob(logits, acts)
        entropy = policy.entropy(logits).mean()
    else:
        mean = policy(obs)[0]
        log_std = policy.log_std
        std = log_std.exp()
        logp = (-((acts - mean) ** 2) / (2 * std * std) - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
        entropy = (0.5 + 0.5 * math.log(2 * math.pi) + log_std).sum()
    neglogp = -logp.mean()
    l2_norm = sum(p.square().sum() for p in policy.parameters()) / 2
    ent_loss, l2_loss = -ent_weight * entropy, l2_weight * l2_norm
    loss = neglogp + ent_loss + l2_loss
    return loss, (neglogp, entropy, ent_loss, logp.exp().mean(), l2_norm, l2_loss, loss)


class BCUpdate(_AdamState):
    """One behaviour-cloning minibatch step as ONE library call (``rr_bc_update``): the loss of this
    module's head and its backward on fp32 MFMA, then ``torch.optim.Adam``'s capturable step on the
    optimizer's own state tensors, without gradient clipping. Four launches, three when chained.

    ``__call__(idx, chained=False)``: ``idx`` is a contiguous int64 device tensor of 2 ..
    ``batch_size`` rows of ``demos``. It writes ``p.grad`` of the policy's 13 parameters (the value
    tower's are ``l2_weight * w``: zeros at 0), steps all 13 and returns ``stats`` (device, 8
    floats). ``chained=True`` says that the previous call on this object was the last writer of the
    parameters: the packing launch is skipped. The requirements are ``PPOUpdate``'s: an
    ``MlpActorCritic`` with 64x64 towers, a capturable Adam over exactly its parameters, and the
    gradient and state tensors kept (the library holds their addresses). ``lr`` is read from a device
    scalar that eager calls refresh; ``sync_lr()`` before replays of a captured graph.
    ``last_stats()`` returns the seven figures as a dict (one copy, which waits for the stream).

    An ``MlpCategoricalActorCritic`` (64x64 towers, 3DOF observations, 2 .. 4 choices) takes the same step
    through ``rr_bc_update_discrete`` on its 12 tensors: ``demos.acts`` is [M, 1] indices, checked here once
    (``ValueError`` for a value that is no integer in ``[0, n_choices)``); the entropy is the minibatch's
    mean. Everything else, ``chained=`` included, is as above."""

    def __init__(self, policy, optimizer, demos, batch_size, ent_weight=1e-3, l2_weight=0.0):
        ns, na = demos.obs.shape[1], demos.acts.shape[1]
        self._call = "rr_bc_update"
        if isinstance(policy, MlpCategoricalActorCritic):
            if not fused_discrete_supported(policy, ns):
                raise ValueError("BCUpdate needs an MlpCategoricalActorCritic with 64x64 towers and 2 .. 4 choices "
                                 "on 3DOF observations")
            _check_indices(demos.acts, policy.n_choices)
            self._call, na = "rr_bc_update_discrete", policy.n_choices  # the call's shape is (ns, n_choices)
        elif not fused_grad_supported(policy, ns, na):
            raise ValueError("BCUpdate needs an MlpActorCritic with 64x64 towers and (obs, act) in ((14, 3), (7, 2))")
        if not 2 <= batch_size <= len(demos):
            raise ValueError("batch_size must be in [2, len(demos)]")
        for name, v in (("ent_weight", ent_weight), ("l2_weight", l2_weight)):
            if not 0.0 <= float(v) < float("inf"):
                raise ValueError("%s must be a finite number >= 0, not %r" % (name, v))
        if not clip_adam_supported(optimizer, list(policy.parameters())):
            raise ValueError("BCUpdate needs a capturable torch.optim.Adam over the policy's parameters "
                             "(one group, no weight decay / amsgrad / maximize)")
        self._lib = _lib.load()
        self.ns, self.na, self.bs = ns, na, int(batch_size)
        self.ent_weight, self.l2_weight = float(ent_weight), float(l2_weight)
        self.demos = demos
        dev = demos.device
        self.params = _policy_tensors(policy)
        _check_params(self._call, self.params, dev, "demonstrations'")
        self._bind_adam(optimizer, self.params)
        self.ws, self._nbytes = _workspace(self._lib, self._call + "_workspace_size", dev, ns, na, self.bs)
        self.stats = torch.zeros(_lib.RR_BC_STAT_SLOTS, dtype=torch.float32, device=dev)
        self._versions = None  # the parameters' version counters after the last call: what chained=True may follow

    def last_stats(self):
        return dict(zip(STAT_NAMES, self.stats.tolist()))

    def __call__(self, idx, chained=False):
        _check_idx(idx, self.bs, self.ws.device, flat=True)
        if chained and self._versions != [p._version for p in self.params]:
            raise ValueError("chained=True needs the previous call on this BCUpdate to be the last writer of the "
                             "parameters")
        _lib.check(getattr(self._lib, self._call)(
            self.ns, self.na, *self._ptrs, self.demos.obs.data_ptr(), self.demos.acts.data_ptr(), idx.data_ptr(),
            idx.numel(), self.ent_weight, self.l2_weight, *self._adam_args(), self.stats.data_ptr(),
            _lib.RR_BC_CHAINED if chained else 0, self.ws.data_ptr(), self._nbytes, _stream(self.ws.device)),
            self._call)
        self._versions = [p._version for p in self.params]
        return self.stats


def bc_train(policy, optimizer, demos, n_epochs=1, batch_size=None, generator=None, ent_weight=1e-3, l2_weight=0.0,
             fused=None, group=None):
    """``n_epochs`` passes of behaviour cloning over ``demos``, as ``imitation``'s ``bc.BC.train``
    makes them: per epoch one permutation, minibatches of ``batch_size`` rows with the short
    remainder dropped (``DataLoader(shuffle=True, drop_last=True)``), the module's loss, Adam without
    a gradient clip. ``batch_size=None`` is ``min(len(demos), 65536)``. Returns the last minibatch's
    figures (``STAT_NAMES``) as a dict of floats, ``{}`` when no minibatch ran.

    ``fused=None`` takes ``BCUpdate`` (chained within the epoch) for an ``MlpActorCritic`` with 64x64
    towers on a GPU with a capturable Adam, and the same loss through PyTorch autograd otherwise
    (any policy whose ``policy(obs)[0]`` is the action mean and that has ``log_std``); ``fused=True``
    insists, ``fused=False`` is the autograd path. An ``MlpCategoricalActorCritic`` is cloned on indices
    (``acts`` [M, 1], checked once before anything indexes with them: ``ValueError``): the fused call is
    ``rr_bc_update_discrete`` under the same conditions, the autograd path the loss through the policy's
    ``log_prob`` / ``entropy`` on any device. A ``torch.distributed`` ``group`` averages the
    minibatch gradients over the ranks on the autograd path; the fused call has no gradient-only half
    and refuses it."""
    m = len(demos)
    bs = min(m, 65536) if batch_size is None else int(batch_size)
    if not 1 <= bs <= m:
        raise ValueError("batch_size must be in [1, len(demos)]")
    params = list(policy.parameters())
    if isinstance(policy, MlpCategoricalActorCritic):
        _check_indices(demos.acts, policy.n_choices)
        shape_ok = fused_discrete_supported(policy, demos.obs.shape[1])
    else:
        shape_ok = fused_grad_supported(policy, demos.obs.shape[1], demos.acts.shape[1])
    can = demos.obs.is_cuda and bs >= 2 and shape_ok and clip_adam_supported(optimizer, params)
    if fused is None:
        fused = can and group is None
    if fused and group is not None:
        raise ValueError("bc_train(fused=True) takes no group: rr_bc_update has no gradient-only call for an "
                         "all_reduce between its halves; use fused=False")
    if fused and not can:
        raise ValueError("bc_train(fused=True) needs an MlpActorCritic with 64x64 towers, a capturable "
                         "torch.optim.Adam over its parameters, CUDA demonstrations and batch_size >= 2")
    last = m - m % bs
    if fused:
        step = BCUpdate(policy, optimizer, demos, bs, ent_weight, l2_weight)
        ran = False
        for perm in _epoch_perms(m, n_epochs, demos.device, generator):
            for s in range(0, last, bs):
                step(perm[s:s + bs], chained=s > 0)
                ran = True
        return step.last_stats() if ran else {}
    figures = None
    for _ in range(n_epochs):
        perm = torch.randperm(m, device=demos.device, generator=generator)
        for s in range(0, last, bs):
            idx = perm[s:s + bs]
            loss, figures = _bc_loss(policy, demos.obs[idx], demos.acts[idx], ent_weight, l2_weight)
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            if group is not None:
                _allreduce_grads(params, group)
            optimizer.step()
    return {} if figures is None else {k: float(v.detach()) for k, v in zip(STAT_NAMES, figures)}
