"""A2C for the Categorical policy of the discrete 3DOF actions (``MlpCategoricalActorCritic``, the reference's
``DiscreteActions3DOF`` stack) on a ``DeviceRollout``'s buffers: ``a2c.py``'s three entry points under names
of their own, because ``A2CUpdate``, ``a2c_update(fused=True)`` and ``GraphedA2C`` refuse that policy.

``A2CUpdateDiscrete`` is one ``A2C.train()`` as ONE library call (``rr_a2c_update_discrete``: the PPO
learner's towers with a softmax head, the A2C head derivative and the entropy's gradient per sample, the
fixed-order finish, ``clip_grad_norm_`` and the optimizer's step: four launches); ``a2c_update_discrete`` is
that call where it applies and ``a2c._a2c_loss`` in PyTorch autograd elsewhere, the very function
``a2c_update(fused=False)`` runs; ``GraphedA2CDiscrete`` captures the one-launch Categorical collect
followed by the update into one hipGraph.

The loss is SB3 1.6 ``A2C.train``'s behind a ``CategoricalDistribution`` over K = 2 .. 4 choices:

    A           = advantages, or (A - mean(A)) / (std(A) + 1e-8) with normalize_advantage
    log_prob    = logit_a - logsumexp(logits)
    entropy     = mean_i -sum_k p_ik log p_ik          (state dependent)
    policy_loss = -mean(A * log_prob)
    value_loss  = F.mse_loss(returns, values)
    loss        = policy_loss + ent_coef * -entropy + vf_coef * value_loss

The optimizers, the optimizer state binding, ``idx``, ``lr`` and the statistics block are ``a2c.A2CUpdate``'s.
Not available, and refused by name where asked for: 6DOF batches (the table rows are [gimbal, thrust]),
``policy_dtype`` other than fp32 (``DeviceRollout`` refuses both), a process ``group`` on the fused call, the
two-launch or per-step collect inside ``GraphedA2CDiscrete``, a dopri5 batch there.
"""
import torch

from . import a2c
from .a2c import STAT_NAMES, A2CUpdate, GraphedA2C, _coefficients, _optimizer_kind
from .policy import MlpCategoricalActorCritic, fused_discrete_supported


def _fused_reason(policy, optimizer, ro):
    """Why ``rr_a2c_update_discrete`` does not take this policy, optimizer and rollout; None if it does."""
    if not isinstance(policy, MlpCategoricalActorCritic):
        return ("the fused Categorical A2C call takes an MlpCategoricalActorCritic, not the Gaussian %s "
                "(a2c.A2CUpdate, a2c_update and GraphedA2C take that one)" % type(policy).__name__)
    if policy.hidden != (64, 64):
        return "the fused Categorical A2C call needs 64x64 towers"
    if not 2 <= policy.n_choices <= 4:
        return "the fused Categorical A2C call takes K = 2 .. 4 choices, not %d" % policy.n_choices
    if not fused_discrete_supported(policy, ro.env.state_dim):
        return "the fused Categorical A2C call drives the 3DOF env (obs 7): a 6DOF table is refused"
    if ro.actions.shape[-1] != 1:
        return "the fused Categorical A2C call reads ro.actions as [n, 1] indices, not %d columns" % ro.actions.shape[-1]
    reason = _optimizer_kind(optimizer, list(policy.parameters()))[1]
    if reason is None and not ro.obs.is_cuda:
        reason = "the fused Categorical A2C call needs a rollout on the GPU, not CPU tensors"
    return reason


def _check_indices(actions, n_choices):
    """One reduction on the rollout's device: every stored action is an integer in [0, n_choices) (the
    kernel compares an index against k and never forms an address from it, but a row that names no choice
    would be trained on as if its log-prob were 0)."""
    if not bool(((actions == actions.floor()) & (actions >= 0) & (actions < n_choices)).all()):  # NaN fails the first
        raise ValueError("A2CUpdateDiscrete: ro.actions must hold integers in [0, %d)" % n_choices)


class A2CUpdateDiscrete(A2CUpdate):
    """``a2c.A2CUpdate``'s contract for a 64x64 ``MlpCategoricalActorCritic`` on a 3DOF rollout: one
    ``A2C.train()`` as ONE library call (``rr_a2c_update_discrete``, four launches) on the policy's 12
    tensors and the optimizer's own state.

    ``ro.actions`` is ``[n_steps, N, 1]``, the chosen index as a float (what the Categorical collects
    write); the indices present at construction are validated once, on the device. ``ro.log_probs`` is never
    read. ``__call__(idx=None)``, ``sync_lr()`` and ``last_stats()`` are ``A2CUpdate``'s; ``stats[2]`` is
    the mean entropy of the rows. ``train_stats()`` has no ``train/std``: SB3 logs that only for a policy
    with ``log_std``. Refused, with the reason: a Gaussian policy, towers other than 64x64, K outside
    2 .. 4, CPU tensors, the optimizer cases of ``a2c._optimizer_kind``, a rollout under 2 rows; ``group=``
    (multi-GPU) is not an argument of the fused call."""

    _call = "rr_a2c_update_discrete"

    def __init__(self, policy, optimizer, ro, normalize_advantage=False, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5):
        self.ent_coef, self.vf_coef, self.max_norm = _coefficients(ent_coef, vf_coef, max_grad_norm)
        reason = _fused_reason(policy, optimizer, ro)
        if reason is not None:
            raise ValueError("A2CUpdateDiscrete: " + reason)
        self._bind(policy, optimizer, ro, normalize_advantage, policy.n_choices, 1)
        _check_indices(self.data[1], policy.n_choices)

    def train_stats(self):
        """SB3 ``A2C.train``'s log figures for the last call (one copy of the statistics, which waits for
        the stream)."""
        st = self.stats.tolist()
        return {"train/policy_loss": st[0], "train/value_loss": st[1], "train/entropy_loss": -st[2],
                "train/n_updates": self.n_updates}


def a2c_update_discrete(policy, optimizer, ro, normalize_advantage=False, ent_coef=0.0, vf_coef=0.5,
                        max_grad_norm=0.5, fused=None):
    """``a2c.a2c_update`` with the fused call of the Categorical policy: one SB3 ``A2C.train()`` on all
    ``n_steps * num_envs`` rows of the device-resident rollout. Returns the five figures (``STAT_NAMES``)
    as a dict of floats.

    ``fused=None`` takes ``A2CUpdateDiscrete`` where it applies. Otherwise, and with ``fused=False``, the
    loss is ``a2c._a2c_loss`` through PyTorch autograd, then ``clip_grad_norm_`` and ``optimizer.step()``:
    ``a2c_update(fused=False)`` itself, for any policy that function takes. ``fused=True`` where the call
    does not apply raises and names the reason."""
    _coefficients(ent_coef, vf_coef, max_grad_norm)
    reason = _fused_reason(policy, optimizer, ro)
    if fused is None:
        fused = reason is None
    if fused and reason is not None:
        raise ValueError("a2c_update_discrete(fused=True): " + reason)
    if not fused:
        return a2c.a2c_update(policy, optimizer, ro, normalize_advantage, ent_coef, vf_coef, max_grad_norm, fused=False)
    step = A2CUpdateDiscrete(policy, optimizer, ro, normalize_advantage, ent_coef, vf_coef, max_grad_norm)
    step()
    return step.last_stats()


class GraphedA2CDiscrete(GraphedA2C):
    """``a2c.GraphedA2C`` for the Categorical policy: ``ro.collect()`` followed by ``A2CUpdateDiscrete`` on
    all its rows, captured ONCE into one linear hipGraph; ``step()`` replays it. ``ro`` is
    ``DeviceRollout(batch, cat_policy, one_launch=True)`` (not ``per_step``), optionally with
    ``stats=True``. The warm-up iteration and the put-back are ``GraphedA2C``'s, so the first ``step()``
    starts where an eager ``ro.collect(); update()`` would and computes the same bits. The two-launch
    collect (a Categorical policy's default, and the only one on a dopri5 batch) and the per-step collect
    are refused by name."""

    def __init__(self, policy, optimizer, ro, normalize_advantage=False, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5):
        _coefficients(ent_coef, vf_coef, max_grad_norm)
        reason = _fused_reason(policy, optimizer, ro)
        if reason is not None:
            raise ValueError("GraphedA2CDiscrete: " + reason)
        if not (getattr(ro, "fused", False) and getattr(ro, "one_launch", False)):
            raise ValueError("GraphedA2CDiscrete needs DeviceRollout(batch, policy, one_launch=True): the two-launch "
                             "collect (the Categorical policy's default, and a dopri5 batch's only one) is not captured")
        if getattr(ro, "per_step", True):
            raise ValueError("GraphedA2CDiscrete needs DeviceRollout(batch, policy, one_launch=True): the per-step "
                             "collect (per_step=True) is not captured")
        self._capture(ro, A2CUpdateDiscrete(policy, optimizer, ro, normalize_advantage, ent_coef, vf_coef,
                                            max_grad_norm))


__all__ = ["A2CUpdateDiscrete", "GraphedA2CDiscrete", "a2c_update_discrete", "STAT_NAMES"]
