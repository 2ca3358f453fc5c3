"""The behaviour-cloning loss of rr_bc_update_discrete restated in PyTorch autograd, for the tests (tests
only; no kernels here). `imitation`'s BehaviorCloningLossCalculator on SB3's CategoricalDistribution:

    log p_ik = z_ik - logsumexp_k z_ik          logp_i = log p_{i, a_i}
    H_i      = -sum_k p_ik log p_ik             (a term whose p_ik is 0 counts 0)
    neglogp  = -mean_i logp_i                   entropy = mean_i H_i
    prob_true_act = mean_i exp(logp_i)
    l2_norm  = 0.5 * sum over the 12 tensors of sum(w^2)
    loss     = neglogp - ent_weight * entropy + l2_weight * l2_norm

`loss_terms` is the formula on plain tensors (tests/test_bc_discrete_host.py pins it against a case worked
by hand); `reference` applies it to an MlpCategoricalActorCritic in a chosen dtype and returns the 12
gradients (rr_ppo_update_discrete's order, zeros where autograd reaches none) and the seven figures;
`sweep_inputs` builds the GPU tests' policy and rows from discrete_ref.cat_policy / learner_inputs."""
import copy

import torch

import discrete_ref as D

STATS = ("neglogp", "entropy", "ent_loss", "prob_true_act", "l2_norm", "l2_loss", "loss")
NAMES = D.NAMES
VF_NAMES = tuple(NAMES[k] for k in (4, 5, 6, 7, 10, 11))
N_ROWS = 17001
_cache = {}


def loss_terms(logits, acts, params, ent_weight=1e-3, l2_weight=0.0):
    """(loss, the seven figures as tensors) from the logits [B, K], the demonstrated indices [B] (int64)
    and the list of ALL parameter tensors. Written with log_softmax / where, not with the policy's own
    methods: the module under test is not its own reference."""
    lp = torch.log_softmax(logits, dim=-1)
    p = lp.exp()
    logp = lp[torch.arange(lp.shape[0], device=lp.device), acts]
    ent_rows = -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(-1)
    neglogp = -logp.mean()
    entropy = ent_rows.mean()
    l2_norm = 0.5 * sum((w * w).sum() for w in params)
    ent_loss, l2_loss = -ent_weight * entropy, l2_weight * l2_norm
    loss = neglogp + ent_loss + l2_loss
    return loss, (neglogp, entropy, ent_loss, logp.exp().mean(), l2_norm, l2_loss, loss)


def reference(pol, obs, acts, idx, dtype=torch.float64, ent_weight=1e-3, l2_weight=0.0):
    """One minibatch's gradients (list of 12, float64) and figures (list of 7 floats) in `dtype`, on the
    device the inputs are on. acts is [M, 1] or [M] floats holding valid indices."""
    from rl_rocket_amd.rollout import _policy_tensors

    p = copy.deepcopy(pol).to(dtype)
    tensors = _policy_tensors(p)
    logits, _ = p(obs[idx].to(dtype))
    a = acts.reshape(-1)[idx].long()
    assert int(a.min()) >= 0 and int(a.max()) < logits.shape[-1]
    loss, figures = loss_terms(logits, a, tensors, ent_weight, l2_weight)
    grads = torch.autograd.grad(loss, tensors, allow_unused=True)
    return ([torch.zeros_like(t, dtype=torch.float64) if g is None else g.double() for t, g in zip(tensors, grads)],
            [float(v.detach()) for v in figures])


def case_inputs(n_choices, n=N_ROWS, seed=0, device="cuda:0", **kw):
    """(policy, obs [n, 7], acts [n, 1] float indices drawn from the policy) on `device`, from
    discrete_ref.learner_inputs (kw: head_scale, bias_last, ...)."""
    pol, ro, _ = D.learner_inputs(n_choices, n=n, seed=seed, **kw)
    return (copy.deepcopy(pol).to(device), ro.obs.reshape(n, 7).to(device).contiguous(),
            ro.actions.reshape(n, 1).to(device).contiguous())


def sweep_inputs(n_choices):
    """One policy and 17 001 rows per K, built once and read-only: (pol, obs, acts) on the GPU."""
    if n_choices not in _cache:
        _cache[n_choices] = case_inputs(n_choices, seed=40 + n_choices)
    return _cache[n_choices]
