"""SB3 1.6 A2C.train's loss behind a CategoricalDistribution, restated for the tests of rr_a2c_update_discrete
(tests only; no kernels here, and nothing that calls one):

    A    = adv, or (adv - adv.mean()) / (adv.std() + 1e-8) with normalize_advantage
    lp   = logit_a - logsumexp(logits)
    H    = -sum_k p_k log p_k                     (per sample)
    policy_loss = -(A * lp).mean();  value_loss = mse_loss(returns, values);  entropy = H.mean()
    loss = policy_loss - ent_coef * entropy + vf_coef * value_loss

`reference` applies it to an MlpCategoricalActorCritic in a chosen dtype through autograd, on the CPU, and
returns the 12 gradients (rr_ppo_update_discrete's order, float64) and the five figures (a2c_ref.STATS). The
inputs are the existing discrete helpers': discrete_ref.cat_policy's policies, discrete_edge_ref.sweep_pool's
70 001-row rollout per K and its edge_case; the optimizers and the stub rollout are a2c_ref's."""
import copy

import torch

import a2c_ref as R
import discrete_edge_ref as E
import discrete_ref as D

STATS = R.STATS
NAMES = D.NAMES
N_ROWS = E.N_ROWS
KINDS = R.KINDS
optimizer_ref, make_optimizer, stub_rollout = R.optimizer_ref, R.make_optimizer, R.stub_rollout


def flat(ro):
    """(obs [n, 7], actions [n, 1], advantages [n], returns [n]) of a one-step rollout of the discrete helpers."""
    n = ro.env.num_envs
    return ro.obs.reshape(n, 7), ro.actions.reshape(n, 1), ro.advantages.reshape(n), ro.returns.reshape(n)


def loss_terms(logits, value, act, adv, ret, normalize=False, ent_coef=0.0, vf_coef=0.5):
    """(loss, the five figures as tensors) from the logits [B, K], the values [B] and the gathered rows;
    act [B] integers."""
    lsm = torch.log_softmax(logits, dim=-1)
    lp = lsm.gather(1, act[:, None])[:, 0]
    p = lsm.exp()
    entropy = -torch.where(p > 0, p * lsm, torch.zeros_like(p)).sum(-1).mean()
    if normalize:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    policy_loss = -(adv * lp).mean()
    value_loss = ((ret - value) ** 2).mean()
    loss = policy_loss - ent_coef * entropy + vf_coef * value_loss
    return loss, (policy_loss, value_loss, entropy, loss, lp.mean())


def reference(pol, obs, act, adv, ret, idx, dtype=torch.float64, normalize=False, ent_coef=0.0, vf_coef=0.5):
    """One call's gradients before the clip (list of 12, float64, on the CPU) and figures (list of 5 floats)
    in `dtype`; obs [N, 7], act [N, 1] or [N] indices as floats, adv / ret [N], idx the rows (any device)."""
    from rl_rocket_amd.rollout import _policy_tensors

    p = copy.deepcopy(pol).to(dtype).cpu()
    idx = idx.cpu()
    tensors = _policy_tensors(p)
    assert len(tensors) == 12
    logits, value = p(obs.cpu()[idx].to(dtype))
    loss, figures = loss_terms(logits, value, act.cpu().reshape(-1)[idx].long(), adv.cpu()[idx].to(dtype),
                               ret.cpu()[idx].to(dtype), normalize, ent_coef, vf_coef)
    grads = torch.autograd.grad(loss, tensors, allow_unused=True)
    return ([torch.zeros_like(t, dtype=torch.float64) if g is None else g.double() for t, g in zip(tensors, grads)],
            [float(v.detach()) for v in figures])


def sweep_cpu(k):
    """(pol, obs, act, adv, ret) of discrete_edge_ref.sweep_pool(k), on the CPU; read-only."""
    pol, ro = E.sweep_pool(k)
    return (pol,) + flat(ro)


_device = {}


def sweep_gpu(k, device="cuda:0"):
    """sweep_cpu(k) moved to the device once; read-only."""
    if k not in _device:
        pol, *data = sweep_cpu(k)
        _device[k] = (copy.deepcopy(pol).to(device),) + tuple(t.to(device).contiguous() for t in data)
    return _device[k]


def rollout(obs, act, adv, ret, log_probs=None):
    """a2c_ref.stub_rollout for the Categorical policy: [n, 1] indices on the 3DOF env."""
    return R.stub_rollout(7, 1, obs, act, adv, ret, log_probs)


# The loss terms off their defaults: name -> (discrete_edge_ref.edge_case's name, the call's keywords).
# "plain" inputs are edge_case("ent0")'s: nothing special about them (its ratios are not read here).
TERMS = {
    "ent0": ("ent0", dict(ent_coef=0.0)),
    "ent0.01": ("ent0", dict(ent_coef=0.01)),
    "ent0.1": ("ent0", dict(ent_coef=0.1)),
    "vf0.25": ("ent0", dict(ent_coef=0.01, vf_coef=0.25)),
    "peaked": ("peaked", dict(ent_coef=0.01)),
    "underflow": (None, dict(ent_coef=0.01)),  # discrete_ref.learner_inputs(bias_last=-120): p_last is 0 in fp32
    "saturated": ("saturated", dict(ent_coef=0.01)),
    "const_adv_ent0": ("const_adv", dict(normalize=True, ent_coef=0.0)),
    "const_adv_ent0.1": ("const_adv", dict(normalize=True, ent_coef=0.1)),
}
TERM_BATCHES = (1000, 33)
UNDERFLOW_BIAS = -120.0


def terms_case(name, bs, k=4):
    """(pol, (obs, act, adv, ret), idx, keywords) of one case, on the CPU."""
    edge, kw = TERMS[name]
    if edge is None:
        n = 1500
        pol, ro, g = D.learner_inputs(k, n=n, seed=2900 + (bs & 1), bias_last=UNDERFLOW_BIAS)
        idx = torch.randperm(n, generator=g)[:bs].contiguous()
    else:
        c = E.edge_case(edge, bs, k)
        pol, ro, idx = c.pol, c.ro, c.idx
    return pol, tuple(t.contiguous() for t in flat(ro)), idx, dict(kw)


def shares(pol, data, idx, **kw):
    """The fp32 reference's error against the float64 one as shares of the project's bars (per tensor 1e-4
    max |fp64| + 1e-7, statistics 1e-5 |r| + 1e-6): {tensor or statistic: share}."""
    ref64, st64 = reference(pol, *data, idx, torch.float64, **kw)
    ref32, st32 = reference(pol, *data, idx, torch.float32, **kw)
    out = {}
    for name, a, r in zip(NAMES, ref32, ref64):
        out[name] = (a - r).abs().max().item() / (1e-4 * r.abs().max().item() + 1e-7)
    for name, a, r in zip(STATS, st32, st64):
        out[name] = abs(a - r) / (1e-5 * abs(r) + 1e-6)
    return out
