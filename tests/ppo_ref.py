"""Shared inputs and fp64 references for the PPO learner's tests (tests only; no kernels here).

* ``setup`` / ``reference`` / ``NAMES``: a perturbed ``MlpActorCritic`` with a synthetic one-step
  rollout, and ``ppo_update``'s minibatch loss through PyTorch autograd in a chosen dtype
  (tests/test_gpu_ppo.py, tests/test_gpu_ppo_edges.py).
* ``setup_cpu`` / ``to_device``: the same kind of inputs drawn from a CPU ``torch.Generator`` and
  then moved, so that what a test feeds the kernels can be checked without a GPU.
* ``edge_case``: the loss-branch cases of tests/test_gpu_ppo_edges.py. Each one chooses
  ``old_log_prob`` from the float64 forward so that every sample of the minibatch sits at least
  ``MARGIN`` away from each branch point of the clipped surrogate (tests/test_ppo_edge_inputs.py
  checks that on the CPU): the fp32 kernel and the fp64 reference then take the same branch on
  every sample, and ``clip_fraction`` can be compared exactly.
* ``clip_adam_ref``: ``clip_grad_norm_`` + ``torch.optim.Adam``'s step restated in float64."""
import copy
import types

import torch

NAMES = ["pi.W1", "pi.b1", "pi.W2", "pi.b2", "vf.W1", "vf.b1", "vf.W2", "vf.b2", "W_action", "b_action",
         "W_value", "b_value", "log_std"]
PI_NAMES = ("pi.W1", "pi.b1", "pi.W2", "pi.b2", "W_action", "b_action")  # what d loss / d log_prob reaches
VF_NAMES = ("vf.W1", "vf.b1", "vf.W2", "vf.b2", "W_value", "b_value")

# The distance every edge case keeps, in float64, between a sample's ratio and 1 - clip, 1, 1 + clip,
# and between its normalised advantage and 0: 25 x the ~4e-5 log-prob gap between the project's two
# fp32 forwards (test_rollout_and_learner_forwards_agree). The builders aim for BUILD_MARGIN, four
# times that, so that rounding old_log_prob and the advantages to fp32 cannot eat into it.
MARGIN = 1e-3
BUILD_MARGIN = 4e-3


def make_rollout(n, ns, na, obs, act, old_lp, adv, ret):
    return types.SimpleNamespace(n_steps=1, env=types.SimpleNamespace(num_envs=n, state_dim=ns, action_dim=na),
                                 obs=obs.view(1, n, ns), actions=act.view(1, n, na), log_probs=old_lp.view(1, n),
                                 advantages=adv.view(1, n), returns=ret.view(1, n))


def setup(ns, na, n, seed=0):
    from rl_rocket_amd.rollout import MlpActorCritic

    g = torch.Generator("cuda:0").manual_seed(seed)
    torch.manual_seed(seed)
    pol = MlpActorCritic(ns, na).cuda()
    with torch.no_grad():  # off SB3's small-gain init so every weight and bias matters
        for p in pol.parameters():
            p.add_(0.2 * torch.randn(p.shape, device="cuda:0", generator=g))
    f = dict(device="cuda:0", dtype=torch.float32)
    obs = 0.7 * torch.randn((n, ns), generator=g, **f)
    act = torch.randn((n, na), generator=g, **f)
    with torch.no_grad():
        mean, _ = pol(obs)
        old_lp = pol.log_prob(mean, act) + 0.25 * torch.randn((n,), generator=g, **f)  # ratios on both sides of the clip
    adv = 2.0 * torch.randn((n,), generator=g, **f) + 0.3
    ret = 5.0 * torch.randn((n,), generator=g, **f)
    return pol, make_rollout(n, ns, na, obs, act, old_lp, adv, ret), g


def setup_cpu(ns, na, n, seed=0, obs_scale=0.7, log_std=None):
    """`setup` on the CPU, every draw from one CPU generator (the policy's own initialisation under
    a forked global seed): the same tensors on every machine. obs_scale scales the observations,
    log_std (a float) overrides every component of the policy's."""
    from rl_rocket_amd.rollout import MlpActorCritic

    g = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        pol = MlpActorCritic(ns, na)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g))
        if log_std is not None:
            pol.log_std.fill_(float(log_std))
    obs = obs_scale * torch.randn((n, ns), generator=g)
    act = torch.randn((n, na), generator=g)
    with torch.no_grad():
        mean, _ = pol(obs)
        old_lp = pol.log_prob(mean, act) + 0.25 * torch.randn((n,), generator=g)
    adv = 2.0 * torch.randn((n,), generator=g) + 0.3
    ret = 5.0 * torch.randn((n,), generator=g)
    return pol, make_rollout(n, ns, na, obs, act, old_lp, adv, ret), g


def to_device(pol, ro, device="cuda:0"):
    """Copies of a CPU policy and rollout on `device` (the originals stay as they are)."""
    n, ns, na = ro.env.num_envs, ro.env.state_dim, ro.env.action_dim
    t = [x.reshape(-1).to(device).contiguous() for x in (ro.obs, ro.actions, ro.log_probs, ro.advantages, ro.returns)]
    return copy.deepcopy(pol).to(device), make_rollout(n, ns, na, *t)


def reference(pol, ro, idx, dtype, clip=0.2, ent_coef=0.01, vf_coef=0.5):
    """ppo_update's loss for one minibatch (autograd) in `dtype`."""
    from rl_rocket_amd.rollout import _policy_tensors

    p = copy.deepcopy(pol).to(dtype)
    n = ro.env.num_envs
    obs = ro.obs.reshape(n, -1)[idx].to(dtype)
    act = ro.actions.reshape(n, -1)[idx].to(dtype)
    old = ro.log_probs.reshape(n)[idx].to(dtype)
    adv = ro.advantages.reshape(n)[idx].to(dtype)
    ret = ro.returns.reshape(n)[idx].to(dtype)
    mean, value = p(obs)
    lp = p.log_prob(mean, act)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old)
    pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vf = torch.nn.functional.mse_loss(ret, value)
    ent = -p.entropy(len(idx)).mean()
    (pg + ent_coef * ent + vf_coef * vf).backward()
    with torch.no_grad():
        lr = lp - old
        stats = [pg.item(), vf.item(), -ent.item(), ((ratio - 1).abs() > clip).double().mean().item(),
                 ((torch.exp(lr) - 1) - lr).mean().item()]
    return [t.grad.double() for t in _policy_tensors(p)], stats


def clip_coef64(grads, max_norm):
    """clip_grad_norm_'s coefficient for fp64 gradients: min(1, max_norm / (||g|| + 1e-6))."""
    norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    return min(1.0, max_norm / (norm.item() + 1e-6))


def ratios64(pol, ro, idx):
    """(ratio, normalised advantage) of the minibatch in float64: what `reference` branches on."""
    p = copy.deepcopy(pol).double()
    n = ro.env.num_envs
    with torch.no_grad():
        mean, _ = p(ro.obs.reshape(n, -1)[idx].double())
        lp = p.log_prob(mean, ro.actions.reshape(n, -1)[idx].double())
        adv = ro.advantages.reshape(n)[idx].double()
        A = (adv - adv.mean()) / (adv.std() + 1e-8)
        return torch.exp(lp - ro.log_probs.reshape(n)[idx].double()), A


def _off_the_edges(r, clip):
    """Ratios closer than BUILD_MARGIN to 1 - clip, 1 or 1 + clip moved out to that distance, on
    the side they were on (the edges are 0 or >= 0.05 apart: one move cannot land near another)."""
    for b in sorted({1.0 - clip, 1.0, 1.0 + clip}):
        near = (r - b).abs() < BUILD_MARGIN
        r = torch.where(near, b + torch.where(r >= b, BUILD_MARGIN, -BUILD_MARGIN), r)
    return r


def _advantages_off_zero(adv, idx):
    """The minibatch's raw advantages nudged, in place, until no normalised one is within
    BUILD_MARGIN of 0 (each nudge moves the mean by ~1e-5 standard deviations: a pass or two)."""
    for _ in range(20):
        a = adv[idx].double()
        A = (a - a.mean()) / (a.std() + 1e-8)
        near = A.abs() < BUILD_MARGIN
        if not near.any():
            return
        step = 3.0 * BUILD_MARGIN * a.std()
        adv[idx] = torch.where(near, a + torch.where(A >= 0, step, -step), a).float()
    raise AssertionError("advantages still within the margin of the minibatch mean")


# name -> (loss coefficients, what is special about the inputs)
EDGE_CASES = {
    "clipped": {},         # r beyond the clip on the side where min() picks the clipped term
    "mirror": {},          # r beyond the clip on the side where min() picks the unclipped term
    "clip0": dict(clip=0.0),
    "clip0.05": dict(clip=0.05),
    "clip0.4": dict(clip=0.4),
    "const_adv": {},       # one fp32 value: std 0, normalised advantages 0
    "offset_adv": {},      # 50 + 0.5 randn
    "vf0": dict(vf_coef=0.0),
    "vf1.3": dict(vf_coef=1.3),
    "ent0": dict(ent_coef=0.0),
    "ent0.3": dict(ent_coef=0.3),
    "saturated": {},       # obs x 30: most hidden units at +-1
    "logstd-2": {},        # log_std on every component; the actions drawn from that policy
    "logstd+1": {},
}
EDGE_BATCHES = (1000, 33)


def edge_case(name, bs, ns=14, na=3, n=1500):
    """One loss-branch case, on the CPU: a namespace of pol, ro, idx (bs distinct rows of n), coef
    (the clip_range / ent_coef / vf_coef keywords of `reference` and PPOGrad) and name."""
    coef = dict(clip=0.2, ent_coef=0.01, vf_coef=0.5)
    coef.update(EDGE_CASES[name])
    clip = coef["clip"]
    seed = 1000 + 10 * sorted(EDGE_CASES).index(name) + (bs & 1)
    kw = {}
    if name == "saturated":
        kw["obs_scale"] = 0.7 * 30.0
    if name.startswith("logstd"):
        kw["log_std"] = float(name[len("logstd"):])
    pol, ro, g = setup_cpu(ns, na, n, seed=seed, **kw)
    idx = torch.randperm(n, generator=g)[:bs].contiguous()
    if name.startswith("logstd"):
        # Actions as a rollout draws them, mean + exp(log_std) eps, so that |log_prob| stays O(10).
        # setup's unit-normal actions sit ~7 sigma off the mean at log_std -2: log-probs of -160 on
        # average and down to -1100, where one fp32 ulp of the log-prob (1.5e-5 .. 1.2e-4) is a
        # relative step of the ratio that no fp32 forward can stay inside the statistics' 1e-5 bar with.
        with torch.no_grad():
            mean, _ = copy.deepcopy(pol).double()(ro.obs.view(n, ns).double())
            eps = torch.randn((n, na), generator=g, dtype=torch.float64)
            ro.actions.view(n, na).copy_((mean + pol.log_std.double().exp() * eps).float())
    adv = ro.advantages.view(n)
    if name == "const_adv":
        adv[idx] = 0.3
    else:
        if name == "offset_adv":
            adv[idx] = 50.0 + 0.5 * torch.randn((bs,), generator=g)
        _advantages_off_zero(adv, idx)
    # the ratios: drawn in float64 around the float64 forward's log-prob, old_log_prob follows
    _, A = ratios64(pol, ro, idx)
    u = torch.rand((bs,), generator=g, dtype=torch.float64)
    above = (1.0 + clip) + BUILD_MARGIN + 0.3 * u
    below = (1.0 - clip) * (1.0 - 0.5 * u) - BUILD_MARGIN
    if name == "clipped":
        r = torch.where(A > 0, above, below)
    elif name == "mirror":
        r = torch.where(A > 0, below, above)
    else:
        r = _off_the_edges(torch.exp(0.25 * torch.randn((bs,), generator=g, dtype=torch.float64)), clip)
    p64 = copy.deepcopy(pol).double()
    with torch.no_grad():
        mean, _ = p64(ro.obs.view(n, ns)[idx].double())
        lp = p64.log_prob(mean, ro.actions.view(n, na)[idx].double())
        ro.log_probs.view(n)[idx] = (lp - torch.log(r)).float()
    return types.SimpleNamespace(name=name, bs=bs, pol=pol, ro=ro, idx=idx, coef=coef)


def clip_adam_ref(params, grads, state, max_norm, lr, betas=(0.9, 0.999), eps=1e-5):
    """One clip_grad_norm_ + torch.optim.Adam step (no weight decay, no amsgrad) in float64, in
    place on the lists of fp64 tensors `params` and state = dict(step, exp_avg, exp_avg_sq);
    returns the clipped gradients. max_norm <= 0: no clip.
      coef = min(1, max_norm / (||g|| + 1e-6)); g *= coef; step += 1
      m = m + (1 - b1) (g - m); v = b2 v + (1 - b2) g g
      p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)"""
    b1, b2 = betas
    coef = clip_coef64(grads, max_norm) if max_norm > 0 else 1.0
    state["step"] += 1
    t = state["step"]
    out = []
    for p, g, m, v in zip(params, grads, state["exp_avg"], state["exp_avg_sq"]):
        g = g.double() * coef
        m.add_((1.0 - b1) * (g - m))
        v.mul_(b2).add_((1.0 - b2) * g * g)
        p.sub_(lr / (1.0 - b1 ** t) * m / (v.sqrt() / (1.0 - b2 ** t) ** 0.5 + eps))
        out.append(g)
    return out
