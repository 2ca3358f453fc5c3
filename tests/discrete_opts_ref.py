"""Inputs and float64 references for the Categorical learner's SB3 options (rr_ppo_update_discrete_opts:
clip_range_vf, normalize_advantage=False, target_kl and the train() log means). Tests only; no kernels
here, and nothing that calls one: tests/test_discrete_opts_host.py checks every input condition on the
CPU, tests/test_gpu_discrete_opts.py feeds the same inputs to the kernels.

* ``reference``: SB3 1.6 PPO.train's minibatch loss with ``torch.distributions.Categorical`` and the
  options, through autograd in float64: discrete_ref.loss_reference plus the two lines of
  ppo_opts_ref.reference (``values_pred = old + clamp(V - old, -c, c)``, the raw advantages).
* ``vclip_case``: ppo_opts_ref.vclip_case's construction on discrete_ref.learner_inputs. Built with
  ``VBUILD`` (ppo_ref.BUILD_MARGIN and a little more, so that the fp32 rounding of the stored
  old values leaves |V - old| at least BUILD_MARGIN off c).
* ``raw_case``: the 50 + 0.5 randn advantages, optionally with old values 0.1 / 0.4 off V.
* ``train_ref``: ppo_opts_ref.train_ref over the 12 tensors (ppo_ref.clip_adam_ref).
* ``kl_case``: the KL-stop inputs, with ppo_opts_ref.pick_target, KL_GAP and KL_FLOOR as they are.
"""
import copy
import types

import torch

import discrete_ref as D
import ppo_opts_ref as R
import ppo_ref as P

STAT_NAMES = R.STAT_NAMES
NAMES = D.NAMES
VF_NAMES = P.VF_NAMES
COEF = dict(clip=0.2, ent_coef=0.01, vf_coef=0.5)


def with_values(ro, old_values):
    """discrete_ref.make_rollout's namespace with the rollout's values beside the other tensors."""
    out = copy.copy(ro)
    out.values = old_values.reshape(1, ro.env.num_envs)
    return out


def to_device(pol, ro, device="cuda:0"):
    pol_d, ro_d = D.to_device(pol, ro, device)
    if getattr(ro, "values", None) is not None:
        ro_d.values = ro.values.reshape(1, -1).to(device).contiguous()
    return pol_d, ro_d


def reference(pol, ro, idx, dtype=torch.float64, clip=0.2, ent_coef=0.01, vf_coef=0.5, clip_range_vf=None,
              normalize_advantage=True):
    """SB3 1.6 PPO.train's loss for one minibatch with a Categorical distribution (autograd) in `dtype`
    on the CPU: (the 12 gradients in float64, [policy_loss, value_loss, entropy, clip_fraction, approx_kl])."""
    from rl_rocket_amd.rollout import _policy_tensors

    p = copy.deepcopy(pol).to(dtype).cpu()
    idx = idx.cpu()
    n = ro.env.num_envs
    obs = ro.obs.reshape(n, -1).cpu()[idx].to(dtype)
    act = ro.actions.reshape(n).cpu()[idx].long()
    old = ro.log_probs.reshape(n).cpu()[idx].to(dtype)
    adv = ro.advantages.reshape(n).cpu()[idx].to(dtype)
    ret = ro.returns.reshape(n).cpu()[idx].to(dtype)
    logits, value = p(obs)
    dist = torch.distributions.Categorical(logits=logits)
    lp = dist.log_prob(act)
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old)
    pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    if clip_range_vf is not None:
        old_v = ro.values.reshape(n).cpu()[idx].to(dtype)
        value = old_v + torch.clamp(value - old_v, -clip_range_vf, clip_range_vf)
    vf = torch.nn.functional.mse_loss(ret, value)
    ent = -dist.entropy().mean()
    (pg + ent_coef * ent + vf_coef * vf).backward()
    with torch.no_grad():
        lr = lp - old
        stats = [pg.item(), vf.item(), -ent.item(), ((ratio - 1).abs() > clip).double().mean().item(),
                 ((torch.exp(lr) - 1) - lr).mean().item()]
    return [t.grad.double() for t in _policy_tensors(p)], stats


def values(pol, ro, idx, dtype):
    """V of the minibatch from the forward in `dtype`, as float64."""
    p = copy.deepcopy(pol).to(dtype)
    n = ro.env.num_envs
    with torch.no_grad():
        return p(ro.obs.reshape(n, -1)[idx].to(dtype))[1].reshape(-1).double()


VCLIP_KINDS = R.VCLIP_KINDS
VCLIP_SHAPES = ((4, 33), (4, 1000), (2, 33), (3, 33))  # (n_choices, minibatch rows)
VCLIP_C = R.VCLIP_C
# old values are stored in fp32: |V - old| ~ 1 moves by up to an ulp of |old| (<= 1e-6 for |old| < 8)
VBUILD = P.BUILD_MARGIN + 1e-5


def vclip_case(kind, k, bs, n=1500):
    """A value-clip case on the CPU: namespace of pol, ro (with .values), idx, c, coef. The kinds are
    ppo_opts_ref.vclip_case's; the minibatch's returns are V + 0.5 randn, the ratios learner_inputs'
    (off the clip's edges)."""
    seed = 3000 + 100 * VCLIP_KINDS.index(kind) + 10 * k + (bs & 1)
    pol, ro, g = D.learner_inputs(k, n=n, seed=seed)
    idx = torch.randperm(n, generator=g)[:bs].contiguous()
    V = values(pol, ro, idx, torch.float64)
    u = torch.rand((bs,), generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand((bs,), generator=g) < 0.5, -1.0, 1.0).double()
    M = VBUILD
    c = VCLIP_C
    if kind == "half":
        d = 0.3 * torch.randn((bs,), generator=g, dtype=torch.float64)
        c = float(d.abs().median())
        near = (d.abs() - c).abs() < M
        d = torch.where(near, torch.sign(d) * (c + torch.where(d.abs() >= c, M, -M)), d)
    else:
        inside = (c - M) * u
        outside = c + M + 0.3 * u
        pick = {"inside": torch.ones(bs, dtype=torch.bool), "outside": torch.zeros(bs, dtype=torch.bool),
                "mixed": torch.rand((bs,), generator=g) < 0.5}[kind]
        d = sign * torch.where(pick, inside, outside)
    old = torch.zeros(n)  # rows outside the minibatch keep 0: the kernel must not read them
    old[idx] = (V - d).float()
    ro.returns.view(n)[idx] = (V + 0.5 * torch.randn((bs,), generator=g, dtype=torch.float64)).float()
    return types.SimpleNamespace(kind=kind, k=k, bs=bs, pol=pol, ro=with_values(ro, old), idx=idx, c=c, coef=dict(COEF))


def vclip_distance(case):
    """(| |V - old| - c | per sample, fraction outside the clip) in float64, old as stored (fp32)."""
    V = values(case.pol, case.ro, case.idx, torch.float64)
    d = (V - case.ro.values.reshape(-1)[case.idx].double()).abs()
    return (d - case.c).abs(), (d > case.c).double().mean().item()


RAW_SHAPES = ((4, 33), (4, 1000), (3, 33))


def raw_case(k, bs, vclip, n=1500):
    """normalize_advantage=False on advantages 50 + 0.5 randn (ppo_ref's offset_adv), alone or with rollout
    values a fixed 0.1 (inside) or 0.4 (outside) either side of V at c = 0.2."""
    pol, ro, g = D.learner_inputs(k, n=n, seed=4000 + 10 * k + (bs & 1))
    idx = torch.randperm(n, generator=g)[:bs].contiguous()
    ro.advantages.view(n)[idx] = 50.0 + 0.5 * torch.randn((bs,), generator=g)
    opts = dict(normalize_advantage=False)
    if vclip:
        V = values(pol, ro, torch.arange(n), torch.float64)
        d = torch.where(torch.rand(n, generator=g) < 0.5, 0.1, 0.4)
        d = d * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        ro = with_values(ro, (V - d).float())
        opts["clip_range_vf"] = VCLIP_C
    return types.SimpleNamespace(k=k, bs=bs, pol=pol, ro=ro, idx=idx, opts=opts, coef=dict(COEF))


# ---- PPO.train in float64 ----

def train_ref(pol, ro, perms, sizes, target_kl=None, clip=0.2, ent_coef=0.01, vf_coef=0.5, max_norm=0.5, lr=1e-3,
              eps=1.0, clip_range_vf=None, normalize_advantage=True):
    """ppo_opts_ref.train_ref with the Categorical loss over the policy's 12 tensors: SB3 1.6 PPO.train in
    float64, its ``break`` ahead of the optimizer step, clip_grad_norm_ and Adam (ppo_ref.clip_adam_ref),
    and its log means."""
    from rl_rocket_amd.rollout import _policy_tensors

    p = copy.deepcopy(pol).double()
    params = [t.data for t in _policy_tensors(p)]
    state = dict(step=0, exp_avg=[torch.zeros_like(t) for t in params], exp_avg_sq=[torch.zeros_like(t) for t in params])
    pg_losses, value_losses, entropy_losses, clip_fractions, kls = [], [], [], [], []
    approx_kl_divs = []
    stop_epoch = None
    for epoch, perm in enumerate(perms):
        approx_kl_divs = []
        for idx in torch.split(perm[:sum(sizes)], list(sizes)):
            grads, st = reference(p, ro, idx, torch.float64, clip, ent_coef, vf_coef, clip_range_vf, normalize_advantage)
            pg_losses.append(st[0])
            value_losses.append(st[1])
            entropy_losses.append(-st[2])
            clip_fractions.append(st[3])
            approx_kl_divs.append(st[4])
            kls.append(st[4])
            if target_kl is not None and st[4] > 1.5 * target_kl:
                stop_epoch = epoch
                break
            P.clip_adam_ref(params, grads, state, max_norm, lr, eps=eps)
        if stop_epoch is not None:
            break
    mean = lambda v: sum(v) / len(v)  # noqa: E731
    log = {"train/policy_gradient_loss": mean(pg_losses), "train/value_loss": mean(value_losses),
           "train/entropy_loss": mean(entropy_losses), "train/clip_fraction": mean(clip_fractions),
           "train/approx_kl": mean(approx_kl_divs)}
    return types.SimpleNamespace(params=params, exp_avg=state["exp_avg"], exp_avg_sq=state["exp_avg_sq"],
                                 steps=state["step"], evals=len(kls), stop_epoch=stop_epoch, kls=kls, log=log)


KL_SIZES, KL_EPOCHS, KL_PLACES, KL_MOVED = R.KL_SIZES, R.KL_EPOCHS, R.KL_PLACES, R.KL_MOVED
KL_GAP, KL_FLOOR, pick_target = R.KL_GAP, R.KL_FLOOR, R.pick_target
# The knobs of kl_inputs, chosen on the CPU (tests/test_discrete_opts_host.py prints every case's
# approx_kl). The Gaussian helper's displacement and returns stay. Its learning rate 1e-3 leaves the
# unmoved cases' approx_kl at 3e-9 .. 1e-7, below KL_FLOOR: this policy's gradient norm is ~0.1, under
# clip_grad_norm_'s 0.5, so a step is lr g / (|g| + eps) with Adam's eps 1.0 and the returns' distance
# from V changes nothing. At 1e-2 approx_kl runs 3e-7 .. 1e-5 as it does there, every place of
# KL_PLACES admits a target with the unchanged gaps, and a step still moves a parameter by ~1e-4.
KL_DISPLACEMENT, KL_LR, KL_RETURN_NOISE = 0.02, 1e-2, 0.5
_kl_cache = {}


def kl_inputs(k=4, sizes=KL_SIZES, n_epochs=KL_EPOCHS, seed=41, moved=False, perms=None, n=None):
    """ppo_opts_ref.kl_inputs for the Categorical policy: old_log_prob is the float64 forward's log-prob of
    the unmoved policy (rounded to fp32), returns = V + KL_RETURN_NOISE randn, and with `moved` the
    learner's policy is the rollout's with every parameter displaced by KL_DISPLACEMENT randn."""
    n = sum(sizes) + 11 if n is None else n
    pol, ro, g = D.learner_inputs(k, n=n, seed=seed)
    _, v64, lp64 = D.forward64(pol, ro.obs.view(n, 7))
    lp64, v64 = torch.from_numpy(lp64), torch.from_numpy(v64).reshape(n)
    with torch.no_grad():
        ro.log_probs.view(n).copy_(lp64.gather(1, ro.actions.view(n).long()[:, None])[:, 0].float())
        ro.returns.view(n).copy_((v64 + KL_RETURN_NOISE * torch.randn(n, generator=g, dtype=torch.float64)).float())
        if moved:
            for t in pol.parameters():
                t.add_(KL_DISPLACEMENT * torch.randn(t.shape, generator=g))
    if perms is None:
        perms = [torch.randperm(n, generator=g)[:sum(sizes)].contiguous() for _ in range(n_epochs)]
    return pol, ro, perms


def kl_case(name):
    """One KL-stop case on the CPU (cached): ppo_opts_ref.kl_case's namespace."""
    if name in _kl_cache:
        return _kl_cache[name]
    pol, ro, perms = kl_inputs(moved=name in KL_MOVED)
    free = train_ref(pol, ro, perms, KL_SIZES, lr=KL_LR)
    for place in KL_PLACES[name]:
        target = pick_target(free.kls, place)
        if target is not None:
            break
    else:
        raise AssertionError("no admissible stop for %s in approx_kl %s" % (name, free.kls))
    ref = train_ref(pol, ro, perms, KL_SIZES, target_kl=target, lr=KL_LR)
    _kl_cache[name] = types.SimpleNamespace(name=name, pol=pol, ro=ro, perms=perms, sizes=KL_SIZES, target_kl=target,
                                            place=place, free=free, ref=ref)
    return _kl_cache[name]
