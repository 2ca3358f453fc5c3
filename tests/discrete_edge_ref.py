"""Inputs of the Categorical PPO learner's edge tests (tests only; no kernels here, and nothing that calls
one): tests/test_discrete_edge_inputs.py checks every condition on the CPU, tests/test_gpu_discrete_edges.py
feeds the same inputs to rr_ppo_update_discrete. Every draw comes from a CPU generator.

* ``sweep_pool`` / ``sweep_inputs`` / ``minibatch``: one policy and 70 001-row rollout per K
  (discrete_ref.learner_inputs) and the rows of a sweep case, as test_gpu_ppo_edges._sweep_inputs has them.
* ``edge_case``: ppo_ref.edge_case's loss-branch cases for the softmax head, with ppo_ref's margins and
  its two helpers (_off_the_edges, _advantages_off_zero), plus the cases only a softmax head has.
* ``admission``: the fp32 reference's error against the float64 one as a share of each of the project's
  bars; a case is used only where every share is at most ADMIT.
"""
import types

import torch

import discrete_ref as D
import ppo_ref as P

N_ROWS = 70001
SWEEP = [(bs, 4) for bs in (3, 31, 32, 33, 127, 128, 129, 4096, 4097, 16256, 16384, 16385, 40000, 40001, 65537, 70001)]
SWEEP += [(bs, 3) for bs in (33, 4097, 16385)]
SWEEP += [(bs, 2) for bs in (3, 31, 32, 33, 4097, 16385, 40001)]

_pool, _device_pool = {}, {}


def sweep_pool(k):
    """(policy, rollout) of the batch-size sweep for K = k, on the CPU; cached, read-only."""
    if k not in _pool:
        _pool[k] = D.learner_inputs(k, n=N_ROWS, seed=200 + k)[:2]
    return _pool[k]


def sweep_inputs(k):
    """sweep_pool(k) moved to the device once; read-only."""
    if k not in _device_pool:
        _device_pool[k] = D.to_device(*sweep_pool(k))
    return _device_pool[k]


def minibatch(n, bs, extra=0):
    """bs + extra distinct rows of n, from a generator seeded with bs (test_gpu_ppo_edges._minibatch, on the CPU)."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(bs))[:bs + extra].contiguous()


# name -> the loss coefficients off their defaults. What is special about the inputs is beside each name.
EDGE_CASES = dict(P.EDGE_CASES)
del EDGE_CASES["logstd-2"], EDGE_CASES["logstd+1"]  # no log_std here
EDGE_CASES.update({
    "clipped_ent0": dict(ent_coef=0.0),  # `clipped` without the entropy's gradient: nothing reaches the pi side
    "peaked": {},                        # head_scale PEAKED_HEAD_SCALE: the largest probability near 1
    "all_first": {},                     # every action of the minibatch is index 0
    "all_last": {},                      # ... is index K - 1, the last head before the zero-packed ones
})
EDGE_BATCHES = P.EDGE_BATCHES
# every name at K = 4, and the cases where the sign of the advantage or its absence decides at K = 2 and 3
EDGES = [(name, bs, 4) for name in EDGE_CASES for bs in EDGE_BATCHES]
EDGES += [(name, bs, k) for k in (2, 3) for name in ("clipped", "mirror", "const_adv") for bs in EDGE_BATCHES]

# What the admission rule (ADMIT below; tests/test_discrete_edge_inputs.py asserts it and prints every share)
# decided about the inputs. The shares are the fp32 reference's error over the bar, the worst over both sizes.
#   peaked     cat_policy's head_scale (0.5 elsewhere): the smallest of 2, 4, 8, 16 at which the float64
#              largest probability exceeds PEAK_P on at least half of both minibatches (0.75 of the 1000 rows,
#              0.73 of the 33; at 4 it is 0.55 and 0.45). Worst share 0.05 (pi.b2): nothing had to be lowered.
#   saturated  ppo_ref's obs x 30 as it is: worst share 0.07 (policy_loss).
#   all_last   learner_inputs' policy as it is: worst share 0.02 (approx_kl).
#   offset_adv ppo_ref's 50 + 0.5 randn is not admitted: the fp32 reference's own mean and std of advantages
#              near 50 leave its policy_loss 4.8 (1000 rows) and 10.0 (33 rows) bars off the float64 one; at
#              an offset of 20 the shares are 1.8 and 2.0, at 10 they are 0.20 and 2.0. OFFSET_ADV 5 is the
#              largest of 50, 20, 10, 5 that is admitted at both sizes: worst share 0.25 (policy_loss, 33
#              rows). The mean is still 10 standard deviations from 0. (Measured once, outside the suite: the
#              kernel itself on 50 + 0.5 randn is at 0.04 of policy_loss's bar; it sums in float64.)
#   const_adv  CONST_ADV 0.25, not ppo_ref's 0.3: the fp32 reference's mean of 33 x 0.3f is an ulp off 0.3f,
#              and (adv - mean) / (0 + 1e-8) makes advantages of order 1 of that (its policy_loss then misses
#              the bar 7e5-fold). Sums of k x 0.25 are exact in any order and in either precision, so both
#              references normalise to exactly 0. (test_gpu_discrete.test_entropy_gradient_alone_and_switched_off
#              runs the kernel on 0.3, which its float64 sums take.) Worst share 0.01.
PEAKED_HEAD_SCALE = 8.0
PEAK_P = 0.99
SATURATED_OBS = 30.0
OFFSET_ADV = 5.0
CONST_ADV = 0.25


def normalised_advantages(ro, idx):
    a = ro.advantages.reshape(-1)[idx].double()
    return (a - a.mean()) / (a.std() + 1e-8)


def edge_case(name, bs, k, n=1500):
    """One loss-branch case on the CPU: a namespace of pol, ro, idx (bs distinct rows of n), coef (the clip /
    ent_coef / vf_coef keywords of discrete_ref.loss_reference) and name, bs, k. The old log-probs of the
    minibatch follow from the float64 log-softmax at the chosen ratios."""
    coef = dict(clip=0.2, ent_coef=0.01, vf_coef=0.5)
    coef.update(EDGE_CASES[name])
    clip = coef["clip"]
    seed = 2000 + 100 * k + 10 * sorted(EDGE_CASES).index(name) + (bs & 1)
    kw = {}
    if name == "saturated":
        kw["obs_scale"] = 0.7 * SATURATED_OBS
    if name == "peaked":
        kw["head_scale"] = PEAKED_HEAD_SCALE
    pol, ro, g = D.learner_inputs(k, n=n, seed=seed, clip=clip, **kw)
    idx = torch.randperm(n, generator=g)[:bs].contiguous()
    if name in ("all_first", "all_last"):
        ro.actions.view(n)[idx] = 0.0 if name == "all_first" else float(k - 1)
    adv = ro.advantages.view(n)
    if name == "const_adv":
        adv[idx] = CONST_ADV
    else:
        if name == "offset_adv":
            adv[idx] = OFFSET_ADV + 0.5 * torch.randn((bs,), generator=g)
        P._advantages_off_zero(adv, idx)
    A = normalised_advantages(ro, idx)
    u = torch.rand((bs,), generator=g, dtype=torch.float64)
    above = (1.0 + clip) + P.BUILD_MARGIN + 0.3 * u
    below = (1.0 - clip) * (1.0 - 0.5 * u) - P.BUILD_MARGIN
    if name in ("clipped", "clipped_ent0"):
        r = torch.where(A > 0, above, below)
    elif name == "mirror":
        r = torch.where(A > 0, below, above)
    else:
        r = P._off_the_edges(torch.exp(0.25 * torch.randn((bs,), generator=g, dtype=torch.float64)), clip)
    lp = torch.from_numpy(D.forward64(pol, ro.obs.view(n, 7)[idx])[2])
    lp = lp.gather(1, ro.actions.view(n)[idx].long()[:, None])[:, 0]
    ro.log_probs.view(n)[idx] = (lp - torch.log(r)).float()
    return types.SimpleNamespace(name=name, bs=bs, k=k, pol=pol, ro=ro, idx=idx, coef=coef)


STATS = ("policy_loss", "value_loss", "entropy", "clip_fraction", "approx_kl")
ADMIT = 0.5


def admission(pol, ro, idx, **coef):
    """discrete_ref.loss_reference in torch.float32 against itself in float64, as shares of the project's bars
    (per tensor 1e-4 max |fp64| + 1e-7, statistics 1e-5 |r| + 1e-6): ({tensor or statistic: share}, the two
    clip fractions' difference in samples, the float64 gradients, the float64 statistics)."""
    ref64, st64 = D.loss_reference(pol, ro, idx, torch.float64, **coef)
    ref32, st32 = D.loss_reference(pol, ro, idx, torch.float32, **coef)
    share = {}
    for name, a, r in zip(D.NAMES, ref32, ref64):
        share[name] = (a - r).abs().max().item() / (1e-4 * r.abs().max().item() + 1e-7)
    for name, a, r in zip(STATS, st32, st64):
        if name != "clip_fraction":
            share[name] = abs(a - r) / (1e-5 * abs(r) + 1e-6)
    return share, abs(st32[3] - st64[3]) * idx.numel(), ref64, st64
