"""The input conditions of the PPO learner's loss-branch cases (tests/ppo_ref.py edge_case, run on
the GPU by tests/test_gpu_ppo_edges.py), checked in float64 on the CPU: every sample of every
minibatch keeps its ratio at least MARGIN away from 1 - clip, 1 and 1 + clip and, where the sign of
the normalised advantage picks a branch, that advantage at least MARGIN away from 0; the quadrant
cases hold every sample in its quadrant; constant advantages normalise to exactly 0. No sample is
left out of any of it: the fp32 kernel and the fp64 reference branch alike on the whole minibatch."""
import copy

import pytest
import torch

import ppo_ref as P

CASES = [(name, bs) for name in P.EDGE_CASES for bs in P.EDGE_BATCHES]


@pytest.fixture(scope="module", params=CASES, ids=["%s-%d" % c for c in CASES])
def case(request):
    c = P.edge_case(*request.param)
    c.r, c.A = P.ratios64(c.pol, c.ro, c.idx)
    return c


def test_minibatch_is_whole_and_finite(case):
    n = case.ro.env.num_envs
    assert case.idx.dtype == torch.int64 and case.idx.numel() == case.bs
    assert len(set(case.idx.tolist())) == case.bs and 0 <= int(case.idx.min()) and int(case.idx.max()) < n
    assert case.r.numel() == case.A.numel() == case.bs  # nothing masked out below
    for t in (case.ro.obs, case.ro.actions, case.ro.log_probs, case.ro.advantages, case.ro.returns):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    assert bool(torch.isfinite(case.r).all()) and bool((case.r > 0).all())


def test_every_ratio_keeps_the_margin(case):
    clip = case.coef["clip"]
    for edge in (1.0 - clip, 1.0, 1.0 + clip):
        gap = (case.r - edge).abs().min().item()
        assert gap >= P.MARGIN, (case.name, case.bs, edge, gap)


def test_every_advantage_keeps_the_margin(case):
    if case.name == "const_adv":
        # (adv - mean) / (0 + 1e-8) with one fp32 value everywhere: exactly 0, no sign to decide
        assert torch.equal(case.A, torch.zeros_like(case.A))
        a = case.ro.advantages.reshape(-1)[case.idx]
        assert bool((a == a[0]).all()) and a[0].item() != 0.0
        return
    assert case.A.abs().min().item() >= P.MARGIN, (case.name, case.bs)
    assert bool((case.A > 0).any()) and bool((case.A < 0).any())


def test_quadrants(case):
    clip, r, A = case.coef["clip"], case.r, case.A
    out = (r - 1.0).abs() > clip
    if case.name == "clipped":  # min() picks the clamped term on every sample
        assert bool(((A > 0) & (r > 1 + clip + P.MARGIN) | (A < 0) & (r < 1 - clip - P.MARGIN)).all())
    elif case.name == "mirror":  # beyond the clip on the side where min() keeps the unclipped term
        assert bool(((A > 0) & (r < 1 - clip - P.MARGIN) | (A < 0) & (r > 1 + clip + P.MARGIN)).all())
    elif case.name == "clip0":
        assert bool(out.all())
    elif case.name == "const_adv":  # no sign of A: the ratios alone, on both sides and inside
        assert bool((r > 1 + clip).any()) and bool((r < 1 - clip).any()) and bool((~out).any())
    elif case.bs >= 1000:  # the general cases reach all four quadrants and the inside of the clip
        for sel in (A > 0, A < 0):
            assert bool((sel & (r > 1 + clip)).any()) and bool((sel & (r < 1 - clip)).any())
            assert bool((sel & ~out).any())
    if case.name in ("clipped", "mirror"):
        assert bool(out.all())


def test_special_inputs_are_what_the_names_say(case):
    obs = case.ro.obs.reshape(-1, 14)[case.idx]
    if case.name == "saturated":
        pre = obs.double() @ case.pol.pi_net[0].weight.double().T + case.pol.pi_net[0].bias.double()
        assert (pre.abs() > 9.0).double().mean().item() > 0.5  # 1 - tanh^2 < 2^-24: exactly 0 in fp32
        assert pre.abs().max().item() > 45.0  # exp(2 x) overflows fp32
    if case.name == "offset_adv":
        a = case.ro.advantages.reshape(-1)[case.idx]
        assert 49.5 < a.mean().item() < 50.5 and 0.3 < a.std().item() < 0.7
    if case.name.startswith("logstd"):
        assert bool((case.pol.log_std == float(case.name[6:])).all())
        # the actions are the policy's own draws: |log_prob| <= 32, an fp32 ulp of it <= 3.8e-6
        p = copy.deepcopy(case.pol).double()
        with torch.no_grad():
            mean, _ = p(obs.double())
            lp = p.log_prob(mean, case.ro.actions.reshape(-1, 3)[case.idx].double())
        assert lp.abs().max().item() <= 32.0
