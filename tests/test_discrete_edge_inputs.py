"""The inputs of tests/test_gpu_discrete_edges.py (tests/discrete_edge_ref.py), checked on the CPU before any
of them reaches a kernel. The case sets are defined once, in discrete_edge_ref: EDGES (every edge_case name at
1000 and 33 rows with K = 4; clipped, mirror and const_adv also at K = 2 and 3) and SWEEP (the batch-size
sweep's rows of the 70 001-row pools).

* Margins, in float64: every sample's ratio is at least ppo_ref.MARGIN from 1 - clip, 1 and 1 + clip; every
  normalised advantage at least MARGIN from 0 (const_adv: exactly 0); the quadrant cases hold every sample in
  its quadrant; the action column, the peaked probabilities and the saturated units are what the names say.
  No sample is left out: the fp32 kernel and the float64 reference branch alike on the whole minibatch.
* Admission: the project's bars (per tensor 1e-4 max |fp64| + 1e-7, statistics 1e-5 |r| + 1e-6) were not
  derived for a peaked softmax or for 70 001 rows. A case is used only if discrete_ref.loss_reference in
  torch.float32 stays within HALF of each bar against itself in float64, and counts the same clipped
  samples. Every share is printed (pytest -s). discrete_edge_ref's comments say which inputs that rule changed.
* The options call's cases at 4 097 and 16 385 rows of a 20 000-row pool keep discrete_opts_ref's margins."""
import pytest
import torch

import discrete_edge_ref as E
import discrete_opts_ref as Q
import discrete_ref as D
import ppo_ref as P

# The builders put a float64 ratio exactly BUILD_MARGIN off an edge, and old_log_prob is then stored in fp32:
# |log-prob| < 16 has an ulp of at most 1e-6 (tests/test_discrete_opts_host.py RATIO_MARGIN).
RATIO_MARGIN = P.BUILD_MARGIN - 1e-6


@pytest.fixture(scope="module", params=E.EDGES, ids=["%s-%d-k%d" % c for c in E.EDGES])
def case(request):
    c = E.edge_case(*request.param)
    c.r, c.A = D.ratios64(c.pol, c.ro, c.idx), E.normalised_advantages(c.ro, c.idx)
    c.share, c.dclip, c.ref64, c.st64 = E.admission(c.pol, c.ro, c.idx, **c.coef)
    return c


def _print_shares(label, share, dclip):
    worst = max(share, key=share.get)
    print("%s: fp32 reference / bar: worst %s %.3f; clip_fraction off by %.1f samples; %s"
          % (label, worst, share[worst], dclip, " ".join("%s %.3f" % kv for kv in share.items())))


def test_case_sets_are_the_ones_the_gpu_file_runs():
    assert len(E.EDGES) == len(set(E.EDGES)) == 2 * len(E.EDGE_CASES) + 12 and len(E.EDGE_CASES) == 16
    for name in ("clipped", "mirror", "clip0", "clip0.05", "clip0.4", "const_adv", "offset_adv", "vf0", "vf1.3", "ent0",
                 "ent0.3", "saturated", "clipped_ent0", "peaked", "all_first", "all_last"):
        assert (name, 1000, 4) in E.EDGES and (name, 33, 4) in E.EDGES
    for name, rest in P.EDGE_CASES.items():  # the shared names keep ppo_ref's coefficients
        assert name.startswith("logstd") or E.EDGE_CASES[name] == rest
    assert [bs for bs, k in E.SWEEP if k == 4] == [3, 31, 32, 33, 127, 128, 129, 4096, 4097, 16256, 16384, 16385, 40000,
                                                   40001, 65537, 70001]  # test_gpu_ppo_edges.SWEEP's at (14, 3)
    assert [bs for bs, k in E.SWEEP if k == 3] == [33, 4097, 16385]
    assert [bs for bs, k in E.SWEEP if k == 2] == [3, 31, 32, 33, 4097, 16385, 40001]
    assert len(E.SWEEP) == 26 and (E.ADMIT, P.MARGIN, P.BUILD_MARGIN) == (0.5, 1e-3, 4e-3)


def test_minibatch_is_whole_and_finite(case):
    n = case.ro.env.num_envs
    assert case.idx.dtype == torch.int64 and case.idx.numel() == case.bs
    assert len(set(case.idx.tolist())) == case.bs and 0 <= int(case.idx.min()) and int(case.idx.max()) < n
    assert case.r.numel() == case.A.numel() == case.bs  # nothing masked out below
    for t in (case.ro.obs, case.ro.actions, case.ro.log_probs, case.ro.advantages, case.ro.returns):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    act = case.ro.actions.reshape(-1)
    assert torch.equal(act, act.long().float()) and int(act.min()) >= 0 and int(act.max()) < case.k
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
        assert bool((a == a[0]).all()) and a[0].item() == E.CONST_ADV != 0.0
        assert case.st64[0] == 0.0
        return
    assert case.A.abs().min().item() >= P.MARGIN, (case.name, case.bs)
    assert bool((case.A > 0).any()) and bool((case.A < 0).any())


def test_quadrants(case):
    clip, r, A = case.coef["clip"], case.r, case.A
    out = (r - 1.0).abs() > clip
    if case.name in ("clipped", "clipped_ent0"):  # min() picks the clamped term on every sample
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
    if case.name in ("clipped", "clipped_ent0", "mirror", "clip0"):
        assert bool(out.all()) and case.st64[3] == 1.0


def test_special_inputs_are_what_the_names_say(case):
    n = case.ro.env.num_envs
    obs = case.ro.obs.reshape(n, 7)[case.idx]
    act = case.ro.actions.reshape(n)[case.idx]
    pi = max(case.ref64[D.NAMES.index(name)].abs().max().item() for name in P.PI_NAMES)
    if case.name == "saturated":
        pre = obs.double() @ case.pol.pi_net[0].weight.double().T + case.pol.pi_net[0].bias.double()
        assert (pre.abs() > 9.0).double().mean().item() > 0.5  # 1 - tanh^2 < 2^-24: exactly 0 in fp32
        assert pre.abs().max().item() > 45.0  # exp(2 x) overflows fp32
    if case.name == "offset_adv":
        a = case.ro.advantages.reshape(-1)[case.idx]
        assert abs(a.mean().item() - E.OFFSET_ADV) < 0.5 and 0.3 < a.std().item() < 0.7
        assert a.mean().item() > 7.0 * a.std().item()
    if case.name == "peaked":
        p = torch.from_numpy(D.forward64(case.pol, obs)[2]).exp()
        share = (p.max(1).values > E.PEAK_P).double().mean().item()
        print("peaked bs=%d: largest probability > %.2f on %.3f of the rows, entropy %.4f"
              % (case.bs, E.PEAK_P, share, case.st64[2]))
        assert share >= 0.5 and case.st64[2] < 0.15
    if case.name in ("all_first", "all_last"):
        one = 0 if case.name == "all_first" else case.k - 1
        assert bool((act == float(one)).all()) and case.k == 4
        # the heads not chosen get -dlp p_k and the entropy's term: each row far above the tensor's bar
        W = case.ref64[D.NAMES.index("W_action")]
        bar = 1e-4 * W.abs().max().item() + 1e-7
        for row in range(case.k):
            assert W[row].abs().max().item() >= 100.0 * bar, (row, W[row].abs().max().item(), bar)
    elif case.bs >= 1000:
        assert len(set(act.tolist())) == case.k  # every head is somebody's action
    if case.name == "clipped_ent0":  # float64 itself: nothing reaches the pi side
        assert pi == 0.0
    if case.name == "mirror":  # a gradient to agree on
        assert pi > 1e-3
    if case.name in ("clipped", "const_adv"):  # the entropy's gradient alone, 1000 x the bar's absolute part
        assert 1e-4 < pi < 1e-2
    if case.name == "vf0":
        assert all(torch.count_nonzero(case.ref64[D.NAMES.index(name)]).item() == 0 for name in P.VF_NAMES)


def test_fp32_reference_stays_within_half_of_every_bar(case):
    _print_shares("%s bs=%d k=%d" % (case.name, case.bs, case.k), case.share, case.dclip)
    for name, share in case.share.items():
        assert share <= E.ADMIT, (case.name, case.bs, case.k, name, share)
    assert case.dclip == 0.0  # clip_fraction is compared exactly: the fp32 reference counts the same samples


@pytest.mark.parametrize("k", [4, 3, 2])
def test_sweep_pool_keeps_the_ratio_margin_on_every_row(k):
    """Every sweep row draws from these pools: no ratio of any row is near a branch point."""
    pol, ro = E.sweep_pool(k)
    assert ro.env.num_envs == E.N_ROWS == 70001
    r = D.ratios64(pol, ro, torch.arange(E.N_ROWS))
    for edge in (0.8, 1.0, 1.2):
        assert (r - edge).abs().min().item() >= RATIO_MARGIN, (k, edge)
    assert float(ro.log_probs.abs().max()) < 16.0
    act = ro.actions.reshape(-1)
    assert torch.equal(act, act.long().float()) and sorted(set(act.tolist())) == [float(j) for j in range(k)]
    for t in (ro.obs, ro.log_probs, ro.advantages, ro.returns):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())


@pytest.mark.parametrize("bs,k", E.SWEEP)
def test_sweep_rows_are_whole_and_admitted(bs, k):
    """The rows of one sweep case, the 97 further ones of the poison test among them, and the fp32 reference
    within half of every bar at that size (70 001 and 40 001 rows included)."""
    pol, ro = E.sweep_pool(k)
    long_idx = E.minibatch(E.N_ROWS, bs, extra=97 if bs + 97 <= E.N_ROWS else 0)
    idx = long_idx[:bs]
    assert torch.equal(idx, E.minibatch(E.N_ROWS, bs)) and idx.dtype == torch.int64
    assert len(set(long_idx.tolist())) == long_idx.numel() and 0 <= int(idx.min()) and int(idx.max()) < E.N_ROWS
    share, dclip, _, st64 = E.admission(pol, ro, idx)
    _print_shares("sweep bs=%d k=%d" % (bs, k), share, dclip)
    for name, s in share.items():
        assert s <= E.ADMIT, (bs, k, name, s)
    assert dclip <= 1.0  # the sweep's bar is 2 samples
    if bs >= 127:
        assert 0.2 < st64[3] < 0.6  # samples on both sides of the clip


OPTS_SHAPES = ((4, 4097), (4, 16385), (2, 16385))
OPTS_POOL = 20000


@pytest.mark.parametrize("k,bs", OPTS_SHAPES)
@pytest.mark.parametrize("kind", Q.VCLIP_KINDS)
def test_value_clip_inputs_keep_the_margin_at_scale(kind, k, bs):
    """tests/test_discrete_opts_host.py's conditions on discrete_opts_ref.vclip_case at these sizes."""
    c = Q.vclip_case(kind, k, bs, n=OPTS_POOL)
    assert c.ro.env.num_envs == OPTS_POOL and c.idx.numel() == bs == len(set(c.idx.tolist()))
    dist, outside = Q.vclip_distance(c)
    assert dist.numel() == bs and dist.min().item() >= P.BUILD_MARGIN, (kind, dist.min().item())
    want = {"inside": (0.0, 0.0), "outside": (1.0, 1.0), "mixed": (0.4, 0.6), "half": (0.45, 0.55)}[kind]
    assert want[0] <= outside <= want[1], (kind, outside)
    gap = (Q.values(c.pol, c.ro, c.idx, torch.float32) - Q.values(c.pol, c.ro, c.idx, torch.float64)).abs().max().item()
    assert P.MARGIN >= 25 * gap, gap
    r = D.ratios64(c.pol, c.ro, c.idx)
    margin = min((r - edge).abs().min().item() for edge in (0.8, 1.0, 1.2))
    print("%s k=%d bs=%d: min distance %.2e, outside %.3f, fp32-fp64 V gap %.2e, ratio margin %.6e"
          % (kind, k, bs, dist.min().item(), outside, gap, margin))
    assert margin >= RATIO_MARGIN and float(c.ro.log_probs.reshape(-1)[c.idx].abs().max()) < 16.0


@pytest.mark.parametrize("k,bs", OPTS_SHAPES)
@pytest.mark.parametrize("vclip", [False, True])
def test_raw_advantage_inputs_at_scale(k, bs, vclip):
    c = Q.raw_case(k, bs, vclip, n=OPTS_POOL)
    adv = c.ro.advantages.view(-1)[c.idx]
    assert 49.0 < adv.mean().item() < 51.0 and 0.3 < adv.std().item() < 0.7 and adv.min().item() > 40.0
    r = D.ratios64(c.pol, c.ro, c.idx)
    assert min((r - edge).abs().min().item() for edge in (0.8, 1.0, 1.2)) >= RATIO_MARGIN
    if vclip:
        d = (Q.values(c.pol, c.ro, c.idx, torch.float64) - c.ro.values.reshape(-1)[c.idx].double()).abs()
        assert ((d - 0.2).abs() > 0.09).all() and 0.4 < (d > 0.2).double().mean().item() < 0.6
