"""The PPO learner (rr_ppo_grad, rr_ppo_update, rr_clip_adam: rl_rocket_amd/csrc/rocket_ppo.inc) at
the sizes and inputs where its kernels change path, against PyTorch autograd in float64 on the same
fp32 inputs (tests/ppo_ref.py reference) or a float64 restatement of clip_grad_norm_ + Adam
(ppo_ref.clip_adam_ref). The fused path is never its own reference.

1. Batch sizes of rr_ppo_grad: one tile and idle waves, the 32-sample tile boundary, 1 -> 2
   workgroups, the finish kernel's 16-way / 4-way / tail loops alone and mixed (nwg 32, 33, 127,
   128), waves of one launch with different tile counts (40 000: two and three full tiles; 40 001:
   one wave's third tile holds a single sample), a ragged last tile behind full ones, a fifth
   tile. Bars of test_gpu_ppo.test_ppo_grad_matches_autograd: per tensor max |fused - fp64| <=
   1e-4 max |fp64| + 1e-7, stats 1e-5 relative + 1e-6, clip_fraction within 2 samples. A poison
   test: rows outside the minibatch are NaN and the result is bitwise that of clean rows.
2. Loss branches (ppo_ref.edge_case; the input conditions are checked on the CPU by
   tests/test_ppo_edge_inputs.py): every sample clipped, its mirror, clip_range 0 / 0.05 / 0.4,
   constant and offset advantages, vf_coef and ent_coef off their defaults, saturated towers,
   log_std -2 and +1. With the margins held, clip_fraction is the reference's sample count exactly.
3. rr_ppo_update where the chain changes its number of workgroups (a short last minibatch):
   chained against each call packing for itself bitwise, both against PPOGrad + ClipAdam, the
   clipped gradients against float64, and ppo_update(fused=True) against the autograd ppo_update.
4. rr_clip_adam on lists of 1 .. 16 tensors whose 1024-element blocks straddle tensors, the clip
   active, inactive and off."""
import copy

import pytest

import ppo_ref as P

pytestmark = pytest.mark.gpu

N_ROWS = 70001
_cache = {}


def _sweep_inputs(ns, na):
    """One policy and 70 001-row rollout per (ns, na), built on the CPU and moved once; read-only."""
    if (ns, na) not in _cache:
        pol, ro, _ = P.setup_cpu(ns, na, N_ROWS, seed=100 + ns)
        _cache[ns, na] = P.to_device(pol, ro)
    return _cache[ns, na]


def _minibatch(n, bs, extra=0):
    import torch

    g = torch.Generator().manual_seed(bs)
    return torch.randperm(n, generator=g)[:bs + extra].contiguous().cuda()


def _check_against_fp64(label, pol, ro, idx, stats, coef, exact_clip=False, bitwise_zero=()):
    """The bars of test_ppo_grad_matches_autograd on pol's .grad and stats; returns the fp64
    gradients. exact_clip: clip_fraction is the reference's count of samples exactly."""
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    bs = idx.numel()
    fused = [t.grad.double() for t in _policy_tensors(pol)]
    ref64, st64 = P.reference(pol, ro, idx, torch.float64, **coef)
    ref32, _ = P.reference(pol, ro, idx, torch.float32, **coef)
    for name, a, r, t in zip(P.NAMES, fused, ref64, ref32):
        scale = r.abs().max().item()
        err, err32 = (a - r).abs().max().item(), (t - r).abs().max().item()
        print("%s %-9s max|ref| %.3e  fused err %.2e  torch-fp32 err %.2e" % (label, name, scale, err, err32))
        assert bool(torch.isfinite(a).all()), name
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale, err32)
        if name in bitwise_zero:
            assert torch.count_nonzero(a).item() == 0, name
    assert all(v == v and abs(v) != float("inf") for v in stats), stats
    for k, (a, r) in enumerate(zip(stats, st64)):
        tol = 2.0 / bs if k == 3 else 1e-5 * abs(r) + 1e-6
        assert abs(a - r) <= tol, (k, a, r)
    if exact_clip:
        assert round(stats[3] * bs) == round(st64[3] * bs) and abs(stats[3] - st64[3]) <= 1e-6, (stats[3], st64[3])
    return ref64, st64


SWEEP = [(bs, 14, 3) for bs in (3, 31, 32, 33, 127, 128, 129, 4096, 4097, 16256, 16384, 16385, 40000, 40001, 65537,
                                70001)]
SWEEP += [(bs, 7, 2) for bs in (3, 31, 32, 33, 40000)]


@pytest.mark.parametrize("bs,ns,na", SWEEP)
def test_ppo_grad_batch_size_sweep(bs, ns, na):
    from rl_rocket_amd.rollout import PPOGrad

    pol0, ro = _sweep_inputs(ns, na)
    pol = copy.deepcopy(pol0)
    idx = _minibatch(N_ROWS, bs)
    stats = PPOGrad(pol, ro, bs)(idx).tolist()
    _check_against_fp64("bs=%d (%d,%d)" % (bs, ns, na), pol, ro, idx, stats, {})


@pytest.mark.parametrize("bs", [33, 16385])
def test_ppo_grad_reads_nothing_outside_the_minibatch(bs):
    """idx is the head of a longer tensor of valid rows; every rollout row that idx[:bs] does not
    name (the longer tensor's tail included) is NaN in obs, actions, log-probs, advantages and
    returns. Gradients and stats are bitwise those of clean rows: the padding lanes of a ragged
    tile, the gathers issued past a wave's last tile and the advantage sums reach no row outside."""
    import torch
    from rl_rocket_amd.rollout import PPOGrad, _policy_tensors

    pol0, ro = _sweep_inputs(14, 3)
    long_idx = _minibatch(N_ROWS, bs, extra=97)
    idx = long_idx[:bs]
    assert idx.data_ptr() == long_idx.data_ptr() and idx.is_contiguous()
    outside = torch.ones(N_ROWS, dtype=torch.bool, device="cuda:0")
    outside[idx] = False
    assert bool(outside[long_idx[bs:]].all())
    bad = [x.reshape(N_ROWS, -1).clone() for x in (ro.obs, ro.actions, ro.log_probs, ro.advantages, ro.returns)]
    for x in bad:
        x[outside] = float("nan")
    ro_bad = P.make_rollout(N_ROWS, 14, 3, *[x.reshape(-1) for x in bad])
    out = []
    for r in (ro, ro_bad):
        pol = copy.deepcopy(pol0)
        stats = PPOGrad(pol, r, bs)(idx).clone()
        torch.cuda.synchronize()
        out.append(([t.grad.clone() for t in _policy_tensors(pol)], stats))
    (ga, sa), (gb, sb) = out
    assert all(bool(torch.isfinite(g).all()) for g in ga) and bool(torch.isfinite(sa).all())
    for name, a, b in zip(P.NAMES, ga, gb):
        assert torch.equal(a, b), name
    assert torch.equal(sa, sb)


EDGES = [(name, bs) for name in P.EDGE_CASES for bs in P.EDGE_BATCHES]


@pytest.mark.parametrize("name,bs", EDGES)
def test_ppo_grad_loss_branches(name, bs):
    """Every case at the bars of the sweep, with clip_fraction the reference's sample count exactly
    (the margins of ppo_ref.edge_case put kernel and reference in the same branch on every sample)
    and finite results. On top of that:
      clipped    the pi tower's four tensors, W_action and b_action are exactly 0, the log_std
                 gradient is exactly -ent_coef, clip_fraction is 1, the vf tensors match float64;
      mirror     clip_fraction is 1 and the gradients are those of the unclipped surrogate, which
                 is what `reference` gives: min() keeps the unclipped term;
      clip0      clip_range 0 is accepted and clips every sample;
      const_adv  std 0: as `clipped` for the pi side, policy_loss exactly 0;
      vf0        the vf tower's four tensors, W_value and b_value are exactly 0."""
    import torch
    from rl_rocket_amd.rollout import PPOGrad, _policy_tensors

    c = P.edge_case(name, bs)
    pol, ro = P.to_device(c.pol, c.ro)
    idx = c.idx.cuda()
    coef = c.coef
    stats = PPOGrad(pol, ro, bs, coef["clip"], coef["ent_coef"], coef["vf_coef"])(idx).tolist()
    zero = ()
    if name in ("clipped", "const_adv"):
        zero = P.PI_NAMES
    if name == "vf0":
        zero = P.VF_NAMES
    ref64, st64 = _check_against_fp64("%s bs=%d" % (name, bs), pol, ro, idx, stats, coef, exact_clip=True,
                                      bitwise_zero=zero)
    g = dict(zip(P.NAMES, [t.grad for t in _policy_tensors(pol)]))
    if name in ("clipped", "const_adv"):  # nothing but the entropy term reaches log_std
        want = torch.full((3,), -coef["ent_coef"], dtype=torch.float32, device="cuda:0")
        assert torch.equal(g["log_std"], want)
    if name in ("clipped", "mirror", "clip0"):
        assert st64[3] == 1.0 and stats[3] == 1.0
    if name == "const_adv":
        assert stats[0] == 0.0 and st64[0] == 0.0
    if name == "mirror":  # min() keeps the unclipped term: the gradient is the plain surrogate's
        assert max(r.abs().max().item() for r in ref64[:4]) > 1e-3


CHAINS = [((4096, 4096, 1000), 14, 3), ((16385, 16385, 33), 14, 3), ((3999, 3999, 2), 14, 3), ((3999, 3999, 2), 7, 2)]


@pytest.mark.parametrize("sizes,ns,na", CHAINS)
def test_ppo_update_chain_into_a_short_minibatch(sizes, ns, na):
    """Two epochs of three minibatches whose last is short enough to run fewer workgroups per
    tower (nwg 32, 32, 8 / 128, 128, 1 / 32, 32, 1) on three copies: chained (each call's
    optimizer launch packs the towers and sums the advantages for the next), unchained (each call
    packs for itself), PPOGrad + ClipAdam. Chained == unchained bitwise in parameters, .grad,
    exp_avg, exp_avg_sq, step; both within 1e-6 max(1, |z|) of the third. Through the first epoch
    the chained path's clipped .grad is also held to float64 autograd from the parameters the call
    started from, scaled by float64 clip_grad_norm_'s coefficient, at the 1e-4 bar."""
    import torch
    from rl_rocket_amd.rollout import ClipAdam, PPOGrad, PPOUpdate, _policy_tensors

    n = sum(sizes) + 11
    pol0, ro0, _ = P.setup_cpu(ns, na, n, seed=sum(sizes) + ns)
    pol, ro = P.to_device(pol0, ro0)
    bs = sizes[0]
    pols = [copy.deepcopy(pol) for _ in range(3)]
    opts = [torch.optim.Adam(p.parameters(), lr=1e-3, eps=1.0, capturable=True) for p in pols]
    upd = [PPOUpdate(pols[k], opts[k], ro, bs) for k in range(2)]
    grad, adam = PPOGrad(pols[2], ro, bs), ClipAdam(opts[2], list(pols[2].parameters()), 0.5)
    g = torch.Generator().manual_seed(5)
    for epoch in range(2):
        perm = torch.randperm(n, generator=g)[:sum(sizes)].cuda()
        mbs = list(torch.split(perm, list(sizes)))
        for k, idx in enumerate(mbs):
            start = copy.deepcopy(pols[0]) if epoch == 0 else None
            nxt = mbs[k + 1] if k + 1 < len(mbs) else None
            upd[0](idx, nxt, chained=k > 0)
            upd[1](idx)
            grad(idx)
            adam()
            if start is None:
                continue
            ref64, _ = P.reference(start, ro, idx, torch.float64)
            coef = P.clip_coef64(ref64, 0.5)
            for name, t, r in zip(P.NAMES, _policy_tensors(pols[0]), ref64):
                r = r * coef
                scale, err = r.abs().max().item(), (t.grad.double() - r).abs().max().item()
                print("minibatch %d (%d rows) %-9s max|ref| %.3e clipped-grad err %.2e"
                      % (k, len(idx), name, scale, err))
                assert err <= 1e-4 * scale + 1e-7, (k, name, err, scale)
    torch.cuda.synchronize()
    for name, x, y, z in zip(P.NAMES, *[_policy_tensors(p) for p in pols]):
        assert torch.equal(x, y), name
        assert torch.equal(x.grad, y.grad), name
        assert torch.equal(opts[0].state[x]["exp_avg"], opts[1].state[y]["exp_avg"]), name
        assert torch.equal(opts[0].state[x]["exp_avg_sq"], opts[1].state[y]["exp_avg_sq"]), name
        assert float(opts[0].state[x]["step"]) == float(opts[1].state[y]["step"]) == 6
        assert float(opts[2].state[z]["step"]) == 6
        assert (x - z).abs().max().item() <= 1e-6 * max(1.0, z.abs().max().item()), name


def test_fused_ppo_update_with_a_two_row_remainder_tracks_autograd():
    """ppo_update(fused=True) over 8000 rows at batch_size 3999 (minibatches of 3999, 3999, 2: the
    last two chained) against the PyTorch-autograd ppo_update from the same state and generator,
    two epochs, Adam(eps=1.0): the bars of test_fused_update_graphed_equals_eager_and_tracks_autograd,
    parameters within 1e-6 and the returned statistics within 1e-4."""
    import torch
    from rl_rocket_amd.rollout import ppo_update

    pol0, ro0, _ = P.setup_cpu(14, 3, 8000, seed=77)
    pol, ro = P.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [torch.optim.Adam(p.parameters(), lr=1e-3, eps=1.0, capturable=True) for p in pols]
    gen = lambda: torch.Generator("cuda:0").manual_seed(9)  # noqa: E731
    sa = ppo_update(pols[0], opts[0], ro, n_epochs=2, batch_size=3999, generator=gen())
    sb = ppo_update(pols[1], opts[1], ro, n_epochs=2, batch_size=3999, generator=gen(), fused=True)
    torch.cuda.synchronize()
    moved = max((x - y).abs().max().item() for x, y in zip(pol.parameters(), pols[0].parameters()))
    worst = max((x - y).abs().max().item() for x, y in zip(pols[0].parameters(), pols[1].parameters()))
    print("moved %.3e, fused vs autograd %.3e" % (moved, worst), sa, sb)
    assert moved > 1e-5
    assert worst <= 1e-6, worst
    assert set(sa) == set(sb) and len(sa) == 3
    for k in sa:
        assert abs(sa[k] - sb[k]) <= 1e-4 * max(1.0, abs(sa[k])), (k, sa[k], sb[k])


POLICY_7_2 = [(64, 7), (64,), (64, 64), (64,), (64, 7), (64,), (64, 64), (64,), (2, 64), (2,), (1, 64), (1,), (2,)]
ADAM_LISTS = {
    "one": [(1,)],
    "sixteen": [(k,) for k in (1, 63, 64, 65, 1023, 1024, 1025, 1, 2, 3, 5000, 7, 1, 64, 4096, 31)],
    "policy_7_2": POLICY_7_2,
}
# max_grad_norm, gradient scale. Clip active: 10 x unit-normal gradients (the test asserts a float64
# coefficient < 0.9 at every step, the one-element list included). Inactive: 1e-4 x unit-normal.
# Off: 1e-3, so that exp_avg's fp32 rounding, 2^-24 |g| per operation, stays under the 1e-9
# absolute bar where m passes near 0.
ADAM_CLIPS = {"active": (0.5, 10.0), "inactive": (0.5, 1e-4), "off": (0.0, 1e-3)}


@pytest.mark.parametrize("clip", list(ADAM_CLIPS))
@pytest.mark.parametrize("shapes", list(ADAM_LISTS))
def test_clip_adam_on_general_tensor_lists(shapes, clip):
    """ClipAdam on plain nn.Parameter lists for 4 steps (gradients redrawn each step, the learning
    rate changed after the second) against ppo_ref.clip_adam_ref, the float64 restatement of
    clip_grad_norm_ and torch's Adam formulas carried in float64 from the same start. Bars of
    test_clip_adam_matches_torch: parameters 1e-6 max(1, |p|), gradients and exp_avg rtol 1e-5 atol
    1e-9, exp_avg_sq rtol 1e-5 atol 1e-12, step exact. With the clip off the gradients come back
    bitwise as they went in."""
    import torch
    from rl_rocket_amd.rollout import ClipAdam

    max_norm, gscale = ADAM_CLIPS[clip]
    g = torch.Generator().manual_seed(len(ADAM_LISTS[shapes]))
    params = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in ADAM_LISTS[shapes]]
    opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5, capturable=True)
    adam = ClipAdam(opt, params, max_norm)
    p64 = [p.detach().double().clone() for p in params]
    st64 = dict(step=0, exp_avg=[torch.zeros_like(p) for p in p64], exp_avg_sq=[torch.zeros_like(p) for p in p64])
    lr = 3e-4
    for step in range(4):
        if step == 2:
            lr = 1e-4
            opt.param_groups[0]["lr"] = lr
        raw = [(gscale * torch.randn(p.shape, generator=g)).cuda() for p in params]
        for p, r in zip(params, raw):
            p.grad.copy_(r)
        if clip == "active":
            assert P.clip_coef64(raw, max_norm) < 0.9
        if clip == "inactive":
            assert P.clip_coef64(raw, max_norm) == 1.0
        adam()
        torch.cuda.synchronize()
        g64 = P.clip_adam_ref(p64, raw, st64, max_norm, lr, eps=1e-5)
        for k, (p, r) in enumerate(zip(params, raw)):
            st = opt.state[p]
            assert float(st["step"]) == step + 1, k
            if clip != "active":
                assert torch.equal(p.grad, r), k
            err = (p.detach().double() - p64[k]).abs().max().item()
            assert err <= 1e-6 * max(1.0, p64[k].abs().max().item()), (k, err)
            assert torch.allclose(p.grad.double(), g64[k], rtol=1e-5, atol=1e-9), k
            assert torch.allclose(st["exp_avg"].double(), st64["exp_avg"][k], rtol=1e-5, atol=1e-9), k
            assert torch.allclose(st["exp_avg_sq"].double(), st64["exp_avg_sq"][k], rtol=1e-5, atol=1e-12), k
