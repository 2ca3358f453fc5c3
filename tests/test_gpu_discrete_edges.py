"""The Categorical PPO learner (rr_ppo_update_discrete: rl_rocket_amd/csrc/discrete/rocket_discrete.hip, the
<7, 4> pi tower with LOSS 2 of rocket_ppo.inc and discrete_finish_kernel) at the sizes and inputs where its
kernels change path, against discrete_ref.loss_reference: SB3's loss with torch.distributions.Categorical
through autograd in float64 on the same fp32 inputs. The fused path is never its own reference. The inputs
are built on the CPU (tests/discrete_edge_ref.py) and their conditions checked there by
tests/test_discrete_edge_inputs.py, which also admits a case only where the fp32 reference stays within half
of every bar below.

Bars, those of test_gpu_discrete._check_against_fp64 (test_gpu_ppo's): per tensor max |fused - fp64| <=
1e-4 max |fp64| + 1e-7, statistics 1e-5 |r| + 1e-6, clip_fraction within 2 samples (the sweep) or the
reference's sample count exactly (the edge cases, as test_gpu_ppo_edges.test_ppo_grad_loss_branches). Under
them the CPU's fp32 reference sits at, worst case of each group (share of the bar): sweep 0.05 of a tensor's
(b_value, 33 rows, K = 2) and 0.07 of a statistic's (policy_loss, 32 rows, K = 2), at 70 001 rows 0.02 (pi.b1)
and 0.01 (entropy), at 40 001 rows 0.01 (b_action) and 0.03 (policy_loss, K = 2); edge cases 0.08 of a
tensor's (b_value, mirror, 33 rows, K = 2) and 0.25 of a statistic's (policy_loss, offset_adv, 33 rows: the
offset is 5 because 50 is not admitted), without offset_adv 0.07 (policy_loss, saturated, 33 rows); the worst
of any bar for peaked is 0.05 (pi.b2), for all_last 0.02 (approx_kl); the fp32 reference's clip_fraction never
differs from the float64 one's.

1. Batch sizes (one unchained call, test_gpu_discrete._one_call: a copy of the policy, the workspace NaN
   first): one tile and idle waves, the 32-sample tile boundary, 1 -> 2 workgroups, the finish body's 16-way /
   4-way / tail loops over nwg alone and mixed (nwg 32, 33, 127, 128) summing a Categorical tower's partials,
   the fourth per-sample sum (the entropy) among them, and its `spare` choice of the sink per element; a
   wave's second, third and fifth tile with the head derivative and the entropy's gradient accumulated across
   them (16 385, 40 000 / 40 001: a ragged last tile of one sample, 65 537, 70 001). K = 4 at every size, K = 3
   and K = 2 (whose PPO gradient no other test holds to float64) at the sizes where a path changes.
2. Rows outside the minibatch are NaN at 16 385 rows: bitwise the clean call, and finite
   (test_gpu_discrete's test at 333 rows).
3. Heads past K at 16 385 and 4 097 rows: the sink's rows >= K are zeros and its rows < K keep the NaN fill
   (the same test's assertions), and guard floats directly behind W_action.grad and b_action.grad keep their
   bit pattern (test_gpu_discrete_opts's GUARD).
4. Loss branches (discrete_edge_ref.edge_case): ppo_ref.edge_case's names for a softmax head, where the
   entropy's gradient enters per sample, so "every sample clipped" leaves a pi-side gradient unless ent_coef is
   0; a peaked policy; minibatches whose actions are all index 0 or all index K - 1.
5. Chains of three minibatches, the last short (nwg 128, 128, 1 at K = 4; 32, 32, 1 at K = 2): the clipped
   gradients against float64 autograd times float64 clip_grad_norm_'s coefficient at the 1e-4 bar,
   parameters and Adam state at test_whole_call_matches_float64_adam_over_six_calls's bars, the chained epoch
   bitwise the one in which every call packs for itself.
6. rr_ppo_update_discrete_opts at 4 097 and 16 385 rows of a 20 000-row pool: the value clip's four kinds and
   raw advantages, bars and guards of test_gpu_discrete_opts.test_value_clip_matches_float64 /
   test_raw_advantages_match_float64 (their _one_call and _check)."""
import copy

import pytest

import discrete_edge_ref as E
import discrete_opts_ref as Q
import discrete_ref as D
import ppo_ref as P
import test_gpu_discrete as T
import test_gpu_discrete_opts as O

pytestmark = pytest.mark.gpu

DEV = T.DEV


def _check(label, pol0, ro, idx, grads, stats, coef, exact_clip=False, bitwise_zero=()):
    """test_gpu_discrete._check_against_fp64's bars on the 12 gradients and the 5 statistics, every figure
    printed first; returns the float64 (gradients by name, statistics). exact_clip: clip_fraction is the
    reference's count of samples exactly."""
    import torch

    bs = idx.numel()
    ref64, st64 = D.loss_reference(pol0, ro, idx, **coef)
    fused = [g.double().cpu() for g in grads]
    st = stats.tolist()
    for name, a, r in zip(D.NAMES, fused, ref64):
        print("%s %-9s max|ref| %.3e  fused err %.2e" % (label, name, r.abs().max().item(), (a - r).abs().max().item()))
    for name, a, r in zip(E.STATS, st, st64):
        print("%s %-13s fused %.9e fp64 %.9e" % (label, name, a, r))
    for name, a, r in zip(D.NAMES, fused, ref64):
        scale, err = r.abs().max().item(), (a - r).abs().max().item()
        assert a.shape == r.shape and bool(torch.isfinite(a).all()), (label, name)
        assert err <= 1e-4 * scale + 1e-7, (label, name, err, scale)
        if name in bitwise_zero:
            assert torch.count_nonzero(a).item() == 0, (label, name)
    assert all(v == v and abs(v) != float("inf") for v in st), st
    for name, a, r in zip(E.STATS, st, st64):
        if name == "clip_fraction":
            assert abs(a - r) <= 2.0 / bs + 1e-7, (label, name, a, r)
        else:
            assert abs(a - r) <= 1e-5 * abs(r) + 1e-6, (label, name, a, r)
    if exact_clip:
        assert round(st[3] * bs) == round(st64[3] * bs) and abs(st[3] - st64[3]) <= 1e-6, (label, st[3], st64[3])
    return dict(zip(D.NAMES, ref64)), st64


# ---- 1. batch sizes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,k", E.SWEEP)
def test_batch_size_sweep(bs, k):
    pol0, ro = E.sweep_inputs(k)
    idx = E.minibatch(E.N_ROWS, bs).to(DEV)
    _, grads, stats, _ = T._one_call(pol0, ro, idx)
    _check("bs=%d k=%d" % (bs, k), pol0, ro, idx, grads, stats, {})


# ---- 2. rows outside the minibatch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 2])
def test_rows_outside_the_minibatch_are_not_read_at_16385_rows(k):
    """idx is the head of a longer tensor of valid rows; every rollout row that idx does not name (the longer
    tensor's tail included) is NaN in obs, actions, log-probs, advantages and returns. Gradients, the parameters
    after the step and the statistics are bitwise those of the clean call, and finite: the padding lanes of the
    ragged 513th tile, the gathers issued past a wave's last tile and the advantage sums reach no row outside."""
    import torch

    bs, n = 16385, E.N_ROWS
    pol0, ro = E.sweep_inputs(k)
    long_idx = E.minibatch(n, bs, extra=97).to(DEV)
    idx = long_idx[:bs]
    assert idx.data_ptr() == long_idx.data_ptr() and idx.is_contiguous()
    outside = torch.ones(n, dtype=torch.bool, device=DEV)
    outside[idx] = False
    assert bool(outside[long_idx[bs:]].all()) and int(outside.sum()) == n - bs
    dirty = copy.copy(ro)
    for name in ("obs", "actions", "log_probs", "advantages", "returns"):
        t = getattr(ro, name).clone()
        t.reshape(n, -1)[outside] = float("nan")
        setattr(dirty, name, t)
    pa, ga, sa, _ = T._one_call(pol0, ro, idx, max_grad_norm=0.5)
    pb, gb, sb, _ = T._one_call(pol0, dirty, idx, max_grad_norm=0.5)
    moved = max((x - y).abs().max().item() for x, y in zip(pol0.parameters(), pa.parameters()))
    assert moved > 1e-4  # the step was taken
    for a, b in zip(ga + list(pa.parameters()) + [sa], gb + list(pb.parameters()) + [sb]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


# ---- 3. heads past K -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 2])
@pytest.mark.parametrize("bs", [16385, 4097])
def test_heads_past_k_get_nothing_at_scale(bs, k):
    """nwg 128 and 33: every loop of the finish body feeds the elements that `spare` sends to the sink. The
    [K][64] and [K] head gradients are the fronts of sentinel-filled buffers."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdateDiscrete, _policy_tensors

    pol0, ro = E.sweep_inputs(k)
    idx = E.minibatch(E.N_ROWS, bs).to(DEV)
    pol = copy.deepcopy(pol0)
    guards = O._guarded(pol)
    step = PPOUpdateDiscrete(pol, T._adam(pol), ro, bs, max_grad_norm=None)
    step.ws.fill_(float("nan"))
    stats = step(idx).clone()
    torch.cuda.synchronize()
    pattern = torch.full((O.GUARD,), O.SENTINEL, dtype=torch.float32, device=DEV).view(torch.int32)
    for buf, numel in guards:
        assert buf.numel() == numel + O.GUARD
        assert torch.equal(buf[numel:].view(torch.int32), pattern), "written past a head gradient"
        assert not bool((buf[:numel] == O.SENTINEL).any()), "a head gradient element was not written"
    grads = [t.grad.clone() for t in _policy_tensors(pol)]
    assert grads[8].shape == (k, 64) and grads[9].shape == (k,)
    for p, (buf, _) in zip((pol.action_net.weight, pol.action_net.bias), guards):
        assert p.grad.data_ptr() == buf.data_ptr()  # the call wrote into the guarded buffers
    _check("heads past K bs=%d k=%d" % (bs, k), pol0, ro, idx, grads, stats, {})
    # the sink, the workspace's last 264 floats: [4][64] weights, [4] biases, [4] for the body's log_std slot
    sink = step.ws[step._nbytes // 4 - 264:step._nbytes // 4]
    w, b, ls = sink[:256].reshape(4, 64), sink[256:260], sink[260:264]
    assert bool((w[k:] == 0).all()) and bool((b[k:] == 0).all()) and bool((ls == 0).all())
    assert bool(torch.isnan(w[:k]).all()) and bool(torch.isnan(b[:k]).all())


# ---- 4. loss branches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bs,k", E.EDGES)
def test_loss_branches(name, bs, k):
    """Every case at the bars of the sweep, with clip_fraction the reference's sample count exactly (the margins
    of discrete_edge_ref.edge_case put kernel and reference in the same branch on every sample). On top of that:
      clipped       clip_fraction is 1; the pi-side gradient is the entropy's alone and matches float64;
      clipped_ent0  the pi tower's four tensors, W_action and b_action are exactly 0, clip_fraction is 1;
      mirror        clip_fraction is 1 and the gradients are those of the unclipped surrogate, which is what
                    the reference gives (min() keeps the unclipped term), above 1e-3 on the pi side;
      clip0         clip_range 0 is accepted and clips every sample;
      const_adv     std 0: policy_loss exactly 0, the pi-side gradient is the entropy's alone;
      vf0           the vf tower's four tensors, W_value and b_value are exactly 0;
      all_first, all_last  the rows of W_action of the heads not chosen are non-zero and match float64."""
    import torch

    c = E.edge_case(name, bs, k)
    pol0, ro = D.to_device(c.pol, c.ro)
    idx = c.idx.to(DEV)
    coef = c.coef
    _, grads, stats, _ = T._one_call(pol0, ro, idx, clip_range=coef["clip"], ent_coef=coef["ent_coef"],
                                     vf_coef=coef["vf_coef"])
    zero = ()
    if name == "clipped_ent0":
        zero = P.PI_NAMES
    if name == "vf0":
        zero = P.VF_NAMES
    ref64, st64 = _check("%s bs=%d k=%d" % (name, bs, k), pol0, ro, idx, grads, stats, coef, exact_clip=True,
                         bitwise_zero=zero)
    st = stats.tolist()
    pi64 = max(ref64[n].abs().max().item() for n in P.PI_NAMES)
    if name in ("clipped", "mirror", "clipped_ent0", "clip0"):
        assert st64[3] == 1.0 and st[3] == 1.0
    if name == "const_adv":
        assert st[0] == 0.0 and st64[0] == 0.0
    if name in ("clipped", "const_adv"):  # the entropy's gradient: 1000 x the absolute part of the bar it met
        assert pi64 > 1e-4 and torch.count_nonzero(grads[8]).item() > 0
    if name == "mirror":
        assert pi64 > 1e-3
    if name in ("all_first", "all_last"):
        chosen = 0 if name == "all_first" else k - 1
        W, W64 = grads[8].double().cpu(), ref64["W_action"]
        bar = 1e-4 * W64.abs().max().item() + 1e-7
        for row in range(k):
            if row != chosen:
                assert torch.count_nonzero(W[row]).item() > 0 and W64[row].abs().max().item() >= 100.0 * bar, row
                assert (W[row] - W64[row]).abs().max().item() <= bar, row


# ---- 5. chains -----------------------------------------------------------------------------------------------------
CHAINS = [((16385, 16385, 33), 4), ((3999, 3999, 2), 2)]


@pytest.mark.parametrize("sizes,k", CHAINS)
def test_chain_into_a_short_minibatch_is_held_to_float64(sizes, k):
    """One epoch of three minibatches with max_grad_norm 0.5 on two copies: the first call unchained and the
    next two chained, against every call packing for itself. After each call the chained copy's .grad is float64
    autograd from the parameters the call started from times ppo_ref.clip_coef64's coefficient, at the 1e-4 bar;
    parameters, exp_avg and exp_avg_sq are float64 Adam (ppo_ref.clip_adam_ref, no second clip) applied from
    the fp32 state the call started from to the gradients it left, at the bars of
    test_gpu_discrete.test_whole_call_matches_float64_adam_over_six_calls. Chained == packed bitwise in
    parameters, .grad, exp_avg, exp_avg_sq, step and the statistics of every call."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdateDiscrete, _policy_tensors

    n = sum(sizes) + 11
    pol0, ro0, _ = D.learner_inputs(k, n=n, seed=sum(sizes) + k)
    pol, ro = D.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [T._adam(p) for p in pols]
    upd = [PPOUpdateDiscrete(pols[j], opts[j], ro, sizes[0], max_grad_norm=0.5) for j in range(2)]
    tensors = _policy_tensors(pols[0])
    lr = opts[0].param_groups[0]["lr"]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))[:sum(sizes)].to(DEV)
    mbs = list(torch.split(perm, list(sizes)))
    coefs = []
    for j, idx in enumerate(mbs):
        torch.cuda.synchronize()
        start = copy.deepcopy(pols[0])
        before = [t.detach().double().cpu() for t in tensors]
        state = dict(step=j, exp_avg=[opts[0].state[t]["exp_avg"].double().cpu() for t in tensors],
                     exp_avg_sq=[opts[0].state[t]["exp_avg_sq"].double().cpu() for t in tensors])
        sa = upd[0](idx, mbs[j + 1] if j + 1 < len(mbs) else None, chained=j > 0).clone()
        sb = upd[1](idx).clone()
        torch.cuda.synchronize()
        assert torch.equal(sa, sb) and bool(torch.isfinite(sa).all()), (j, sa, sb)
        ref64, _ = D.loss_reference(start, ro, idx)
        coef = P.clip_coef64(ref64, 0.5)
        coefs.append(coef)
        left = [t.grad.double().cpu() for t in tensors]
        for name, a, r in zip(D.NAMES, left, ref64):
            r = r * coef
            scale, err = r.abs().max().item(), (a - r).abs().max().item()
            print("minibatch %d (%d rows) coef %.4f %-9s max|ref| %.3e clipped-grad err %.2e"
                  % (j, len(idx), coef, name, scale, err))
            assert err <= 1e-4 * scale + 1e-7, (j, name, err, scale)
        P.clip_adam_ref(before, left, state, 0.0, lr)
        for name, t, p, m, v in zip(D.NAMES, tensors, before, state["exp_avg"], state["exp_avg_sq"]):
            st = opts[0].state[t]
            assert float(st["step"]) == j + 1, name
            assert (t.detach().double().cpu() - p).abs().max().item() <= 1e-6 * max(1.0, p.abs().max().item()), name
            assert torch.allclose(st["exp_avg"].double().cpu(), m, rtol=1e-5, atol=1e-9), name
            assert torch.allclose(st["exp_avg_sq"].double().cpu(), v, rtol=1e-5, atol=1e-12), name
    assert min(coefs) < 1.0  # the clip was active
    chained, packed = T._state(pols[0], opts[0]), T._state(pols[1], opts[1])
    assert len(chained) == len(packed) == 12 * 5
    for j, (a, b) in enumerate(zip(chained, packed)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (D.NAMES[j // 5], j % 5)
    assert float(chained[4]) == 3.0


# ---- 6. the options call -------------------------------------------------------------------------------------------
OPTS_SHAPES = ((4, 4097), (4, 16385), (2, 16385))
OPTS_POOL = 20000


@pytest.mark.parametrize("k,bs", OPTS_SHAPES)
@pytest.mark.parametrize("kind", Q.VCLIP_KINDS)
def test_value_clip_matches_float64_at_scale(kind, k, bs):
    c = Q.vclip_case(kind, k, bs, n=OPTS_POOL)
    ref64, st64 = Q.reference(c.pol, c.ro, c.idx, clip_range_vf=c.c, **c.coef)
    pol, ro = Q.to_device(c.pol, c.ro)
    _, stats = O._one_call(pol, ro, c.idx.to(DEV), c.coef, clip_range_vf=c.c)
    zero = Q.VF_NAMES if kind == "outside" else ()
    O._check("%s k=%d bs=%d" % (kind, k, bs), pol, stats, ref64, st64, bs, bitwise_zero=zero)
    assert pol.action_net.weight.grad.shape == (k, 64) and pol.action_net.bias.grad.shape == (k,)


@pytest.mark.parametrize("k,bs", OPTS_SHAPES)
@pytest.mark.parametrize("vclip", [False, True])
def test_raw_advantages_match_float64_at_scale(k, bs, vclip):
    c = Q.raw_case(k, bs, vclip, n=OPTS_POOL)
    ref64, st64 = Q.reference(c.pol, c.ro, c.idx, clip_range_vf=c.opts.get("clip_range_vf"), normalize_advantage=False,
                              **c.coef)
    pol, ro = Q.to_device(c.pol, c.ro)
    _, stats = O._one_call(pol, ro, c.idx.to(DEV), c.coef, **c.opts)
    O._check("raw_adv k=%d bs=%d vclip=%s" % (k, bs, vclip), pol, stats, ref64, st64, bs)
