"""rr_ppo_update_opts (rl_rocket_amd/csrc/ppo_opts/: SB3's clip_range_vf, normalize_advantage=False,
target_kl and the train() log means on the device) against float64 PyTorch restatements of SB3 1.6's
minibatch loss and PPO.train loop (tests/ppo_opts_ref.py); the fused path is never its own
reference. Inputs are built on the CPU (ppo_ref.setup_cpu / to_device); their conditions (clip
margins, KL thresholds) are checked there by tests/test_ppo_opts_host.py.

1. Gradients with the options on, one unchained call without a gradient clip, so that .grad is the
   loss's gradient at the parameters the call started from: the value clip with every sample
   inside, every sample outside (vf-tower gradients exactly 0), mixed, and c at the median; raw
   advantages on the
   50 + 0.5 randn case. Bars of test_gpu_ppo_edges: per tensor max |fused - fp64| <= 1e-4 max |fp64|
   + 1e-7, stats 1e-5 relative + 1e-6, clip_fraction the reference's sample count exactly.
2. Options off: bitwise rr_ppo_update on the chains of test_ppo_update_chain_into_a_short_minibatch,
   chained and unchained, in parameters, .grad, exp_avg, exp_avg_sq, step and stats.
3. The KL stop at its four places against ppo_opts_ref.train_ref, and GraphedPPOUpdate(target_kl)
   against the eager PPOUpdate loop.
4. The C call itself without a control block, and without stats.
5. ppo_update(fused=True) with the three options against a PPOUpdate loop and the float64 loop;
   GraphedPPOUpdate(fused=False) with the two it takes against the eager autograd ppo_update."""
import copy
import types

import pytest

import ppo_opts_ref as R
import ppo_ref as P

pytestmark = pytest.mark.gpu


def _adam(pol, lr=1e-3):
    import torch

    return torch.optim.Adam(pol.parameters(), lr=lr, eps=1.0, capturable=True)


def _check(label, pol, stats, ref64, st64, bs, bitwise_zero=()):
    """test_gpu_ppo_edges._check_against_fp64's bars with clip_fraction exact, against a given reference."""
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    for name, t, r in zip(P.NAMES, _policy_tensors(pol), ref64):
        a = t.grad.double().cpu()
        scale, err = r.abs().max().item(), (a - r).abs().max().item()
        print("%s %-9s max|ref| %.3e  fused err %.2e" % (label, name, scale, err))
        assert bool(torch.isfinite(a).all()), name
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale)
        if name in bitwise_zero:
            assert torch.count_nonzero(a).item() == 0, name
    assert all(v == v and abs(v) != float("inf") for v in stats), stats
    for k, (a, r) in enumerate(zip(stats, st64)):
        print("%s %-13s fused %.9e fp64 %.9e" % (label, R.STAT_NAMES[k], a, r))
        assert abs(a - r) <= 1e-5 * abs(r) + 1e-6, (k, a, r)
    assert round(stats[3] * bs) == round(st64[3] * bs), (stats[3], st64[3])


def _one_call(pol, ro, idx, coef, **opts):
    """One unchained PPOUpdate call with max_grad_norm None: .grad is left unscaled, the gradient at
    the parameters the call started from (the caller's reference is taken from the CPU original)."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdate

    upd = PPOUpdate(pol, _adam(pol), ro, idx.numel(), coef["clip"], coef["ent_coef"], coef["vf_coef"],
                    max_grad_norm=None, **opts)
    assert upd.opts is not None
    stats = upd(idx, epoch_start=True).tolist()
    torch.cuda.synchronize()
    return upd, stats


@pytest.mark.parametrize("ns,na,bs", R.VCLIP_SHAPES)
@pytest.mark.parametrize("kind", R.VCLIP_KINDS)
def test_value_clip_matches_float64(kind, ns, na, bs):
    c = R.vclip_case(kind, ns, na, bs)
    ref64, st64 = R.reference(c.pol, c.ro, c.idx, clip_range_vf=c.c, **c.coef)
    pol, ro = R.to_device(c.pol, c.ro)
    upd, stats = _one_call(pol, ro, c.idx.cuda(), c.coef, clip_range_vf=c.c)
    zero = P.VF_NAMES if kind == "outside" else ()
    _check("%s (%d,%d) bs=%d" % (kind, ns, na, bs), pol, stats, ref64, st64, bs, bitwise_zero=zero)
    if kind == "outside":
        assert max(r.abs().max().item() for r in ref64[4:8]) == 0.0
    else:  # the clip is not what makes the vf side small
        assert max(r.abs().max().item() for r in ref64[4:8]) > 1e-4
    if kind != "inside":  # and it changes the loss: the unclipped reference is far outside the bars
        _, plain = R.reference(c.pol, c.ro, c.idx, **c.coef)
        assert abs(plain[1] - st64[1]) > 30 * (1e-5 * abs(st64[1]) + 1e-6)
    d = upd.train_stats()  # one evaluated minibatch: the means are its figures
    assert d["train/n_minibatches"] == 1 and d["train/n_evaluated"] == 1 and d["train/early_stop"] is False
    assert d["train/value_loss"] == stats[1] and d["train/approx_kl"] == stats[4]
    assert d["train/entropy_loss"] == -stats[2] and d["train/policy_gradient_loss"] == stats[0]


@pytest.mark.parametrize("ns,na,bs", R.VCLIP_SHAPES)
@pytest.mark.parametrize("vclip", [False, True])
def test_raw_advantages_match_float64(ns, na, bs, vclip):
    """normalize_advantage=False on the 50 + 0.5 randn advantages (every A ~ 50: 50 x the normalised
    case's gradients on the pi side), alone and together with the value clip, on the value-clip
    tests' three shapes."""
    import torch

    c = P.edge_case("offset_adv", bs, ns, na)
    ro = c.ro
    opts = dict(normalize_advantage=False)
    if vclip:
        g = torch.Generator().manual_seed(bs)
        V = R.values(c.pol, c.ro, torch.arange(1500), torch.float64)
        # a fixed distance either side of c = 0.2: 0.1 (inside) or 0.4 (outside), far from the edge
        d = torch.where(torch.rand(1500, generator=g) < 0.5, 0.1, 0.4)
        d = d * torch.where(torch.rand(1500, generator=g) < 0.5, -1.0, 1.0)
        ro = R.with_values(c.ro, (V - d).float())
        opts["clip_range_vf"] = 0.2
    ref64, st64 = R.reference(c.pol, ro, c.idx, clip_range_vf=opts.get("clip_range_vf"), normalize_advantage=False,
                              **c.coef)
    _, normed = R.reference(c.pol, ro, c.idx, **c.coef)
    assert abs(st64[0]) > 20.0 * abs(normed[0])  # not the normalised loss
    pol, ro_d = R.to_device(c.pol, ro)
    _, stats = _one_call(pol, ro_d, c.idx.cuda(), c.coef, **opts)
    _check("raw_adv (%d,%d) bs=%d vclip=%s" % (ns, na, bs, vclip), pol, stats, ref64, st64, bs)


CHAINS = [((4096, 4096, 1000), 14, 3), ((16385, 16385, 33), 14, 3), ((3999, 3999, 2), 14, 3)]


@pytest.mark.parametrize("sizes,ns,na", CHAINS)
def test_options_off_is_bitwise_rr_ppo_update(sizes, ns, na):
    """Two epochs of three minibatches on four copies: rr_ppo_update chained and unchained,
    rr_ppo_update_opts (options off, control block on: train_stats=True) chained and unchained.
    After every call the two entry points agree bitwise in parameters, .grad, exp_avg, exp_avg_sq,
    step and stats; the control block counted every step."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdate, _policy_tensors

    n = sum(sizes) + 11
    pol0, ro0, _ = P.setup_cpu(ns, na, n, seed=sum(sizes) + ns)
    pol, ro = P.to_device(pol0, ro0)
    bs = sizes[0]
    pols = [copy.deepcopy(pol) for _ in range(4)]
    opts = [_adam(p) for p in pols]
    upd = [PPOUpdate(pols[k], opts[k], ro, bs, train_stats=k >= 2) for k in range(4)]
    assert upd[0].opts is None and upd[1].opts is None and upd[2].opts is not None and upd[3].opts is not None
    g = torch.Generator().manual_seed(5)
    for epoch in range(2):
        perm = torch.randperm(n, generator=g)[:sum(sizes)].cuda()
        mbs = list(torch.split(perm, list(sizes)))
        for k, idx in enumerate(mbs):
            nxt = mbs[k + 1] if k + 1 < len(mbs) else None
            st = [upd[0](idx, nxt, chained=k > 0), upd[1](idx), upd[2](idx, nxt, chained=k > 0, epoch_start=k == 0),
                  upd[3](idx, epoch_start=k == 0)]
            torch.cuda.synchronize()
            for old, new in ((0, 2), (1, 3)):
                assert torch.equal(st[old], st[new]), (epoch, k, st[old], st[new])
                for name, x, y in zip(P.NAMES, _policy_tensors(pols[old]), _policy_tensors(pols[new])):
                    where = (epoch, k, name)
                    assert torch.equal(x, y), where
                    assert torch.equal(x.grad, y.grad), where
                    assert torch.equal(opts[old].state[x]["exp_avg"], opts[new].state[y]["exp_avg"]), where
                    assert torch.equal(opts[old].state[x]["exp_avg_sq"], opts[new].state[y]["exp_avg_sq"]), where
                    assert torch.equal(opts[old].state[x]["step"], opts[new].state[y]["step"]), where
    assert float(opts[2].state[pols[2].log_std]["step"]) == 6
    for u in upd[2:]:
        d = u.train_stats()
        assert d["train/n_minibatches"] == 6 and d["train/n_evaluated"] == 6 and d["train/early_stop"] is False
        assert d["train/stop_epoch"] is None


def _snapshot(pol, opt):
    from rl_rocket_amd.rollout import _policy_tensors

    out = []
    for t in _policy_tensors(pol):
        st = opt.state[t]
        out.append((t.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone()))
    return out


def _same(a, b):
    import torch

    return all(torch.equal(x, y) for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def _check_train(c, pol, opt, d, ctl, n_mb=3):
    """The device run against ppo_opts_ref.train_ref: counts exactly, parameters and Adam state
    within 1e-6 max(1, |z|), the log means at the statistics bar. The statistics bar's 1e-6 says
    nothing about an approx_kl of 1e-7, so the control block's KL words are held to the reference's
    last-epoch list directly: the count exactly, the sum and the last value within 1e-5 relative +
    ppo_opts_ref.KL_FLOOR per minibatch (the fp32 estimator's rounding, reasoned there)."""
    from rl_rocket_amd import _lib
    from rl_rocket_amd.rollout import _policy_tensors

    ref = c.ref
    last = ref.kls[ref.stop_epoch * n_mb:] if ref.stop_epoch is not None else ref.kls[-n_mb:]
    print("KL words", ctl[_lib.RR_PPO_CTL_KL_SUM], ctl[_lib.RR_PPO_CTL_KL_COUNT], ctl[_lib.RR_PPO_CTL_KL_LAST], last)
    assert ctl[_lib.RR_PPO_CTL_KL_COUNT] == len(last)
    assert abs(ctl[_lib.RR_PPO_CTL_KL_SUM] - sum(last)) <= 1e-5 * sum(last) + len(last) * R.KL_FLOOR
    assert abs(ctl[_lib.RR_PPO_CTL_KL_LAST] - last[-1]) <= 1e-5 * last[-1] + R.KL_FLOOR
    assert ctl[_lib.RR_PPO_CTL_EPOCHS] == (ref.evals + n_mb - 1) // n_mb
    print(c.name, "target_kl %.3e" % c.target_kl, d)
    assert d["train/n_minibatches"] == ref.steps and d["train/n_evaluated"] == ref.evals
    assert d["train/early_stop"] is (ref.stop_epoch is not None) and d["train/stop_epoch"] == ref.stop_epoch
    for name, t, p64, m64, v64 in zip(P.NAMES, _policy_tensors(pol), ref.params, ref.exp_avg, ref.exp_avg_sq):
        st = opt.state[t]
        assert float(st["step"]) == ref.steps, name
        for what, a, z in (("param", t, p64), ("exp_avg", st["exp_avg"], m64), ("exp_avg_sq", st["exp_avg_sq"], v64)):
            err = (a.detach().double().cpu() - z).abs().max().item()
            assert err <= 1e-6 * max(1.0, z.abs().max().item()), (name, what, err)
    for k, r in ref.log.items():
        print("%-28s device %.9e fp64 %.9e" % (k, d[k], r))
        assert abs(d[k] - r) <= 1e-5 * abs(r) + 1e-6, (k, d[k], r)


@pytest.mark.parametrize("name", list(R.KL_PLACES))
def test_kl_stop_follows_the_float64_train_loop(name):
    """Three epochs of (4096, 4096, 1000) through PPOUpdate(target_kl), chained within each epoch,
    against SB3's loop in float64. The stopping call and every call after it leave parameters and
    optimizer state bitwise as they were before the stopping call."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdate

    c = R.kl_case(name)
    pol, ro = P.to_device(c.pol, c.ro)
    opt = _adam(pol)
    upd = PPOUpdate(pol, opt, ro, c.sizes[0], target_kl=c.target_kl)
    upd.reset()
    call, before_stop = 0, None
    for perm in c.perms:
        mbs = list(torch.split(perm.cuda(), list(c.sizes)))
        for k, idx in enumerate(mbs):
            if call == c.place:
                torch.cuda.synchronize()
                before_stop = _snapshot(pol, opt)
                stats_at_stop = None
            upd(idx, mbs[k + 1] if k + 1 < len(mbs) else None, chained=k > 0, epoch_start=k == 0)
            if before_stop is not None:
                torch.cuda.synchronize()
                assert _same(before_stop, _snapshot(pol, opt)), call
                if stats_at_stop is None:
                    stats_at_stop = upd.stats.clone()
                    assert abs(float(stats_at_stop[4]) - c.ref.kls[-1]) <= 1e-5 * c.ref.kls[-1] + R.KL_FLOOR
                assert torch.equal(upd.stats, stats_at_stop), call  # a no-op for stats too
            call += 1
    torch.cuda.synchronize()
    assert call == 9 and (before_stop is None) == (c.place is None)
    _check_train(c, pol, opt, upd.train_stats(), upd.ctl.tolist())


def test_graphed_kl_stop_replays_the_eager_loop_and_runs_again():
    """GraphedPPOUpdate(target_kl) over 3 x 4096 rows, three epochs, against the eager PPOUpdate loop
    on the same permutations (same generator): bitwise parameters, optimizer state and control
    block, the stop mid-epoch in the second epoch as the float64 loop has it. A second update() runs
    again on the next iteration's rollout: update() cleared the block."""
    import torch
    from rl_rocket_amd.rollout import GraphedPPOUpdate, PPOUpdate

    sizes, n = (4096, 4096, 4096), 3 * 4096
    gen = lambda: torch.Generator("cuda:0").manual_seed(9)  # noqa: E731
    g = gen()
    perms = [torch.randperm(n, device="cuda:0", generator=g).cpu() for _ in range(3)]
    pol0, ro0, _ = R.kl_inputs(sizes=sizes, perms=perms)
    ro0 = P.make_rollout(n, 14, 3, *[x.reshape(-1)[:n * w].contiguous() for x, w in
                                     ((ro0.obs, 14), (ro0.actions, 3), (ro0.log_probs, 1), (ro0.advantages, 1),
                                      (ro0.returns, 1))])
    free = R.train_ref(pol0, ro0, perms, sizes)
    place, target = next((k, R.pick_target(free.kls, k)) for k in (4, 5, 7, 8) if R.pick_target(free.kls, k) is not None)
    c = types.SimpleNamespace(name="graphed", target_kl=target, ref=R.train_ref(pol0, ro0, perms, sizes, target_kl=target))
    for k in c.ref.kls:  # the input condition of the KL cases (tests/test_ppo_opts_host.py checks theirs)
        assert abs(k - 1.5 * target) >= max(R.KL_GAP * 1.5 * target, R.KL_FLOOR), (k, target)
    assert (c.ref.steps, c.ref.evals, c.ref.stop_epoch) == (place, place + 1, place // 3) and place % 3
    pol, ro = P.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [_adam(p) for p in pols]
    eager = PPOUpdate(pols[0], opts[0], ro, 4096, target_kl=target)
    graphed = GraphedPPOUpdate(pols[1], opts[1], ro, batch_size=4096, target_kl=target)
    assert graphed.fused and graphed._update is not None and graphed._update.opts is not None
    eager.reset()
    for perm in perms:
        mbs = list(torch.split(perm.cuda(), list(sizes)))
        for k, idx in enumerate(mbs):
            eager(idx, mbs[k + 1] if k + 1 < 3 else None, chained=k > 0, epoch_start=k == 0)
    graphed.update(n_epochs=3, generator=gen())
    torch.cuda.synchronize()
    assert _same(_snapshot(pols[0], opts[0]), _snapshot(pols[1], opts[1]))
    assert torch.equal(eager.ctl, graphed._update.ctl)
    d = graphed.train_stats()
    assert d == eager.train_stats()
    _check_train(c, pols[1], opts[1], d, graphed._update.ctl.tolist())
    stopped = _snapshot(pols[1], opts[1])
    # a new iteration: the rollout's log-probs are the current policy's (approx_kl starts near 0
    # again; against the old ones the first minibatch would stop at once, as in SB3), written in
    # place into the tensors the graph reads
    with torch.no_grad():
        p64 = copy.deepcopy(pols[1]).double()
        mean, _ = p64(ro.obs.view(n, 14).double())
        ro.log_probs.view(n).copy_(p64.log_prob(mean, ro.actions.view(n, 3).double()).float())
    graphed.update(n_epochs=1, generator=gen())  # update() cleared the block: minibatches step again
    torch.cuda.synchronize()
    d2 = graphed.train_stats()
    print("second update", d2)
    assert d2["train/n_minibatches"] >= 1 and not _same(stopped, _snapshot(pols[1], opts[1]))
    assert float(opts[1].state[pols[1].log_std]["step"]) == place + d2["train/n_minibatches"]


@pytest.mark.parametrize("null", ["control", "stats"])
def test_the_c_call_without_a_control_block_or_without_stats(null):
    """rr_ppo_update_opts called directly with control NULL (options off: nothing needs it) or with
    stats NULL (the control block's sums are then the only record): bitwise rr_ppo_update's step on a
    copy, and the block's sums are that minibatch's figures."""
    import ctypes

    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.rollout import PPOUpdate

    bs = 1000
    pol0, ro0, _ = P.setup_cpu(14, 3, 1500, seed=12)
    pol, ro = P.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [_adam(p) for p in pols]
    plain = PPOUpdate(pols[0], opts[0], ro, bs)
    u = PPOUpdate(pols[1], opts[1], ro, bs, train_stats=True)  # its buffers; the call below is made by hand
    idx = torch.randperm(1500, generator=torch.Generator().manual_seed(3))[:bs].cuda()
    want = plain(idx).clone()
    o, a, lp, adv, ret = u.data
    clip, ent, vf = u.coef
    record = _lib.RrPpoOptions(0.0, 0.0, 1, 0 if null == "control" else 1)
    u.stats.fill_(-7.0)
    rc = u._lib.rr_ppo_update_opts(
        14, 3, u._params_w, u._dst, u._m, u._v, u._s, o.data_ptr(), a.data_ptr(), lp.data_ptr(), adv.data_ptr(),
        ret.data_ptr(), None, idx.data_ptr(), bs, None, 0, clip, ent, vf, u.max_norm, u.lr.data_ptr(), 0.9, 0.999, 1.0,
        ctypes.byref(record), None if null == "control" else u.ctl.data_ptr(),
        None if null == "stats" else u.stats.data_ptr(), _lib.RR_PPO_EPOCH_START, u.ws.data_ptr(), u._nbytes,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.RR_OK, u._lib.rr_last_error()
    torch.cuda.synchronize()
    assert _same(_snapshot(pols[0], opts[0]), _snapshot(pols[1], opts[1]))
    for x, y in zip(pols[0].parameters(), pols[1].parameters()):
        assert torch.equal(x.grad, y.grad)
    ctl = u.ctl.tolist()
    if null == "control":
        assert torch.equal(u.stats, want) and ctl == [0.0] * 16
    else:
        assert u.stats.tolist() == [-7.0] * 5  # not written
        w = want.tolist()
        assert [ctl[k] for k in (_lib.RR_PPO_CTL_SUM_POLICY, _lib.RR_PPO_CTL_SUM_VALUE, _lib.RR_PPO_CTL_SUM_ENTROPY,
                                 _lib.RR_PPO_CTL_SUM_CLIP, _lib.RR_PPO_CTL_KL_SUM, _lib.RR_PPO_CTL_KL_LAST)] == \
            [w[0], w[1], w[2], w[3], w[4], w[4]]
        assert [ctl[k] for k in (_lib.RR_PPO_CTL_STOP, _lib.RR_PPO_CTL_DECIDE, _lib.RR_PPO_CTL_STEPS,
                                 _lib.RR_PPO_CTL_EVALS, _lib.RR_PPO_CTL_EPOCHS, _lib.RR_PPO_CTL_KL_COUNT)] == \
            [0.0, 0.0, 1.0, 1.0, 1.0, 1.0]


def _options_case(seed, n=8192, bs=4096, n_epochs=2):
    """8192 rows with rollout values 0.3 randn off the float64 V, the epochs' permutations drawn as
    ppo_update and GraphedPPOUpdate.update draw them (one CUDA generator), and the options."""
    import torch

    pol0, ro0, _ = R.kl_inputs(sizes=(n - 11,), seed=seed, perms=[])
    V = R.values(pol0, ro0, torch.arange(n), torch.float64)
    ro0 = R.with_values(ro0, (V + 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(seed))).float())
    g = torch.Generator("cuda:0").manual_seed(seed)
    perms = [torch.randperm(n, device="cuda:0", generator=g).cpu() for _ in range(n_epochs)]
    return pol0, ro0, perms, dict(clip_range_vf=0.2, normalize_advantage=False)


def _close_to(ref, pol, opt):
    from rl_rocket_amd.rollout import _policy_tensors

    for name, t, z in zip(P.NAMES, _policy_tensors(pol), ref.params):
        assert float(opt.state[t]["step"]) == ref.steps, name
        err = (t.detach().double().cpu() - z).abs().max().item()
        assert err <= 1e-6 * max(1.0, z.abs().max().item()), (name, err)


def test_fused_ppo_update_with_the_three_options():
    """ppo_update(fused=True, clip_range_vf, normalize_advantage=False, target_kl), the one-replica
    call sequence (epoch_start on each epoch's first minibatch, a fresh control block), against a
    PPOUpdate loop on the same permutations bitwise, and against SB3's loop in float64: the stop in
    the second epoch, the step count, parameters within 1e-6 max(1, |z|)."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdate, ppo_update

    pol0, ro0, perms, kw = _options_case(21)
    sizes = (4096, 4096)
    free = R.train_ref(pol0, ro0, perms, sizes, **kw)
    place, target = next((k, R.pick_target(free.kls, k)) for k in (3, 2) if R.pick_target(free.kls, k) is not None)
    ref = R.train_ref(pol0, ro0, perms, sizes, target_kl=target, **kw)
    plain = R.train_ref(pol0, ro0, perms, sizes, target_kl=target)
    assert (ref.steps, ref.evals, ref.stop_epoch) == (place, place + 1, 1)
    assert max((a - b).abs().max().item() for a, b in zip(ref.params, plain.params)) > 1e-4  # the options matter
    pol, ro = R.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [_adam(p) for p in pols]
    st = ppo_update(pols[0], opts[0], ro, n_epochs=2, batch_size=4096, fused=True, target_kl=target,
                    generator=torch.Generator("cuda:0").manual_seed(21), **kw)
    upd = PPOUpdate(pols[1], opts[1], ro, 4096, target_kl=target, **kw)
    upd.reset()
    for perm in perms:
        a, b = torch.split(perm.cuda(), list(sizes))
        upd(a, b, epoch_start=True)
        upd(b, None, chained=True)
    torch.cuda.synchronize()
    assert _same(_snapshot(pols[0], opts[0]), _snapshot(pols[1], opts[1]))
    assert st == dict(zip(("policy_loss", "value_loss", "entropy"), upd.stats[:3].tolist()))
    _close_to(ref, pols[0], opts[0])
    d = upd.train_stats()
    assert d["train/n_minibatches"] == ref.steps and d["train/stop_epoch"] == 1
    for k, r in ref.log.items():
        assert abs(d[k] - r) <= 1e-5 * abs(r) + 1e-6, (k, d[k], r)


def test_captured_pytorch_update_takes_value_clip_and_raw_advantages():
    """GraphedPPOUpdate(fused=False, clip_range_vf, normalize_advantage=False): the captured PyTorch
    ops against the eager autograd ppo_update with the same options and permutations at
    test_graphed_ppo_update_equals_eager's bar (1e-6), and both against SB3's loop in float64."""
    import torch
    from rl_rocket_amd.rollout import GraphedPPOUpdate, ppo_update

    pol0, ro0, perms, kw = _options_case(22)
    ref = R.train_ref(pol0, ro0, perms, (4096, 4096), **kw)
    plain = R.train_ref(pol0, ro0, perms, (4096, 4096))
    assert max((a - b).abs().max().item() for a, b in zip(ref.params, plain.params)) > 1e-4
    pol, ro = R.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [_adam(p) for p in pols]
    g = GraphedPPOUpdate(pols[1], opts[1], ro, batch_size=4096, fused=False, **kw)
    assert not g.fused and g._update is None
    gen = lambda: torch.Generator("cuda:0").manual_seed(22)  # noqa: E731
    sa = ppo_update(pols[0], opts[0], ro, n_epochs=2, batch_size=4096, generator=gen(), **kw)
    sb = g.update(n_epochs=2, generator=gen())
    torch.cuda.synchronize()
    worst = max((x - y).abs().max().item() for x, y in zip(pols[0].parameters(), pols[1].parameters()))
    assert worst <= 1e-6, worst
    for k in sa:
        assert abs(sa[k] - sb[k]) <= 1e-5 * max(1.0, abs(sa[k])), (k, sa[k], sb[k])
    _close_to(ref, pols[0], opts[0])
    _close_to(ref, pols[1], opts[1])
