"""rr_ppo_update_discrete_opts (rl_rocket_amd/csrc/discrete_opts/: SB3's clip_range_vf,
normalize_advantage=False, target_kl and the train() log means on the device, for the Categorical policy)
against float64 PyTorch restatements of SB3 1.6's minibatch loss and PPO.train loop
(tests/discrete_opts_ref.py); the fused path is never its own reference. Inputs are built on the CPU;
their conditions (clip margins, KL thresholds) are checked there by tests/test_discrete_opts_host.py.

1. Gradients with the options on, one unchained call without a gradient clip: the value clip's four
   kinds, raw advantages alone and with the value clip. Bars of test_gpu_ppo_opts._check: per tensor
   max |fused - fp64| <= 1e-4 max |fp64| + 1e-7, stats 1e-5 relative + 1e-6, clip_fraction the
   reference's sample count exactly. The [K][64] / [K] head gradients sit in front of guard regions.
2. Options off: bitwise rr_ppo_update_discrete, chained and unchained.
3. The KL stop at its places against discrete_opts_ref.train_ref, and GraphedPPOUpdate(fused=True,
   target_kl, train_stats) against the eager PPOUpdate loop.
4. The C call itself without a control block, without stats, without old_values.
5. ppo_update(fused=True) with the three options against a PPOUpdate loop and the float64 loop."""
import copy
import types

import pytest

import discrete_opts_ref as Q
import discrete_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -777.0
GUARD = 512  # floats after each head gradient: more than the [4][64] + [4] a full-width write would reach


def _adam(pol, lr=1e-3):
    import torch

    return torch.optim.Adam(pol.parameters(), lr=lr, eps=1.0, capturable=True)


def _check(label, pol, stats, ref64, st64, bs, bitwise_zero=()):
    """test_gpu_ppo_opts._check over the 12 tensors: the project's bars with clip_fraction exact."""
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    for name, t, r in zip(Q.NAMES, _policy_tensors(pol), ref64):
        a = t.grad.double().cpu()
        scale, err = r.abs().max().item(), (a - r).abs().max().item()
        print("%s %-9s max|ref| %.3e  fused err %.2e" % (label, name, scale, err))
        assert a.shape == r.shape, name
        assert bool(torch.isfinite(a).all()), name
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale)
        if name in bitwise_zero:
            assert torch.count_nonzero(a).item() == 0, name
    assert all(v == v and abs(v) != float("inf") for v in stats), stats
    for k, (a, r) in enumerate(zip(stats, st64)):
        print("%s %-13s fused %.9e fp64 %.9e" % (label, Q.STAT_NAMES[k], a, r))
        assert abs(a - r) <= 1e-5 * abs(r) + 1e-6, (k, a, r)
    assert round(stats[3] * bs) == round(st64[3] * bs), (stats[3], st64[3])


def _guarded(pol):
    """The action head's .grad tensors as the front of sentinel-filled buffers: [(buffer, numel)]."""
    import torch

    out = []
    for p in (pol.action_net.weight, pol.action_net.bias):
        buf = torch.full((p.numel() + GUARD,), SENTINEL, dtype=torch.float32, device=p.device)
        p.grad = buf[:p.numel()].view_as(p)
        out.append((buf, p.numel()))
    return out


def _one_call(pol, ro, idx, coef, **opts):
    """One unchained PPOUpdateDiscrete call with max_grad_norm None: .grad is left unscaled, the gradient at
    the parameters the call started from. The head gradients are written in full and nothing past them."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdateDiscrete

    guards = _guarded(pol)
    upd = PPOUpdateDiscrete(pol, _adam(pol), ro, idx.numel(), coef["clip"], coef["ent_coef"], coef["vf_coef"],
                            max_grad_norm=None, **opts)
    assert upd.opts is not None and upd._call == "rr_ppo_update_discrete_opts"
    upd.ws.fill_(float("nan"))  # an unchained call reads nothing a previous call left
    stats = upd(idx, epoch_start=True).tolist()
    torch.cuda.synchronize()
    for buf, numel in guards:
        assert bool((buf[numel:] == SENTINEL).all()), "written past a head gradient"
        assert not bool((buf[:numel] == SENTINEL).any()), "a head gradient element was not written"
    return upd, stats


@pytest.mark.parametrize("k,bs", Q.VCLIP_SHAPES)
@pytest.mark.parametrize("kind", Q.VCLIP_KINDS)
def test_value_clip_matches_float64(kind, k, bs):
    c = Q.vclip_case(kind, k, bs)
    ref64, st64 = Q.reference(c.pol, c.ro, c.idx, clip_range_vf=c.c, **c.coef)
    pol, ro = Q.to_device(c.pol, c.ro)
    upd, stats = _one_call(pol, ro, c.idx.to(DEV), c.coef, clip_range_vf=c.c)
    zero = Q.VF_NAMES if kind == "outside" else ()
    _check("%s k=%d bs=%d" % (kind, k, bs), pol, stats, ref64, st64, bs, bitwise_zero=zero)
    assert pol.action_net.weight.grad.shape == (k, 64) and pol.action_net.bias.grad.shape == (k,)
    d = upd.train_stats()  # one evaluated minibatch: the means are its figures
    assert d["train/n_minibatches"] == 1 and d["train/n_evaluated"] == 1 and d["train/early_stop"] is False
    assert d["train/value_loss"] == stats[1] and d["train/approx_kl"] == stats[4]
    assert d["train/entropy_loss"] == -stats[2] and d["train/policy_gradient_loss"] == stats[0]
    assert d["train/clip_fraction"] == stats[3] and d["train/stop_epoch"] is None


@pytest.mark.parametrize("k,bs", Q.RAW_SHAPES)
@pytest.mark.parametrize("vclip", [False, True])
def test_raw_advantages_match_float64(k, bs, vclip):
    """normalize_advantage=False on the 50 + 0.5 randn advantages, alone and together with the value clip."""
    c = Q.raw_case(k, bs, vclip)
    ref64, st64 = Q.reference(c.pol, c.ro, c.idx, clip_range_vf=c.opts.get("clip_range_vf"), normalize_advantage=False,
                              **c.coef)
    pol, ro = Q.to_device(c.pol, c.ro)
    _, stats = _one_call(pol, ro, c.idx.to(DEV), c.coef, **c.opts)
    _check("raw_adv k=%d bs=%d vclip=%s" % (k, bs, vclip), pol, stats, ref64, st64, bs)


CHAINS = [((4096, 4096, 1000), 4), ((4096, 4096, 1000), 2), ((16385, 16385, 33), 4), ((3999, 3999, 2), 4)]


@pytest.mark.parametrize("sizes,k", CHAINS)
def test_options_off_is_bitwise_rr_ppo_update_discrete(sizes, k):
    """Two epochs of three minibatches on four copies: rr_ppo_update_discrete chained and unchained,
    rr_ppo_update_discrete_opts (options off, control block on: train_stats=True) chained and unchained.
    After every call the two entry points agree bitwise in parameters, .grad, exp_avg, exp_avg_sq, step and
    stats; the control block counted every call."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.rollout import PPOUpdateDiscrete, _policy_tensors

    n = sum(sizes) + 11
    pol0, ro0, _ = D.learner_inputs(k, n=n, seed=sum(sizes) + k)
    pol, ro = D.to_device(pol0, ro0)
    bs = sizes[0]
    pols = [copy.deepcopy(pol) for _ in range(4)]
    opts = [_adam(p) for p in pols]
    upd = [PPOUpdateDiscrete(pols[j], opts[j], ro, bs, train_stats=j >= 2) for j in range(4)]
    assert [u._call for u in upd] == ["rr_ppo_update_discrete"] * 2 + ["rr_ppo_update_discrete_opts"] * 2
    assert upd[0].opts is None and upd[1].opts is None and upd[0].ctl is None
    g = torch.Generator().manual_seed(5)
    for epoch in range(2):
        perm = torch.randperm(n, generator=g)[:sum(sizes)].to(DEV)
        mbs = list(torch.split(perm, list(sizes)))
        for j, idx in enumerate(mbs):
            nxt = mbs[j + 1] if j + 1 < len(mbs) else None
            st = [upd[0](idx, nxt, chained=j > 0), upd[1](idx), upd[2](idx, nxt, chained=j > 0, epoch_start=j == 0),
                  upd[3](idx, epoch_start=j == 0)]
            torch.cuda.synchronize()
            for old, new in ((0, 2), (1, 3)):
                assert torch.equal(st[old], st[new]), (epoch, j, st[old], st[new])
                for name, x, y in zip(Q.NAMES, _policy_tensors(pols[old]), _policy_tensors(pols[new])):
                    where = (epoch, j, name)
                    assert torch.equal(x, y), where
                    assert torch.equal(x.grad, y.grad), where
                    assert torch.equal(opts[old].state[x]["exp_avg"], opts[new].state[y]["exp_avg"]), where
                    assert torch.equal(opts[old].state[x]["exp_avg_sq"], opts[new].state[y]["exp_avg_sq"]), where
                    assert torch.equal(opts[old].state[x]["step"], opts[new].state[y]["step"]), where
    assert float(opts[2].state[pols[2].action_net.bias]["step"]) == 6
    for u in upd[2:]:
        ctl = u.ctl.tolist()
        assert ctl[_lib.RR_PPO_CTL_STEPS] == 6.0 and ctl[_lib.RR_PPO_CTL_EVALS] == 6.0
        assert ctl[_lib.RR_PPO_CTL_EPOCHS] == 2.0 and ctl[_lib.RR_PPO_CTL_STOP] == 0.0
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
    """test_gpu_ppo_opts._check_train over the 12 tensors: counts exactly, parameters and Adam state within
    1e-6 max(1, |z|), the log means at the statistics bar, the control block's KL words against the
    reference's last-epoch list (1e-5 relative + KL_FLOOR per minibatch)."""
    from rl_rocket_amd import _lib
    from rl_rocket_amd.rollout import _policy_tensors

    ref = c.ref
    last = ref.kls[ref.stop_epoch * n_mb:] if ref.stop_epoch is not None else ref.kls[-n_mb:]
    print("KL words", ctl[_lib.RR_PPO_CTL_KL_SUM], ctl[_lib.RR_PPO_CTL_KL_COUNT], ctl[_lib.RR_PPO_CTL_KL_LAST], last)
    assert ctl[_lib.RR_PPO_CTL_KL_COUNT] == len(last)
    assert abs(ctl[_lib.RR_PPO_CTL_KL_SUM] - sum(last)) <= 1e-5 * sum(last) + len(last) * Q.KL_FLOOR
    assert abs(ctl[_lib.RR_PPO_CTL_KL_LAST] - last[-1]) <= 1e-5 * last[-1] + Q.KL_FLOOR
    assert ctl[_lib.RR_PPO_CTL_EPOCHS] == (ref.evals + n_mb - 1) // n_mb
    print(c.name, "target_kl %.3e" % c.target_kl, d)
    assert d["train/n_minibatches"] == ref.steps and d["train/n_evaluated"] == ref.evals
    assert d["train/early_stop"] is (ref.stop_epoch is not None) and d["train/stop_epoch"] == ref.stop_epoch
    for name, t, p64, m64, v64 in zip(Q.NAMES, _policy_tensors(pol), ref.params, ref.exp_avg, ref.exp_avg_sq):
        st = opt.state[t]
        assert float(st["step"]) == ref.steps, name
        for what, a, z in (("param", t, p64), ("exp_avg", st["exp_avg"], m64), ("exp_avg_sq", st["exp_avg_sq"], v64)):
            err = (a.detach().double().cpu() - z).abs().max().item()
            assert err <= 1e-6 * max(1.0, z.abs().max().item()), (name, what, err)
    for key, r in ref.log.items():
        print("%-28s device %.9e fp64 %.9e" % (key, d[key], r))
        assert abs(d[key] - r) <= 1e-5 * abs(r) + 1e-6, (key, d[key], r)


@pytest.mark.parametrize("name", list(Q.KL_PLACES))
def test_kl_stop_follows_the_float64_train_loop(name):
    """Three epochs of (4096, 4096, 1000) through PPOUpdate(target_kl) on a Categorical policy, chained
    within each epoch, against SB3's loop in float64. The stopping call and every call after it leave
    parameters and optimizer state bitwise as they were before the stopping call; the calls after it also
    leave stats, the control block and the whole workspace (the packed images among it) as they were."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdate

    c = Q.kl_case(name)
    pol, ro = D.to_device(c.pol, c.ro)
    opt = _adam(pol, Q.KL_LR)
    upd = PPOUpdate(pol, opt, ro, c.sizes[0], target_kl=c.target_kl)
    assert upd._call == "rr_ppo_update_discrete_opts" and upd.ctl is not None
    upd.reset()
    call, before_stop, at_stop = 0, None, None
    for perm in c.perms:
        mbs = list(torch.split(perm.to(DEV), list(c.sizes)))
        for j, idx in enumerate(mbs):
            if call == c.place:
                torch.cuda.synchronize()
                before_stop = _snapshot(pol, opt)
            upd(idx, mbs[j + 1] if j + 1 < len(mbs) else None, chained=j > 0, epoch_start=j == 0)
            if before_stop is not None:
                torch.cuda.synchronize()
                assert _same(before_stop, _snapshot(pol, opt)), call  # the stopping minibatch took no step
                if at_stop is None:
                    at_stop = (upd.stats.clone(), upd.ctl.clone(), upd.ws.clone())
                    assert abs(float(at_stop[0][4]) - c.ref.kls[-1]) <= 1e-5 * c.ref.kls[-1] + Q.KL_FLOOR
                for was, now in zip(at_stop, (upd.stats, upd.ctl, upd.ws)):  # a later call changes nothing
                    assert torch.equal(was.view(torch.int32), now.view(torch.int32)), call
            call += 1
    torch.cuda.synchronize()
    assert call == 9 and (before_stop is None) == (c.place is None)
    _check_train(c, pol, opt, upd.train_stats(), upd.ctl.tolist())


def _current_log_probs(pol, ro, n):
    """The float64 forward's log-prob of the rollout's actions under `pol`, written in place (fp32)."""
    import torch

    _, _, lp = D.forward64(pol, ro.obs.reshape(n, 7))
    lp = torch.from_numpy(lp).gather(1, ro.actions.reshape(n).long().cpu()[:, None])[:, 0]
    ro.log_probs.view(n).copy_(lp.float().to(ro.log_probs.device))


def test_graphed_kl_stop_replays_the_eager_loop_and_runs_again():
    """GraphedPPOUpdate(fused=True, target_kl, train_stats=True) over 3 x 4096 rows, KL_EPOCHS epochs,
    against the eager PPOUpdate loop on the same permutations (same generator): bitwise parameters,
    optimizer state and control block, the stop mid-epoch in the second epoch as the float64 loop has it;
    the replays after the stop are no-ops that update() never read anything for. A second update() runs
    again on the next iteration's rollout: update() cleared the block."""
    import torch
    from rl_rocket_amd.rollout import GraphedPPOUpdate, PPOUpdate

    sizes, n = (4096, 4096, 4096), 3 * 4096
    gen = lambda: torch.Generator(DEV).manual_seed(9)  # noqa: E731
    g = gen()
    perms = [torch.randperm(n, device=DEV, generator=g).cpu() for _ in range(Q.KL_EPOCHS)]
    pol0, ro0, _ = Q.kl_inputs(sizes=sizes, perms=perms, n=n)
    free = Q.train_ref(pol0, ro0, perms, sizes, lr=Q.KL_LR)
    place, target = next((j, Q.pick_target(free.kls, j)) for j in (4, 5, 7, 8) if Q.pick_target(free.kls, j) is not None)
    c = types.SimpleNamespace(name="graphed", target_kl=target,
                              ref=Q.train_ref(pol0, ro0, perms, sizes, target_kl=target, lr=Q.KL_LR))
    for kl in c.ref.kls:  # the input condition of the KL cases (tests/test_discrete_opts_host.py checks theirs)
        assert abs(kl - 1.5 * target) >= max(Q.KL_GAP * 1.5 * target, Q.KL_FLOOR), (kl, target)
    assert (c.ref.steps, c.ref.evals, c.ref.stop_epoch) == (place, place + 1, place // 3) and place % 3
    pol, ro = D.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [_adam(p, Q.KL_LR) for p in pols]
    eager = PPOUpdate(pols[0], opts[0], ro, 4096, target_kl=target, train_stats=True)
    graphed = GraphedPPOUpdate(pols[1], opts[1], ro, batch_size=4096, fused=True, target_kl=target, train_stats=True)
    assert graphed.fused and graphed._update is not None and graphed._update.opts is not None
    assert graphed._update._call == "rr_ppo_update_discrete_opts"
    eager.reset()
    for perm in perms:
        mbs = list(torch.split(perm.to(DEV), list(sizes)))
        for j, idx in enumerate(mbs):
            eager(idx, mbs[j + 1] if j + 1 < 3 else None, chained=j > 0, epoch_start=j == 0)
    graphed.update(n_epochs=Q.KL_EPOCHS, generator=gen())
    torch.cuda.synchronize()
    assert _same(_snapshot(pols[0], opts[0]), _snapshot(pols[1], opts[1]))
    assert torch.equal(eager.ctl, graphed._update.ctl)
    d = graphed.train_stats()
    assert d == eager.train_stats()
    _check_train(c, pols[1], opts[1], d, graphed._update.ctl.tolist())
    stopped = _snapshot(pols[1], opts[1])
    # a new iteration: the rollout's log-probs are the current policy's, written in place into the tensors
    # the graph reads (against the old ones the first minibatch would stop at once, as in SB3)
    _current_log_probs(pols[1], ro, n)
    graphed.update(n_epochs=1, generator=gen())  # update() cleared the block: minibatches step again
    torch.cuda.synchronize()
    d2 = graphed.train_stats()
    print("second update", d2)
    assert d2["train/n_minibatches"] >= 1 and not _same(stopped, _snapshot(pols[1], opts[1]))
    assert float(opts[1].state[pols[1].action_net.bias]["step"]) == place + d2["train/n_minibatches"]


@pytest.mark.parametrize("null", ["control", "stats", "old_values"])
def test_the_c_call_with_a_null_argument(null):
    """rr_ppo_update_discrete_opts called directly with control NULL (options off: nothing needs it), with
    stats NULL (the control block's sums are then the only record), or with everything but old_values (no
    value clip: nothing reads it; it is NULL in all three): bitwise rr_ppo_update_discrete's step on a copy,
    and the block's sums are that minibatch's figures."""
    import ctypes

    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.rollout import PPOUpdateDiscrete

    bs, k = 1000, 4
    pol0, ro0, _ = D.learner_inputs(k, seed=12)
    pol, ro = D.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [_adam(p) for p in pols]
    plain = PPOUpdateDiscrete(pols[0], opts[0], ro, bs)
    u = PPOUpdateDiscrete(pols[1], opts[1], ro, bs, train_stats=True)  # its buffers; the call below is made by hand
    idx = torch.randperm(1500, generator=torch.Generator().manual_seed(3))[:bs].to(DEV)
    want = plain(idx).clone()
    o, a, lp, adv, ret = u.data
    clip, ent, vf = u.coef
    record = _lib.RrPpoOptions(0.0, 0.0, 1, 0 if null == "control" else 1)
    u.stats.fill_(-7.0)
    rc = u._lib.rr_ppo_update_discrete_opts(
        7, k, u._params_w, u._dst, u._m, u._v, u._s, o.data_ptr(), a.data_ptr(), lp.data_ptr(), adv.data_ptr(),
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
    if null == "stats":
        assert u.stats.tolist() == [-7.0] * 5  # not written
    else:
        assert torch.equal(u.stats, want)
    if null == "control":
        assert ctl == [0.0] * 16
    else:
        w = want.tolist()
        assert [ctl[j] for j in (_lib.RR_PPO_CTL_SUM_POLICY, _lib.RR_PPO_CTL_SUM_VALUE, _lib.RR_PPO_CTL_SUM_ENTROPY,
                                 _lib.RR_PPO_CTL_SUM_CLIP, _lib.RR_PPO_CTL_KL_SUM, _lib.RR_PPO_CTL_KL_LAST)] == \
            [w[0], w[1], w[2], w[3], w[4], w[4]]
        assert [ctl[j] for j in (_lib.RR_PPO_CTL_STOP, _lib.RR_PPO_CTL_DECIDE, _lib.RR_PPO_CTL_STEPS,
                                 _lib.RR_PPO_CTL_EVALS, _lib.RR_PPO_CTL_EPOCHS, _lib.RR_PPO_CTL_KL_COUNT)] == \
            [0.0, 0.0, 1.0, 1.0, 1.0, 1.0]


@pytest.mark.parametrize("chained", [False, True])
def test_the_stop_word_alone_makes_a_call_a_no_op(chained):
    """RR_PPO_CTL_STOP written by the caller on an otherwise clear block (RR_PPO_CTL_DECIDE 0): all four
    launches, or the three of a chained call, return at entry. Parameters, optimizer state, .grad, stats, the
    block and the workspace keep every bit."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.rollout import PPOUpdateDiscrete

    pol0, ro0, _ = D.learner_inputs(4, seed=13)
    pol, ro = D.to_device(pol0, ro0)
    opt = _adam(pol)
    upd = PPOUpdateDiscrete(pol, opt, ro, 1000, train_stats=True)
    g = torch.Generator().manual_seed(4)
    a, b = torch.randperm(1500, generator=g)[:1000].to(DEV), torch.randperm(1500, generator=g)[:333].to(DEV)
    upd(a, b, epoch_start=True)  # a step: the state below is no fresh optimizer's, and b's statistics are summed
    upd.ctl[_lib.RR_PPO_CTL_STOP] = 1.0
    torch.cuda.synchronize()
    keep = [x.clone() for x in (upd.stats, upd.ctl, upd.ws)] + [p.grad.clone() for p in pol.parameters()]
    before = _snapshot(pol, opt)
    upd(b, None, chained=True) if chained else upd(b, epoch_start=True)
    torch.cuda.synchronize()
    assert _same(before, _snapshot(pol, opt))
    for was, now in zip(keep, [upd.stats, upd.ctl, upd.ws] + [p.grad for p in pol.parameters()]):
        assert torch.equal(was.view(torch.int32), now.view(torch.int32))
    assert upd.train_stats()["train/n_minibatches"] == 1


def test_fused_ppo_update_with_the_three_options():
    """ppo_update(fused=True, clip_range_vf, normalize_advantage=False, target_kl) on a Categorical policy,
    the one-replica call sequence (epoch_start on each epoch's first minibatch, a fresh control block),
    against a PPOUpdate loop on the same permutations bitwise, and against SB3's loop in float64: the stop in
    the second epoch, the step count, parameters within 1e-6 max(1, |z|)."""
    import torch
    from rl_rocket_amd.rollout import PPOUpdate, _policy_tensors, ppo_update

    n, sizes, seed = 8192, (4096, 4096), 21
    pol0, ro0, _ = Q.kl_inputs(sizes=(n,), seed=seed, perms=[], n=n)
    V = Q.values(pol0, ro0, torch.arange(n), torch.float64)
    ro0 = Q.with_values(ro0, (V + 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(seed))).float())
    g = torch.Generator(DEV).manual_seed(seed)
    perms = [torch.randperm(n, device=DEV, generator=g).cpu() for _ in range(2)]
    kw = dict(clip_range_vf=0.2, normalize_advantage=False)
    free = Q.train_ref(pol0, ro0, perms, sizes, lr=Q.KL_LR, **kw)
    place, target = next((j, Q.pick_target(free.kls, j)) for j in (3, 2) if Q.pick_target(free.kls, j) is not None)
    ref = Q.train_ref(pol0, ro0, perms, sizes, target_kl=target, lr=Q.KL_LR, **kw)
    plain = Q.train_ref(pol0, ro0, perms, sizes, target_kl=target, lr=Q.KL_LR)
    for kl in ref.kls:
        assert abs(kl - 1.5 * target) >= max(Q.KL_GAP * 1.5 * target, Q.KL_FLOOR), (kl, target)
    assert (ref.steps, ref.evals, ref.stop_epoch) == (place, place + 1, 1)
    assert max((a - b).abs().max().item() for a, b in zip(ref.params, plain.params)) > 1e-4  # the options matter
    pol, ro = Q.to_device(pol0, ro0)
    pols = [copy.deepcopy(pol) for _ in range(2)]
    opts = [_adam(p, Q.KL_LR) for p in pols]
    st = ppo_update(pols[0], opts[0], ro, n_epochs=2, batch_size=4096, fused=True, target_kl=target,
                    generator=torch.Generator(DEV).manual_seed(seed), **kw)
    upd = PPOUpdate(pols[1], opts[1], ro, 4096, target_kl=target, **kw)
    assert upd._call == "rr_ppo_update_discrete_opts"
    upd.reset()
    for perm in perms:
        a, b = torch.split(perm.to(DEV), list(sizes))
        upd(a, b, epoch_start=True)
        upd(b, None, chained=True)
    torch.cuda.synchronize()
    assert _same(_snapshot(pols[0], opts[0]), _snapshot(pols[1], opts[1]))
    assert st == dict(zip(("policy_loss", "value_loss", "entropy"), upd.stats[:3].tolist()))
    for name, t, z in zip(Q.NAMES, _policy_tensors(pols[0]), ref.params):
        assert float(opts[0].state[t]["step"]) == ref.steps, name
        err = (t.detach().double().cpu() - z).abs().max().item()
        assert err <= 1e-6 * max(1.0, z.abs().max().item()), (name, err)
    d = upd.train_stats()
    assert d["train/n_minibatches"] == ref.steps and d["train/stop_epoch"] == 1
    for key, r in ref.log.items():
        assert abs(d[key] - r) <= 1e-5 * abs(r) + 1e-6, (key, d[key], r)
