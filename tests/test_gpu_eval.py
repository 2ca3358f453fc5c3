"""rr_policy_evaluate (whole deterministic episodes in one launch) against the per-step path.

The bitwise reference is rr_rollout_step with the policy's log_std at -60: exp(log_std) * eps
< 6e-26 is absorbed by any mean above 1e-18 in magnitude, so the per-step kernel executes the
mean action. Handle A is stepped max_steps times and read back after every step (done,
truncated, terms, the terminal rows, the state planes); handle B, created with the same seed,
is evaluated once. Everything the evaluation writes for an env's first n_episodes episodes,
and the state it leaves, must equal A's bit for bit."""
import ctypes
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TL, NE = 80, 2            # TimeLimit and episodes per env: 160 steps
SENT = -12345.0           # pre-fill of B's outputs: rows that must stay untouched
KEEP = (50,)              # steps after which A's snapshot is kept (the max_steps cap test)


def _kw(model):
    from rl_rocket_amd.params import ENV_CONFIG_6DOF

    return ENV_CONFIG_6DOF if model == 6 else {}


def _policy(model, zero_head=False):
    import torch
    from rollout_ref import scaled_policy

    ns, na = (14, 3) if model == 6 else (7, 2)
    pol = scaled_policy(ns, na, seed=5, head_scale=1.0 if model == 6 else 0.05)
    with torch.no_grad():
        pol.log_std.fill_(-60.0)
        if zero_head:
            pol.action_net.weight.zero_()
    return pol.to(DEV)


def _batch(model, n, landing=False, **over):
    """A reset batch; `landing`: the first 32 envs 2 cm above the pad descending at 0.5 m/s, the
    next 32 at 5 m/s (see test_landing_bit)."""
    import torch
    from rl_rocket_amd.batch import RocketBatch

    args = dict(_kw(model))
    args.update(model=model, device=DEV, max_episode_steps=TL, compute_terms=True, seed=1234)
    args.update(over)
    b = RocketBatch(n, **args)
    b.reset()
    if landing:
        st, v0, _ = b.get_state()
        m = 0.5 * (float(b.cfg.ic_low[-1]) + float(b.cfg.ic_high[-1]))
        row = [0.02, 0, 0, -0.5, 0, 0, 1, 0, 0, 0, 0, 0, 0, m] if model == 6 else [0, 0.02, math.pi / 2, 0, -0.5, 0, m]
        st[:, :64] = torch.tensor(row, dtype=torch.float32, device=DEV)[:, None]
        st[3 if model == 6 else 4, 32:64] = -5.0
        v0[:32] = 0.5
        v0[32:64] = 5.0
        b.set_state(st, v0=v0)
    return b


def _aux(b):
    ck = b.checkpoint()
    return ck["state"], ck["v0"], ck["counter"], ck["ep_return"]


def _flags(done_kind):
    import torch
    from rl_rocket_amd import _lib

    event, bounds, trunc, nonfinite, landed = done_kind
    return (event * _lib.RR_EVAL_EVENT + bounds * _lib.RR_EVAL_BOUNDS + trunc * _lib.RR_EVAL_TRUNCATED
            + nonfinite * _lib.RR_EVAL_NONFINITE + landed * _lib.RR_EVAL_LANDED).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _reference(model, prec, n, landing=False, tl=TL, integrator="rk4"):
    """Handle A: NE * tl rr_rollout_step launches, read back after every step. Returns the rows the
    evaluation must write, A's snapshot (state, v0, counter, return) at the step each env's last
    episode ended (its final snapshot where it did not finish), the snapshots after the steps in
    KEEP, and the step of the first done. Never modified by the tests that share it."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout import PolicyPack

    a = _batch(model, n, landing, max_episode_steps=tl, integrator=integrator)
    pol = _policy(model)
    ns, na, nt = a.state_dim, a.action_dim, a.n_terms
    pack = PolicyPack(pol, ns, na, a.device, precision=prec)
    params = pack.pack()
    f = dict(dtype=torch.float32, device=DEV)
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    bufs = [torch.zeros((n, ns), **f), torch.zeros((n, na), **f)] + [torch.zeros(n, **f) for _ in range(4)]
    lib = _lib.load()
    ep = torch.zeros(n, dtype=torch.long, device=DEV)
    ref = dict(ret=torch.full((NE, n), SENT, **f), len=torch.full((NE, n), -7, dtype=torch.int32, device=DEV),
               flags=torch.full((NE, n), 0xEE, dtype=torch.uint8, device=DEV), tobs=torch.full((NE, n, ns), SENT, **f),
               m_first=torch.full((NE, n), SENT, **f))
    m_first = a.get_state()[0][-1].clone()
    last = [t.clone() for t in _aux(a)]
    kept, first_done = {}, None
    for t in range(NE * tl):
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        _lib.check(lib.rr_rollout_step(a._h, _ptr(params), pack.prec, 11, _ptr(it), t, 0.99, *[_ptr(b) for b in bufs],
                                       _ptr(a.obs), _ptr(a.reward), _ptr(a.done), _ptr(a.truncated), _ptr(a.terms),
                                       stream), "rr_rollout_step")
        tobs, tret, tlen = a.copy_terminal()
        snap = _aux(a)
        done, trunc, terms = a.done.bool(), a.truncated.bool(), a.terms
        fl = _flags((terms[nt + 1] > 0, terms[nt] > 0, trunc, terms[nt + 1] < 0, terms[nt - 1] != 0))
        active = ep < NE  # evaluating at this step: the snapshot of the env follows A
        end = active & done
        e_i = end.nonzero().squeeze(1)
        k_i = ep[e_i]
        if first_done is None and bool(done.any()):
            first_done = t + 1
        ref["ret"][k_i, e_i] = tret[e_i]
        ref["len"][k_i, e_i] = tlen[e_i]
        ref["flags"][k_i, e_i] = fl[e_i]
        ref["tobs"][k_i, e_i] = tobs[e_i]
        ref["m_first"][k_i, e_i] = m_first[e_i]
        m_first[e_i] = snap[0][-1, e_i]
        ep = ep + end.long()
        for dst, src in zip(last, snap):
            dst[..., active] = src[..., active]
        if t + 1 in KEEP:
            kept[t + 1] = [x.clone() for x in snap]
    torch.cuda.synchronize()
    ref.update(episodes=ep.to(torch.int32), last=last, kept=kept, first_done=first_done)
    a.close()
    return ref


def _evaluate(model, prec, n, landing=False, max_steps=NE * TL, fused=None, policy=None, record=None, **over):
    """Handle B: one evaluation into sentinel-filled outputs (`record`: a recording one; `over`: _batch's)."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = _batch(model, n, landing, **over)
    ev = PolicyEvaluator(b, policy if policy is not None else _policy(model), n_episodes=NE, max_steps=max_steps,
                         policy_dtype=prec, fused=fused, record=record)
    for t, v in ((ev.ep_return, SENT), (ev.ep_length, -7), (ev.flags, 0xEE), (ev.used_mass, SENT),
                 (ev.final_state, SENT), (ev.episodes, -7)):
        t.fill_(v)
    res = ev.run()
    torch.cuda.synchronize()
    return b, ev, res


def _compare(b, res, ref, model):
    import torch

    inv = torch.tensor((1.0 / b.cfg.state_normalizer).astype(np.float32), device=DEV)  # KParams.inv_norm
    fin = res.finished()
    assert torch.equal(res.episodes, ref["episodes"])
    assert torch.equal(res.ep_length, ref["len"])
    assert torch.equal(res.ep_return, ref["ret"])
    assert torch.equal(res.flags, ref["flags"])
    obs_rows = (res.final_state * inv[None, :, None]).permute(0, 2, 1)  # [ep][i][ns]
    assert torch.equal(torch.where(fin[:, :, None], obs_rows, torch.full_like(obs_rows, SENT)), ref["tobs"])
    # the mass at the episode's first state is A's; the terminal mass is the row just checked
    um = ref["m_first"] - res.final_state[:, -1, :]
    assert torch.equal(res.used_mass, torch.where(fin, um, torch.full_like(um, SENT)))
    # the state B is left in: A's at the step each env's last episode ended (where it finished)
    for got, want in zip(_aux(b), ref["last"]):
        assert torch.equal(got, want)
    # the post-call obs is the obs of that state
    tmp = torch.empty_like(b.obs)
    b.reset(mask=torch.zeros(b.num_envs, dtype=torch.uint8, device=DEV), obs=tmp)
    assert torch.equal(b.obs, tmp)


def _counts(ref):
    from rl_rocket_amd import _lib

    fl = ref["flags"].cpu().numpy().astype(np.int64)
    fl = fl[fl != 0xEE]
    return {k: int(((fl & bit) != 0).sum()) for k, bit in (("event", _lib.RR_EVAL_EVENT), ("bounds", _lib.RR_EVAL_BOUNDS),
                                                           ("trunc", _lib.RR_EVAL_TRUNCATED),
                                                           ("landed", _lib.RR_EVAL_LANDED))}


@pytest.mark.parametrize("n", [300, 37])  # 300: two workgroups, a ragged 44-env wave, three dead waves; 37: one partial wave
@pytest.mark.parametrize("model,prec", [(6, "fp32"), (6, "fp16x3"), (6, "bf16"), (3, "fp32")])
def test_evaluate_bitwise_equals_per_step_rollout(model, prec, n):
    """Every output row, the episode counts, and the state / counter word / running return B is
    left with, against handle A stepped 160 times with rr_rollout_step. The fp64 CPU oracle ends
    the 600 episodes of the 300 envs as 25 ground events, 548 bounds violations, 27 truncations
    (6DOF) and 362 ground events, 238 truncations, 0 bounds violations (3DOF); the fp32 kernels may
    differ by a few, so each way an episode can end is only required to occur."""
    ref = _reference(model, prec, n)
    if n == 300:
        c = _counts(ref)
        print("ends of handle A (%dDOF, %s): %s" % (model, prec, c))
        assert c["trunc"] >= 1 and c["event"] >= 1
        if model == 6:
            assert c["bounds"] >= 1
    assert int(ref["episodes"].min()) == NE  # TimeLimit 80: every env ends two episodes in 160 steps
    b, ev, res = _evaluate(model, prec, n)
    _compare(b, res, ref, model)
    assert res.stats()["episodes"] == NE * n
    b.close()


@pytest.mark.parametrize("model", [6, 3])
def test_landing_bit(model):
    """No random episode lands, so the first 32 envs of both handles start 2 cm above the pad at
    -0.5 m/s (on the CPU oracle such a state ends in one step with rew_goal = kappa for 1 529 of
    2 000 uniform random actions, 6DOF, and 1 643 of 2 000, 3DOF). The 32 envs share one state,
    so under the deterministic policy they share one fate: the 3DOF policy lands them, but the
    6DOF policy (head_scale 1.0) answers that state with a thrust mean of 1.42, full thrust after
    the clip, and the rocket lifts off (CPU oracle: 0.027 m after one step, climbing). Envs
    32..63 therefore start from the same state descending at 5 m/s, which no thrust stops within
    2 cm: both models land them in one step on the oracle (rew_goal = kappa), under the
    10 m/s landing limit."""
    ref = _reference(model, "fp32", 300, True)
    c = _counts(ref)
    print("ends of handle A with 64 landing states (%dDOF): %s" % (model, c))
    assert c["landed"] >= 1
    b, ev, res = _evaluate(model, "fp32", 300, landing=True)
    _compare(b, res, ref, model)
    s = res.stats()
    assert s["ep_statistic/landing_success"] == pytest.approx(c["landed"] / (NE * 300), rel=1e-12)
    b.close()


def test_max_steps_cap_leaves_rows_untouched():
    """3DOF, max_steps = 50 (the shortest oracle episode is 73 steps): no env finishes, no row is
    written, and B's state is A's after 50 steps."""
    import torch

    ref = _reference(3, "fp32", 300)
    assert ref["first_done"] > 50
    b, ev, res = _evaluate(3, "fp32", 300, max_steps=50)
    assert torch.equal(res.episodes, torch.zeros_like(res.episodes))
    for t, v in ((res.ep_return, SENT), (res.ep_length, -7), (res.flags, 0xEE), (res.used_mass, SENT),
                 (res.final_state, SENT)):
        assert torch.equal(t, torch.full_like(t, v))
    for got, want in zip(_aux(b), ref["kept"][50]):
        assert torch.equal(got, want)
    s = res.stats()
    assert s["episodes"] == 0 and s["unfinished"] == NE * 300
    b.close()


def test_fused_equals_unfused_with_a_constant_mean():
    """With the action head's weight zeroed the mean is the bias whatever the tower arithmetic, so
    the one-launch kernel and the PyTorch-op path (fused=False) agree on every output bit."""
    import torch

    pol = _policy(6, zero_head=True)
    outs = []
    for fused in (True, False):
        b, ev, res = _evaluate(6, "fp32", 300, fused=fused, policy=pol)
        assert ev.fused == fused
        outs.append((b, res))
    (b0, r0), (b1, r1) = outs
    assert int(r0.episodes.min()) == NE
    for name in ("episodes", "ep_return", "ep_length", "flags", "used_mass", "final_state"):
        assert torch.equal(getattr(r0, name), getattr(r1, name)), name
    for x, y in zip(_aux(b0), _aux(b1)):
        assert torch.equal(x, y)
    assert torch.equal(b0.obs, b1.obs)
    b0.close()
    b1.close()


def test_unfused_dopri5_equals_a_plain_step_loop_and_evaluate_policy():
    """Exact-mode envs are evaluated by the PyTorch-op path (chosen automatically): each env's
    first episode has the return and length the Monitor rows of a plain mean-action step loop on
    a twin batch report, bit for bit; evaluate_policy returns the same episodes SB3-style."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator, evaluate_policy

    n, tl = 64, 20
    pol = _policy(6)
    b = _batch(6, n, integrator="dopri5", max_episode_steps=tl)
    ev = PolicyEvaluator(b, pol, n_episodes=1)
    assert not ev.fused and ev.max_steps == tl
    res = ev.run()
    twin = _batch(6, n, integrator="dopri5", max_episode_steps=tl)
    obs = twin.obs
    seen = torch.zeros(n, dtype=torch.bool, device=DEV)
    ret = torch.zeros(n, device=DEV)
    ln = torch.zeros(n, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for _ in range(tl):
            obs, rew, done, trunc = twin.step(torch.clamp(pol.action_net(pol.pi_net(obs)), -1.0, 1.0))
            _, tret, tlen = twin.copy_terminal()
            first = done.bool() & ~seen
            ret = torch.where(first, tret, ret)
            ln = torch.where(first, tlen, ln)
            seen |= done.bool()
    torch.cuda.synchronize()
    assert bool(seen.all()) and torch.equal(res.episodes, torch.ones_like(res.episodes))
    assert torch.equal(res.ep_return[0], ret) and torch.equal(res.ep_length[0], ln)
    assert int(ln.min()) >= 1 and int(ln.max()) <= tl
    rewards, lengths = evaluate_policy(pol, twin, n_eval_episodes=1, return_episode_rewards=True)
    assert len(rewards) == n and len(lengths) == n and max(lengths) <= tl
    mean, std = evaluate_policy(pol, _batch(6, 300), n_eval_episodes=NE)
    assert math.isfinite(mean) and std > 0.0
    b.close()
    twin.close()


def test_graph_replay_equals_eager():
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = _batch(6, 300)
    ck = b.checkpoint()
    ev = PolicyEvaluator(b, _policy(6), n_episodes=NE, max_steps=NE * TL)
    res = ev.run()
    torch.cuda.synchronize()
    names = ("episodes", "ep_return", "ep_length", "flags", "used_mass", "final_state")
    eager = {k: getattr(res, k).clone() for k in names}
    eager_state = [t.clone() for t in _aux(b)]
    eager_obs = b.obs.clone()
    b.restore(ck)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ev.run()
    torch.cuda.current_stream().wait_stream(s)
    b.restore(ck)
    for k in names:
        getattr(res, k).fill_(0)
    b.obs.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(res, k), eager[k]), k
    for x, y in zip(_aux(b), eager_state):
        assert torch.equal(x, y)
    assert torch.equal(b.obs, eager_obs)
    b.close()


def test_argument_errors():
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout import PolicyPack

    lib = _lib.load()
    n = 64
    pol = _policy(6)
    params = PolicyPack(pol, 14, 3, torch.device(DEV)).pack()
    ep = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = _lib.RrEvalOut(episodes=ep.data_ptr())

    def call(b, n_episodes=1, max_steps=0, o=out):
        return lib.rr_policy_evaluate(b._h, _ptr(params), 0, n_episodes, max_steps, ctypes.byref(o), None, None)

    def refused(rc):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(b"rr_policy_evaluate: ") and len(msg) > 30, msg

    ok = _batch(6, n)
    refused(call(_batch(6, n, auto_reset=False)))
    refused(call(_batch(6, n, integrator="dopri5")))
    refused(call(ok, n_episodes=0))
    refused(call(_batch(6, n, max_episode_steps=0), max_steps=0))
    refused(call(ok, o=_lib.RrEvalOut()))
    refused(lib.rr_policy_evaluate(ok._h, _ptr(params), 7, 1, 0, ctypes.byref(out), None, None))
    assert call(ok) == 0  # the same call with nothing wrong: only `episodes` is written
    torch.cuda.synchronize()
    assert torch.equal(ep, torch.ones_like(ep))


def test_full_size_sanity():
    """N = 65 536, 6DOF, TimeLimit 80, one episode per env: every env finishes it."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    n = 65536
    b = _batch(6, n)
    res = PolicyEvaluator(b, _policy(6), n_episodes=1).run()
    torch.cuda.synchronize()
    assert torch.equal(res.episodes, torch.ones_like(res.episodes))
    assert int(res.ep_length.min()) >= 1 and int(res.ep_length.max()) <= TL
    assert res.stats()["episodes"] == n
    b.close()
