"""rr_policy_evaluate_exact (whole deterministic episodes under the exact integrator in one launch)
against the per-step path the library documents for exact-mode envs.

The bitwise reference is rr_policy_act + rr_step with the policy's log_std at -60 (exp(log_std) *
eps < 6e-26 is absorbed by any mean above 1e-18 in magnitude, so rr_policy_act hands rr_step the
clipped mean). Handle A is stepped NE * TL times and read back after every step: done, truncated,
terms, the terminal return / length, both state images, v0, counter word, running return and the
obs rows. The un-reset terminal state of a step (rr_eval_out.final_state) is not among rr_step's
outputs: a shadow handle S without auto-reset or TimeLimit takes the same step from the same fp64
state with the same action, as PolicyEvaluator's step-by-step path does. rr_reset writes its obs
as state * inv_norm in fp32 where the exact kernels write float32(state64 / norm), so before A's
first rr_policy_act its obs buffer is overwritten with those rows (torch's fp64 division is
correctly rounded, as the device's); from then on rr_step supplies A's observations. Handle B,
created with the same seed and given the same state, is evaluated once into sentinel-filled
outputs. Everything the evaluation writes for an env's first NE episodes, and the state it leaves,
must equal A's bit for bit.

The fixture (set through set_state64 on both handles): envs 0..31 2 cm above the pad descending at
0.5 m/s and envs 32..63 at 5 m/s (the landing states of test_gpu_eval.py), envs 64..95 at 50 m/s
(a ground event far above the 10 m/s landing limit: an event without the landing bit)."""
import ctypes
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TL, NE = 20, 2            # TimeLimit and episodes per env: 40 steps
SENT = -12345.0           # pre-fill of B's outputs: rows that must stay untouched
NAN_ENV = 130             # the env of the non-finite test: workgroup 0, wave 2, away from the fixture's envs
NAMES = ("episodes", "ep_return", "ep_length", "flags", "used_mass", "final_state")


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


def _batch(model, n, fixture="landing", **over):
    """A reset exact-mode batch. fixture "landing": see the module docstring; "nan": the same with
    one velocity component of env NAN_ENV NaN; None: the reset's own states."""
    import torch
    from rl_rocket_amd.batch import RocketBatch

    args = dict(_kw(model))
    args.update(model=model, device=DEV, max_episode_steps=TL, compute_terms=True, seed=1234, integrator="dopri5")
    args.update(over)
    b = RocketBatch(n, **args)
    b.reset()
    if fixture:
        st, v0, _ = b.get_state64()
        m = 0.5 * (float(b.cfg.ic_low[-1]) + float(b.cfg.ic_high[-1]))
        row = [0.02, 0, 0, -0.5, 0, 0, 1, 0, 0, 0, 0, 0, 0, m] if model == 6 else [0, 0.02, math.pi / 2, 0, -0.5, 0, m]
        vz = 3 if model == 6 else 4
        st[:, :96] = torch.tensor(row, dtype=torch.float64, device=DEV)[:, None]
        st[vz, 32:64] = -5.0
        st[vz, 64:96] = -50.0
        v0[:32] = 0.5
        v0[32:64] = 5.0
        v0[64:96] = 50.0
        if fixture == "nan":
            st[vz + 1, NAN_ENV] = float("nan")
        b.set_state64(st, v0=v0)
    return b


def _exact_obs(b):
    """The obs rows [n][ns] of b's state by the exact mode's formula: float32(state64 / norm) (6DOF),
    float32(float32(state64) / norm) (3DOF)."""
    import torch

    y = b.get_state64()[0]
    norm = torch.tensor(np.asarray(b.cfg.state_normalizer, dtype=np.float64), device=DEV)
    if b.model != 6:
        y = y.float().double()
    return (y / norm[:, None]).float().T.contiguous()


def _aux(b):
    """What a handle is left with: fp32 state planes, v0, counter words, running returns, fp64 state."""
    ck = b.checkpoint()
    return [ck["state"], ck["v0"], ck["counter"], ck["ep_return"], b.get_state64()[0]]


def _flags(done_kind):
    import torch
    from rl_rocket_amd import _lib

    event, bounds, trunc, nonfinite, landed = done_kind
    return (event * _lib.RR_EVAL_EVENT + bounds * _lib.RR_EVAL_BOUNDS + trunc * _lib.RR_EVAL_TRUNCATED
            + nonfinite * _lib.RR_EVAL_NONFINITE + landed * _lib.RR_EVAL_LANDED).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _reference(model, prec, n, fixture="landing", over=()):
    """Handle A: NE * TL times rr_policy_act + rr_step, read back after every step. Returns the rows
    the evaluation must write, A's snapshot (_aux and the obs rows) at the step each env's last
    episode ended (its final snapshot where it did not finish), the snapshots after every step and
    the step of the first done. Never modified by the tests that share it."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import RocketBatch, _ptr
    from rl_rocket_amd.rollout import PolicyPack

    over = dict(over)
    a = _batch(model, n, fixture, **over)
    sh = RocketBatch(n, model=model, device=DEV, max_episode_steps=0, auto_reset=False, episode_stats=False,
                     integrator="dopri5", compute_terms=True, **dict(_kw(model), **over))
    pol = _policy(model)
    ns, na, nt = a.state_dim, a.action_dim, a.n_terms
    el_mask = (1 << a.counter_bits) - 1
    pack = PolicyPack(pol, ns, na, a.device, precision=prec)
    params = pack.pack()
    f = dict(dtype=torch.float32, device=DEV)
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    act_env, act = torch.zeros((n, na), **f), torch.zeros((n, na), **f)
    val, lp = torch.zeros(n, **f), torch.zeros(n, **f)
    lib = _lib.load()
    ep = torch.zeros(n, dtype=torch.long, device=DEV)
    ref = dict(ret=torch.full((NE, n), SENT, **f), len=torch.full((NE, n), -7, dtype=torch.int32, device=DEV),
               flags=torch.full((NE, n), 0xEE, dtype=torch.uint8, device=DEV), fin=torch.full((NE, ns, n), SENT, **f),
               mass=torch.full((NE, n), SENT, **f))
    a.obs.copy_(_exact_obs(a))
    pre = _aux(a)
    m_first = pre[0][-1].clone()
    last = [t.clone() for t in pre] + [a.obs.clone()]
    kept, first_done = {}, None
    for t in range(NE * TL):
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        _lib.check(lib.rr_policy_act(_ptr(params), ns, na, pack.prec, n, 0, _ptr(a.obs), 11, _ptr(it), t, _ptr(act_env),
                                     _ptr(act), _ptr(val), _ptr(lp), None, None, None, None, 0.0, None, None, None,
                                     stream), "rr_policy_act")
        # the un-reset state after the step: the same step of the shadow handle
        sh.set_state64(pre[4], v0=pre[1], elapsed=pre[2] & el_mask)
        sh.step(act_env)
        y1 = sh.get_state64()[0].float()
        a.step(act_env)
        _, tret, tlen = a.copy_terminal()
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
        ref["fin"][k_i, :, e_i] = y1[:, e_i].T
        ref["mass"][k_i, e_i] = m_first[e_i] - y1[-1, e_i]
        m_first[e_i] = snap[0][-1, e_i]
        ep = ep + end.long()
        for dst, src in zip(last, snap):
            dst[..., active] = src[..., active]
        last[5][active] = a.obs[active]
        kept[t + 1] = [x.clone() for x in snap] + [a.obs.clone()]
        pre = snap
    torch.cuda.synchronize()
    ref.update(episodes=ep.to(torch.int32), last=last, kept=kept, first_done=first_done)
    a.close()
    sh.close()
    return ref


def _evaluate(model, prec, n, fixture="landing", max_steps=NE * TL, fused=True, policy=None, **over):
    """Handle B: one evaluation into sentinel-filled outputs (`over`: _batch's)."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = _batch(model, n, fixture, **over)
    ev = PolicyEvaluator(b, policy if policy is not None else _policy(model), n_episodes=NE, max_steps=max_steps,
                         policy_dtype=prec, fused=fused)
    assert ev.fused == fused
    for t, v in ((ev.ep_return, SENT), (ev.ep_length, -7), (ev.flags, 0xEE), (ev.used_mass, SENT),
                 (ev.final_state, SENT), (ev.episodes, -7)):
        t.fill_(v)
    b.obs.fill_(SENT)
    res = ev.run()
    torch.cuda.synchronize()
    return b, ev, res


def _same(x, y):
    """torch.equal, with NaNs in the same places counting as equal (the non-finite test only)."""
    import torch

    if not x.is_floating_point():
        return torch.equal(x, y)
    nx, ny = x.isnan(), y.isnan()
    return torch.equal(nx, ny) and torch.equal(torch.where(nx, torch.zeros_like(x), x),
                                               torch.where(ny, torch.zeros_like(y), y))


def _compare(b, res, ref, snapshot=None, eq=None):
    import torch

    eq = eq or torch.equal
    assert eq(res.episodes, ref["episodes"])
    assert eq(res.ep_length, ref["len"])
    assert eq(res.ep_return, ref["ret"])
    assert eq(res.flags, ref["flags"])
    assert eq(res.final_state, ref["fin"])  # rows of unfinished episodes: the sentinel on both sides
    assert eq(res.used_mass, ref["mass"])
    # the state B is left in: A's at the step each env's last episode ended (where it finished)
    want = snapshot if snapshot is not None else ref["last"]
    for name, got, w in zip(("state", "v0", "counter", "ep_return", "state64"), _aux(b), want):
        assert eq(got, w), name
    assert eq(b.obs, want[5])


def _counts(ref):
    from rl_rocket_amd import _lib

    fl = ref["flags"].cpu().numpy().astype(np.int64)
    ep = ref["episodes"].cpu().numpy()
    fl = fl[fl != 0xEE]
    ev, la = (fl & _lib.RR_EVAL_EVENT) != 0, (fl & _lib.RR_EVAL_LANDED) != 0
    return dict(event_landed=int((ev & la).sum()), event_not_landed=int((ev & ~la).sum()),
                trunc=int(((fl & _lib.RR_EVAL_TRUNCATED) != 0).sum()), bounds=int(((fl & _lib.RR_EVAL_BOUNDS) != 0).sum()),
                nonfinite=int(((fl & _lib.RR_EVAL_NONFINITE) != 0).sum()), both_episodes=int((ep == NE).sum()))


def _assert_coverage(ref, what):
    c = _counts(ref)
    print("ends of handle A (%s): %s" % (what, c))
    assert c["event_landed"] >= 1      # a ground event with the landing bit
    assert c["event_not_landed"] >= 1  # a ground event without it
    assert c["trunc"] >= 1             # a TimeLimit truncation
    assert c["both_episodes"] >= 1     # an env that went through the in-kernel auto-reset and finished again
    return c


@pytest.mark.parametrize("n", [300, 37])  # 300: two workgroups, a ragged 44-env wave, three dead waves; 37: one partial wave
@pytest.mark.parametrize("model,prec", [(6, "fp32"), (6, "fp16x3"), (6, "bf16"), (3, "fp32")])
def test_evaluate_exact_bitwise_equals_policy_act_plus_step(model, prec, n):
    """Every output row, the episode counts, and both state images / v0 / counter word / running
    return / obs row B is left with, against handle A stepped 40 times. At n = 300 the reference
    itself must hold every way an episode ends here."""
    ref = _reference(model, prec, n)
    if n == 300:
        _assert_coverage(ref, "%dDOF, %s" % (model, prec))
    b, ev, res = _evaluate(model, prec, n)
    _compare(b, res, ref)
    assert res.stats()["episodes"] == int(ref["episodes"].sum())
    b.close()


def test_a_non_finite_env_ends_nonfinite_and_leaves_the_others_alone():
    """Env NAN_ENV starts with a NaN velocity component: the solver stops it as status -1 at its first
    step (RR_EVAL_NONFINITE), it is reset and runs on. B equals A on every env (NaNs in the same
    places), and A's other envs are bit for bit those of the reference without the NaN."""
    import torch
    from rl_rocket_amd import _lib

    ref = _reference(6, "fp32", 300, "nan")
    plain = _reference(6, "fp32", 300)
    assert int(ref["flags"][0, NAN_ENV]) & _lib.RR_EVAL_NONFINITE and int(ref["len"][0, NAN_ENV]) == 1
    assert _counts(ref)["nonfinite"] == 1 and _counts(plain)["nonfinite"] == 0
    others = torch.arange(300, device=DEV) != NAN_ENV
    for k in ("ret", "len", "flags", "fin", "mass", "episodes"):
        assert torch.equal(ref[k][..., others], plain[k][..., others]), k
    for x, y in zip(ref["last"][:5], plain["last"][:5]):
        assert torch.equal(x[..., others], y[..., others])
    assert torch.equal(ref["last"][5][others], plain["last"][5][others])
    b, ev, res = _evaluate(6, "fp32", 300, "nan")
    _compare(b, res, ref, eq=_same)
    assert int(res.flags[0, NAN_ENV]) & _lib.RR_EVAL_NONFINITE
    for name, k in (("ep_return", "ret"), ("ep_length", "len"), ("flags", "flags"), ("final_state", "fin"),
                    ("used_mass", "mass"), ("episodes", "episodes")):
        assert torch.equal(getattr(res, name)[..., others], plain[k][..., others]), name
    for x, y in zip(_aux(b), plain["last"][:5]):
        assert torch.equal(x[..., others], y[..., others])
    assert res.stats()["n_nonfinite"] == 1
    b.close()


@pytest.mark.parametrize("flag", ["reward_annealing", "scipy_h0_clamp"])
def test_reward_annealing_and_h0_clamp(flag):
    ref = _reference(6, "fp32", 300, "landing", ((flag, True),))
    base = _reference(6, "fp32", 300)
    import torch

    if flag == "reward_annealing":  # the flag is live: another reward
        assert not torch.equal(ref["ret"], base["ret"])
    b, ev, res = _evaluate(6, "fp32", 300, **{flag: True})
    _compare(b, res, ref)
    b.close()


def test_max_steps_cap_leaves_rows_untouched():
    """3DOF without the fixture, max_steps below the first done of A: no env finishes, no row is
    written, and B's state is A's after that many steps."""
    import torch

    ref = _reference(3, "fp32", 300, None)
    cap = min(ref["first_done"] - 1, 7)
    assert cap >= 2
    b, ev, res = _evaluate(3, "fp32", 300, None, max_steps=cap)
    assert torch.equal(res.episodes, torch.zeros_like(res.episodes))
    for t, v in ((res.ep_return, SENT), (res.ep_length, -7), (res.flags, 0xEE), (res.used_mass, SENT),
                 (res.final_state, SENT)):
        assert torch.equal(t, torch.full_like(t, v))
    snap = ref["kept"][cap]
    for got, want in zip(_aux(b), snap):
        assert torch.equal(got, want)
    assert torch.equal(b.obs, snap[5])
    s = res.stats()
    assert s["episodes"] == 0 and s["unfinished"] == NE * 300
    b.close()


def test_graph_replay_equals_eager():
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = _batch(6, 300)
    st0 = [t.clone() for t in b.get_state64()[:2]]
    ck = b.checkpoint()

    def rewind():
        b.restore(ck)
        b.set_state64(st0[0], v0=st0[1], elapsed=ck["counter"])

    ev = PolicyEvaluator(b, _policy(6), n_episodes=NE, max_steps=NE * TL, fused=True)
    res = ev.run()
    torch.cuda.synchronize()
    eager = {k: getattr(res, k).clone() for k in NAMES}
    eager_state = [t.clone() for t in _aux(b)]
    eager_obs = b.obs.clone()
    assert int(res.episodes.max()) == NE
    rewind()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ev.run()
    torch.cuda.current_stream().wait_stream(s)
    rewind()
    for k in NAMES:
        getattr(res, k).fill_(0)
    b.obs.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(getattr(res, k), eager[k]), k
    for x, y in zip(_aux(b), eager_state):
        assert torch.equal(x, y)
    assert torch.equal(b.obs, eager_obs)
    b.close()


def test_argument_errors():
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout import PolicyEvaluator, PolicyPack

    lib = _lib.load()
    n = 64
    pol = _policy(6)
    params = PolicyPack(pol, 14, 3, torch.device(DEV)).pack()
    ep = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = _lib.RrEvalOut(episodes=ep.data_ptr())

    def call(b, n_episodes=1, max_steps=0, precision=0):
        return lib.rr_policy_evaluate_exact(b._h, _ptr(params), precision, n_episodes, max_steps, ctypes.byref(out),
                                            None, None)

    def refused(rc):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(b"rr_policy_evaluate_exact: ") and len(msg) > 36, msg
        return msg

    ok = _batch(6, n, None)
    assert b"rr_policy_evaluate" in refused(call(_batch(6, n, None, integrator="rk4"))).split(b": ", 1)[1]
    refused(call(_batch(6, n, None, auto_reset=False)))
    refused(call(ok, n_episodes=0))
    refused(call(ok, precision=7))
    refused(call(_batch(6, n, None, max_episode_steps=0), max_steps=0))
    with pytest.raises(ValueError):
        PolicyEvaluator(ok, pol, n_episodes=1, fused=True, record=[0])
    assert not PolicyEvaluator(ok, pol, n_episodes=1).fused  # the default of an exact-mode batch stays step by step
    assert call(ok) == 0  # the same call with nothing wrong: only `episodes` is written
    torch.cuda.synchronize()
    assert torch.equal(ep, torch.ones_like(ep))


def test_fused_equals_unfused_with_a_constant_mean():
    """With the action head's weight zeroed the mean is the bias whatever the tower arithmetic and
    whatever obs the tower reads, so the one-launch kernel and the PyTorch-op path (fused=False, two
    exact steps per iteration) agree on every output bit and leave the handle in the same state.
    batch.obs is the exception by construction: the step-by-step path ends with rr_reset's obs
    (state * inv_norm in fp32), the kernel writes the exact mode's float32(state64 / norm), which
    is checked against that formula instead."""
    import torch

    pol = _policy(6, zero_head=True)
    outs = []
    for fused in (True, False):
        b, ev, res = _evaluate(6, "fp32", 300, fused=fused, policy=pol)
        outs.append((b, res))
    (b0, r0), (b1, r1) = outs
    assert int(r0.episodes.max()) == NE and int(r0.episodes.sum()) > 300
    for name in NAMES:
        assert torch.equal(getattr(r0, name), getattr(r1, name)), name
    for x, y in zip(_aux(b0), _aux(b1)):
        assert torch.equal(x, y)
    assert torch.equal(b0.obs, _exact_obs(b0))
    b0.close()
    b1.close()


def test_evaluate_policy_passes_fused_through():
    """evaluate_policy(..., fused=True) on an exact-mode batch: the episodes of the one-launch call."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator, evaluate_policy

    pol = _policy(6)
    rewards, lengths = evaluate_policy(pol, _batch(6, 64, None), n_eval_episodes=1, return_episode_rewards=True,
                                       fused=True)
    twin = _batch(6, 64, None)
    twin.reset()  # evaluate_policy resets the batch it is given once more
    res = PolicyEvaluator(twin, pol, n_episodes=1, fused=True).run()
    torch.cuda.synchronize()
    assert len(rewards) == 64 and rewards == res.ep_return[0].cpu().tolist()
    assert lengths == res.ep_length[0].cpu().tolist() and max(lengths) <= TL
    twin.close()
