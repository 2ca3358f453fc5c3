"""rr_policy_evaluate_exact_discrete (PolicyEvaluator(dopri5_batch, categorical_policy, fused=True): whole
deterministic episodes of the Categorical policy under the exact integrator in one launch).

The set-up is tests/test_gpu_eval_exact.py's: 3DOF, integrator="dopri5", TimeLimit 20, 2 episodes (40
steps), compute_terms, seed 1234, its landing fixture (envs 0..95 2 cm above the pad at 0.5 / 5 / 50 m/s,
the rest from the reset), sentinel-filled outputs, n = 300 (two workgroups, a ragged 44-env wave, three dead
waves) and n = 37 (one partial wave).

E1, constant logits: with the action head's weight zeroed the logits are the biases whatever the tower
arithmetic, so the one launch and the step-by-step path (fused=False) agree on every bit.
E3, the contract: bitwise against rr_policy_act_discrete + rr_step with the head scaled by 1e6, where the
softmax is saturated and the sampled index is the argmax (see _reference).
E2: against fused=False with the unscaled policy, off the knife edge."""
import ctypes
import functools

import numpy as np
import pytest

from test_eval_exact_discrete_host import E3_CASES, E3_GAP, E3_SCALE, scaled_cat_policy
from test_gpu_eval_exact import (DEV, NAMES, NAN_ENV, NE, SENT, TL, _assert_coverage, _aux, _batch, _compare, _counts,
                                 _evaluate, _exact_obs, _flags, _same)

pytestmark = pytest.mark.gpu

KNIFE_CAP = 0.05  # of the envs: tests/test_gpu_eval_discrete.py's


def _row(index, hi=1.0, lo=-1.0, k=4):
    return tuple(hi if q == index else lo for q in range(k))


def _constant(k, biases):
    """A K-choice policy whose logits are `biases` for every observation."""
    import torch
    from discrete_ref import cat_policy

    pol = cat_policy(k, 100 + k)
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.copy_(torch.tensor(biases, dtype=torch.float32))
    return pol.to(DEV)


def _run(pol, n, fused, fixture="landing", max_steps=NE * TL, **over):
    """One evaluation into sentinel-filled outputs: (outputs cloned, state left, batch.obs, the exact
    mode's obs of the state left)."""
    b, ev, res = _evaluate(3, "fp32", n, fixture, max_steps=max_steps, fused=fused, policy=pol, **over)
    assert ev._exact == fused
    out = {name: getattr(res, name).clone() for name in NAMES}
    state = [t.clone() for t in _aux(b)]
    obs, want_obs = b.obs.clone(), _exact_obs(b)
    b.close()
    return out, state, obs, want_obs


@functools.lru_cache(maxsize=None)
def _fused_constant(k, biases, n):
    """The one-launch evaluation of a constant-logit policy, shared (never modified) by the E1 tests."""
    return _run(_constant(k, biases), n, True)


def _equal_runs(x, y, tag, ok=None):
    """Every output plane and the state left; batch.obs of the one-launch run `x` against the exact mode's
    formula (the step-by-step path ends with rr_reset's obs formula: tests/test_gpu_eval_exact.py)."""
    import torch

    sel = (lambda t: t) if ok is None else (lambda t: t[..., ok])
    for name in NAMES:
        assert torch.equal(sel(x[0][name]), sel(y[0][name])), (tag, name)
    for a, b in zip(x[1], y[1]):
        assert torch.equal(sel(a), sel(b)), tag
    assert torch.equal(x[2], x[3]), tag


# ---- E1 ----

E1_CASES = [(4, _row(0), 0), (4, _row(1), 1), (4, _row(2), 2), (4, _row(3), 3),
            (4, (0.5, 0.5, 0.5, 0.5), 0),      # all equal: index 0
            (4, (-1.0, 0.7, -1.0, 0.7), 1),    # a tie of 1 and 3 above the rest
            (2, (-3.0, -3.0), 0),              # a zero head >= K is larger than every real logit:
            (3, (-3.0, -3.0, -3.0), 0)]        # it must not win


@pytest.mark.parametrize("n", [300, 37])
@pytest.mark.parametrize("k,biases,winner", E1_CASES)
def test_constant_logits_fused_equals_unfused(k, biases, winner, n):
    """Bit for bit the step-by-step evaluator's outputs and state, and the launch took `winner`: its outputs
    are those of a K = 4 policy whose logit at `winner` is strictly the largest (the tables' rows 0 are the
    same row; row 1 is only asked for at K = 4). At n = 300 the step-by-step run itself holds every way an
    episode ends here."""
    want = _run(_constant(k, biases), n, False)
    if n == 300:
        _assert_coverage(dict(flags=want[0]["flags"], episodes=want[0]["episodes"]), "K %d, biases %s" % (k, biases))
    got = _fused_constant(k, biases, n)
    _equal_runs(got, want, "fused against unfused")
    _equal_runs(got, _fused_constant(4, _row(winner), n), "the winner")
    other = _fused_constant(4, _row(3 if winner == 1 else 1), n)
    assert not all(bool((got[0][name] == other[0][name]).all()) for name in NAMES)  # the comparison can tell


# ---- E3 ----

def _table(pol):
    return (ctypes.c_float * (2 * pol.n_choices))(*pol.table.reshape(-1).tolist())


@functools.lru_cache(maxsize=None)
def _reference(k, seed, n, fixture="landing", over=()):
    """Handle A: NE * TL times rr_policy_act_discrete + rr_step, read back after every step, as
    test_gpu_eval_exact._reference (a shadow handle without auto-reset supplies the un-reset terminal
    state; A's obs is overwritten with the exact mode's rows before the first act). The policy is
    scaled_cat_policy(k, seed, E3_SCALE). Where the two largest fp32 logits differ by 104 or more, every
    exp(z_k - m) of a loser is exactly 0 in fp32 (expf reaches 0 below -103.98, flushing comes earlier),
    the winner's probability is exactly 1 and the inverse-CDF index is the argmax for every draw u in
    [0, 1): so rr_policy_act_discrete hands rr_step the row the evaluation must take. "gap" is each env's
    smallest difference of the two largest float64 logits (discrete_ref.forward64 on A's obs) over the
    steps it took while evaluating, "took" the indices A took there. Never modified by the tests."""
    import torch
    from discrete_ref import forward64
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import RocketBatch, _ptr
    from rl_rocket_amd.rollout import PolicyPack

    over = dict(over)
    a = _batch(3, n, fixture, **over)
    sh = RocketBatch(n, model=3, device=DEV, max_episode_steps=0, auto_reset=False, episode_stats=False,
                     integrator="dopri5", compute_terms=True, **over)
    pol = scaled_cat_policy(k, seed, E3_SCALE).to(DEV)
    table = _table(pol)
    ns, nt = a.state_dim, a.n_terms
    el_mask = (1 << a.counter_bits) - 1
    pack = PolicyPack(pol, ns, k, a.device, precision="fp32")
    params = pack.pack()
    f = dict(dtype=torch.float32, device=DEV)
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    act_env, act = torch.zeros((n, 2), **f), torch.zeros(n, **f)
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
    gap = np.full(n, np.inf)
    took = np.zeros((n, 4), bool)
    for t in range(NE * TL):
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        _lib.check(lib.rr_policy_act_discrete(_ptr(params), ns, k, table, pack.prec, n, 0, _ptr(a.obs), 11, _ptr(it), t,
                                              _ptr(act_env), _ptr(act), _ptr(val), _ptr(lp), None, None, None, None,
                                              0.0, None, None, None, stream), "rr_policy_act_discrete")
        z = np.sort(forward64(pol, a.obs)[0], axis=1)
        evaluating = (ep < NE).cpu().numpy()
        d = z[:, -1] - z[:, -2]
        d = np.where(np.isnan(d), np.inf, d)  # NaN logits (the non-finite env's first step) are no knife edge
        gap = np.where(evaluating, np.minimum(gap, d), gap)
        took[np.arange(n)[evaluating], act.cpu().numpy().astype(np.int64)[evaluating]] = True
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
    ref.update(episodes=ep.to(torch.int32), last=last, kept=kept, first_done=first_done, gap=gap, took=took)
    a.close()
    sh.close()
    return ref


def _compared(ref, k, what, meaningful=True):
    """The envs E3 compares (a bool tensor): all but those whose two largest float64 logits came closer
    than E3_GAP (120: the 104 of _reference with margin, far above the towers' ~5e-6 x 1e6 error) at a step
    they took on handle A. At most KNIFE_CAP of the envs may be left out; at least a quarter of the compared
    ones must have taken two or more distinct indices, and every index below K must occur."""
    import torch

    gap, took = ref["gap"], ref["took"]
    out = gap < E3_GAP
    two = (took.sum(1) >= 2) & ~out
    print("E3 %s: %d envs of %d left out, %d of the %d compared take two or more indices, envs per index %s, "
          "smallest gap %.3g" % (what, int(out.sum()), len(gap), int(two.sum()), int((~out).sum()),
                                 took[~out].sum(0).tolist(), float(gap.min())))
    assert out.mean() <= KNIFE_CAP
    if meaningful:
        assert two.sum() >= (~out).sum() / 4
        assert took[~out].any(0)[:k].all()
    assert not took[:, k:].any()
    return torch.as_tensor(~out, device=DEV)


def _compare_on(ok, b, res, ref, snapshot=None, eq=None):
    """test_gpu_eval_exact._compare on the envs `ok`."""
    import torch

    eq = eq or torch.equal
    sub = dict(episodes=ref["episodes"][ok], len=ref["len"][:, ok], ret=ref["ret"][:, ok], flags=ref["flags"][:, ok],
               fin=ref["fin"][..., ok], mass=ref["mass"][:, ok])
    assert eq(res.episodes[ok], sub["episodes"])
    assert eq(res.ep_length[:, ok], sub["len"])
    assert eq(res.ep_return[:, ok], sub["ret"])
    assert eq(res.flags[:, ok], sub["flags"])
    assert eq(res.final_state[..., ok], sub["fin"])  # rows of unfinished episodes: the sentinel on both sides
    assert eq(res.used_mass[:, ok], sub["mass"])
    want = snapshot if snapshot is not None else ref["last"]
    for name, got, w in zip(("state", "v0", "counter", "ep_return", "state64"), _aux(b), want):
        assert eq(got[..., ok], w[..., ok]), name
    assert eq(b.obs[ok], want[5][ok])


def _e3_policy(k):
    seed = dict(E3_CASES)[k]
    return seed, scaled_cat_policy(k, seed, E3_SCALE).to(DEV)


@pytest.mark.parametrize("n", [300, 37])
@pytest.mark.parametrize("k", [4, 3, 2])
def test_evaluate_bitwise_equals_policy_act_discrete_plus_step(k, n):
    """E3. Every output row, the episode count, both state images / v0 / counter word / running return and
    the obs row of every compared env, against handle A stepped 40 times. The CPU oracle's figures for these
    cases are in tests/test_eval_exact_discrete_host.py. Measured on an MI355X (envs left out; compared
    envs with two or more indices), n = 300: K = 4, 6 and 115 of 294 (envs per index 72, 32, 293, 36); K = 3,
    6 and 124 of 294 (13, 281, 129); K = 2, 5 and 97 of 295 (103, 289). n = 37: K = 4, 1 and 10 of 36; K = 3, 0
    and 12 of 37; K = 2, 0 and 7 of 37 (the conditions on the indices are n = 300's: 37 envs, 32 of them on one
    fixture state, need not reach every index)."""
    seed, pol = _e3_policy(k)
    ref = _reference(k, seed, n)
    if n == 300:
        _assert_coverage(ref, "K %d" % k)
    ok = _compared(ref, k, "K %d seed %d n %d" % (k, seed, n), meaningful=n == 300)
    b, ev, res = _evaluate(3, "fp32", n, policy=pol)
    assert ev._exact
    _compare_on(ok, b, res, ref)
    b.close()


@pytest.mark.parametrize("flag", ["reward_annealing", "scipy_h0_clamp"])
def test_reward_annealing_and_h0_clamp(flag):
    import torch

    seed, pol = _e3_policy(4)
    ref = _reference(4, seed, 300, "landing", ((flag, True),))
    base = _reference(4, seed, 300)
    if flag == "reward_annealing":  # the flag is live: another reward (its thrust is the table row's)
        assert not torch.equal(ref["ret"], base["ret"])
    ok = _compared(ref, 4, flag)
    b, ev, res = _evaluate(3, "fp32", 300, policy=pol, **{flag: True})
    _compare_on(ok, b, res, ref)
    b.close()


def test_a_non_finite_env_ends_nonfinite_and_leaves_the_others_alone():
    """Env NAN_ENV starts with a NaN velocity component: the solver stops it as status -1 at its first step
    (RR_EVAL_NONFINITE), it is reset and runs on. All other envs are bit for bit those of the run without
    the NaN, on handle A and in the launch."""
    import torch
    from rl_rocket_amd import _lib

    seed, pol = _e3_policy(4)
    ref = _reference(4, seed, 300, "nan")
    plain = _reference(4, seed, 300)
    assert int(ref["flags"][0, NAN_ENV]) & _lib.RR_EVAL_NONFINITE and int(ref["len"][0, NAN_ENV]) == 1
    assert _counts(ref)["nonfinite"] == 1 and _counts(plain)["nonfinite"] == 0
    others = torch.arange(300, device=DEV) != NAN_ENV
    for key in ("ret", "len", "flags", "fin", "mass", "episodes"):
        assert torch.equal(ref[key][..., others], plain[key][..., others]), key
    for x, y in zip(ref["last"][:5], plain["last"][:5]):
        assert torch.equal(x[..., others], y[..., others])
    assert torch.equal(ref["last"][5][others], plain["last"][5][others])
    ok = _compared(ref, 4, "with a NaN env")
    assert bool(ok[NAN_ENV])  # its NaN logits are no knife edge: every compare of the head is false, index 0
    b, ev, res = _evaluate(3, "fp32", 300, "nan", policy=pol)
    _compare_on(ok, b, res, ref, eq=_same)
    assert int(res.flags[0, NAN_ENV]) & _lib.RR_EVAL_NONFINITE and int(res.ep_length[0, NAN_ENV]) == 1
    assert int(res.episodes[NAN_ENV]) == int(ref["episodes"][NAN_ENV]) >= 1
    b2, ev2, res2 = _evaluate(3, "fp32", 300, policy=pol)
    for name in NAMES:
        assert torch.equal(getattr(res, name)[..., others], getattr(res2, name)[..., others]), name
    for x, y in zip(_aux(b), _aux(b2)):
        assert torch.equal(x[..., others], y[..., others])
    assert res.stats()["n_nonfinite"] == 1
    b.close()
    b2.close()


def test_max_steps_cap_leaves_rows_untouched():
    """Without the fixture, max_steps below the first done of A: no env finishes, no row is written, and the
    state of the compared envs is A's after that many steps."""
    import torch

    seed, pol = _e3_policy(4)
    ref = _reference(4, seed, 300, None)
    cap = min(ref["first_done"] - 1, 7)
    assert cap >= 2
    ok = _compared(ref, 4, "without the fixture", meaningful=False)
    b, ev, res = _evaluate(3, "fp32", 300, None, max_steps=cap, policy=pol)
    assert torch.equal(res.episodes, torch.zeros_like(res.episodes))
    for t, v in ((res.ep_return, SENT), (res.ep_length, -7), (res.flags, 0xEE), (res.used_mass, SENT),
                 (res.final_state, SENT)):
        assert torch.equal(t, torch.full_like(t, v))
    snap = ref["kept"][cap]
    for got, want in zip(_aux(b), snap):
        assert torch.equal(got[..., ok], want[..., ok])
    assert torch.equal(b.obs[ok], snap[5][ok])
    s = res.stats()
    assert s["episodes"] == 0 and s["unfinished"] == NE * 300
    b.close()


# ---- E2 ----

def test_unscaled_policy_agrees_with_the_step_by_step_path_off_the_knife_edge():
    """The step-by-step path computes its logits in PyTorch and the unsaturated head picks the winner among
    near logits: an env is compared where its two largest float64 logits stay further apart than
    discrete_ref.KNIFE on every step it took, measured on a third twin stepped by hand with the argmax of a
    float64 copy of the policy. Measured on an MI355X: 4 knife-edge envs of 300, 120 envs take two or more
    indices, smallest gap 4.9e-5."""
    import torch
    from discrete_ref import KNIFE, forward64

    k, n = 4, 300
    pol = scaled_cat_policy(k, dict(E3_CASES)[k], 1.0).to(DEV)
    got = _run(pol, n, True)
    want = _run(pol, n, False)
    tw = _batch(3, n)
    table = pol.table
    ep = np.zeros(n, dtype=np.int64)
    gap = np.full(n, np.inf)
    took = np.zeros((n, 4), bool)
    obs = _exact_obs(tw)
    for _ in range(NE * TL):
        z = forward64(pol, obs)[0]
        top = np.sort(z, axis=1)
        idx = z.argmax(1)
        active = ep < NE
        gap = np.where(active, np.minimum(gap, top[:, -1] - top[:, -2]), gap)
        took[np.arange(n)[active], idx[active]] = True
        obs, _, done, _ = tw.step(table[torch.as_tensor(idx, device=DEV)])
        ep += (torch.as_tensor(active, device=DEV) & done.bool()).cpu().numpy()
    torch.cuda.synchronize()
    tw.close()
    knife = gap < KNIFE
    print("E2 K = %d: %d knife-edge envs of %d, %d envs take two or more indices, smallest gap %.3g"
          % (k, int(knife.sum()), n, int((took.sum(1) >= 2).sum()), float(gap.min())))
    assert knife.mean() <= KNIFE_CAP
    assert ((took.sum(1) >= 2) & ~knife).sum() >= n // 4, "the chosen index hardly ever changes: the case checks nothing"
    _equal_runs(got, want, "fused against unfused", ok=torch.as_tensor(~knife, device=DEV))


# ---- capture, arguments ----

def test_graph_replay_equals_eager():
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    seed, pol = _e3_policy(4)
    b = _batch(3, 300)
    st0 = [t.clone() for t in b.get_state64()[:2]]
    ck = b.checkpoint()

    def rewind():
        b.restore(ck)
        b.set_state64(st0[0], v0=st0[1], elapsed=ck["counter"])

    ev = PolicyEvaluator(b, pol, n_episodes=NE, max_steps=NE * TL, fused=True)
    assert ev._exact
    res = ev.run()
    torch.cuda.synchronize()
    eager = {name: getattr(res, name).clone() for name in NAMES}
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
    for name in NAMES:
        getattr(res, name).fill_(0)
    b.obs.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(getattr(res, name), eager[name]), name
    for x, y in zip(_aux(b), eager_state):
        assert torch.equal(x, y)
    assert torch.equal(b.obs, eager_obs)
    b.close()


def test_c_abi_argument_errors_on_real_handles():
    import torch
    from discrete_ref import TABLES
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import RocketBatch, _ptr
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import PolicyPack

    lib, n = _lib.load(), 64
    seed, pol = _e3_policy(4)
    params = PolicyPack(pol, 7, 4, torch.device(DEV)).pack()
    episodes = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    out = _lib.RrEvalOut(episodes.data_ptr(), None, None, None, None, None)
    name = "rr_policy_evaluate_exact_discrete"

    def table(k, bad=None):
        rows = [list(r) for r in TABLES[4]] + [[0.0, 0.0]]
        if bad is not None:
            rows[bad][0] = float("inf")
        return (ctypes.c_float * (2 * k))(*[v for r in rows[:k] for v in r])

    def call(env, k=4, tab=None, prec=0, ne=1, max_steps=0, p=None):
        return lib.rr_policy_evaluate_exact_discrete(env._h, _ptr(params) if p is None else p, k,
                                                     tab or table(min(k, 5)), prec, ne, max_steps, ctypes.byref(out),
                                                     None, None)

    def refused(rc, word):
        msg = lib.rr_last_error().decode()
        assert rc == _lib.RR_EINVAL and msg.startswith(name + ": ") and word in msg, (rc, msg)

    kw = dict(model=3, device=DEV, max_episode_steps=20, integrator="dopri5")
    ed = RocketBatch(n, **kw)
    e4 = RocketBatch(n, **dict(kw, integrator="rk4"))
    e6 = RocketBatch(n, **dict(kw, model=6, **ENV_CONFIG_6DOF))
    en = RocketBatch(n, **dict(kw, auto_reset=False))
    e0 = RocketBatch(n, **dict(kw, max_episode_steps=0))
    refused(call(e4), "rr_policy_evaluate_discrete")
    refused(call(e6), "6DOF")
    refused(call(en), "RR_FLAG_AUTO_RESET")
    refused(call(e0), "max_steps")
    refused(call(ed, k=5), "2 .. 4")
    refused(call(ed, tab=table(4, bad=1)), "finite")
    refused(call(ed, prec=_lib.RR_POLICY_BF16), "RR_POLICY_FP32")
    refused(call(ed, p=ctypes.c_void_p(params.data_ptr() + 4)), "16-B aligned")
    torch.cuda.synchronize()
    assert torch.equal(episodes, torch.full_like(episodes, -7))  # nothing was launched
    ed.reset()
    assert call(ed) == _lib.RR_OK, lib.rr_last_error()  # one valid call with only `episodes` set
    torch.cuda.synchronize()
    assert torch.equal(episodes, torch.ones_like(episodes))
    for e in (ed, e4, e6, en, e0):
        e.close()


def test_evaluate_policy_passes_fused_through():
    """evaluate_policy(..., fused=True) on an exact-mode batch: the rows of a twin PolicyEvaluator run."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator, evaluate_policy

    seed, pol = _e3_policy(4)
    rewards, lengths = evaluate_policy(pol, _batch(3, 64, None), n_eval_episodes=1, return_episode_rewards=True,
                                       fused=True)
    twin = _batch(3, 64, None)
    twin.reset()  # evaluate_policy resets the batch it is given once more
    ev = PolicyEvaluator(twin, pol, n_episodes=1, fused=True)
    assert ev._exact
    res = ev.run()
    torch.cuda.synchronize()
    assert len(rewards) == 64 and rewards == res.ep_return[0].cpu().tolist()
    assert lengths == res.ep_length[0].cpu().tolist() and max(lengths) <= TL
    twin.close()
