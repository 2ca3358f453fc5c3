"""rr_policy_evaluate_discrete (PolicyEvaluator(batch, categorical_policy, fused=True): whole
deterministic episodes in one launch, the action being the table row of the largest logit) against the
step-by-step evaluator (fused=False: PyTorch ops around rr_step), which never runs the kernel under test.

E1, constant logits: with the action head's weight zeroed the logits are the biases whatever the tower
arithmetic, so both paths must agree on every output bit, on the state they leave and on batch.obs.
E2, a choice that changes along the episode: the two paths compute their logits differently (MFMA
towers against torch.nn.Linear), so an env is compared only where the two largest float64 logits stay
further apart than discrete_ref.KNIFE on every step it took; the share of the others is capped."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TL, NE = 80, 2
SENT = -12345.0
NAMES = ("episodes", "ep_return", "ep_length", "flags", "used_mass", "final_state")
FILL = dict(episodes=-7, ep_return=SENT, ep_length=-7, flags=0xEE, used_mass=SENT, final_state=SENT)
KNIFE_CAP = 0.05  # of the envs (tests/test_rollout_discrete_host.py holds the CPU oracle to half of it)


def _batch(n, integrator="rk4", tl=TL, **over):
    from rl_rocket_amd.batch import RocketBatch

    args = dict(model=3, device=DEV, max_episode_steps=tl, compute_terms=True, seed=1234, integrator=integrator)
    args.update(over)
    b = RocketBatch(n, **args)
    b.reset()
    return b


def _aux(b):
    ck = b.checkpoint()
    return ck["state"], ck["v0"], ck["counter"], ck["ep_return"]


def _constant(k, biases):
    """A K-choice policy whose logits are `biases` for every observation."""
    import torch
    from discrete_ref import cat_policy

    pol = cat_policy(k, 100 + k)
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.copy_(torch.tensor(biases, dtype=torch.float32))
    return pol.to(DEV)


def _evaluate(pol, n, integrator="rk4", fused=True, tl=TL, max_steps=None):
    """One evaluation into sentinel-filled outputs: (batch, outputs cloned, state left, batch.obs)."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = _batch(n, integrator, tl)
    ev = PolicyEvaluator(b, pol, n_episodes=NE, max_steps=max_steps or NE * tl, fused=fused)
    assert ev.fused == fused
    for name in NAMES:
        getattr(ev, name).fill_(FILL[name])
    res = ev.run()
    torch.cuda.synchronize()
    out = {name: getattr(res, name).clone() for name in NAMES}
    state = [t.clone() for t in _aux(b)]
    obs = b.obs.clone()
    return b, ev, out, state, obs


@functools.lru_cache(maxsize=None)
def _fused(k, biases, n, integrator):
    """The fused evaluation of a constant-logit policy, shared (never modified) by the tests that compare
    against it."""
    b, _, out, state, obs = _evaluate(_constant(k, biases), n, integrator, True)
    b.close()
    return out, state, obs


def _equal(x, y, tag):
    import torch

    (ox, sx, bx), (oy, sy, by) = x, y
    for name in NAMES:
        assert torch.equal(ox[name], oy[name]), (tag, name)
    for a, b in zip(sx, sy):
        assert torch.equal(a, b), tag
    assert torch.equal(bx, by), tag


def _ends(out):
    from rl_rocket_amd import _lib

    fl = out["flags"].cpu().numpy().astype(np.int64)
    fl = fl[fl != 0xEE]
    return {name: int(((fl & bit) != 0).sum()) for name, bit in (("event", _lib.RR_EVAL_EVENT),
                                                                  ("bounds", _lib.RR_EVAL_BOUNDS),
                                                                  ("trunc", _lib.RR_EVAL_TRUNCATED))}


def _row(index, hi=1.0, lo=-1.0, k=4):
    return tuple(hi if q == index else lo for q in range(k))


# ---- E1 ----

@pytest.mark.parametrize("n,integrator", [(300, "rk4"), (37, "rk4"), (300, "euler"), (37, "euler")])
@pytest.mark.parametrize("index", [0, 1, 2, 3])
def test_constant_logits_fused_equals_unfused(index, n, integrator):
    """The maximum at each index in turn. On the CPU oracle (512 envs, 80 steps of a constant row) index 1
    of the default table (gimbal -1, full thrust) ends every episode on the ground or out of bounds, as do
    indices 0 (no gimbal, least thrust: the rocket falls) and 3, while index 2 (no gimbal, full thrust) runs
    every env into the TimeLimit: both kinds of end must occur where the oracle has them."""
    pol = _constant(4, _row(index))
    b, _, out, state, obs = _evaluate(pol, n, integrator, False)
    b.close()
    _equal(_fused(4, _row(index), n, integrator), (out, state, obs), "index %d" % index)
    assert int(out["episodes"].min()) == NE
    c = _ends(out)
    print("ends with index %d, n %d, %s: %s" % (index, n, integrator, c))
    if index == 2:
        assert c["trunc"] >= 1
    if index == 1:
        assert c["event"] + c["bounds"] >= 1


@pytest.mark.parametrize("n,integrator", [(300, "rk4"), (37, "euler")])
@pytest.mark.parametrize("k,biases,winner", [(4, (0.5, 0.5, 0.5, 0.5), 0),      # all equal: index 0
                                             (4, (-1.0, 0.7, -1.0, 0.7), 1),    # a tie of 1 and 3 above the rest
                                             (2, (-3.0, -3.0), 0),              # a zero head >= K is larger than
                                             (3, (-3.0, -3.0, -3.0), 0)])       # every real logit: it must not win
def test_ties_and_heads_past_k(k, biases, winner, n, integrator):
    """Both paths agree bit for bit, and the fused one took `winner`: its outputs are those of a K = 4 policy
    whose logit at `winner` is strictly the largest (the tables' rows 0 are the same row, and row 1 is only
    asked for at K = 4)."""
    b, _, out, state, obs = _evaluate(_constant(k, biases), n, integrator, False)
    b.close()
    got = _fused(k, biases, n, integrator)
    _equal(got, (out, state, obs), "fused against unfused")
    _equal(got, _fused(4, _row(winner), n, integrator), "the winner")
    other = _fused(4, _row(3 if winner == 1 else 1), n, integrator)
    assert not all(bool((got[0][name] == other[0][name]).all()) for name in NAMES)  # the comparison can tell


def test_max_steps_cap_leaves_rows_untouched():
    """Index 2 never ends an episode before the TimeLimit (80), so with max_steps = 50 no env finishes: no
    row is written, episodes is 0 everywhere, and the state is the step-by-step evaluator's after 50 steps."""
    import torch

    pol = _constant(4, _row(2))
    full = _fused(4, _row(2), 300, "rk4")[0]
    assert int(full["ep_length"].min()) > 50
    b, ev, out, state, obs = _evaluate(pol, 300, max_steps=50)
    assert torch.equal(out["episodes"], torch.zeros_like(out["episodes"]))
    for name in NAMES[1:]:
        assert torch.equal(out[name], torch.full_like(out[name], FILL[name])), name
    s = ev.result.stats()
    assert s["episodes"] == 0 and s["unfinished"] == NE * 300
    b.close()
    b2, _, out2, state2, obs2 = _evaluate(pol, 300, fused=False, max_steps=50)
    b2.close()
    for x, y in zip(state, state2):
        assert torch.equal(x, y)
    assert torch.equal(obs, obs2)


# ---- E2 ----

E2_TL, E2_N = 40, 300


@pytest.mark.parametrize("k,seed", [(4, 1), (3, 13), (3, 39)])
def test_changing_choice_agrees_off_the_knife_edge(k, seed):
    """The reference is the fused=False evaluator on a twin batch; a third twin is stepped by hand with the
    argmax of a float64 copy of the policy, which gives each env's smallest gap between its two largest
    logits and a return and length of its own. Measured on an MI355X, knife-edge envs of 300: K = 4 seed 1,
    4; K = 3 seed 13, 2; K = 3 seed 39, 2; the index changes within an episode in all 300 envs each time (the
    CPU oracle's figures are in tests/test_rollout_discrete_host.py)."""
    import torch
    from discrete_ref import KNIFE, cat_policy, forward64

    pol = cat_policy(k, seed).to(DEV)
    n = E2_N
    bf, _, fo, fs, fobs = _evaluate(pol, n, tl=E2_TL, fused=True)
    br, _, ro, rs, robs = _evaluate(pol, n, tl=E2_TL, fused=False)
    bf.close()
    br.close()
    # the third twin, stepped by hand with the argmax of a float64 copy of the policy
    tw = _batch(n, tl=E2_TL)
    table = pol.table
    ep = np.zeros(n, dtype=np.int64)
    gap = np.full(n, np.inf)
    changed = np.zeros(n, dtype=bool)
    prev = np.full(n, -1)
    h_ret = torch.full((NE, n), SENT, device=DEV)
    h_len = torch.full((NE, n), -7, dtype=torch.int32, device=DEV)
    obs = tw.obs
    for _ in range(NE * E2_TL):
        z = forward64(pol, obs)[0]
        top = np.sort(z, axis=1)
        idx = z.argmax(1)
        active = ep < NE
        gap = np.where(active, np.minimum(gap, top[:, -1] - top[:, -2]), gap)
        changed |= active & (prev >= 0) & (prev != idx)
        obs, _, done, _ = tw.step(table[torch.as_tensor(idx, device=DEV)])
        _, tret, tlen = tw.copy_terminal()
        end = torch.as_tensor(active, device=DEV) & done.bool()
        e_i = end.nonzero().squeeze(1)
        k_i = torch.as_tensor(ep, device=DEV)[e_i]
        h_ret[k_i, e_i] = tret[e_i]
        h_len[k_i, e_i] = tlen[e_i]
        end_h = end.cpu().numpy()
        ep += end_h
        prev = np.where(end_h, -1, idx)  # a change is counted inside an episode only
    torch.cuda.synchronize()
    tw.close()
    knife = gap < KNIFE
    print("E2 K = %d seed %d: %d knife-edge envs of %d, the index changes in %d envs, smallest gap %.3g"
          % (k, seed, int(knife.sum()), n, int(changed.sum()), float(gap.min())))
    assert knife.mean() <= KNIFE_CAP
    assert changed.sum() >= n // 2, "the chosen index hardly ever changes: the case checks nothing"
    assert int(ep.min()) == NE
    ok = torch.as_tensor(~knife, device=DEV)
    for name in NAMES:
        assert torch.equal(fo[name][..., ok], ro[name][..., ok]), name
    for x, y in zip(fs, rs):
        assert torch.equal(x[..., ok], y[..., ok])
    assert torch.equal(fobs[ok], robs[ok])
    assert torch.equal(h_ret[:, ok], fo["ep_return"][:, ok]) and torch.equal(h_len[:, ok], fo["ep_length"][:, ok])


# ---- capture, arguments ----

def test_graph_replay_equals_eager():
    import torch
    from discrete_ref import cat_policy
    from rl_rocket_amd.rollout import PolicyEvaluator

    pol = cat_policy(4, 1).to(DEV)
    b = _batch(300, tl=E2_TL)
    ck = b.checkpoint()
    ev = PolicyEvaluator(b, pol, n_episodes=NE, fused=True)
    res = ev.run()
    torch.cuda.synchronize()
    eager = {name: getattr(res, name).clone() for name in NAMES}
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
    assert int(res.episodes.min()) == NE
    b.close()


def test_evaluate_policy_passes_fused_through():
    import math

    from discrete_ref import cat_policy
    from rl_rocket_amd.rollout import evaluate_policy

    b = _batch(300, tl=E2_TL)
    mean, std = evaluate_policy(cat_policy(4, 1).to(DEV), b, n_eval_episodes=NE, fused=True)
    assert math.isfinite(mean) and std > 0.0
    b.close()


def test_c_abi_argument_errors():
    import torch
    from discrete_ref import TABLES, cat_policy
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import RocketBatch, _ptr
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import PolicyPack

    lib, n = _lib.load(), 64
    params = PolicyPack(cat_policy(4, 104).to(DEV), 7, 4, torch.device(DEV)).pack()
    episodes = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = _lib.RrEvalOut(episodes.data_ptr(), None, None, None, None, None)
    name = "rr_policy_evaluate_discrete"

    def table(k, bad=None):
        rows = [list(r) for r in TABLES[4]] + [[0.0, 0.0]]
        if bad is not None:
            rows[bad][0] = float("inf")
        return (ctypes.c_float * (2 * k))(*[v for r in rows[:k] for v in r])

    def call(env, k=4, tab=None, prec=0, ne=1, max_steps=0, o=out, p=None):
        return lib.rr_policy_evaluate_discrete(env._h, _ptr(params) if p is None else p, k, tab or table(min(k, 5)),
                                               prec, ne, max_steps, ctypes.byref(o) if o is not None else None, None,
                                               None)

    def refused(rc, word):
        msg = lib.rr_last_error().decode()
        assert rc == _lib.RR_EINVAL and msg.startswith(name) and word in msg, (rc, msg)

    e3 = RocketBatch(n, model=3, device=DEV, max_episode_steps=20)
    e6 = RocketBatch(n, model=6, device=DEV, max_episode_steps=20, **ENV_CONFIG_6DOF)
    ed = RocketBatch(n, model=3, device=DEV, max_episode_steps=20, integrator="dopri5")
    en = RocketBatch(n, model=3, device=DEV, max_episode_steps=20, auto_reset=False)
    e0 = RocketBatch(n, model=3, device=DEV, max_episode_steps=0)
    refused(call(e6), "6DOF")
    refused(call(ed), "RR_INT_DOPRI5")
    refused(call(e3, k=5), "2 .. 4")
    refused(call(e3, tab=table(4, bad=1)), "finite")
    refused(call(e3, prec=_lib.RR_POLICY_BF16), "RR_POLICY_FP32")
    refused(call(e3, prec=_lib.RR_POLICY_FP16X3), "RR_POLICY_FP32")
    refused(call(e3, p=ctypes.c_void_p(params.data_ptr() + 4)), "16-B aligned")
    refused(call(e3, ne=0), "n_episodes")
    refused(call(e3, o=None), "out")
    refused(call(e3, o=_lib.RrEvalOut()), "episodes")
    refused(call(en), "RR_FLAG_AUTO_RESET")
    refused(call(e0), "max_steps")
    for e in (e3, e0):  # rows past n_choices are not read; an env without a TimeLimit takes max_steps
        e.reset()
        assert call(e, k=3, tab=table(4, bad=3), max_steps=5) == _lib.RR_OK, lib.rr_last_error()
    torch.cuda.synchronize()
    assert int(episodes.max()) <= 1
    for e in (e3, e6, ed, en, e0):
        e.close()
