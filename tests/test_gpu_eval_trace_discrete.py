"""rr_policy_evaluate_discrete_trace (PolicyEvaluator(batch, categorical_policy, record=ids, fused=True):
whole deterministic episodes in one launch, recording the chosen envs' states, table rows, reward terms and
the index of every choice) with the recipes of tests/test_gpu_eval_discrete.py: TimeLimit 80, 2 episodes per
env, sentinel-filled outputs, and the step-by-step evaluator (fused=False), which never runs the kernel under
test, as the recorder to compare with.

Recording must not disturb the evaluation (against the fused plain run, bit for bit). With constant logits
(E1) both recorders must agree on every recorded bit. With a choice that changes along the episode (E2) the two
paths compute their logits differently, so an env is compared only where the two largest float64 logits stay
further apart than discrete_ref.KNIFE on every step either path recorded for it; the share of the others is
capped by that file's KNIFE_CAP. Whatever the path and the env, action == table[choice] bit for bit."""
import functools

import numpy as np
import pytest

import test_gpu_eval_discrete as D

pytestmark = pytest.mark.gpu

DEV, TL, NE, SENT, NAMES = D.DEV, D.TL, D.NE, D.SENT, D.NAMES
LSENT, CSENT = -7, -9
# n = 300: both ends of the batch, both ends of a wave, the second workgroup, the ragged 44-env wave, unsorted.
# n = 37: one partial wave
RECORD = {300: (299, 0, 63, 64, 256, 270, 17), 37: (36, 0, 20)}
PLANES = ("state", "action", "terms", "length", "choice")


def _record(pol, n, integrator="rk4", fused=True, tl=TL, max_steps=None, record=None, record_steps=None):
    """One recording evaluation into sentinel-filled buffers: (batch, evaluator, result), synchronised."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = D._batch(n, integrator, tl)
    ev = PolicyEvaluator(b, pol, n_episodes=NE, max_steps=max_steps or NE * tl, fused=fused,
                         record=RECORD[n] if record is None else record, record_steps=record_steps)
    assert ev.fused == fused and ev.trace.choice.dtype == torch.int32
    for name in NAMES:
        getattr(ev, name).fill_(D.FILL[name])
    tr = ev.trace
    for t, v in ((tr.state, SENT), (tr.action, SENT), (tr.terms, SENT), (tr.length, LSENT), (tr.choice, CSENT)):
        t.fill_(v)
    res = ev.run()
    torch.cuda.synchronize()
    return b, ev, res


def _planes(tr):
    return {k: getattr(tr, k).clone() for k in PLANES}


def _written(tr):
    """[K, ne, S] bool: the step rows the record owns (t < min(length, S) of an episode that was started)."""
    import torch

    S = tr.steps
    length = tr.length.T.long()  # [K, ne]
    return (length != LSENT)[:, :, None] & (torch.arange(S, device=DEV)[None, None, :] < length[:, :, None])


def _table_rows_match(tr, pol):
    """action == table[choice] on every written row, bit for bit; choice in [0, K); sentinels elsewhere."""
    import torch

    w = _written(tr)
    ch = tr.choice[w].long()
    assert int(ch.min()) >= 0 and int(ch.max()) < pol.n_choices
    assert torch.equal(tr.action[w], pol.table.to(DEV)[ch])
    assert torch.equal(tr.choice[~w], torch.full_like(tr.choice[~w], CSENT))
    assert torch.equal(tr.action[~w], torch.full_like(tr.action[~w], SENT))
    return w


# ---- recording does not disturb the evaluation ----

@pytest.mark.parametrize("n,integrator", [(300, "rk4"), (37, "rk4"), (300, "euler"), (37, "euler")])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_recording_does_not_disturb_the_evaluation(k, n, integrator):
    import torch
    from discrete_ref import cat_policy

    pol = cat_policy(k, 100 + k).to(DEV)
    b, ev, res = _record(pol, n, integrator)
    out = {name: getattr(res, name).clone() for name in NAMES}
    got = (out, [t.clone() for t in D._aux(b)], b.obs.clone())
    b.close()
    c, ev2, pout, pstate, pobs = D._evaluate(pol, n, integrator, True)
    assert ev2.trace is None
    c.close()
    D._equal(got, (pout, pstate, pobs), "recorded against plain")
    assert int(out["episodes"].min()) == NE
    tr = res.trace
    assert tr.env_ids.tolist() == list(RECORD[n])
    assert torch.equal(tr.length, out["ep_length"][:, tr.env_ids])
    _table_rows_match(tr, pol)


# ---- E1 ----

@functools.lru_cache(maxsize=None)
def _e1(index, n, integrator, fused):
    """Every env recorded under the constant-logit policy whose maximum is at `index`; never modified."""
    pol = D._constant(4, D._row(index))
    b, _, res = _record(pol, n, integrator, fused, record=tuple(range(n)))
    b.close()
    return _planes(res.trace), {name: getattr(res, name).clone() for name in NAMES}


@pytest.mark.parametrize("n,integrator", [(300, "rk4"), (37, "rk4"), (300, "euler"), (37, "euler")])
@pytest.mark.parametrize("index", [0, 1, 2, 3])
def test_constant_logits_fused_recorder_equals_unfused(index, n, integrator):
    import torch

    f, fo = _e1(index, n, integrator, True)
    u, uo = _e1(index, n, integrator, False)
    for name in NAMES:
        assert torch.equal(fo[name], uo[name]), name
    for k in PLANES:
        x, y = f[k], u[k]
        if x.is_floating_point():
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k
    length = f["length"].T.long()  # [K, ne]
    assert int(length.min()) >= 1 and int(fo["episodes"].min()) == NE
    w = torch.arange(TL, device=DEV)[None, None, :] < length[:, :, None]
    assert torch.equal(f["choice"][w], torch.full_like(f["choice"][w], index))  # the index everywhere ...
    assert bool((~w).any()) or index == 2
    assert torch.equal(f["choice"][~w], torch.full_like(f["choice"][~w], CSENT))  # ... and nothing past the length
    for k, past in (("action", ~w), ("terms", ~w)):
        assert torch.equal(f[k][past], torch.full_like(f[k][past], SENT)), k
    ws = torch.arange(TL + 1, device=DEV)[None, None, :] <= length[:, :, None]
    assert torch.equal(f["state"][~ws], torch.full_like(f["state"][~ws], SENT))
    assert not bool((f["state"][ws] == SENT).any())


# ---- ties and heads past K ----

@pytest.mark.parametrize("n,integrator", [(300, "rk4"), (37, "euler")])
@pytest.mark.parametrize("k,biases,winner", [(4, (0.5, 0.5, 0.5, 0.5), 0), (4, (-1.0, 0.7, -1.0, 0.7), 1),
                                             (2, (-3.0, -3.0), 0), (3, (-3.0, -3.0, -3.0), 0)])
def test_ties_and_heads_past_k(k, biases, winner, n, integrator):
    """The bias sets of tests/test_gpu_eval_discrete.py: a tie goes to the lowest index, and a zero-packed head
    >= K, larger than every real logit, is never recorded."""
    import torch

    pol = D._constant(k, biases)
    b, _, res = _record(pol, n, integrator)
    b.close()
    tr = res.trace
    w = _table_rows_match(tr, pol)
    assert int(w.sum()) >= NE * len(RECORD[n])
    assert torch.equal(tr.choice[w], torch.full_like(tr.choice[w], winner))
    assert int(tr.choice[w].max()) < k


# ---- E2 ----

E2_TL, E2_N = 40, 300


def _logits64(pol, tr, batch_cfg):
    """float64 logits of every recorded step's observation (the recorded state row times the float32
    reciprocal normaliser: bitwise what the policy was given), the written mask, gap and argmax."""
    import torch
    from discrete_ref import forward64

    w = _written(tr)
    inv = torch.tensor((1.0 / np.asarray(batch_cfg.state_normalizer, dtype=np.float64)).astype(np.float32),
                       device=DEV)[:7]
    obs = tr.state[:, :, :tr.steps][w] * inv
    z = forward64(pol, obs)[0]
    top = np.sort(z, axis=1)
    return w, top[:, -1] - top[:, -2], z.argmax(1)


@pytest.mark.parametrize("k,seed", [(4, 1), (3, 13), (3, 39)])
def test_changing_choice_agrees_off_the_knife_edge(k, seed):
    """Every env recorded on both paths. An env is knife-edge when, on a step either path recorded for it, the
    two largest float64 logits come within KNIFE of each other. On record (tests/test_gpu_eval_discrete.py,
    tests/test_rollout_discrete_host.py): 4, 2 and 2 of 300 on an MI355X; 9 of 1024, 4 of 512 and 3 of 512 on
    the CPU oracle."""
    import torch
    from discrete_ref import KNIFE, cat_policy

    pol = cat_policy(k, seed).to(DEV)
    n, rec = E2_N, tuple(range(E2_N))
    bf, _, rf = _record(pol, n, tl=E2_TL, fused=True, record=rec)
    cfg = bf.cfg
    bf.close()
    bu, _, ru = _record(pol, n, tl=E2_TL, fused=False, record=rec)
    bu.close()
    knife = np.zeros(n, dtype=bool)
    for tr in (rf.trace, ru.trace):
        w = _table_rows_match(tr, pol)  # for every recorded step of every env, knife-edge or not
        _, gap, arg = _logits64(pol, tr, cfg)
        env_of = torch.arange(n, device=DEV)[:, None, None].expand_as(w)[w].cpu().numpy()
        knife[env_of[gap < KNIFE]] = True
        off = gap >= KNIFE
        assert np.array_equal(tr.choice[w].cpu().numpy()[off], arg[off])  # off the knife edge: the float64 argmax
    changed = ((rf.trace.choice[:, :, 1:] != rf.trace.choice[:, :, :-1]) & _written(rf.trace)[:, :, 1:]).any(2).any(1)
    print("E2 recorded, K = %d seed %d: %d knife-edge envs of %d, the index changes in %d envs"
          % (k, seed, int(knife.sum()), n, int(changed.sum())))
    assert knife.mean() <= D.KNIFE_CAP
    assert int(changed.sum()) >= n // 2, "the chosen index hardly ever changes: the case checks nothing"
    assert int(rf.episodes.min()) == NE
    ok = torch.as_tensor(~knife, device=DEV)
    for name in PLANES:
        x, y = getattr(rf.trace, name), getattr(ru.trace, name)
        if name == "length":
            x, y = x.T, y.T
        if x.is_floating_point():
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x[ok], y[ok]), name
    for name in NAMES:
        assert torch.equal(getattr(rf, name)[..., ok], getattr(ru, name)[..., ok]), name


# ---- capacity, max_steps ----

def test_capacity_clips_rows_and_keeps_counting():
    """record_steps = 10 under TimeLimit 80 (no 3DOF episode of these settings is that short): rows 0 .. 10 of
    the states and 0 .. 9 of the other planes are the full record's, length reports the full count and
    episode() raises without clipped=True."""
    import torch
    from discrete_ref import cat_policy

    pol = cat_policy(4, 104).to(DEV)
    b, _, full = _record(pol, 300)
    b.close()
    b, ev, res = _record(pol, 300, record_steps=10)
    b.close()
    tr, ft = res.trace, full.trace
    assert tr.steps == 10 and tr.choice.shape == (len(RECORD[300]), NE, 10)
    assert torch.equal(tr.length, ft.length) and int(tr.length.min()) > 10
    assert torch.equal(tr.state, ft.state[:, :, :11]) and torch.equal(tr.action, ft.action[:, :, :10])
    assert torch.equal(tr.terms, ft.terms[:, :, :10]) and torch.equal(tr.choice, ft.choice[:, :, :10])
    assert int(tr.choice.min()) >= 0  # every row written, none past the plane
    for name in NAMES:
        assert torch.equal(getattr(res, name), getattr(full, name)), name
    with pytest.raises(ValueError, match="clipped=True"):
        tr.episode(RECORD[300][0], 0)
    rec = tr.episode(RECORD[300][0], 0, clipped=True)
    assert len(rec) == 10 and not rec.complete and rec.choices.tolist() == tr.choice[0, 0].tolist()


def test_max_steps_below_the_first_ending_writes_partial_lengths():
    """Index 2 (no gimbal, full thrust) never ends an episode before the TimeLimit, so with max_steps = 50 no
    env finishes: length[0] is 50, length[1] keeps its sentinel, 50 rows of episode 0 are written."""
    import torch

    pol = D._constant(4, D._row(2))
    b, ev, res = _record(pol, 300, max_steps=50)
    b.close()
    tr = res.trace
    assert torch.equal(res.episodes, torch.zeros_like(res.episodes))
    assert torch.equal(tr.length[0], torch.full_like(tr.length[0], 50))
    assert torch.equal(tr.length[1], torch.full_like(tr.length[1], LSENT))
    assert torch.equal(tr.choice[:, 0, :50], torch.full_like(tr.choice[:, 0, :50], 2))
    assert torch.equal(tr.choice[:, 0, 50:], torch.full_like(tr.choice[:, 0, 50:], CSENT))
    assert torch.equal(tr.choice[:, 1], torch.full_like(tr.choice[:, 1], CSENT))
    _table_rows_match(tr, pol)
    with pytest.raises(ValueError, match="partial=True"):
        tr.episode(RECORD[300][1], 0)
    rec = tr.episode(RECORD[300][1], 0, partial=True)
    assert len(rec) == 50 and not rec.complete and rec.choices.tolist() == [2] * 50


# ---- capture ----

def test_graph_replay_equals_eager():
    import torch
    from discrete_ref import cat_policy
    from rl_rocket_amd.rollout import PolicyEvaluator

    pol = cat_policy(4, 1).to(DEV)
    b = D._batch(300, tl=E2_TL)
    ck = b.checkpoint()
    ev = PolicyEvaluator(b, pol, n_episodes=NE, fused=True, record=RECORD[300])
    res = ev.run()
    torch.cuda.synchronize()
    eager = {name: getattr(res, name).clone() for name in NAMES}
    eager_tr = _planes(res.trace)
    eager_state = [t.clone() for t in D._aux(b)]
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
    for k in PLANES:
        getattr(res.trace, k).fill_(0)
    b.obs.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(getattr(res, name), eager[name]), name
    # rows past an episode's length are not written: compare what the record owns
    w = _written(res.trace)
    assert torch.equal(res.trace.length, eager_tr["length"])
    for k in ("action", "terms", "choice"):
        assert torch.equal(getattr(res.trace, k)[w], eager_tr[k][w]), k
    ws = torch.cat([w[:, :, :1], w], dim=2)  # state row 0 and the row after every written step
    assert torch.equal(res.trace.state[ws], eager_tr["state"][ws])
    for x, y in zip(D._aux(b), eager_state):
        assert torch.equal(x, y)
    assert torch.equal(b.obs, eager_obs)
    assert int(res.episodes.min()) == NE
    b.close()


# ---- demonstrations ----

def test_demonstrations_from_a_recorded_run_feed_bc_update():
    import torch
    from discrete_ref import cat_policy
    from rl_rocket_amd.bc import _check_indices
    from rl_rocket_amd.rollout import BCUpdate, Demonstrations

    pol = cat_policy(4, 1).to(DEV)
    b, ev, res = _record(pol, 300, tl=E2_TL)
    tr = res.trace
    demos = Demonstrations.from_trace(tr, b)
    w = _written(tr)
    assert int(tr.length.max()) <= tr.steps and int(res.episodes.min()) == NE  # every episode finished, unclipped
    assert demos.acts.shape == (int(w.sum()), 1) and demos.acts.dtype == torch.float32
    assert torch.equal(demos.acts[:, 0], tr.choice[w].float())  # slot, episode, step order: the mask's
    _check_indices(demos.acts, 4)
    inv = torch.tensor((1.0 / np.asarray(b.cfg.state_normalizer, dtype=np.float64)).astype(np.float32), device=DEV)[:7]
    assert torch.equal(demos.obs, tr.state[:, :, :tr.steps][w] * inv)
    b.close()
    student = cat_policy(4, 7).to(DEV)
    opt = torch.optim.Adam(student.parameters(), lr=1e-3, capturable=True)
    bs = min(256, len(demos))
    step = BCUpdate(student, opt, demos, bs)
    before = [p.detach().clone() for p in student.parameters()]
    stats = step(torch.arange(bs, device=DEV))
    torch.cuda.synchronize()
    s = step.last_stats()
    assert stats is step.stats and np.isfinite(list(s.values())).all() and s["neglogp"] > 0.0
    assert any(not torch.equal(x, y) for x, y in zip(before, student.parameters()))
