"""rr_policy_evaluate_exact_trace (the one-launch exact-mode evaluation that records whole episodes)
against the per-step path, with the fixture, shapes and helpers of test_gpu_eval_exact.py.

The bitwise reference is that file's handle-A / shadow loop: rr_policy_act at log_std = -60 +
rr_step on handle A, NE * TL times, a shadow handle without auto-reset taking each step from the same
fp64 state for the un-reset terminal state. Besides what that loop keeps (the rr_eval_out rows and the
snapshots of the handle after every step), this one keeps every step's y1.float() (the shadow's
state), act_env (the clipped mean), terms[:nt] and reward of every env. `_expected` replays those
rows through the recording contract stated at rr_policy_evaluate_trace (rocket_hip.h) on the host:
slots, t counted from the call, capacity clipping, partial lengths, sentinel everywhere else.
Handle B is evaluated once into sentinel-filled outputs and trace buffers; everything must agree bit
for bit."""
import ctypes
import functools

import pytest

from test_gpu_eval_exact import (DEV, NAMES, NAN_ENV, NE, SENT, TL, _aux, _batch, _compare, _exact_obs, _flags, _kw,
                                 _policy, _same)

pytestmark = pytest.mark.gpu

LSENT = -7  # pre-fill of the int32 planes
# recorded envs in a permuted slot order. 300: the first and the last env, one of each fixture class
# (0..31, 32..63, 64..95), both sides of the workgroup edge (255 | 256), NAN_ENV and the ragged last
# wave (256..299); every wave keeps unrecorded lanes. 37: one partial wave.
IDS = {300: (299, 0, 40, 70, 130, 256, 257, 200), 37: (36, 0, 33, 5)}
assert NAN_ENV in IDS[300]


@functools.lru_cache(maxsize=None)
def _reference(model, prec, n, fixture="landing", over=()):
    """test_gpu_eval_exact._reference's loop, which also keeps the per-step rows of every env: y1
    [T, ns, n] (float32 of the shadow's fp64 state), act [T, n, na], terms [T, nt, n], rew [T, n], done
    [T, n] and the fp32 cast of the state at the call. Never modified by the tests that share it."""
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
    ref = dict(ret=torch.full((NE, n), SENT, **f), len=torch.full((NE, n), LSENT, dtype=torch.int32, device=DEV),
               flags=torch.full((NE, n), 0xEE, dtype=torch.uint8, device=DEV), fin=torch.full((NE, ns, n), SENT, **f),
               mass=torch.full((NE, n), SENT, **f))
    a.obs.copy_(_exact_obs(a))
    pre = _aux(a)
    m_first = pre[0][-1].clone()
    last = [t.clone() for t in pre] + [a.obs.clone()]
    kept = {0: [x.clone() for x in pre] + [a.obs.clone()]}
    steps = dict(y1=[], act=[], terms=[], rew=[], done=[])
    for t in range(NE * TL):
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        _lib.check(lib.rr_policy_act(_ptr(params), ns, na, pack.prec, n, 0, _ptr(a.obs), 11, _ptr(it), t, _ptr(act_env),
                                     _ptr(act), _ptr(val), _ptr(lp), None, None, None, None, 0.0, None, None, None,
                                     stream), "rr_policy_act")
        # the un-reset state after the step: the same step of the shadow handle
        sh.set_state64(pre[4], v0=pre[1], elapsed=pre[2] & el_mask)
        sh.step(act_env)
        y1 = sh.get_state64()[0].float()
        _, rew, _, _ = a.step(act_env)
        _, tret, tlen = a.copy_terminal()
        snap = _aux(a)
        done, trunc, terms = a.done.bool(), a.truncated.bool(), a.terms
        fl = _flags((terms[nt + 1] > 0, terms[nt] > 0, trunc, terms[nt + 1] < 0, terms[nt - 1] != 0))
        for k, v in (("y1", y1), ("act", act_env), ("terms", terms[:nt]), ("rew", rew), ("done", done)):
            steps[k].append(v.clone())
        active = ep < NE  # evaluating at this step: the snapshot of the env follows A
        end = active & done
        e_i = end.nonzero().squeeze(1)
        k_i = ep[e_i]
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
    ref.update(episodes=ep.to(torch.int32), last=last, kept=kept)
    ref.update({k: torch.stack(v).cpu() for k, v in steps.items()})
    ref["start"] = torch.stack([kept[t][4].float().cpu() for t in range(NE * TL + 1)])  # [T + 1, ns, n]: float32(state64)
    a.close()
    sh.close()
    return ref


def _expected(ref, ids, cap=TL, max_steps=NE * TL):
    """The trace buffers the call must leave for the recorded envs `ids` (slot s = ids[s]), from the
    reference's per-step rows; everything it must not write holds the sentinel. Also each env's
    stop: the step after which the evaluation no longer changes it."""
    import torch

    ns, na, nt = ref["y1"].shape[1], ref["act"].shape[2], ref["terms"].shape[1]
    K = len(ids)
    state = torch.full((K, NE, cap + 1, ns), SENT)
    action = torch.full((K, NE, cap, na), SENT)
    terms = torch.full((K, NE, cap, nt + 1), SENT)
    length = torch.full((NE, K), LSENT, dtype=torch.int32)
    for s, i in enumerate(ids):
        ep, t = 0, 0
        state[s, 0, 0] = ref["start"][0, :, i]
        for T in range(max_steps):
            if ep >= NE:
                break
            if t < cap:  # steps past the capacity are counted, not written
                state[s, ep, t + 1] = ref["y1"][T, :, i]
                action[s, ep, t] = ref["act"][T, i]
                terms[s, ep, t, :nt] = ref["terms"][T, :, i]
                terms[s, ep, t, nt] = ref["rew"][T, i]
            t += 1
            if bool(ref["done"][T, i]):
                length[ep, s] = t
                ep, t = ep + 1, 0
                if ep < NE:  # row 0 of the next episode: the state the auto-reset left
                    state[s, ep, 0] = ref["start"][T + 1, :, i]
        if ep < NE:
            length[ep, s] = t  # cut by max_steps: the partial count
    return dict(state=state.to(DEV), action=action.to(DEV), terms=terms.to(DEV), length=length.to(DEV))


def _handle_after(ref, max_steps):
    """The snapshot (_aux and the obs rows) handle B must be left with after a call of `max_steps`: per
    env A's snapshot at the step its NE-th episode ended, or after max_steps steps."""
    import torch

    done = ref["done"].bool()
    n = done.shape[1]
    stop = torch.full((n,), max_steps, dtype=torch.long)
    for i in range(n):
        ends = done[:max_steps, i].nonzero().squeeze(1)
        if ends.numel() >= NE:
            stop[i] = int(ends[NE - 1]) + 1
    out = [x.clone() for x in ref["kept"][max_steps]]
    for T in set(stop.tolist()):
        m = (stop == T).to(DEV)
        for dst, src in zip(out, ref["kept"][T]):
            if dst.dim() == 2 and dst.shape[0] == n:  # the obs rows [n][ns]
                dst[m] = src[m]
            else:
                dst[..., m] = src[..., m]
    return out


def _run(model, prec, n, ids=None, cap=None, max_steps=NE * TL, fixture="landing", policy=None, slots=None, **over):
    """Handle B: one recording evaluation into sentinel-filled outputs and trace buffers. `slots`:
    a function that edits the slot plane before the call."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = _batch(model, n, fixture, **over)
    ev = PolicyEvaluator(b, policy if policy is not None else _policy(model), n_episodes=NE, max_steps=max_steps,
                         policy_dtype=prec, fused=True, record=list(ids if ids is not None else IDS[n]),
                         record_steps=cap, record_in_launch=True)
    assert ev.fused and ev.trace.choice is None
    for t, v in ((ev.ep_return, SENT), (ev.ep_length, LSENT), (ev.flags, 0xEE), (ev.used_mass, SENT),
                 (ev.final_state, SENT), (ev.episodes, LSENT)):
        t.fill_(v)
    tr = ev.trace
    for t, v in ((tr.state, SENT), (tr.action, SENT), (tr.terms, SENT), (tr.length, LSENT)):
        t.fill_(v)
    if slots is not None:
        slots(ev._slot)
    b.obs.fill_(SENT)
    res = ev.run()
    torch.cuda.synchronize()
    return b, ev, res


def _assert_trace(tr, want, eq=None, slots=None):
    import torch

    eq = eq or torch.equal
    sl = slice(None) if slots is None else slots
    for name in ("state", "action", "terms"):
        assert eq(getattr(tr, name)[sl], want[name][sl]), name
    assert torch.equal(tr.length[:, sl], want["length"][:, sl])


def _recorded_counts(ref, ids):
    """test_gpu_eval_exact._counts over the recorded envs only."""
    from rl_rocket_amd import _lib

    fl = ref["flags"][:, list(ids)].cpu().numpy().astype("int64")
    ep = ref["episodes"][list(ids)].cpu().numpy()
    fl = fl[fl != 0xEE]
    ev, la = (fl & _lib.RR_EVAL_EVENT) != 0, (fl & _lib.RR_EVAL_LANDED) != 0
    return dict(event_landed=int((ev & la).sum()), event_not_landed=int((ev & ~la).sum()),
                trunc=int(((fl & _lib.RR_EVAL_TRUNCATED) != 0).sum()), both_episodes=int((ep == NE).sum()))


CASES = [(6, "fp32", 300), (6, "fp16x3", 300), (3, "fp32", 300), (6, "fp32", 37), (6, "fp16x3", 37), (3, "fp32", 37),
         (6, "bf16", 37)]


@pytest.mark.parametrize("model,prec,n", CASES)
def test_trace_bitwise_equals_policy_act_plus_step(model, prec, n):
    """1. state, action, terms and length rows of the one launch against handle A's rows; every row
    past an episode's length keeps the sentinel (it is part of `want`). The rr_eval_out rows and the
    handle are the reference's as well. At n = 300 the reference's recorded envs hold every way an
    episode ends here (asserted on the reference loop alone)."""
    ref = _reference(model, prec, n)
    if n == 300:
        c = _recorded_counts(ref, IDS[n])
        print("ends of handle A's recorded envs (%dDOF, %s): %s" % (model, prec, c))
        assert c["event_landed"] >= 1 and c["event_not_landed"] >= 1 and c["trunc"] >= 1 and c["both_episodes"] >= 1
    b, ev, res = _run(model, prec, n)
    want = _expected(ref, IDS[n])
    _assert_trace(res.trace, want)
    assert int((want["state"] == SENT).sum()) > 0 and int((want["length"] != LSENT).sum()) > 0
    _compare(b, res, ref)
    b.close()


@pytest.mark.parametrize("model,prec,n", CASES)
def test_recording_does_not_disturb_the_evaluation(model, prec, n):
    """2. Twin handles: rr_eval_out rows, episodes, obs and the five handle images of the recording
    call against rr_policy_evaluate_exact's."""
    import torch
    from test_gpu_eval_exact import _evaluate

    b0, ev0, r0 = _evaluate(model, prec, n)
    b1, ev1, r1 = _run(model, prec, n)
    assert int(r0.episodes.max()) == NE
    for name in NAMES:
        assert torch.equal(getattr(r0, name), getattr(r1, name)), name
    for x, y in zip(_aux(b0), _aux(b1)):
        assert torch.equal(x, y)
    assert torch.equal(b0.obs, b1.obs)
    b0.close()
    b1.close()


@pytest.mark.parametrize("model,n", [(6, 300), (3, 37)])
def test_internal_consistency(model, n):
    """3. The last recorded state row of a finished episode is its final_state row; row 0 of
    episode 1 is the state the auto-reset left (the reference loop's post-step snapshot)."""
    import torch

    ref = _reference(model, "fp32", n)
    b, ev, res = _run(model, "fp32", n)
    tr = res.trace
    checked = 0
    for s, i in enumerate(IDS[n]):
        for k in range(int(res.episodes[i])):
            L = int(tr.length[k, s])
            assert 1 <= L <= TL
            assert torch.equal(tr.state[s, k, L], res.final_state[k, :, i])
            checked += 1
            if k + 1 < NE:
                T = int(ref["done"][:, i].nonzero()[k])  # the step that ended episode k
                assert torch.equal(tr.state[s, k + 1, 0], ref["kept"][T + 1][4][:, i].float())
                assert torch.equal(tr.state[s, k + 1, 0], ref["kept"][T + 1][0][:, i])  # the fp32 planes hold the same
    assert checked > len(IDS[n])
    b.close()


def test_capacity_clips_rows_and_keeps_counting():
    """4. record_steps = 5 < TL: length > 5 marks the clipped episodes, rows 0..5 are test 1's, nothing
    past them is written (the buffers end there, and the sentinel check of `want` covers the rest)."""
    import torch

    cap = 5
    ref = _reference(6, "fp32", 300)
    b, ev, res = _run(6, "fp32", 300, cap=cap)
    want, full = _expected(ref, IDS[300], cap=cap), _expected(ref, IDS[300])
    _assert_trace(res.trace, want)
    assert torch.equal(res.trace.length, full["length"])  # every step still counted
    clipped = res.trace.length > cap
    assert bool(clipped.any()) and bool(((res.trace.length <= cap) & (res.trace.length > 0)).any())
    assert torch.equal(res.trace.state, full["state"][:, :, :cap + 1])
    assert torch.equal(res.trace.action, full["action"][:, :, :cap])
    _compare(b, res, ref)
    b.close()


def test_max_steps_cut_writes_partial_lengths():
    """5. max_steps = 7: unfinished episodes report their partial count, episodes never started keep
    the sentinel in length and in every row, the handle equals the reference after 7 steps."""
    import torch

    cut = 7
    ref = _reference(6, "fp32", 300)
    b, ev, res = _run(6, "fp32", 300, max_steps=cut)
    want = _expected(ref, IDS[300], max_steps=cut)
    _assert_trace(res.trace, want)
    tr = res.trace
    done = ref["done"][:cut].bool()
    partial = never = 0
    for s, i in enumerate(IDS[300]):
        e = int(done[:, i].sum())
        assert int(res.episodes[i]) == min(e, NE)
        if e < NE:  # the running episode: steps since its start
            ends = done[:, i].nonzero().squeeze(1)
            since = cut - (int(ends[-1]) + 1 if ends.numel() else 0)
            assert int(tr.length[e, s]) == since
            partial += 1
            for k in range(e + 1, NE):
                assert int(tr.length[k, s]) == LSENT
                assert bool((tr.state[s, k] == SENT).all()) and bool((tr.action[s, k] == SENT).all())
                assert bool((tr.terms[s, k] == SENT).all())
                never += 1
    assert partial >= 1 and never >= 1
    for name, got, w in zip(("state", "v0", "counter", "ep_return", "state64"), _aux(b), _handle_after(ref, cut)):
        assert torch.equal(got, w), name
    assert torch.equal(b.obs, _handle_after(ref, cut)[5])
    b.close()


def test_slots_outside_the_range_record_nothing():
    """6. A slot plane of all -1 leaves every trace buffer untouched; a slot no env maps to stays
    untouched while the others are written; the evaluation is the reference's either way."""
    import torch

    ref = _reference(6, "fp32", 300)
    b, ev, res = _run(6, "fp32", 300, slots=lambda p: p.fill_(-1))
    tr = res.trace
    for t, v in ((tr.state, SENT), (tr.action, SENT), (tr.terms, SENT), (tr.length, LSENT)):
        assert torch.equal(t, torch.full_like(t, v))
    _compare(b, res, ref)
    b.close()

    ids = IDS[300]
    gone = 3  # env 70's slot: no env maps to it; a value past n_slots records nothing either

    def edit(p):
        p[ids[gone]] = -1
        p[100] = len(ids)
        p[101] = 1 << 30

    b, ev, res = _run(6, "fp32", 300, slots=edit)
    want = _expected(ref, ids)
    for name in ("state", "action", "terms"):
        want[name][gone] = SENT
    want["length"][:, gone] = LSENT
    _assert_trace(res.trace, want)
    _compare(b, res, ref)
    b.close()


def test_a_non_finite_env_is_recorded_and_leaves_the_others_alone():
    """7. NAN_ENV (recorded) ends RR_EVAL_NONFINITE at its first step with the NaN in its recorded
    row; every other recorded env's rows are test 1's."""
    import torch
    from rl_rocket_amd import _lib

    ids = IDS[300]
    s_nan = ids.index(NAN_ENV)
    ref, plain = _reference(6, "fp32", 300, "nan"), _reference(6, "fp32", 300)
    assert int(ref["flags"][0, NAN_ENV]) & _lib.RR_EVAL_NONFINITE and int(ref["len"][0, NAN_ENV]) == 1
    b, ev, res = _run(6, "fp32", 300, fixture="nan")
    tr = res.trace
    assert int(res.flags[0, NAN_ENV]) & _lib.RR_EVAL_NONFINITE
    assert int(tr.length[0, s_nan]) == 1
    assert bool(tr.state[s_nan, 0, 0].isnan().any()) and bool(tr.state[s_nan, 0, 1].isnan().any())
    _assert_trace(tr, _expected(ref, ids), eq=_same)
    others = [s for s in range(len(ids)) if s != s_nan]
    _assert_trace(tr, _expected(plain, ids), slots=others)
    _compare(b, res, ref, eq=_same)
    b.close()


def test_reward_annealing_records_the_annealed_reward_and_the_plain_terms():
    import torch

    ref, base = _reference(6, "fp32", 300, "landing", (("reward_annealing", True),)), _reference(6, "fp32", 300)
    assert not torch.equal(ref["rew"], base["rew"])  # the flag is live
    b, ev, res = _run(6, "fp32", 300, reward_annealing=True)
    _assert_trace(res.trace, _expected(ref, IDS[300]))
    _compare(b, res, ref)
    b.close()


def test_graph_replay_equals_eager():
    """8. A captured replay equals the eager call: outputs, handle and traces."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = _batch(6, 300)
    st0 = [t.clone() for t in b.get_state64()[:2]]
    ck = b.checkpoint()

    def rewind():
        b.restore(ck)
        b.set_state64(st0[0], v0=st0[1], elapsed=ck["counter"])

    ev = PolicyEvaluator(b, _policy(6), n_episodes=NE, max_steps=NE * TL, fused=True, record=list(IDS[300]),
                         record_in_launch=True)
    tr = ev.trace
    planes = (tr.state, tr.action, tr.terms, tr.length)
    res = ev.run()
    torch.cuda.synchronize()
    eager = {k: getattr(res, k).clone() for k in NAMES}
    eager_tr = [t.clone() for t in planes]
    eager_state = [t.clone() for t in _aux(b)]
    eager_obs = b.obs.clone()
    assert int(res.episodes.max()) == NE and int(tr.length.max()) > 1
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
    for t in planes:
        t.fill_(0)
    b.obs.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(getattr(res, k), eager[k]), k
    for got, w in zip(planes, eager_tr):
        assert torch.equal(got, w)
    for x, y in zip(_aux(b), eager_state):
        assert torch.equal(x, y)
    assert torch.equal(b.obs, eager_obs)
    b.close()


def test_fused_recorder_equals_the_step_by_step_recorder_with_a_constant_mean():
    """9. With a zero action head the mean is the bias whatever the tower arithmetic: the one launch
    (record_in_launch=True) and the PyTorch-op path (fused=False, record=) write equal EvalTrace
    tensors; an episode's analyzer_log has the reference's keys."""
    import torch
    from rl_rocket_amd.eval_trace import ANALYZER_KEYS
    from rl_rocket_amd.params import STATE_NAMES_6DOF
    from rl_rocket_amd.rollout import PolicyEvaluator

    pol = _policy(6, zero_head=True)
    ids = list(IDS[300])
    outs = []
    for fused in (True, False):
        b = _batch(6, 300)
        kw = dict(record_in_launch=True) if fused else {}
        ev = PolicyEvaluator(b, pol, n_episodes=NE, max_steps=NE * TL, fused=fused, record=ids, **kw)
        assert ev.fused == fused
        res = ev.run()
        torch.cuda.synchronize()
        outs.append((b, res))
    (b0, r0), (b1, r1) = outs
    assert int(r0.episodes.max()) == NE
    for name in ("state", "action", "terms", "length", "env_ids"):
        assert torch.equal(getattr(r0.trace, name), getattr(r1.trace, name)), name
    assert r0.trace.choice is None and r1.trace.choice is None
    for name in NAMES:
        assert torch.equal(getattr(r0, name), getattr(r1, name)), name
    for x, y in zip(_aux(b0), _aux(b1)):
        assert torch.equal(x, y)
    i = next(i for i in ids if int(r0.episodes[i]) >= 1)
    log = r0.trace.episode(i, k=0).analyzer_log()
    assert set(log) == {"ep_history/states", "ep_history/actions", "ep_history/vtarg", "ep_history/rewards",
                        "plots3d/vtarg_trajectory", "plots3d/trajectory", "ep_statistic/landing_success",
                        "ep_statistic/used_mass"} | {"final_errors/" + n for n in STATE_NAMES_6DOF}
    assert set(ANALYZER_KEYS) <= set(log)
    b0.close()
    b1.close()


def test_evaluate_policy_passes_the_keyword_through_and_the_refusals():
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic, PolicyEvaluator, PolicyPack, evaluate_policy

    pol = _policy(6)
    kw = dict(n_eval_episodes=1, return_episode_rewards=True, fused=True, record=[0, 63])
    with pytest.raises(ValueError, match="record_in_launch"):
        evaluate_policy(pol, _batch(6, 64, None), **kw)
    rewards, lengths = evaluate_policy(pol, _batch(6, 64, None), record_in_launch=True, **kw)
    twin = _batch(6, 64, None)
    twin.reset()  # evaluate_policy resets the batch it is given once more
    res = PolicyEvaluator(twin, pol, n_episodes=1, fused=True).run()
    torch.cuda.synchronize()
    assert len(rewards) == 64 and rewards == res.ep_return[0].cpu().tolist()
    assert lengths == res.ep_length[0].cpu().tolist()

    with pytest.raises(ValueError, match="fused=True"):
        PolicyEvaluator(twin, pol, n_episodes=1, fused=False, record=[0], record_in_launch=True)
    with pytest.raises(ValueError, match="fused=True"):
        PolicyEvaluator(twin, pol, n_episodes=1, record=[0], record_in_launch=True)
    with pytest.raises(ValueError, match="needs record"):
        PolicyEvaluator(twin, pol, n_episodes=1, fused=True, record_in_launch=True)
    with pytest.raises(ValueError):  # the refusal without the keyword stays
        PolicyEvaluator(twin, pol, n_episodes=1, fused=True, record=[0])
    d3 = _batch(3, 64, None)
    with pytest.raises(ValueError, match="Categorical"):
        PolicyEvaluator(d3, MlpCategoricalActorCritic(7, 4).to(DEV), n_episodes=1, fused=True, record=[0],
                        record_in_launch=True)
    # a fused RK4 batch records in its launch already: the keyword changes nothing
    got = []
    for k in (dict(), dict(record_in_launch=True)):
        rk = _batch(6, 64, None, integrator="rk4")
        r = PolicyEvaluator(rk, pol, n_episodes=1, fused=True, record=[5, 2], **k).run()
        torch.cuda.synchronize()
        got.append([t.clone() for t in (r.trace.state, r.trace.action, r.trace.terms, r.trace.length, r.ep_return)])
        # the C call refuses such a handle and points to the fast modes' recording call
        if k:
            lib = _lib.load()
            ev = PolicyEvaluator(twin, pol, n_episodes=1, fused=True, record=[5, 2], record_in_launch=True)
            params = PolicyPack(pol, 14, 3, torch.device(DEV)).pack()
            rc = lib.rr_policy_evaluate_exact_trace(rk._h, _ptr(params), 0, 1, 0, ctypes.byref(ev._out),
                                                    ctypes.byref(ev._trace_io), None, None)
            assert rc == _lib.RR_EINVAL
            msg = lib.rr_last_error()
            assert msg.startswith(b"rr_policy_evaluate_exact_trace: ") and msg.endswith(b"rr_policy_evaluate_trace"), msg
        rk.close()
    for x, y in zip(*got):
        assert torch.equal(x, y)
    twin.close()
    d3.close()
