"""rr_policy_evaluate_trace (the one-launch evaluation recording whole episodes of chosen envs)
against the per-step path, with the conventions of tests/test_gpu_eval.py: TimeLimit 80, 2 episodes
per env, rollout_ref.scaled_policy at log_std = -60, sentinel-filled outputs.

Handle A is stepped 160 times with rr_rollout_step and read back after every step (buf_action, the
env reward, terms, done, the terminal rows, the state planes), for the recorded envs. Handle B, same
seed, gets one recording call. Every recorded row must equal A's bit for bit, every byte the
recording does not own must keep its sentinel, and the evaluation itself must be the plain one's."""
import ctypes
import functools

import numpy as np
import pytest

import rollout_ref as R
import test_gpu_eval as E
from gpu_util import TOL_STATE

pytestmark = pytest.mark.gpu

DEV, TL, NE, SENT = E.DEV, E.TL, E.NE, E.SENT
LSENT = -7
# n = 300: two workgroups, a ragged 44-env wave, dead waves; both ends of a wave, both workgroups, the
# ragged wave, unsorted. n = 37: one partial wave, every env recorded (K = n).
RECORD = {300: (299, 0, 63, 64, 256, 255, 17), 37: tuple(range(37))}


def _inv(b):
    import torch

    return torch.tensor((1.0 / b.cfg.state_normalizer).astype(np.float32), device=DEV)  # KParams.inv_norm


@functools.lru_cache(maxsize=None)
def _reference(model, prec, n, annealing=False):
    """Handle A: NE * TL rr_rollout_step launches; after each, what the recorded envs did. Shared by
    the tests below and never modified."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout import PolicyPack

    a = E._batch(model, n, reward_annealing=annealing)
    pol = E._policy(model)
    ns, na, nt = a.state_dim, a.action_dim, a.n_terms
    pack = PolicyPack(pol, ns, na, a.device, precision=prec)
    params = pack.pack()
    f = dict(dtype=torch.float32, device=DEV)
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    bufs = [torch.zeros((n, ns), **f), torch.zeros((n, na), **f)] + [torch.zeros(n, **f) for _ in range(4)]
    lib = _lib.load()
    rec = torch.tensor(RECORD[n], device=DEV)
    keys = ("state", "act", "rew", "terms", "done", "trunc", "tobs", "tlen")
    steps = {k: [] for k in keys}
    init = a.get_state()[0][:, rec].T.clone()
    for t in range(NE * TL):
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        _lib.check(lib.rr_rollout_step(a._h, _ptr(params), pack.prec, 11, _ptr(it), t, 0.99, *[_ptr(b) for b in bufs],
                                       _ptr(a.obs), _ptr(a.reward), _ptr(a.done), _ptr(a.truncated), _ptr(a.terms),
                                       stream), "rr_rollout_step")
        tobs, _tret, tlen = a.copy_terminal()
        for k, v in zip(keys, (a.get_state()[0][:, rec].T, bufs[1][rec].clamp(-1.0, 1.0),
                               a.reward[rec], a.terms[:nt, rec].T, a.done[rec].bool(), a.truncated[rec].bool(),
                               tobs[rec], tlen[rec])):
            steps[k].append(v.clone())
    torch.cuda.synchronize()
    ref = {k: torch.stack(v) for k, v in steps.items()}  # [T, K, ...]
    ref["init"] = init
    a.close()
    return ref


def _record(model, prec, n, annealing=False, record_steps=None, max_steps=NE * TL, fused=None, policy=None,
            record=None):
    """Handle B: one recording evaluation into sentinel-filled buffers."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = E._batch(model, n, reward_annealing=annealing)
    ev = PolicyEvaluator(b, policy if policy is not None else E._policy(model), n_episodes=NE, max_steps=max_steps,
                         policy_dtype=prec, fused=fused, record=RECORD[n] if record is None else record,
                         record_steps=record_steps)
    _fill(ev)
    res = ev.run()
    torch.cuda.synchronize()
    return b, ev, res


def _fill(ev):
    for t, v in ((ev.ep_return, SENT), (ev.ep_length, -7), (ev.flags, 0xEE), (ev.used_mass, SENT),
                 (ev.final_state, SENT), (ev.episodes, -7)):
        t.fill_(v)
    tr = ev.trace
    for t, v in ((tr.state, SENT), (tr.action, SENT), (tr.terms, SENT), (tr.length, LSENT)):
        t.fill_(v)


def _check_against_reference(ref, b, res, cap, max_steps=NE * TL):
    """Every recorded row against A's per-step read-backs; everything else keeps its sentinel.
    Returns (natural ends, truncations) among the recorded episodes."""
    import torch

    tr = res.trace
    K = tr.env_ids.numel()
    inv = _inv(b)
    want = {k: torch.full_like(getattr(tr, k), SENT) for k in ("state", "action", "terms")}
    want_len = torch.full_like(tr.length, LSENT)
    ks = torch.arange(K, device=DEV)
    ep = torch.zeros(K, dtype=torch.long, device=DEV)
    tc = torch.zeros(K, dtype=torch.long, device=DEV)
    want["state"][:, 0, 0] = ref["init"]
    n_nat = n_trunc = 0
    for t in range(max_steps):
        active = ep < NE
        w = active & (tc < cap)
        done = ref["done"][t] & active
        cont, term = w & ~done, w & done
        want["state"][ks[cont], ep[cont], tc[cont] + 1] = ref["state"][t][cont]
        # a terminal row: A has only its obs row; the recorded state times inv_norm must be it
        # (the multiplication of test_gpu_eval._compare), then the row counts as checked
        got = tr.state[ks[term], ep[term], tc[term] + 1]
        assert torch.equal(got * inv[None, :], ref["tobs"][t][term]), t
        want["state"][ks[term], ep[term], tc[term] + 1] = got
        want["action"][ks[w], ep[w], tc[w]] = ref["act"][t][w]
        want["terms"][ks[w], ep[w], tc[w]] = torch.cat([ref["terms"][t], ref["rew"][t][:, None]], dim=1)[w]
        tc = tc + active.long()
        want_len[ep[done], ks[done]] = ref["tlen"][t][done]
        assert torch.equal(tc[done].to(torch.int32), ref["tlen"][t][done])  # episodes start at the call: elapsed = count
        n_trunc += int((done & ref["trunc"][t]).sum())
        n_nat += int((done & ~ref["trunc"][t]).sum())
        nxt = done & (ep + 1 < NE)
        want["state"][ks[nxt], ep[nxt] + 1, 0] = ref["state"][t][nxt]  # the post-reset state
        ep = ep + done.long()
        tc = torch.where(done, torch.zeros_like(tc), tc)
    cut = ep < NE
    want_len[ep[cut], ks[cut]] = tc[cut].to(torch.int32)
    for k in ("state", "action", "terms"):
        assert torch.equal(getattr(tr, k), want[k]), k
    assert torch.equal(tr.length, want_len)
    assert torch.equal(res.episodes[tr.env_ids].long(), ep)
    return n_nat, n_trunc


@pytest.mark.parametrize("n", [300, 37])
@pytest.mark.parametrize("model,prec,annealing", [(6, "fp32", False), (6, "fp16x3", False), (3, "fp32", False),
                                                  (6, "fp32", True)])
def test_trace_bitwise_equals_per_step_rollout(model, prec, annealing, n):
    """State rows (non-terminal: A's state planes; terminal: times inv_norm A's terminal obs row; row
    0 of a later episode: A's post-reset state), actions = clamp(buf_action), terms and reward, length
    = A's terminal length; the fp32 sequential sum of the recorded rewards is ep_return; every byte
    outside the recorded rows keeps its sentinel."""
    import torch

    ref = _reference(model, prec, n, annealing)
    b, ev, res = _record(model, prec, n, annealing)
    assert ev.fused and res.trace is ev.trace and res.trace.env_ids.tolist() == list(RECORD[n])
    n_nat, n_trunc = _check_against_reference(ref, b, res, cap=TL)
    print("recorded episodes (%dDOF %s n=%d): %d natural ends, %d truncations" % (model, prec, n, n_nat, n_trunc))
    K = len(RECORD[n])
    assert n_nat + n_trunc == NE * K  # TimeLimit 80: every env ends two episodes in 160 steps
    assert n_nat >= 1                 # the terminal-row and post-reset-row checks above ran
    # ret += r in step order from 0.0 (the handle was reset: no running return)
    length = res.trace.length.cpu().numpy()
    rew = res.trace.terms[..., -1].cpu().numpy()
    ep_return = res.ep_return[:, res.trace.env_ids].cpu().numpy()
    for s in range(K):
        for k in range(NE):
            acc = np.float32(0.0)
            for r in rew[s, k, :length[k, s]]:
                acc = np.float32(acc + r)
            assert acc == ep_return[k, s], (s, k)
    assert torch.equal(res.trace.length, res.ep_length[:, res.trace.env_ids])
    rec = res.trace.episode(RECORD[n][0], k=1)
    assert len(rec) == int(length[1, 0]) and rec.complete
    b.close()


@pytest.mark.parametrize("model,prec", [(6, "fp32"), (3, "fp32")])
def test_recording_does_not_disturb_the_evaluation(model, prec):
    """A third handle evaluated with plain rr_policy_evaluate from the same state: the rr_eval_out
    rows, episodes, the handle's state / v0 / counter / running return and the post-call obs are
    bit for bit equal."""
    import torch

    b, ev, res = _record(model, prec, 300)
    c, _, plain = E._evaluate(model, prec, 300)
    assert plain.trace is None
    for name in ("episodes", "ep_return", "ep_length", "flags", "used_mass", "final_state"):
        assert torch.equal(getattr(res, name), getattr(plain, name)), name
    for x, y in zip(E._aux(b), E._aux(c)):
        assert torch.equal(x, y)
    assert torch.equal(b.obs, c.obs)
    b.close()
    c.close()


def test_capacity_clips_rows_and_keeps_counting():
    """3DOF, record_steps = 10 (the shortest oracle episode at these settings is 73 steps): rows
    0..10 are written, everything past them keeps the sentinel, length reports the full count and
    episode() raises without clipped=True."""
    import torch

    ref = _reference(3, "fp32", 300)
    b, ev, res = _record(3, "fp32", 300, record_steps=10)
    tr = res.trace
    assert tr.state.shape[2] == 11 and tr.action.shape[2] == 10
    _check_against_reference(ref, b, res, cap=10)
    assert int(tr.length.min()) > 10
    assert torch.equal(tr.length, res.ep_length[:, tr.env_ids])
    assert bool((tr.state != SENT).all()) and bool((tr.action != SENT).all())  # rows 0..10 of every episode
    with pytest.raises(ValueError, match="record holds 10"):
        tr.episode(299, k=0)
    rec = tr.episode(299, k=0, clipped=True)
    assert len(rec) == 10 and rec.length == int(tr.length[0, 0]) and not rec.complete
    b.close()


def test_max_steps_cap_writes_partial_lengths():
    """3DOF, max_steps = 50: no episode finishes, length[0] is 50 for every recorded env, rows 0..50
    equal A's first 50 steps, episode(..., partial=True) works."""
    import torch

    ref = _reference(3, "fp32", 300)
    assert not bool(ref["done"][:50].any())
    b, ev, res = _record(3, "fp32", 300, max_steps=50)
    tr = res.trace
    _check_against_reference(ref, b, res, cap=TL, max_steps=50)
    assert torch.equal(tr.length[0], torch.full_like(tr.length[0], 50))
    assert torch.equal(tr.length[1], torch.full_like(tr.length[1], LSENT))
    assert torch.equal(res.episodes, torch.zeros_like(res.episodes))
    with pytest.raises(ValueError, match="did not finish"):
        tr.episode(17)
    rec = tr.episode(17, partial=True)
    assert len(rec) == 50 and rec.states.shape == (51, 7) and not rec.complete
    assert rec.vtarg_to_dataframe().shape == (50, 2)
    b.close()


def test_fused_equals_unfused_with_a_constant_mean():
    """With the action head's weight zeroed the mean is the bias whatever the tower arithmetic: the
    kernel and the PyTorch-op loop (fused=False) write the same trace, bit for bit."""
    import torch

    pol = E._policy(6, zero_head=True)
    outs = []
    for fused in (True, False):
        b, ev, res = _record(6, "fp32", 300, fused=fused, policy=pol)
        assert ev.fused == fused
        outs.append((b, res))
    (b0, r0), (b1, r1) = outs
    assert int(r0.episodes.min()) == NE
    for name in ("state", "action", "terms", "length"):
        assert torch.equal(getattr(r0.trace, name), getattr(r1.trace, name)), name
    assert bool((r0.trace.length > 0).all())
    for name in ("episodes", "ep_return", "ep_length"):
        assert torch.equal(getattr(r0, name), getattr(r1, name)), name
    b0.close()
    b1.close()


def test_graph_replay_equals_eager():
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    b = E._batch(6, 300)
    ck = b.checkpoint()
    ev = PolicyEvaluator(b, E._policy(6), n_episodes=NE, max_steps=NE * TL, record=RECORD[300])
    _fill(ev)
    res = ev.run()
    torch.cuda.synchronize()
    names = ("state", "action", "terms", "length")
    eager = {k: getattr(res.trace, k).clone() for k in names}
    eager_ret = res.ep_return.clone()
    b.restore(ck)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ev.run()
    torch.cuda.current_stream().wait_stream(s)
    b.restore(ck)
    _fill(ev)
    g.replay()
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(res.trace, k), eager[k]), k
    assert torch.equal(res.ep_return, eager_ret)
    b.close()


ORACLE_ENVS = (3, 40, 77, 130, 191, 222, 260, 299)  # two per wave of the first workgroup and four of the second
MAX_MISMATCH_ROWS = 6  # the replay test's cap (tests/test_gpu_rollout_replay.py: 1e-5 of 661 280 rows)


@pytest.mark.parametrize("model", [6, 3])
def test_recorded_steps_against_the_cpu_oracle(model, oracle_mod):
    """Every recorded (state[t], action[t]) stepped by the fp64 oracle gives state[t + 1] within the
    fast-mode bar (1e-5 floored-relative, DESIGN.md section 4 / tests/test_gpu_parity.py; theta on
    the circle), on the rows where the oracle's done agrees with the record; done / not-done agree
    on all but at most 6 rows.
    Measured (MI355X): 6DOF 748 recorded steps, 15 natural ends, 0 mismatches, max error 3.42e-7;
    3DOF 1 266 steps, 11 natural ends, 0 mismatches, 1.27e-7. The 8 envs were fixed before the first
    run; a CPU-only pre-check that the oracle replaying its own episodes of these envs meets no
    marginal row was not made."""
    from rl_rocket_amd import _lib

    b, ev, res = _record(model, "fp32", 300, record=ORACLE_ENVS)
    tr = res.trace
    cfg = oracle_mod.make_cfg(model, **(oracle_mod.ENV_CONFIG_6DOF if model == 6 else oracle_mod.DEFAULTS_3DOF))
    ns = b.state_dim
    norm = np.array(cfg.normalizer[:ns])
    state, action = tr.state.cpu().numpy(), tr.action.cpu().numpy()
    length = tr.length.cpu().numpy()
    flags = res.flags[:, tr.env_ids].cpu().numpy()
    ic, t_in, s_in, a_in, s_out, ended = [], [], [], [], [], []
    for s in range(len(ORACLE_ENVS)):
        for k in range(NE):
            L = int(length[k, s])
            assert 1 <= L <= TL
            natural = (int(flags[k, s]) & _lib.RR_EVAL_TRUNCATED) == 0
            for t in range(L):
                ic.append(state[s, k, 0])
                t_in.append(t * cfg.dt)
                s_in.append(state[s, k, t].astype(np.float64))
                a_in.append(action[s, k, t])
                s_out.append(state[s, k, t + 1].astype(np.float64))
                ended.append(natural and t == L - 1)
    o = oracle_mod.step(cfg, np.array(ic), np.array(t_in), np.array(s_in), np.array(a_in), nthreads=8)
    ended = np.array(ended)
    mism = o["done"] != ended
    agree = ~mism
    err = R._obs_err(model, np.array(s_out)[agree] / norm, o["state_out"][agree] / norm)
    print("%dDOF: %d recorded steps, %d natural ends, done mismatches %d, max floored-relative error %.3g" % (
        model, len(ended), int(ended.sum()), int(mism.sum()), float(err.max())))
    assert int(mism.sum()) <= MAX_MISMATCH_ROWS, np.argwhere(mism).ravel()
    assert float(err.max()) <= TOL_STATE
    b.close()


def test_full_size_sanity():
    """N = 65 536, K = 64, TimeLimit 80, one episode: length of every recorded env is its ep_length
    and the recorded terminal row is final_state."""
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    n = 65536
    b = E._batch(6, n)
    record = torch.arange(64) * 1021 + 5  # spread over the grid; 64 327 is the last
    ev = PolicyEvaluator(b, E._policy(6), n_episodes=1, record=record)
    res = ev.run()
    torch.cuda.synchronize()
    tr = res.trace
    ids = tr.env_ids
    assert torch.equal(res.episodes, torch.ones_like(res.episodes))
    assert torch.equal(tr.length[0], res.ep_length[0, ids])
    ks = torch.arange(64, device=DEV)
    assert torch.equal(tr.state[ks, 0, tr.length[0].long()], res.final_state[0][:, ids].T)
    b.close()
