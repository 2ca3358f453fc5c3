"""rr_policy_evaluate_sampled / rr_policy_evaluate_discrete_sampled (PolicyEvaluator(deterministic=False): whole
episodes under the SAMPLED action in one launch, plain or recording) against the per-step rollout, with the
scheme and shapes of tests/test_gpu_eval.py: n = 300 and 37, TimeLimit 80, two episodes per env, seed 11,
iter 0, sentinel-filled outputs, torch.equal everywhere.

Handle A is stepped with rr_rollout_step (rr_rollout_step_discrete for a Categorical policy) at t = 0, 1, ...
under (seed, iter) and read back after every step: done, truncated, terms, the terminal rows, the state planes,
the rollout buffers' obs and action rows. Twin handle B, created with the same seed, is evaluated once. The
policy is rollout_ref.scaled_policy at log_std = -1 (exp(-1) = 0.37: the noise moves every action and clips
some), or discrete_ref.cat_policy with discrete_ref.TABLES. Every row the evaluation writes for an env's first
two episodes, the state it leaves, every recorded row and every byte it does not own must equal A's.

Ends of handle A on an MI355X, event / bounds / truncation of the 600 episodes at n = 300 (the tests print
them): 6DOF fp32 and fp16x3 47 / 511 / 44, bf16 42 / 511 / 49, 3DOF 317 / 0 / 283; the CPU oracle with numpy
resets (tests/test_eval_sampled_host.py) gave 45 / 521 / 34 and 345 / 1 / 254 beforehand."""
import ctypes
import functools

import numpy as np
import pytest

import test_gpu_eval as E
import test_gpu_eval_discrete as D
import test_gpu_eval_trace as T

pytestmark = pytest.mark.gpu

DEV, TL, NE, SENT = E.DEV, E.TL, E.NE, E.SENT
LSENT, CSENT = T.LSENT, -9
SEED = 11
LOG_STD = -1.0
NAMES = D.NAMES
FILL = D.FILL
CAT = {4: 25, 3: 0, 2: 1}  # K: discrete_ref.cat_policy's seed
# n = 300: both ends of the batch, both ends of a wave, both workgroups, the ragged wave, scrambled; the other
# 293 envs are not recorded. n = 37: one partial wave, a scrambled subset
RECORD = {300: (299, 0, 63, 64, 256, 255, 17), 37: (36, 0, 20, 5)}


def _is_cat(kind):
    return isinstance(kind, tuple)


def _policy(kind, log_std=LOG_STD):
    """kind: 6 / 3 (the Gaussian policy of the model) or ("cat", K)."""
    import torch
    from discrete_ref import cat_policy
    from rollout_ref import scaled_policy

    if _is_cat(kind):
        return cat_policy(kind[1], CAT[kind[1]]).to(DEV)
    ns, na = (14, 3) if kind == 6 else (7, 2)
    pol = scaled_policy(ns, na, seed=5, head_scale=1.0 if kind == 6 else 0.05)
    with torch.no_grad():
        pol.log_std.fill_(log_std)
    return pol.to(DEV)


def _batch(kind, n, **over):
    if _is_cat(kind):
        over = dict(over)
        return D._batch(n, over.pop("integrator", "rk4"), over.pop("max_episode_steps", TL), **over)
    return E._batch(kind, n, **over)


class _Stepper:
    """rr_rollout_step / rr_rollout_step_discrete on a batch: step(seed, iter tensor, t) fills bufs (obs [n, ns],
    action [n, na] or the index [n], value, log-prob, start, reward) and the batch's own outputs."""

    def __init__(self, b, kind, pol, prec):
        import torch
        from rl_rocket_amd import _lib
        from rl_rocket_amd.rollout import PolicyPack

        n, ns = b.num_envs, b.state_dim
        f = dict(dtype=torch.float32, device=DEV)
        self.b, self.cat, self.lib = b, _is_cat(kind), _lib.load()
        self.pack = PolicyPack(pol, ns, pol.n_choices if self.cat else b.action_dim, b.device, precision=prec)
        self.params = self.pack.pack()
        self.bufs = [torch.zeros((n, ns), **f), torch.zeros(n, **f) if self.cat else torch.zeros((n, b.action_dim), **f)]
        self.bufs += [torch.zeros(n, **f) for _ in range(4)]
        if self.cat:
            self.k = pol.n_choices
            self.table_dev = pol.table.to(DEV)
            self.table = (ctypes.c_float * (2 * self.k))(*pol.table.reshape(-1).tolist())

    def step(self, seed, it, t):
        import torch
        from rl_rocket_amd import _lib
        from rl_rocket_amd.batch import _ptr

        a = self.b
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        tail = [_ptr(x) for x in self.bufs] + [_ptr(a.obs), _ptr(a.reward), _ptr(a.done), _ptr(a.truncated),
                                                _ptr(a.terms), stream]
        if self.cat:
            _lib.check(self.lib.rr_rollout_step_discrete(a._h, _ptr(self.params), self.k, self.table, self.pack.prec,
                                                         seed, _ptr(it), t, 0.99, *tail), "rr_rollout_step_discrete")
        else:
            _lib.check(self.lib.rr_rollout_step(a._h, _ptr(self.params), self.pack.prec, seed, _ptr(it), t, 0.99,
                                                *tail), "rr_rollout_step")

    def action_env(self):
        """What the env stepped with: the clipped sample, or the table row of the sampled index."""
        if self.cat:
            return self.table_dev[self.bufs[1].long()]
        return self.bufs[1].clamp(-1.0, 1.0)


def _prestep(b, kind, prec, pre):
    """`pre` sampled steps under another key (seed 77, iter 3): both handles start mid-episode, some past a reset."""
    import torch

    if pre:
        st = _Stepper(b, kind, _policy(kind), prec)
        it = torch.full((1,), 3, dtype=torch.int64, device=DEV)
        for t in range(pre):
            st.step(77, it, t)
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _reference(kind, prec, n, integrator="rk4", steps=NE * TL, tl=TL, pre=0, stats=True, it0=0, seed=SEED):
    """Handle A: `steps` per-step launches at t = 0 .. steps - 1 under (seed, it0), read back after every step.
    The rows the evaluation must write (test_gpu_eval._reference's keys, so that test_gpu_eval._compare reads
    them), A's snapshot at the step each env's last episode ended (its final one where it did not finish two),
    and for every env and step what test_gpu_eval_trace._check_against_reference reads, plus the obs row the
    policy was given (bobs) and, for a Categorical policy, the sampled index. Shared and never modified."""
    import torch

    a = _batch(kind, n, max_episode_steps=tl, integrator=integrator, episode_stats=stats)
    _prestep(a, kind, prec, pre)
    st = _Stepper(a, kind, _policy(kind), prec)
    ns, nt = a.state_dim, a.n_terms
    f = dict(dtype=torch.float32, device=DEV)
    it = torch.full((1,), it0, dtype=torch.int64, device=DEV)
    ep = torch.zeros(n, dtype=torch.long, device=DEV)
    ref = dict(ret=torch.full((NE, n), SENT, **f), len=torch.full((NE, n), -7, dtype=torch.int32, device=DEV),
               flags=torch.full((NE, n), 0xEE, dtype=torch.uint8, device=DEV), tobs=torch.full((NE, n, ns), SENT, **f),
               m_first=torch.full((NE, n), SENT, **f))
    snap0 = [t.clone() for t in E._aux(a)]
    m_first = snap0[0][-1].clone()
    acc = snap0[3].clone() if stats else torch.zeros(n, **f)  # ret: the running return, else 0 at the call
    last = [t.clone() for t in snap0]
    keys = ("state", "act", "rew", "terms", "done", "trunc", "tobs", "tlen", "bobs", "index")
    rows = {k: [] for k in keys}
    for t in range(steps):
        st.step(seed, it, t)
        tobs, tret, tlen = a.copy_terminal()
        snap = E._aux(a)
        done, trunc, terms = a.done.bool(), a.truncated.bool(), a.terms
        fl = E._flags((terms[nt + 1] > 0, terms[nt] > 0, trunc, terms[nt + 1] < 0, terms[nt - 1] != 0))
        acc = acc + a.reward  # ret += r, fp32 in step order
        active = ep < NE
        end = active & done
        e_i = end.nonzero().squeeze(1)
        k_i = ep[e_i]
        if stats:  # the Monitor return of the per-step path is that sum
            assert torch.equal(acc[e_i], tret[e_i])
        ref["ret"][k_i, e_i] = acc[e_i]
        ref["len"][k_i, e_i] = tlen[e_i]
        ref["flags"][k_i, e_i] = fl[e_i]
        ref["tobs"][k_i, e_i] = tobs[e_i]
        ref["m_first"][k_i, e_i] = m_first[e_i]
        m_first[e_i] = snap[0][-1, e_i]
        acc = torch.where(done, torch.zeros_like(acc), acc)
        ep = ep + end.long()
        for dst, src in zip(last, snap):
            dst[..., active] = src[..., active]
        index = st.bufs[1].to(torch.int32) if st.cat else torch.zeros(n, dtype=torch.int32, device=DEV)
        for k, v in zip(keys, (snap[0].T, st.action_env(), a.reward, terms[:nt].T, done, trunc, tobs, tlen,
                               st.bufs[0], index)):
            rows[k].append(v.clone())
    torch.cuda.synchronize()
    ref.update(episodes=ep.to(torch.int32), last=last, init=snap0[0].T.clone())
    ref["steps"] = {k: torch.stack(v) for k, v in rows.items()}  # [T, n, ...]
    a.close()
    return ref


def _rec_ref(ref, record):
    """The per-step rows of the recorded envs, in slot order: test_gpu_eval_trace._check_against_reference's input."""
    import torch

    ids = torch.tensor(record, device=DEV)
    out = {k: v[:, ids] for k, v in ref["steps"].items()}
    out["init"] = ref["init"][ids]
    return out


def _fill(ev):
    for name in NAMES:
        getattr(ev, name).fill_(FILL[name])
    tr = ev.trace
    if tr is not None:
        for t, v in ((tr.state, SENT), (tr.action, SENT), (tr.terms, SENT), (tr.length, LSENT)):
            t.fill_(v)
        if tr.choice is not None:
            tr.choice.fill_(CSENT)


def _evaluator(b, kind, prec="fp32", max_steps=NE * TL, record=None, record_steps=None, seed=SEED, it0=0,
               deterministic=False):
    from rl_rocket_amd.rollout import PolicyEvaluator

    kw = dict(deterministic=False, seed=seed) if not deterministic else {}
    ev = PolicyEvaluator(b, _policy(kind), n_episodes=NE, max_steps=max_steps, policy_dtype=prec,
                         fused=True if _is_cat(kind) else None, record=record, record_steps=record_steps, **kw)
    assert ev.fused
    if not deterministic:
        import torch

        assert ev.seed == seed and ev.iter.dtype == torch.int64 and tuple(ev.iter.shape) == (1,) and int(ev.iter) == 0
        ev.iter.fill_(it0)
    _fill(ev)
    return ev


def _evaluate(kind, prec, n, integrator="rk4", max_steps=NE * TL, tl=TL, pre=0, stats=True, it0=0, seed=SEED,
              record=None, record_steps=None, **over):
    """Handle B: one sampled evaluation into sentinel-filled outputs."""
    import torch

    b = _batch(kind, n, max_episode_steps=tl, integrator=integrator, episode_stats=stats, **over)
    _prestep(b, kind, prec, pre)
    ev = _evaluator(b, kind, prec, max_steps, record, record_steps, seed, it0)
    res = ev.run()
    torch.cuda.synchronize()
    assert int(ev.iter) == it0 + 1  # advanced in stream order
    return b, ev, res


def _outputs(b, res):
    return ({name: getattr(res, name).clone() for name in NAMES}, [t.clone() for t in E._aux(b)], b.obs.clone())


# ---- 1. bitwise against the per-step rollout ----

@pytest.mark.parametrize("n", [300, 37])  # 300: two workgroups, a ragged 44-env wave, three dead waves; 37: one partial wave
@pytest.mark.parametrize("model,prec", [(6, "fp32"), (6, "fp16x3"), (6, "bf16"), (3, "fp32")])
def test_sampled_bitwise_equals_per_step_rollout(model, prec, n):
    """The rows, the episode counts, the state / counter word / running return B is left with and the post-call
    obs, against handle A stepped 160 times with rr_rollout_step under the same (seed, iter), t = the step. At
    n = 300 each way an episode can end must occur. The CPU oracle (tests/test_eval_sampled_host.py) ends the 600
    episodes as event / bounds / truncation 45 / 521 / 34 (6DOF) and 345 / 1 / 254 (3DOF); handle A on an MI355X:
    47 / 511 / 44 (6DOF fp32, fp16x3), 42 / 511 / 49 (6DOF bf16), 317 / 0 / 283 (3DOF)."""
    ref = _reference(model, prec, n)
    if n == 300:
        c = E._counts(ref)
        print("ends of handle A under sampled actions (%dDOF, %s): %s" % (model, prec, c))
        assert c["trunc"] >= 1 and c["event"] >= 1
        if model == 6:
            assert c["bounds"] >= 1
    assert int(ref["episodes"].min()) == NE  # TimeLimit 80: every env ends two episodes in 160 steps
    b, ev, res = _evaluate(model, prec, n)
    E._compare(b, res, ref, model)
    assert res.stats()["episodes"] == NE * n
    b.close()


# ---- 2. the noise is live and keyed as stated ----

def test_noise_is_live_and_keyed_by_seed_and_iter():
    import torch

    n = 300
    b, ev, res = _evaluate(6, "fp32", n)
    first = _outputs(b, res)
    # against the deterministic evaluation of a twin batch
    c = _batch(6, n)
    det = _evaluator(c, 6, deterministic=True).run()
    torch.cuda.synchronize()
    assert not torch.equal(det.ep_return, first[0]["ep_return"])
    assert int((det.ep_return != first[0]["ep_return"]).any(0).sum()) >= n // 2  # not one env: most of them
    c.close()
    # another seed: other bits; the same (seed, iter): the same bits
    b2, _, r2 = _evaluate(6, "fp32", n, seed=12)
    assert not torch.equal(r2.ep_return, first[0]["ep_return"])
    b2.close()
    b3, _, r3 = _evaluate(6, "fp32", n)
    D._equal(first, _outputs(b3, r3), "same (seed, iter)")
    b3.close()
    # another iter: other bits, and exactly handle A's stepped with *iter = 1. Here as the evaluator's SECOND
    # run(), after the batch is put back where the first one started
    d = _batch(6, n)
    ck = d.checkpoint()
    ev = _evaluator(d, 6)
    ev.run()
    d.restore(ck)
    _fill(ev)
    res2 = ev.run()
    torch.cuda.synchronize()
    assert int(ev.iter) == 2
    assert not torch.equal(res2.ep_return, first[0]["ep_return"])
    E._compare(d, res2, _reference(6, "fp32", n, it0=1), 6)
    d.close()
    b.close()


# ---- 3. Euler ----

def test_euler_3dof():
    ref = _reference(3, "fp32", 300, integrator="euler")
    assert int(ref["episodes"].min()) == NE
    b, ev, res = _evaluate(3, "fp32", 300, integrator="euler")
    E._compare(b, res, ref, 3)
    b.close()


# ---- 4. the max_steps cap ----

@pytest.mark.parametrize("model", [6, 3])
def test_max_steps_cap_keeps_sentinels_and_leaves_the_state_of_50_steps(model):
    """max_steps = 50: rows of episodes not finished by then keep their sentinels (the reference writes none for
    them either), episodes[] counts the finished ones and every env's state, counter word and running return are
    A's after 50 steps. Under the noise some 6DOF envs end an episode inside 50 steps and most do not: both kinds
    must be there."""
    import torch

    ref = _reference(model, "fp32", 300, steps=50)
    b, ev, res = _evaluate(model, "fp32", 300, max_steps=50)
    E._compare(b, res, ref, model)
    unfinished = ~res.finished()
    assert int(unfinished.sum()) >= 300  # every env leaves at least its second row
    if model == 6:
        assert int(res.episodes.max()) >= 1 and int(res.episodes.min()) == 0
    for t, v in ((res.ep_return, SENT), (res.ep_length, -7), (res.flags, 0xEE), (res.used_mass, SENT)):
        assert torch.equal(t[unfinished], torch.full_like(t[unfinished], v))
    fs = res.final_state.permute(0, 2, 1)[unfinished]
    assert torch.equal(fs, torch.full_like(fs, SENT))
    assert res.stats()["unfinished"] == int(unfinished.sum())
    b.close()


# ---- 5. mid-episode start ----

@pytest.mark.parametrize("stats", [True, False])
def test_mid_episode_start(stats):
    """Both handles take ten sampled steps first (another key), so the call starts mid-episode with elapsed fields
    above 0 and, with episode_stats, running returns the first episode continues; without it the first return
    starts at 0 at the call (so the two references differ in first-episode returns and in nothing else). t counts
    from the call on both."""
    import torch

    ref = _reference(6, "fp32", 300, pre=10, stats=stats)
    assert int(ref["episodes"].min()) == NE
    other = _reference(6, "fp32", 300, pre=10, stats=not stats)
    assert torch.equal(ref["len"], other["len"]) and torch.equal(ref["ret"][1], other["ret"][1])
    assert not torch.equal(ref["ret"][0], other["ret"][0])
    b, ev, res = _evaluate(6, "fp32", 300, pre=10, stats=stats)
    E._compare(b, res, ref, 6)
    b.close()


# ---- 6. shards ----

def test_shards_reproduce_the_unsharded_evaluation():
    """128 + 172 envs with env_id_offset 0 / 128: the draws depend on the global id only, so the shards' rows,
    states and obs are the 300-env handle's, bit for bit (against handle A of the 300-env case)."""
    import torch

    ref = _reference(6, "fp32", 300)
    parts = [_evaluate(6, "fp32", m, env_id_offset=off) for m, off in ((128, 0), (172, 128))]
    for name, want in (("episodes", ref["episodes"]), ("ep_return", ref["ret"]), ("ep_length", ref["len"]),
                       ("flags", ref["flags"])):
        got = torch.cat([getattr(r, name) for _, _, r in parts], dim=-1)
        assert torch.equal(got, want), name
    for k, want in enumerate(ref["last"]):
        got = torch.cat([E._aux(b)[k] for b, _, _ in parts], dim=-1)
        assert torch.equal(got, want), k
    for b, _, _ in parts:
        b.close()


# ---- 7. recording ----

def _check_trace(kind, prec, n, b, res, ref, cap=TL, max_steps=NE * TL):
    """The recorded rows against A (test_gpu_eval_trace's check: state rows A's un-reset states, action rows the
    action the env stepped with, terms, rewards, lengths; sentinels elsewhere), and for a Categorical policy the
    choice plane against A's buf_action indices."""
    import torch

    tr = res.trace
    rr = _rec_ref(ref, RECORD[n])
    n_nat, n_trunc = T._check_against_reference(rr, b, res, cap=cap, max_steps=max_steps)
    if _is_cat(kind):
        want = torch.full_like(tr.choice, CSENT)
        K = len(RECORD[n])
        ks = torch.arange(K, device=DEV)
        ep = torch.zeros(K, dtype=torch.long, device=DEV)
        tc = torch.zeros(K, dtype=torch.long, device=DEV)
        for t in range(max_steps):
            active = ep < NE
            w = active & (tc < cap)
            want[ks[w], ep[w], tc[w]] = rr["index"][t][w]
            done = rr["done"][t] & active
            tc = torch.where(done, torch.zeros_like(tc), tc + active.long())
            ep = ep + done.long()
        assert torch.equal(tr.choice, want)
        w = tr.choice != CSENT
        assert torch.equal(tr.action[w], _policy(kind).table.to(DEV)[tr.choice[w].long()])
    else:
        assert tr.choice is None
    return n_nat, n_trunc


@pytest.mark.parametrize("n", [300, 37])
@pytest.mark.parametrize("model,prec", [(6, "fp32"), (6, "fp16x3"), (6, "bf16"), (3, "fp32")])
def test_recording_bitwise_equals_per_step_rollout(model, prec, n):
    """Slots in scrambled order, most envs unrecorded. The evaluation is the unrecorded sampled one (A's rows and
    state); action rows are clip(A's buf_action, -1, 1), some of them clipped; state rows A's un-reset states;
    terms, rewards and lengths A's; every other byte keeps its sentinel."""
    import torch

    ref = _reference(model, prec, n)
    b, ev, res = _evaluate(model, prec, n, record=RECORD[n])
    assert res.trace is ev.trace and res.trace.env_ids.tolist() == list(RECORD[n])
    E._compare(b, res, ref, model)
    n_nat, n_trunc = _check_trace(model, prec, n, b, res, ref)
    assert n_nat + n_trunc == NE * len(RECORD[n]) and n_nat >= 1
    assert torch.equal(res.trace.length, res.ep_length[:, res.trace.env_ids])
    if model == 6 and n == 300:  # the clip is exercised: the recorded rows hold +-1 where the sample left the box
        w = res.trace.action != SENT
        assert bool((res.trace.action[w].abs() == 1.0).any()) and float(res.trace.action[w].abs().max()) == 1.0
    b.close()


def _guarded(t, fill, guard=4096):
    """A tensor of t's shape inside a larger allocation whose `guard` elements before and after it hold `fill`."""
    import torch

    big = torch.full((t.numel() + 2 * guard,), fill, dtype=t.dtype, device=t.device)
    return big, big[guard:guard + t.numel()].view(t.shape)


def test_record_steps_below_the_length_clips_inside_guard_regions():
    """record_steps = 10 under TimeLimit 80: rows 0 .. 10 of the episodes are written, length still counts every
    step, and the 4096 elements before and after each trace buffer keep their fill."""
    import torch
    from rl_rocket_amd import _lib

    n = 300
    ref = _reference(3, "fp32", n)
    b = _batch(3, n)
    ev = _evaluator(b, 3, record=RECORD[n], record_steps=10)
    tr = ev.trace
    bigs = {}
    for name, fill in (("state", SENT), ("action", SENT), ("terms", SENT), ("length", LSENT)):
        bigs[name], view = _guarded(getattr(tr, name), fill)
        setattr(tr, name, view)
    ev._trace_io = _lib.RrEvalTrace(ev._slot.data_ptr(), tr.state.shape[0], tr.steps, tr.state.data_ptr(),
                                    tr.action.data_ptr(), tr.terms.data_ptr(), tr.length.data_ptr())
    res = ev.run()
    torch.cuda.synchronize()
    assert tr.state.shape[2] == 11 and tr.action.shape[2] == 10
    E._compare(b, res, ref, 3)
    _check_trace(3, "fp32", n, b, res, ref, cap=10)
    assert int(tr.length.min()) > 10 and torch.equal(tr.length, res.ep_length[:, tr.env_ids])
    for name, fill in (("state", SENT), ("action", SENT), ("terms", SENT), ("length", LSENT)):
        big, g = bigs[name], 4096
        assert torch.equal(big[:g], torch.full_like(big[:g], fill)), name
        assert torch.equal(big[-g:], torch.full_like(big[-g:], fill)), name
    b.close()


def test_demonstrations_from_a_sampled_trace():
    """obs rows are bitwise the rows A's rollout buffer received (buf_obs: what the policy was given), acts the
    clipped samples, slot-major then in step order (every episode finishes unclipped, so a slot's rows are its
    env's first length[0] + length[1] steps)."""
    import torch
    from rl_rocket_amd.bc import Demonstrations

    n = 300
    ref = _reference(6, "fp32", n)
    b, ev, res = _evaluate(6, "fp32", n, record=RECORD[n])
    demo = Demonstrations.from_trace(res.trace, b)
    total = res.trace.length.sum(0).tolist()  # per slot
    obs = torch.cat([ref["steps"]["bobs"][:m, e] for m, e in zip(total, RECORD[n])])
    act = torch.cat([ref["steps"]["act"][:m, e] for m, e in zip(total, RECORD[n])])
    assert len(demo) == sum(total) and torch.equal(demo.obs, obs) and torch.equal(demo.acts, act)
    b.close()


# ---- 8. the Categorical policy ----

@pytest.mark.parametrize("n", [300, 37])
@pytest.mark.parametrize("k", [4, 3, 2])
def test_categorical_bitwise_equals_per_step_rollout(k, n):
    """Plain and recording, against rr_rollout_step_discrete. choice equals A's buf_action indices and the action
    rows the table rows. At n = 300 every index occurs, and for K = 4 and 3 events and truncations both occur (K = 2
    truncates nearly every episode). Handle A on an MI355X, index usage over the 160 x 300 steps and ends as event
    / bounds / truncation: K = 4 6348 / 14545 / 16458 / 10649 and 131 / 253 / 217; K = 3 18316 / 13766 / 15918 and
    523 / 14 / 64; K = 2 20191 / 27809 and 2 / 0 / 598. CPU oracle (tests/test_eval_sampled_host.py): K = 4
    6350 / 14537 / 16446 / 10667 and 136 / 251 / 213; K = 3 18349 / 13729 / 15922 and 531 / 20 / 51; K = 2
    20217 / 27783 and 3 / 0 / 597."""
    import torch

    kind = ("cat", k)
    ref = _reference(kind, "fp32", n)
    assert int(ref["episodes"].min()) == NE
    if n == 300:
        c = E._counts(ref)
        use = torch.bincount(ref["steps"]["index"].reshape(-1).long(), minlength=4).tolist()
        print("K = %d: index usage over all 160 x 300 steps %s, ends %s" % (k, use, c))
        assert all(u >= 1 for u in use[:k]) and not any(use[k:])
        if k >= 3:
            assert c["event"] >= 1 and c["trunc"] >= 1
    b, ev, res = _evaluate(kind, "fp32", n)
    assert res.trace is None
    E._compare(b, res, ref, 3)
    plain = _outputs(b, res)
    b.close()
    b, ev, res = _evaluate(kind, "fp32", n, record=RECORD[n])
    assert res.trace.choice.dtype == torch.int32
    D._equal(plain, _outputs(b, res), "recording against plain")
    _check_trace(kind, "fp32", n, b, res, ref)
    b.close()


# ---- every dispatch arm: model x integrator x precision (and the Categorical integrators), plain and recording ----

ARMS = [(m, i, p) for m in (6, 3) for i in ("rk4", "euler") for p in ("fp32", "fp16x3", "bf16")] + \
       [(("cat", 4), i, "fp32") for i in ("rk4", "euler")]


@pytest.mark.parametrize("kind,integrator,prec", ARMS)
def test_every_arm_plain_and_recording(kind, integrator, prec):
    """n = 37 under TimeLimit 20 (40 steps): the plain and the recording kernel of every instantiation against the
    per-step path of the same instantiation."""
    n, tl = 37, 20
    ref = _reference(kind, prec, n, integrator=integrator, steps=NE * tl, tl=tl)
    assert int(ref["episodes"].min()) == NE
    model = 3 if _is_cat(kind) else kind
    b, ev, res = _evaluate(kind, prec, n, integrator=integrator, tl=tl, max_steps=NE * tl)
    E._compare(b, res, ref, model)
    plain = _outputs(b, res)
    b.close()
    b, ev, res = _evaluate(kind, prec, n, integrator=integrator, tl=tl, max_steps=NE * tl, record=RECORD[n])
    D._equal(plain, _outputs(b, res), "recording against plain")
    _check_trace(kind, prec, n, b, res, ref, cap=tl, max_steps=NE * tl)
    b.close()


# ---- 9. graph capture ----

def _planes(tr):
    names = ("state", "action", "terms", "length") + (("choice",) if tr.choice is not None else ())
    return {k: getattr(tr, k).clone() for k in names}


@pytest.mark.parametrize("kind", [6, ("cat", 4)])
def test_graph_replays_draw_fresh_noise(kind):
    """A captured run() replayed twice equals two eager runs: iter is advanced inside the graph. One stream, no
    parallel branches."""
    import torch

    n = 300
    b = _batch(kind, n)
    ck = b.checkpoint()
    ev = _evaluator(b, kind, record=RECORD[n])
    eager = []
    for _ in range(2):
        b.restore(ck)
        _fill(ev)
        res = ev.run()
        torch.cuda.synchronize()
        eager.append((_outputs(b, res), _planes(res.trace)))
    assert int(ev.iter) == 2 and not torch.equal(eager[0][0][0]["ep_return"], eager[1][0][0]["ep_return"])
    ev.iter.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ev.run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert int(ev.iter) == 0  # capture ran nothing
    for k in range(2):
        b.restore(ck)
        _fill(ev)
        g.replay()
        torch.cuda.synchronize()
        assert int(ev.iter) == k + 1
        D._equal(eager[k][0], _outputs(b, res), "replay %d" % k)
        for name, want in eager[k][1].items():
            assert torch.equal(getattr(res.trace, name), want), (k, name)
    b.close()


# ---- 10. RR_EINVAL, before any launch ----

def test_argument_errors_leave_the_outputs_untouched():
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout import PolicyPack

    lib = _lib.load()
    n = 64
    g = PolicyPack(_policy(6), 14, 3, torch.device(DEV)).pack()
    cat = _policy(("cat", 4))
    c = PolicyPack(cat, 7, 4, torch.device(DEV)).pack()
    table = (ctypes.c_float * 8)(*cat.table.reshape(-1).tolist())
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    outs = dict(ep=torch.full((n,), -7, dtype=torch.int32, device=DEV), ret=torch.full((1, n), SENT, device=DEV),
                obs6=torch.full((n, 14), SENT, device=DEV), obs3=torch.full((n, 7), SENT, device=DEV),
                slot=torch.zeros(n, dtype=torch.int32, device=DEV), st=torch.full((1, 1, 5, 14), SENT, device=DEV),
                ln=torch.full((1, 1), LSENT, dtype=torch.int32, device=DEV),
                ch=torch.full((1, 1, 4), CSENT, dtype=torch.int32, device=DEV))
    keep = {k: v.clone() for k, v in outs.items()}
    out = _lib.RrEvalOut(episodes=outs["ep"].data_ptr(), ep_return=outs["ret"].data_ptr())
    o = ctypes.byref(out)

    def trace(n_slots=1, steps=4, state=True):
        return ctypes.byref(_lib.RrEvalTrace(outs["slot"].data_ptr(), n_slots, steps,
                                             outs["st"].data_ptr() if state else None, None, None,
                                             outs["ln"].data_ptr()))

    def gauss(b, params=g, prec=0, iter_=it, ne=1, ms=0, o_=o, tr=None):
        return lib.rr_policy_evaluate_sampled(b._h if b is not None else None, _ptr(params), prec, SEED,
                                              _ptr(iter_) if iter_ is not None else None, ne, ms, o_, tr,
                                              _ptr(outs["obs6"]), None)

    def disc(b, params=c, k=4, prec=0, iter_=it, ne=1, ms=0, o_=o, tr=None, ch=None):
        return lib.rr_policy_evaluate_discrete_sampled(b._h if b is not None else None, _ptr(params), k, table, prec,
                                                       SEED, _ptr(iter_) if iter_ is not None else None, ne, ms, o_,
                                                       tr, _ptr(ch) if ch is not None else None, _ptr(outs["obs3"]),
                                                       None)

    def refused(rc, name, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(name + b": ") and word in msg, msg
        torch.cuda.synchronize()
        for k, v in outs.items():
            assert torch.equal(v, keep[k]), (msg, k)

    G, C = b"rr_policy_evaluate_sampled", b"rr_policy_evaluate_discrete_sampled"
    ok6, ok3 = E._batch(6, n), E._batch(3, n)
    refused(gauss(ok6, iter_=None), G, b"iter")
    refused(gauss(None), G, b"handle")
    refused(gauss(ok6, ms=2 ** 31), G, b"2^31")
    refused(gauss(ok6, ne=30_000_000), G, b"2^31")  # 30e6 episodes x TimeLimit 80: the effective max_steps
    assert gauss(ok6, ms=2 ** 31 - 1, ne=1) == 0  # the largest max_steps: accepted (one episode ends the launch)
    torch.cuda.synchronize()
    assert torch.equal(outs["ep"], torch.ones_like(outs["ep"])) and bool((outs["ret"] != SENT).all())
    for k in ("ep", "ret", "obs6"):
        outs[k].copy_(keep[k])
    refused(gauss(E._batch(6, n, integrator="dopri5")), G, b"RR_INT_DOPRI5")
    refused(gauss(E._batch(6, n, auto_reset=False)), G, b"RR_FLAG_AUTO_RESET")
    refused(gauss(E._batch(6, n, max_episode_steps=0)), G, b"TimeLimit")
    refused(gauss(ok6, ne=0), G, b"n_episodes")
    refused(gauss(ok6, prec=7), G, b"precision")
    refused(gauss(ok6, o_=ctypes.byref(_lib.RrEvalOut())), G, b"episodes")
    refused(gauss(ok6, tr=trace(n_slots=0)), G, b"n_slots")
    refused(gauss(ok6, tr=trace(steps=0)), G, b"steps")
    refused(gauss(ok6, tr=trace(state=False)), G, b"trace->state")
    refused(disc(ok3, iter_=None), C, b"iter")
    refused(disc(ok3, ch=outs["ch"]), C, b"choice")
    refused(disc(ok3, prec=_lib.RR_POLICY_BF16), C, b"RR_POLICY_FP32")
    refused(disc(ok3, k=5), C, b"2 .. 4")
    refused(disc(ok6), C, b"6DOF")
    refused(disc(D._batch(n, "dopri5")), C, b"RR_INT_DOPRI5")
    refused(disc(ok3, ms=2 ** 31), C, b"2^31")
    refused(disc(ok3, tr=trace(n_slots=0), ch=outs["ch"]), C, b"n_slots")
    refused(disc(None), C, b"handle")
    assert disc(ok3) == 0  # the same call with nothing wrong
    torch.cuda.synchronize()
    assert torch.equal(outs["ep"], torch.ones_like(outs["ep"]))


# ---- 11. evaluate_policy ----

@pytest.mark.parametrize("kind", [6, ("cat", 4)])
def test_evaluate_policy_deterministic_false(kind):
    """SB3's (mean_reward, std_reward) are the population mean and std of the evaluator's finished rows (float64:
    two summation orders of 600 fp32 values agree to 600 x 2^-53 relative, held to 1e-12), and the episode lists
    are those rows exactly."""
    import torch
    from rl_rocket_amd.rollout import evaluate_policy

    n = 300
    pol = _policy(kind)
    kw = dict(fused=True) if _is_cat(kind) else {}
    mean, std = evaluate_policy(pol, _batch(kind, n), n_eval_episodes=NE, deterministic=False, seed=SEED, **kw)
    rewards, lengths = evaluate_policy(pol, _batch(kind, n), n_eval_episodes=NE, return_episode_rewards=True,
                                       deterministic=False, seed=SEED, **kw)
    twin = _batch(kind, n)
    twin.reset()  # evaluate_policy resets the batch it is given
    ev = _evaluator(twin, kind)
    res = ev.run()
    torch.cuda.synchronize()
    assert int(res.episodes.min()) == NE
    ret = res.ep_return.cpu().numpy().astype(np.float64)
    assert mean == pytest.approx(ret.mean(), rel=1e-12) and std == pytest.approx(ret.std(), rel=1e-12)
    assert rewards == res.ep_return.cpu().reshape(-1).tolist() and lengths == res.ep_length.cpu().reshape(-1).tolist()
    det_mean, _ = evaluate_policy(pol, _batch(kind, n), n_eval_episodes=NE, **kw)
    assert det_mean != mean  # the default stays the deterministic evaluation
    twin.close()
