"""The Categorical sampler and act kernel at their domain edges (inputs: tests/discrete_sampler_ref.py, checked on
the CPU by tests/test_discrete_sampler_inputs.py). The sampler text (fp32 softmax, one uniform draw u = r 2^-24, the
inverse-CDF index, the table row) exists in three copies, discrete_act_kernel (rr_policy_act_discrete),
rocket_rollout_body.inc (rr_rollout_step_discrete, rr_rollout_collect_discrete) and rocket_eval_body.inc
(rr_policy_evaluate_discrete_sampled); tests/test_gpu_discrete.py and tests/test_gpu_rollout_discrete.py hold them
to float64 and to one another on random draws, which land on one given u once in 2^24 rows.

a. The sampler on all four entry points, with constant-logit policies (const_policy: the logits are the fp32
   biases whatever the obs) and the committed draws r = 0, 2^24 - 1, 2^24 - 2, 2^24 - 3, 2^22, 2^23, 3 2^22: the
   ends of the range with every choice live (K = 4, 3, 2); logit sets with dead choices (ex = 0 in fp32) on which
   a running sum that stops short of 1 - 2^-24 would walk into a dead trailing choice; exact ties with a running
   sum (the boundary value goes to the next choice); one 65 536-row launch per K with equal logits (every bit of
   u). The expected index is the float64 reference's (discrete_sampler_ref.live_ref), on whole launches: the
   special row sits at lane 0, 31, 32 or 63 of a 64-row call, and its 63 neighbours are compared too.
b. rr_policy_act_discrete as tests/test_gpu_policy_edges.py a, c, d, e have rr_policy_act: value inside
   policy_bound.forward_bound's bound and log-prob inside 2 max dz + 2^-24 (2 |z_a - z_max| + 2 |lse| + 12) of
   float64 on 2 K x 3 weight sets x 6 obs classes; peaked logits; neighbours (zeros, 1e6, NaN, inf rows) and the
   position in the wave, bitwise; n = 1 .. 257 between sentinel pads; obs / obs_copy off 16-B alignment;
   rr_policy_pack_discrete at K = 2 and 4.

Measured (MI355X): in each test's docstring. The whole file runs in 4 s."""
import ctypes

import numpy as np
import pytest

import discrete_ref as D
import discrete_sampler_ref as S
import policy_bound as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64
SENT = -12345.678
GAMMA = 0.99
LANES = (0, 31, 32, 63)
OUTS = ("act_env", "act", "value", "logp", "obs_copy", "reward_out", "start_out")
FIVE = ("act_env", "act", "value", "logp")  # act_env holds two of the five
SETS = {"live": tuple(S.LIVE_ENDS.values()), "shortfall": tuple(z for _, z in S.SHORTFALL),
        "ties": tuple(S.TIES.values()) + S.TIES_DEAD}
_packs, _obs = {}, {}


def _lib_p():
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr

    return _lib, _lib.load(), _ptr


def _pack(pol):
    from rl_rocket_amd.rollout import PolicyPack

    pk = PolicyPack(pol, 7, pol.n_choices, DEV)
    pk.pack()
    return pk


def _const(z):
    """(policy on the device, its pack) of a constant-logit set, built once."""
    if z not in _packs:
        pol = S.const_policy(z, DEV)
        _packs[z] = (pol, _pack(pol))
    return _packs[z]


def _randn(n, seed=0, scale=1.0):
    import torch

    if (n, seed, scale) not in _obs:
        _obs[(n, seed, scale)] = (scale * torch.randn((n, 7), generator=torch.Generator().manual_seed(seed))).to(DEV)
    return _obs[(n, seed, scale)]


def _padded(n, cols):
    import torch

    whole = torch.full((n + 2 * PAD,) + ((cols,) if cols else ()), SENT, dtype=torch.float32, device=DEV)
    return whole, whole[PAD:PAD + n]


def _pads_untouched(whole, n):
    import torch

    ref = torch.full_like(whole[:PAD], SENT).view(torch.int32)
    return torch.equal(whole[:PAD].view(torch.int32), ref) and torch.equal(whole[PAD + n:].view(torch.int32), ref)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _act(pk, pol, obs, n, id_off, t=D.ACT_T, boot=None, done=None, ocopy=False, obs_copy_view=None):
    """One rr_policy_act_discrete launch at (ACT_SEED, ACT_ITER, t) on rows < n of obs into sentinel-padded
    outputs: {name: (whole, rows)}. boot = (term_obs, truncated, reward); done: the start flags."""
    import torch

    _lib, lib, p = _lib_p()
    k = pol.n_choices
    out = {"act_env": _padded(n, 2), "act": _padded(n, 0), "value": _padded(n, 0), "logp": _padded(n, 0)}
    if ocopy:
        out["obs_copy"] = _padded(n, 7)
    if obs_copy_view is not None:
        out["obs_copy"] = (obs_copy_view, obs_copy_view)
    if boot is not None:
        out["reward_out"] = _padded(n, 0)
    if done is not None:
        out["start_out"] = _padded(n, 0)
    g = lambda name: p(out[name][1]) if name in out else None  # noqa: E731
    tobs, trunc, rew = boot if boot is not None else (None, None, None)
    it = torch.tensor([D.ACT_ITER], dtype=torch.int64, device=DEV)
    table = (ctypes.c_float * (2 * k))(*pol.table.reshape(-1).tolist())
    _lib.check(lib.rr_policy_act_discrete(p(pk.buf), 7, k, table, 0, n, id_off, p(obs), D.ACT_SEED, p(it), t, g("act_env"),
                                          g("act"), g("value"), g("logp"), g("obs_copy"), p(tobs), p(trunc), p(rew), GAMMA,
                                          g("reward_out"), p(done), g("start_out"), None), "rr_policy_act_discrete")
    torch.cuda.synchronize()
    return out


def _index(t, k):
    """The stored indices as integers; they are whole numbers below k (a head past K is never chosen)."""
    got = t.detach().cpu().numpy()
    idx = got.astype(np.int64)
    assert np.array_equal(got, idx.astype(np.float32)) and idx.min() >= 0 and idx.max() < k, got
    return idx


def _logp_share(z, idx, logp):
    """max |logp - float64| over its bar for constant logits z (dz = 0); inf if a log-prob is not finite."""
    z64 = np.broadcast_to(np.asarray(z, np.float64), (idx.size, len(z)))
    lp64 = np.log(S.probs64(z))[idx.reshape(-1)]
    bar = S.logp_bar(z64, np.zeros_like(z64), idx.reshape(-1))
    return B.worst_ratio(logp.reshape(-1), lp64, bar)


class _Bad:
    """Collects what a sampler test found wrong, so that one run reports every row and case."""

    def __init__(self):
        self.rows, self.cases, self.dead, self.share = 0, [], 0, 0.0

    def check(self, label, z, idx, want, logp=None):
        idx, want = idx.reshape(-1), want.reshape(-1)
        wrong = idx != want
        dead = S.probs64(z)[idx] <= S.DEAD
        self.dead += int(dead.sum())
        if wrong.any() or dead.any():
            self.rows += int((wrong | dead).sum())
            self.cases.append((label, z, idx[wrong | dead].tolist(), want[wrong | dead].tolist()))
        if logp is not None:
            self.share = max(self.share, _logp_share(z, idx, logp))

    def report(self, what):
        print("%s: %d wrong rows in %d launches, %d draws of a dead choice, worst log-prob error / bar %.3f"
              % (what, self.rows, len(self.cases), self.dead, self.share))
        for c in self.cases[:12]:
            print("   ", c)
        assert not self.cases and self.dead == 0, "%s: %d rows, %d launches" % (what, self.rows, len(self.cases))
        assert self.share <= 1.0, (what, self.share)


# ---- a. the sampler --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(SETS))
def test_act_kernel_on_the_committed_draws(group):
    """rr_policy_act_discrete, one 64-row launch per logit set and committed draw with the special row at lane
    0, 31, 32 or 63 (id_off shifted), and an n = 1 launch per logit set and end value: every index is the float64
    reference's and no choice with ex = 0 is drawn; the table row is bitwise the table's; the log-prob of the
    stored index is finite and inside its bar.

    Measured (MI355X): before the dead-choice guard (categorical_index, rocket_device.h) the shortfall group
    failed on 55 rows in 55 launches: each of the 10 logit sets on the 4 draws at r = 2^24 - 1 and one set on the 4
    at r = 2^24 - 2 too (44 launches of 64 rows, the special row alone wrong, e.g. index 3 for 1 at [0, -1.8, -120,
    -120], stored with a log-prob of -120), and the 11 n = 1 launches at those draws; live and ties passed. With
    the guard 0 rows. Worst log-prob error / bar 0.21 (shortfall), 0.076 (live), 0.004 (ties)."""
    import torch

    bad = _Bad()
    obs = _randn(64)
    for z in SETS[group]:
        pol, pk = _const(z)
        k, tab = len(z), pol.table.cpu()
        for i, (id_off, t, r) in enumerate(S.ACT_DRAWS):
            lane = LANES[i % 4]
            for n, off in ((64, id_off - lane),) + (((1, id_off),) if i % 4 == 0 and r in S.R_ENDS else ()):
                out = _act(pk, pol, obs, n, off, t)
                idx = _index(out["act"][1], k)
                assert idx.shape == (n,)
                bad.check("r %d lane %d n %d" % (r, lane, n), z, idx, S.live_ref(z, S.act_u(n, off, t)), _np(out["logp"][1]))
                assert torch.equal(out["act_env"][1].cpu(), tab[torch.from_numpy(idx)]), (z, r)
                assert all(_pads_untouched(out[name][0], n) for name in out), (z, r)
    bad.report("act, " + group)


def test_constant_logits_do_not_depend_on_the_obs():
    """The derivation behind const_policy, on the device: two obs batches (N(0, 1) and 90 N(0, 1)) give the
    same bits in the index, the table row and the log-prob, and different values."""
    import torch

    z = S.SHORTFALL[0][1]
    pol, pk = _const(z)
    a = _act(pk, pol, _randn(257, 1), 257, S.EDGE_ID_OFF)
    b = _act(pk, pol, _randn(257, 2, 90.0), 257, S.EDGE_ID_OFF)
    for name in ("act", "act_env", "logp"):
        assert np.array_equal(_bits(a[name][1]), _bits(b[name][1])), name
    assert not torch.equal(a["value"][1], b["value"][1])
    lp64 = np.log(S.probs64(z))
    lp = np.unique(_np(a["logp"][1]))
    assert len(lp) == 2 and np.abs(lp - lp64[:2][::-1]).max() < 1e-6  # z_a - z_max - lse of exact logits


@pytest.mark.parametrize("group", list(SETS))
def test_step_kernel_on_the_committed_draws(group):
    """rr_rollout_step_discrete at (ACT_SEED, ACT_ITER, ACT_T) on 64-env 3DOF batches whose env_id_offset puts
    the special env at lane 0, 31, 32 or 63: as the act kernel's test, on the stored index and log-prob.

    Measured (MI355X): before the guard the shortfall group failed on 44 rows in 44 launches, the act kernel's 64-row
    ones; with it 0 rows. Log-prob shares as the act kernel's."""
    import torch
    from rl_rocket_amd.batch import RocketBatch

    _lib, lib, p = _lib_p()
    bad = _Bad()
    f = dict(dtype=torch.float32, device=DEV)
    bufs = [torch.zeros((64, 7), **f)] + [torch.zeros(64, **f) for _ in range(5)]
    it = torch.tensor([D.ACT_ITER], dtype=torch.int64, device=DEV)
    envs = [RocketBatch(64, model=3, device=DEV, max_episode_steps=1000, seed=77, env_id_offset=id_off - LANES[i % 4])
            for i, (id_off, t, r) in enumerate(S.ACT_DRAWS)]
    for env in envs:
        env.reset()
    for z in SETS[group]:
        pol, pk = _const(z)
        k = len(z)
        table = (ctypes.c_float * (2 * k))(*pol.table.reshape(-1).tolist())
        for env, (id_off, t, r) in zip(envs, S.ACT_DRAWS):
            bufs[1].fill_(-7.0)
            _lib.check(lib.rr_rollout_step_discrete(env._h, p(pk.buf), k, table, 0, D.ACT_SEED, p(it), t, GAMMA,
                                                    *[p(b) for b in bufs], p(env.obs), p(env.reward), p(env.done),
                                                    p(env.truncated), None, None), "rr_rollout_step_discrete")
            torch.cuda.synchronize()
            idx = _index(bufs[1], k)
            bad.check("r %d id_off %d" % (r, env.env_id_offset), z, idx, S.live_ref(z, S.act_u(64, env.env_id_offset, t)),
                      _np(bufs[3]))
    for env in envs:
        env.close()
    bad.report("per-step, " + group)


def _by_k(zs):
    out = {}
    for z in zs:
        out.setdefault(len(z), []).append(z)
    return out


def _set_bias(pol, z):
    import torch

    with torch.no_grad():
        pol.action_net.bias.copy_(torch.tensor(z, dtype=torch.float32))


@pytest.mark.parametrize("group", list(SETS))
def test_one_launch_collect_on_the_committed_draws(group):
    """rr_rollout_collect_discrete through DeviceRollout(one_launch=True), 64 envs x 8 steps under the committed
    seeds at iter 0: all 512 stored indices of every call are the float64 reference's, the special (env, t)
    among them, and the stored log-probs are inside their bar.

    Measured (MI355X): before the guard the shortfall group failed on 44 rows in 44 calls (the special (env, t) of
    every call at r = 2^24 - 1, of one logit set at 2^24 - 2 too); with it 0 rows of the 112 640."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.rollout import DeviceRollout

    bad = _Bad()
    us = {seed: S.collect_u(seed) for seed, _, _, _ in S.COLLECT_DRAWS}
    for k, zs in _by_k(SETS[group]).items():
        pol = S.const_policy(zs[0], DEV)
        env = RocketBatch(S.N_ENVS, model=3, device=DEV, max_episode_steps=1000, seed=77)
        ro = DeviceRollout(env, pol, n_steps=S.N_STEPS, one_launch=True)
        assert ro.discrete and ro.one_launch and not ro.per_step
        for z in zs:
            _set_bias(pol, z)
            for seed, e, t, r in S.COLLECT_DRAWS:
                ro.seed = seed
                ro.iter.zero_()
                ro.actions.fill_(-7.0)
                ro.collect()
                torch.cuda.synchronize()
                idx = _index(ro.actions[..., 0], k)
                want = S.live_ref(z, us[seed].reshape(-1)).reshape(S.N_STEPS, S.N_ENVS)
                assert us[seed][t, e] == r * 2.0 ** -24
                bad.check("r %d seed %d" % (r, seed), z, idx, want, _np(ro.log_probs))
        env.close()
    bad.report("one-launch collect, " + group)


@pytest.mark.parametrize("group", list(SETS))
def test_sampled_evaluation_on_the_committed_draws(group):
    """rr_policy_evaluate_discrete_sampled recording all 64 envs for 8 steps from a fresh reset under the
    committed seeds: the recorded choices are the float64 reference's and the recorded action rows are bitwise
    the table's.

    Measured (MI355X): before the guard the shortfall group failed on 44 rows in 44 calls, as the collect; with it
    0 rows."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.rollout import PolicyEvaluator

    bad = _Bad()
    us = {seed: S.collect_u(seed) for seed, _, _, _ in S.COLLECT_DRAWS}
    for k, zs in _by_k(SETS[group]).items():
        pol = S.const_policy(zs[0], DEV)
        env = RocketBatch(S.N_ENVS, model=3, device=DEV, max_episode_steps=1000, seed=77)
        ev = PolicyEvaluator(env, pol, n_episodes=1, max_steps=S.N_STEPS, fused=True, record=list(range(S.N_ENVS)),
                             record_steps=S.N_STEPS, deterministic=False, seed=0)
        tr = ev.trace
        for z in zs:
            _set_bias(pol, z)
            for seed, e, t, r in S.COLLECT_DRAWS:
                env.reset()
                ev.seed = seed
                ev.iter.zero_()
                tr.choice.fill_(-7)
                ev.run()
                torch.cuda.synchronize()
                choice = tr.choice[:, 0, :].T.cpu().numpy().astype(np.int64)  # [t][env]
                assert choice.min() >= 0 and choice.max() < k, (z, seed)
                want = S.live_ref(z, us[seed].reshape(-1)).reshape(S.N_STEPS, S.N_ENVS)
                bad.check("r %d seed %d" % (r, seed), z, choice, want)
                assert torch.equal(tr.action[:, 0], pol.table[tr.choice[:, 0].long()]), (z, seed)
        env.close()
    bad.report("sampled evaluation, " + group)


@pytest.mark.parametrize("k", [4, 2, 3])
def test_every_bit_of_u(k):
    """One 65 536-row act launch with equal logits. K = 4 and 2: the running sums k / K are exact, every index is
    floor(K u) of uniform_ref, no row left out. K = 3: every index is the float64 reference's outside the rows
    within 2^-22 of a running sum, at most 4 (counted on the CPU: 0). A comparator turned round, a u of half the
    range or a swapped key stage fails thousands of rows.

    Measured (MI355X): 0 rows differ at every K."""
    z = S.TIES[k] if k != 3 else S.EQUAL3
    pol, pk = _const(z)
    n = S.N_BITS
    out = _act(pk, pol, _randn(n, 3), n, 0)
    idx = _index(out["act"][1], k)
    u = S.act_u(n, 0)
    if k == 3:
        c = np.cumsum(S.probs64(z))[:-1]
        knife = (np.abs(u[:, None] - c[None, :]) < S.KNIFE3).any(1)
        assert knife.sum() <= S.KNIFE3_ROWS
        want = S.live_ref(z, u)
    else:
        knife, want = np.zeros(n, bool), np.floor(k * u).astype(np.int64)
    print("K %d: %d of %d rows differ, %d knife rows" % (k, (idx != want)[~knife].sum(), n, knife.sum()))
    assert np.array_equal(idx[~knife], want[~knife])
    assert np.bincount(idx, minlength=k).min() > n // (2 * k)
    assert _pads_untouched(out["act"][0], n) and _pads_untouched(out["act_env"][0], n)


# ---- b. the act kernel at its domain edges ---------------------------------------------------------------------
_edge_packs = {}


def _edge_pack(k, ws):
    if (k, ws) not in _edge_packs:
        pol = S.cat_weight_set(ws, k).to(DEV)
        _edge_packs[(k, ws)] = (pol, _pack(pol))
    return _edge_packs[(k, ws)]


def _cuda(x, dtype=None):
    import torch

    return torch.as_tensor(x, dtype=dtype).to(DEV).contiguous()


@pytest.mark.parametrize("k", S.EDGE_K)
def test_forward_stays_inside_the_fp64_bound(k):
    """Every row of 3 weight sets x 6 obs classes at 257 rows: the value inside forward_bound's value bound, the
    log-prob of the stored index within 2 max dz + 2^-24 (2 |z_a - z_max| + 2 |lse| + 12) of float64, and, on the
    cases discrete_sampler_ref.INDEX_ADMITTED names (the others have more than 1 % knife-edge rows under the
    worst-case bound), the index equal to float64's outside the knife-edge rows. Prints the worst share per case.

    Measured (MI355X), largest err / bound over the obs classes as value / log-prob: K = 4 suite 5.2e-4 / 3.0e-4,
    saturated 2.0e-4 / 7.8e-5, constant 8.0e-5 / 6.5e-4; K = 2 suite 8.3e-4 / 2.8e-4, saturated 3.5e-4 / 5.0e-5,
    constant 2.2e-4 / 1.2e-4 (the worst-case bound is three orders above the kernel, as for the Gaussian policy).
    The index differed from float64's on no row of any of the 36 cases, admitted or not."""
    for ws in S.WEIGHT_SETS:
        pol, pk = _edge_pack(k, ws)
        for oc in S.EDGE_OBS:
            c = S.edge_case(k, ws, oc)
            out = _act(pk, pol, _cuda(c.obs), S.EDGE_N, S.EDGE_ID_OFF)
            idx = _index(out["act"][1], k)
            r = np.arange(S.EDGE_N)
            rv = B.worst_ratio(_np(out["value"][1]), c.v64, c.dv)
            rl = B.worst_ratio(_np(out["logp"][1]), c.lp64[r, idx], S.logp_bar(c.z64, c.dz, idx))
            differ = int((idx != c.ref).sum())
            print("K %d %-9s %-11s err/bound value %.2e log_prob %.2e | %d rows differ from float64, %d knife-edge"
                  % (k, ws, oc, rv, rl, differ, c.knife.sum()))
            assert rv <= 1.0 and rl <= 1.0, (k, ws, oc, rv, rl)
            if (k, ws, oc) in S.INDEX_ADMITTED:
                assert c.knife.mean() <= D.KNIFE_CAP
                assert np.array_equal(idx[~c.knife], c.ref[~c.knife]), (k, ws, oc)
                assert (np.abs(idx[c.knife] - c.ref[c.knife]) <= 1).all()
            assert (out["act_env"][1].cpu().numpy() == np.asarray(D.TABLES[k], np.float32)[idx]).all()


def test_peaked_logits():
    """Constant logits [80, 0, -80, -120], [-60, -60.5, -61, -61.5] and all-equal +-80 at 257 rows: log-probs
    finite and inside the bar, the index the reference's (floor(4 u) for the equal sets; outside the rows within
    discrete_ref.KNIFE of a running sum, at most 1 %, for the second).

    Measured (MI355X): worst log-prob error / bar 0.071 ([-60, -60.5, -61, -61.5]), 0.004 at the equal sets and
    0.000 at [80, 0, -80, -120]; no index differs and no row is knife-edge."""
    n = S.EDGE_N
    u = S.act_u(n, S.EDGE_ID_OFF)
    for z in S.PEAKED:
        pol, pk = _const(z)
        out = _act(pk, pol, _randn(n, 4), n, S.EDGE_ID_OFF)
        idx = _index(out["act"][1], 4)
        logp = _np(out["logp"][1])
        share = _logp_share(z, idx, logp)
        if len(set(z)) == 1:
            want, knife = np.floor(4 * u).astype(np.int64), np.zeros(n, bool)
        else:
            lp = np.log(np.broadcast_to(S.probs64(z), (n, 4)))
            want, knife, _ = D.act_ref(lp, u)
            assert np.array_equal(S.live_ref(z, u)[~knife], want[~knife])
        print("peaked %s: log-prob error / bar %.3f, %d knife rows, %d differ" % (z, share, knife.sum(), (idx != want).sum()))
        assert np.isfinite(logp).all() and share <= 1.0, (z, share)
        assert knife.mean() <= D.KNIFE_CAP and np.array_equal(idx[~knife], want[~knife]), z
    z = S.PEAKED[0]
    assert (S.live_ref(z, u) == 0).all()  # [80, 0, -80, -120]: p_0 = 1 - 2e-35


def test_row_outputs_do_not_depend_on_position_or_neighbours():
    """One obs row, with its env id kept (id_off shifted), at rows 0, 31, 32, 63, 64 and 256 of a 257-row batch
    whose other rows are zeros, 1e6, or hold NaN / +inf / -inf: its table row, index, value and log-prob have the
    same bits in all 24 places, at K = 4 and K = 2."""
    where = [0, 31, 32, 63, 64, 256]
    n, ident = S.EDGE_N, 5000
    rng = np.random.default_rng(61)
    probe = rng.standard_normal(7).astype(np.float32)
    r = np.arange(n)
    bad = rng.standard_normal((n, 7)).astype(np.float32)
    bad[r, r % 7] = np.asarray([np.nan, np.inf, -np.inf], np.float32)[r % 3]
    batches = {"zeros": np.zeros((n, 7), np.float32), "1e6": np.full((n, 7), 1e6, np.float32), "nonfinite": bad,
               "inf": np.full((n, 7), np.inf, np.float32)}
    for k in S.EDGE_K:
        pol, pk = _edge_pack(k, "suite")
        first = None
        for name, x in batches.items():
            for w in where:
                x = x.copy()
                x[w] = probe
                out = _act(pk, pol, _cuda(x), n, ident - w)
                got = [_bits(out[key][1][w]) for key in FIVE]
                assert all(np.isfinite(out[key][1][w].cpu().numpy()).all() for key in FIVE)
                if first is None:
                    first = got
                for key, a, b in zip(FIVE, got, first):
                    assert np.array_equal(a, b), (k, name, w, key)
                x[w] = batches[name][w]


def _edge_inputs(seed=3):
    """Inputs of 257 rows inside allocations padded by PAD finite rows on both sides."""
    import torch

    g = torch.Generator().manual_seed(seed)
    tot = S.EDGE_N + 2 * PAD
    obs = (2 * torch.randn((tot, 7), generator=g)).to(DEV)
    tobs = torch.randn((tot, 7), generator=g).to(DEV)
    trunc = (torch.rand((tot,), generator=g) < 0.3).to(torch.uint8).to(DEV)
    done = (torch.rand((tot,), generator=g) < 0.3).to(torch.uint8).to(DEV)
    rew = torch.randn((tot,), generator=g).to(DEV)
    return tuple(t[PAD:PAD + S.EDGE_N] for t in (obs, tobs, trunc, rew, done))


@pytest.mark.parametrize("k", S.EDGE_K)
def test_shape_edges_write_nothing_outside_their_rows(k):
    """n = 1, 63, 64, 65, 255, 256, 257 with every optional output: act_env, act, value, logp, obs_copy,
    reward_out and start_out sit between 64-row sentinel pads, which keep their bits; rows < n are bitwise those
    of the n = 257 call."""
    import torch

    pol, pk = _edge_pack(k, "suite")
    obs, tobs, trunc, rew, done = _edge_inputs()
    kw = dict(boot=(tobs, trunc, rew), done=done, ocopy=True)
    full = _act(pk, pol, obs, S.EDGE_N, S.EDGE_ID_OFF, **kw)
    assert torch.equal(full["obs_copy"][1], obs) and torch.equal(full["start_out"][1], done.float())
    assert len(set(_index(full["act"][1], k).tolist())) == k
    for name in OUTS:
        assert torch.isfinite(full[name][1]).all(), name
    for n in (1, 63, 64, 65, 255, 256, 257):
        o = _act(pk, pol, obs, n, S.EDGE_ID_OFF, **kw)
        for name in OUTS:
            whole, rows = o[name]
            assert _pads_untouched(whole, n), (n, name)
            assert np.array_equal(_bits(rows), _bits(full[name][1][:n])), (n, name)


@pytest.mark.parametrize("k", S.EDGE_K)
def test_unaligned_obs_pointers_give_the_same_bits(k):
    """obs, then obs_copy, 4 bytes past a 16-B boundary at n = 257 and 256 (rr_policy_act_discrete admits them, as
    rr_policy_act does: stage_obs leaves its 16-B path): every output has the bits of the aligned call and the
    sentinels around the unaligned obs_copy hold."""
    import torch

    pol, pk = _edge_pack(k, "suite")
    obs, tobs, trunc, rew, done = _edge_inputs(seed=4)

    def off4(t):
        flat = torch.full((t.numel() + 8,), SENT, device=DEV)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return flat, v

    for n in (257, 256):
        kw = dict(boot=(tobs, trunc, rew), done=done)
        ref = _act(pk, pol, obs, n, S.EDGE_ID_OFF, ocopy=True, **kw)
        assert obs.data_ptr() % 16 == 0 and ref["obs_copy"][1].data_ptr() % 16 == 0
        _, obs_u = off4(obs[:n])
        a = _act(pk, pol, obs_u, n, S.EDGE_ID_OFF, ocopy=True, **kw)
        flat, oc_u = off4(torch.full((n, 7), SENT, device=DEV))
        b = _act(pk, pol, obs, n, S.EDGE_ID_OFF, obs_copy_view=oc_u, **kw)
        assert flat[0].item() == np.float32(SENT) and bool((flat[1 + n * 7:] == np.float32(SENT)).all())
        for res in (a, b):
            for name in OUTS:
                assert np.array_equal(_bits(res[name][1]), _bits(ref[name][1])), (n, name)


@pytest.mark.parametrize("k", [2, 4])
def test_pack_is_the_reference_layout(k):
    """rr_policy_pack_discrete at K = 2 and 4 (K = 3: tests/test_gpu_discrete.py) equals pack_reference() bitwise,
    with zeros for the heads past K."""
    import torch

    pol = D.cat_policy(k, 7).to(DEV)
    pk = _pack(pol)
    got = pk.buf.clone()
    pk.buf.fill_(0.0)
    ref = pk.pack_reference().clone()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    o = pk.off
    assert bool((got[o["HA"]:o["HA"] + k * 64] != 0).all()) and bool((got[o["HB"]:o["HB"] + k] != 0).all())
    assert bool((got[o["HA"] + k * 64:o["HV"]] == 0).all()) and bool((got[o["HB"] + k:o["VB"]] == 0).all())
    assert o["HV"] - o["HA"] == 4 * 64 and o["VB"] - o["HB"] == 4
