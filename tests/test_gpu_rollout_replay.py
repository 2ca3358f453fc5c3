"""The on-device PPO rollout against independent fp64 references (tests/rollout_ref.py), where
tests/test_gpu_rollout.py compares its three launch paths with one another:

a. every action-noise draw, element by element, against the NumPy restatement of the documented
   key (seed words with bits above 2^32, *iter above 2^32, env ids that wrap the 32-bit cast);
b. a rollout sharded by env_id_offset against the one-batch rollout, bitwise;
c. ten consecutive collects replayed row by row through the CPU oracle: next obs, rewards with
   the timeout bootstrap on truncated rows only, episode-start flags, values, log-probs,
   actions and GAE.

All sizes n = 4096 + 37 (a ragged last wave). Measured maxima (MI355X): in each test's docstring."""
import numpy as np
import pytest

import rollout_ref as R
from gpu_util import TOL_STATE

pytestmark = pytest.mark.gpu

N = 4096 + 37
PREC = {"fp32": 0, "bf16": 1, "fp16x3": 2}
TOL_DRAW = 1e-3   # a mis-keyed draw differs by O(1) on all but ~1e-3 of the elements
PATHS = {"one_launch": dict(one_launch=True, per_step=False), "per_step": dict(one_launch=True, per_step=True),
         "two_launch": dict(one_launch=False, per_step=True)}


def _zero_head_policy(ns, na):
    """action_net and log_std zero: mean 0, std 1, so the stored unclipped actions are the draws."""
    import torch

    pol = R.scaled_policy(ns, na, seed=9, device="cuda:0")
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.zero_()
        pol.log_std.zero_()
    return pol


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16x3"])
@pytest.mark.parametrize("ns,na", [(14, 3), (7, 2)])
def test_policy_act_draws_match_noise_ref(ns, na, prec):
    """rr_policy_act's draws against noise_ref on every element, over env_id_offset {0, 70 000,
    2^32 - 20 (wraps inside the batch)} x seed {11, (7 << 32) | 5} x *iter {3, 2^32 + 3} x t {0, 36}.
    Bar 1e-3: the fast intrinsics' (__logf, __sincosf, v_sqrt) own error; measured max
    1.75e-6 at (14, 3), 1.52e-6 at (7, 2), the same for the three precisions (MI355X). The action fed to the env is clip(actions, -1, 1), bitwise."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout import PolicyPack

    lib = _lib.load()
    dev = torch.device("cuda:0")
    pol = _zero_head_policy(ns, na)
    params = PolicyPack(pol, ns, na, dev, precision=prec).pack()
    obs = torch.randn((N, ns), device=dev, generator=torch.Generator(dev).manual_seed(1))
    act_env, act = torch.empty((N, na), device=dev), torch.empty((N, na), device=dev)
    val, lp = torch.empty((N,), device=dev), torch.empty((N,), device=dev)
    worst = 0.0
    for id_off in (0, 70000, 2 ** 32 - 20):
        for seed in (11, (7 << 32) | 5):
            for itv in (3, (1 << 32) + 3):
                it = torch.tensor([itv], dtype=torch.int64, device=dev)
                for t in (0, 36):
                    _lib.check(lib.rr_policy_act(_ptr(params), ns, na, PREC[prec], N, id_off, _ptr(obs), seed, _ptr(it), t,
                                                 _ptr(act_env), _ptr(act), _ptr(val), _ptr(lp), None, None, None, None,
                                                 0.0, None, None, None, None), "rr_policy_act")
                    torch.cuda.synchronize()
                    got = act.cpu().numpy().astype(np.float64)
                    err = np.abs(got - R.noise_ref(N, id_off, seed, itv, t, na)).max()
                    worst = max(worst, err)
                    assert err <= TOL_DRAW, (id_off, seed, itv, t, err)
                    assert torch.equal(act_env, act.clamp(-1, 1))
    print("rr_policy_act", (ns, na), prec, "max |draw - noise_ref|", worst)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("model", [6, 3])
def test_rollout_draws_match_noise_ref(model, path):
    """DeviceRollout's draws on each launch path: env_id_offset 70 000, T = 37, seed (7 << 32) | 5,
    the iteration counter started at 2^32 + 3, two collects; every [t] slice against noise_ref
    within 1e-3 (measured max 1.87e-6 on every path, MI355X)."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import DeviceRollout

    T, id_off, seed, it0 = 37, 70000, (7 << 32) | 5, (1 << 32) + 3
    ns, na = (14, 3) if model == 6 else (7, 2)
    env = RocketBatch(N, model=model, device="cuda:0", max_episode_steps=6, env_id_offset=id_off,
                      **(ENV_CONFIG_6DOF if model == 6 else {}))
    ro = DeviceRollout(env, _zero_head_policy(ns, na), n_steps=T, seed=seed, **PATHS[path])
    ro.iter.fill_(it0)
    worst = 0.0
    for c in range(2):
        ro.collect()
        torch.cuda.synchronize()
        got = ro.actions.cpu().numpy().astype(np.float64)
        for t in range(T):
            err = np.abs(got[t] - R.noise_ref(N, id_off, seed, it0 + c, t, na)).max()
            worst = max(worst, err)
            assert err <= TOL_DRAW, (c, t, err)
    assert int(ro.iter.item()) == it0 + 2
    print("DeviceRollout", model, path, "max |draw - noise_ref|", worst)
    env.close()


@pytest.mark.parametrize("path", ["one_launch", "two_launch"])
@pytest.mark.parametrize("model", [6, 3])
def test_sharded_rollout_is_bitwise_one_batch(model, path):
    """Three uneven shards (dist.shard: 1378 + 1378 + 1377 envs at offsets 0, 1378, 2756) with the
    same seed and policy, TimeLimit 6, T = 8, two collects: every rollout buffer, last_* and the
    env state equal the slices of the one-batch collect (noise and resets keyed on global ids)."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.dist import shard
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import DeviceRollout

    T, seed = 8, (3 << 32) | 21
    ns, na = (14, 3) if model == 6 else (7, 2)
    kw = ENV_CONFIG_6DOF if model == 6 else {}
    pol = R.scaled_policy(ns, na, seed=3, head_scale=1.0, device="cuda:0")

    def make(n, off):
        env = RocketBatch(n, model=model, device="cuda:0", max_episode_steps=6, env_id_offset=off, **kw)
        return DeviceRollout(env, pol, n_steps=T, seed=seed, **PATHS[path])

    whole = make(N, 0)
    parts = [(make(*shard(N, 3, r)), shard(N, 3, r)) for r in range(3)]
    assert sorted({p[1][0] for p in parts}) == [N // 3, N // 3 + 1] and sum(p[1][0] for p in parts) == N
    for _ in range(2):
        whole.collect()
        for ro, _s in parts:
            ro.collect()
        torch.cuda.synchronize()
        for ro, (n, off) in parts:
            for name in ("obs", "actions", "values", "log_probs", "starts", "rewards", "advantages", "returns"):
                assert torch.equal(getattr(ro, name), getattr(whole, name)[:, off:off + n]), (name, off)
            for name in ("last_value", "last_done", "last_start"):
                assert torch.equal(getattr(ro, name), getattr(whole, name)[off:off + n]), (name, off)
            for name in ("obs", "reward", "done", "truncated"):
                assert torch.equal(getattr(ro.env, name), getattr(whole.env, name)[off:off + n]), (name, off)
            for x, y in zip(ro.env.get_state(), whole.env.get_state()):
                assert torch.equal(x, y[..., off:off + n]), off
    assert whole.starts[1:].sum() > 0
    for ro in [whole] + [p[0] for p in parts]:
        ro.env.close()


TIME_LIMIT, T_REPLAY, COLLECTS = 80, 16, 10
MIN_EVENTS = 200
MAX_MISMATCH = 1e-5  # of the replayed rows


@pytest.fixture(scope="module", params=[(6, "fp32"), (6, "fp16x3"), (6, "unfused"), (3, "fp32"), (3, "fp16x3")],
                ids=lambda p: "%dDOF-%s" % p)
def replayed(request, oracle_mod):
    """Ten consecutive collects (T = 16, TimeLimit 80: 661 280 rows) of one model and path (the
    default one-launch fp32 collect, its fp16x3 towers, or the PyTorch path fused=False), replayed
    row by row once for the tests below: each row restarts from the collect's own
    obs[t] * normalizer in float64 and is stepped by the oracle (fp64 RK45) with clip(actions[t]),
    t_in = elapsed * dt and the episode's ic, both carried from the collect's own starts flags."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF, make_config
    from rl_rocket_amd.rollout import DeviceRollout

    model, path = request.param
    kw = ENV_CONFIG_6DOF if model == 6 else {}
    ec = make_config(model, **kw)
    ns, na = ec.state_dim, ec.action_dim
    cfg = oracle_mod.make_cfg(model, **(oracle_mod.ENV_CONFIG_6DOF if model == 6 else oracle_mod.DEFAULTS_3DOF))
    seed = (7 << 32) | 5
    pol = R.scaled_policy(ns, na, seed=5, device="cuda:0")
    pol64 = R.policy64(pol)
    env = RocketBatch(N, model=model, device="cuda:0", max_episode_steps=TIME_LIMIT, **kw)
    if path == "unfused":
        ro = DeviceRollout(env, pol, n_steps=T_REPLAY, fused=False,
                           generator=torch.Generator("cuda:0").manual_seed(4))
    else:
        ro = DeviceRollout(env, pol, n_steps=T_REPLAY, seed=seed, policy_dtype=path)
        assert ro.one_launch and not ro.per_step
    snaps = []
    for _ in range(COLLECTS):
        ro.collect()
        snaps.append(R.snapshot(ro))
    env.close()

    carry = R.new_carry(N, ns)
    keys = ("obs", "reward", "value", "last_value", "logp", "adv", "ret", "adv_rel", "ret_rel") + \
        (("action",) if ro.fused else ())
    worst = dict.fromkeys(keys, 0.0)
    tot = dict.fromkeys(("rows", "events", "bounds", "natural", "truncated", "marginal", "reset_bad", "reward_over",
                         "reset_rows"), 0)
    mism, G, amax = [], 0.0, 0.0
    for it, s in enumerate(snaps):
        r = R.replay_collect(oracle_mod, cfg, s, carry, pol64, TIME_LIMIT, gamma=ro.gamma, lam=ro.lam,
                             ic_low=ec.ic_low, ic_high=ec.ic_high, noise=(0, seed, it) if ro.fused else None)
        for k in keys:
            worst[k] = max(worst[k], float(r[k].max()))
        for k in tot:
            tot[k] += r[k]
        mism += [(it, int(t), int(e)) for t, e in r["mismatch_rows"]]
        G, amax = max(G, r["G"]), max(amax, r["adv_abs_max"])
    print("replay", model, path, "max errors", {k: "%.3g" % v for k, v in worst.items()}, "counts", tot,
          "G %.3g max |A| %.4g" % (G, amax), "flag mismatches", mism)
    return {"worst": worst, "tot": tot, "mism": mism, "fused": ro.fused}


def test_replay_flags_next_obs_resets_and_rewards(replayed):
    """starts[t + 1] (last_done after the last step) is the oracle's done-or-truncated (truncated:
    not done and elapsed + 1 == 80); next obs within 1e-5 (floored relative, theta on the circle)
    on rows that go on; reset rows inside the init space; rewards = oracle reward +
    gamma V64(oracle terminal obs) on truncated rows and only those, within 1e-5 max(|ref|, 1)
    (+ gamma (2e-5 + G 1e-5) where truncated, G = max L1 norm of grad V64 over those rows). At least
    200 ground events, bounds ends and truncations each. Flag mismatches between the fp32 RK4 and
    the fp64 RK45: at most 1e-5 of the rows (6), each marginal (one of 8 oracle re-steps perturbed
    by <= 1e-6 relative gives the GPU's flags).
    Measured (MI355X), 6DOF / 3DOF: 0 flag mismatches of 661 280 rows on every path; next obs
    <= 1.51e-7 / 1.74e-7; reward error <= 3.1e-6 / 6.5e-6 (G 21.4 / 7.7); ground events 297-311 /
    3 735, bounds ends 4 724-4 730 / 360, truncations 3 340-3 353 / 4 191."""
    tot, worst, mism = replayed["tot"], replayed["worst"], replayed["mism"]
    assert tot["rows"] == COLLECTS * T_REPLAY * N
    assert min(tot["events"], tot["bounds"], tot["truncated"]) >= MIN_EVENTS, tot
    assert len(mism) <= int(MAX_MISMATCH * tot["rows"]), mism
    assert tot["marginal"] == len(mism), (tot["marginal"], mism)
    assert tot["reset_bad"] == 0 and tot["reset_rows"] >= tot["natural"] + tot["truncated"] - len(mism)
    assert worst["obs"] <= TOL_STATE, worst
    assert tot["reward_over"] == 0, (tot["reward_over"], worst["reward"])


def test_replay_values_log_probs_and_actions(replayed):
    """values / last_value against V64(obs) within 2e-5 (the suite's TOL); log_probs against the
    fp64 log-density of the stored actions under the fp64 mean within 5e-4; on the fused paths
    actions against mean64(obs[t]) + std * noise_ref within 1e-3 (the keying at a real std, seed
    and rollout counter through DeviceRollout).
    Measured (MI355X): values 4.3e-6 (fp32), 2.0e-6 (fp16x3), 2.7e-6 (PyTorch path); log-probs
    <= 2.2e-6; actions <= 1.6e-6."""
    worst = replayed["worst"]
    assert worst["value"] <= 2e-5 and worst["last_value"] <= 2e-5, worst
    assert worst["logp"] <= 5e-4, worst
    if replayed["fused"]:
        assert worst["action"] <= TOL_DRAW, worst


def test_replay_gae_on_the_envs_scale(replayed):
    """advantages / returns against the fp64 GAE scan of the collect's own rewards, values, starts,
    last_value, last_done, relative to each env's scale S = max(1, max_t |A| + |V| + |r|): within
    96 * 2^-24 = 5.7e-6 (rollout_ref.GAE_REL_BAR: six fp32 roundings per step at magnitudes <= S,
    16 steps, gamma lambda <= 1 amplifies nothing). A wrong mask or a shifted slice is O(1) of S.
    Measured (MI355X): <= 5.5e-8 on every path (4.4e-7 with the fp32 scan this replay replaced)."""
    worst = replayed["worst"]
    assert worst["adv_rel"] <= R.GAE_REL_BAR and worst["ret_rel"] <= R.GAE_REL_BAR, worst


def test_replay_gae_absolute(replayed):
    """The same comparison at test_policy_bootstrap_and_gae's absolute 1e-5. Terminal rewards of
    +-60 make |A| reach 136 (6DOF) / 162 (3DOF), where one fp32 rounding is up to 7.63e-6: the bar
    needs the scan in fp64 with each stored value rounded once (gae_env, DeviceRollout._gae) and
    gamma, lambda as doubles. An fp32 scan measured 3.5e-5 - 5.4e-5 on these collects, an fp64 scan
    with 0.99f / 0.95f 1.07e-5.
    Measured (MI355X): advantages and returns <= 7.63e-6 on every path."""
    worst = replayed["worst"]
    assert worst["adv"] <= 1e-5 and worst["ret"] <= 1e-5, worst
