"""rr_rollout_collect_discrete_stats / DeviceRollout(batch, categorical_policy, one_launch=True, stats=True):
the Categorical policy's one-launch collect that also accounts for the episodes it finishes.

As tests/test_gpu_collect_stats.py for the Gaussian policy, whose helpers, sizes (T = 16, TimeLimit 5, three
collects in a row) and bounds this file uses: the collect itself is bitwise rr_rollout_collect_discrete
(buffers, env outputs, the handle's state), and the statistics block equals what a per-step loop of
rr_rollout_step_discrete on a twin handle sees when it is read after every step. The policy is
discrete_ref.cat_policy. The int64 slots and the fp32 extremes are exact; an fp64 sum of K terms is held
to K * 2^-52 * sum|term| (that file's docstring)."""
import ctypes
import functools

import numpy as np
import pytest

import test_gpu_collect_stats as G

pytestmark = pytest.mark.gpu

DEV, T, TL, SEED = G.DEV, G.T, G.TL, G.SEED


def _policy(k=4):
    from discrete_ref import cat_policy

    return cat_policy(k, 100 + k).to(DEV)


def _env(n, integrator="rk4", **over):
    return G._env(3, n, integrator, **over)


def _ro(env, pol, stats=False, per_step=False):
    from rl_rocket_amd.rollout import DeviceRollout

    ro = DeviceRollout(env, pol, n_steps=T, seed=SEED, one_launch=True, per_step=per_step, stats=stats)
    assert ro.discrete and ro.fused and ro.one_launch and ro.per_step == per_step
    return ro


# ---- 1. the collect is rr_rollout_collect_discrete's, bit for bit ----

@pytest.mark.parametrize("k,integrator,annealing", [(2, "rk4", False), (3, "rk4", False), (4, "rk4", False),
                                                    (2, "euler", False), (3, "euler", False), (4, "euler", False),
                                                    (4, "rk4", True)])
def test_collect_is_bitwise_the_plain_collect(k, integrator, annealing):
    """n = 300 (four full waves, one wave of 44 envs, three dead waves in the last workgroup), three collects
    in a row: every env finishes three episodes per collect and episodes straddle the collect boundary."""
    import torch
    from rl_rocket_amd import _lib

    pol = _policy(k)
    a = _ro(_env(300, integrator, reward_annealing=annealing), pol)
    b = _ro(_env(300, integrator, reward_annealing=annealing), pol, stats=True)
    assert a.stats is None and b.stats is not None
    assert a._collect == "rr_rollout_collect_discrete" and b._collect_stats == "rr_rollout_collect_discrete_stats"
    for c in range(3):
        a.collect()
        b.collect()
        torch.cuda.synchronize()
        G._same(G._snapshot(a), G._snapshot(b), "collect %d" % c)
        blk = b.stats.last_block().view(np.int64)
        assert blk[_lib.RR_RSTAT_SAMPLES] == T * 300
        assert blk[_lib.RR_RSTAT_EPISODES] == int(a.starts[1:].sum().item() + a.last_done.sum().item())
        assert blk[_lib.RR_RSTAT_EPISODES] >= 3 * 300
    idx = a.actions.long().flatten()
    assert int(idx.min()) == 0 and int(idx.max()) == k - 1  # a Categorical collect: indices 0 .. K - 1
    a.env.close()
    b.env.close()


# ---- 2. the statistics against the per-step loop's list of finished episodes ----

@functools.lru_cache(maxsize=None)
def _episode_reference(n, collects=3):
    """Per collect, the finished episodes of a handle stepped by rr_rollout_step_discrete and read after every
    step: float32 returns and int lengths / flags, in the order they were seen. Never modified."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr

    env = _env(n)
    ro = _ro(env, _policy(), per_step=True)
    G._landing_and_nan(env, 3)
    lib, nt = _lib.load(), env.n_terms
    params = _ptr(ro._pack.pack())
    out = []
    for _c in range(collects):
        eps = dict(ret=[], len=[], landed=[], event=[], bounds=[], trunc=[], nonfinite=[], env=[])
        for t in range(T):
            stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
            _lib.check(lib.rr_rollout_step_discrete(env._h, params, *ro._head, ro._pack.prec, ro.seed, _ptr(ro.iter), t,
                                                    ro.gamma, _ptr(ro.obs[t]), _ptr(ro.actions[t]),
                                                    _ptr(ro.values[t]), _ptr(ro.log_probs[t]), _ptr(ro.starts[t]),
                                                    _ptr(ro.rewards[t]), _ptr(env.obs), _ptr(env.reward),
                                                    _ptr(env.done), _ptr(env.truncated), _ptr(env.terms), stream),
                       "rr_rollout_step_discrete")
            tobs, tret, tlen = env.copy_terminal()
            d = env.done.bool().cpu().numpy()
            status = env.terms[nt + 1].cpu().numpy()[d]
            bad_obs = ~np.isfinite(tobs.cpu().numpy()[d]).all(1)
            eps["env"].append(np.nonzero(d)[0])
            eps["ret"].append(tret.cpu().numpy()[d])
            eps["len"].append(tlen.cpu().numpy()[d])
            eps["landed"].append(env.terms[nt - 1].cpu().numpy()[d] != 0)
            eps["event"].append(status > 0)
            eps["bounds"].append(env.terms[nt].cpu().numpy()[d] > 0)
            eps["trunc"].append(env.truncated.bool().cpu().numpy()[d])
            eps["nonfinite"].append((status < 0) | bad_obs)  # the status plane shows the event where both hold
        ro.iter.add_(1)
        out.append({k: np.concatenate(v) for k, v in eps.items()})
    env.close()
    return out


def _stats_run(n, collects=3):
    """The same handle and states collected by rr_rollout_collect_discrete_stats: the `out` block after every
    collect, `accum` after the last, and the rollout object (its env still open)."""
    import torch

    env = _env(n)
    ro = _ro(env, _policy(), stats=True)
    G._landing_and_nan(env, 3)
    blocks = []
    for _c in range(collects):
        ro.collect()
        blocks.append(ro.stats.last_block().copy())
    torch.cuda.synchronize()
    return blocks, ro.stats.accum.cpu().numpy().copy(), ro


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_statistics_equal_the_per_step_loop(n):
    from rl_rocket_amd import _lib as L

    ref = _episode_reference(n)
    # the reference first: the test cannot pass on an empty set
    allr = {k: np.concatenate([r[k] for r in ref]) for k in ref[0]}
    assert allr["nonfinite"].sum() >= 1 and allr["trunc"].sum() >= 1
    if n >= 64:  # whatever the policy chooses (tests/test_collect_stats_discrete_host.py)
        assert allr["landed"].sum() >= 1
        assert (allr["event"] & ~allr["landed"]).sum() >= 1
    if n == 300:
        assert max(np.bincount(r["env"], minlength=n).max() for r in ref) >= 2
    blocks, _accum, ro = _stats_run(n)
    ro.env.close()
    finite_sums = 0
    for c, (blk, r) in enumerate(zip(blocks, ref)):
        i, f = blk.view(np.int64), blk.view(np.float64)
        want = [r["ret"].size, int(r["len"].sum()), int(r["landed"].sum()), int(r["event"].sum()),
                int(r["bounds"].sum()), int(r["trunc"].sum()), int(r["nonfinite"].sum()), T * n]
        print("collect %d ints: got %s want %s" % (c, G._ints(blk), want))
        assert G._ints(blk) == want, c  # n = 1: a clamped lane counted would show here
        ret = r["ret"].astype(np.float32)
        lo = np.fmin.reduce(ret, initial=np.float32(np.inf)) if ret.size else np.float32(np.inf)
        hi = np.fmax.reduce(ret, initial=np.float32(-np.inf)) if ret.size else np.float32(-np.inf)
        assert np.float32(f[L.RR_RSTAT_RET_MIN]) == lo and np.float32(f[L.RR_RSTAT_RET_MAX]) == hi, c
        assert f[L.RR_RSTAT_RET_MIN] == np.float64(lo) and f[L.RR_RSTAT_RET_MAX] == np.float64(hi), c
        r64 = ret.astype(np.float64)
        ok = G._sum_ok(float(f[L.RR_RSTAT_RET_SUM]), r64, "n %d collect %d sum ret" % (n, c))
        ok &= G._sum_ok(float(f[L.RR_RSTAT_RET_SQ]), r64 * r64, "n %d collect %d sum ret^2" % (n, c))
        finite_sums += bool(ok and ret.size)
    assert finite_sums >= 1  # at least one collect's sums were held to the bound, not to NaN == NaN


# ---- 3. the explained-variance sums against the returned buffers ----

def test_sample_sums_equal_the_buffers():
    import torch
    from rl_rocket_amd import _lib as L
    from rl_rocket_amd.rollout_stats import stats_dict

    n = 65
    ro = _ro(_env(n), _policy(), stats=True)
    for c in range(2):
        ro.collect()
        torch.cuda.synchronize()
        f = ro.stats.last_block().view(np.float64)
        y = ro.returns.cpu().numpy().astype(np.float64)
        d = y - ro.values.cpu().numpy().astype(np.float64)
        assert np.isfinite(y).all() and np.isfinite(d).all()
        for slot, terms, name in ((L.RR_RSTAT_Y_SUM, y, "y"), (L.RR_RSTAT_Y_SQ, y * y, "y^2"),
                                  (L.RR_RSTAT_D_SUM, d, "d"), (L.RR_RSTAT_D_SQ, d * d, "d^2")):
            assert G._sum_ok(float(f[slot]), terms, "collect %d sum %s" % (c, name))
        assert ro.stats.last_block().view(np.int64)[L.RR_RSTAT_SAMPLES] == T * n
        ev = stats_dict(ro.stats.last_block())["train/explained_variance"]
        assert abs(ev - (1.0 - d.var() / y.var())) < 1e-9 * max(1.0, d.var() / y.var())
    ro.env.close()


# ---- 4. 66 rows of partials, the last wave holding one env ----

def test_rows_of_partials_with_a_last_wave_of_one_env():
    import torch
    from rl_rocket_amd import _lib as L

    n = 4161  # 65 full waves and one env: 17 workgroups, the last with one live lane and three dead waves
    ro = _ro(_env(n), _policy(), stats=True)
    assert ro.stats.partials.shape[0] == 66 == L.load().rr_rollout_stats_rows(n)
    for _c in range(2):
        ro.collect()
        torch.cuda.synchronize()
        blk = ro.stats.last_block().view(np.int64)
        assert blk[L.RR_RSTAT_EPISODES] == int(ro.starts[1:].sum().item() + ro.last_done.sum().item()) >= 3 * n
        assert blk[L.RR_RSTAT_SAMPLES] == T * n
        rows = ro.stats.partials.cpu().numpy().view(np.int64)
        assert rows[:65, L.RR_RSTAT_SAMPLES].tolist() == [T * 64] * 65 and rows[65, L.RR_RSTAT_SAMPLES] == T
        assert rows[:, L.RR_RSTAT_EPISODES].sum() == blk[L.RR_RSTAT_EPISODES]
        last = int(ro.starts[1:, n - 1].sum().item() + ro.last_done[n - 1].item())
        assert rows[65, L.RR_RSTAT_EPISODES] == last >= 3  # the lone env's episodes, no clamped lane's
    ro.env.close()


# ---- 5. accum, window() ----

def test_accum_folds_the_collects():
    import torch
    from rl_rocket_amd.rollout_stats import empty_block, fold_blocks, stats_dict

    blocks, accum, ro = _stats_run(300)
    assert np.array_equal(accum, fold_blocks(blocks))  # bit for bit: the same fold in the same order
    assert int(accum[0]) == sum(int(b[0]) for b in blocks) > 0
    win = ro.stats.window()
    assert G._nan_to_none(win) == G._nan_to_none(stats_dict(accum))
    torch.cuda.synchronize()
    assert np.array_equal(ro.stats.accum.cpu().numpy(), empty_block())
    ro.collect()  # the next window holds this collect alone
    assert np.array_equal(ro.stats.accum.cpu().numpy(), fold_blocks([ro.stats.last_block()]))
    ro.env.close()


# ---- 6. captured in a graph ----

def test_graph_replay_equals_eager():
    import torch

    pol = _policy()
    a = _ro(_env(300), pol, stats=True)
    b = _ro(_env(300), pol, stats=True)
    a.collect()
    b.collect()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            b.collect()
    torch.cuda.current_stream().wait_stream(st)
    for c in range(2):
        a.collect()
        g.replay()
        torch.cuda.synchronize()
        G._same(G._snapshot(a), G._snapshot(b), "replay %d" % c)
        assert np.array_equal(a.stats.last_block(), b.stats.last_block())
        assert np.array_equal(a.stats.accum.cpu().numpy(), b.stats.accum.cpu().numpy())
    assert a.stats.last()["rollout/episodes"] >= 3 * 300
    a.env.close()
    b.env.close()


# ---- 7. refusals on real handles ----

def test_refusals_on_real_handles():
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import DeviceRollout
    from rl_rocket_amd.rollout_stats import empty_block

    lib, name = _lib.load(), "rr_rollout_collect_discrete_stats"
    pol = _policy()
    env = _env(70)
    ro = _ro(env, pol, stats=True)
    stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
    st = ro.stats.struct()

    def call(e):
        return lib.rr_rollout_collect_discrete_stats(
            e._h, _ptr(ro._pack.pack()), *ro._head, ro._pack.prec, ro.seed, _ptr(ro.iter), T, 0.99, 0.95, _ptr(ro.obs),
            _ptr(ro.actions), _ptr(ro.values), _ptr(ro.log_probs), _ptr(ro.starts), _ptr(ro.rewards),
            _ptr(ro.advantages), _ptr(ro.returns), _ptr(ro.last_value), _ptr(ro.last_done), _ptr(ro.last_start),
            _ptr(e.obs), _ptr(e.reward), _ptr(e.done), _ptr(e.truncated), None, ctypes.byref(st), stream)

    def refused(rc, word):
        msg = lib.rr_last_error().decode()
        assert rc == _lib.RR_EINVAL and msg.startswith(name + ": ") and word in msg, (rc, msg)

    for kw, word in ((dict(model=6, **ENV_CONFIG_6DOF), "6DOF"), (dict(integrator="dopri5"), "RR_INT_DOPRI5"),
                     (dict(episode_stats=False), "RR_FLAG_EPISODE_STATS"), (dict(auto_reset=False), "RR_FLAG_AUTO_RESET")):
        from rl_rocket_amd.batch import RocketBatch

        other = RocketBatch(70, **dict(dict(model=3, device=DEV, max_episode_steps=TL), **kw))
        refused(call(other), word)
        other.close()
    torch.cuda.synchronize()
    assert np.array_equal(ro.stats.accum.cpu().numpy(), empty_block())  # the refused calls launched nothing
    # the Python surface
    for kw in (dict(integrator="dopri5"), dict(episode_stats=False), dict(auto_reset=False)):
        other = _env(70, **kw)
        with pytest.raises(ValueError):
            DeviceRollout(other, pol, n_steps=T, one_launch=True, stats=True)
        other.close()
    for kw in (dict(), dict(per_step=True), dict(one_launch=True, per_step=True)):
        with pytest.raises(ValueError, match="stats=True"):
            DeviceRollout(env, pol, n_steps=T, stats=True, **kw)
    env.close()
