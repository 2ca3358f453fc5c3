"""rr_rollout_collect_stats / DeviceRollout(stats=True): the one-launch collect that also accounts
for the episodes it finishes.

Two things are held: the collect itself is bitwise rr_rollout_collect (buffers, env outputs, the
handle's state), and the statistics block equals what a per-step loop sees. That loop is the one of
tests/test_gpu_eval.py::_reference: a second handle with the same seed is stepped by rr_rollout_step
(same noise key: seed, *iter, t) and read after every step (done, truncated, terms, copy_terminal);
the finished episodes are listed from that.

Bounds. The int64 slots and the fp32 extremes are exact. An fp64 sum of K terms computed in any order
is within (K - 1) * 2^-53 * sum|term| of the exact sum, so two such sums differ by at most
K * 2^-52 * sum|term|: derived, not tuned. A NaN term (the return of an episode that ended on a
non-finite state) makes both sums NaN; min / max skip it (fmin / fmax)."""
import ctypes
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, TL, SEED = 16, 5, 11
BUFS = ("obs", "actions", "values", "log_probs", "starts", "rewards", "advantages", "returns", "last_value",
        "last_done", "last_start")
ENV_OUT = ("obs", "reward", "done", "truncated", "terms")


def _dims(model):
    return (14, 3) if model == 6 else (7, 2)


def _policy(model):
    from rollout_ref import scaled_policy

    ns, na = _dims(model)
    return scaled_policy(ns, na, seed=5, head_scale=1.0 if model == 6 else 0.05).to(DEV)


def _env(model, n, integrator="rk4", tl=TL, **over):
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF

    args = dict(ENV_CONFIG_6DOF if model == 6 else {})
    args.update(model=model, device=DEV, max_episode_steps=tl, compute_terms=True, seed=1234, integrator=integrator)
    args.update(over)
    return RocketBatch(n, **args)


def _ro(env, pol, prec="fp32", stats=False, per_step=False):
    from rl_rocket_amd.rollout import DeviceRollout

    return DeviceRollout(env, pol, n_steps=T, policy_dtype=prec, seed=SEED, per_step=per_step, stats=stats)


def _landing_and_nan(b, model):
    """The `landing=True` states of tests/test_gpu_eval.py::_batch (the first 32 envs 2 cm above the
    pad descending at 0.5 m/s, the next 32 at 5 m/s: soft and hard touchdowns, see test_landing_bit
    there), the last 16 of those at 30 m/s instead (above the 10 m/s landing limit: a ground event
    that is no landing), and the last env with a NaN velocity: its episode ends on a non-finite
    state at the first step."""
    import torch

    n = b.num_envs
    st, v0, _ = b.get_state()
    m = 0.5 * (float(b.cfg.ic_low[-1]) + float(b.cfg.ic_high[-1]))
    row = [0.02, 0, 0, -0.5, 0, 0, 1, 0, 0, 0, 0, 0, 0, m] if model == 6 else [0, 0.02, math.pi / 2, 0, -0.5, 0, m]
    st[:, :64] = torch.tensor(row, dtype=torch.float32, device=DEV)[:, None]
    st[3 if model == 6 else 4, 32:64] = -5.0
    v0[:32] = 0.5
    v0[32:64] = 5.0
    st[3 if model == 6 else 4, 48:64] = -30.0
    v0[48:64] = 30.0
    st[4 if model == 6 else 3, n - 1] = float("nan")
    b.set_state(st, v0=v0)


def _snapshot(ro):
    import torch

    env = ro.env
    out = {"ro." + k: getattr(ro, k).clone() for k in BUFS}
    out.update({"env." + k: getattr(env, k).clone() for k in ENV_OUT})
    out.update({"ck." + k: v.clone() for k, v in env.checkpoint().items() if torch.is_tensor(v)})
    out.update({"term.%d" % k: v.clone() for k, v in enumerate(env.copy_terminal())})
    out["iter"] = ro.iter.clone()
    return out


def _same(a, b, what=""):
    import torch

    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if x.is_floating_point():  # bit for bit, NaNs included
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (what, k)


def _sum_ok(got, terms, what):
    """got against the fp64 sum of `terms` within K * 2^-52 * sum|term| (module docstring)."""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    if np.isnan(terms).any():  # a NaN term: the sum is NaN on both sides, nothing to bound
        assert math.isnan(got), (what, got)
        return False
    want, mag = math.fsum(terms), math.fsum(np.abs(terms))
    bound = terms.size * 2.0 ** -52 * mag
    print("%s: got %.17g want %.17g |diff| %.3g bound %.3g (K = %d)" % (what, got, want, abs(got - want), bound, terms.size))
    assert abs(got - want) <= bound, (what, got, want, bound)
    return True


def _ints(block):
    from rl_rocket_amd import _lib

    return [int(np.asarray(block).view(np.int64)[s]) for s in _lib.RR_RSTAT_INT_SLOTS]


# ---- 1. the collect is rr_rollout_collect's, bit for bit ----

@pytest.mark.parametrize("prec", ["fp32", "fp16x3", "bf16"])
@pytest.mark.parametrize("integrator", ["rk4", "euler"])
@pytest.mark.parametrize("model", [6, 3])
def test_collect_is_bitwise_the_plain_collect(model, integrator, prec):
    """Every arm of dispatch_env_prec at n = 300 (four full waves, one wave of 44 envs, three dead
    waves in the last workgroup), T = 16, TimeLimit 5, three collects in a row: every env finishes
    three episodes per collect (the terminal rows are overwritten) and episodes straddle the collect
    boundary (16 = 3 * 5 + 1)."""
    import torch
    from rl_rocket_amd import _lib

    pol = _policy(model)
    a = _ro(_env(model, 300, integrator), pol, prec)
    b = _ro(_env(model, 300, integrator), pol, prec, stats=True)
    assert a.stats is None and b.stats is not None and not a.per_step and not b.per_step
    for c in range(3):
        a.collect()
        b.collect()
        torch.cuda.synchronize()
        _same(_snapshot(a), _snapshot(b), "collect %d" % c)
        blk = b.stats.last_block().view(np.int64)
        assert blk[_lib.RR_RSTAT_SAMPLES] == T * 300
        assert blk[_lib.RR_RSTAT_EPISODES] == int(a.starts[1:].sum().item() + a.last_done.sum().item())
        assert blk[_lib.RR_RSTAT_EPISODES] >= 3 * 300
    a.env.close()
    b.env.close()


# ---- 2. the statistics against the per-step loop's list of finished episodes ----

@functools.lru_cache(maxsize=None)
def _episode_reference(model, n, collects=3):
    """Per collect, the finished episodes of a handle stepped by rr_rollout_step and read after every
    step: float32 returns and int lengths / flags, in the order they were seen. Never modified."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr

    env = _env(model, n)
    ro = _ro(env, _policy(model), per_step=True)
    _landing_and_nan(env, model)
    lib, nt = _lib.load(), env.n_terms
    params = _ptr(ro._pack.pack())
    out = []
    for _c in range(collects):
        eps = dict(ret=[], len=[], landed=[], event=[], bounds=[], trunc=[], nonfinite=[], env=[])
        for t in range(T):
            stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
            _lib.check(lib.rr_rollout_step(env._h, params, ro._pack.prec, ro.seed, _ptr(ro.iter), t, ro.gamma,
                                           _ptr(ro.obs[t]), _ptr(ro.actions[t]), _ptr(ro.values[t]),
                                           _ptr(ro.log_probs[t]), _ptr(ro.starts[t]), _ptr(ro.rewards[t]),
                                           _ptr(env.obs), _ptr(env.reward), _ptr(env.done), _ptr(env.truncated),
                                           _ptr(env.terms), stream), "rr_rollout_step")
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


def _stats_run(model, n, collects=3):
    """The same handle and states collected by rr_rollout_collect_stats: the `out` block after every
    collect, `accum` after the last, and the rollout object (its env still open)."""
    import torch

    env = _env(model, n)
    ro = _ro(env, _policy(model), stats=True)
    _landing_and_nan(env, model)
    blocks = []
    for _c in range(collects):
        ro.collect()
        blocks.append(ro.stats.last_block().copy())
    torch.cuda.synchronize()
    return blocks, ro.stats.accum.cpu().numpy().copy(), ro


@pytest.mark.parametrize("n", [1, 64, 65, 300])
@pytest.mark.parametrize("model", [6, 3])
def test_statistics_equal_the_per_step_loop(model, n):
    from rl_rocket_amd import _lib as L

    ref = _episode_reference(model, n)
    # the reference first: the test cannot pass on an empty set
    allr = {k: np.concatenate([r[k] for r in ref]) for k in ref[0]}
    assert allr["nonfinite"].sum() >= 1 and allr["trunc"].sum() >= 1
    if n >= 64:
        assert allr["landed"].sum() >= 1
        assert (allr["event"] & ~allr["landed"]).sum() >= 1
    if n == 300:
        assert max(np.bincount(r["env"], minlength=n).max() for r in ref) >= 2
    blocks, _accum, ro = _stats_run(model, n)
    ro.env.close()
    finite_sums = 0
    for c, (blk, r) in enumerate(zip(blocks, ref)):
        i, f = blk.view(np.int64), blk.view(np.float64)
        want = [r["ret"].size, int(r["len"].sum()), int(r["landed"].sum()), int(r["event"].sum()),
                int(r["bounds"].sum()), int(r["trunc"].sum()), int(r["nonfinite"].sum()), T * n]
        print("collect %d ints: got %s want %s" % (c, _ints(blk), want))
        assert _ints(blk) == want, c  # n = 1: a clamped lane counted would show here
        ret = r["ret"].astype(np.float32)
        lo = np.fmin.reduce(ret, initial=np.float32(np.inf)) if ret.size else np.float32(np.inf)
        hi = np.fmax.reduce(ret, initial=np.float32(-np.inf)) if ret.size else np.float32(-np.inf)
        assert np.float32(f[L.RR_RSTAT_RET_MIN]) == lo and np.float32(f[L.RR_RSTAT_RET_MAX]) == hi, c
        assert f[L.RR_RSTAT_RET_MIN] == np.float64(lo) and f[L.RR_RSTAT_RET_MAX] == np.float64(hi), c
        r64 = ret.astype(np.float64)
        ok = _sum_ok(float(f[L.RR_RSTAT_RET_SUM]), r64, "model %d n %d collect %d sum ret" % (model, n, c))
        ok &= _sum_ok(float(f[L.RR_RSTAT_RET_SQ]), r64 * r64, "model %d n %d collect %d sum ret^2" % (model, n, c))
        finite_sums += bool(ok and ret.size)
    assert finite_sums >= 1  # at least one collect's sums were held to the bound, not to NaN == NaN


# ---- 3. the explained-variance sums against the returned buffers ----

@pytest.mark.parametrize("model,n", [(6, 300), (3, 65)])
def test_sample_sums_equal_the_buffers(model, n):
    import torch
    from rl_rocket_amd import _lib as L
    from rl_rocket_amd.rollout_stats import stats_dict

    ro = _ro(_env(model, n), _policy(model), stats=True)
    for c in range(2):
        ro.collect()
        torch.cuda.synchronize()
        f = ro.stats.last_block().view(np.float64)
        y = ro.returns.cpu().numpy().astype(np.float64)
        d = y - ro.values.cpu().numpy().astype(np.float64)
        assert np.isfinite(y).all() and np.isfinite(d).all()
        for slot, terms, name in ((L.RR_RSTAT_Y_SUM, y, "y"), (L.RR_RSTAT_Y_SQ, y * y, "y^2"),
                                  (L.RR_RSTAT_D_SUM, d, "d"), (L.RR_RSTAT_D_SQ, d * d, "d^2")):
            assert _sum_ok(float(f[slot]), terms, "model %d collect %d sum %s" % (model, c, name))
        assert ro.stats.last_block().view(np.int64)[L.RR_RSTAT_SAMPLES] == T * n
        ev = stats_dict(ro.stats.last_block())["train/explained_variance"]
        assert abs(ev - (1.0 - d.var() / y.var())) < 1e-9 * max(1.0, d.var() / y.var())
    ro.env.close()


# ---- 4. accum, window(), determinism ----

def test_accum_folds_the_collects_and_the_run_is_deterministic():
    import torch
    from rl_rocket_amd.rollout_stats import empty_block, fold_blocks, stats_dict

    blocks, accum, ro = _stats_run(6, 300)
    assert np.array_equal(accum, fold_blocks(blocks))  # bit for bit: the same fold in the same order
    assert int(accum[0]) == sum(int(b[0]) for b in blocks) > 0
    win = ro.stats.window()
    assert _nan_to_none(win) == _nan_to_none(stats_dict(accum))  # the NaN-state env makes the return sums NaN
    torch.cuda.synchronize()
    assert np.array_equal(ro.stats.accum.cpu().numpy(), empty_block())
    assert ro.stats.window()["rollout/episodes"] == 0
    ro.collect()  # the next window holds this collect alone
    assert np.array_equal(ro.stats.accum.cpu().numpy(), fold_blocks([ro.stats.last_block()]))
    ro.env.close()
    blocks2, accum2, ro2 = _stats_run(6, 300)
    ro2.env.close()
    for x, y in zip(blocks, blocks2):
        assert np.array_equal(x, y)  # int64 patterns: the same bits on every run
    assert np.array_equal(accum, accum2)


def _nan_to_none(d):
    return {k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in d.items()}


# ---- 5. captured in a graph ----

def test_graph_replay_equals_eager():
    import torch

    pol = _policy(6)
    a = _ro(_env(6, 300), pol, stats=True)
    b = _ro(_env(6, 300), pol, stats=True)
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
        _same(_snapshot(a), _snapshot(b), "replay %d" % c)
        assert np.array_equal(a.stats.last_block(), b.stats.last_block())
        assert np.array_equal(a.stats.accum.cpu().numpy(), b.stats.accum.cpu().numpy())
    assert a.stats.last()["rollout/episodes"] >= 3 * 300
    a.env.close()
    b.env.close()


# ---- 6. argument errors ----

def test_argument_errors():
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout_stats import empty_block

    lib = _lib.load()
    pol = _policy(6)
    env = _env(6, 70)
    ro = _ro(env, pol, stats=True)
    V = ctypes.c_void_p
    stream = V(torch.cuda.current_stream(env.device).cuda_stream)
    good = dict(e=env._h, params=_ptr(ro._pack.pack()), prec=ro._pack.prec, T=T, adv=_ptr(ro.advantages),
                ret=_ptr(ro.returns), st=ro.stats.struct())

    def call(**over):
        a = dict(good)
        a.update(over)
        st = a["st"]
        return lib.rr_rollout_collect_stats(a["e"], a["params"], a["prec"], ro.seed, _ptr(ro.iter), a["T"], 0.99, 0.95,
                                            _ptr(ro.obs), _ptr(ro.actions), _ptr(ro.values), _ptr(ro.log_probs),
                                            _ptr(ro.starts), _ptr(ro.rewards), a["adv"], a["ret"], _ptr(ro.last_value),
                                            _ptr(ro.last_done), _ptr(ro.last_start), _ptr(env.obs), _ptr(env.reward),
                                            _ptr(env.done), _ptr(env.truncated), _ptr(env.terms),
                                            None if st is None else ctypes.byref(st), stream)

    def refused(rc, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(b"rr_rollout_collect_stats: ") and word in msg, msg

    def st(**over):
        s = ro.stats.struct()
        for k, v in over.items():
            setattr(s, k, v)
        return s

    # what rr_rollout_collect refuses
    refused(call(e=None), b"handle")
    refused(call(T=0), b"n_steps")
    refused(call(params=None), b"null")
    refused(call(prec=7), b"precision")
    refused(call(ret=None), b"buf_advantage")
    # the statistics' own arguments
    refused(call(st=None), b"stats")
    refused(call(st=st(partials=None)), b"partials")
    refused(call(st=st(out=None)), b"out")
    refused(call(st=st(partials=ro.stats.partials.data_ptr() + 64)), b"128-B")
    refused(call(st=st(out=ro.stats.out.data_ptr() + 4)), b"8-B")
    refused(call(st=st(accum=ro.stats.accum.data_ptr() + 4)), b"8-B")
    refused(call(adv=None, ret=None), b"buf_advantage")
    assert call(st=st(accum=None)) == _lib.RR_OK  # accum is optional
    torch.cuda.synchronize()
    # nothing was folded: the refused calls launched nothing, the accepted one had no accum
    assert np.array_equal(ro.stats.accum.cpu().numpy(), empty_block())
    # handles the call refuses
    for kw, word in ((dict(episode_stats=False), b"RR_FLAG_EPISODE_STATS"), (dict(auto_reset=False), b"RR_FLAG_AUTO_RESET"),
                     (dict(integrator="dopri5"), b"DOPRI5")):
        other = _env(6, 70, **kw)
        refused(call(e=other._h), word)
        other.close()
    # the Python surface
    from rl_rocket_amd.rollout import DeviceRollout

    for kw in (dict(integrator="dopri5"), dict(episode_stats=False), dict(auto_reset=False)):
        other = _env(6, 70, **kw)
        with pytest.raises(ValueError):
            DeviceRollout(other, pol, n_steps=T, stats=True)
        other.close()
    with pytest.raises(ValueError):
        DeviceRollout(env, pol, n_steps=T, stats=True, per_step=True)
    env.close()


# ---- 7. full size ----

def test_full_size():
    import torch
    from rl_rocket_amd import _lib as L

    n = 65536
    ro = _ro(_env(6, n, tl=6), _policy(6), stats=True)
    ro.collect()
    torch.cuda.synchronize()
    blk = ro.stats.last_block().view(np.int64)
    assert blk[L.RR_RSTAT_EPISODES] == int(ro.starts[1:].sum().item() + ro.last_done.sum().item()) > n
    assert blk[L.RR_RSTAT_SAMPLES] == T * n
    d = ro.stats.last()
    assert 1.0 <= d["rollout/ep_len_mean"] <= 6.0
    assert d["rollout/ep_rew_min"] <= d["rollout/ep_rew_mean"] <= d["rollout/ep_rew_max"]
    ro.env.close()


# ---- 8. the learner's five figures beside the rollout's ----

@pytest.mark.parametrize("fused", [True, False])
def test_last_stats_of_the_graphed_update(fused):
    """GraphedPPOUpdate.last_stats(): update()'s three figures under train/* keys plus clip_fraction
    and approx_kl of the same (last) minibatch step; update()'s return value keeps its three keys.
    One epoch of one minibatch from the collecting policy: the ratio is exp(log-prob difference between
    the learner and the collect), within 5e-4 of 1 (the agreement tests/test_gpu_rollout.py holds the
    collect's log-probs to), so no sample is clipped at 0.2 and 0 <= approx_kl <= (5e-4)^2 up to the
    fp32 rounding of a mean of values near 1e-7."""
    import torch
    from rl_rocket_amd.rollout import GraphedPPOUpdate

    n = 1024
    pol = _policy(6)
    ro = _ro(_env(6, n, tl=6), pol, stats=True)
    ro.collect()
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4, eps=1e-5, capturable=True)
    upd = GraphedPPOUpdate(pol, opt, ro, batch_size=T * n, fused=fused)
    assert upd.fused == fused
    three = upd.update(n_epochs=1, generator=torch.Generator(DEV).manual_seed(5))
    assert sorted(three) == ["entropy", "policy_loss", "value_loss"]
    five = upd.last_stats()
    assert sorted(five) == ["train/approx_kl", "train/clip_fraction", "train/entropy", "train/policy_loss",
                            "train/value_loss"]
    for k, v in three.items():
        assert five["train/" + k] == v
    if fused:
        raw = upd._update.stats.cpu().numpy()
        assert five["train/clip_fraction"] == float(raw[3]) and five["train/approx_kl"] == float(raw[4])
    print("fused %s: %s" % (fused, five))
    assert five["train/clip_fraction"] == 0.0
    assert -1e-6 <= five["train/approx_kl"] <= 2.5e-7 + 1e-6
    log = ro.stats.last() | five  # one iteration's log dict
    assert log["rollout/episodes"] > n and "train/explained_variance" in log and len(log) == 17
    ro.env.close()
