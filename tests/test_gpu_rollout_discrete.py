"""The Categorical policy's one-launch collect (rr_rollout_collect_discrete) and its per-step form
(rr_rollout_step_discrete) against the two-launch path (rr_policy_act_discrete + the env step, then
rr_policy_bootstrap(7, 4) and rr_gae), bit for bit. The two-launch path is checked against float64 in
tests/test_gpu_discrete.py and never runs the kernels under test here. The pattern is
test_gpu_rollout.three_rollout_paths_agree: three DeviceRollouts on twin batches from one seed, two
collects, every rollout buffer, env output, terminal row, state plane and the noise counter equal.

Sizes: n = 300 is two workgroups, a ragged 44-env wave and three dead waves, n = 37 one partial wave;
T = 8 under TimeLimit 6 puts truncation bootstraps and auto-resets inside the rollout; T = 37 makes the
collect's GAE scan run its 16 + 16 + 5 chunks."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BUFS = ("obs", "actions", "values", "log_probs", "starts", "rewards", "advantages", "returns", "last_value",
        "last_done", "last_start")
ENV_OUT = ("obs", "reward", "done", "truncated", "terms")
PATHS = ((None, False), (True, True), (True, False))  # two-launch, per-step, one-launch
TL = 6  # the TimeLimit: below the rollout lengths


def _env(n, integrator="rk4", annealing=False, offset=0, tl=TL):
    from rl_rocket_amd.batch import RocketBatch

    return RocketBatch(n, model=3, device=DEV, max_episode_steps=tl, compute_terms=True, integrator=integrator,
                       reward_annealing=annealing, env_id_offset=offset, seed=77)


def _ro(env, pol, T, one_launch, per_step):
    from rl_rocket_amd.rollout import DeviceRollout

    ro = DeviceRollout(env, pol, n_steps=T, one_launch=one_launch, per_step=per_step, seed=11)
    assert ro.discrete and ro.fused and ro.one_launch == bool(one_launch) and ro.per_step == (per_step or not one_launch)
    return ro


def _same(a, b, tag):
    import torch

    for name in BUFS:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, y), (tag, name, (x - y).abs().max().item())
    for name in ENV_OUT:
        assert torch.equal(getattr(a.env, name), getattr(b.env, name)), (tag, name)
    for x, y in zip(a.env.get_state(), b.env.get_state()):
        assert torch.equal(x, y), tag
    for x, y in zip(a.env.copy_terminal(), b.env.copy_terminal()):
        assert torch.equal(x, y), tag
    ca, cb = a.env.checkpoint(), b.env.checkpoint()
    for k in ("counter", "ep_return"):
        assert torch.equal(ca[k], cb[k]), (tag, k)
    assert torch.equal(a.iter, b.iter), tag


def _paths_agree(pol, T, n, integrator="rk4", annealing=False, collects=2):
    """Two collects on the three paths; returns the two-launch rollout's actions, log-probs and the counts
    of episode starts and truncations seen (the batches are closed)."""
    import torch

    pol = pol.to(DEV)
    ros = [_ro(_env(n, integrator, annealing), pol, T, one, per) for one, per in PATHS]
    acts, lps, starts, truncs = [], [], 0, 0
    for c in range(collects):
        for ro in ros:
            ro.collect()
        torch.cuda.synchronize()
        for b, tag in zip(ros[1:], ("per-step", "one-launch")):
            _same(ros[0], b, "%s, collect %d" % (tag, c))
        a = ros[0]
        assert a.actions.shape == (T, n, 1)
        acts.append(a.actions.clone())
        lps.append(a.log_probs.clone())
        starts += int(a.starts[1:].sum())
        if c == 0 and T > TL:
            # every episode of the first collect starts at step 0 with an elapsed count of 0, so an env whose
            # first start flag after step 0 stands at step TL ran into the TimeLimit (the 3DOF env's shortest
            # oracle episode takes 73 steps: nothing lands or leaves the bounds within 6)
            truncs += int(((a.starts[TL] == 1) & (a.starts[1:TL].sum(0) == 0)).sum())
    for ro in ros:
        ro.env.close()
    return torch.cat(acts), torch.cat(lps), starts, truncs


@pytest.mark.parametrize("n", [300, 37])
@pytest.mark.parametrize("annealing", [False, True])
@pytest.mark.parametrize("integrator", ["rk4", "euler"])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_three_paths_agree(k, integrator, annealing, n):
    import torch
    from discrete_ref import cat_policy

    acts, lps, starts, truncs = _paths_agree(cat_policy(k, 100 + k), 8, n, integrator, annealing)
    assert starts > 0, "no episode ended inside the rollouts"
    assert truncs > 0, "no env ran into the TimeLimit inside the rollout"
    assert torch.isfinite(lps).all()
    idx = acts.long().flatten()
    assert torch.equal(acts.flatten(), idx.float()) and int(idx.min()) == 0 and int(idx.max()) == k - 1
    assert sorted(idx.unique().tolist()) == list(range(k)), "an index was never drawn"


def test_gae_scan_chunks():
    from discrete_ref import cat_policy

    _, _, starts, _ = _paths_agree(cat_policy(4, 104), 37, 300)
    assert starts > 0


@pytest.mark.parametrize("k", [2, 3])
def test_heads_past_k_stay_out(k):
    """Every real bias at -30 and the head weights at 0.01 of their size: the zero-packed heads k >= K hold
    logits of 0, 30 above the real ones, so a softmax, a draw or a compare that looked at them would put
    all the mass (or the index) there."""
    import torch
    from discrete_ref import cat_policy

    pol = cat_policy(k, 100 + k)
    with torch.no_grad():
        pol.action_net.weight.mul_(0.01)
        pol.action_net.bias.fill_(-30.0)
    acts, lps, _, _ = _paths_agree(pol, 8, 300)
    idx = acts.long().flatten()
    assert int(idx.min()) == 0 and int(idx.max()) == k - 1
    # the real logits are within a few 0.01 of each other: log p is near -log K, not near -30
    assert float(lps.min()) > -2.0 and float(lps.max()) < 0.0


def test_underflowing_probability():
    """K = 4 with the last bias at -120: exp(z_3 - max) underflows to 0 in fp32 (e^-103 is the smallest
    subnormal); every stored log-prob is finite and the paths agree on them. A choice whose fp32 weight is 0 is
    never drawn, at any u: the sampler counts a step past choice q only while some weight beyond q is positive
    (categorical_index, rocket_device.h). These 2 x 2 400 random draws would not see a sampler without that
    rule, which drew such a choice only at u >= 1 - 3 x 2^-24; tests/test_gpu_discrete_sampler.py runs those
    draws on every entry point."""
    import torch
    from discrete_ref import cat_policy

    pol = cat_policy(4, 104)
    with torch.no_grad():
        pol.action_net.bias[-1] = -120.0
    acts, lps, _, _ = _paths_agree(pol, 8, 300)
    assert torch.isfinite(lps).all()
    assert int(acts.max()) <= 2  # a probability of 0 is never drawn


def test_shards_concatenate_to_the_single_batch():
    import torch
    from discrete_ref import cat_policy

    pol = cat_policy(4, 104).to(DEV)
    whole = _ro(_env(300), pol, 8, True, False)
    parts = [_ro(_env(128, offset=0), pol, 8, True, False), _ro(_env(172, offset=128), pol, 8, True, False)]
    for _ in range(2):
        for ro in [whole] + parts:
            ro.collect()
        torch.cuda.synchronize()
        for name in BUFS:
            cat = torch.cat([getattr(p, name) for p in parts], dim=0 if name.startswith("last_") else 1)
            assert torch.equal(getattr(whole, name), cat), name
        for name in ("obs", "reward", "done", "truncated"):
            assert torch.equal(getattr(whole.env, name), torch.cat([getattr(p.env, name) for p in parts])), name
        assert torch.equal(whole.env.terms, torch.cat([p.env.terms for p in parts], dim=1))
        for k, x in enumerate(whole.env.get_state()):
            assert torch.equal(x, torch.cat([p.env.get_state()[k] for p in parts], dim=-1))
    assert whole.starts[1:].sum() > 0
    for ro in [whole] + parts:
        ro.env.close()


def test_graph_replay_equals_eager():
    import torch
    from discrete_ref import cat_policy

    pol = cat_policy(4, 104).to(DEV)
    a, b = _ro(_env(300), pol, 8, True, False), _ro(_env(300), pol, 8, True, False)
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
        _same(a, b, "replay %d" % c)
    assert int(a.iter) == 3
    a.env.close()
    b.env.close()


def test_c_abi_refusals_on_real_handles():
    import torch
    from discrete_ref import TABLES, cat_policy
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import RocketBatch, _ptr
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import PolicyPack

    lib, n, T = _lib.load(), 64, 2
    pol = cat_policy(4, 104).to(DEV)
    params = PolicyPack(pol, 7, 4, torch.device(DEV)).pack()
    f = dict(dtype=torch.float32, device=DEV)
    it = torch.zeros(1, dtype=torch.int64, device=DEV)
    bufs = [torch.zeros((T, n, 7), **f), torch.zeros((T, n), **f)] + [torch.zeros((T, n), **f) for _ in range(6)]
    last = [torch.zeros(n, **f) for _ in range(3)]

    def table(k, bad=None):
        rows = [list(r) for r in TABLES[4]] + [[0.0, 0.0]]
        if bad is not None:
            rows[bad][1] = float("nan")
        return (ctypes.c_float * (2 * k))(*[v for r in rows[:k] for v in r])

    def collect(env, k=4, tab=None, prec=0):
        return lib.rr_rollout_collect_discrete(env._h, _ptr(params), k, tab or table(min(k, 5)), prec, 11, _ptr(it), T,
                                               0.99, 0.95, *[_ptr(b) for b in bufs], *[_ptr(b) for b in last],
                                               _ptr(env.obs), _ptr(env.reward), _ptr(env.done), _ptr(env.truncated),
                                               None, None)

    def step(env, k=4, tab=None, prec=0):
        return lib.rr_rollout_step_discrete(env._h, _ptr(params), k, tab or table(min(k, 5)), prec, 11, _ptr(it), 0,
                                            0.99, *[_ptr(b) for b in bufs[:6]], _ptr(env.obs), _ptr(env.reward),
                                            _ptr(env.done), _ptr(env.truncated), None, None)

    def refused(rc, name, word):
        msg = lib.rr_last_error().decode()
        assert rc == _lib.RR_EINVAL and msg.startswith(name) and word in msg, (name, rc, msg)

    e3 = RocketBatch(n, model=3, device=DEV, max_episode_steps=6)
    e6 = RocketBatch(n, model=6, device=DEV, max_episode_steps=6, **ENV_CONFIG_6DOF)
    ed = RocketBatch(n, model=3, device=DEV, max_episode_steps=6, integrator="dopri5")
    for call, name in ((collect, "rr_rollout_collect_discrete"), (step, "rr_rollout_step_discrete")):
        refused(call(e6), name, "6DOF")
        refused(call(ed), name, "RR_INT_DOPRI5")
        refused(call(e3, k=5), name, "2 .. 4")
        refused(call(e3, k=1), name, "2 .. 4")
        refused(call(e3, tab=table(4, bad=2)), name, "finite")
        refused(call(e3, prec=_lib.RR_POLICY_BF16), name, "RR_POLICY_FP32")
        # a NaN in a row past n_choices is not read
        assert call(e3, k=2, tab=table(4, bad=3)) == _lib.RR_OK, lib.rr_last_error()
    torch.cuda.synchronize()
    for e in (e3, e6, ed):
        e.close()
