"""rr_bc_update (behaviour cloning on the device: rl_rocket_amd/csrc/bc/rocket_bc.hip, the PPO
learner's pi tower with another head derivative) and the Python layer over it (rl_rocket_amd/bc.py),
against tests/bc_ref.py: the loss in PyTorch autograd, float64, on the same fp32 inputs, and
ppo_ref.clip_adam_ref without a clip for the optimizer. The fused path is never its own reference.

1. Gradients and the seven statistics at the batch sizes where the kernel changes path, minibatches
   drawn from 70 001 rows. Bars, the learner's own (tests/test_gpu_ppo_edges.py): per tensor
   max |fused - fp64| <= 1e-4 max |fp64| + 1e-7; statistics 1e-5 relative + 1e-6. The value half is
   bitwise zero at l2_weight 0 and l2_weight w within one fp32 rounding otherwise.
2. The loss terms off their defaults: ent_weight 0 / 0.1, l2_weight 0.01, log_std -2 / +1, actions
   at +-1 (what a clipped recording holds).
3. Rows outside the minibatch are NaN: bitwise the result of clean rows.
4. The optimizer half of 6 calls against float64 Adam on the gradients each call left.
5. The same call twice, a chained epoch against one that packs per call, a captured epoch against
   the eager one: bitwise.
6. bc_train fused against fused=False over a few epochs.
7. Demonstrations from a recording evaluation and from a collect.
8. The compat kick-starter on tuples built from a recording."""
import copy
import os
import sys

import numpy as np
import pytest

import bc_ref as R
import ppo_ref as P
from bc_gpu_common import BcHelpers

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ROWS = R.N_ROWS

_H = BcHelpers(R, P.NAMES, P.VF_NAMES, "rr_bc_update", lambda: R.sweep_inputs(14, 3))
_minibatch, _adam, _one_call, _check_against_fp64, _state, _epoch = (
    _H.minibatch, _H.adam, _H.one_call, _H.check_against_fp64, _H.state, _H.epoch)


# 16 385: one past kMaxWG workgroups x 4 waves x 32 samples, a wave's second tile
SWEEP = [(bs, 14, 3) for bs in (2, 31, 32, 33, 129, 4097, 16385, 40001)] + [(bs, 7, 2) for bs in (3, 33, 4097)]


@pytest.mark.parametrize("bs,ns,na", SWEEP)
def test_bc_gradients_and_statistics_batch_size_sweep(bs, ns, na):
    pol0, obs, acts = R.sweep_inputs(ns, na)
    idx = _minibatch(bs)
    label = "bs=%d (%d,%d)" % (bs, ns, na)
    _, grads, stats = _one_call(pol0, obs, acts, idx)
    _check_against_fp64(label, pol0, obs, acts, idx, grads, stats)
    _, grads, stats = _one_call(pol0, obs, acts, idx, l2_weight=0.01)
    _check_against_fp64(label + " l2", pol0, obs, acts, idx, grads, stats, l2_weight=0.01)


TERMS = {"ent0": dict(ent_weight=0.0), "ent0.1": dict(ent_weight=0.1), "l2_0.01": dict(l2_weight=0.01),
         "ent0.1_l2_0.01": dict(ent_weight=0.1, l2_weight=0.01), "logstd-2": {}, "logstd+1": {}, "clipped_actions": {}}


@pytest.mark.parametrize("bs", [1000, 33])
@pytest.mark.parametrize("name", list(TERMS))
def test_bc_loss_terms_off_their_defaults(name, bs):
    """log_std -2 / +1: every component, the actions drawn from that policy as a recording would hold
    them (ppo_ref.edge_case's reason: unit-normal actions sit 7 sigma off the mean at log_std -2,
    log-probs of -160 whose fp32 ulp alone is the statistics' bar). clipped_actions: every action
    component at -1 or +1."""
    import torch

    n, ns, na = 1500, 14, 3
    kw = {}
    if name.startswith("logstd"):
        kw["log_std"] = float(name[len("logstd"):])
    pol, ro, g = P.setup_cpu(ns, na, n, seed=500 + sorted(TERMS).index(name), **kw)
    obs, acts = ro.obs.reshape(n, ns), ro.actions.reshape(n, na)
    if name.startswith("logstd"):
        with torch.no_grad():
            mean, _ = copy.deepcopy(pol).double()(obs.double())
            eps = torch.randn((n, na), generator=g, dtype=torch.float64)
            acts = (mean + pol.log_std.double().exp() * eps).float()
    if name == "clipped_actions":
        acts = torch.where(acts >= 0, 1.0, -1.0)
    idx = torch.randperm(n, generator=g)[:bs].contiguous().cuda()
    pol, obs, acts = pol.cuda(), obs.cuda().contiguous(), acts.cuda().contiguous()
    _, grads, stats = _one_call(pol, obs, acts, idx, **TERMS[name])
    _check_against_fp64("%s bs=%d" % (name, bs), pol, obs, acts, idx, grads, stats, **TERMS[name])
    if name == "ent0":
        assert stats[2].item() == 0.0
    if name == "clipped_actions":
        assert bool((acts[idx].abs() == 1.0).all())


@pytest.mark.parametrize("bs", [33, 16385])
def test_bc_reads_nothing_outside_the_minibatch(bs):
    """idx is the head of a longer tensor of valid rows; every row of obs / acts that idx[:bs] does
    not name is NaN. Gradients, statistics, parameters and Adam state are bitwise those of clean rows."""
    import torch

    pol0, obs, acts = R.sweep_inputs(14, 3)
    long_idx = _minibatch(bs, extra=97)
    idx = long_idx[:bs]
    assert idx.data_ptr() == long_idx.data_ptr() and idx.is_contiguous()
    outside = torch.ones(N_ROWS, dtype=torch.bool, device=DEV)
    outside[idx] = False
    assert bool(outside[long_idx[bs:]].all())
    bad = [obs.clone(), acts.clone()]
    for x in bad:
        x[outside] = float("nan")
    (pa, ga, sa), (pb, gb, sb) = _one_call(pol0, obs, acts, idx, l2_weight=0.01), _one_call(pol0, *bad, idx, l2_weight=0.01)
    assert all(bool(torch.isfinite(g).all()) for g in ga) and bool(torch.isfinite(sa).all())
    for name, a, b in zip(P.NAMES, ga, gb):
        assert torch.equal(a, b), name
    for a, b in zip(pa.parameters(), pb.parameters()):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert torch.equal(sa, sb)


def test_bc_optimizer_half_matches_float64_adam():
    """After each of 6 calls (a learning-rate change after 3, l2 on so that the value half moves):
    parameters, exp_avg and exp_avg_sq are float64 Adam applied, from the fp32 state the call started
    from, to the gradients it left; step counts the calls on all 13 tensors. Bars of
    test_gpu_ppo.test_clip_adam_matches_torch."""
    import torch
    from rl_rocket_amd.bc import BCUpdate, Demonstrations
    from rl_rocket_amd.rollout import _policy_tensors

    pol0, obs, acts = R.sweep_inputs(14, 3)
    pol = copy.deepcopy(pol0)
    opt = _adam(pol)
    step = BCUpdate(pol, opt, Demonstrations(obs, acts), 1000, l2_weight=0.01)
    tensors = _policy_tensors(pol)
    g = torch.Generator().manual_seed(9)
    for call in range(6):
        if call == 3:
            opt.param_groups[0]["lr"] = 2.5e-4
        lr = opt.param_groups[0]["lr"]
        idx = torch.randperm(N_ROWS, generator=g)[:1000 if call != 4 else 333].contiguous().cuda()
        before = [t.detach().clone() for t in tensors]
        m0 = [opt.state[t]["exp_avg"].clone() for t in tensors]
        v0 = [opt.state[t]["exp_avg_sq"].clone() for t in tensors]
        step(idx, chained=call in (1, 2, 5))
        torch.cuda.synchronize()
        p64, m64, v64, n = R.adam_step_ref(before, [t.grad for t in tensors], m0, v0, call, lr)
        assert n == call + 1
        for name, t, p, m, v in zip(P.NAMES, tensors, p64, m64, v64):
            st = opt.state[t]
            assert float(st["step"]) == call + 1, name
            assert (t.detach().double() - p).abs().max().item() <= 1e-6 * max(1.0, p.abs().max().item()), name
            assert torch.allclose(st["exp_avg"].double(), m, rtol=1e-5, atol=1e-9), name
            assert torch.allclose(st["exp_avg_sq"].double(), v, rtol=1e-5, atol=1e-12), name
            assert not torch.equal(t.detach(), before[P.NAMES.index(name)]), name
    assert all(float(opt.state[t]["step"]) == 6.0 for t in tensors) and len(tensors) == 13


def test_bc_same_call_twice_gives_the_same_bits():
    import torch

    pol0, obs, acts = R.sweep_inputs(14, 3)
    idx = _minibatch(40001)
    (pa, ga, sa), (pb, gb, sb) = _one_call(pol0, obs, acts, idx), _one_call(pol0, obs, acts, idx)
    for a, b in zip(ga + list(pa.parameters()) + [sa], gb + list(pb.parameters()) + [sb]):
        assert torch.equal(a, b)


def test_bc_without_a_statistics_block_is_the_same_step():
    """stats = NULL through the C ABI (the finish launches no statistics block): gradients,
    parameters and Adam state are bitwise those of the call that writes statistics."""
    import ctypes

    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.bc import BCUpdate, Demonstrations

    pol0, obs, acts = R.sweep_inputs(7, 2)
    idx = _minibatch(4097)
    out = []
    for with_stats in (True, False):
        pol = copy.deepcopy(pol0)
        opt = _adam(pol)
        s = BCUpdate(pol, opt, Demonstrations(obs, acts), 4097, 0.01, 1e-3)
        s.stats.fill_(-7.0)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(s._lib.rr_bc_update(7, 2, s._params_w, s._dst, s._m, s._v, s._s, obs.data_ptr(), acts.data_ptr(),
                                       idx.data_ptr(), 4097, 0.01, 1e-3, s.lr.data_ptr(), 0.9, 0.999, 1e-8,
                                       s.stats.data_ptr() if with_stats else None, 0, s.ws.data_ptr(), s._nbytes, stream),
                   "rr_bc_update")
        out.append((_state(pol, opt), s.stats.clone()))
    (a, sa), (b, sb) = out
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)
    assert bool((sb == -7.0).all()) and sa[0].item() > 0.0 and sa[7].item() == 0.0


def test_bc_chained_epoch_is_bitwise_the_packed_and_the_replayed_one():
    import torch

    packed, st_p = _epoch("packed")
    chained, st_c = _epoch("chained")
    replayed, st_g = _epoch("graph")
    assert len(packed) == len(chained) == len(replayed) == 13 * 5 and len(st_p) == len(st_c) == len(st_g) == 3
    for k, (a, b, c) in enumerate(zip(packed, chained, replayed)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(a, c), (P.NAMES[k // 5], k % 5)
    for a, b in zip(st_p, st_c):
        assert torch.equal(a, b)
    for a, c in zip(st_p, st_g):
        assert torch.equal(a, c)
    assert float(packed[4]) == 3.0


CARVING = [("gauss", 14, 3), ("gauss", 7, 2), ("cat", 7, 2), ("cat", 7, 4)]


@pytest.mark.parametrize("bs", [33, 129])  # one workgroup, two
@pytest.mark.parametrize("head,ns,na", CARVING, ids=["14-3", "7-2", "K2", "K4"])
def test_bc_workspace_carving_leaves_the_tail_and_reads_no_state(head, ns, na, bs):
    """Both calls through the C ABI on a workspace that is the first `bytes` of a larger buffer: one
    unchained call, then one chained call. The 256 floats after the workspace keep their bit pattern, and
    parameters, gradients, Adam state and both calls' statistics are bitwise those of the same two calls on
    a workspace pre-filled with 0xFF bytes (NaNs): an unchained call reads no state from the workspace, and
    the host's sections (images | finish sums | sink | partial vectors) lie inside the size the
    *_workspace_size call returned."""
    import ctypes

    import bc_discrete_ref
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.bc import BCUpdate, Demonstrations

    cat = head == "cat"
    pol0, obs, acts = bc_discrete_ref.sweep_inputs(na) if cat else R.sweep_inputs(ns, na)
    call = "rr_bc_update_discrete" if cat else "rr_bc_update"
    rows = obs.shape[0]  # the two references' demonstrations differ in length
    idx = [_minibatch(bs, n=rows), _minibatch(bs + 1, n=rows)[1:].contiguous()]
    assert all(int(ix.max()) < rows and ix.numel() == bs for ix in idx)
    tail = (0x5A5A0000 + torch.arange(256, dtype=torch.int32)).to(DEV)
    out = []
    for fill in (0x00, 0xFF):
        pol = copy.deepcopy(pol0)
        opt = _adam(pol)
        s = BCUpdate(pol, opt, Demonstrations(obs, acts), bs, 0.01, 1e-3)
        assert s._call == call and s._nbytes % 16 == 0
        buf = torch.full((s._nbytes + 4 * 256,), fill, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        buf[s._nbytes:].view(torch.int32).copy_(tail)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        stats = []
        for flags, ix in zip((0, _lib.RR_BC_CHAINED), idx):
            _lib.check(getattr(s._lib, call)(ns, na, s._params_w, s._dst, s._m, s._v, s._s, obs.data_ptr(),
                                             acts.data_ptr(), ix.data_ptr(), bs, 0.01, 1e-3, s.lr.data_ptr(), 0.9,
                                             0.999, 1e-8, s.stats.data_ptr(), flags, buf.data_ptr(), s._nbytes,
                                             stream), call)
            stats.append(s.stats.clone())
        out.append((_state(pol, opt) + stats, buf[s._nbytes:].view(torch.int32).clone()))
    (a, ta), (b, tb) = out
    assert torch.equal(ta, tail) and torch.equal(tb, tail)
    assert len(a) == len(b) == 5 * (12 if cat else 13) + 2
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)
    assert float(a[4]) == 2.0 and not torch.equal(a[-1], a[-2])


def test_bc_chained_misuse_is_refused():
    import torch
    from rl_rocket_amd.bc import BCUpdate, Demonstrations

    pol0, obs, acts = R.sweep_inputs(7, 2)
    pol = copy.deepcopy(pol0)
    step = BCUpdate(pol, _adam(pol), Demonstrations(obs, acts), 64)
    idx = _minibatch(64)
    with pytest.raises(ValueError, match="chained"):  # no call before it
        step(idx, chained=True)
    step(idx)
    step(idx, chained=True)
    with torch.no_grad():
        pol.log_std.add_(0.1)  # somebody else wrote a parameter: the packed image is stale
    with pytest.raises(ValueError, match="chained"):
        step(idx, chained=True)
    step(idx)
    with pytest.raises(ValueError, match="idx"):
        step(_minibatch(65))
    with pytest.raises(ValueError, match="idx"):
        step(idx.int())
    pol.log_std.grad = torch.zeros_like(pol.log_std)
    with pytest.raises(RuntimeError, match="replaced"):
        step(idx)
    assert set(step.last_stats()) == set(R.STATS)


def test_bc_train_tracks_autograd():
    """3 epochs of 4 minibatches on 8192 rows, fused against fused=False from equal starts and the
    same shuffling: parameters within 5 % of how far training moved them (the bar and its reason:
    test_gpu_ppo.test_fused_update_with_the_shipped_adam_tracks_autograd), and both fit the
    demonstrations better than the start."""
    import torch
    from rl_rocket_amd.bc import Demonstrations, bc_train

    pol0, obs, acts = R.sweep_inputs(14, 3)
    demos = Demonstrations(obs[:8192].contiguous(), acts[:8192].contiguous())
    pols = [copy.deepcopy(pol0) for _ in range(2)]
    opts = [_adam(p) for p in pols]
    gen = lambda: torch.Generator(DEV).manual_seed(21)  # noqa: E731
    sa = bc_train(pols[0], opts[0], demos, n_epochs=3, batch_size=2048, generator=gen(), fused=False)
    sb = bc_train(pols[1], opts[1], demos, n_epochs=3, batch_size=2048, generator=gen(), fused=True)
    torch.cuda.synchronize()
    assert float(opts[0].state[pols[0].log_std]["step"]) == float(opts[1].state[pols[1].value_net.bias]["step"]) == 12.0
    moved = max((x - y).abs().max().item() for x, y in zip(pol0.parameters(), pols[0].parameters()))
    drift = max((x - y).abs().max().item() for x, y in zip(pols[0].parameters(), pols[1].parameters()))
    every = torch.arange(8192, device=DEV)
    n0, na_, nb_ = (R.reference(p, demos.obs, demos.acts, every)[1][0] for p in (pol0, pols[0], pols[1]))
    print("moved %.3e, parameter drift %.3e, neglogp %.6f -> autograd %.6f, fused %.6f" % (moved, drift, n0, na_, nb_), sa, sb)
    assert moved > 1e-3
    assert drift <= 0.05 * moved, (drift, moved)
    assert na_ < n0 and nb_ < n0
    assert set(sa) == set(sb) == set(R.STATS)
    for k in sa:
        assert abs(sa[k] - sb[k]) <= 0.02 * max(1.0, abs(sa[k])), (k, sa[k], sb[k])


def _recording(model):
    """64 envs under TimeLimit 30, two episodes each within 45 steps (the second is cut short where
    the first ran long), envs 63, 0 and 17 recorded."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import MlpActorCritic, PolicyEvaluator

    kw = dict(ENV_CONFIG_6DOF if model == 6 else {}, seed=77)
    b = RocketBatch(64, model=model, device=DEV, max_episode_steps=30, **kw)
    obs0 = b.reset().clone()
    torch.manual_seed(3)
    pol = MlpActorCritic(b.state_dim, b.action_dim).to(DEV)
    rec = (63, 0, 17)
    res = PolicyEvaluator(b, pol, n_episodes=2, max_steps=45, record=rec).run()
    torch.cuda.synchronize()
    return b, pol, obs0, rec, res.trace


@pytest.mark.parametrize("model", [6, 3])
def test_demonstrations_from_a_recording(model):
    import torch
    from rl_rocket_amd.bc import Demonstrations

    b, pol, obs0, rec, trace = _recording(model)
    demos = Demonstrations.from_trace(trace, b)
    inv = (1.0 / b.cfg.state_normalizer).astype(np.float32)
    want_obs, want_act, first, finished, left_out = [], [], [], 0, 0
    for env in rec:  # slot-major, then episode, then step
        for k in range(2):
            try:
                ep = trace.episode(env, k)
            except ValueError:
                left_out += 1
                continue
            if k == 0:
                first.append((sum(len(a) for a in want_act), env))
            finished += 1
            assert ep.complete and len(ep.states) == ep.length + 1
            want_obs.append(ep.states[:-1] * inv)
            want_act.append(ep.actions)
    assert finished >= 3 and len(first) == 3
    print("model %d: %d finished episodes, %d left out, M = %d" % (model, finished, left_out, len(demos)))
    assert len(demos) == sum(len(a) for a in want_act)
    np.testing.assert_array_equal(demos.obs.cpu().numpy(), np.concatenate(want_obs))
    np.testing.assert_array_equal(demos.acts.cpu().numpy(), np.concatenate(want_act))
    for row, env in first:  # bitwise the observation the policy was given first
        assert torch.equal(demos.obs[row], obs0[env]), env
    b.close()


def test_demonstrations_from_a_rollout_are_the_collects_buffers():
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.bc import Demonstrations
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import DeviceRollout, MlpActorCritic

    env = RocketBatch(64, model=6, device=DEV, max_episode_steps=30, **ENV_CONFIG_6DOF)
    torch.manual_seed(11)
    pol = MlpActorCritic(env.state_dim, env.action_dim).to(DEV)
    ro = DeviceRollout(env, pol, n_steps=4, seed=4)
    ro.collect()
    torch.cuda.synchronize()
    d = Demonstrations.from_rollout(ro)
    assert len(d) == 4 * 64 and d.obs.data_ptr() == ro.obs.data_ptr() and d.acts.data_ptr() == ro.actions.data_ptr()
    assert torch.equal(d.obs, ro.obs.reshape(256, 14)) and torch.equal(d.acts, ro.actions.reshape(256, 3))
    assert torch.equal(d.obs[64 + 5], ro.obs[1, 5]) and bool(d.obs.abs().sum() > 0)
    env.close()


def test_compat_kickstarter_trains_on_recorded_tuples():
    import torch

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat")
    if path not in sys.path:
        sys.path.insert(0, path)
    from my_environment.utils.imitation_kickstarter import imitationKickstarter
    from rl_rocket_amd.rollout import MlpActorCritic, _policy_tensors

    b, teacher, _, rec, trace = _recording(6)
    inv = (1.0 / b.cfg.state_normalizer).astype(np.float32)
    eps = [trace.episode(env, 0) for env in rec]
    tuples = [(ep.states * inv, ep.actions, [{}] * ep.length, True) for ep in eps]
    rows = sum(ep.length for ep in eps)
    torch.manual_seed(8)
    student = MlpActorCritic(14, 3).to(DEV)
    before = [t.detach().clone() for t in _policy_tensors(student)]
    kick = imitationKickstarter(policy=student)
    kick.trajectories = tuples
    assert kick.train(n_epochs=2) is student and kick.policy is student
    torch.cuda.synchronize()
    for name, a, t in zip(P.NAMES, before, _policy_tensors(student)):  # the value half's gradient is zero
        assert bool(torch.isfinite(t).all()) and torch.equal(a, t) == (name in P.VF_NAMES), name
    assert float(kick.optimizer.state[student.log_std]["step"]) == 2 * (rows // min(32, rows))
    assert set(kick.stats) == set(R.STATS) and kick.stats["neglogp"] == kick.stats["neglogp"]
    b.close()
