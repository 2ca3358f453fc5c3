"""rr_bc_update_discrete (behaviour cloning of the Categorical policy on the device:
rl_rocket_amd/csrc/bc_discrete/rocket_bc_discrete.hip, the learner's pi tower with the softmax head and the
cloning derivative) and the Python layer over it (rl_rocket_amd/bc.py), against tests/bc_discrete_ref.py:
the loss in PyTorch autograd, float64, on the same fp32 inputs, and bc_ref.adam_step_ref for the optimizer.
The fused path is never its own reference. No test here hands the kernel an invalid index: those cases are
tests/test_bc_discrete_host.py's.

1. Gradients and the seven statistics at the batch sizes where the kernel changes path, minibatches drawn
   from 17 001 rows. Bars, the learner's own (tests/test_gpu_ppo_edges.py, tests/test_gpu_bc.py): per tensor
   max |fused - fp64| <= 1e-4 max |fp64| + 1e-7; statistics 1e-5 relative + 1e-6. The value half is bitwise
   zero at l2_weight 0 and l2_weight w within one fp32 rounding otherwise.
2. The loss terms off their defaults: ent_weight 0 / 0.1, l2_weight 0.01, a head whose probability
   underflows to 0 and that some demonstrations name, a sharply peaked policy, one index on every row.
3. Rows outside the minibatch are NaN: bitwise the result of clean rows. At K = 2 and 3 the head gradients
   sit inside larger buffers whose floats after them stay.
4. The optimizer half of 6 calls against float64 Adam on the gradients each call left.
5. The same call twice, stats = NULL, a chained epoch against one that packs per call, a captured epoch
   against the eager one: bitwise. Chained misuse is refused.
6. bc_train fused against fused=False over a few epochs.
7. Demonstrations from a Categorical collect are its buffers, and cloning a fresh policy on them raises
   prob_true_act.
8. The compat kick-starter on integer-action tuples on the device."""
import copy
import os
import sys

import numpy as np
import pytest

import bc_discrete_ref as R
import bc_ref
import discrete_ref as D
from bc_gpu_common import BcHelpers

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ROWS = R.N_ROWS

# one_call asserts step._call and len(step.params) == 12; check_against_fp64 that a.shape == w.shape
_H = BcHelpers(R, R.NAMES, R.VF_NAMES, "rr_bc_update_discrete", lambda: R.sweep_inputs(4))
_minibatch, _adam, _one_call, _check_against_fp64, _state, _epoch = (
    _H.minibatch, _H.adam, _H.one_call, _H.check_against_fp64, _H.state, _H.epoch)


# K = 4: the minimum, the 32-sample tile's edges, one past a workgroup, 33 workgroups, one past kMaxWG
# workgroups x 4 waves x 32 samples (a wave's second tile)
SWEEP = [(bs, 4) for bs in (2, 31, 32, 33, 129, 4097, 16385)] + [(33, 3), (4097, 3), (3, 2), (33, 2)]


@pytest.mark.parametrize("bs,k", SWEEP)
def test_gradients_and_statistics_batch_size_sweep(bs, k):
    pol0, obs, acts = R.sweep_inputs(k)
    idx = _minibatch(bs)
    label = "bs=%d K=%d" % (bs, k)
    _, grads, stats = _one_call(pol0, obs, acts, idx)
    st = _check_against_fp64(label, pol0, obs, acts, idx, grads, stats)
    assert 0.0 < st[1] <= np.log(k) + 1e-12
    _, grads, stats = _one_call(pol0, obs, acts, idx, l2_weight=0.01)
    _check_against_fp64(label + " l2", pol0, obs, acts, idx, grads, stats, l2_weight=0.01)


TERMS = {"ent0": dict(ent_weight=0.0), "ent0.1": dict(ent_weight=0.1), "l2_0.01": dict(l2_weight=0.01),
         "underflow": dict(ent_weight=0.1), "peaked": dict(ent_weight=0.1), "same_index": dict(ent_weight=0.1)}


@pytest.mark.parametrize("bs", [1000, 33])
@pytest.mark.parametrize("name", list(TERMS))
def test_loss_terms_off_their_defaults(name, bs):
    """underflow: the last head's bias is -120, so its probability is 0 in fp32 (~e^-120 in float64) and its
    entropy term counts 0; every seventh row demonstrates that head (log p ~ -120: finite). peaked: the head
    scaled by 8, probabilities near 0 and 1. same_index: every row demonstrates choice 1."""
    import torch

    n, k = 1500, 4
    kw = {"underflow": dict(bias_last=-120.0), "peaked": dict(head_scale=8.0)}.get(name, {})
    pol, obs, acts = R.case_inputs(k, n=n, seed=600 + sorted(TERMS).index(name), **kw)
    if name == "underflow":
        acts[::7] = float(k - 1)
    if name == "same_index":
        acts.fill_(1.0)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(bs))[:bs].contiguous().cuda()
    _, grads, stats = _one_call(pol, obs, acts, idx, **TERMS[name])
    st = _check_against_fp64("%s bs=%d" % (name, bs), pol, obs, acts, idx, grads, stats, **TERMS[name])
    if name == "ent0":
        assert stats[2].item() == 0.0
    if name == "underflow":
        with torch.no_grad():
            p = torch.softmax(pol(obs[idx])[0], -1)
        assert bool((p[:, k - 1] == 0.0).all()) and int((acts[idx] == k - 1).sum()) >= 2
        assert st[0] > 10.0 and 0.0 < stats[1].item() <= np.log(k - 1) + 1e-6  # three live choices
    if name == "peaked":
        assert st[1] < 0.5 * np.log(k)
    if name == "same_index":
        assert bool((acts[idx] == 1.0).all())


@pytest.mark.parametrize("bs,k", [(33, 4), (16385, 4), (33, 3), (33, 2), (4097, 2)])
def test_reads_nothing_outside_the_minibatch_and_writes_nothing_past_the_head(bs, k):
    """idx is the head of a longer tensor of valid rows; every row of obs / acts that idx[:bs] does not name
    is NaN. Gradients, statistics, parameters and Adam state are bitwise those of clean rows. BCUpdate checks
    every index of the demonstrations it is given, so the rows are made NaN in the tensors it holds after it
    was built on clean ones. The action head's gradients are views of larger buffers: the floats after
    [K][64] and [K] keep their fill."""
    import torch
    from rl_rocket_amd.bc import BCUpdate, Demonstrations
    from rl_rocket_amd.rollout import _policy_tensors

    pol0, obs, acts = R.sweep_inputs(k)
    long_idx = _minibatch(bs, extra=97)
    idx = long_idx[:bs]
    assert idx.data_ptr() == long_idx.data_ptr() and idx.is_contiguous()
    outside = torch.ones(N_ROWS, dtype=torch.bool, device=DEV)
    outside[idx] = False
    assert bool(outside[long_idx[bs:]].all())
    out = []
    for poison in (False, True):
        o, a = obs.clone(), acts.clone()
        pol = copy.deepcopy(pol0)
        big_w = torch.full((4 * 64 + 64,), -7.0, device=DEV)
        big_b = torch.full((4 + 64,), -7.0, device=DEV)
        pol.action_net.weight.grad = big_w[:k * 64].view(k, 64)
        pol.action_net.bias.grad = big_b[:k]
        opt = _adam(pol)
        step = BCUpdate(pol, opt, Demonstrations(o, a), bs, 0.01, 0.01)
        assert pol.action_net.weight.grad.data_ptr() == big_w.data_ptr()
        if poison:
            o[outside] = float("nan")
            a[outside] = float("nan")
            assert step.demos.obs.data_ptr() == o.data_ptr() and int(torch.isnan(step.demos.acts).sum()) == N_ROWS - bs
        stats = step(idx).clone()
        torch.cuda.synchronize()
        assert bool((big_w[k * 64:] == -7.0).all()) and bool((big_b[k:] == -7.0).all())
        assert bool((big_w[:k * 64] != -7.0).all()) and bool((big_b[:k] != -7.0).all())
        ts = _policy_tensors(pol)
        out.append(([t.grad.clone() for t in ts], [t.detach().clone() for t in ts],
                    [opt.state[t][s].clone() for t in ts for s in ("exp_avg", "exp_avg_sq", "step")], stats))
    (ga, pa, sa, ta), (gb, pb, sb, tb) = out
    assert all(bool(torch.isfinite(g).all()) for g in ga) and bool(torch.isfinite(ta).all())
    for name, a, b in zip(R.NAMES, ga, gb):
        assert torch.equal(a, b), name
    for a, b in zip(pa + sa, pb + sb):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert torch.equal(ta, tb)


def test_optimizer_half_matches_float64_adam():
    """After each of 6 calls (a learning-rate change after 3, l2 on so that the value half moves, K = 3):
    parameters, exp_avg and exp_avg_sq are float64 Adam applied, from the fp32 state the call started from,
    to the gradients it left; step counts the calls on all 12 tensors. Bars of tests/test_gpu_bc.py."""
    import torch
    from rl_rocket_amd.bc import BCUpdate, Demonstrations
    from rl_rocket_amd.rollout import _policy_tensors

    pol0, obs, acts = R.sweep_inputs(3)
    pol = copy.deepcopy(pol0)
    opt = _adam(pol)
    step = BCUpdate(pol, opt, Demonstrations(obs, acts), 1000, ent_weight=0.01, l2_weight=0.01)
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
        p64, m64, v64, n = bc_ref.adam_step_ref(before, [t.grad for t in tensors], m0, v0, call, lr)
        assert n == call + 1
        for name, t, p, m, v in zip(R.NAMES, tensors, p64, m64, v64):
            st = opt.state[t]
            assert float(st["step"]) == call + 1, name
            assert (t.detach().double() - p).abs().max().item() <= 1e-6 * max(1.0, p.abs().max().item()), name
            assert torch.allclose(st["exp_avg"].double(), m, rtol=1e-5, atol=1e-9), name
            assert torch.allclose(st["exp_avg_sq"].double(), v, rtol=1e-5, atol=1e-12), name
            assert not torch.equal(t.detach(), before[R.NAMES.index(name)]), name
    assert all(float(opt.state[t]["step"]) == 6.0 for t in tensors) and len(tensors) == 12


def test_same_call_twice_gives_the_same_bits():
    import torch

    pol0, obs, acts = R.sweep_inputs(4)
    idx = _minibatch(16385)
    (pa, ga, sa), (pb, gb, sb) = _one_call(pol0, obs, acts, idx), _one_call(pol0, obs, acts, idx)
    for a, b in zip(ga + list(pa.parameters()) + [sa], gb + list(pb.parameters()) + [sb]):
        assert torch.equal(a, b)


def test_without_a_statistics_block_is_the_same_step():
    """stats = NULL through the C ABI (the finish launches no statistics block): gradients, parameters and
    Adam state are bitwise those of the call that writes statistics."""
    import ctypes

    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.bc import BCUpdate, Demonstrations

    pol0, obs, acts = R.sweep_inputs(3)
    idx = _minibatch(4097)
    out = []
    for with_stats in (True, False):
        pol = copy.deepcopy(pol0)
        opt = _adam(pol)
        s = BCUpdate(pol, opt, Demonstrations(obs, acts), 4097, 0.01, 1e-3)
        s.stats.fill_(-7.0)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(s._lib.rr_bc_update_discrete(7, 3, s._params_w, s._dst, s._m, s._v, s._s, obs.data_ptr(),
                                                acts.data_ptr(), idx.data_ptr(), 4097, 0.01, 1e-3, s.lr.data_ptr(),
                                                0.9, 0.999, 1e-8, s.stats.data_ptr() if with_stats else None, 0,
                                                s.ws.data_ptr(), s._nbytes, stream), "rr_bc_update_discrete")
        out.append((_state(pol, opt), s.stats.clone()))
    (a, sa), (b, sb) = out
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)
    assert bool((sb == -7.0).all()) and sa[0].item() > 0.0 and sa[7].item() == 0.0


def test_chained_epoch_is_bitwise_the_packed_and_the_replayed_one():
    import torch

    packed, st_p = _epoch("packed")
    chained, st_c = _epoch("chained")
    replayed, st_g = _epoch("graph")
    assert len(packed) == len(chained) == len(replayed) == 12 * 5 and len(st_p) == len(st_c) == len(st_g) == 3
    for k, (a, b, c) in enumerate(zip(packed, chained, replayed)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(a, c), (R.NAMES[k // 5], k % 5)
    for a, b in zip(st_p, st_c):
        assert torch.equal(a, b)
    for a, c in zip(st_p, st_g):
        assert torch.equal(a, c)
    assert float(packed[4]) == 3.0


def test_chained_misuse_is_refused():
    import torch
    from rl_rocket_amd.bc import BCUpdate, Demonstrations

    pol0, obs, acts = R.sweep_inputs(2)
    pol = copy.deepcopy(pol0)
    step = BCUpdate(pol, _adam(pol), Demonstrations(obs, acts), 64)
    idx = _minibatch(64)
    with pytest.raises(ValueError, match="chained"):  # no call before it
        step(idx, chained=True)
    step(idx)
    step(idx, chained=True)
    with torch.no_grad():
        pol.action_net.bias.add_(0.1)  # somebody else wrote a parameter: the packed image is stale
    with pytest.raises(ValueError, match="chained"):
        step(idx, chained=True)
    step(idx)
    with pytest.raises(ValueError, match="idx"):
        step(_minibatch(65))
    with pytest.raises(ValueError, match="idx"):
        step(idx.int())
    pol.action_net.bias.grad = torch.zeros_like(pol.action_net.bias)
    with pytest.raises(RuntimeError, match="replaced"):
        step(idx)
    assert set(step.last_stats()) == set(R.STATS)


def test_bc_train_tracks_autograd():
    """3 epochs of 4 minibatches on 8192 rows, fused against fused=False from equal starts and the same
    shuffling: parameters within 5 % of how far training moved them (the bar and its reason:
    test_gpu_ppo.test_fused_update_with_the_shipped_adam_tracks_autograd), and both fit the demonstrations
    better than the start. fused=None picks the fused call."""
    import torch
    from rl_rocket_amd import bc
    from rl_rocket_amd.bc import Demonstrations, bc_train

    pol0, obs, acts = R.sweep_inputs(4)
    demos = Demonstrations(obs[:8192].contiguous(), acts[:8192].contiguous())
    pols = [copy.deepcopy(pol0) for _ in range(3)]
    opts = [_adam(p) for p in pols]
    gen = lambda: torch.Generator(DEV).manual_seed(21)  # noqa: E731
    sa = bc_train(pols[0], opts[0], demos, n_epochs=3, batch_size=2048, generator=gen(), fused=False)
    sb = bc_train(pols[1], opts[1], demos, n_epochs=3, batch_size=2048, generator=gen(), fused=True)
    made = []
    real = bc.BCUpdate

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    bc.BCUpdate = Spy
    try:
        sc = bc_train(pols[2], opts[2], demos, n_epochs=3, batch_size=2048, generator=gen())
    finally:
        bc.BCUpdate = real
    torch.cuda.synchronize()
    assert len(made) == 1 and made[0]._call == "rr_bc_update_discrete" and sc == sb
    for x, y in zip(pols[1].parameters(), pols[2].parameters()):
        assert torch.equal(x, y)
    assert float(opts[0].state[pols[0].action_net.bias]["step"]) == float(opts[1].state[pols[1].value_net.bias]["step"]) == 12.0
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


def test_demonstrations_from_a_categorical_collect_clone_a_fresh_policy():
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.bc import Demonstrations, bc_train
    from rl_rocket_amd.rollout import DeviceRollout, MlpCategoricalActorCritic

    n, T, k = 300, 4, 4
    teacher = D.cat_policy(k, 31, head_scale=2.0).to(DEV)
    env = RocketBatch(n, model=3, device=DEV, max_episode_steps=30, seed=5)
    ro = DeviceRollout(env, teacher, n_steps=T, seed=4)
    assert ro.discrete and ro.actions.shape == (T, n, 1)
    ro.collect()
    torch.cuda.synchronize()
    d = Demonstrations.from_rollout(ro)
    assert len(d) == T * n and d.obs.data_ptr() == ro.obs.data_ptr() and d.acts.data_ptr() == ro.actions.data_ptr()
    assert d.acts.shape == (T * n, 1) and torch.equal(d.acts[:, 0], ro.actions.reshape(T * n))
    assert torch.equal(d.obs[n + 5], ro.obs[1, 5]) and len(set(d.acts[:, 0].tolist())) == k
    torch.manual_seed(12)
    student = MlpCategoricalActorCritic(7, k, D.TABLES[k]).to(DEV)
    every = torch.arange(T * n, device=DEV)
    before = R.reference(student, d.obs, d.acts, every)[1]
    opt = _adam(student)
    st = bc_train(student, opt, d, n_epochs=30, batch_size=T * n // 2)
    torch.cuda.synchronize()
    after = R.reference(student, d.obs, d.acts, every)[1]
    print("prob_true_act %.6f -> %.6f, neglogp %.6f -> %.6f" % (before[3], after[3], before[0], after[0]), st)
    assert float(opt.state[student.action_net.bias]["step"]) == 60.0
    assert after[3] > before[3] and after[0] < before[0]
    env.close()


def test_compat_kickstarter_trains_on_integer_action_tuples():
    import torch

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat")
    if path not in sys.path:
        sys.path.insert(0, path)
    from my_environment.utils.imitation_kickstarter import imitationKickstarter
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic, _policy_tensors

    _, obs, acts = R.sweep_inputs(4)
    o, a = obs[:201].cpu().numpy(), acts[:200, 0].cpu().numpy().astype(np.int64)
    cuts = (0, 90, 91, 200)
    tuples = [(o[lo:hi + 1], a[lo:hi], [{}] * (hi - lo), True) for lo, hi in zip(cuts[:-1], cuts[1:])]
    torch.manual_seed(8)
    student = MlpCategoricalActorCritic(7, 4, D.TABLES[4]).to(DEV)
    before = [t.detach().clone() for t in _policy_tensors(student)]
    kick = imitationKickstarter(policy=student)
    kick.trajectories = tuples
    assert kick.train(n_epochs=2) is student and kick.policy is student
    torch.cuda.synchronize()
    for name, x, t in zip(R.NAMES, before, _policy_tensors(student)):  # the value half's gradient is zero
        assert bool(torch.isfinite(t).all()) and torch.equal(x, t) == (name in R.VF_NAMES), name
    assert float(kick.optimizer.state[student.action_net.bias]["step"]) == 2 * (200 // 32)
    assert set(kick.stats) == set(R.STATS) and kick.stats["neglogp"] == kick.stats["neglogp"]
    assert 0.0 < kick.stats["entropy"] <= np.log(4.0) + 1e-6
