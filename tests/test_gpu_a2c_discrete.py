"""rr_a2c_update_discrete (A2C for the Categorical policy on the device:
rl_rocket_amd/csrc/a2c_discrete/rocket_a2c_discrete.hip, the PPO learner's towers with the softmax head, the
A2C head derivative and the per-sample entropy gradient) and the Python layer over it
(rl_rocket_amd/a2c_discrete.py), against tests/a2c_discrete_ref.py: the loss in PyTorch autograd, float64, on
the same fp32 inputs, and a2c_ref's three optimizers written out in float64. The fused path is never its own
reference. Shapes are the smallest at which the kernel changes path.

1. Gradients and the five statistics at the batch sizes where the kernel changes path, rows drawn from the
   70 001-row pool of discrete_edge_ref, K = 4, 3, 2, normalize_advantage on and off. Bars, the learner's own
   (tests/test_gpu_a2c.py, tests/test_gpu_ppo_edges.py): per tensor max |fused - fp64| <= 1e-4 max |fp64| +
   1e-7; statistics 1e-5 relative + 1e-6. The torch-fp32 error is printed beside each
   (tests/test_a2c_discrete_host.py asserts on the CPU that it has room under every bar).
2. Heads past K: the gradients are [K][64] and [K] views in the middle of a larger patterned buffer.
3. The loss terms off their defaults.
4. Rows outside the minibatch are NaN, ro.log_probs is all NaN: bitwise the result of clean rows.
5. The optimizer half of 6 calls, for each optimizer, against float64 on the gradients each call left.
6. The same call twice; the call without a statistics block.
7. The workspace's carving.
8. a2c_update_discrete fused against fused=False on a real 3DOF batch.
9. GraphedA2CDiscrete's replays against eager iterations, bitwise.
10. The refusals only a device rollout reaches: a rollout under 2 rows, and the two-launch and per-step
    collects inside GraphedA2CDiscrete, each by its message."""
import copy
import ctypes

import pytest

import a2c_discrete_ref as A
import discrete_edge_ref as E
import ppo_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ROWS = A.N_ROWS
PI_SIDE = P.PI_NAMES


def _minibatch(bs):
    return E.minibatch(N_ROWS, bs).cuda()


def _update(pol, data, kind="tf", lr=1e-3, **kw):
    """(A2CUpdateDiscrete, optimizer) on a stub rollout of the flat tensors `data` = (obs, act, adv, ret);
    ro.log_probs is all NaN."""
    from rl_rocket_amd.a2c_discrete import A2CUpdateDiscrete

    opt = A.make_optimizer(kind, pol, lr)
    return A2CUpdateDiscrete(pol, opt, A.rollout(*data), **kw), opt


def _one_call(pol0, data, idx, normalize=False, ent_coef=0.0, vf_coef=0.5, max_grad_norm=None, kind="tf"):
    """A copy of pol0 after one fused call on idx: (policy, its gradients fp32, the 8 stats). Without a clip
    the gradients the call leaves are the loss's own."""
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    pol = copy.deepcopy(pol0)
    step, _ = _update(pol, data, kind, normalize_advantage=normalize, ent_coef=ent_coef, vf_coef=vf_coef,
                      max_grad_norm=max_grad_norm)
    stats = step(idx).clone()
    torch.cuda.synchronize()
    return pol, [t.grad.clone() for t in _policy_tensors(pol)], stats


def _check_against_fp64(label, pol0, data, idx, grads, stats, normalize=False, ent_coef=0.0, vf_coef=0.5):
    """The learner's bars on the gradients a call left and its statistics; pol0 holds the parameters the call
    started from. Returns the float64 gradients."""
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    kw = dict(normalize=normalize, ent_coef=ent_coef, vf_coef=vf_coef)
    ref64, st64 = A.reference(pol0, *data, idx, torch.float64, **kw)
    ref32, st32 = A.reference(pol0, *data, idx, torch.float32, **kw)
    assert len(grads) == len(ref64) == 12
    for name, a, r, t, w in zip(A.NAMES, grads, ref64, ref32, _policy_tensors(pol0)):
        a = a.double().cpu()
        scale = r.abs().max().item()
        err, err32 = (a - r).abs().max().item(), (t - r).abs().max().item()
        print("%s %-9s max|ref| %.3e  fused err %.2e  torch-fp32 err %.2e" % (label, name, scale, err, err32))
        assert a.shape == w.shape and bool(torch.isfinite(a).all()), name
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale, err32)
    st = stats.tolist()
    assert all(v == v and abs(v) != float("inf") for v in st), st
    assert st[5:] == [0.0, 0.0, 0.0]
    for name, a, r, t in zip(A.STATS, st, st64, st32):
        print("%s %-12s fp64 %.9e  fused err %.2e  torch-fp32 err %.2e" % (label, name, r, abs(a - r), abs(t - r)))
        assert abs(a - r) <= 1e-5 * abs(r) + 1e-6, (name, a, r)
    return ref64


# 129: a second workgroup; 4097: one past 32 workgroups; 16 385: one past kMaxWG workgroups x 4 waves x 32
# samples, a wave's second tile; 40 001: a ragged third tile
SWEEP = [(bs, 4) for bs in (2, 31, 32, 33, 129, 4097, 16385, 40001)] + [(bs, k) for k in (3, 2) for bs in (3, 33, 4097)]


@pytest.mark.parametrize("normalize", (False, True))
@pytest.mark.parametrize("bs,k", SWEEP)
def test_gradients_and_statistics_batch_size_sweep(bs, k, normalize):
    pol0, *data = A.sweep_gpu(k)
    idx = _minibatch(bs)
    _, grads, stats = _one_call(pol0, data, idx, normalize, ent_coef=0.01)
    assert grads[8].shape == (k, 64) and grads[9].shape == (k,)
    _check_against_fp64("bs=%d K=%d norm=%d" % (bs, k, normalize), pol0, data, idx, grads, stats, normalize, ent_coef=0.01)


@pytest.mark.parametrize("k", (2, 3))
@pytest.mark.parametrize("bs", (33, 4097))
def test_heads_past_k_write_nothing_past_the_gradient_tensors(k, bs):
    """W_action.grad [K][64] and b_action.grad [K] are views in the middle of a larger buffer pre-filled with a
    bit pattern: the elements before and after them keep it (the zero sums of heads >= K go to the sink)."""
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    pol0, *data = A.sweep_gpu(k)
    pol = copy.deepcopy(pol0)
    pattern = (0x7FC5A000 + torch.arange(1024, dtype=torch.int32)).to(DEV)  # NaNs with a payload
    buf = pattern.clone().view(torch.float32)
    t = _policy_tensors(pol)
    w0, b0 = 256, 256 + 64 * k + 64  # 16-B aligned starts, a gap of 64 floats between the two
    t[8].grad = buf[w0:w0 + 64 * k].view(k, 64)
    t[9].grad = buf[b0:b0 + k]
    step, _ = _update(pol, data, normalize_advantage=True, ent_coef=0.01, max_grad_norm=None)
    assert step._tensors[8][1] is t[8].grad and step._tensors[9][1] is t[9].grad
    idx = _minibatch(bs)
    stats = step(idx).clone()
    torch.cuda.synchronize()
    grads = [x.grad.clone() for x in t]
    assert grads[8].shape == (k, 64) and grads[9].shape == (k,)
    bits = buf.view(torch.int32)
    keep = torch.ones(1024, dtype=torch.bool, device=DEV)
    keep[w0:w0 + 64 * k] = False
    keep[b0:b0 + k] = False
    assert torch.equal(bits[keep], pattern[keep])
    assert bool(torch.isfinite(buf[~keep]).all())
    _check_against_fp64("views K=%d bs=%d" % (k, bs), pol0, data, idx, grads, stats, True, ent_coef=0.01)


_terms_cache = {}


def _terms_case(name, bs):
    if (name, bs) not in _terms_cache:
        pol, data, idx, kw = A.terms_case(name, bs)
        _terms_cache[name, bs] = (pol.cuda(), [t.cuda() for t in data], idx.cuda(), kw)
    return _terms_cache[name, bs]


@pytest.mark.parametrize("bs", A.TERM_BATCHES)
@pytest.mark.parametrize("name", list(A.TERMS))
def test_loss_terms_off_their_defaults(name, bs):
    import torch

    pol0, data, idx, kw = _terms_case(name, bs)
    _, grads, stats = _one_call(pol0, data, idx, **kw)
    ref64 = _check_against_fp64("%s bs=%d" % (name, bs), pol0, data, idx, grads, stats, **kw)
    if name == "const_adv_ent0":  # A = 0 on every row and no entropy term: the policy half has no gradient at all
        for nm, gr in zip(A.NAMES, grads):
            if nm in PI_SIDE:
                assert torch.count_nonzero(gr).item() == 0, nm
        assert stats[0].item() == 0.0
    if name == "const_adv_ent0.1":  # the pi gradients are the entropy's alone (the reference's A is 0 too)
        assert stats[0].item() == 0.0
        for nm, gr, r in zip(A.NAMES, grads, ref64):
            if nm in PI_SIDE:
                assert torch.count_nonzero(gr).item() > 0 and r.abs().max().item() > 0.0, nm


@pytest.mark.parametrize("bs", [33, 16385])
@pytest.mark.parametrize("normalize", (False, True))
def test_reads_only_the_minibatch_rows_and_never_the_log_probs(bs, normalize):
    import torch

    pol0, *data = A.sweep_gpu(4)
    idx = _minibatch(bs)
    keep = torch.zeros(N_ROWS, dtype=torch.bool, device=DEV)
    keep[idx] = True
    dirty = [torch.where(keep.view(-1, *[1] * (t.dim() - 1)), t, torch.full_like(t, float("nan"))) for t in data]
    assert all(int(torch.isnan(t).any(-1).sum() if t.dim() > 1 else torch.isnan(t).sum()) == N_ROWS - bs for t in dirty)
    kw = dict(normalize=normalize, ent_coef=0.01, max_grad_norm=0.5)
    pa, ga, sa = _one_call(pol0, data, idx, **kw)
    # (the constructor's index check reads every row: built on the clean rollout, then pointed at the dirty one)
    from rl_rocket_amd.rollout import _policy_tensors

    pb = copy.deepcopy(pol0)
    step, _ = _update(pb, data, normalize_advantage=normalize, ent_coef=0.01, max_grad_norm=0.5)
    step.data = dirty
    sb = step(idx).clone()  # ro.log_probs: NaN, and no argument of the call
    torch.cuda.synchronize()
    gb = [t.grad.clone() for t in _policy_tensors(pb)]
    for a, b in zip(ga + list(pa.parameters()) + [sa], gb + list(pb.parameters()) + [sb]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("kind", A.KINDS)
def test_optimizer_half_matches_float64(kind):
    """After each of 6 calls (a learning-rate change after 3; max_grad_norm 0.5, a loose 1e6, none):
    parameters and optimizer state are the float64 step applied, from the fp32 state the call started from,
    to the gradients it left; those are the float64 loss gradients times clip_grad_norm_'s coefficient; step
    counts the calls on all 12 tensors. Bars of test_gpu_a2c.test_a2c_optimizer_half_matches_float64."""
    import torch
    from rl_rocket_amd.a2c_discrete import A2CUpdateDiscrete
    from rl_rocket_amd.rollout import _policy_tensors

    pol0, *data = A.sweep_gpu(4)
    second = "exp_avg_sq" if kind == "adam" else "square_avg"
    g = torch.Generator().manual_seed(9)
    pol = copy.deepcopy(pol0)
    tensors = _policy_tensors(pol)
    steps = {}
    opt = A.make_optimizer(kind, pol, 1e-3)
    ro = A.rollout(*data)
    for clip in (0.5, 1e6, None):  # one optimizer, three bindings of its state
        steps[clip] = A2CUpdateDiscrete(pol, opt, ro, normalize_advantage=True, ent_coef=0.01, max_grad_norm=clip)
    bit = []
    for call, clip in enumerate((0.5, 0.5, 1e6, None, 0.5, None)):
        if call == 3:
            opt.param_groups[0]["lr"] = 2.5e-4
        lr = opt.param_groups[0]["lr"]
        idx = torch.randperm(N_ROWS, generator=g)[:1000 if call != 4 else 333].contiguous().cuda()
        before = copy.deepcopy(pol)
        state = dict(step=call)
        state[second] = [opt.state[t][second].double().cpu().clone() for t in tensors]
        if kind == "adam":
            state["exp_avg"] = [opt.state[t]["exp_avg"].double().cpu().clone() for t in tensors]
        steps[clip](idx)
        torch.cuda.synchronize()
        left = [t.grad.cpu().clone() for t in tensors]
        raw, _ = A.reference(before, *data, idx, torch.float64, normalize=True, ent_coef=0.01)
        coef = P.clip_coef64(raw, clip) if clip else 1.0
        bit.append(coef < 1.0)
        for name, a, r in zip(A.NAMES, left, raw):
            assert (a.double() - coef * r).abs().max().item() <= 1e-4 * coef * r.abs().max().item() + 1e-7, (call, name)
        p64 = [t.detach().double().cpu().clone() for t in _policy_tensors(before)]
        A.optimizer_ref(kind, p64, left, state, lr)
        assert state["step"] == call + 1
        for i, (name, t, p) in enumerate(zip(A.NAMES, tensors, p64)):
            st = opt.state[t]
            assert float(st["step"]) == call + 1, name
            assert (t.detach().double().cpu() - p).abs().max().item() <= 1e-6 * max(1.0, p.abs().max().item()), (call, name)
            assert torch.allclose(st[second].double().cpu(), state[second][i], rtol=1e-5, atol=1e-12), (call, name)
            if kind == "adam":
                assert torch.allclose(st["exp_avg"].double().cpu(), state["exp_avg"][i], rtol=1e-5, atol=1e-9), (call, name)
            if not bit[-1]:  # (under the clip a step can be below half an ulp of every element of a tensor)
                assert not torch.equal(t.detach(), _policy_tensors(before)[i]), name
    assert bit == [True, True, False, False, True, False]  # the returns' scale puts the norm ~8x over 0.5
    assert all(float(opt.state[t]["step"]) == 6.0 for t in tensors) and len(tensors) == 12


def _raw_call(step, idx, stats, ws=None):
    """rr_a2c_update_discrete through the C ABI with A2CUpdateDiscrete's own arrays, on `ws` (a uint8 tensor)
    or its own."""
    import torch
    from rl_rocket_amd import _lib

    kind, lr, a, b2, eps = step._opt_args()
    _lib.check(step._lib.rr_a2c_update_discrete(
        step.ns, step.na, *step._ptrs, *[t.data_ptr() for t in step.data], idx.data_ptr(), idx.numel(),
        int(step.normalize), step.ent_coef, step.vf_coef, step.max_norm, kind, lr, a, b2, eps,
        None if stats is None else stats.data_ptr(), (step.ws if ws is None else ws).data_ptr(), step._nbytes,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "rr_a2c_update_discrete")


def _state(pol, opt):
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    torch.cuda.synchronize()
    out = []
    for t in _policy_tensors(pol):
        out += [t.detach().clone(), t.grad.clone()] + [v.clone() for _, v in sorted(opt.state[t].items())]
    return out


@pytest.mark.parametrize("kind", A.KINDS)
def test_same_call_twice_and_without_statistics_gives_the_same_bits(kind):
    import torch

    pol0, *data = A.sweep_gpu(3)
    idx = _minibatch(40001)
    out = []
    for with_stats in (True, True, False):
        pol = copy.deepcopy(pol0)
        step, opt = _update(pol, data, kind, normalize_advantage=True, ent_coef=0.01)
        step.stats.fill_(-7.0)
        _raw_call(step, idx, step.stats if with_stats else None)
        out.append(_state(pol, opt) + [step.stats.clone()])
    a, b, c = out
    assert len(a) == 12 * (5 if kind == "adam" else 4) + 1
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(a[:-1], c[:-1]):
        assert torch.equal(x, y)
    assert bool((c[-1] == -7.0).all()) and not bool((a[-1] == -7.0).any())  # NULL: the block is not written


@pytest.mark.parametrize("bs,k", [(33, 4), (129, 4), (33, 2), (129, 2)])
def test_workspace_carving_leaves_the_tail_and_reads_no_state(bs, k):
    """The call on a workspace that is the first `bytes` of a larger buffer: the 256 floats after it keep
    their bit pattern, and parameters, gradients, optimizer state and statistics are bitwise those of the
    same call on a workspace pre-filled with 0xFF bytes (NaNs): the call reads no state from the workspace
    (the sink included), and the host's sections lie inside the size rr_a2c_update_discrete_workspace_size
    returned for THIS batch."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.a2c_discrete import A2CUpdateDiscrete

    pol0, *data = A.sweep_gpu(k)
    rows = [_minibatch(bs), _minibatch(bs + 1)[1:].contiguous()]
    tail = (0x5A5A0000 + torch.arange(256, dtype=torch.int32)).to(DEV)
    small = [t[:bs].contiguous() for t in data]  # a rollout of bs rows sizes the workspace for bs
    out = []
    for fill in (0x00, 0xFF):
        pol = copy.deepcopy(pol0)
        opt = A.make_optimizer("tf", pol, 1e-3)
        s = A2CUpdateDiscrete(pol, opt, A.rollout(*small), normalize_advantage=True, ent_coef=0.01)
        s.data = list(data)  # the call's rows come from the whole pool; bs rows of it per call
        need = ctypes.c_int64()
        assert s._lib.rr_a2c_update_discrete_workspace_size(7, k, bs, ctypes.byref(need)) == _lib.RR_OK
        assert s._nbytes == need.value and need.value % 16 == 0
        buf = torch.full((s._nbytes + 4 * 256,), fill, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        buf[s._nbytes:].view(torch.int32).copy_(tail)
        stats = []
        for ix in rows:
            _raw_call(s, ix, s.stats, ws=buf)
            stats.append(s.stats.clone())
        out.append((_state(pol, opt) + stats, buf[s._nbytes:].view(torch.int32).clone()))
    (a, ta), (b, tb) = out
    assert torch.equal(ta, tail) and torch.equal(tb, tail)
    assert len(a) == len(b) == 4 * 12 + 2
    for x, y in zip(a, b):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def _env(n=256, seed=77, **over):
    from rl_rocket_amd.batch import RocketBatch

    return RocketBatch(n, model=3, device=DEV, max_episode_steps=30, seed=seed, **over)


def _policy(k=4):
    from discrete_ref import cat_policy

    return cat_policy(k, 100 + k).to(DEV)


def test_a2c_update_discrete_fused_tracks_autograd_on_a_real_batch():
    """5 iterations of collect + a2c_update_discrete on two 3DOF batches of 256 envs from equal starts
    (TimeLimit 30, n_steps 5, gae_lambda 1: SB3's A2C defaults), fused against fused=False: parameters within
    5 % of how far training moved them, statistics within 2 % (the bars of
    test_gpu_a2c.test_a2c_update_fused_tracks_autograd_on_a_real_batch)."""
    import torch
    from rl_rocket_amd.a2c import RMSpropTFLike
    from rl_rocket_amd.a2c_discrete import a2c_update_discrete
    from rl_rocket_amd.rollout import DeviceRollout

    runs = []
    for fused in (False, True):
        env = _env()
        pol = _policy()
        pol0 = copy.deepcopy(pol)
        opt = RMSpropTFLike(pol.parameters(), lr=7e-4)
        ro = DeviceRollout(env, pol, n_steps=5, gae_lambda=1.0, seed=5, one_launch=True)
        for _ in range(5):
            ro.collect()
            st = a2c_update_discrete(pol, opt, ro, ent_coef=0.01, fused=fused)
            assert set(st) == set(A.STATS) and all(v == v for v in st.values())
        torch.cuda.synchronize()
        assert float(opt.state[pol.value_net.bias]["step"]) == 5.0
        runs.append((pol, st))
        env.close()
    (pa, sa), (pb, sb) = runs
    moved = max((x - y).abs().max().item() for x, y in zip(pol0.parameters(), pa.parameters()))
    drift = max((x - y).abs().max().item() for x, y in zip(pa.parameters(), pb.parameters()))
    print("moved %.3e, parameter drift %.3e" % (moved, drift), sa, sb)
    assert moved > 0.0 and drift <= 0.05 * moved, (drift, moved)
    for k in sa:
        assert abs(sa[k] - sb[k]) <= 0.02 * max(1.0, abs(sa[k])), (k, sa[k], sb[k])


@pytest.mark.parametrize("k,kind,normalize,with_stats", [(4, "tf", False, False), (3, "adam", True, False),
                                                         (2, "rmsprop", False, True)])
def test_graphed_a2c_discrete_replays_are_the_eager_iterations(k, kind, normalize, with_stats):
    """Four GraphedA2CDiscrete.step() replays leave bitwise what four eager collect(); update() iterations
    from the same seed leave: parameters, gradients, optimizer state, the statistics, ro.iter, the rollout's
    buffers and the env (its checkpoint); with DeviceRollout(stats=True) also the episode statistics."""
    import torch
    from rl_rocket_amd.a2c_discrete import A2CUpdateDiscrete, GraphedA2CDiscrete
    from rl_rocket_amd.rollout import DeviceRollout

    out = []
    for graphed in (False, True):
        env = _env()
        pol = _policy(k)
        opt = A.make_optimizer(kind, pol, 7e-4)
        ro = DeviceRollout(env, pol, n_steps=5, gae_lambda=1.0, seed=5, one_launch=True, stats=with_stats)
        assert ro.discrete and ro.one_launch and not ro.per_step and (ro.stats is not None) == with_stats
        kw = dict(normalize_advantage=normalize, ent_coef=0.01)
        if graphed:
            it = GraphedA2CDiscrete(pol, opt, ro, **kw)
            assert it.update.n_updates == 0 and int(ro.iter) == 0
            for j in range(4):
                if j == 2:
                    opt.param_groups[0]["lr"] = 3e-4  # read from the device scalar: no new capture
                stats = it.step().clone()
            ts = it.train_stats()
        else:
            upd = A2CUpdateDiscrete(pol, opt, ro, **kw)
            for j in range(4):
                if j == 2:
                    opt.param_groups[0]["lr"] = 3e-4
                ro.collect()
                stats = upd().clone()
            ts = upd.train_stats()
        assert set(ts) == {"train/policy_loss", "train/value_loss", "train/entropy_loss", "train/n_updates"}
        assert ts["train/n_updates"] == 4 and ts["train/entropy_loss"] == -stats[2].item() < 0.0
        torch.cuda.synchronize()
        ck = env.checkpoint()
        extra = [ro.stats.out.clone(), ro.stats.accum.clone()] if with_stats else []
        out.append(_state(pol, opt) + [stats, ro.iter.clone(), ro.last_value.clone(), ro.last_done.clone(),
                                       ro.last_start.clone(), ro.advantages.clone(), ro.returns.clone(), ro.obs.clone(),
                                       ro.actions.clone(), ro.log_probs.clone(), ro.values.clone(), ro.rewards.clone(),
                                       ro.starts.clone(), env.obs.clone(), env.done.clone()]
                   + extra + [ck[name].clone() for name in sorted(ck)])
        env.close()
    a, b = out
    assert len(a) == len(b) and int(a[12 * (5 if kind == "adam" else 4) + 1]) == 4
    for j, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), j
    assert all(bool(torch.isfinite(x).all()) for x in a[:12 * 4])


def test_a_rollout_under_two_rows_is_refused_by_name():
    """The refusal that comes after the CPU-tensor one, so only a device rollout reaches it: one row, for the
    three entry points and for a2c.A2CUpdate, whose message is built by the same line."""
    import torch
    from rl_rocket_amd.a2c import A2CUpdate
    from rl_rocket_amd.a2c_discrete import A2CUpdateDiscrete, GraphedA2CDiscrete, a2c_update_discrete
    from rl_rocket_amd.rollout import MlpActorCritic

    pol = _policy()
    opt = A.make_optimizer("tf", pol, 7e-4)
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    ro = A.rollout(z(1, 7), z(1, 1), z(1), z(1))
    ro.fused, ro.one_launch, ro.per_step = True, True, False  # what GraphedA2CDiscrete asks of a collect
    for f in (A2CUpdateDiscrete, lambda *a: a2c_update_discrete(*a, fused=True), GraphedA2CDiscrete):
        with pytest.raises(ValueError, match="A2CUpdateDiscrete needs a rollout of at least 2 rows"):
            f(pol, opt, ro)
    gauss = MlpActorCritic(7, 2).to(DEV)
    with pytest.raises(ValueError, match="A2CUpdate needs a rollout of at least 2 rows"):
        A2CUpdate(gauss, A.make_optimizer("tf", gauss, 7e-4), A.stub_rollout(7, 2, z(1, 7), z(1, 2), z(1), z(1)))
    A2CUpdateDiscrete(pol, opt, A.rollout(z(2, 7), z(2, 1), z(2), z(2)))  # two rows are taken


def test_graphed_a2c_discrete_refuses_the_other_collects_by_name():
    from rl_rocket_amd.a2c_discrete import GraphedA2CDiscrete
    from rl_rocket_amd.rollout import DeviceRollout

    pol = _policy()
    for kw, match in ((dict(), "the two-launch"), (dict(per_step=True), "the per-step")):
        env = _env(64)
        ro = DeviceRollout(env, pol, n_steps=5, seed=5, **kw)
        with pytest.raises(ValueError, match=match):
            GraphedA2CDiscrete(pol, A.make_optimizer("tf", pol, 7e-4), ro)
        env.close()
