"""rr_a2c_update (A2C on the device: rl_rocket_amd/csrc/a2c/rocket_a2c.hip, the PPO learner's towers with the
A2C head derivative, RMSprop) and the Python layer over it (rl_rocket_amd/a2c.py), against tests/a2c_ref.py:
the loss in PyTorch autograd, float64, on the same fp32 inputs, and the three optimizers written out in
float64. The fused path is never its own reference.

1. Gradients and the five statistics at the batch sizes where the kernel changes path, rows drawn from a
   70 001-row pool, with normalize_advantage on and off. Bars, the learner's own
   (tests/test_gpu_ppo_edges.py): per tensor max |fused - fp64| <= 1e-4 max |fp64| + 1e-7; statistics 1e-5
   relative + 1e-6.
2. The loss terms off their defaults: ent_coef, vf_coef, log_std -2 / +1, actions at +-1, constant
   advantages under normalize_advantage.
3. Rows outside the minibatch are NaN, ro.log_probs is all NaN: bitwise the result of clean rows.
4. The optimizer half of 6 calls, for each optimizer, against float64 on the gradients each call left.
5. The same call twice; the call without a statistics block.
6. The workspace's carving.
7. a2c_update fused against fused=False on a real 6DOF batch.
8. GraphedA2C's replays against eager iterations, bitwise, on 3DOF and 6DOF batches and rollouts of every
   policy_dtype."""
import copy
import ctypes

import pytest

import a2c_ref as R
import ppo_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ROWS = R.N_ROWS


def _minibatch(bs, n=N_ROWS):
    import torch

    return torch.randperm(n, generator=torch.Generator().manual_seed(bs))[:bs].contiguous().cuda()


def _update(pol, data, kind="tf", lr=1e-3, **kw):
    """(A2CUpdate, optimizer) on a stub rollout of the flat tensors `data` = (obs, act, adv, ret)."""
    from rl_rocket_amd.a2c import A2CUpdate

    obs, act = data[0], data[1]
    opt = R.make_optimizer(kind, pol, lr)
    return A2CUpdate(pol, opt, R.stub_rollout(obs.shape[1], act.shape[1], *data), **kw), opt


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
    started from."""
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    kw = dict(normalize=normalize, ent_coef=ent_coef, vf_coef=vf_coef)
    ref64, st64 = R.reference(pol0, *data, idx, torch.float64, **kw)
    ref32, st32 = R.reference(pol0, *data, idx, torch.float32, **kw)
    assert len(grads) == len(ref64) == 13
    for name, a, r, t, w in zip(P.NAMES, grads, ref64, ref32, _policy_tensors(pol0)):
        a = a.double()
        scale = r.abs().max().item()
        err, err32 = (a - r).abs().max().item(), (t - r).abs().max().item()
        print("%s %-9s max|ref| %.3e  fused err %.2e  torch-fp32 err %.2e" % (label, name, scale, err, err32))
        assert a.shape == w.shape and bool(torch.isfinite(a).all()), name
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale, err32)
    st = stats.tolist()
    assert all(v == v and abs(v) != float("inf") for v in st), st
    assert st[5:] == [0.0, 0.0, 0.0]
    for name, a, r, t in zip(R.STATS, st, st64, st32):
        print("%s %-12s fp64 %.9e  fused err %.2e  torch-fp32 err %.2e" % (label, name, r, abs(a - r), abs(t - r)))
        assert abs(a - r) <= 1e-5 * abs(r) + 1e-6, (name, a, r)


# 16 385: one past kMaxWG workgroups x 4 waves x 32 samples, a wave's second tile
SWEEP = [(bs, 14, 3) for bs in (2, 31, 32, 33, 129, 4097, 16385, 40001)] + [(bs, 7, 2) for bs in (3, 33, 4097)]


@pytest.mark.parametrize("normalize", (False, True))
@pytest.mark.parametrize("bs,ns,na", SWEEP)
def test_a2c_gradients_and_statistics_batch_size_sweep(bs, ns, na, normalize):
    pol0, *data = R.sweep_inputs(ns, na)
    idx = _minibatch(bs)
    _, grads, stats = _one_call(pol0, data, idx, normalize, ent_coef=0.01)
    _check_against_fp64("bs=%d (%d,%d) norm=%d" % (bs, ns, na, normalize), pol0, data, idx, grads, stats, normalize,
                        ent_coef=0.01)


TERMS = {"ent0": dict(ent_coef=0.0), "ent0.01": dict(ent_coef=0.01), "ent0.1": dict(ent_coef=0.1),
         "vf0.25": dict(vf_coef=0.25), "logstd-2": {}, "logstd+1": {}, "clipped_actions": {},
         "const_adv": dict(normalize=True)}
_terms_cache = {}


def _terms_case(name, bs):
    """(pol, data, idx) of one case on the GPU, built once on the CPU from 1500 rows (ppo_ref.edge_case's
    sizes). logstd*: log_std on every component and the actions drawn from that policy (unit-normal
    actions sit ~7 sigma off the mean at log_std -2: log-probs near -1000, where one fp32 ulp of the
    log-prob is more than the statistics' bar leaves; ppo_ref.edge_case). clipped_actions: every action
    component at +-1. const_adv: one advantage value on the minibatch's rows: std 0, so the 1e-8 floor
    decides and every normalised advantage is 0 (0.3 - mean is exactly 0 in both precisions)."""
    import torch

    if (name, bs) not in _terms_cache:
        n = 1500
        kw = {"log_std": float(name[len("logstd"):])} if name.startswith("logstd") else {}
        pol, obs, act, adv, ret = R.pool_cpu(14, 3, n, seed=2000 + 10 * sorted(TERMS).index(name) + (bs & 1), **kw)
        g = torch.Generator().manual_seed(bs)
        idx = torch.randperm(n, generator=g)[:bs].contiguous()
        if name.startswith("logstd"):
            with torch.no_grad():
                mean, _ = copy.deepcopy(pol).double()(obs.double())
                eps = torch.randn((n, 3), generator=g, dtype=torch.float64)
                act = (mean + pol.log_std.double().exp() * eps).float().contiguous()
        if name == "clipped_actions":
            act = torch.where(torch.randn((n, 3), generator=g) >= 0, 1.0, -1.0).contiguous()
        if name == "const_adv":
            adv[idx] = 0.3
        _terms_cache[name, bs] = (pol.cuda(), [t.cuda() for t in (obs, act, adv, ret)], idx.cuda())
    return _terms_cache[name, bs]


@pytest.mark.parametrize("bs", [1000, 33])
@pytest.mark.parametrize("name", list(TERMS))
def test_a2c_loss_terms_off_their_defaults(name, bs):
    import torch

    pol0, data, idx = _terms_case(name, bs)
    kw = dict(TERMS[name])
    _, grads, stats = _one_call(pol0, data, idx, **kw)
    _check_against_fp64("%s bs=%d" % (name, bs), pol0, data, idx, grads, stats, **kw)
    if name == "const_adv":  # A = 0 on every row: the policy half has no gradient at all, the loss is the value half
        for nm, gr in zip(P.NAMES, grads):
            if nm in P.PI_NAMES or nm == "log_std":
                assert torch.count_nonzero(gr).item() == 0, nm
        assert stats[0].item() == 0.0


@pytest.mark.parametrize("bs", [33, 16385])
@pytest.mark.parametrize("normalize", (False, True))
def test_a2c_reads_only_the_minibatch_rows_and_never_the_log_probs(bs, normalize):
    import torch

    pol0, *data = R.sweep_inputs(14, 3)
    idx = _minibatch(bs)
    keep = torch.zeros(N_ROWS, dtype=torch.bool, device=DEV)
    keep[idx] = True
    dirty = [torch.where(keep.view(-1, *[1] * (t.dim() - 1)), t, torch.full_like(t, float("nan"))) for t in data]
    assert all(int(torch.isnan(t).any(-1).sum() if t.dim() > 1 else torch.isnan(t).sum()) == N_ROWS - bs for t in dirty)
    kw = dict(normalize=normalize, ent_coef=0.01, max_grad_norm=0.5)
    (pa, ga, sa), (pb, gb, sb) = _one_call(pol0, data, idx, **kw), _one_call(pol0, dirty, idx, **kw)  # log_probs: NaN
    for a, b in zip(ga + list(pa.parameters()) + [sa], gb + list(pb.parameters()) + [sb]):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("kind", R.KINDS)
def test_a2c_optimizer_half_matches_float64(kind):
    """After each of 6 calls (a learning-rate change after 3; max_grad_norm 0.5, which bites under the
    returns' scale, then a loose 1e6, then none): parameters and optimizer state are the float64 step
    applied, from the fp32 state the call started from, to the gradients it left; those are the float64
    loss gradients times clip_grad_norm_'s coefficient; step counts the calls on all 13 tensors. Bars of
    test_gpu_bc.test_bc_optimizer_half_matches_float64_adam."""
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    pol0, *data = R.sweep_inputs(14, 3)
    second = "exp_avg_sq" if kind == "adam" else "square_avg"
    g = torch.Generator().manual_seed(9)
    pol = copy.deepcopy(pol0)
    tensors = _policy_tensors(pol)
    steps = {}
    opt = R.make_optimizer(kind, pol, 1e-3)
    from rl_rocket_amd.a2c import A2CUpdate

    ro = R.stub_rollout(14, 3, *data)
    for clip in (0.5, 1e6, None):  # one optimizer, three bindings of its state
        steps[clip] = A2CUpdate(pol, opt, ro, normalize_advantage=True, ent_coef=0.01, max_grad_norm=clip)
    bit = []
    for call, clip in enumerate((0.5, 0.5, 1e6, None, 0.5, None)):
        if call == 3:
            opt.param_groups[0]["lr"] = 2.5e-4
        lr = opt.param_groups[0]["lr"]
        idx = torch.randperm(N_ROWS, generator=g)[:1000 if call != 4 else 333].contiguous().cuda()
        before = copy.deepcopy(pol)
        state = dict(step=call)
        state[second] = [opt.state[t][second].double().clone() for t in tensors]
        if kind == "adam":
            state["exp_avg"] = [opt.state[t]["exp_avg"].double().clone() for t in tensors]
        steps[clip](idx)
        torch.cuda.synchronize()
        left = [t.grad.clone() for t in tensors]
        raw, _ = R.reference(before, *data, idx, torch.float64, normalize=True, ent_coef=0.01)
        coef = P.clip_coef64(raw, clip) if clip else 1.0
        bit.append(coef < 1.0)
        for name, a, r in zip(P.NAMES, left, raw):
            assert (a.double() - coef * r).abs().max().item() <= 1e-4 * coef * r.abs().max().item() + 1e-7, (call, name)
        p64 = [t.detach().double().clone() for t in _policy_tensors(before)]
        R.optimizer_ref(kind, p64, left, state, lr)
        assert state["step"] == call + 1
        for i, (name, t, p) in enumerate(zip(P.NAMES, tensors, p64)):
            st = opt.state[t]
            assert float(st["step"]) == call + 1, name
            assert (t.detach().double() - p).abs().max().item() <= 1e-6 * max(1.0, p.abs().max().item()), (call, name)
            assert torch.allclose(st[second].double(), state[second][i], rtol=1e-5, atol=1e-12), (call, name)
            if kind == "adam":
                assert torch.allclose(st["exp_avg"].double(), state["exp_avg"][i], rtol=1e-5, atol=1e-9), (call, name)
            if not bit[-1]:  # (under the clip a step can be below half an ulp of every element of a tensor)
                assert not torch.equal(t.detach(), _policy_tensors(before)[i]), name
    assert bit == [True, True, False, False, True, False]
    assert all(float(opt.state[t]["step"]) == 6.0 for t in tensors) and len(tensors) == 13
    if kind == "tf":  # the state began at ones: SB3's optimizer, not torch's
        fresh = R.make_optimizer("tf", copy.deepcopy(pol0), 1e-3)
        assert all(bool((fresh.init_state(p)["square_avg"] == 1).all()) for p in fresh.param_groups[0]["params"])


def _raw_call(step, idx, stats, ws=None):
    """rr_a2c_update through the C ABI with A2CUpdate's own arrays, on `ws` (a uint8 tensor) or its own."""
    import torch
    from rl_rocket_amd import _lib

    kind, lr, a, b2, eps = step._opt_args()
    _lib.check(step._lib.rr_a2c_update(step.ns, step.na, *step._ptrs, *[t.data_ptr() for t in step.data],
                                       idx.data_ptr(), idx.numel(), int(step.normalize), step.ent_coef, step.vf_coef,
                                       step.max_norm, kind, lr, a, b2, eps, None if stats is None else stats.data_ptr(),
                                       (step.ws if ws is None else ws).data_ptr(), step._nbytes,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "rr_a2c_update")


def _state(pol, opt):
    import torch
    from rl_rocket_amd.rollout import _policy_tensors

    torch.cuda.synchronize()
    out = []
    for t in _policy_tensors(pol):
        out += [t.detach().clone(), t.grad.clone()] + [v.clone() for _, v in sorted(opt.state[t].items())]
    return out


@pytest.mark.parametrize("kind", R.KINDS)
def test_a2c_same_call_twice_and_without_statistics_gives_the_same_bits(kind):
    import torch

    pol0, *data = R.sweep_inputs(14, 3)
    idx = _minibatch(40001)
    out = []
    for with_stats in (True, True, False):
        pol = copy.deepcopy(pol0)
        step, opt = _update(pol, data, kind, normalize_advantage=True, ent_coef=0.01)
        step.stats.fill_(-7.0)
        _raw_call(step, idx, step.stats if with_stats else None)
        out.append(_state(pol, opt) + [step.stats.clone()])
    a, b, c = out
    assert len(a) == 13 * (5 if kind == "adam" else 4) + 1
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(a[:-1], c[:-1]):
        assert torch.equal(x, y)
    assert bool((c[-1] == -7.0).all()) and not bool((a[-1] == -7.0).any())  # NULL: the block is not written


@pytest.mark.parametrize("bs,ns,na", [(33, 14, 3), (129, 14, 3), (33, 7, 2), (129, 7, 2)])
def test_a2c_workspace_carving_leaves_the_tail_and_reads_no_state(bs, ns, na):
    """The call on a workspace that is the first `bytes` of a larger buffer: the 256 floats after it keep
    their bit pattern, and parameters, gradients, optimizer state and statistics are bitwise those of the
    same call on a workspace pre-filled with 0xFF bytes (NaNs): the call reads no state from the workspace,
    and the host's sections lie inside the size rr_a2c_update_workspace_size returned for THIS batch."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.a2c import A2CUpdate

    pol0, *data = R.sweep_inputs(ns, na)
    rows = [_minibatch(bs), _minibatch(bs + 1)[1:].contiguous()]
    tail = (0x5A5A0000 + torch.arange(256, dtype=torch.int32)).to(DEV)
    small = [t[:bs].contiguous() for t in data]  # a rollout of bs rows sizes the workspace for bs
    out = []
    for fill in (0x00, 0xFF):
        pol = copy.deepcopy(pol0)
        opt = R.make_optimizer("tf", pol, 1e-3)
        s = A2CUpdate(pol, opt, R.stub_rollout(ns, na, *small), normalize_advantage=True, ent_coef=0.01)
        s.data = list(data)  # the call's rows come from the whole pool; bs rows of it per call
        need = ctypes.c_int64()
        assert s._lib.rr_a2c_update_workspace_size(ns, na, bs, ctypes.byref(need)) == _lib.RR_OK
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
    assert len(a) == len(b) == 4 * 13 + 2
    for x, y in zip(a, b):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def _env(model, n=256, seed=77):
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF

    return RocketBatch(n, model=model, device=DEV, max_episode_steps=30, **dict(ENV_CONFIG_6DOF if model == 6 else {},
                                                                                seed=seed))


def _policy(env, seed=3):
    import torch
    from rl_rocket_amd.rollout import MlpActorCritic

    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return MlpActorCritic(env.state_dim, env.action_dim).to(DEV)


def test_a2c_update_fused_tracks_autograd_on_a_real_batch():
    """5 iterations of collect + a2c_update on two 6DOF batches of 256 envs from equal starts (n_steps 5,
    gae_lambda 1: SB3's A2C defaults), fused against fused=False: parameters within 5 % of how far training
    moved them (the bar of test_gpu_bc.test_bc_train_tracks_autograd)."""
    import torch
    from rl_rocket_amd.a2c import RMSpropTFLike, a2c_update
    from rl_rocket_amd.rollout import DeviceRollout

    runs = []
    for fused in (False, True):
        env = _env(6)
        pol = _policy(env)
        pol0 = copy.deepcopy(pol)
        opt = RMSpropTFLike(pol.parameters(), lr=7e-4)
        ro = DeviceRollout(env, pol, n_steps=5, gae_lambda=1.0, seed=5)
        for _ in range(5):
            ro.collect()
            st = a2c_update(pol, opt, ro, ent_coef=0.01, fused=fused)
            assert set(st) == set(R.STATS) and all(v == v for v in st.values())
        torch.cuda.synchronize()
        assert float(opt.state[pol.log_std]["step"]) == 5.0
        runs.append((pol, st))
        env.close()
    (pa, sa), (pb, sb) = runs
    moved = max((x - y).abs().max().item() for x, y in zip(pol0.parameters(), pa.parameters()))
    drift = max((x - y).abs().max().item() for x, y in zip(pa.parameters(), pb.parameters()))
    print("moved %.3e, parameter drift %.3e" % (moved, drift), sa, sb)
    assert moved > 0.0 and drift <= 0.05 * moved, (drift, moved)
    for k in sa:
        assert abs(sa[k] - sb[k]) <= 0.02 * max(1.0, abs(sa[k])), (k, sa[k], sb[k])


@pytest.mark.parametrize("model,prec,kind", [(3, "fp32", "tf"), (6, "fp32", "tf"), (6, "bf16", "rmsprop"),
                                             (6, "fp16x3", "adam")])
def test_graphed_a2c_replays_are_the_eager_iterations(model, prec, kind):
    """Four GraphedA2C.step() replays leave bitwise what four eager collect(); update() iterations from the
    same seed leave: parameters, gradients, optimizer state, ro.iter, the rollout's last buffers and the env
    (its checkpoint). A bf16 and an fp16x3 rollout go through the same call: the learner is fp32."""
    import torch
    from rl_rocket_amd.a2c import A2CUpdate, GraphedA2C
    from rl_rocket_amd.rollout import DeviceRollout

    out = []
    for graphed in (False, True):
        env = _env(model)
        pol = _policy(env)
        opt = R.make_optimizer(kind, pol, 7e-4)
        ro = DeviceRollout(env, pol, n_steps=5, gae_lambda=1.0, seed=5, policy_dtype=prec)
        kw = dict(normalize_advantage=model == 3, ent_coef=0.01)
        if graphed:
            it = GraphedA2C(pol, opt, ro, **kw)
            assert it.update.n_updates == 0 and int(ro.iter) == 0
            for k in range(4):
                if k == 2:
                    opt.param_groups[0]["lr"] = 3e-4  # read from the device scalar: no new capture
                stats = it.step().clone()
            assert it.train_stats()["train/n_updates"] == 4
        else:
            upd = A2CUpdate(pol, opt, ro, **kw)
            for k in range(4):
                if k == 2:
                    opt.param_groups[0]["lr"] = 3e-4
                ro.collect()
                stats = upd().clone()
            ts = upd.train_stats()
            assert set(ts) == {"train/policy_loss", "train/value_loss", "train/entropy_loss", "train/std",
                               "train/n_updates"} and ts["train/n_updates"] == 4
            assert ts["train/entropy_loss"] == -stats[2].item() and ts["train/std"] > 0.0
        torch.cuda.synchronize()
        ck = env.checkpoint()
        out.append(_state(pol, opt) + [stats, ro.iter.clone(), ro.last_value.clone(), ro.advantages.clone(),
                                       ro.returns.clone(), ro.obs.clone(), env.obs.clone(), env.done.clone()]
                   + [ck[k].clone() for k in sorted(ck)])
        env.close()
    a, b = out
    assert len(a) == len(b) and int(a[13 * (5 if kind == "adam" else 4) + 1]) == 4
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), k
    assert all(bool(torch.isfinite(x).all()) for x in a[:13 * 4])
