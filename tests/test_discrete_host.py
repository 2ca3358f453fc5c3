"""The Categorical policy of the discrete 3DOF actions, without a GPU: the module against
torch.distributions.Categorical in float64, the uniform draw's restatement, the compat wrapper on a stub
env, what is refused before anything touches a device, the C ABI's refusals (test_capi.py's fake-pointer
pattern), and the knife-edge share of the act kernel's GPU cases (tests/discrete_ref.py)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

import discrete_ref as D
from rl_rocket_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [2, 3, 4])
def test_module_matches_torch_categorical_in_float64(k):
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic, _policy_tensors

    pol = MlpCategoricalActorCritic(7, k, D.TABLES[k]).double()
    g = torch.Generator().manual_seed(k)
    logits = 3.0 * torch.randn((257, k), generator=g, dtype=torch.float64)
    logits[0] = torch.tensor([80.0, 0.0, -80.0, 0.0], dtype=torch.float64)[:k]
    acts = torch.randint(0, k, (257,), generator=g)
    ref = torch.distributions.Categorical(logits=logits)
    lp, ent = pol.log_prob(logits, acts.double()[:, None]), pol.entropy(logits)
    assert torch.isfinite(lp).all() and torch.isfinite(ent).all()
    assert torch.isfinite(pol.log_prob(logits[:1].expand(k, k), torch.arange(k))).all()  # every choice of the +-80 row
    assert (lp - ref.log_prob(acts)).abs().max() <= 1e-13
    assert (ent - ref.entropy()).abs().max() <= 1e-13
    assert 0.0 <= float(ent[0]) < 1e-30  # p = (1, e^-80, ..): the entropy is ~80 e^-80
    assert torch.equal(pol.mode(logits), ref.probs.argmax(-1))
    assert torch.equal(pol.continuous(acts), torch.tensor(D.TABLES[k], dtype=torch.float32)[acts])
    ts = _policy_tensors(pol)
    assert len(ts) == 12 and ts[8].shape == (k, 64) and ts[9].shape == (k,) and not hasattr(pol, "log_std")
    x = torch.randn((5, 7), generator=g, dtype=torch.float64)
    logits2, value = pol(x)
    assert logits2.shape == (5, k) and value.shape == (5,) and torch.equal(value, pol.value(x))


def test_fp32_row_with_an_underflowing_probability_stays_finite():
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic

    pol = MlpCategoricalActorCritic(7, 4)
    logits = torch.tensor([[120.0, 0.0, -120.0, 0.0]])
    assert float(torch.softmax(logits, -1)[0, 2]) == 0.0  # underflows in fp32
    lp = pol.log_prob(logits.expand(4, 4), torch.arange(4))
    assert torch.isfinite(lp).all() and float(lp[2]) == -240.0
    assert float(pol.entropy(logits)) == 0.0


def test_ppo_loss_is_unchanged_for_the_gaussian_policy():
    """_ppo_loss on an MlpActorCritic: bitwise the loss of the expression it had before the Categorical
    branch (restated here)."""
    import ppo_ref as P
    from rl_rocket_amd.learner import _ppo_loss

    pol, ro, g = P.setup_cpu(7, 2, 300, seed=4)
    n = 300
    idx = torch.randperm(n, generator=g)[:100]
    obs, act = ro.obs.reshape(n, -1)[idx], ro.actions.reshape(n, -1)[idx]
    old, adv, ret = ro.log_probs.reshape(n)[idx], ro.advantages.reshape(n)[idx], ro.returns.reshape(n)[idx]
    loss, stats, lp, ratio = _ppo_loss(pol, obs, act, old, adv, ret, None, 100, 0.2, 0.01, 0.5, 0.0, True)
    mean, value = pol(obs)
    lp0 = pol.log_prob(mean, act)
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    r0 = torch.exp(lp0 - old)
    pg = -torch.min(a * r0, a * torch.clamp(r0, 1 - 0.2, 1 + 0.2)).mean()
    vf = torch.nn.functional.mse_loss(ret, value)
    ent = -pol.entropy(100).mean()
    assert torch.equal(loss, pg + 0.01 * ent + 0.5 * vf) and torch.equal(ratio, r0)
    assert float(stats["entropy"]) == float(-ent.detach())


def test_ppo_loss_takes_the_entropy_from_the_logits():
    from rl_rocket_amd.learner import _ppo_loss

    pol, ro, g = D.learner_inputs(3, n=200, seed=2)
    idx = torch.arange(200)
    loss, stats, _, _ = _ppo_loss(pol, ro.obs.reshape(200, 7), ro.actions.reshape(200, 1), ro.log_probs.reshape(200),
                                  ro.advantages.reshape(200), ro.returns.reshape(200), None, 200, 0.2, 0.01, 0.5, 0.0, True)
    _, ref = D.loss_reference(pol, ro, idx, torch.float32)
    assert abs(float(stats["entropy"]) - ref[2]) <= 1e-6 and abs(float(stats["policy_loss"]) - ref[0]) <= 1e-6
    assert 0.0 < ref[2] < np.log(3.0)


def test_uniform_ref_is_uniform_and_shards():
    n = 65536
    u = D.uniform_ref(n, 0, D.ACT_SEED, D.ACT_ITER, D.ACT_T)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) <= 5.0 * np.sqrt(1.0 / 12.0 / n)
    counts = np.histogram(u, bins=16, range=(0.0, 1.0))[0]
    assert counts.sum() == n
    assert np.abs(counts - n / 16.0).max() <= 5.0 * np.sqrt(n * (1.0 / 16.0) * (15.0 / 16.0))
    assert np.array_equal(D.uniform_ref(300, 1000, D.ACT_SEED, D.ACT_ITER, D.ACT_T), u[1000:1300])
    assert not np.array_equal(D.uniform_ref(300, 0, D.ACT_SEED, D.ACT_ITER, D.ACT_T + 1), u[:300])


def test_act_cases_stay_under_the_knife_edge_cap():
    """The GPU test asserts that at most 1 % of rows are knife-edge; the share depends on the float64
    reference alone (expected 3 x 2e-4), so it is known here for the seeds discrete_ref chose."""
    for k in D.ACT_CHOICES:
        for n in D.ACT_SIZES:
            pol, obs, u = D.act_case(n, k)
            _, _, lp = D.forward64(pol, obs)
            idx, knife, _ = D.act_ref(lp, u)
            assert knife.mean() <= D.KNIFE_CAP, (k, n, knife.sum())
            assert idx.min() >= 0 and idx.max() <= k - 1
        p = np.exp(lp)  # the largest case: the probabilities spread, every choice is drawn
        assert p.max(1).mean() < 0.9 and len(set(idx.tolist())) == k


class _StubEnv:
    def __init__(self):
        self.action_space, self.observation_space, self.got = "box", "obs", []

    def step(self, action):
        self.got.append(np.asarray(action))
        return "obs", 1.5, False, {}

    def reset(self, **kw):
        return "obs0"


def test_compat_wrapper_on_a_stub_env():
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        from my_environment.wrappers import DiscreteActions3DOF
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    env = _StubEnv()
    w = DiscreteActions3DOF(env)
    assert w.action_space.n == 4 and w.disc_to_cont == [[0, -1], [-1, 1], [0, 1], [1, 1]]
    assert w.step(3) == ("obs", 1.5, False, {}) and np.array_equal(env.got[-1], [1, 1])
    assert np.array_equal(w.action(0), [0, -1]) and w.reset() == "obs0"
    w3 = DiscreteActions3DOF(env, [[0.0, -1.0], [-0.5, 0.25], [0.75, 1.0]])
    assert w3.action_space.n == 3
    w3.step(np.int64(1))
    assert np.array_equal(env.got[-1], [-0.5, 0.25])
    with pytest.raises(NotImplementedError, match="pygame"):
        w.get_keys_to_action()


def _stub_batch(dof=3):
    ns, na = (7, 2) if dof == 3 else (14, 3)
    return types.SimpleNamespace(num_envs=8, state_dim=ns, action_dim=na, device="cpu", model=dof)


def test_refusals_come_before_anything_touches_a_device():
    from rl_rocket_amd.rollout import (DeviceRollout, GraphedPPOUpdate, MlpCategoricalActorCritic, PolicyEvaluator,
                                       ppo_update)

    pol = MlpCategoricalActorCritic(7, 4)
    for kw, word in ((dict(one_launch=True), "one_launch=True"), (dict(per_step=True), "per_step=True"),
                     (dict(stats=True), "stats=True"), (dict(policy_dtype="bf16"), "policy_dtype='bf16'"),
                     (dict(policy_dtype="fp16x3"), "policy_dtype='fp16x3'")):
        with pytest.raises(ValueError, match=word):
            DeviceRollout(_stub_batch(), pol, **kw)
    with pytest.raises(ValueError, match="6DOF"):
        DeviceRollout(_stub_batch(6), pol)
    with pytest.raises(ValueError, match="2 .. 4"):
        DeviceRollout(_stub_batch(), MlpCategoricalActorCritic(7, 5, [[0.0, 0.0]] * 5), fused=True)
    with pytest.raises(ValueError, match="finite"):
        MlpCategoricalActorCritic(7, 2, [[0.0, float("nan")], [0.0, 1.0]])
    with pytest.raises(ValueError, match="fused=True"):
        PolicyEvaluator(_stub_batch(), pol, fused=True)
    with pytest.raises(ValueError, match="record="):
        PolicyEvaluator(_stub_batch(), pol, record=[0])
    ro = types.SimpleNamespace(n_steps=1, env=_stub_batch())
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    for kw, word in ((dict(clip_range_vf=0.2), "clip_range_vf"), (dict(normalize_advantage=False), "normalize_advantage"),
                     (dict(target_kl=0.01), "target_kl"), (dict(group=object()), "group=")):
        with pytest.raises(ValueError, match=word):
            ppo_update(pol, opt, ro, fused=True, **kw)
    with pytest.raises(ValueError, match="another optimizer"):  # not a capturable Adam on the device
        ppo_update(pol, opt, ro, fused=True)
    cap = types.SimpleNamespace(param_groups=[dict(capturable=True)])
    for kw, word in ((dict(train_stats=True), "train_stats"), (dict(target_kl=0.01), "target_kl")):
        with pytest.raises(ValueError, match=word):
            GraphedPPOUpdate(pol, cap, ro, batch_size=8, fused=True, **kw)


def _ptrs(k, null_at=None):
    arr = (ctypes.c_void_p * k)(*[0x10000 + 0x1000 * i for i in range(k)])
    if null_at is not None:
        arr[null_at] = None
    return arr


def test_c_abi_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    E, V = _lib.RR_EINVAL, ctypes.c_void_p
    fake, lr = V(0x10000), V(0x20000)

    def refused(rc, name, word=None):
        assert rc == E, (name, rc)
        msg = lib.rr_last_error()
        assert name.encode() in msg and (word is None or word.encode() in msg), (name, msg)

    off = (ctypes.c_int64 * 12)()
    size = lib.rr_policy_layout_discrete(7, off)
    assert size > 0 and size % 4 == 0 and off[7] - 2 * off[4] == 0 and off[8] - off[7] == 4 * 64  # HA = 2 TOWER, 4 heads
    refused(lib.rr_policy_layout_discrete(14, None), "rr_policy_layout_discrete")
    refused(lib.rr_policy_pack_discrete(7, 4, None, fake, None), "rr_policy_pack_discrete")
    refused(lib.rr_policy_pack_discrete(7, 4, _ptrs(12, null_at=9), fake, None), "rr_policy_pack_discrete")
    refused(lib.rr_policy_pack_discrete(7, 5, _ptrs(12), fake, None), "rr_policy_pack_discrete", "n_choices")
    refused(lib.rr_policy_bootstrap(fake, 7, 4, _lib.RR_POLICY_BF16, 64, None, None, None, 0.99, None, fake, fake, None),
            "rr_policy_bootstrap", "RR_POLICY_FP32")

    table = (ctypes.c_float * 8)(0, -1, -1, 1, 0, 1, 1, 1)

    def act(obs_dim=7, k=4, tab=table, prec=0, n=64, params=fake, reward_out=None, start_out=None):
        return lib.rr_policy_act_discrete(params, obs_dim, k, tab, prec, n, 0, fake, 1, fake, 0, fake, fake, fake, fake,
                                          None, None, None, None, 0.99, reward_out, None, start_out, None)

    who = "rr_policy_act_discrete"
    refused(act(obs_dim=14), who, "obs_dim")
    refused(act(k=1), who, "n_choices")
    refused(act(k=5), who, "n_choices")
    refused(act(prec=_lib.RR_POLICY_BF16), who, "RR_POLICY_FP32")
    refused(act(prec=_lib.RR_POLICY_FP16X3), who, "RR_POLICY_FP32")
    refused(act(tab=None), who)
    refused(act(n=0), who)
    refused(act(params=V(0x10004)), who, "aligned")
    refused(act(reward_out=fake), who, "reward_out")
    refused(act(start_out=fake), who, "start_out")
    for bad in (float("nan"), float("inf")):
        t = (ctypes.c_float * 8)(0, -1, -1, 1, 0, bad, 1, 1)
        refused(act(tab=t), who, "finite")
        refused(act(k=3, tab=t), who, "finite")
    t = (ctypes.c_float * 8)(0, -1, -1, 1, 0, 1, float("nan"), 1)  # a row past n_choices is not read
    refused(act(k=3, tab=t, n=0), who, "n <= 0")

    nbytes = ctypes.c_int64()
    sz = "rr_ppo_update_discrete_workspace_size"
    refused(lib.rr_ppo_update_discrete_workspace_size(14, 4, 64, ctypes.byref(nbytes)), sz, "obs_dim")
    refused(lib.rr_ppo_update_discrete_workspace_size(7, 5, 64, ctypes.byref(nbytes)), sz, "n_choices")
    refused(lib.rr_ppo_update_discrete_workspace_size(7, 1, 64, ctypes.byref(nbytes)), sz, "n_choices")
    refused(lib.rr_ppo_update_discrete_workspace_size(7, 4, 1, ctypes.byref(nbytes)), sz, "batch")
    refused(lib.rr_ppo_update_discrete_workspace_size(7, 4, 64, None), sz)
    assert lib.rr_ppo_update_discrete_workspace_size(7, 3, 64, ctypes.byref(nbytes)) == 0 and nbytes.value % 16 == 0
    small = nbytes.value
    assert lib.rr_ppo_update_discrete_workspace_size(7, 3, 65536, ctypes.byref(nbytes)) == 0 and nbytes.value > small

    def update(shape=(7, 4), lists=None, batch=64, nxt=None, next_batch=0, clip=0.2, flags=0, wsp=fake, ws_bytes=1 << 30,
               data=fake):
        lists = lists or [_ptrs(12)] * 5
        return lib.rr_ppo_update_discrete(*shape, *lists, data, fake, fake, fake, fake, fake, batch, nxt, next_batch,
                                          clip, 0.01, 0.5, 0.5, lr, 0.9, 0.999, 1e-5, None, flags, wsp, ws_bytes, None)

    who = "rr_ppo_update_discrete"
    refused(update(shape=(14, 4)), who, "obs_dim")
    refused(update(shape=(7, 5)), who, "n_choices")
    refused(update(batch=1), who, "batch")
    refused(update(data=None), who, "null")
    refused(update(lists=[_ptrs(12)] * 2 + [_ptrs(12, null_at=11)] + [_ptrs(12)] * 2), who, "tensor")
    refused(update(ws_bytes=small - 16, batch=64, shape=(7, 3)), who, "workspace")
    refused(update(wsp=V(0x10008)), who, "aligned")
    refused(update(flags=0x2), who, "flag")
    refused(update(clip=-0.1), who, "clip_range")
    refused(update(nxt=fake, next_batch=65), who, "next_batch")
    refused(update(nxt=fake, next_batch=1), who, "next_batch")


# rr_ppo_update_discrete_workspace_size's bytes, read from the build in which it had size functions of its own:
# one row either side of a tile (64 / 65) and either side of the first batch with 128 workgroups (16 257). The
# <7, 4> image is sized whatever n_choices is.
_WS_BATCHES = (2, 64, 65, 16256, 16257, 16258)
_WS_BYTES = (131360, 131360, 131360, 6659168, 6710976, 6710976)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_workspace_size_is_the_one_before_the_shared_shape_record(k):
    lib = _lib.load()
    ws = ctypes.c_int64()
    got = []
    for batch in _WS_BATCHES:
        assert lib.rr_ppo_update_discrete_workspace_size(7, k, batch, ctypes.byref(ws)) == 0, (k, batch)
        got.append(ws.value)
    assert tuple(got) == _WS_BYTES, (k, got)


# sha256[:16] over (key, bytes) of every state_dict entry in order, and the global generator's next draw, of the
# policy classes as they were before they shared a base (seed, class, arguments)
_INIT = {
    (0, "MlpActorCritic", (14, 3)): ("ea58bb50846b9a93", 0.6514866352081299),
    (0, "MlpActorCritic", (7, 2)): ("75b369ceab8e3071", 0.5089229941368103),
    (0, "MlpCategoricalActorCritic", (7, 2)): ("b96ba1da2637977d", 0.5089229941368103),
    (0, "MlpCategoricalActorCritic", (7, 3)): ("9b3e2f38197d14be", 0.5294811129570007),
    (0, "MlpCategoricalActorCritic", (7, 4)): ("519aee89807598e0", 0.887469470500946),
    (7, "MlpActorCritic", (14, 3)): ("0099244a820a3ccc", 0.1816447377204895),
    (7, "MlpActorCritic", (7, 2)): ("392c9f5435f817cc", 0.1446022391319275),
    (7, "MlpCategoricalActorCritic", (7, 2)): ("352e2db7795b165d", 0.1446022391319275),
    (7, "MlpCategoricalActorCritic", (7, 3)): ("0652bf770afb4387", 0.7231861352920532),
    (7, "MlpCategoricalActorCritic", (7, 4)): ("ce7811a7c3364d2b", 0.9301236271858215),
}
_NETS = ["pi_net.0.weight", "pi_net.0.bias", "pi_net.2.weight", "pi_net.2.bias", "vf_net.0.weight", "vf_net.0.bias",
         "vf_net.2.weight", "vf_net.2.bias", "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"]


def test_both_policies_initialise_as_before_they_shared_a_base():
    import hashlib

    from rl_rocket_amd import rollout

    for (seed, cls, args), (digest, draw) in _INIT.items():
        torch.manual_seed(seed)
        if cls == "MlpCategoricalActorCritic":
            pol = rollout.MlpCategoricalActorCritic(*args, D.TABLES[args[1]])
        else:
            pol = rollout.MlpActorCritic(*args)
        after = float(torch.rand(()))
        sd = pol.state_dict()
        h = hashlib.sha256()
        for key, v in sd.items():
            h.update(key.encode())
            h.update(v.numpy().tobytes())
        assert h.hexdigest()[:16] == digest and after == draw, (seed, cls, args, h.hexdigest()[:16], after)
        gauss = cls == "MlpActorCritic"
        assert list(sd) == (["log_std"] if gauss else ["table"]) + _NETS
        named = dict(pol.named_parameters())
        assert list(named) == (["log_std"] if gauss else []) + _NETS
        ts = rollout._policy_tensors(pol)
        assert len(ts) == (13 if gauss else 12)
        assert all(t is named[n] for t, n in zip(ts, _NETS + ["log_std"]))
