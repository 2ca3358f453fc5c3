"""rr_bc_update's host side (no GPU): the C declarations and their ctypes mirrors, the refusals that
come before any HIP call, the translation unit of its own and its kernels' descriptors, the float64
reference of the GPU tests (bc_ref) against a closed form, the compat kick-starter's flattening of
trajectories, Demonstrations.from_trace on a hand-built EvalTrace, and the Python refusals."""
import copy
import ctypes
import json
import math
import os
import re
import struct
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bc_host_common as C
import bc_ref as R
import ppo_ref as P
from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compat():
    path = os.path.join(ROOT, "compat")
    if path not in sys.path:
        sys.path.insert(0, path)
    from my_environment.utils import imitation_kickstarter

    return imitation_kickstarter


def test_header_declares_the_entry_points_and_signatures_mirror_them():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14  # a pure addition
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    new = re.search(r"int\s+rr_bc_update\s*\(([^;]*)\)\s*;", code)
    args = [" ".join(a.split()) for a in new.group(1).split(",")]
    assert args == ["int obs_dim", "int act_dim", "float* const* params", "float* const* grads",
                    "float* const* exp_avg", "float* const* exp_avg_sq", "float* const* step", "const float* obs",
                    "const float* actions", "const int64_t* idx", "int64_t batch", "float ent_weight",
                    "float l2_weight", "const float* lr", "double beta1", "double beta2", "float eps", "float* stats",
                    "uint32_t flags", "void* workspace", "int64_t workspace_bytes", "void* stream"]
    res, argtypes = _lib.SIGNATURES["rr_bc_update"]
    assert res is ctypes.c_int and len(argtypes) == len(args)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
             "uint32_t": ctypes.c_uint32}
    for a, t in zip(args, argtypes):
        assert t is (ctypes.c_void_p if "*" in a else kinds[a.split()[0]]), a
    assert _lib.SIGNATURES["rr_bc_update_workspace_size"] == _lib.SIGNATURES["rr_ppo_update_workspace_size"]
    assert re.search(r"int\s+rr_bc_update_workspace_size\s*\(\s*int obs_dim,\s*int act_dim,\s*int64_t batch,\s*"
                     r"int64_t\* bytes\)\s*;", code)
    enum = re.findall(r"\b(RR_BC_STAT_[A-Z0-9_]+)\b", code[code.index("RR_BC_STAT_NEGLOGP = 0"):code.index("RR_BC_STAT_SLOTS")])
    assert enum == ["RR_BC_STAT_" + s.upper() for s in R.STATS] and [getattr(_lib, k) for k in enum] == list(range(7))
    assert re.search(r"RR_BC_STAT_SLOTS\s*=\s*8\b", code) and _lib.RR_BC_STAT_SLOTS == 8
    assert re.search(r"#define\s+RR_BC_CHAINED\s+0x1u", code) and _lib.RR_BC_CHAINED == 1
    from rl_rocket_amd import bc

    assert bc.STAT_NAMES == R.STATS


def test_library_exports_the_symbols_and_keeps_the_launcher_hidden():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("rr_bc_update", "rr_bc_update_workspace_size"):
        assert re.search(r"\bT %s\b" % name, out)
    assert not re.search(r"rrc_launch_bc", out)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for ns, na in ((14, 3), (7, 2)):
        sizes = []
        for bs in (2, 128, 129, 16384, 16385, 65536):
            assert lib.rr_bc_update_workspace_size(ns, na, bs, ctypes.byref(a)) == _lib.RR_OK
            assert a.value % 16 == 0
            sizes.append(a.value)
        # one partial-gradient vector per workgroup, one workgroup per 128 rows up to 128 of them
        assert sizes[0] == sizes[1] < sizes[2] < sizes[3] == sizes[4] == sizes[5]
        assert sizes[3] - sizes[0] == 127 * (sizes[2] - sizes[1])
        # one tower's partial vectors: less than the PPO call's two
        assert lib.rr_ppo_update_workspace_size(ns, na, 65536, ctypes.byref(b)) == _lib.RR_OK and sizes[5] < b.value
    for bad in ((5, 2, 64), (14, 2, 64), (14, 3, 1), (14, 3, 0)):
        assert lib.rr_bc_update_workspace_size(*bad, ctypes.byref(b)) == _lib.RR_EINVAL
        assert lib.rr_last_error().startswith(b"rr_bc_update_workspace_size: ")
    assert lib.rr_bc_update_workspace_size(14, 3, 64, None) == _lib.RR_EINVAL


def test_refuses_bad_arguments_before_any_hip_call():
    """Never-read fake device addresses and a NULL stream: every refusal returns before a launch, with the
    text it had before the two calls shared their host path."""
    C.check_refusals("rr_bc_update", (14, 3), 13, [((5, 2), C.GAUSS_SHAPE), ((14, 2), C.GAUSS_SHAPE),
                                                     ((7, 3), C.GAUSS_SHAPE), ((7, 4), C.GAUSS_SHAPE)])
    # rr_ppo_update keeps its own prefix
    lib = _lib.load()
    V = ctypes.c_void_p
    fake, p = (V * 13)(*[0x100000 + 0x1000 * k for k in range(13)]), V(0x70000)
    assert lib.rr_ppo_update(14, 3, fake, fake, fake, fake, fake, p, p, p, p, p, p, 4096, None, 0, 0.2, 0.01, 0.5, 0.5, p,
                             0.9, 0.999, 1e-5, p, 0x2, V(0x200000), 1 << 30, None) == _lib.RR_EINVAL
    assert lib.rr_last_error() == b"rr_ppo_update: unknown flag bits"


def test_workspace_sizes_are_the_ones_before_the_fold():
    C.check_workspace_sizes("rr_bc_update")


def test_build_compiles_the_translation_unit_of_its_own():
    C.check_unit(B.SRC_BC, "bc", B.SRC_PPO_OPTS, 0)


def test_new_kernels_use_no_scratch_and_the_learner_kernels_are_all_there():
    """From the built library: the new instantiations use no scratch (private_segment_fixed_size,
    bytes 4..8 of the kernel descriptor) and the learner's own kernels are still beside them."""
    kd = C.kernel_descriptors()
    new = {n: v for n, v in kd.items() if "bc_" in n and "_kernel" in n}
    for name in ("bc_pack_kernel", "bc_grad_kernel", "bc_finish_kernel", "bc_adam_kernel"):  # two shapes of each
        assert sum(name + "IL" in n for n in new) == 2, name
    assert len(new) == 8
    for n, v in new.items():
        assert struct.unpack_from("<I", v, 4)[0] == 0, n
    for name in ("ppo_prep_kernel", "ppo_grad_kernel", "ppo_finish_kernel", "adam_chain_kernel"):
        assert sum(name + "IL" in n for n in kd) == 2, name


def test_committed_isa_comparison_covers_every_kernel_of_the_parent():
    with open(os.path.join(ROOT, "profiles", "bc", "isa_before_after.json")) as f:
        rec = json.load(f)
    assert rec["kernels_in_parent"] == len(rec["before"]) >= 160
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert sorted(rec["added"]) == sorted(k for k in rec["after"] if k not in rec["before"])
    assert len(rec["added"]) == 8 and all("::bc_" in k for k in rec["added"])


def test_committed_isa_comparison_of_the_fold_covers_every_kernel_of_the_parent():
    """profiles/bc_fold: the two units on one kernel text against the build before it, no kernel renamed. The
    parent's kernels are the ones its own record (profiles/bc_discrete, `after`) lists: all 179, each with
    the hash it had there."""
    with open(os.path.join(ROOT, "profiles", "bc_fold", "isa_before_after.json")) as f:
        rec = json.load(f)
    with open(os.path.join(ROOT, "profiles", "bc_discrete", "isa_before_after.json")) as f:
        parent = json.load(f)["after"]
    assert rec["kernels_A"] == rec["kernels_B"] == len(rec["hashes"]) == len(parent) == 179
    assert rec["only in A"] == rec["only in B"] == rec["hash differs"] == [] and rec["renamed"] == {}
    assert rec["hashes"] == parent
    assert sum("::bc_" in k for k in parent) == 8 and sum("::bcd_" in k for k in parent) == 4


def test_bc_ref_against_a_closed_form():
    """Two samples, one action dimension, mean = w x: every figure and gradient written out by hand."""
    w, s, v = 0.7, -0.3, 1.9  # the 'policy' weight, log_std, and a parameter the mean does not use
    x, a = (0.5, -1.25), (1.0, 0.2)
    ew, l2w = 0.05, 0.3
    t = [torch.tensor([z], dtype=torch.float64, requires_grad=True) for z in (w, s, v)]
    mean = t[0] * torch.tensor(x, dtype=torch.float64)[:, None]
    loss, figures = R.loss_terms(mean, t[1], torch.tensor(a, dtype=torch.float64)[:, None], t, ew, l2w)
    gw, gs, gv = [g.item() for g in torch.autograd.grad(loss, t)]
    var = math.exp(2 * s)
    d = [ai - w * xi for ai, xi in zip(a, x)]
    logp = [-di * di / (2 * var) - s - 0.5 * math.log(2 * math.pi) for di in d]
    neglogp = -(logp[0] + logp[1]) / 2
    entropy = 0.5 + 0.5 * math.log(2 * math.pi) + s
    l2_norm = 0.5 * (w * w + s * s + v * v)
    want = (neglogp, entropy, -ew * entropy, (math.exp(logp[0]) + math.exp(logp[1])) / 2, l2_norm, l2w * l2_norm,
            neglogp - ew * entropy + l2w * l2_norm)
    assert len(figures) == len(R.STATS) == 7
    for name, got, ref in zip(R.STATS, figures, want):
        assert got.item() == pytest.approx(ref, rel=1e-13, abs=1e-15), name
    # d neglogp / d w = -mean_i d_i x_i / var; d neglogp / d log_std = 1 - mean_i d_i^2 / var
    assert gw == pytest.approx(-(d[0] * x[0] + d[1] * x[1]) / (2 * var) + l2w * w, rel=1e-13)
    assert gs == pytest.approx(1.0 - (d[0] ** 2 + d[1] ** 2) / (2 * var) - ew + l2w * s, rel=1e-13)
    assert gv == pytest.approx(l2w * v, rel=1e-13)


def test_bc_ref_reference_on_a_policy():
    """`reference` on an MlpActorCritic: 13 gradients in rr_ppo_grad's order, the value half exactly
    l2_weight w (zeros without it), and the package's own autograd loss gives the same figures."""
    from rl_rocket_amd.bc import _bc_loss
    from rl_rocket_amd.rollout import _policy_tensors

    pol, ro, g = P.setup_cpu(7, 2, 50, seed=3)
    obs, acts = ro.obs.reshape(50, 7), ro.actions.reshape(50, 2)
    idx = torch.randperm(50, generator=g)[:20]
    g0, st0 = R.reference(pol, obs, acts, idx)
    g1, st1 = R.reference(pol, obs, acts, idx, ent_weight=0.1, l2_weight=0.01)
    assert len(g0) == len(g1) == 13 and len(st0) == 7
    for name, a, b, w in zip(P.NAMES, g0, g1, _policy_tensors(pol)):
        assert a.shape == w.shape and a.dtype == torch.float64
        if name in P.VF_NAMES:
            assert torch.count_nonzero(a).item() == 0 and torch.equal(b, 0.01 * w.detach().double())
        elif name == "log_std":
            assert torch.allclose(b - a, -0.099 + 0.01 * w.detach().double(), rtol=0, atol=1e-15)
        else:
            assert torch.allclose(b - a, 0.01 * w.detach().double(), rtol=0, atol=1e-15) and a.abs().max() > 0
    assert st0[0] == st1[0] and st1[2] == pytest.approx(-0.1 * st1[1]) and st1[5] == pytest.approx(0.01 * st1[4])
    p64 = copy.deepcopy(pol).double()
    _, figures = _bc_loss(p64, obs[idx].double(), acts[idx].double(), 0.1, 0.01)
    for a, b in zip(figures, st1):
        assert float(a.detach()) == pytest.approx(b, rel=1e-12)


def test_kickstarter_flattens_trajectories_in_order_without_the_last_observation():
    K = _compat()
    rng = np.random.default_rng(0)
    lens = (3, 1, 5)
    tuples = [(rng.normal(size=(L + 1, 7)), rng.normal(size=(L, 2)), [{}] * L, True) for L in lens]
    objs = [types.SimpleNamespace(obs=t[0], acts=t[1], infos=None, terminal=True) for t in tuples]
    for trajs in (tuples, objs, [tuples[0], objs[1], tuples[2]]):
        obs, acts = K.flatten_trajectories(trajs)
        assert obs.shape == (9, 7) and acts.shape == (9, 2) and obs.dtype == acts.dtype == np.float32
        np.testing.assert_array_equal(obs, np.concatenate([t[0][:-1] for t in tuples]).astype(np.float32))
        np.testing.assert_array_equal(acts, np.concatenate([t[1] for t in tuples]).astype(np.float32))
    with pytest.raises(ValueError, match="observations"):
        K.flatten_trajectories([(tuples[0][0][:-1], tuples[0][1], [], True)])
    with pytest.raises(ValueError, match="no trajectories"):
        K.flatten_trajectories([])
    # the callback builds those tuples; without `imitation` returnTrajectories hands them back
    cb = K.RecordTrajectoryCallback()
    for L, (o, a, _, _) in zip(lens, tuples):
        for t in range(L):
            cb.callback(o[t], o[t + 1], a[t], 0.0, t == L - 1, {"t": t})
    assert cb.numTrajectories == 3 and cb.trajectoryObs == []
    got = cb.returnTrajectories()
    assert len(got) == 3
    o2, a2 = K.flatten_trajectories(got)
    np.testing.assert_array_equal(o2, obs)
    np.testing.assert_array_equal(a2, acts)
    assert [len(t[2]) for t in cb.trajectories] == list(lens) and all(t[3] is True for t in cb.trajectories)
    k = K.imitationKickstarter(env="e", obs=1, actions=2, policy=3)
    assert (k.env, k.obs, k.actions, k.policy, k.trajectories) == ("e", 1, 2, 3, [])
    with pytest.raises(NotImplementedError):
        k.play()


def test_kickstarter_trains_on_the_cpu_through_autograd():
    """No GPU: bc_train takes the autograd path; the policy moves, is returned, and fits better."""
    K = _compat()
    pol, ro, _ = P.setup_cpu(7, 2, 96, seed=4)
    obs, acts = ro.obs.reshape(96, 7), ro.actions.reshape(96, 2)
    from rl_rocket_amd.rollout import _policy_tensors

    before = [p.detach().clone() for p in _policy_tensors(pol)]
    n0 = R.reference(pol, obs, acts, torch.arange(96))[1][0]
    k = K.imitationKickstarter(obs=obs.numpy(), actions=acts.numpy(), policy=pol)
    assert k.train(n_epochs=5) is pol
    for name, a, b in zip(P.NAMES, before, _policy_tensors(pol)):  # the value half's gradient is zero: it stays
        assert torch.equal(a, b) == (name in P.VF_NAMES), name
    assert int(k.optimizer.state[pol.log_std]["step"]) == 15  # 96 rows in minibatches of 32, 5 epochs
    assert int(k.optimizer.state[pol.value_net.weight]["step"]) == 15  # the value half steps too (zeros)
    assert R.reference(pol, obs, acts, torch.arange(96))[1][0] < n0 and set(k.stats) == set(R.STATS)


def _hand_trace():
    from rl_rocket_amd.eval_trace import EvalTrace

    K, ne, cap, ns, na = 2, 3, 4, 7, 2
    norm = np.array([3.0, 7.0, 0.1, 11.0, 1e3, 0.3, 41000.0])
    cfg = types.SimpleNamespace(state_normalizer=norm)
    state = torch.full((K, ne, cap + 1, ns), float("nan"))
    action = torch.full((K, ne, cap, na), float("nan"))
    code = lambda s, k, t: 100.0 * s + 10.0 * k + t  # noqa: E731
    for s in range(K):
        for k in range(ne):
            for t in range(cap + 1):
                state[s, k, t] = code(s, k, t) + 0.125 * torch.arange(ns)
                if t < cap:
                    action[s, k, t] = torch.tensor([code(s, k, t), -code(s, k, t)]) / 1000.0
    # slot 0 records env 5 (2 episodes finished: 3 and 4 steps; the third cut by max_steps after 2),
    # slot 1 env 2 (3 finished: 6 steps, clipped at the capacity of 4; 1 step; 4 steps)
    length = torch.tensor([[3, 6], [4, 1], [2, 4]], dtype=torch.int32)
    episodes = torch.zeros(8, dtype=torch.int32)
    episodes[5], episodes[2] = 2, 3
    tr = EvalTrace(cfg, state, action, torch.zeros((K, ne, cap, 3)), length, torch.tensor([5, 2]), episodes=episodes)
    rows = [(0, 0, t) for t in range(3)] + [(0, 1, t) for t in range(4)] + [(1, 1, 0)] + [(1, 2, t) for t in range(4)]
    return tr, cfg, rows, code


def test_demonstrations_from_a_hand_built_trace():
    from rl_rocket_amd.bc import Demonstrations

    tr, cfg, rows, code = _hand_trace()
    d = Demonstrations.from_trace(tr, types.SimpleNamespace(cfg=cfg))
    assert len(d) == len(rows) == 3 + 4 + 1 + 4  # the sum of the finished, unclipped lengths
    assert d.obs.shape == (12, 7) and d.acts.shape == (12, 2) and d.obs.is_contiguous() and d.acts.is_contiguous()
    inv = (1.0 / cfg.state_normalizer).astype(np.float32)
    for i, (s, k, t) in enumerate(rows):  # slot-major, then episode, then step
        want = (code(s, k, t) + 0.125 * np.arange(7)).astype(np.float32) * inv
        np.testing.assert_array_equal(d.obs[i].numpy(), want)
        np.testing.assert_array_equal(d.acts[i].numpy(), np.float32([code(s, k, t), -code(s, k, t)]) / np.float32(1000.0))
    assert bool(torch.isfinite(d.obs).all()) and bool(torch.isfinite(d.acts).all())
    # without the evaluator's count every episode of the trace counts as finished; the clipped one still leaves
    tr.episodes = None
    assert len(Demonstrations.from_trace(tr, types.SimpleNamespace(cfg=cfg))) == 12 + 2
    with pytest.raises(ValueError, match="finished"):
        Demonstrations.from_trace(tr, types.SimpleNamespace(cfg=cfg), episodes="all")


def test_demonstrations_and_python_refusals():
    from rl_rocket_amd.bc import BCUpdate, Demonstrations, bc_train
    from rl_rocket_amd import rollout

    assert rollout.BCUpdate is BCUpdate and rollout.Demonstrations is Demonstrations and rollout.bc_train is bc_train
    d = Demonstrations.from_arrays(np.zeros((5, 14)), [[0.0, 1.0, 2.0]] * 5, "cpu")
    assert len(d) == 5 and d.obs.dtype == d.acts.dtype == torch.float32 and d.acts.shape == (5, 3)
    ro = types.SimpleNamespace(obs=torch.arange(2.0 * 3 * 7).reshape(2, 3, 7), actions=torch.ones(2, 3, 2))
    r = Demonstrations.from_rollout(ro)
    assert torch.equal(r.obs, ro.obs.reshape(6, 7)) and r.obs.data_ptr() == ro.obs.data_ptr() and len(r) == 6
    with pytest.raises(ValueError):
        Demonstrations(torch.zeros(4, 14), torch.zeros(5, 3))
    with pytest.raises(ValueError):
        Demonstrations(torch.zeros(4, 14, dtype=torch.float64), torch.zeros(4, 3))
    with pytest.raises(ValueError):
        Demonstrations(torch.zeros(14, 4).T, torch.zeros(4, 3))
    pol, ro, _ = P.setup_cpu(14, 3, 64, seed=3)
    demos = Demonstrations(ro.obs.reshape(64, 14), ro.actions.reshape(64, 3))
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="fused=True"):  # CPU tensors, no capturable Adam
        bc_train(pol, opt, demos, fused=True)
    with pytest.raises(ValueError, match="group"):
        bc_train(pol, opt, demos, fused=True, group=object())
    with pytest.raises(ValueError, match="batch_size"):
        bc_train(pol, opt, demos, batch_size=65)
    with pytest.raises(ValueError, match="capturable"):
        BCUpdate(pol, opt, demos, 32)
    with pytest.raises(ValueError, match="ent_weight"):
        BCUpdate(pol, opt, demos, 32, ent_weight=-1.0)
    with pytest.raises(ValueError, match="l2_weight"):
        BCUpdate(pol, opt, demos, 32, l2_weight=float("nan"))
    # drop_last: 64 rows at 24 per minibatch are 2 steps per epoch; batch_size=None is one of 64 rows
    before = pol.log_std.detach().clone()
    st = bc_train(pol, opt, demos, n_epochs=2, batch_size=24)
    assert int(opt.state[pol.log_std]["step"]) == 4 and set(st) == set(R.STATS) and not torch.equal(before, pol.log_std)
    bc_train(pol, opt, demos)
    assert int(opt.state[pol.log_std]["step"]) == 5
    assert bc_train(pol, opt, demos, n_epochs=0) == {}
