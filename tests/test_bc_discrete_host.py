"""rr_bc_update_discrete's host side (no GPU): the loss against a case worked by hand, bc_train's autograd
path on CPU tensors against tests/bc_discrete_ref.py, the refusals from Python (an index that names no
choice never reaches a gather), the C ABI's refusals with fake pointers (tests/test_discrete_host.py's
method), the translation unit of its own with its kernels' descriptors, the committed ISA comparison, and
the compat kick-starter on integer-action tuples."""
import copy
import ctypes
import json
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import bc_discrete_ref as R
import bc_host_common as C
import discrete_ref as D
from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compat():
    path = os.path.join(ROOT, "compat")
    if path not in sys.path:
        sys.path.insert(0, path)
    from my_environment.utils import imitation_kickstarter

    return imitation_kickstarter


def test_loss_on_a_hand_computed_case():
    """3 rows, K = 3, the logits themselves the only 'parameters': every figure and the gradient
    d loss / d z_ik = -(1/B) ((k == a_i) - p_ik) + (ent_weight/B) p_ik (log p_ik + H_i) + l2_weight z_ik
    from the exponentials written out."""
    z = [[0.2, -1.0, 0.5], [1.5, 0.0, -0.5], [-0.3, -0.3, 2.0]]
    a = [2, 1, 0]
    ew, l2w, Bn = 0.05, 0.3, 3
    t = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    loss, figures = R.loss_terms(t, torch.tensor(a), [t], ew, l2w)
    grad, = torch.autograd.grad(loss, [t])
    p = [[math.exp(v) / sum(math.exp(u) for u in row) for v in row] for row in z]
    H = [-sum(q * math.log(q) for q in row) for row in p]
    logp = [math.log(p[i][a[i]]) for i in range(Bn)]
    neglogp, entropy = -sum(logp) / Bn, sum(H) / Bn
    l2_norm = 0.5 * sum(v * v for row in z for v in row)
    want = (neglogp, entropy, -ew * entropy, sum(p[i][a[i]] for i in range(Bn)) / Bn, l2_norm, l2w * l2_norm,
            neglogp - ew * entropy + l2w * l2_norm)
    assert len(figures) == len(R.STATS) == 7
    for name, got, ref in zip(R.STATS, figures, want):
        assert got.item() == pytest.approx(ref, rel=1e-13, abs=1e-15), name
    for i in range(Bn):
        for k in range(3):
            dz = (-((k == a[i]) - p[i][k]) + ew * p[i][k] * (math.log(p[i][k]) + H[i])) / Bn + l2w * z[i][k]
            assert grad[i, k].item() == pytest.approx(dz, rel=1e-12, abs=1e-15), (i, k)
    # the package's own loss on a policy gives the reference's figures (float64, K = 3)
    from rl_rocket_amd.bc import _bc_loss

    pol, ro, _ = D.learner_inputs(3, n=40, seed=5)
    p64 = copy.deepcopy(pol).double()
    obs, acts = ro.obs.reshape(40, 7), ro.actions.reshape(40, 1)
    _, st = R.reference(pol, obs, acts, torch.arange(40), ent_weight=0.1, l2_weight=0.01)
    _, fig = _bc_loss(p64, obs.double(), acts.double(), 0.1, 0.01)
    for name, x, y in zip(R.STATS, fig, st):
        assert float(x.detach()) == pytest.approx(y, rel=1e-12), name


def test_a_probability_that_underflows_counts_zero_entropy():
    lp = torch.tensor([[120.0, 0.0, -120.0, 0.0]])
    _, fig = R.loss_terms(lp, torch.tensor([2]), [], 0.0, 0.0)
    assert fig[0].item() == 240.0 and fig[1].item() == 0.0 and fig[3].item() == 0.0


@pytest.mark.parametrize("k", [4, 2])
def test_bc_train_autograd_on_cpu_matches_the_reference_after_one_step(k):
    """One minibatch of all 48 rows (one permutation, one step): the gradients left in .grad are the
    reference's (the learner's bar: 1e-4 max |fp64| + 1e-7 per tensor), the parameters are float64 Adam
    applied to them, all 12 tensors move (l2 on, so the value half does), and the seven names come back.
    Adam's first step is -lr g / (|g| + eps): where |g| >= 1e-4 a gradient error within the bar moves it by
    less than 1e-8, so there the step is the float64 one within fp32 rounding of the parameter (2e-7
    max(1, |p|)); everywhere it is at most lr."""
    import bc_ref
    from rl_rocket_amd.bc import Demonstrations, bc_train
    from rl_rocket_amd.rollout import _policy_tensors

    pol, ro, _ = D.learner_inputs(k, n=48, seed=7)
    obs, acts = ro.obs.reshape(48, 7).contiguous(), ro.actions.reshape(48, 1).contiguous()
    grads, st = R.reference(pol, obs, acts, torch.arange(48), ent_weight=0.02, l2_weight=0.05)
    before = [t.detach().clone() for t in _policy_tensors(pol)]
    zeros = [torch.zeros_like(t) for t in before]
    p64, _, _, _ = bc_ref.adam_step_ref(before, grads, zeros, zeros, 0, 1e-3)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    out = bc_train(pol, opt, Demonstrations(obs, acts), n_epochs=1, ent_weight=0.02, l2_weight=0.05, fused=False)
    assert tuple(out) == R.STATS
    for name, got, want in zip(R.STATS, (out[s] for s in R.STATS), st):
        assert got == pytest.approx(want, rel=1e-5, abs=1e-6), name
    tensors = _policy_tensors(pol)
    assert len(tensors) == 12
    for name, t, a, p, g in zip(R.NAMES, tensors, before, p64, grads):
        assert not torch.equal(t.detach(), a), name
        assert int(opt.state[t]["step"]) == 1
        assert (t.grad.double() - g).abs().max().item() <= 1e-4 * g.abs().max().item() + 1e-7, name
        err = (t.detach().double() - p).abs()
        big = g.abs() >= 1e-4
        assert bool(big.any()) and bool((err[big] <= 2e-7 * p[big].abs().clamp(min=1.0)).all()), name
        assert (t.detach().double() - a.double()).abs().max().item() <= 1e-3 * (1 + 1e-6) + 2e-7, name
    assert 0.0 < out["entropy"] <= math.log(k) and 0.0 < out["prob_true_act"] < 1.0


def test_python_refusals():
    from rl_rocket_amd.bc import BCUpdate, Demonstrations, _check_indices, bc_train
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic

    pol, ro, _ = D.learner_inputs(4, n=32, seed=1)
    obs, acts = ro.obs.reshape(32, 7).contiguous(), ro.actions.reshape(32, 1).contiguous()
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    start = [p.detach().clone() for p in pol.parameters()]
    for bad in (4.0, -1.0, 1.5, float("nan"), float("inf")):
        a = acts.clone()
        a[17, 0] = bad
        with pytest.raises(ValueError, match=r"integers in \[0, 4\)"):
            bc_train(pol, opt, Demonstrations(obs, a), fused=False)
        with pytest.raises(ValueError, match=r"integers in \[0, 4\)"):
            bc_train(pol, opt, Demonstrations(obs, a))
        with pytest.raises(ValueError, match=r"integers in \[0, 4\)"):
            BCUpdate(pol, opt, Demonstrations(obs, a), 16)
    a3 = acts.clone()
    a3[0, 0] = 3.0  # valid at K = 4, out of range at K = 3
    _check_indices(a3, 4)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        bc_train(MlpCategoricalActorCritic(7, 3, D.TABLES[3]), opt, Demonstrations(obs, a3), fused=False)
    wide = torch.zeros(32, 2)
    with pytest.raises(ValueError, match=r"\[M, 1\]"):
        bc_train(pol, opt, Demonstrations(obs, wide), fused=False)
    with pytest.raises(ValueError, match=r"\[M, 1\]"):
        BCUpdate(pol, opt, Demonstrations(obs, wide), 16)
    for p, s in zip(pol.parameters(), start):  # refused before any step
        assert torch.equal(p.detach(), s)
    demos = Demonstrations(obs, acts)
    with pytest.raises(ValueError, match="fused=True"):  # CPU tensors, no capturable Adam
        bc_train(pol, opt, demos, fused=True)
    with pytest.raises(ValueError, match="group"):
        bc_train(pol, opt, demos, fused=True, group=object())
    with pytest.raises(ValueError, match="capturable"):
        BCUpdate(pol, opt, demos, 16)
    with pytest.raises(ValueError, match="2 .. 4"):
        BCUpdate(MlpCategoricalActorCritic(7, 5, [[0.0, 0.0]] * 5), opt, demos, 16)
    # Demonstrations: integer arrays become [M, 1] float32; a Categorical collect's buffers are viewed
    d = Demonstrations.from_arrays(np.zeros((5, 7)), np.array([0, 3, 1, 2, 3]), "cpu")
    assert d.acts.shape == (5, 1) and d.acts.dtype == torch.float32 and d.acts[:, 0].tolist() == [0, 3, 1, 2, 3]
    r = Demonstrations.from_rollout(ro)
    assert r.acts.shape == (32, 1) and r.acts.data_ptr() == ro.actions.data_ptr()


def test_c_abi_refuses_bad_arguments_before_any_hip_call():
    """Never-read fake device addresses and a NULL stream: every refusal returns RR_EINVAL with the message
    it had before the two calls shared their host path, before a launch."""
    C.check_refusals("rr_bc_update_discrete", (7, 4), 12, [((14, 4), C.CAT_OBS), ((14, 3), C.CAT_OBS), ((5, 2), C.CAT_OBS),
                                                            ((7, 5), C.CAT_K), ((7, 1), C.CAT_K)])


def test_workspace_size_grows_with_batch_and_is_one_tower():
    lib = _lib.load()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for k in (2, 3, 4):
        sizes = []
        for bs in (2, 128, 129, 16384, 16385, 65536):
            assert lib.rr_bc_update_discrete_workspace_size(7, k, bs, ctypes.byref(a)) == _lib.RR_OK
            assert a.value % 16 == 0
            sizes.append(a.value)
        # one partial-gradient vector per workgroup, one workgroup per 128 rows up to 128 of them
        assert sizes[0] == sizes[1] < sizes[2] < sizes[3] == sizes[4] == sizes[5], sizes
        assert sizes[3] - sizes[0] == 127 * (sizes[2] - sizes[1])
        # one tower's partial vectors: less than the PPO call's two
        assert lib.rr_ppo_update_discrete_workspace_size(7, k, 65536, ctypes.byref(b)) == _lib.RR_OK
        assert sizes[5] < b.value
    C.check_workspace_sizes("rr_bc_update_discrete")


def test_header_signatures_and_exports():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14  # a pure addition
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    new = re.search(r"int\s+rr_bc_update_discrete\s*\(([^;]*)\)\s*;", code)
    args = [" ".join(a.split()) for a in new.group(1).split(",")]
    old = re.search(r"int\s+rr_bc_update\s*\(([^;]*)\)\s*;", code)
    old_args = [" ".join(a.split()) for a in old.group(1).split(",")]
    assert args == [a if a != "int act_dim" else "int n_choices" for a in old_args]  # rr_bc_update's, K for act_dim
    assert _lib.SIGNATURES["rr_bc_update_discrete"] == _lib.SIGNATURES["rr_bc_update"]
    assert _lib.SIGNATURES["rr_bc_update_discrete_workspace_size"] == _lib.SIGNATURES["rr_bc_update_workspace_size"]
    comment = text[text.index("rr_bc_update for this policy"):text.index("int rr_bc_update_discrete_workspace_size")]
    assert "MUST hold integers in [0, n_choices)" in comment and "no address depends on them" in comment
    _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("rr_bc_update_discrete", "rr_bc_update_discrete_workspace_size"):
        assert re.search(r"\bT %s\b" % name, out)
    assert not re.search(r"rrc_launch_bc_discrete", out)


def test_build_compiles_the_translation_unit_of_its_own():
    C.check_unit(B.SRC_BC_DISCRETE, "bc_discrete", B.SRC_DISCRETE, 1)


def test_new_kernels_use_no_scratch():
    """From the built library: the four new kernels, one instantiation each, with no scratch
    (private_segment_fixed_size, bytes 4..8 of the kernel descriptor)."""
    kd = C.kernel_descriptors()
    new = {n: v for n, v in kd.items() if "bcd_" in n and "_kernel" in n}
    for name in ("bcd_pack_kernel", "bcd_grad_kernel", "bcd_finish_kernel", "bcd_adam_kernel"):
        assert sum(name + "ILi7ELi4E" in n for n in new) == 1, name
    assert len(new) == 4
    for n, v in new.items():
        assert struct.unpack_from("<I", v, 4)[0] == 0, n


def test_committed_isa_comparison_covers_every_kernel_of_the_parent():
    with open(os.path.join(ROOT, "profiles", "bc_discrete", "isa_before_after.json")) as f:
        rec = json.load(f)
    assert rec["kernels_in_parent"] == len(rec["before"]) >= 175 and rec["changed"] == 0
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert sorted(rec["added"]) == sorted(k for k in rec["after"] if k not in rec["before"])
    assert len(rec["added"]) == 4 and all("::bcd_" in k for k in rec["added"])


def test_kickstarter_trains_a_categorical_policy_on_integer_action_tuples():
    """RecordTrajectoryCallback tuples whose actions are the keyboard's indices (integers): flattened to
    [M, 1] float32, cloned through autograd on the CPU; the policy is returned, fits better, and the value
    half (zero gradient at l2_weight 0) stays. Arrays of obs / actions are taken too; an index that names no
    choice is refused."""
    K = _compat()
    from rl_rocket_amd.rollout import _policy_tensors

    pol, ro, _ = D.learner_inputs(4, n=96, seed=4)
    teacher, _, _ = D.learner_inputs(4, n=96, seed=9, head_scale=4.0)
    obs = ro.obs.reshape(96, 7)
    with torch.no_grad():
        acts = teacher(obs)[0].argmax(-1)  # what a deterministic demonstrator chose
    cb = K.RecordTrajectoryCallback()
    rows = 0
    for lo, hi in ((0, 40), (40, 41), (41, 95)):  # three episodes; row 95 is the last one's final observation
        for t in range(lo, hi):
            cb.callback(obs[t].numpy(), obs[t + 1].numpy(), int(acts[t]), 0.0, t == hi - 1, {})
            rows += 1
    assert cb.numTrajectories == 3 and cb.trajectories[0][1].dtype.kind == "i"
    o, a = K.flatten_trajectories(cb.trajectories)
    assert o.shape == (rows, 7) and a.shape == (rows, 1) and a.dtype == np.float32
    np.testing.assert_array_equal(a[:, 0], acts[:95].numpy().astype(np.float32))
    every = torch.arange(rows)
    n0 = R.reference(pol, torch.from_numpy(o), torch.from_numpy(a), every)[1][0]
    before = [p.detach().clone() for p in _policy_tensors(pol)]
    kick = K.imitationKickstarter(policy=pol)
    kick.trajectories = cb.trajectories
    assert kick.train(n_epochs=5) is pol
    for name, x, y in zip(R.NAMES, before, _policy_tensors(pol)):
        assert torch.equal(x, y) == (name in R.VF_NAMES), name
    assert int(kick.optimizer.state[pol.action_net.bias]["step"]) == 5 * (rows // 32)
    assert int(kick.optimizer.state[pol.value_net.weight]["step"]) == 5 * (rows // 32)
    assert R.reference(pol, torch.from_numpy(o), torch.from_numpy(a), every)[1][0] < n0
    assert set(kick.stats) == set(R.STATS)
    k2 = K.imitationKickstarter(obs=o, actions=acts[:95].numpy(), policy=pol)  # a 1-D integer array
    assert k2.train(n_epochs=1) is pol and int(k2.optimizer.state[pol.action_net.bias]["step"]) == rows // 32
    bad = acts[:95].numpy().copy()
    bad[3] = 4
    with pytest.raises(ValueError, match="integers"):
        K.imitationKickstarter(obs=o, actions=bad, policy=pol).train()
    assert "MlpCategoricalActorCritic" in K.__doc__
