"""rr_a2c_update's host side (no GPU): the C declarations and their ctypes mirrors, the refusals that come
before any HIP call, the translation unit of its own and its kernels' descriptors, RMSpropTFLike against a
hand-written float64 loop, a2c_update's autograd path against the explicit restatement in a2c_ref, and the
Python refusals."""
import copy
import ctypes
import json
import os
import re
import struct
import subprocess

import pytest
import torch

import a2c_ref as R
import bc_host_common as C
import ppo_ref as P
from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["int obs_dim", "int act_dim", "float* const* params", "float* const* grads", "float* const* square_avg",
        "float* const* exp_avg", "float* const* step", "const float* obs", "const float* actions",
        "const float* advantages", "const float* returns", "const int64_t* idx", "int64_t batch",
        "int normalize_advantage", "float ent_coef", "float vf_coef", "float max_grad_norm", "int optimizer",
        "const float* lr", "double alpha_or_beta1", "double beta2", "float eps", "float* stats", "void* workspace",
        "int64_t workspace_bytes", "void* stream"]


def test_header_declares_the_entry_points_and_signatures_mirror_them():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14  # a pure addition
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    new = re.search(r"int\s+rr_a2c_update\s*\(([^;]*)\)\s*;", code)
    assert [" ".join(a.split()) for a in new.group(1).split(",")] == ARGS
    res, argtypes = _lib.SIGNATURES["rr_a2c_update"]
    assert res is ctypes.c_int and len(argtypes) == len(ARGS)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
    for a, t in zip(ARGS, argtypes):
        assert t is (ctypes.c_void_p if "*" in a else kinds[a.split()[0]]), a
    assert _lib.SIGNATURES["rr_a2c_update_workspace_size"] == _lib.SIGNATURES["rr_ppo_update_workspace_size"]
    assert re.search(r"int\s+rr_a2c_update_workspace_size\s*\(\s*int obs_dim,\s*int act_dim,\s*int64_t batch,\s*"
                     r"int64_t\* bytes\)\s*;", code)
    assert re.search(r"RR_A2C_RMSPROP = 0, RR_A2C_RMSPROP_TF = 1, RR_A2C_ADAM = 2", code)
    assert (_lib.RR_A2C_RMSPROP, _lib.RR_A2C_RMSPROP_TF, _lib.RR_A2C_ADAM) == (0, 1, 2)
    enum = re.findall(r"\b(RR_A2C_STAT_[A-Z0-9_]+)\b",
                      code[code.index("RR_A2C_STAT_POLICY_LOSS = 0"):code.index("RR_A2C_STAT_SLOTS")])
    assert enum == ["RR_A2C_STAT_" + s.upper() for s in R.STATS] and [getattr(_lib, k) for k in enum] == list(range(5))
    assert re.search(r"RR_A2C_STAT_SLOTS\s*=\s*8\b", code) and _lib.RR_A2C_STAT_SLOTS == 8
    from rl_rocket_amd import a2c

    assert a2c.STAT_NAMES == R.STATS


def test_library_exports_the_symbols_and_keeps_the_launcher_hidden():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("rr_a2c_update", "rr_a2c_update_workspace_size"):
        assert re.search(r"\bT %s\b" % name, out)
    assert not re.search(r"rrc_launch_a2c", out)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for ns, na in ((14, 3), (7, 2)):
        for bs in (2, 128, 129, 16385, 65536, 327680):  # rr_ppo_update's sections: both towers' partial vectors
            assert lib.rr_a2c_update_workspace_size(ns, na, bs, ctypes.byref(a)) == _lib.RR_OK
            assert lib.rr_ppo_update_workspace_size(ns, na, bs, ctypes.byref(b)) == _lib.RR_OK
            assert a.value == b.value and a.value % 16 == 0


def _ptrs(k=13, null_at=None):
    arr = (ctypes.c_void_p * k)(*[0x100000 + 0x1000 * i for i in range(k)])
    if null_at is not None:
        arr[null_at] = None
    return arr


def test_refuses_bad_arguments_before_any_hip_call():
    """Never-read fake device addresses and a NULL stream: every refusal returns RR_EINVAL with its text
    before a launch (a launch on these addresses would fault or fail: there is no device here)."""
    lib = _lib.load()
    V = ctypes.c_void_p
    call, sz = "rr_a2c_update", "rr_a2c_update_workspace_size"
    p, nbytes = V(0x70000), ctypes.c_int64()

    def refused(rc, who, text):
        assert rc == _lib.RR_EINVAL, (who, text, rc)
        assert lib.rr_last_error() == ("%s: %s" % (who, text)).encode(), (lib.rr_last_error(), who, text)

    bad_shapes = ((5, 2), (14, 2), (7, 3), (7, 4), (0, 0))
    for bad in bad_shapes:
        refused(lib.rr_a2c_update_workspace_size(*bad, 64, ctypes.byref(nbytes)), sz, C.GAUSS_SHAPE)
    for bs in (1, 0, -5):
        refused(lib.rr_a2c_update_workspace_size(14, 3, bs, ctypes.byref(nbytes)), sz, "batch >= 2 and bytes required")
    refused(lib.rr_a2c_update_workspace_size(14, 3, 64, None), sz, "batch >= 2 and bytes required")
    assert lib.rr_a2c_update_workspace_size(14, 3, 4096, ctypes.byref(nbytes)) == _lib.RR_OK
    need = nbytes.value
    names = ("params", "grads", "sq", "m", "step")

    def run(shape=(14, 3), obs=p, act=p, adv=p, ret=p, idx=p, batch=4096, norm=0, ent=0.0, vf=0.5, clip=0.5, opt=1,
            lr=p, a=0.99, b2=0.0, eps=1e-5, stats=p, ws=V(0x200000), ws_bytes=need, **lists):
        ls = [lists.get(k, _ptrs()) for k in names]
        return lib.rr_a2c_update(*shape, *ls, obs, act, adv, ret, idx, batch, norm, ent, vf, clip, opt, lr, a, b2, eps,
                                 stats, ws, ws_bytes, None)

    for bad in bad_shapes:
        refused(run(shape=bad), call, C.GAUSS_SHAPE)
    for bs in (1, 0, -5):
        refused(run(batch=bs), call, "batch >= 2 required")
    for opt in (-1, 3, 17):
        refused(run(opt=opt), call, "optimizer must be RR_A2C_RMSPROP, RR_A2C_RMSPROP_TF or RR_A2C_ADAM")
    for name in ("params", "grads", "sq", "step", "obs", "act", "adv", "ret", "idx", "lr", "ws"):
        for opt in (0, 1, 2):
            refused(run(opt=opt, **{name: None}), call, "null argument")
    refused(run(opt=2, b2=0.999, m=None), call, "null argument")  # Adam needs exp_avg; RMSprop takes NULL
    for name in ("params", "grads", "sq", "step"):
        for hole in (0, 7, 12):
            refused(run(m=None, **{name: _ptrs(null_at=hole)}), call, "null parameter, gradient or optimizer-state tensor")
    refused(run(opt=2, b2=0.999, m=_ptrs(null_at=5)), call, "null parameter, gradient or optimizer-state tensor")
    refused(run(ws_bytes=need - 16), call, "workspace smaller than %s" % sz)
    refused(run(batch=8192), call, "workspace smaller than %s" % sz)  # sized for 4096 rows: 32 workgroups, not 64
    refused(run(ws=V(0x200008)), call, "workspace must be 16-B aligned")
    for bad in (float("nan"), -0.1, float("inf"), -float("inf")):
        refused(run(ent=bad), call, "ent_coef must be finite and >= 0")
        refused(run(vf=bad), call, "vf_coef must be finite and >= 0")
        refused(run(clip=bad), call, "max_grad_norm must be finite and >= 0 (0: no clip)")
        refused(run(eps=bad), call, "eps must be finite and >= 0")
    for bad in (float("nan"), -0.1, 1.0, 1.5):
        refused(run(a=bad), call, "alpha must be in [0, 1)")
        refused(run(opt=2, a=bad, b2=0.999), call, "beta1 must be in [0, 1)")
        refused(run(opt=2, a=0.9, b2=bad), call, "beta2 must be in [0, 1)")
    for stats in (p, None):  # the statistics are optional: refused for the coefficient, not for them
        refused(run(stats=stats, ent=-1.0), call, "ent_coef must be finite and >= 0")


def test_build_compiles_the_translation_unit_of_its_own():
    src, inc = B.SRC_A2C, B.INC_A2C_RMSPROP
    assert os.path.dirname(src) == os.path.dirname(inc) == os.path.join(C.CSRC, "a2c")
    assert sorted(os.listdir(os.path.dirname(src))) == ["rocket_a2c.hip", "rocket_rmsprop_body.inc"]
    assert src in B.sources() and inc in B.sources() and B.sources() == sorted(B.sources())
    cmds = B.commands()
    mine = [c for c in cmds if src in c]
    assert len(cmds) == 6 and mine == [cmds[-1]] and "-shared" in mine[0]  # compiled in the linking step
    assert mine[0].index(B.SRC_BC) < mine[0].index(src) < mine[0].index(B.SRC_COLLECT_STATS)
    assert mine[0][-1] == B.SRC_COLLECT_STATS and not any(inc in c for c in cmds)
    for flag in B.COLLECT_FLAGS:  # the learner's code-generation setting
        assert flag in mine[0]
    unit = open(src).read()
    assert unit.index("#define RR_POL_PREFETCH_A 1") < unit.index('#include "rocket_policy.inc"')
    includes = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', unit, flags=re.M)
    assert includes == ["rocket_device.h", "rocket_policy.inc", "rocket_ppo.inc", "rocket_ppo_finish_body.inc",
                        "rocket_rmsprop_body.inc", "rocket_ppo_adam_body.inc"]  # the learner's bodies, not copies
    assert "ppo_grad_tower<OBS, ACT, 0, false, NORM, 4>" in unit and "ppo_grad_tower<OBS, ACT, 1, false, true>" in unit
    assert "ppo_prep_body<OBS, ACT>" in unit and "__builtin_amdgcn_mfma" not in unit
    assert unit.count("__global__") == 5


def test_new_kernels_use_no_scratch_and_the_learner_kernels_are_all_there():
    kd = C.kernel_descriptors()
    new = {n: v for n, v in kd.items() if "a2c_" in n and "_kernel" in n}
    for name, count in (("a2c_prep_kernelIL", 2), ("a2c_grad_kernelIL", 4), ("a2c_finish_kernelIL", 2),
                        ("a2c_adam_kernelIL", 2), ("a2c_rmsprop_kernelE", 1)):
        assert sum(name in n for n in new) == count, name
    assert len(new) == 11
    for n, v in new.items():
        assert struct.unpack_from("<I", v, 4)[0] == 0, n  # private_segment_fixed_size
    for name in ("ppo_prep_kernel", "ppo_grad_kernel", "ppo_finish_kernel", "adam_chain_kernel", "bc_grad_kernel"):
        assert sum(name + "IL" in n for n in kd) == 2, name


def test_committed_isa_comparison_covers_every_kernel_of_the_parent():
    with open(os.path.join(ROOT, "profiles", "a2c", "isa_before_after.json")) as f:
        rec = json.load(f)
    assert rec["kernels_in_parent"] == len(rec["before"]) >= 231
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert sorted(rec["added"]) == sorted(k for k in rec["after"] if k not in rec["before"])
    assert len(rec["added"]) == 11 and all("::a2c_" in k for k in rec["added"])
    assert sorted(rec["resources"]) == sorted(rec["added"])
    for k, r in rec["resources"].items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgprs"] <= 256, k


def test_rmsprop_tf_like_matches_a_float64_loop_and_differs_from_torch_rmsprop():
    from rl_rocket_amd.a2c import RMSpropTFLike

    g = torch.Generator().manual_seed(5)
    p0 = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((4, 3), (5,), ())]
    grads = [[torch.randn(t.shape, generator=g, dtype=torch.float64) * 10.0 ** (k - 2) for t in p0] for k in range(5)]
    ps = [torch.nn.Parameter(t.clone()) for t in p0]
    opt = RMSpropTFLike(ps, lr=7e-4)
    assert opt.defaults == dict(lr=7e-4, alpha=0.99, eps=1e-5)
    want, sq = [t.clone() for t in p0], [torch.ones_like(t) for t in p0]
    for k in range(5):
        if k == 3:
            opt.param_groups[0]["lr"] = 2e-2
        lr = opt.param_groups[0]["lr"]
        for p, gk in zip(ps, grads[k]):
            p.grad = gk.clone()
        opt.step()
        for i in range(3):  # the hand-written loop, element by element
            flat_p, flat_s, flat_g = want[i].reshape(-1), sq[i].reshape(-1), grads[k][i].reshape(-1)
            for e in range(flat_p.numel()):
                flat_s[e] = 0.99 * flat_s[e] + (1 - 0.99) * flat_g[e] * flat_g[e]
                flat_p[e] = flat_p[e] - lr * flat_g[e] / (float(flat_s[e]) + 1e-5) ** 0.5
        for p, w, s in zip(ps, want, sq):
            st = opt.state[p]
            assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == k + 1
            assert (p.detach() - w).abs().max().item() <= 1e-12 and (st["square_avg"] - s).abs().max().item() <= 1e-12
    # ones-init and eps inside the root: the first step is not torch.optim.RMSprop's
    a, b = torch.nn.Parameter(p0[0].clone()), torch.nn.Parameter(p0[0].clone())
    a.grad, b.grad = grads[2][0].clone(), grads[2][0].clone()
    tf, tr = RMSpropTFLike([a], lr=7e-4), torch.optim.RMSprop([b], lr=7e-4, alpha=0.99, eps=1e-5)
    tf.step()
    tr.step()
    assert torch.equal(tf.state[a]["square_avg"], 0.99 + 0.01 * grads[2][0] ** 2)  # from ones
    assert torch.allclose(tr.state[b]["square_avg"], 0.01 * grads[2][0] ** 2, rtol=1e-14, atol=0)  # from zeros
    assert (a.detach() - b.detach()).abs().max().item() > 1e-4
    # a closure is evaluated with gradients on; parameters without a gradient are left alone
    c = torch.nn.Parameter(torch.ones(2, dtype=torch.float64))
    o = RMSpropTFLike([c, torch.nn.Parameter(torch.ones(1))], lr=0.1)

    def closure():
        o.zero_grad()
        loss = (c ** 2).sum()
        loss.backward()
        return loss

    assert float(o.step(closure).detach()) == 2.0 and len(o.state) == 1 and bool((c.detach() < 1.0).all())
    for bad in (dict(lr=-1.0), dict(alpha=1.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            RMSpropTFLike([c], **bad)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("normalize", (False, True))
def test_a2c_update_autograd_path_matches_the_restatement(kind, normalize):
    """a2c_update(fused=False) on CPU tensors, in float64 so that the comparison is tight: the parameters
    after one call, and after a second from the state the first left, are a2c_ref.train_ref's (loss, clip,
    optimizer written out) to 1e-10."""
    from rl_rocket_amd.a2c import a2c_update
    from rl_rocket_amd.rollout import _policy_tensors

    pol, obs, act, adv, ret = R.pool_cpu(7, 2, 96, seed=11)
    pol, obs, act, adv, ret = pol.double(), obs.double(), act.double(), adv.double(), ret.double()
    ro = R.stub_rollout(7, 2, obs, act, adv, ret, log_probs=torch.full((96,), float("nan"), dtype=torch.float64))
    assert bool(torch.isnan(ro.log_probs).all())  # never read
    opt = R.make_optimizer(kind, pol, 1e-2, capturable=False)
    state = R.fresh_state(kind, _policy_tensors(pol))
    coef = dict(ent_coef=0.01, vf_coef=0.25)
    for call, max_norm in enumerate((0.5, None)):
        idx = torch.arange(96)
        _, st64 = R.reference(pol, obs, act, adv, ret, idx, torch.float64, normalize, **coef)
        raw, _ = R.reference(pol, obs, act, adv, ret, idx, torch.float64, normalize, **coef)
        want = R.train_ref(kind, pol, obs, act, adv, ret, state, 1e-2, normalize, max_norm=max_norm, **coef)
        got = a2c_update(pol, opt, ro, normalize, max_grad_norm=max_norm, fused=False, **coef)
        assert set(got) == set(R.STATS)
        for name, r in zip(R.STATS, st64):
            assert got[name] == pytest.approx(r, rel=1e-10, abs=1e-12), name
        if call == 0:  # the clip bit: the returns' scale puts the norm far above 0.5
            assert P.clip_coef64(raw, 0.5) < 0.1
        for name, t, w in zip(P.NAMES, _policy_tensors(pol), want):
            assert t.dtype == torch.float64
            assert (t.detach() - w).abs().max().item() <= 1e-10 * max(1.0, w.abs().max().item()), (call, name)
        assert state["step"] == call + 1


def _cpu_case(hidden=(64, 64)):
    from rl_rocket_amd.rollout import MlpActorCritic

    pol = MlpActorCritic(14, 3, hidden=hidden)
    n = 32
    ro = R.stub_rollout(14, 3, torch.zeros(n, 14), torch.zeros(n, 3), torch.zeros(n), torch.zeros(n))
    return pol, ro


def test_python_refusals():
    from rl_rocket_amd import a2c, rollout
    from rl_rocket_amd.a2c import A2CUpdate, GraphedA2C, RMSpropTFLike, _check_rows, a2c_update
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic

    for name in ("A2CUpdate", "GraphedA2C", "RMSpropTFLike", "a2c_update"):
        assert getattr(rollout, name) is getattr(a2c, name) and getattr(a2c, name).__module__ == a2c.__name__
    entries = (lambda *a, **k: A2CUpdate(*a, **k), lambda *a, **k: a2c_update(*a, fused=True, **k),
               lambda *a, **k: GraphedA2C(*a, **k))

    def all_refuse(pol, opt, ro, match):
        for f in entries:
            with pytest.raises(ValueError, match=match):
                f(pol, opt, ro)

    pol, ro = _cpu_case()
    tf = RMSpropTFLike(pol.parameters())
    all_refuse(pol, tf, ro, "CPU tensors")
    cat = MlpCategoricalActorCritic(7, 4)
    ro7 = R.stub_rollout(7, 1, torch.zeros(8, 7), torch.zeros(8, 1), torch.zeros(8), torch.zeros(8))  # [n, 1] indices
    all_refuse(cat, RMSpropTFLike(cat.parameters()), ro7, "Categorical A2C call is a follow-up")
    small, _ = _cpu_case(hidden=(32, 32))
    all_refuse(small, RMSpropTFLike(small.parameters()), ro, "64x64")
    for kw, match in ((dict(momentum=0.9), "momentum"), (dict(centered=True), "centered"),
                      (dict(weight_decay=1e-3), "weight decay"), (dict(), "capturable")):
        all_refuse(pol, torch.optim.RMSprop(pol.parameters(), **kw), ro, match)
    all_refuse(pol, torch.optim.Adam(pol.parameters()), ro, "capturable")
    all_refuse(pol, torch.optim.SGD(pol.parameters(), lr=0.1), ro, "SGD")
    all_refuse(pol, RMSpropTFLike(list(pol.parameters())[:3]), ro, "exactly the policy's parameters")
    for bad in (dict(ent_coef=-0.1), dict(vf_coef=float("nan")), dict(max_grad_norm=float("inf"))):
        for f in entries:
            with pytest.raises(ValueError, match=next(iter(bad))):
                f(pol, tf, ro, **bad)
    # idx: int64, one dimension, 2 .. n rows, contiguous, on the rollout's device
    dev = torch.device("cpu")
    _check_rows(torch.arange(32), 32, dev)
    _check_rows(torch.arange(2), 32, dev)
    for bad in (torch.arange(32, dtype=torch.int32), torch.arange(32.0), torch.arange(33), torch.arange(1),
                torch.arange(32).reshape(2, 16), torch.arange(64)[::2], [0, 1, 2]):
        with pytest.raises(ValueError, match="idx must be"):
            _check_rows(bad, 32, dev)
    with pytest.raises(ValueError, match="idx must be"):
        _check_rows(torch.arange(8), 32, torch.device("meta"))
    # fused=None and fused=False take the autograd path here, a Categorical policy included
    before = copy.deepcopy(pol.state_dict())
    ro.returns.fill_(1.0)
    st = a2c_update(pol, tf, ro)
    assert set(st) == set(R.STATS) and float(tf.state[pol.log_std]["step"]) == 1.0
    assert any(not torch.equal(v, before[k]) for k, v in pol.state_dict().items())
    ro7.actions.fill_(1.0)
    ro7.advantages.fill_(0.5)
    st = a2c_update(cat, RMSpropTFLike(cat.parameters()), ro7, ent_coef=0.01, fused=False)
    assert st["entropy"] == pytest.approx(1.3863, abs=1e-2)  # four near-equal logits: log 4
