"""rr_a2c_update_discrete's host side (no GPU): the C declarations and their ctypes mirrors, the refusals that
come before any HIP call, the workspace size, the translation unit of its own and its kernels' descriptors,
the committed ISA comparison, a2c_update_discrete's autograd path against a2c_update(fused=False) and, on
every loss-term case, against the restatement in a2c_discrete_ref, and the Python refusals that CPU tensors can
reach. The refusals that come after the CPU-tensor one (a rollout under 2 rows, the two-launch and per-step
collects inside GraphedA2CDiscrete) are raised in tests/test_gpu_a2c_discrete.py.
test_the_restated_derivative_is_autograd_s is a check of the helper alone (it runs nothing the feature adds,
so it is no feature test): it shows that the reference is independent of the kernel's formula."""
import copy
import ctypes
import json
import os
import re
import struct
import subprocess

import pytest
import torch

import a2c_discrete_ref as A
import bc_host_common as C
import discrete_ref as D
import ppo_ref as P
from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["int obs_dim", "int n_choices", "float* const* params", "float* const* grads", "float* const* square_avg",
        "float* const* exp_avg", "float* const* step", "const float* obs", "const float* actions",
        "const float* advantages", "const float* returns", "const int64_t* idx", "int64_t batch",
        "int normalize_advantage", "float ent_coef", "float vf_coef", "float max_grad_norm", "int optimizer",
        "const float* lr", "double alpha_or_beta1", "double beta2", "float eps", "float* stats", "void* workspace",
        "int64_t workspace_bytes", "void* stream"]
CALL, SIZE = "rr_a2c_update_discrete", "rr_a2c_update_discrete_workspace_size"


def test_header_declares_the_entry_points_and_signatures_mirror_them():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14  # a pure addition
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    new = re.search(r"int\s+rr_a2c_update_discrete\s*\(([^;]*)\)\s*;", code)
    assert [" ".join(a.split()) for a in new.group(1).split(",")] == ARGS
    res, argtypes = _lib.SIGNATURES[CALL]
    assert res is ctypes.c_int and len(argtypes) == len(ARGS)
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
    for a, t in zip(ARGS, argtypes):
        assert t is (ctypes.c_void_p if "*" in a else kinds[a.split()[0]]), a
    assert _lib.SIGNATURES[CALL] == _lib.SIGNATURES["rr_a2c_update"]  # the Gaussian call's, n_choices for act_dim
    assert _lib.SIGNATURES[SIZE] == _lib.SIGNATURES["rr_ppo_update_discrete_workspace_size"]
    assert re.search(r"int\s+rr_a2c_update_discrete_workspace_size\s*\(\s*int obs_dim,\s*int n_choices,\s*"
                     r"int64_t batch,\s*int64_t\* bytes\)\s*;", code)
    # the header carries the call's own contract
    doc = text[text.index("One A2C update of this policy"):text.index("int rr_a2c_update_discrete_workspace_size")]
    for words in ("n_choices outside 2 .. 4", "obs_dim != 7", "four launches", "no atomics", "[4][64] + [4]",
                  "RR_A2C_STAT_SLOTS", "never used as an offset"):
        assert words in " ".join(doc.replace("*", " ").split()), words


def test_library_exports_the_symbols_and_keeps_the_launcher_hidden():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in (CALL, SIZE):
        assert re.search(r"\bT %s\b" % name, out)
    assert not re.search(r"rrc_launch_a2c_discrete", out)


def test_workspace_size_is_a_multiple_of_16_monotone_and_holds_the_sink():
    lib = _lib.load()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for k in (2, 3, 4):
        last = 0
        for bs in (2, 33, 128, 129, 4097, 16385, 65536, 327680):
            assert lib.rr_a2c_update_discrete_workspace_size(7, k, bs, ctypes.byref(a)) == _lib.RR_OK
            assert a.value % 16 == 0 and a.value >= last
            last = a.value
            # rr_ppo_update_discrete's sections: both towers' partial vectors, then the [4][64] + [4] sink
            assert lib.rr_ppo_update_discrete_workspace_size(7, k, bs, ctypes.byref(b)) == _lib.RR_OK
            assert a.value == b.value
        assert lib.rr_a2c_update_discrete_workspace_size(7, k, 129, ctypes.byref(a)) == _lib.RR_OK
        assert lib.rr_a2c_update_discrete_workspace_size(7, k, 128, ctypes.byref(b)) == _lib.RR_OK
        assert a.value > b.value  # a second workgroup's partial vectors


def _ptrs(k=12, null_at=None):
    arr = (ctypes.c_void_p * k)(*[0x100000 + 0x1000 * i for i in range(k)])
    if null_at is not None:
        arr[null_at] = None
    return arr


def test_refuses_bad_arguments_before_any_hip_call():
    """Never-read fake device addresses and a NULL stream: every refusal returns RR_EINVAL with its text
    before a launch (a launch on these addresses would fault or fail: there is no device here)."""
    lib = _lib.load()
    V = ctypes.c_void_p
    p, nbytes = V(0x70000), ctypes.c_int64()

    def refused(rc, who, text):
        assert rc == _lib.RR_EINVAL, (who, text, rc)
        assert lib.rr_last_error() == ("%s: %s" % (who, text)).encode(), (lib.rr_last_error(), who, text)

    bad_obs = ((14, 3), (5, 4), (0, 2), (6, 4))
    bad_k = ((7, 1), (7, 5), (7, 0), (7, -2))
    for bad in bad_obs:
        refused(lib.rr_a2c_update_discrete_workspace_size(*bad, 64, ctypes.byref(nbytes)), SIZE,
                "obs_dim must be 7 (the 3DOF env)")
    for bad in bad_k:
        refused(lib.rr_a2c_update_discrete_workspace_size(*bad, 64, ctypes.byref(nbytes)), SIZE,
                "n_choices must be in 2 .. 4")
    for bs in (1, 0, -5):
        refused(lib.rr_a2c_update_discrete_workspace_size(7, 4, bs, ctypes.byref(nbytes)), SIZE,
                "batch >= 2 and bytes required")
    refused(lib.rr_a2c_update_discrete_workspace_size(7, 4, 64, None), SIZE, "batch >= 2 and bytes required")
    assert lib.rr_a2c_update_discrete_workspace_size(7, 4, 4096, ctypes.byref(nbytes)) == _lib.RR_OK
    need = nbytes.value
    names = ("params", "grads", "sq", "m", "step")

    def run(shape=(7, 4), obs=p, act=p, adv=p, ret=p, idx=p, batch=4096, norm=0, ent=0.0, vf=0.5, clip=0.5, opt=1,
            lr=p, a=0.99, b2=0.0, eps=1e-5, stats=p, ws=V(0x200000), ws_bytes=need, **lists):
        ls = [lists.get(k, _ptrs()) for k in names]
        return lib.rr_a2c_update_discrete(*shape, *ls, obs, act, adv, ret, idx, batch, norm, ent, vf, clip, opt, lr, a,
                                          b2, eps, stats, ws, ws_bytes, None)

    for bad in bad_obs:
        refused(run(shape=bad), CALL, "obs_dim must be 7 (the 3DOF env)")
    for bad in bad_k:
        refused(run(shape=bad), CALL, "n_choices must be in 2 .. 4")
    for bs in (1, 0, -5):
        refused(run(batch=bs), CALL, "batch >= 2 required")
    for opt in (-1, 3, 17):
        refused(run(opt=opt), CALL, "optimizer must be RR_A2C_RMSPROP, RR_A2C_RMSPROP_TF or RR_A2C_ADAM")
    for name in ("params", "grads", "sq", "step", "obs", "act", "adv", "ret", "idx", "lr", "ws"):
        for opt in (0, 1, 2):
            refused(run(opt=opt, **{name: None}), CALL, "null argument")
    refused(run(opt=2, b2=0.999, m=None), CALL, "null argument")  # Adam needs exp_avg; RMSprop takes NULL
    for k in (2, 3, 4):
        for name in ("params", "grads", "sq", "step"):
            for hole in (0, 8, 11):  # 12 tensors: the last is b_value
                refused(run(shape=(7, k), m=None, **{name: _ptrs(null_at=hole)}), CALL,
                        "null parameter, gradient or optimizer-state tensor")
    refused(run(opt=2, b2=0.999, m=_ptrs(null_at=5)), CALL, "null parameter, gradient or optimizer-state tensor")
    refused(run(ws_bytes=need - 16), CALL, "workspace smaller than %s" % SIZE)
    refused(run(batch=8192), CALL, "workspace smaller than %s" % SIZE)  # sized for 4096 rows
    b = ctypes.c_int64()  # rr_ppo_update's bytes alone leave no room for the sink
    assert lib.rr_ppo_update_workspace_size(7, 2, 4096, ctypes.byref(b)) == _lib.RR_OK and b.value < need
    refused(run(ws=V(0x200008)), CALL, "workspace must be 16-B aligned")
    for bad in (float("nan"), -0.1, float("inf"), -float("inf")):
        refused(run(ent=bad), CALL, "ent_coef must be finite and >= 0")
        refused(run(vf=bad), CALL, "vf_coef must be finite and >= 0")
        refused(run(clip=bad), CALL, "max_grad_norm must be finite and >= 0 (0: no clip)")
        refused(run(eps=bad), CALL, "eps must be finite and >= 0")
    for bad in (float("nan"), -0.1, 1.0, 1.5):
        refused(run(a=bad), CALL, "alpha must be in [0, 1)")
        refused(run(opt=2, a=bad, b2=0.999), CALL, "beta1 must be in [0, 1)")
        refused(run(opt=2, a=0.9, b2=bad), CALL, "beta2 must be in [0, 1)")
    for stats in (p, None):  # the statistics are optional: refused for the coefficient, not for them
        refused(run(stats=stats, ent=-1.0), CALL, "ent_coef must be finite and >= 0")


def test_build_compiles_the_translation_unit_of_its_own():
    src = B.SRC_A2C_DISCRETE
    assert os.path.dirname(src) == os.path.join(C.CSRC, "a2c_discrete")
    assert os.listdir(os.path.dirname(src)) == ["rocket_a2c_discrete.hip"]
    assert src in B.sources() and B.INC_A2C_RMSPROP in B.sources() and B.sources() == sorted(B.sources())
    cmds = B.commands()
    mine = [c for c in cmds if src in c]
    assert len(cmds) == 6 and mine == [cmds[-1]] and "-shared" in mine[0]  # compiled in the linking step
    assert mine[0].index(B.SRC_A2C) < mine[0].index(src) < mine[0].index(B.SRC_COLLECT_STATS)
    for flag in B.COLLECT_FLAGS:  # the learner's code-generation setting
        assert flag in mine[0]
    unit = open(src).read()
    assert unit.index("#define RR_POL_PREFETCH_A 1") < unit.index('#include "rocket_policy.inc"')
    includes = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', unit, flags=re.M)
    assert includes == ["rocket_device.h", "rocket_policy.inc", "rocket_ppo.inc", "rocket_ppo_finish_body.inc",
                        "a2c/rocket_rmsprop_body.inc", "rocket_ppo_adam_body.inc"]  # the shared bodies, not copies
    assert "ppo_grad_tower<OBS, ACT, 0, false, NORM, 5>" in unit and "ppo_grad_tower<OBS, ACT, 1, false, true>" in unit
    assert "ppo_prep_body<OBS, ACT>" in unit and "discrete_pack_value<OBS, ACT>" in unit
    assert "__builtin_amdgcn_mfma" not in unit and "atomic" not in unit.replace("No atomics", "") and "asm" not in unit
    assert unit.count("__global__") == 5
    shared = open(os.path.join(C.CSRC, "rocket_ppo.inc")).read()
    assert "LOSS 5 (A2C for the Categorical policy" in shared and "struct A2cDiscreteLaunch" in shared


def test_new_kernels_use_no_scratch_and_the_earlier_a2c_kernels_are_all_there():
    kd = C.kernel_descriptors()
    new = {n: v for n, v in kd.items() if "a2cd_" in n and "_kernel" in n}
    for name, count in (("a2cd_prep_kernelIL", 1), ("a2cd_grad_kernelIL", 2), ("a2cd_finish_kernelIL", 1),
                        ("a2cd_adam_kernelIL", 1), ("a2cd_rmsprop_kernelE", 1)):
        assert sum(name in n for n in new) == count, name
    assert len(new) == 6
    for n, v in new.items():
        assert struct.unpack_from("<I", v, 4)[0] == 0, n  # private_segment_fixed_size
    assert sum("a2c_" in n and "_kernel" in n for n in kd) == 11  # rr_a2c_update's
    for name in ("discrete_grad_kernel", "discrete_finish_kernel", "dopts_finish_kernel"):
        assert sum(name + "IL" in n for n in kd) >= 1, name


def test_committed_isa_comparison_covers_every_kernel_of_the_parent():
    with open(os.path.join(ROOT, "profiles", "a2c_discrete", "isa_before_after.json")) as f:
        rec = json.load(f)
    assert rec["kernels_in_parent"] == len(rec["before"]) >= 242 and rec["changed"] == 0 and rec["removed"] == []
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert sorted(rec["added"]) == sorted(k for k in rec["after"] if k not in rec["before"])
    assert len(rec["added"]) == 6 and all("::a2cd_" in k for k in rec["added"])
    assert sorted(rec["resources"]) == sorted(rec["added"])
    for k, r in rec["resources"].items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgprs"] <= 256, k
    if os.path.exists(B.OUT):  # the record is of this tree's library
        now = B.kernel_isa_hashes(B.OUT)
        for k in rec["added"]:
            assert now[k] == rec["after"][k], k


def test_the_restated_derivative_is_autograd_s():
    """d loss / d z_k = -(A / B) ((k == a) - p_k) + (ent_coef / B) p_k (log p_k + H) for k < K, written out in
    float64 on the logits of a K = 3 policy, is what a2c_discrete_ref.loss_terms' autograd gives."""
    pol, obs, act, adv, ret = A.sweep_cpu(3)
    idx = torch.arange(257)
    p64 = copy.deepcopy(pol).double()
    logits, value = p64(obs[idx].double())
    logits = logits.detach().requires_grad_(True)
    a = act.reshape(-1)[idx].long()
    for normalize in (False, True):
        loss, figs = A.loss_terms(logits, value.detach(), a, adv[idx].double(), ret[idx].double(), normalize, 0.03, 0.5)
        (dz,) = torch.autograd.grad(loss, logits)
        Aj = adv[idx].double()
        if normalize:
            Aj = (Aj - Aj.mean()) / (Aj.std() + 1e-8)
        lsm = torch.log_softmax(logits.detach(), -1)
        p = lsm.exp()
        H = -(p * lsm).sum(-1, keepdim=True)
        hit = torch.nn.functional.one_hot(a, 3).double()
        want = (-(Aj[:, None] / 257) * (hit - p) + (0.03 / 257) * p * (lsm + H))
        assert (dz - want).abs().max().item() <= 1e-15
        f = [float(v.detach()) for v in figs]
        assert f[2] == pytest.approx(float(H.mean()), rel=1e-14)
        assert f[3] == pytest.approx(f[0] - 0.03 * f[2] + 0.5 * f[1], rel=1e-14)


@pytest.mark.parametrize("name", list(A.TERMS))
@pytest.mark.parametrize("bs", A.TERM_BATCHES)
def test_every_loss_term_case_is_sized_for_the_bars(name, bs):
    """The fp32 autograd reference meets the GPU tests' bars with room (at most half of each) on every
    loss-term case, so a miss on the GPU is the kernel's; each case is what its name says; and
    a2c_update_discrete's autograd path on the case's rows reports the restatement's five figures."""
    from rl_rocket_amd.a2c import RMSpropTFLike
    from rl_rocket_amd.a2c_discrete import a2c_update_discrete

    pol, data, idx, kw = A.terms_case(name, bs)
    mine = copy.deepcopy(pol)
    got = a2c_update_discrete(mine, RMSpropTFLike(mine.parameters()), A.rollout(*[t[idx].contiguous() for t in data]),
                              kw.get("normalize", False), ent_coef=kw["ent_coef"], vf_coef=kw.get("vf_coef", 0.5),
                              max_grad_norm=None)
    _, st64 = A.reference(pol, *data, idx, torch.float64, **kw)
    for stat, r in zip(A.STATS, st64):
        assert got[stat] == pytest.approx(r, rel=1e-4, abs=1e-5), stat
    share = A.shares(pol, data, idx, **kw)
    worst = max(share, key=share.get)
    print(name, bs, "worst share %s %.3f" % (worst, share[worst]))
    assert share[worst] <= 0.5, share
    with torch.no_grad():
        logits, _ = pol(data[0][idx])
        p = torch.softmax(logits, -1)
    if name == "underflow":
        assert bool((p[:, -1] == 0).all())  # the last choice's probability is 0 in fp32
    if name == "peaked":
        assert float((p.max(-1).values > 0.99).float().mean()) >= 0.5
    if name.startswith("const_adv"):
        assert float(data[2][idx].std()) == 0.0 and kw["normalize"]
        ref, st = A.reference(pol, *data, idx, torch.float64, **kw)
        assert st[0] == 0.0
        pi_zero = all(torch.count_nonzero(g).item() == 0 for n, g in zip(A.NAMES, ref) if n in P.PI_NAMES)
        assert pi_zero == (kw["ent_coef"] == 0.0)


def _cat_case(k=4, n=8, hidden=(64, 64)):
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic

    pol = MlpCategoricalActorCritic(7, k, D.TABLES[k] if k in D.TABLES else [(0.0, 0.0)] * k, hidden=hidden)
    ro = A.rollout(torch.zeros(n, 7), torch.zeros(n, 1), torch.zeros(n), torch.zeros(n))
    return pol, ro


def test_python_refusals():
    from rl_rocket_amd import a2c, a2c_discrete, rollout
    from rl_rocket_amd.a2c import A2CUpdate, GraphedA2C, RMSpropTFLike, a2c_update
    from rl_rocket_amd.a2c_discrete import A2CUpdateDiscrete, GraphedA2CDiscrete, a2c_update_discrete
    from rl_rocket_amd.rollout import MlpActorCritic

    for name in ("A2CUpdateDiscrete", "GraphedA2CDiscrete", "a2c_update_discrete"):
        assert getattr(rollout, name) is getattr(a2c_discrete, name)
        assert getattr(a2c_discrete, name).__module__ == a2c_discrete.__name__
    assert rollout.A2CUpdateDiscrete is a2c_discrete.A2CUpdateDiscrete
    assert issubclass(A2CUpdateDiscrete, A2CUpdate) and issubclass(GraphedA2CDiscrete, GraphedA2C)
    entries = (lambda *a, **k: A2CUpdateDiscrete(*a, **k), lambda *a, **k: a2c_update_discrete(*a, fused=True, **k),
               lambda *a, **k: GraphedA2CDiscrete(*a, **k))

    def all_refuse(pol, opt, ro, match):
        for f in entries:
            with pytest.raises(ValueError, match=match):
                f(pol, opt, ro)

    cat, ro = _cat_case()
    tf = RMSpropTFLike(cat.parameters())
    all_refuse(cat, tf, ro, "CPU tensors")
    gauss = MlpActorCritic(7, 2)
    ro2 = A.stub_rollout(7, 2, torch.zeros(8, 7), torch.zeros(8, 2), torch.zeros(8), torch.zeros(8))
    all_refuse(gauss, RMSpropTFLike(gauss.parameters()), ro2, "not the Gaussian MlpActorCritic")
    small, _ = _cat_case(hidden=(32, 32))
    all_refuse(small, RMSpropTFLike(small.parameters()), ro, "64x64")
    five, _ = _cat_case(k=5)
    all_refuse(five, RMSpropTFLike(five.parameters()), ro, "K = 2 .. 4 choices, not 5")
    ro14 = A.stub_rollout(14, 1, torch.zeros(8, 14), torch.zeros(8, 1), torch.zeros(8), torch.zeros(8))
    all_refuse(cat, tf, ro14, "6DOF")
    all_refuse(cat, tf, ro2, r"\[n, 1\] indices")
    for kw, match in ((dict(momentum=0.9), "momentum"), (dict(centered=True), "centered"),
                      (dict(weight_decay=1e-3), "weight decay"), (dict(), "capturable")):
        all_refuse(cat, torch.optim.RMSprop(cat.parameters(), **kw), ro, match)
    all_refuse(cat, torch.optim.Adam(cat.parameters()), ro, "capturable")
    all_refuse(cat, torch.optim.SGD(cat.parameters(), lr=0.1), ro, "SGD")
    all_refuse(cat, RMSpropTFLike(list(cat.parameters())[:3]), ro, "exactly the policy's parameters")
    for bad in (dict(ent_coef=-0.1), dict(vf_coef=float("nan")), dict(max_grad_norm=float("inf"))):
        for f in entries:
            with pytest.raises(ValueError, match=next(iter(bad))):
                f(cat, tf, ro, **bad)
    # the indices are validated with one reduction, NaN included
    a2c_discrete._check_indices(torch.tensor([[0.0], [3.0], [1.0]]), 4)
    for bad in ([[4.0]], [[-1.0]], [[0.5]], [[float("nan")]], [[2.0]]):
        with pytest.raises(ValueError, match=r"integers in \[0, 2\)"):
            a2c_discrete._check_indices(torch.tensor(bad), 2)
    # a2c.py still refuses a Categorical policy with its words, and now names the classes that take it
    for f in (lambda: A2CUpdate(cat, tf, ro), lambda: a2c_update(cat, tf, ro, fused=True), lambda: GraphedA2C(cat, tf, ro)):
        with pytest.raises(ValueError, match="Categorical A2C call is a follow-up.*A2CUpdateDiscrete"):
            f()
    assert "A2CUpdateDiscrete" in a2c.__doc__ and "A2CUpdateDiscrete" in a2c.A2CUpdate.__doc__


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("fused", (None, False))
def test_autograd_path_is_a2c_update_s_bit_for_bit(kind, fused):
    """a2c_update_discrete(fused=None / False) on CPU tensors: parameters, optimizer state and figures after
    two calls are bitwise a2c_update(fused=False)'s, and the figures are a2c_discrete_ref's."""
    from rl_rocket_amd.a2c import a2c_update
    from rl_rocket_amd.a2c_discrete import a2c_update_discrete

    pol0, obs, act, adv, ret = A.sweep_cpu(4)
    data = [t[:96].contiguous() for t in (obs, act, adv, ret)]
    nan = torch.full((96,), float("nan"))
    out = []
    for f, extra in ((a2c_update_discrete, dict(fused=fused)), (a2c_update, dict(fused=False))):
        pol = copy.deepcopy(pol0)
        opt = A.make_optimizer(kind, pol, 1e-2, capturable=False)
        ro = A.rollout(*data, log_probs=nan)
        figs = []
        for max_norm in (0.5, None):
            before = copy.deepcopy(pol)
            figs.append(f(pol, opt, ro, True, ent_coef=0.01, vf_coef=0.25, max_grad_norm=max_norm, **extra))
            _, st64 = A.reference(before, *data, torch.arange(96), torch.float64, True, 0.01, 0.25)
            for name, r in zip(A.STATS, st64):
                assert figs[-1][name] == pytest.approx(r, rel=1e-4, abs=1e-5), name
        state = [v for p in pol.parameters() for _, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
        out.append((list(pol.parameters()) + state, figs))
    (ta, fa), (tb, fb) = out
    assert fa == fb and len(ta) == len(tb)
    for x, y in zip(ta, tb):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, y) for x, y in zip(pol0.parameters(), ta))
