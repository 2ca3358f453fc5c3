"""rr_ppo_update_opts's host side (no GPU): the C declarations and their ctypes mirrors, the
refusals that come before any HIP call, the Python refusals of rollout.py, the log-mean function on
hand-written control blocks, the translation unit of its own, and the input conditions of
tests/test_gpu_ppo_opts.py (ppo_opts_ref): the value-clip margins, the fp32-vs-fp64 value gap that
justifies them, and the KL-stop thresholds' distance from every evaluated approx_kl."""
import ctypes
import math
import os
import re
import subprocess
import types

import pytest
import torch

import ppo_opts_ref as R
import ppo_ref as P
from rl_rocket_amd import _lib
from rl_rocket_amd import build as B


def test_header_declares_the_entry_point_and_signatures_mirror_it():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14  # a pure addition
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    new = re.search(r"int\s+rr_ppo_update_opts\s*\(([^;]*)\)\s*;", code)
    old = re.search(r"int\s+rr_ppo_update\s*\(([^;]*)\)\s*;", code)
    args = [" ".join(a.split()) for a in new.group(1).split(",")]
    oargs = [" ".join(a.split()) for a in old.group(1).split(",")]
    # rr_ppo_update's arguments with old_values after returns and options, control ahead of stats
    added = ["const float* old_values", "const rr_ppo_options* options", "float* control"]
    assert [a for a in args if a not in added] == oargs and [a for a in args if a in added] == added
    assert args[args.index("const float* returns") + 1] == added[0] and args[args.index("float* stats") - 2:][:2] == added[1:]
    res, argtypes = _lib.SIGNATURES["rr_ppo_update_opts"]
    ores, oargtypes = _lib.SIGNATURES["rr_ppo_update"]
    assert res is ores is ctypes.c_int and len(argtypes) == len(args) == len(oargtypes) + 3
    assert argtypes[args.index(added[1])] == ctypes.POINTER(_lib.RrPpoOptions)
    assert [t for k, t in enumerate(argtypes) if args[k] not in added] == oargtypes
    assert _lib.SIGNATURES["rr_ppo_update_opts_workspace_size"] == _lib.SIGNATURES["rr_ppo_update_workspace_size"]
    body = re.search(r"typedef\s+struct\s+rr_ppo_options\s*\{(.*?)\}\s*rr_ppo_options\s*;", code, re.S).group(1)
    assert re.findall(r"(?:float|int32_t)\s+(\w+)\s*;", body) == [f[0] for f in _lib.RrPpoOptions._fields_]
    assert ctypes.sizeof(_lib.RrPpoOptions) == 16
    enum = re.findall(r"\b(RR_PPO_CTL_[A-Z_]+)\b", code[code.index("RR_PPO_CTL_STOP = 0"):code.index("RR_PPO_CTL_SLOTS")])
    assert len(enum) == 12 and [getattr(_lib, k) for k in enum] == list(range(12))
    assert re.search(r"RR_PPO_CTL_SLOTS\s*=\s*16\b", code) and _lib.RR_PPO_CTL_SLOTS == 16
    assert re.search(r"#define\s+RR_PPO_EPOCH_START\s+0x2u", code) and _lib.RR_PPO_EPOCH_START == 2
    assert re.search(r"#define\s+RR_PPO_CHAINED\s+0x1u", code) and _lib.RR_PPO_CHAINED == 1


def test_library_exports_the_symbols_and_keeps_the_launcher_hidden():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("rr_ppo_update_opts", "rr_ppo_update_opts_workspace_size", "rr_ppo_update"):
        assert re.search(r"\bT %s\b" % name, out)
    assert not re.search(r"rrc_launch_learner_opts", out)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for ns, na, bs in ((14, 3, 65536), (7, 2, 33)):
        assert lib.rr_ppo_update_workspace_size(ns, na, bs, ctypes.byref(a)) == _lib.RR_OK
        assert lib.rr_ppo_update_opts_workspace_size(ns, na, bs, ctypes.byref(b)) == _lib.RR_OK
        assert b.value == a.value + 32 and b.value % 16 == 0
    assert lib.rr_ppo_update_opts_workspace_size(5, 2, 64, ctypes.byref(b)) == _lib.RR_EINVAL
    assert lib.rr_ppo_update_opts_workspace_size(14, 3, 1, ctypes.byref(b)) == _lib.RR_EINVAL


def test_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    V = ctypes.c_void_p
    fake = (V * 13)(*[0x100000 + 0x1000 * k for k in range(13)])  # host arrays of never-read device addresses
    p = V(0x70000)
    nbytes = ctypes.c_int64()
    assert lib.rr_ppo_update_opts_workspace_size(14, 3, 4096, ctypes.byref(nbytes)) == _lib.RR_OK
    nan = float("nan")

    def call(opt=(0.0, 0.0, 1, 0), old_values=p, control=V(0x90000), flags=0, clip=0.2, params=fake, stats=p,
             ws=V(0x200000), ws_bytes=None, next_batch=0, next_idx=None, obs_dim=14):
        o = _lib.RrPpoOptions(*opt) if opt is not None else None
        return lib.rr_ppo_update_opts(obs_dim, 3, params, fake, fake, fake, fake, p, p, p, p, p, old_values, p, 4096,
                                      next_idx, next_batch, clip, 0.01, 0.5, 0.5, p, 0.9, 0.999, 1e-5,
                                      None if o is None else ctypes.byref(o), control, stats, flags, ws,
                                      nbytes.value if ws_bytes is None else ws_bytes, None)

    def refused(rc, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(b"rr_ppo_update_opts") and word in msg, msg

    for bad in (nan, -0.1):
        refused(call(clip=bad), b"clip_range")
        refused(call(opt=(bad, 0.0, 1, 0)), b"clip_range_vf")
        refused(call(opt=(0.0, bad, 1, 0)), b"target_kl")
    refused(call(opt=(0.2, 0.0, 1, 0), old_values=None), b"old_values")
    refused(call(opt=(0.0, 0.01, 1, 0), control=None), b"control")
    refused(call(opt=(0.0, 0.0, 1, 1), control=None), b"control")
    refused(call(control=V(0x90004)), b"16-B")
    refused(call(flags=0x4), b"flag")
    refused(call(flags=0x80000001), b"flag")
    refused(call(opt=None), b"options")
    # what rr_ppo_update refuses
    refused(call(params=None), b"null")
    refused(call(ws=V(0x200008)), b"16-B")
    refused(call(ws_bytes=nbytes.value - 32), b"workspace")  # rr_ppo_update's size is not enough
    refused(call(next_idx=p, next_batch=5000), b"next_batch")
    refused(call(next_idx=p, next_batch=1), b"next_batch")
    refused(call(obs_dim=5), b"obs_dim")
    holes = (V * 13)(*[0x100000 + 0x1000 * k if k != 7 else 0 for k in range(13)])
    refused(call(params=holes), b"null")
    # rr_ppo_update keeps its own prefix and its own flag set
    assert lib.rr_ppo_update(14, 3, fake, fake, fake, fake, fake, p, p, p, p, p, p, 4096, None, 0, 0.2, 0.01, 0.5, 0.5, p,
                             0.9, 0.999, 1e-5, p, _lib.RR_PPO_EPOCH_START, V(0x200000), nbytes.value, None) == _lib.RR_EINVAL
    assert lib.rr_last_error() == b"rr_ppo_update: unknown flag bits"


def _cpu_setup(n=64, capturable=True):
    pol, ro, _ = P.setup_cpu(14, 3, n, seed=3)
    ro = R.with_values(ro, torch.zeros(n))
    return pol, ro, torch.optim.Adam(pol.parameters(), lr=1e-3, capturable=capturable)


def test_python_refusals():
    from rl_rocket_amd.rollout import GraphedPPOUpdate, _ppo_options, ppo_update

    group = object()  # never used: the refusals come first
    pol, ro, opt = _cpu_setup()
    for kw in (dict(clip_range_vf=0.2), dict(normalize_advantage=False), dict(target_kl=0.01)):
        if "target_kl" not in kw:  # with a group target_kl is refused on every path (below)
            with pytest.raises(ValueError, match="fused=True takes"):  # the split path
                ppo_update(pol, opt, ro, n_epochs=1, batch_size=32, fused=True, group=group, **kw)
        with pytest.raises(ValueError, match="fused=True takes"):  # no capturable CUDA Adam
            ppo_update(pol, torch.optim.SGD(pol.parameters(), lr=0.1), ro, n_epochs=1, batch_size=32, fused=True, **kw)
    for fused in (False, True):
        with pytest.raises(ValueError, match="target_kl with a group"):
            ppo_update(pol, opt, ro, n_epochs=1, batch_size=32, fused=fused, group=group, target_kl=0.01)
    with pytest.raises(ValueError, match="target_kl with a group"):
        GraphedPPOUpdate(pol, opt, ro, batch_size=32, group=group, target_kl=0.01)
    with pytest.raises(ValueError, match="target_kl"):  # a break cannot be captured
        GraphedPPOUpdate(pol, opt, ro, batch_size=32, fused=False, target_kl=0.01)
    with pytest.raises(ValueError, match="train_stats"):
        GraphedPPOUpdate(pol, opt, ro, batch_size=32, fused=False, train_stats=True)
    for name in ("clip_range_vf", "target_kl"):
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                _ppo_options(**{"clip_range_vf": None, "normalize_advantage": True, "target_kl": None, name: bad})
            with pytest.raises(ValueError, match=name):
                ppo_update(pol, opt, ro, n_epochs=1, batch_size=32, **{name: bad})
    assert _ppo_options(None, True, None) == (0.0, True, 0.0) and _ppo_options(0.3, 0, 0.02) == (0.3, False, 0.02)


def test_autograd_ppo_update_takes_the_options_on_the_cpu():
    """The PyTorch path on CPU tensors against ppo_opts_ref.train_ref: the options change the result,
    target_kl stops where the float64 loop stops and leaves the parameters of the last step taken."""
    from rl_rocket_amd.rollout import _policy_tensors, ppo_update

    n, bs = 96, 32
    pol0, ro0, _ = P.setup_cpu(14, 3, n, seed=8)
    ro0 = R.with_values(ro0, ro0.returns.reshape(n) + 0.3 * torch.randn(n, generator=torch.Generator().manual_seed(1)))
    perms = []
    with torch.random.fork_rng(devices=[]):  # the draws ppo_update will make
        torch.manual_seed(5)
        perms = [torch.randperm(n) for _ in range(3)]
    free = R.train_ref(pol0, ro0, perms, (bs,) * 3, eps=1e-5, clip_range_vf=0.2, normalize_advantage=False)
    target = (free.kls[3] * free.kls[4]) ** 0.5 / 1.5
    assert free.kls[4] > 1.2 * max(free.kls[:4])
    ref = R.train_ref(pol0, ro0, perms, (bs,) * 3, target_kl=target, eps=1e-5, clip_range_vf=0.2,
                      normalize_advantage=False)
    assert (ref.steps, ref.evals, ref.stop_epoch) == (4, 5, 1)
    import copy
    pol = copy.deepcopy(pol0)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3, eps=1e-5)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        st = ppo_update(pol, opt, ro0, n_epochs=3, batch_size=bs, clip_range_vf=0.2, normalize_advantage=False,
                        target_kl=target)
    assert int(opt.state[pol.log_std]["step"]) == 4
    for t, r in zip(_policy_tensors(pol), ref.params):
        assert (t.detach().double() - r).abs().max().item() <= 2e-5 * max(1.0, r.abs().max().item())
    assert set(st) == {"policy_loss", "value_loss", "entropy"}


def test_train_stats_of_hand_written_blocks():
    from rl_rocket_amd.rollout import _train_stats

    c = [0.0] * 16
    c[_lib.RR_PPO_CTL_STEPS], c[_lib.RR_PPO_CTL_EVALS], c[_lib.RR_PPO_CTL_EPOCHS] = 6.0, 6.0, 2.0
    c[_lib.RR_PPO_CTL_SUM_POLICY], c[_lib.RR_PPO_CTL_SUM_VALUE] = -0.6, 12.0
    c[_lib.RR_PPO_CTL_SUM_ENTROPY], c[_lib.RR_PPO_CTL_SUM_CLIP] = 25.5, 0.3
    c[_lib.RR_PPO_CTL_KL_SUM], c[_lib.RR_PPO_CTL_KL_COUNT] = 0.03, 3.0
    d = _train_stats(c)
    assert d == {"train/policy_gradient_loss": pytest.approx(-0.1), "train/value_loss": 2.0,
                 "train/entropy_loss": -4.25, "train/clip_fraction": pytest.approx(0.05),
                 "train/approx_kl": pytest.approx(0.01), "train/n_minibatches": 6, "train/n_evaluated": 6,
                 "train/early_stop": False, "train/stop_epoch": None}
    c[_lib.RR_PPO_CTL_STOP] = c[_lib.RR_PPO_CTL_DECIDE] = 1.0
    c[_lib.RR_PPO_CTL_EVALS], c[_lib.RR_PPO_CTL_KL_COUNT] = 7.0, 1.0
    d = _train_stats(c)
    assert d["train/early_stop"] is True and d["train/stop_epoch"] == 1 and d["train/n_minibatches"] == 6
    assert d["train/n_evaluated"] == 7 and d["train/approx_kl"] == pytest.approx(0.03)
    z = _train_stats([0.0] * 16)  # a cleared block: nothing evaluated, no division by zero
    assert z["train/n_minibatches"] == 0 and z["train/value_loss"] == 0.0 and not math.isnan(z["train/approx_kl"])


def test_build_compiles_the_translation_unit_of_its_own():
    src = B.SRC_PPO_OPTS
    csrc = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc")
    assert os.path.dirname(src) == os.path.join(csrc, "ppo_opts") and os.path.isfile(src)
    assert src in B.sources() and B.sources() == sorted(B.sources())
    cmds = B.commands()
    mine = [c for c in cmds if src in c]
    assert mine == [cmds[-1]] and "-shared" in mine[0]  # compiled in the linking step, a module of its own
    for flag in B.COLLECT_FLAGS:  # the learner's code-generation setting
        assert flag in mine[0]
    assert not any(f in mine[0] for f in B.EXACT_FLAGS if f != "-mllvm")
    assert os.listdir(os.path.dirname(src)) == ["rocket_ppo_opts.hip"]
    text = open(src).read()
    assert text.index("#define RR_POL_PREFETCH_A 1") < text.index('#include "rocket_policy.inc"')
    for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, flags=re.M):
        assert os.path.join(csrc, inc) in B.sources() and not inc.endswith(".hip"), inc


def test_new_kernels_use_no_scratch_and_the_learner_kernels_are_all_there():
    """From the built library: the new instantiations use no scratch (private_segment_fixed_size,
    bytes 4..8 of the kernel descriptor) and rr_ppo_update's own kernels are still beside them."""
    import struct
    import tempfile

    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    kd = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([B._llvm("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, B.OUT, os.path.join(d, "x")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for k, k0 in enumerate(starts):
            part, co = os.path.join(d, "b%d.bin" % k), os.path.join(d, "b%d.co" % k)
            with open(part, "wb") as f:
                f.write(blob[k0:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            subprocess.check_call([B._llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                                   "--targets=hipv4-amdgcn-amd-amdhsa--%s" % B.ARCH, "--output=" + co])
            kd.update({n: v for n, v in B._elf_symbols(open(co, "rb").read()).items() if n.endswith(".kd")})
    new = {n: v for n, v in kd.items() if "ppo_opts_" in n}
    # 2 shapes x (prep, finish, adam, 4 gradient variants)
    assert len(new) == 14 and sum("ppo_opts_grad_kernel" in n for n in new) == 8
    for n, v in new.items():
        assert struct.unpack_from("<I", v, 4)[0] == 0, n
    for name in ("ppo_prep_kernel", "ppo_grad_kernel", "ppo_finish_kernel", "adam_chain_kernel"):
        assert sum(name + "IL" in n for n in kd) == 2, name


def test_committed_isa_comparison_covers_every_kernel_of_the_parent():
    import json

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "ppo_opts", "isa_before_after.json")) as f:
        rec = json.load(f)
    assert rec["kernels_in_parent"] == len(rec["before"]) > 100
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert sorted(rec["added"]) == sorted(k for k in rec["after"] if k not in rec["before"])
    assert len(rec["added"]) == 14 and all("ppo_opts_" in k for k in rec["added"])


# ---- the input conditions of tests/test_gpu_ppo_opts.py ----

@pytest.mark.parametrize("ns,na,bs", R.VCLIP_SHAPES)
@pytest.mark.parametrize("kind", R.VCLIP_KINDS)
def test_value_clip_inputs_keep_the_margin(kind, ns, na, bs):
    c = R.vclip_case(kind, ns, na, bs)
    dist, outside = R.vclip_distance(c)
    assert dist.min().item() >= P.MARGIN, (kind, dist.min().item())
    want = {"inside": (0.0, 0.0), "outside": (1.0, 1.0), "mixed": (0.25, 0.75), "half": (0.4, 0.6)}[kind]
    assert want[0] <= outside <= want[1], (kind, outside)
    assert c.c > 10 * P.BUILD_MARGIN
    # MARGIN is >= 25 x the gap between the fp32 and the fp64 forward's V on these inputs (how
    # ppo_ref justifies it for log-probs)
    gap = (R.values(c.pol, c.ro, c.idx, torch.float32) - R.values(c.pol, c.ro, c.idx, torch.float64)).abs().max().item()
    print("%s (%d,%d) bs=%d: min distance %.2e, outside %.3f, fp32-fp64 V gap %.2e" % (kind, ns, na, bs, dist.min().item(),
                                                                                      outside, gap))
    assert P.MARGIN >= 25 * gap, gap
    r, _ = P.ratios64(c.pol, c.ro, c.idx)  # the pi side: what clip_fraction's exact comparison needs
    for edge in (0.8, 1.0, 1.2):
        assert (r - edge).abs().min().item() >= P.MARGIN, edge
    assert 0.1 < ((r - 1).abs() > 0.2).double().mean().item() < 0.9


def test_raw_advantage_inputs_are_the_offset_case():
    for ns, na, bs in R.VCLIP_SHAPES:  # the shapes of the gradient tests
        c = P.edge_case("offset_adv", bs, ns, na)
        adv = c.ro.advantages.view(-1)[c.idx]
        assert 49.0 < adv.mean().item() < 51.0 and 0.3 < adv.std().item() < 0.7 and adv.min().item() > 40.0
        r, _ = P.ratios64(c.pol, c.ro, c.idx)
        for edge in (0.8, 1.0, 1.2):  # raw advantages of one sign: the ratio's margins are what clip_fraction needs
            assert (r - edge).abs().min().item() >= P.MARGIN


@pytest.mark.parametrize("name", list(R.KL_PLACES))
def test_kl_stop_inputs(name):
    c = R.kl_case(name)
    limit = 1.5 * c.target_kl
    print(name, "place", c.place, "target_kl %.3e" % c.target_kl, "approx_kl", ["%.3e" % k for k in c.ref.kls])
    for k in c.ref.kls:  # every evaluated minibatch
        assert abs(k - limit) >= max(R.KL_GAP * limit, R.KL_FLOOR), (k, limit)
    n_mb = len(c.sizes)
    if c.place is None:
        assert c.ref.stop_epoch is None and c.ref.steps == c.ref.evals == n_mb * R.KL_EPOCHS
    else:
        assert c.ref.evals == c.place + 1 and c.ref.steps == c.place and c.ref.stop_epoch == c.place // n_mb
        assert c.ref.kls == c.free.kls[:c.place + 1]
    if name == "first":
        assert c.ref.steps == 0 and c.ref.stop_epoch == 0
    if name == "mid_epoch":
        assert c.place % n_mb != 0 and c.ref.stop_epoch >= 1
    if name == "epoch_start":
        assert c.place % n_mb == 0 and c.ref.stop_epoch >= 1
    # the last epoch's mean is over its evaluated minibatches only
    last = c.ref.kls[c.ref.stop_epoch * n_mb:] if c.place is not None else c.ref.kls[-n_mb:]
    assert c.ref.log["train/approx_kl"] == pytest.approx(sum(last) / len(last), rel=1e-12)
    # sums that never restarted at an epoch's first minibatch are far outside the GPU test's bar on
    # RR_PPO_CTL_KL_SUM (1e-5 relative + KL_FLOOR per minibatch), and the count differs
    if c.ref.evals > n_mb:
        assert sum(c.ref.kls) - sum(last) > 1.5 * (1e-5 * sum(c.ref.kls) + len(last) * R.KL_FLOOR)
    if name == "moved_never":  # here the statistics bar itself tells the two means apart
        whole = sum(c.ref.kls) / len(c.ref.kls)
        assert abs(whole - sum(last) / len(last)) > 100 * (1e-5 * whole + 1e-6) and min(c.ref.kls) > 1e-3
    assert isinstance(c.ro, types.SimpleNamespace)
