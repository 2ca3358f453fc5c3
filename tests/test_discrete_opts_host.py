"""rr_ppo_update_discrete_opts's host side (no GPU): the C declarations and their ctypes mirrors, the
refusals that come before any HIP call, the Python refusals and bindings of learner.py on stub batches,
the translation unit of its own, and the input conditions of tests/test_gpu_discrete_opts.py
(discrete_opts_ref): every case is admissible by the float64 reference alone."""
import ctypes
import json
import os
import re
import struct
import subprocess
import types

import pytest
import torch

import bc_host_common as C
import discrete_opts_ref as Q
import discrete_ref as D
import ppo_ref as P
from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point_and_signatures_mirror_it():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14  # a pure addition
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def args_of(name):
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    args, oargs = args_of("rr_ppo_update_discrete_opts"), args_of("rr_ppo_update_discrete")
    # rr_ppo_update_discrete's arguments with old_values after returns and options, control ahead of stats
    added = ["const float* old_values", "const rr_ppo_options* options", "float* control"]
    assert [a for a in args if a not in added] == oargs and [a for a in args if a in added] == added
    assert args[args.index("const float* returns") + 1] == added[0] and args[args.index("float* stats") - 2:][:2] == added[1:]
    # the same extension as rr_ppo_update -> rr_ppo_update_opts, with n_choices for act_dim
    assert args == [a if a != "int act_dim" else "int n_choices" for a in args_of("rr_ppo_update_opts")]
    assert _lib.SIGNATURES["rr_ppo_update_discrete_opts"] == _lib.SIGNATURES["rr_ppo_update_opts"]
    assert len(_lib.SIGNATURES["rr_ppo_update_discrete_opts"][1]) == len(args)
    assert (_lib.SIGNATURES["rr_ppo_update_discrete_opts_workspace_size"]
            == _lib.SIGNATURES["rr_ppo_update_discrete_workspace_size"])
    assert args_of("rr_ppo_update_discrete_opts_workspace_size") == args_of("rr_ppo_update_discrete_workspace_size")
    comment = text[text.index("rr_ppo_update_opts for this policy"):text.index("int rr_ppo_update_discrete_opts_workspace_size")]
    for word in ("bitwise", "RR_PPO_EPOCH_START", "RR_PPO_CTL_STOP", "16-B aligned", "NULL options"):
        assert word in comment, word


def test_library_exports_the_symbols_and_keeps_the_launcher_hidden():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in ("rr_ppo_update_discrete_opts", "rr_ppo_update_discrete_opts_workspace_size", "rr_ppo_update_discrete"):
        assert re.search(r"\bT %s\b" % name, out)
    assert not re.search(r"rrc_launch_discrete_opts", out)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for k, bs in ((4, 65536), (2, 33), (3, 2)):
        assert lib.rr_ppo_update_discrete_workspace_size(7, k, bs, ctypes.byref(a)) == _lib.RR_OK
        assert lib.rr_ppo_update_discrete_opts_workspace_size(7, k, bs, ctypes.byref(b)) == _lib.RR_OK
        assert b.value == a.value + 32 and b.value % 16 == 0
    who = b"rr_ppo_update_discrete_opts_workspace_size: "
    for shape, text in (((14, 4), C.CAT_OBS), ((7, 5), C.CAT_K), ((7, 1), C.CAT_K)):
        assert lib.rr_ppo_update_discrete_opts_workspace_size(*shape, 64, ctypes.byref(b)) == _lib.RR_EINVAL
        assert lib.rr_last_error() == who + text.encode()
    assert lib.rr_ppo_update_discrete_opts_workspace_size(7, 4, 1, ctypes.byref(b)) == _lib.RR_EINVAL
    assert lib.rr_ppo_update_discrete_opts_workspace_size(7, 4, 64, None) == _lib.RR_EINVAL


def test_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    V = ctypes.c_void_p
    fake = (V * 12)(*[0x100000 + 0x1000 * k for k in range(12)])  # host arrays of never-read device addresses
    p = V(0x70000)
    nbytes = ctypes.c_int64()
    assert lib.rr_ppo_update_discrete_opts_workspace_size(7, 4, 4096, ctypes.byref(nbytes)) == _lib.RR_OK
    nan = float("nan")

    def call(opt=(0.0, 0.0, 1, 0), old_values=p, control=V(0x90000), flags=0, clip=0.2, params=fake, stats=p,
             ws=V(0x200000), ws_bytes=None, next_batch=0, next_idx=None, obs_dim=7, k=4, batch=4096, obs=p, lr=p):
        o = _lib.RrPpoOptions(*opt) if opt is not None else None
        return lib.rr_ppo_update_discrete_opts(obs_dim, k, params, fake, fake, fake, fake, obs, p, p, p, p, old_values, p,
                                               batch, next_idx, next_batch, clip, 0.01, 0.5, 0.5, lr, 0.9, 0.999, 1e-5,
                                               None if o is None else ctypes.byref(o), control, stats, flags, ws,
                                               nbytes.value if ws_bytes is None else ws_bytes, None)

    def refused(rc, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(b"rr_ppo_update_discrete_opts: ") and word in msg, msg

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
    # what rr_ppo_update_discrete refuses
    refused(call(obs_dim=14), b"obs_dim")
    for k in (1, 5):
        refused(call(k=k), b"n_choices")
    for bs in (1, 0, -5):
        refused(call(batch=bs), b"batch")
    refused(call(params=None), b"null")
    refused(call(obs=None), b"null")
    refused(call(lr=None), b"null")
    refused(call(ws=None), b"null")
    refused(call(ws=V(0x200008)), b"16-B")
    refused(call(ws_bytes=nbytes.value - 32), b"workspace")  # rr_ppo_update_discrete's size is not enough
    refused(call(batch=8192), b"workspace")  # sized for 4096 rows
    refused(call(next_idx=p, next_batch=5000), b"next_batch")
    refused(call(next_idx=p, next_batch=1), b"next_batch")
    for hole in (0, 8, 9, 11):
        holes = (V * 12)(*[0x100000 + 0x1000 * k if k != hole else 0 for k in range(12)])
        refused(call(params=holes), b"null")
    # the call without options keeps its own prefix and its own flag set
    assert lib.rr_ppo_update_discrete(7, 4, fake, fake, fake, fake, fake, p, p, p, p, p, p, 4096, None, 0, 0.2, 0.01, 0.5,
                                      0.5, p, 0.9, 0.999, 1e-5, p, _lib.RR_PPO_EPOCH_START, V(0x200000), nbytes.value,
                                      None) == _lib.RR_EINVAL
    assert lib.rr_last_error() == b"rr_ppo_update_discrete: unknown flag bits"


def _stub_ro(n=64):
    env = types.SimpleNamespace(num_envs=n, state_dim=7, action_dim=2)
    return types.SimpleNamespace(n_steps=1, env=env)


def test_python_refusals_on_stub_batches():
    """With fused=True and a Categorical policy: group= is refused naming it; an optimizer that is no
    capturable CUDA Adam is refused naming the option that asked (or `another optimizer`); target_kl with a
    group is refused everywhere. All before anything touches a device: the rollout is a stub."""
    from rl_rocket_amd.rollout import GraphedPPOUpdate, MlpCategoricalActorCritic, PPOUpdateDiscrete, ppo_update

    pol = MlpCategoricalActorCritic(7, 4)
    ro, group = _stub_ro(), object()
    options = ((dict(clip_range_vf=0.2), "clip_range_vf"), (dict(normalize_advantage=False), "normalize_advantage"),
               (dict(target_kl=0.01), "target_kl"))
    cpu_adam = torch.optim.Adam(pol.parameters(), lr=1e-3, capturable=True)  # capturable, but not on a device
    for opt in (torch.optim.Adam(pol.parameters(), lr=1e-3), torch.optim.SGD(pol.parameters(), lr=0.1), cpu_adam):
        for kw, word in options:
            with pytest.raises(ValueError, match=word):
                ppo_update(pol, opt, ro, fused=True, **kw)
        with pytest.raises(ValueError, match="another optimizer"):
            ppo_update(pol, opt, ro, fused=True)
    for kw, word in options + ((dict(train_stats=True), "train_stats"),):
        with pytest.raises(ValueError, match=word):
            GraphedPPOUpdate(pol, cpu_adam, ro, batch_size=8, fused=True, **kw)
        with pytest.raises(ValueError, match="group="):
            GraphedPPOUpdate(pol, cpu_adam, ro, batch_size=8, fused=True, group=group, **kw)
    with pytest.raises(ValueError, match="another optimizer"):
        GraphedPPOUpdate(pol, cpu_adam, ro, batch_size=8, fused=True)
    for kw, _ in options[:2] + ((dict(), ""),):
        with pytest.raises(ValueError, match="group="):
            ppo_update(pol, cpu_adam, ro, fused=True, group=group, **kw)
    with pytest.raises(ValueError, match="group="):  # the Categorical refusal comes first with fused=True
        ppo_update(pol, cpu_adam, ro, fused=True, group=group, target_kl=0.01)
    with pytest.raises(ValueError, match="target_kl with a group"):
        ppo_update(pol, cpu_adam, ro, fused=False, group=group, target_kl=0.01)
    with pytest.raises(ValueError, match="target_kl with a group"):
        GraphedPPOUpdate(pol, cpu_adam, ro, batch_size=8, fused=False, group=group, target_kl=0.01)
    # the constructor: bad option values are refused by name, and the optimizer before any rollout tensor is read
    for name in ("clip_range_vf", "target_kl"):
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                PPOUpdateDiscrete(pol, cpu_adam, ro, 8, **{name: bad})
    with pytest.raises(ValueError, match="capturable"):
        PPOUpdateDiscrete(pol, cpu_adam, ro, 8, clip_range_vf=0.2, train_stats=True)


def test_constructor_keywords_and_defaults():
    """PPOUpdateDiscrete gained PPOUpdate's four keywords with the defaults of today."""
    import inspect

    from rl_rocket_amd.rollout import PPOUpdate, PPOUpdateDiscrete

    a, b = inspect.signature(PPOUpdate.__init__).parameters, inspect.signature(PPOUpdateDiscrete.__init__).parameters
    assert list(a) == list(b)
    for name, default in (("clip_range_vf", None), ("normalize_advantage", True), ("target_kl", None), ("train_stats", False)):
        assert b[name].default is default and a[name].default is default


def test_build_compiles_the_translation_unit_of_its_own():
    src = B.SRC_DISCRETE_OPTS
    csrc = C.CSRC
    assert os.path.dirname(src) == os.path.join(csrc, "discrete_opts") and os.path.isfile(src)
    assert os.listdir(os.path.dirname(src)) == ["rocket_ppo_discrete_opts.hip"]
    assert src in B.sources() and B.sources() == sorted(B.sources())
    cmds = B.commands()
    assert len(cmds) == 6
    mine = [c for c in cmds if src in c]
    assert mine == [cmds[-1]] and "-shared" in mine[0]  # compiled in the linking step, a module of its own
    assert mine[0].index(B.SRC_ROLLOUT_DISCRETE) < mine[0].index(src) < mine[0].index(B.SRC_COLLECT_STATS)
    for flag in B.COLLECT_FLAGS:  # the learner's code-generation setting
        assert flag in mine[0]
    assert not any(f in mine[0] for f in B.EXACT_FLAGS if f != "-mllvm")
    text = open(src).read()
    assert text.index("#define RR_POL_PREFETCH_A 1") < text.index('#include "rocket_policy.inc"')
    incs = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, flags=re.M)
    assert incs == ["rocket_device.h", "rocket_policy.inc", "rocket_ppo.inc", "rocket_ppo_finish_body.inc",
                    "rocket_ppo_adam_body.inc"]  # the learner's bodies, not copies of them
    for inc in incs:
        assert os.path.join(csrc, inc) in B.sources() and not inc.endswith(".hip"), inc
    assert "ppo_grad_tower<OBS, ACT, 0, false, NORM, 2>" in text and "ppo_grad_tower<OBS, ACT, 1, VCLIP, true>" in text
    assert text.count("__global__") == 4 and "__builtin_amdgcn_mfma" not in text


def test_new_kernels_use_no_scratch_and_the_discrete_learner_kernels_are_all_there():
    """From the built library: the seven new instantiations use no scratch (private_segment_fixed_size,
    bytes 4..8 of the kernel descriptor) and rr_ppo_update_discrete's own kernels are still beside them."""
    kd = C.kernel_descriptors()
    new = {n: v for n, v in kd.items() if "dopts_" in n}
    for name in ("dopts_prep_kernel", "dopts_finish_kernel", "dopts_adam_kernel"):
        assert sum(name + "ILi7ELi4E" in n for n in new) == 1, name
    assert sum("dopts_grad_kernelILi7ELi4ELb" in n for n in new) == 4 and len(new) == 7
    for n, v in new.items():
        assert struct.unpack_from("<I", v, 4)[0] == 0, n
    for name in ("discrete_prep_kernel", "discrete_grad_kernel", "discrete_finish_kernel", "discrete_adam_kernel"):
        assert sum(name + "ILi7ELi4E" in n for n in kd) == 1, name


def test_committed_isa_comparison_covers_every_kernel_of_the_parent():
    with open(os.path.join(ROOT, "profiles", "discrete_opts", "isa_before_after.json")) as f:
        rec = json.load(f)
    with open(os.path.join(ROOT, "profiles", "rollout_discrete", "isa_before_after.json")) as f:
        parent = json.load(f)["after"]
    assert rec["kernels_in_parent"] == len(rec["before"]) == len(parent) == 185 and rec["changed"] == 0
    assert rec["before"] == parent and rec["removed"] == []  # the parent's own record: every kernel, each hash
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert sorted(rec["added"]) == sorted(k for k in rec["after"] if k not in rec["before"])
    assert len(rec["added"]) == 7 and all("::dopts_" in k for k in rec["added"])


def test_committed_measurement_has_the_five_legs():
    with open(os.path.join(ROOT, "profiles", "discrete_opts", "discrete_opts_bench.json")) as f:
        rec = json.load(f)
    assert (rec["batch"], rec["n_choices"], rec["model"]) == (65536, 4, "3DOF") and rec["runs"] >= 7
    for leg in ("discrete", "opts_off", "opts_on", "stopped", "autograd"):
        us = rec[leg]["us"]
        assert len(us) == rec["runs"] and min(us) <= rec[leg]["median"] <= max(us)
        assert rec[leg]["spread"] == pytest.approx(max(us) - min(us))
    assert rec["parameters_finite_after"] is True and rec["stopped_leg_left_the_parameters"] is True
    assert rec["opts_off_over_discrete"] == pytest.approx(rec["opts_off"]["median"] / rec["discrete"]["median"])
    assert rec["opts_on_over_discrete"] == pytest.approx(rec["opts_on"]["median"] / rec["discrete"]["median"])
    assert rec["stopped"]["median"] < 0.25 * rec["discrete"]["median"]  # launches that return at entry


# ---- the input conditions of tests/test_gpu_discrete_opts.py ----
# The builders move a float64 ratio to exactly BUILD_MARGIN off an edge, and the old log-prob is then stored
# in fp32: |log-prob| < 16 has an ulp of at most 1e-6, which is what the stored ratio may have lost.
RATIO_MARGIN = P.BUILD_MARGIN - 1e-6


def _ratio_margin(c):
    r = D.ratios64(c.pol, c.ro, c.idx)
    assert float(c.ro.log_probs.reshape(-1)[c.idx].abs().max()) < 16.0
    return min((r - edge).abs().min().item() for edge in (0.8, 1.0, 1.2)), r


@pytest.mark.parametrize("k,bs", Q.VCLIP_SHAPES)
@pytest.mark.parametrize("kind", Q.VCLIP_KINDS)
def test_value_clip_inputs_keep_the_margin(kind, k, bs):
    c = Q.vclip_case(kind, k, bs)
    dist, outside = Q.vclip_distance(c)
    assert dist.min().item() >= P.BUILD_MARGIN, (kind, dist.min().item())
    want = {"inside": (0.0, 0.0), "outside": (1.0, 1.0), "mixed": (0.25, 0.75), "half": (0.4, 0.6)}[kind]
    assert want[0] <= outside <= want[1], (kind, outside)
    assert c.c > 10 * P.BUILD_MARGIN
    # MARGIN is >= 25 x the gap between the fp32 and the fp64 forward's V on these inputs
    gap = (Q.values(c.pol, c.ro, c.idx, torch.float32) - Q.values(c.pol, c.ro, c.idx, torch.float64)).abs().max().item()
    margin, r = _ratio_margin(c)
    print("%s k=%d bs=%d: min distance %.2e, outside %.3f, fp32-fp64 V gap %.2e, ratio margin %.6e"
          % (kind, k, bs, dist.min().item(), outside, gap, margin))
    assert P.MARGIN >= 25 * gap, gap
    assert margin >= RATIO_MARGIN  # the pi side: what clip_fraction's exact comparison needs
    assert 0.1 < ((r - 1).abs() > 0.2).double().mean().item() < 0.9
    ref64, st64 = Q.reference(c.pol, c.ro, c.idx, clip_range_vf=c.c, **c.coef)
    assert len(ref64) == 12 and ref64[8].shape == (k, 64) and ref64[9].shape == (k,)
    vf = [ref64[Q.NAMES.index(n)] for n in Q.VF_NAMES]
    if kind == "outside":  # every sample past the clamp: the float64 vf-side gradients are exactly 0
        assert all(torch.count_nonzero(g).item() == 0 for g in vf)
    else:
        assert max(g.abs().max().item() for g in vf) > 1e-4
    if kind != "inside":  # the clip changes the loss by far more than the statistics' bar
        _, plain = Q.reference(c.pol, c.ro, c.idx, **c.coef)
        assert abs(plain[1] - st64[1]) > 30 * (1e-5 * abs(st64[1]) + 1e-6)


@pytest.mark.parametrize("k,bs", Q.RAW_SHAPES)
@pytest.mark.parametrize("vclip", [False, True])
def test_raw_advantage_inputs_are_the_offset_case(k, bs, vclip):
    c = Q.raw_case(k, bs, vclip)
    adv = c.ro.advantages.view(-1)[c.idx]
    assert 49.0 < adv.mean().item() < 51.0 and 0.3 < adv.std().item() < 0.7 and adv.min().item() > 40.0
    margin, _ = _ratio_margin(c)
    assert margin >= RATIO_MARGIN
    _, raw = Q.reference(c.pol, c.ro, c.idx, clip_range_vf=c.opts.get("clip_range_vf"), normalize_advantage=False, **c.coef)
    _, normed = Q.reference(c.pol, c.ro, c.idx, clip_range_vf=c.opts.get("clip_range_vf"), **c.coef)
    print("k=%d bs=%d vclip=%s: raw policy_loss %.4e, normalised %.4e" % (k, bs, vclip, raw[0], normed[0]))
    assert abs(raw[0]) > 20.0 * abs(normed[0])
    if vclip:
        d = (Q.values(c.pol, c.ro, c.idx, torch.float64) - c.ro.values.reshape(-1)[c.idx].double()).abs()
        assert ((d - 0.2).abs() > 0.09).all() and 0.2 < (d > 0.2).double().mean().item() < 0.8


@pytest.mark.parametrize("name", list(Q.KL_PLACES))
def test_kl_stop_inputs(name):
    c = Q.kl_case(name)
    limit = 1.5 * c.target_kl
    print(name, "place", c.place, "target_kl %.3e" % c.target_kl, "approx_kl", ["%.3e" % k for k in c.ref.kls])
    assert (Q.KL_GAP, Q.KL_FLOOR) == (0.05, 2.4e-7)  # the Gaussian helper's, unchanged
    for k in c.ref.kls:  # every evaluated minibatch
        assert abs(k - limit) >= max(Q.KL_GAP * limit, Q.KL_FLOOR), (k, limit)
    n_mb = len(c.sizes)
    if c.place is None:
        assert c.ref.stop_epoch is None and c.ref.steps == c.ref.evals == n_mb * Q.KL_EPOCHS
    else:
        assert c.ref.evals == c.place + 1 and c.ref.steps == c.place and c.ref.stop_epoch == c.place // n_mb
        assert c.ref.kls == c.free.kls[:c.place + 1]
    if name == "first":
        assert c.ref.steps == 0 and c.ref.stop_epoch == 0
    if name == "mid_epoch":
        assert c.place % n_mb != 0 and c.ref.stop_epoch >= 1
    if name == "epoch_start":
        assert c.place % n_mb == 0 and c.ref.stop_epoch >= 1
    last = c.ref.kls[c.ref.stop_epoch * n_mb:] if c.place is not None else c.ref.kls[-n_mb:]
    assert c.ref.log["train/approx_kl"] == pytest.approx(sum(last) / len(last), rel=1e-12)
    # sums that never restarted at an epoch's first minibatch are far outside the GPU test's bar on
    # RR_PPO_CTL_KL_SUM (1e-5 relative + KL_FLOOR per minibatch)
    if c.ref.evals > n_mb:
        assert sum(c.ref.kls) - sum(last) > 1.5 * (1e-5 * sum(c.ref.kls) + len(last) * Q.KL_FLOOR)
    if name == "moved_never":  # here the statistics bar itself tells the two means apart
        whole = sum(c.ref.kls) / len(c.ref.kls)
        assert abs(whole - sum(last) / len(last)) > 100 * (1e-5 * whole + 1e-6) and min(c.ref.kls) > 1e-3
    # the entropy the control block sums is the state-dependent mean, not a constant of the parameters
    assert abs(c.ref.log["train/entropy_loss"]) > 0.5
