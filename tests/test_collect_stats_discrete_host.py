"""The host side of the Categorical policy's statistics collect, rr_rollout_collect_discrete_stats (no GPU): the
C declaration, its ctypes mirror, the export and the unchanged ABI number; every refusal of the call is reached
with fake pointers before the handle is read; the constructor's messages on stub batches; and the touchdown
states of tests/test_gpu_collect_stats.py::_landing_and_nan stepped once on the CPU oracle with every row of
the three tables, so that what the GPU test's reference must hold is on record before anything runs on a GPU."""
import ctypes
import math
import re
import subprocess
import types

import numpy as np
import pytest

import discrete_ref as D
from rl_rocket_amd import _lib

NAME, TWIN = "rr_rollout_collect_discrete_stats", "rr_rollout_collect_stats"


def test_declared_in_header_with_the_twins_prototype_abi_14():
    with open(_lib.HEADER) as f:
        text = f.read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = {}
    for name in (NAME, TWIN):
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name + " is not declared"
        decl[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    args, twin = decl[NAME], decl[TWIN]
    # rr_rollout_collect_stats's arguments with (n_choices, table) after params
    assert args[:2] == twin[:2] and args[2:4] == ["int n_choices", "const float* table"] and args[4:] == twin[2:]
    assert args[-2] == "const rr_rollout_stats* stats"
    res, argtypes = _lib.SIGNATURES[NAME]
    tres, targtypes = _lib.SIGNATURES[TWIN]
    assert res is ctypes.c_int and len(argtypes) == len(args)
    assert argtypes == targtypes[:2] + [ctypes.c_int, ctypes.c_void_p] + targtypes[2:]


def test_library_exports_it_and_keeps_the_launcher_hidden():
    lib = _lib.load()
    assert lib.rr_abi_version() == 14
    assert getattr(lib, NAME) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT %s\b" % NAME, out)
    assert not re.search(r"rrc_launch_collect_discrete_stats", out)


def test_unit_is_a_source_and_is_linked():
    from rl_rocket_amd import build as B

    assert B.SRC_COLLECT_STATS_DISCRETE in B.sources()
    assert B.SRC_COLLECT_STATS_DISCRETE in B.commands()[-1]
    assert "-amdgpu-mfma-vgpr-form" in B.commands()[-1]  # COLLECT_FLAGS reach the units of the linking call


def test_c_abi_refuses_bad_arguments_before_any_hip_call():
    """Fake pointers throughout and a fake or absent handle: every argument check comes before the handle is
    read, so each refusal is reached without a device, and the handle's own is the last."""
    lib = _lib.load()
    V = ctypes.c_void_p
    fake = V(0x10000)
    table = (ctypes.c_float * 8)(0, -1, -1, 1, 0, 1, 1, 1)

    def stats(**over):
        vals = dict(partials=0x20000, out=0x30000, accum=0x40000)
        vals.update(over)
        return _lib.RrRolloutStats(**vals)

    def refused(rc, word):
        msg = lib.rr_last_error().decode()
        assert rc == _lib.RR_EINVAL and msg.startswith(NAME + ": ") and word in msg, (rc, msg)

    def call(h=None, params=fake, k=4, tab=table, prec=0, bufs=None, it=fake, T=8, adv=fake, ret=fake, st=stats()):
        bufs = bufs or [fake] * 6
        return getattr(lib, NAME)(h, params, k, tab, prec, 1, it, T, 0.99, 0.95, *bufs, adv, ret, None, None, None,
                                  None, fake, fake, None, None, None if st is None else ctypes.byref(st), None)

    # what rr_rollout_collect_discrete refuses
    for prec in (_lib.RR_POLICY_BF16, _lib.RR_POLICY_FP16X3, 7):
        refused(call(prec=prec), "RR_POLICY_FP32")
    refused(call(k=1), "2 .. 4")
    refused(call(k=5), "2 .. 4")
    refused(call(tab=None), "table")
    for bad in (float("nan"), float("inf")):
        t = (ctypes.c_float * 8)(0, -1, -1, 1, 0, bad, 1, 1)
        refused(call(tab=t), "finite")
        refused(call(k=3, tab=t), "finite")
        refused(call(k=2, tab=t), "null handle")  # a row past n_choices is not read
    refused(call(params=None), "params")
    refused(call(params=V(0x10004)), "16-B aligned")
    refused(call(T=0), "n_steps")
    for k in range(6):
        refused(call(bufs=[fake] * k + [None] + [fake] * (5 - k)), "null argument")
    refused(call(it=None), "null argument")
    # what rr_rollout_collect_stats refuses
    refused(call(st=None), "stats")
    refused(call(st=stats(partials=None)), "partials")
    refused(call(st=stats(out=None)), "out")
    refused(call(st=stats(partials=0x20040)), "128-B")
    refused(call(st=stats(out=0x30004)), "8-B")
    refused(call(st=stats(accum=0x40004)), "8-B")
    refused(call(adv=None), "buf_advantage")
    refused(call(ret=None), "buf_advantage")
    refused(call(adv=None, ret=None), "buf_advantage")
    # all of them with a non-null handle that is never read: the same refusals
    refused(call(h=fake, st=None), "stats")
    refused(call(h=fake, k=5), "2 .. 4")
    refused(call(h=fake, adv=None), "buf_advantage")
    # and with everything in order, the handle
    refused(call(), "null handle")
    refused(call(st=stats(accum=None)), "null handle")  # accum is optional


def _stub_batch(dof=3, device="cpu"):
    ns, na = (7, 2) if dof == 3 else (14, 3)
    return types.SimpleNamespace(num_envs=8, state_dim=ns, action_dim=na, device=device, model=dof)


def test_constructor_messages_on_stub_batches():
    """stats=True first asks for a real batch (one with params), before the device and the integrator; then for
    the one-launch collect. Nothing below touches a device."""
    from rl_rocket_amd.rollout import DeviceRollout, MlpCategoricalActorCritic

    pol = MlpCategoricalActorCritic(7, 4)
    for dev in ("cpu", "cuda:0"):
        b = _stub_batch(device=dev)
        for kw in (dict(), dict(one_launch=True), dict(per_step=True), dict(one_launch=True, per_step=True)):
            with pytest.raises(ValueError, match="stats=True.*RocketBatch"):
                DeviceRollout(b, pol, stats=True, **kw)
        with pytest.raises(ValueError, match="6DOF"):
            DeviceRollout(_stub_batch(6, dev), pol, stats=True, one_launch=True)
        with pytest.raises(ValueError, match="policy_dtype='bf16'"):
            DeviceRollout(b, pol, stats=True, one_launch=True, policy_dtype="bf16")
        # a batch with params: the default two-launch collect and the per-step form have no statistics
        real = _stub_batch(device=dev)
        real.params = types.SimpleNamespace(integrator=0, flags=0x3)
        for kw in (dict(), dict(one_launch=False), dict(per_step=True), dict(one_launch=True, per_step=True)):
            with pytest.raises(ValueError, match="stats=True.*one_launch=True"):
                DeviceRollout(real, pol, stats=True, **kw)
    # then the one-launch collect's own conditions, in their order: the device, the integrator
    cpu = _stub_batch()
    cpu.params = types.SimpleNamespace(integrator=0, flags=0x3)
    with pytest.raises(ValueError, match="one_launch=True.*CUDA"):
        DeviceRollout(cpu, pol, stats=True, one_launch=True)
    dop = _stub_batch(device="cuda:0")
    dop.params = types.SimpleNamespace(integrator=2, flags=0x3)
    with pytest.raises(ValueError, match="dopri5"):
        DeviceRollout(dop, pol, stats=True, one_launch=True)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_touchdown_states_on_the_cpu_oracle(oracle_mod, k):
    """The 3DOF row of _landing_and_nan (2 cm above the pad, upright, mid mass) descending at 0.5, 5 and 30 m/s,
    one step of the default 3DOF config with every row of discrete_ref.TABLES[k]. From 5 m/s every row ends on
    the ground event and lands (rew_goal 10); from 30 m/s every row ends on the ground event and does not land
    (rew_goal 0); from 0.5 m/s only the rows below full thrust touch down within the step. So the GPU
    reference's envs 32 .. 47 land and 48 .. 63 hit the ground without landing whatever the policy chooses."""
    from rl_rocket_amd.params import TERM_NAMES_3DOF, make_config

    assert TERM_NAMES_3DOF[-1] == "rew_goal"
    cfg = oracle_mod.make_cfg(3, **oracle_mod.DEFAULTS_3DOF)
    ec = make_config(3)
    m = 0.5 * (float(ec.ic_low[-1]) + float(ec.ic_high[-1]))
    table = np.asarray(D.TABLES[k], np.float32)

    def step(v):
        s = np.array([[0, 0.02, math.pi / 2, 0, -v, 0, m]] * k, np.float64)
        out = oracle_mod.step(cfg, s.astype(np.float32), 0.0, s, table, nthreads=0)  # 0: the process's OpenMP setting stays
        assert not out["bounds_violation"].any()
        return out["done"], out["status"], out["terms"][:, -1]

    done, status, goal = step(5.0)
    assert done.all() and (status == 1).all() and (goal == 10.0).all()
    done, status, goal = step(30.0)
    assert done.all() and (status == 1).all() and (goal == 0.0).all()
    done, status, goal = step(0.5)
    low = table[:, 1] < 1.0
    assert low.any() and not low.all()
    assert np.array_equal(done, low) and np.array_equal(status == 1, low) and np.array_equal(goal == 10.0, low)
