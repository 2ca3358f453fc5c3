"""rr_policy_evaluate_exact_discrete's host side (no GPU): the C declaration, its ctypes mirror and the
unchanged ABI number; the library exports the symbol and keeps the cross-unit launcher hidden; the call
refuses null / invalid arguments with its own prefix before any HIP call; the kernel's translation unit
lives in a directory of its own and is compiled by the link call only; its contraction pragma sits
between the policy includes and the solver; the kernel uses no scratch; the ISA record; PolicyEvaluator's
refusals that need no GPU; and the cases of tests/test_gpu_eval_exact_discrete.py (E3, E2) run on the CPU
oracle, so that the share of envs they leave out is known before anything runs on a GPU."""
import ctypes
import math
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

NAME = "rr_policy_evaluate_exact_discrete"


def test_header_declares_it_and_signatures_mirror_it_abi_14():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text)
    assert _lib.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % NAME, code)
    assert m, NAME + " is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 and args[0].startswith("rr_env*") and "rr_eval_out" in args[7]
    assert args[2] == "int n_choices" and args[3] == "const float* table" and args[9].startswith("void*")
    # the same argument list as the fast modes' call, in the header and in the binding
    m2 = re.search(r"int\s+rr_policy_evaluate_discrete\s*\(([^;]*)\)\s*;", code)
    assert [a.strip() for a in m2.group(1).split(",")] == args
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["rr_policy_evaluate_discrete"]
    assert len(_lib.SIGNATURES[NAME][1]) == 10


def test_library_exports_the_symbol_and_the_abi_number_stays():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT %s\b" % NAME, out)
    assert not re.search(r"rrx_launch_eval_exact_discrete", out)  # the cross-TU launcher stays hidden
    assert lib.rr_abi_version() == 14


def test_refuses_null_and_invalid_arguments_before_any_hip_call():
    """Every refusal that comes before the handle is read, on fake pointers that are never dereferenced."""
    lib = _lib.load()
    V = ctypes.c_void_p
    out = _lib.RrEvalOut(episodes=0x60000)
    params = V(0x70000)  # 16-B aligned
    handle = V(0x80000)  # never dereferenced: the checks below come before anything reads it
    call = getattr(lib, NAME)

    def table(k=4, bad=None):
        rows = [[0.0, -1.0], [-1.0, 1.0], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0]]
        if bad is not None:
            rows[bad[0]][bad[1]] = bad[2]
        return (ctypes.c_float * (2 * k))(*[v for r in rows[:k] for v in r])

    def refused(rc, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(NAME.encode() + b": ") and len(msg) > len(NAME) + 10, msg
        assert word in msg, msg

    o = ctypes.byref(out)
    refused(call(handle, None, 4, table(), 0, 1, 10, o, None, None), b"params")
    refused(call(handle, V(0x70004), 4, table(), 0, 1, 10, o, None, None), b"aligned")
    for prec in (_lib.RR_POLICY_BF16, _lib.RR_POLICY_FP16X3, 7):
        refused(call(handle, params, 4, table(), prec, 1, 10, o, None, None), b"RR_POLICY_FP32")
    for k in (1, 5, 0, -1):
        refused(call(handle, params, k, table(5), 0, 1, 10, o, None, None), b"2 .. 4")
    refused(call(handle, params, 4, None, 0, 1, 10, o, None, None), b"table")
    refused(call(handle, params, 4, table(bad=(1, 0, math.inf)), 0, 1, 10, o, None, None), b"finite")
    refused(call(handle, params, 3, table(bad=(2, 1, math.nan)), 0, 1, 10, o, None, None), b"finite")
    refused(call(handle, params, 4, table(), 0, 1, 10, None, None, None), b"out")
    refused(call(handle, params, 4, table(), 0, 1, 10, ctypes.byref(_lib.RrEvalOut()), None, None), b"episodes")
    refused(call(handle, params, 4, table(), 0, 0, 10, o, None, None), b"n_episodes")
    refused(call(None, params, 4, table(), 0, 1, 10, o, None, None), b"handle")
    # the two calls it is composed of keep their own prefixes
    assert lib.rr_policy_evaluate_discrete(None, params, 4, table(), 0, 1, 10, o, None, None) == _lib.RR_EINVAL
    assert lib.rr_last_error().startswith(b"rr_policy_evaluate_discrete: ")
    assert lib.rr_policy_evaluate_exact(None, params, 0, 1, 10, o, None, None) == _lib.RR_EINVAL
    assert lib.rr_last_error().startswith(b"rr_policy_evaluate_exact: ")


def test_build_compiles_the_unit_of_its_own_in_the_link_call():
    src = B.SRC_EVAL_EXACT_DISCRETE
    csrc = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc")
    assert os.path.dirname(src) == os.path.join(csrc, "eval_exact_discrete") and os.path.isfile(src)
    assert src in B.sources()
    cmds = B.commands()
    assert len(cmds) == 6 and len([c for c in cmds if "-c" in c]) == 5
    assert [c for c in cmds if src in c] == [cmds[-1]]  # compiled by the link call only
    assert "-shared" in cmds[-1] and "-c" not in cmds[-1]
    for flag in B.COLLECT_FLAGS:
        assert flag in cmds[-1]
    assert B.EXACT_FLAGS[-1] not in cmds[-1]  # the collect's settings only, not the exact units' scheduler bias
    # every file of the new directory is a source, and each includes only files of csrc/ itself
    for f in os.listdir(os.path.dirname(src)):
        p = os.path.join(os.path.dirname(src), f)
        assert p in B.sources()
        incs = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(p).read(), flags=re.M)
        assert incs
        for inc in incs:
            assert os.path.isfile(os.path.join(csrc, inc)) or inc == "rocket_hip.h", inc


def test_the_solver_is_compiled_without_contraction_and_the_policy_outside_it():
    text = open(B.SRC_EVAL_EXACT_DISCRETE).read()
    off = re.search(r"^#pragma clang fp contract\(off\)", text, flags=re.M).start()
    for inc in ("rocket_policy.inc", "rocket_rollout.inc", "rocket_eval.inc"):
        assert 0 <= text.index('#include "%s"' % inc) < off
    assert text.index('#include "rocket_dopri5.inc"') > off
    assert text.index("__global__") > off


def test_the_kernel_uses_no_scratch():
    """The kernel descriptor's private_segment_fixed_size (bytes 4..8) is 0."""
    from test_eval_trace_host import _kernel_descriptors

    kds = {k: v for k, v in _kernel_descriptors(B.OUT).items() if "eval_exact_discrete_kernel" in k}
    assert len(kds) == 1
    for k, kd in kds.items():
        assert struct.unpack_from("<I", kd, 4)[0] == 0, k


def test_isa_record_lists_every_prior_kernel_unchanged():
    import json

    rec = json.load(open(os.path.join(B.ROOT, "profiles", "eval_exact_discrete", "isa_before_after.json")))
    assert rec["changed"] == 0 and rec["removed"] == [] and len(rec["before"]) == rec["kernels_in_parent"]
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert len(rec["added"]) >= 1 and all("eval_exact_discrete_kernel" in k for k in rec["added"])
    assert sorted(set(rec["after"]) - set(rec["before"])) == sorted(rec["added"])


# ---- PolicyEvaluator ----

def _stub(integrator, device="cuda:0"):
    return types.SimpleNamespace(num_envs=8, state_dim=7, action_dim=2, device=device, model=3,
                                 params=types.SimpleNamespace(integrator=integrator, flags=_lib.RR_FLAG_AUTO_RESET,
                                                              max_episode_steps=8))


class _Reached(Exception):
    pass


def test_policy_evaluator_accepts_the_combination_and_keeps_its_refusals(monkeypatch):
    import torch
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic, PolicyEvaluator

    pol = MlpCategoricalActorCritic(7, 4)
    dop = _lib.RR_INT_DOPRI5
    # accepted: the constructor passes every check, allocates its outputs and goes on to load the library
    # (the stub's device holds no memory here: the output planes are allocated on the CPU instead)
    zeros = torch.zeros

    def load():
        raise _Reached()

    monkeypatch.setattr(torch, "zeros", lambda *a, **kw: zeros(*a, **dict(kw, device="cpu")))
    monkeypatch.setattr(_lib, "load", load)
    with pytest.raises(_Reached):
        PolicyEvaluator(_stub(dop), pol, fused=True)
    with pytest.raises(_Reached):  # as on an RK4 batch
        PolicyEvaluator(_stub(0), pol, fused=True)
    # the refusals that stay
    with pytest.raises(ValueError, match="fused=True.*dopri5"):
        PolicyEvaluator(_stub(dop), pol, fused=True, record=[0])
    with pytest.raises(ValueError, match="Categorical.*dopri5"):
        PolicyEvaluator(_stub(dop), pol, fused=True, record=[0], record_in_launch=True)
    with pytest.raises(ValueError, match="CUDA"):
        PolicyEvaluator(_stub(dop, device="cpu"), pol, fused=True)
    with pytest.raises(ValueError, match="64x64"):
        PolicyEvaluator(_stub(dop), MlpCategoricalActorCritic(7, 4, hidden=(32, 32)), fused=True)
    with pytest.raises(ValueError, match="policy_dtype='bf16'"):
        PolicyEvaluator(_stub(dop), pol, fused=True, policy_dtype="bf16")


def test_the_default_for_a_categorical_policy_stays_step_by_step(monkeypatch):
    """fused=None: the constructor reaches the step-by-step path's set-up with fused == False (seen where it
    loads the library, which comes after `fused` is settled)."""
    import torch
    from rl_rocket_amd import evaluate
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic, PolicyEvaluator

    seen = {}
    zeros = torch.zeros
    monkeypatch.setattr(torch, "zeros", lambda *a, **kw: zeros(*a, **dict(kw, device="cpu")))

    def make_trace(self, record, record_steps):  # called after self.fused is set, before anything is loaded
        seen["fused"], seen["exact"] = self.fused, self._exact
        raise _Reached()

    monkeypatch.setattr(evaluate.PolicyEvaluator, "_make_trace", make_trace)
    with pytest.raises(_Reached):
        PolicyEvaluator(_stub(_lib.RR_INT_DOPRI5), MlpCategoricalActorCritic(7, 4))
    assert seen == dict(fused=False, exact=False)
    with pytest.raises(_Reached):
        PolicyEvaluator(_stub(_lib.RR_INT_DOPRI5), MlpCategoricalActorCritic(7, 4), fused=True)
    assert seen == dict(fused=True, exact=True)


# ---- the E3 and E2 cases of tests/test_gpu_eval_exact_discrete.py on the CPU oracle ----

TL, NE, N = 20, 2, 300
E3_SCALE = 1e6      # the action head's scale of E3
E3_GAP = 120.0      # E3 leaves an env out where its two largest float64 logits come closer than this
E3_CASES = ((4, 25), (3, 0), (2, 1))  # K, cat_policy's seed: the GPU test's
ORACLE_CAP = 0.025  # half the GPU test's cap of 5 %


def scaled_cat_policy(k, seed, scale):
    """discrete_ref.cat_policy with the action bias shifted so that the K float64 logits are equal at the
    upper corner of the init space (every state component at its largest initial value), then the action
    head's weight and bias scaled by `scale`. Without the shift the bias decides: over the 2 s of a
    TimeLimit-20 episode the observations move by a few percent and the logits by a few hundredths, and in
    every seed tried (0 .. 20 and 60 .. 70 at each K) every env kept to one or two indices, never all K.
    With it the K decision regions meet at the edge of the states the envs visit: all K indices occur, and a
    third to a half of the envs cross a boundary. (With the regions meeting at the centre of the init space
    every env crosses, and 10 .. 30 % of them come within E3_GAP of a boundary on some step.)"""
    import torch
    import discrete_ref as D
    from rl_rocket_amd.params import make_config

    pol = D.cat_policy(k, seed)
    ec = make_config(3)
    corner = np.asarray(ec.ic_high, np.float64) / np.asarray(ec.state_normalizer, np.float64)
    with torch.no_grad():
        pol.action_net.bias.sub_(torch.from_numpy(D.forward64(pol, corner.astype(np.float32)[None])[0][0]).float())
        pol.action_net.weight.mul_(scale)
        pol.action_net.bias.mul_(scale)
    return pol


def oracle_run(oracle_mod, k, seed, scale, n=N):
    """oracle.step (the exact integrator) in a loop with TimeLimit 20 and uniform resets inside the init
    space, the action being the table row of the float64 policy's largest logit, for 40 steps. Envs 0..95
    start on the GPU test's landing fixture, the others uniformly inside the init space. Returns each env's
    smallest gap between its two largest logits over the steps of its first two episodes, the number of
    distinct indices it took, and how often each index was taken."""
    import discrete_ref as D
    from rl_rocket_amd.params import make_config

    cfg = oracle_mod.make_cfg(3, **oracle_mod.DEFAULTS_3DOF)
    ec = make_config(3)
    norm = np.array(cfg.normalizer[:7])
    lo, hi = np.asarray(ec.ic_low, np.float64), np.asarray(ec.ic_high, np.float64)
    rng = np.random.default_rng(seed)

    def sample(m):
        return (lo + (hi - lo) * rng.random((m, 7))).astype(np.float32).astype(np.float64)

    pol = scaled_cat_policy(k, seed, scale)
    table = np.asarray(D.TABLES[k], np.float32)
    state = sample(n)
    m = 0.5 * (lo[-1] + hi[-1])
    state[:96] = np.array([0, 0.02, math.pi / 2, 0, -0.5, 0, m])
    state[32:64, 4] = -5.0
    state[64:96, 4] = -50.0
    ic = state.astype(np.float32)
    el = np.zeros(n, np.int64)
    ep = np.zeros(n, np.int64)
    gap = np.full(n, np.inf)
    took = np.zeros((n, 4), bool)
    for _ in range(NE * TL):
        obs = (state.astype(np.float32).astype(np.float64) / norm).astype(np.float32)
        z = D.forward64(pol, obs)[0]
        top = np.sort(z, axis=1)
        idx = z.argmax(1)
        active = ep < NE
        gap = np.where(active, np.minimum(gap, top[:, -1] - top[:, -2]), gap)
        took[np.arange(n)[active], idx[active]] = True
        out = oracle_mod.step(cfg, ic, el * cfg.dt, state, table[idx], nthreads=8)
        end = out["done"] | (el + 1 == TL)
        state = out["state_out"].copy()  # the fp64 state stays fp64 between steps
        el += 1
        if end.any():
            state[end] = sample(int(end.sum()))
            ic[end] = state[end].astype(np.float32)
            el[end] = 0
        ep += end & active
    return gap, took


@pytest.mark.parametrize("k,seed", E3_CASES)
def test_e3_cases_on_the_cpu_oracle(oracle_mod, k, seed):
    """E3's three conditions at half the GPU test's cap. Found here (300 envs x 40 steps; envs left out,
    compared envs that take two or more distinct indices, envs per index): K = 4 seed 25: 5, 131 of 295,
    [84, 35, 295, 40]; K = 3 seed 0: 5, 117 of 295, [18, 286, 109]; K = 2 seed 1: 6, 108 of 294, [120, 282].
    The seeds were chosen here, before anything ran on a GPU: of seeds 0 .. 64 at K = 4, 14, 25 and 46 met
    all three conditions; of 0 .. 5 at K = 3, 0 and 3; of 0 .. 5 at K = 2, 1."""
    gap, took = oracle_run(oracle_mod, k, seed, E3_SCALE)
    out = gap < E3_GAP
    two = (took.sum(1) >= 2) & ~out
    print("E3 on the oracle, K = %d seed %d: %d envs of %d left out, %d of the %d compared take two or more indices, "
          "envs per index %s, smallest gap %.3g" % (k, seed, int(out.sum()), N, int(two.sum()), int((~out).sum()),
                                                    took[~out].sum(0).tolist(), float(gap.min())))
    assert out.mean() <= ORACLE_CAP
    assert two.sum() >= (~out).sum() / 4
    assert took[~out].any(0)[:k].all() and not took[:, k:].any()


@pytest.mark.parametrize("k,seed", E3_CASES[:1])
def test_e2_case_on_the_cpu_oracle(oracle_mod, k, seed):
    """E2 (the unscaled policy, discrete_ref.KNIFE) at half the GPU test's cap. Found here: 3 knife-edge
    envs of 300; 131 envs take two or more indices."""
    import discrete_ref as D

    gap, took = oracle_run(oracle_mod, k, seed, 1.0)
    knife = gap < D.KNIFE
    print("E2 on the oracle, K = %d seed %d: %d knife-edge envs of %d, smallest gap %.3g"
          % (k, seed, int(knife.sum()), N, float(gap.min())))
    assert knife.mean() <= ORACLE_CAP
    assert ((took.sum(1) >= 2) & ~knife).sum() >= N // 4
