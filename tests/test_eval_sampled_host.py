"""The sampled one-launch evaluation's host side (no GPU): rr_policy_evaluate_sampled and
rr_policy_evaluate_discrete_sampled in the header and in the ctypes table, ABI 14 unchanged; the library exports
them and keeps the cross-unit launchers hidden; the refusals that come before the handle is read; the two
translation units in directories of their own, compiled by the link call from the shared evaluation body; no
scratch in any of the 28 kernels; the ISA record; PolicyEvaluator's deterministic= / seed= keywords and their
refusals on stub batches; and the inputs of tests/test_gpu_eval_sampled.py run on the CPU oracle, so that the
ways its episodes end and the indices it draws are known before anything runs on a GPU."""
import ctypes
import json
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

GAUSS, CAT = "rr_policy_evaluate_sampled", "rr_policy_evaluate_discrete_sampled"
SEED, TL, NE, N = 11, 80, 2, 300  # tests/test_gpu_eval_sampled.py's


def _args(name):
    code = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, code)
    assert m, name + " is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_both_and_signatures_mirror_them_abi_14():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14
    g, c = _args(GAUSS), _args(CAT)
    # the recording twins' lists with (seed, iter) after the precision
    tr, ctr = _args("rr_policy_evaluate_trace"), _args("rr_policy_evaluate_discrete_trace")
    assert g == tr[:3] + ["uint64_t seed", "const uint64_t* iter"] + tr[3:]
    assert c == ctr[:5] + ["uint64_t seed", "const uint64_t* iter"] + ctr[5:]
    assert len(g) == 11 and len(c) == 14
    for name, args, twin, at in ((GAUSS, g, "rr_policy_evaluate_trace", 3), (CAT, c, "rr_policy_evaluate_discrete_trace", 5)):
        res, sig = _lib.SIGNATURES[name]
        tres, tsig = _lib.SIGNATURES[twin]
        assert res is ctypes.c_int and len(sig) == len(args)
        assert sig == tsig[:at] + [ctypes.c_uint64, ctypes.c_void_p] + tsig[at:]


def test_library_exports_the_symbols_and_hides_the_launchers():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in (GAUSS, CAT):
        assert re.search(r"\bT %s\b" % name, out)
    assert not re.search(r"rrc_launch_eval_sampled|rrc_launch_eval_discrete_sampled", out)
    assert lib.rr_abi_version() == 14


def test_refusals_before_the_handle_is_read():
    """On fake pointers that are never dereferenced."""
    lib = _lib.load()
    V = ctypes.c_void_p
    out = ctypes.byref(_lib.RrEvalOut(episodes=0x60000))
    params, handle, it = V(0x70000), V(0x80000), V(0x90000)
    table = (ctypes.c_float * 8)(0.0, -1.0, -1.0, 1.0, 0.0, 1.0, 1.0, 1.0)

    def refused(rc, name, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(name.encode() + b": ") and word in msg, msg

    def trace(**kw):
        args = dict(slot=0x100000, n_slots=1, steps=4, state=0x200000, length=0x300000)
        args.update(kw)
        return ctypes.byref(_lib.RrEvalTrace(**args))

    g = lib.rr_policy_evaluate_sampled
    refused(g(handle, params, 0, SEED, None, 1, 10, out, None, None, None), GAUSS, b"iter")
    refused(g(None, params, 0, SEED, it, 1, 10, out, None, None, None), GAUSS, b"handle")
    refused(g(handle, None, 0, SEED, it, 1, 10, out, None, None, None), GAUSS, b"params")
    refused(g(handle, V(0x70004), 0, SEED, it, 1, 10, out, None, None, None), GAUSS, b"aligned")
    refused(g(handle, params, 7, SEED, it, 1, 10, out, None, None, None), GAUSS, b"precision")
    refused(g(handle, params, 0, SEED, it, 1, 10, None, None, None, None), GAUSS, b"out")
    refused(g(handle, params, 0, SEED, it, 1, 10, out, trace(n_slots=0), None, None), GAUSS, b"n_slots")
    refused(g(handle, params, 0, SEED, it, 1, 10, out, trace(state=None), None, None), GAUSS, b"trace->state")
    c = lib.rr_policy_evaluate_discrete_sampled
    refused(c(handle, params, 4, table, 0, SEED, None, 1, 10, out, None, None, None, None), CAT, b"iter")
    refused(c(handle, params, 4, table, 0, SEED, it, 1, 10, out, None, V(0x400000), None, None), CAT, b"choice")
    refused(c(handle, params, 4, table, 0, SEED, it, 1, 10, out, trace(), V(0x400002), None, None), CAT, b"4-B")
    refused(c(handle, params, 4, table, 0, SEED, it, 1, 10, out, trace(steps=0), None, None, None), CAT, b"steps")
    for prec in (_lib.RR_POLICY_BF16, _lib.RR_POLICY_FP16X3, 7):
        refused(c(handle, params, 4, table, prec, SEED, it, 1, 10, out, None, None, None, None), CAT, b"RR_POLICY_FP32")
    for k in (1, 5):
        refused(c(handle, params, k, table, 0, SEED, it, 1, 10, out, None, None, None, None), CAT, b"2 .. 4")
    refused(c(handle, params, 4, None, 0, SEED, it, 1, 10, out, None, None, None, None), CAT, b"table")
    refused(c(handle, params, 4, table, 0, SEED, it, 0, 10, out, None, None, None, None), CAT, b"n_episodes")
    refused(c(handle, params, 4, table, 0, SEED, it, 1, 10, None, None, None, None, None), CAT, b"out")
    refused(c(None, params, 4, table, 0, SEED, it, 1, 10, out, None, None, None, None), CAT, b"handle")
    # the deterministic twins keep their own prefixes
    assert lib.rr_policy_evaluate_trace(None, params, 0, 1, 10, out, trace(), None, None) == _lib.RR_EINVAL
    assert lib.rr_last_error().startswith(b"rr_policy_evaluate_trace: ")


def test_build_compiles_both_units_in_the_link_call_from_the_shared_body():
    csrc = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc")
    cmds = B.commands()
    assert len(cmds) == 6 and len([c for c in cmds if "-c" in c]) == 5
    for src, sub in ((B.SRC_EVAL_SAMPLED, "eval_sampled"), (B.SRC_EVAL_SAMPLED_DISCRETE, "eval_sampled_discrete")):
        assert os.path.dirname(src) == os.path.join(csrc, sub) and os.path.isfile(src)
        assert os.listdir(os.path.dirname(src)) == [os.path.basename(src)] and src in B.sources()
        assert [c for c in cmds if src in c] == [cmds[-1]]  # compiled by the link call only
        text = open(src).read()
        incs = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, flags=re.M)
        assert "rocket_eval.inc" in incs and incs.count("rocket_eval_body.inc") == 2  # plain and recording
        for inc in incs:
            assert os.path.isfile(os.path.join(csrc, inc)), inc
        assert re.search(r"^#define RR_EVAL_SAMPLE\s*$", text, flags=re.M)
        assert re.search(r"^#define RR_POL_PREFETCH_A 1\s*$", text, flags=re.M)
    for flag in B.COLLECT_FLAGS:
        assert flag in cmds[-1]
    # the body is reached through rocket_eval.inc, and no other file defines the macro
    assert '#include "rocket_eval_body.inc"' in open(os.path.join(csrc, "rocket_eval.inc")).read()
    body = open(os.path.join(csrc, "rocket_eval_body.inc")).read()
    assert "RR_EVAL_SAMPLE" in body and "statement for statement" in body
    users = [p for p in B.sources() if re.search(r"^#define RR_EVAL_SAMPLE\b", open(p).read(), flags=re.M)]
    assert sorted(users) == sorted([B.SRC_EVAL_SAMPLED, B.SRC_EVAL_SAMPLED_DISCRETE])


def test_no_new_kernel_uses_scratch():
    """The kernel descriptor's private_segment_fixed_size (bytes 4..8) is 0 in all 24 + 4 instantiations."""
    from test_eval_trace_host import _kernel_descriptors

    kds = {k: v for k, v in _kernel_descriptors(B.OUT).items() if "sampled" in k}
    assert len(kds) == 28
    for k, kd in kds.items():
        assert struct.unpack_from("<I", kd, 4)[0] == 0, k


def test_isa_record_lists_every_prior_kernel_unchanged():
    rec = json.load(open(os.path.join(B.ROOT, "profiles", "eval_sampled", "isa_before_after.json")))
    assert rec["changed"] == 0 and rec["removed"] == [] and len(rec["before"]) == rec["kernels_in_parent"]
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert len(rec["added"]) == 28 and all("sampled" in k for k in rec["added"])
    assert sorted(set(rec["after"]) - set(rec["before"])) == sorted(rec["added"])
    # the parent of this record is the tree the previous record describes
    prev = json.load(open(os.path.join(B.ROOT, "profiles", "eval_exact_discrete", "isa_before_after.json")))
    assert rec["before"] == prev["after"]


# ---- PolicyEvaluator ----

def _stub(model=6, integrator=0, device="cuda:0"):
    ns, na = (14, 3) if model == 6 else (7, 2)
    return types.SimpleNamespace(num_envs=8, state_dim=ns, action_dim=na, device=device, model=model,
                                 params=types.SimpleNamespace(integrator=integrator, flags=_lib.RR_FLAG_AUTO_RESET,
                                                              max_episode_steps=8))


class _Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """The constructor passes every check, allocates its outputs (on the CPU: the stub's device holds no memory
    here) and goes on to load the library, where it is stopped."""
    import torch

    zeros = torch.zeros

    def load():
        raise _Reached()

    monkeypatch.setattr(torch, "zeros", lambda *a, **kw: zeros(*a, **dict(kw, device="cpu")))
    monkeypatch.setattr(_lib, "load", load)


def test_policy_evaluator_refusals_with_deterministic_false(no_device):
    from rl_rocket_amd.rollout import MlpActorCritic, MlpCategoricalActorCritic, PolicyEvaluator

    pol, cat = MlpActorCritic(14, 3), MlpCategoricalActorCritic(7, 4)
    dop = _lib.RR_INT_DOPRI5
    scope = "step-by-step path and the exact integrator are out of scope"
    for kw, stub, p, word in (
            (dict(fused=False), _stub(), pol, "fused=False"),
            (dict(), _stub(), MlpActorCritic(14, 3, hidden=(32, 32)), "64x64"),
            (dict(), _stub(integrator=dop), pol, "dopri5"),
            (dict(fused=True), _stub(integrator=dop), pol, "dopri5"),
            (dict(), _stub(device="cpu"), pol, "CUDA"),
            (dict(record=[0], record_in_launch=True), _stub(), pol, "record_in_launch"),
            (dict(), _stub(3), cat, "Categorical.*fused=True"),
            (dict(fused=False), _stub(3), cat, "fused=False"),
            (dict(fused=True), _stub(3, integrator=dop), cat, "dopri5"),
            (dict(fused=True), _stub(3, device="cpu"), cat, "CUDA")):
        with pytest.raises(ValueError, match=word) as e:
            PolicyEvaluator(stub, p, deterministic=False, **kw)
        assert scope in str(e.value), str(e.value)
    # the refusals it shares with the deterministic evaluator keep their words
    with pytest.raises(ValueError, match="policy_dtype='bf16'"):
        PolicyEvaluator(_stub(3), cat, fused=True, policy_dtype="bf16", deterministic=False)
    with pytest.raises(ValueError, match="64x64"):
        PolicyEvaluator(_stub(3), MlpCategoricalActorCritic(7, 4, hidden=(32, 32)), fused=True, deterministic=False)
    # accepted: Gaussian with fused=None and every policy_dtype, Categorical with fused=True
    for dt in ("fp32", "fp16x3", "bf16"):
        with pytest.raises(_Reached):
            PolicyEvaluator(_stub(), pol, policy_dtype=dt, deterministic=False, seed=3)
    with pytest.raises(_Reached):
        PolicyEvaluator(_stub(3), cat, fused=True, deterministic=False)


def test_deterministic_true_reaches_the_same_code_as_before(monkeypatch):
    """deterministic=True (the default, or given) owns no seed and no iter and run() makes the deterministic
    call: seen on a fake library whose every function records its name."""
    import torch
    from rl_rocket_amd import evaluate
    from rl_rocket_amd.rollout import MlpActorCritic, PolicyEvaluator

    calls = []

    class FakeLib:
        def __getattr__(self, name):
            def f(*a):
                calls.append((name, len(a)))
                return 0
            return f

    zeros = torch.zeros
    monkeypatch.setattr(torch, "zeros", lambda *a, **kw: zeros(*a, **dict(kw, device="cpu")))
    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(evaluate, "PolicyPack", lambda *a, **kw: types.SimpleNamespace(pack=lambda: zeros(4), prec=0))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(cuda_stream=0))
    pol = MlpActorCritic(14, 3)

    def run(**kw):
        del calls[:]
        stub = _stub()
        stub._h, stub.obs = None, zeros(8, 14)
        ev = PolicyEvaluator(stub, pol, **kw)
        ev.run()
        return ev, list(calls)

    for kw in (dict(), dict(deterministic=True), dict(deterministic=True, seed=9)):
        ev, seen = run(**kw)
        assert seen == [("rr_policy_evaluate", 8)] and ev.deterministic
        assert not hasattr(ev, "seed") and not hasattr(ev, "iter")
    ev, seen = run(deterministic=False, seed=2 ** 64 + 5)
    assert seen == [("rr_policy_evaluate_sampled", 11)] and not ev.deterministic
    assert ev.seed == 5 and ev.iter.dtype == torch.int64 and ev.iter.tolist() == [1]  # advanced by run()
    ev.run()
    assert ev.iter.tolist() == [2]


# ---- the inputs of tests/test_gpu_eval_sampled.py on the CPU oracle ----

def _oracle_run(oracle_mod, model, act_of, table=None):
    """oracle.step (the reference integrator, fp64) in a loop of NE * TL steps with TimeLimit TL and numpy resets
    inside the init space in place of the kernel's reset stream; act_of(obs float32 [n, ns], t) gives the action
    rows. Returns per-episode flags (event, bounds, truncation) of the first NE episodes of every env and the
    number of episodes each env finished."""
    from rl_rocket_amd.params import ENV_CONFIG_6DOF, make_config

    kw = oracle_mod.ENV_CONFIG_6DOF if model == 6 else oracle_mod.DEFAULTS_3DOF
    cfg = oracle_mod.make_cfg(model, **kw)
    ec = make_config(model, **(ENV_CONFIG_6DOF if model == 6 else {}))
    ns = 14 if model == 6 else 7
    norm = np.array(cfg.normalizer[:ns])
    lo, hi = np.asarray(ec.ic_low, np.float64), np.asarray(ec.ic_high, np.float64)
    rng = np.random.default_rng(1234)

    def sample(m):
        return (lo + (hi - lo) * rng.random((m, ns))).astype(np.float32).astype(np.float64)

    state = sample(N)
    ic = state.astype(np.float32)
    el = np.zeros(N, np.int64)
    ep = np.zeros(N, np.int64)
    ends = np.zeros(3, np.int64)
    for t in range(NE * TL):
        obs = (state.astype(np.float32).astype(np.float64) / norm).astype(np.float32)
        out = oracle_mod.step(cfg, ic, el * cfg.dt, state, act_of(obs, t), nthreads=8)
        trunc = ~out["done"] & (el + 1 == TL)
        end = out["done"] | trunc
        active = ep < NE
        ends += [int((active & out["done"] & (out["status"] > 0)).sum()), int((active & out["bounds_violation"]).sum()),
                 int((active & trunc).sum())]
        state = out["state_out"].copy()
        el += 1
        if end.any():
            state[end] = sample(int(end.sum()))
            ic[end] = state[end].astype(np.float32)
            el[end] = 0
        ep += end & active
    return ends, ep


@pytest.mark.parametrize("model", [6, 3])
def test_gaussian_cases_on_the_cpu_oracle(oracle_mod, model):
    """rollout_ref.scaled_policy(seed 5, head_scale 1.0 | 0.05) at log_std = -1 with rollout_ref.noise_ref's draws
    at t = the step of the call: every env finishes both episodes and each way an episode can end occurs. Found
    here, event / bounds / truncation of 600: 6DOF 45 / 521 / 34, 3DOF 345 / 1 / 254 (an earlier run with other
    reset draws: 43 / 507 / 50 and 331 / 1 / 268)."""
    import torch
    import rollout_ref as R

    ns, na = (14, 3) if model == 6 else (7, 2)
    p64 = R.policy64(R.scaled_policy(ns, na, seed=5, head_scale=1.0 if model == 6 else 0.05))
    std = np.exp(-1.0)

    def act_of(obs, t):
        with torch.no_grad():
            mean = p64.action_net(p64.pi_net(torch.from_numpy(obs).double())).numpy()
        return np.clip(mean + std * R.noise_ref(N, 0, SEED, 0, t, na), -1.0, 1.0).astype(np.float32)

    ends, ep = _oracle_run(oracle_mod, model, act_of)
    print("%dDOF on the oracle, log_std = -1: event / bounds / truncation %s of %d episodes" % (model, ends.tolist(), NE * N))
    assert int(ep.min()) == NE
    assert ends[0] >= 1 and ends[2] >= 1
    if model == 6:
        assert ends[1] >= 1


@pytest.mark.parametrize("k,seed", [(4, 25), (3, 0), (2, 1)])
def test_categorical_cases_on_the_cpu_oracle(oracle_mod, k, seed):
    """discrete_ref.cat_policy(K, seed) with discrete_ref.TABLES[K], the index from discrete_ref.uniform_ref /
    act_ref at t = the step of the call: every index occurs, and for K = 4 and 3 events and truncations both occur
    (K = 2 truncates nearly every episode). Found here, index usage over the 160 x 300 steps and event / bounds /
    truncation: K = 4 6350 / 14537 / 16446 / 10667 and 136 / 251 / 213; K = 3 18349 / 13729 / 15922 and 531 / 20 /
    51; K = 2 20217 / 27783 and 3 / 0 / 597 (an earlier run with other reset draws, counting the steps inside the
    episodes only: K = 4 5711 / 12779 / 15105 / 9318 and 139 / 249 / 215, K = 3 16681 / 12862 / 14823 and 526 / 15
    / 62, K = 2 20169 / 27831)."""
    import discrete_ref as D

    pol = D.cat_policy(k, seed)
    table = np.asarray(D.TABLES[k], np.float32)
    use = np.zeros(4, np.int64)

    def act_of(obs, t):
        idx, _, _ = D.act_ref(D.forward64(pol, obs)[2], D.uniform_ref(N, 0, SEED, 0, t))
        use[:k] += np.bincount(idx, minlength=k)
        return table[idx]

    ends, ep = _oracle_run(oracle_mod, 3, act_of)
    print("K = %d on the oracle: index usage %s, event / bounds / truncation %s" % (k, use.tolist(), ends.tolist()))
    assert int(ep.min()) == NE
    assert (use[:k] >= 1).all()
    if k >= 3:
        assert ends[0] >= 1 and ends[2] >= 1
