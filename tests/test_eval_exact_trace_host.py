"""rr_policy_evaluate_exact_trace's host side (no GPU): the C declaration, its ctypes mirror and the
unchanged ABI number; the library exports the symbol and keeps the cross-unit launcher hidden; the
call refuses null / invalid arguments with its own prefix before any HIP call; the kernel's
translation unit lives in a directory of its own and is compiled by the link call only; its
contraction pragma sits between the policy includes and the solver; the kernel's trace argument
sits where trace_args reads it and no instantiation uses scratch; PolicyEvaluator's
record_in_launch refusals that need no GPU."""
import ctypes
import os
import re
import struct
import subprocess
import types

import pytest

from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

NAME = "rr_policy_evaluate_exact_trace"


def test_header_declares_it_and_signatures_mirror_it_abi_14():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text)
    assert _lib.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % NAME, code)
    assert m, NAME + " is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[0].startswith("rr_env*") and "rr_eval_out" in args[5]
    assert "rr_eval_trace" in args[6] and args[4].startswith("int64_t") and args[8].startswith("void*")
    # the same argument list as the fast modes' recording call, in the header and in the binding
    m2 = re.search(r"int\s+rr_policy_evaluate_trace\s*\(([^;]*)\)\s*;", code)
    assert [a.strip() for a in m2.group(1).split(",")] == args
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["rr_policy_evaluate_trace"]
    assert len(_lib.SIGNATURES[NAME][1]) == 9


def test_library_exports_the_symbol_and_the_abi_number_stays():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT %s\b" % NAME, out)
    assert not re.search(r"rrx_launch_eval_exact_trace", out)  # the cross-TU launcher stays hidden
    assert lib.rr_abi_version() == 14


def _trace(null=None, n_slots=4, steps=8):
    """An rr_eval_trace of fake non-null device pointers (never dereferenced: every call below is
    refused before it launches)."""
    vals = dict(slot=0x10000, state=0x20000, action=0x30000, terms=0x40000, length=0x50000)
    if null:
        vals[null] = None
    return _lib.RrEvalTrace(n_slots=n_slots, steps=steps, **vals)


def test_refuses_null_and_invalid_arguments_before_any_hip_call():
    lib = _lib.load()
    V = ctypes.c_void_p
    out = _lib.RrEvalOut(episodes=0x60000)
    params = V(0x70000)  # 16-B aligned
    handle = V(0x80000)  # never dereferenced: the checks below come before anything reads it
    call = getattr(lib, NAME)

    def refused(rc, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(NAME.encode() + b": ") and len(msg) > len(NAME) + 10, msg
        assert word in msg, msg

    tr = _trace()
    refused(call(None, params, 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None), b"handle")
    refused(call(handle, None, 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None), b"params")
    refused(call(handle, params, 0, 1, 10, None, ctypes.byref(tr), None, None), b"out")
    refused(call(handle, params, 0, 1, 10, ctypes.byref(_lib.RrEvalOut()), ctypes.byref(tr), None, None), b"episodes")
    refused(call(handle, V(0x70004), 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None), b"aligned")
    refused(call(handle, params, 7, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None), b"precision")
    # the four trace cases
    refused(call(handle, params, 0, 1, 10, ctypes.byref(out), None, None, None), b"trace")
    for null in ("slot", "state", "length"):
        tr = _trace(null=null)
        refused(call(handle, params, 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None), null.encode())
    for kw in (dict(n_slots=0), dict(steps=0)):
        tr = _trace(**kw)
        refused(call(handle, params, 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None), list(kw)[0].encode())
    # the two calls it shares its checks with keep their own prefixes
    tr = _trace()
    assert lib.rr_policy_evaluate_exact(None, params, 0, 1, 10, ctypes.byref(out), None, None) == _lib.RR_EINVAL
    assert lib.rr_last_error().startswith(b"rr_policy_evaluate_exact: ")
    assert lib.rr_policy_evaluate_trace(None, params, 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None,
                                        None) == _lib.RR_EINVAL
    assert lib.rr_last_error().startswith(b"rr_policy_evaluate_trace: ")


def test_build_compiles_the_unit_of_its_own_in_the_link_call():
    src = B.SRC_EVAL_EXACT_TRACE
    csrc = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc")
    assert os.path.dirname(src) == os.path.join(csrc, "eval_exact_trace") and os.path.isfile(src)
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
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(p).read(), flags=re.M):
            assert os.path.isfile(os.path.join(csrc, inc)) or inc == "rocket_hip.h", inc


def test_the_solver_is_compiled_without_contraction_and_the_policy_outside_it():
    text = open(B.SRC_EVAL_EXACT_TRACE).read()
    off = re.search(r"^#pragma clang fp contract\(off\)", text, flags=re.M).start()
    for inc in ("rocket_policy.inc", "rocket_rollout.inc", "rocket_eval.inc"):
        assert 0 <= text.index('#include "%s"' % inc) < off
    assert text.index('#include "rocket_dopri5.inc"') > off
    assert text.index("__global__") > off


def test_trace_argument_sits_where_the_kernel_reads_it_and_no_scratch(tmp_path):
    """eval_exact_trace_kernel reads its trace arguments from the kernel-argument segment at
    kExactTraceArgOff, computed as if the parameters were the members of a C struct: (XParams*, Bufs,
    EvalIO, EvalTraceIO, double*). The code object's metadata must lay them out that way, and every
    kernel descriptor must show no scratch (private_segment_fixed_size, bytes 4..8) and more than the
    256 registers of two waves per SIMD allowed (it runs one wave per SIMD)."""
    from test_eval_trace_host import _code_objects, _kernel_descriptors

    seen = 0
    for co in _code_objects(B.OUT, str(tmp_path)):
        notes = subprocess.run([B._llvm("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        for body, name in re.findall(r"\.args:(.*?)\.group_segment_fixed_size:(?:.*?)\.name:\s+(\S+)", notes, re.S):
            if "eval_exact_trace_kernel" not in name:
                continue
            args = [(int(o), int(sz)) for o, sz, kind in
                    re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+(\w+)", body)
                    if not kind.startswith("hidden")]
            assert len(args) == 5 and args[0] == (0, 8) and args[4][1] == 8, (name, args)
            assert args[3][1] == ctypes.sizeof(_lib.RrEvalTrace), (name, args)
            for (o0, s0), (o1, _s1) in zip(args, args[1:]):
                assert o1 == (o0 + s0 + 7) // 8 * 8, (name, args)
            seen += 1
    assert seen == 6
    kds = {k: v for k, v in _kernel_descriptors(B.OUT).items() if "eval_exact_trace_kernel<" in k}
    assert len(kds) == 6
    for k, kd in kds.items():
        assert struct.unpack_from("<I", kd, 4)[0] == 0, k


def test_isa_record_lists_every_prior_kernel_unchanged():
    import json

    rec = json.load(open(os.path.join(B.ROOT, "profiles", "eval_exact_trace", "isa_before_after.json")))
    assert rec["changed"] == 0 and rec["removed"] == [] and len(rec["before"]) == rec["kernels_in_parent"]
    assert all(rec["after"][k] == h for k, h in rec["before"].items())
    assert len(rec["added"]) == 6 and all("eval_exact_trace_kernel<" in k for k in rec["added"])


# ---- PolicyEvaluator's keyword ----

def _stub(integrator, device="cuda:0", dof=6):
    ns, na = (7, 2) if dof == 3 else (14, 3)
    return types.SimpleNamespace(num_envs=8, state_dim=ns, action_dim=na, device=device, model=dof,
                                 params=types.SimpleNamespace(integrator=integrator, flags=_lib.RR_FLAG_AUTO_RESET,
                                                              max_episode_steps=8))


def test_record_in_launch_refusals():
    from rl_rocket_amd.rollout import MlpActorCritic, MlpCategoricalActorCritic, PolicyEvaluator

    pol = MlpActorCritic(14, 3)
    dop = _lib.RR_INT_DOPRI5
    with pytest.raises(ValueError, match="record_in_launch=True needs record"):
        PolicyEvaluator(_stub(dop), pol, fused=True, record_in_launch=True)
    with pytest.raises(ValueError, match="record_in_launch=True needs fused=True"):
        PolicyEvaluator(_stub(dop), pol, fused=False, record=[0], record_in_launch=True)
    with pytest.raises(ValueError, match="record_in_launch=True needs fused=True"):
        PolicyEvaluator(_stub(dop), pol, record=[0], record_in_launch=True)  # a dopri5 batch defaults to fused=False
    with pytest.raises(ValueError, match="record_in_launch=True needs fused=True"):
        PolicyEvaluator(_stub(0), pol, fused=False, record=[0], record_in_launch=True)
    with pytest.raises(ValueError, match="CUDA"):
        PolicyEvaluator(_stub(dop, device="cpu"), pol, fused=True, record=[0], record_in_launch=True)
    with pytest.raises(ValueError, match="64x64"):
        PolicyEvaluator(_stub(dop), MlpActorCritic(14, 3, hidden=(32, 32)), fused=True, record=[0], record_in_launch=True)
    with pytest.raises(ValueError, match="Categorical.*dopri5"):
        PolicyEvaluator(_stub(dop, dof=3), MlpCategoricalActorCritic(7, 4), fused=True, record=[0],
                        record_in_launch=True)
    # without the keyword the refusal of a recording one-launch exact evaluation stays, and names the keyword
    with pytest.raises(ValueError, match="record_in_launch=True"):
        PolicyEvaluator(_stub(dop), pol, fused=True, record=[0])
    with pytest.raises(ValueError, match="record_in_launch=True"):
        PolicyEvaluator(_stub(dop), pol, fused=True, record=[0], record_in_launch=False)
