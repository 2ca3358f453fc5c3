"""rr_policy_evaluate_exact's host side (no GPU): the C declaration, its ctypes mirror and the
unchanged ABI number; the library exports the symbol and keeps the cross-unit launcher hidden; the
call refuses a null handle / params / out with a message before any HIP call; the build compiles
the kernel's translation unit, which lives in a directory of its own and includes only files of
csrc/."""
import ctypes
import os
import re
import subprocess

from rl_rocket_amd import _lib
from rl_rocket_amd import build as B

NAME = "rr_policy_evaluate_exact"


def test_header_declares_it_and_signatures_mirror_it_abi_14():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text)
    assert _lib.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % NAME, code)
    assert m, NAME + " is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and args[0].startswith("rr_env*") and "rr_eval_out" in args[5]
    assert args[4].startswith("int64_t") and args[7].startswith("void*")
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(argtypes) == 8
    assert argtypes[2:5] == [ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    assert argtypes[5] == ctypes.POINTER(_lib.RrEvalOut)
    # the same argument list as the fast modes' call
    assert argtypes == _lib.SIGNATURES["rr_policy_evaluate"][1]


def test_library_exports_the_symbol_and_the_abi_number_stays():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT %s\b" % NAME, out)
    assert not re.search(r"rrx_launch_eval_exact", out)  # the cross-TU launcher stays hidden
    assert lib.rr_abi_version() == 14


def test_refuses_null_arguments_before_any_hip_call():
    lib = _lib.load()
    V = ctypes.c_void_p
    out = _lib.RrEvalOut(episodes=0x60000)
    params = V(0x70000)  # 16-B aligned
    handle = V(0x80000)  # never dereferenced: the checks below come before anything reads it

    def refused(rc, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(NAME.encode() + b": ") and len(msg) > 36, msg
        assert word in msg, msg

    refused(lib.rr_policy_evaluate_exact(None, params, 0, 1, 10, ctypes.byref(out), None, None), b"handle")
    refused(lib.rr_policy_evaluate_exact(handle, None, 0, 1, 10, ctypes.byref(out), None, None), b"params")
    refused(lib.rr_policy_evaluate_exact(handle, params, 0, 1, 10, None, None, None), b"out")
    refused(lib.rr_policy_evaluate_exact(handle, params, 0, 1, 10, ctypes.byref(_lib.RrEvalOut()), None, None),
            b"episodes")
    refused(lib.rr_policy_evaluate_exact(handle, V(0x70004), 0, 1, 10, ctypes.byref(out), None, None), b"aligned")
    refused(lib.rr_policy_evaluate_exact(handle, params, 7, 1, 10, ctypes.byref(out), None, None), b"precision")
    # the fast modes' call keeps its own prefix
    assert lib.rr_policy_evaluate(None, params, 0, 1, 10, ctypes.byref(out), None, None) == _lib.RR_EINVAL
    assert lib.rr_last_error().startswith(b"rr_policy_evaluate: ")


def test_build_compiles_the_translation_unit_of_its_own():
    src = B.SRC_EVAL_EXACT
    csrc = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc")
    assert os.path.dirname(src) == os.path.join(csrc, "eval_exact") and os.path.isfile(src)
    assert src in B.sources()
    cmds = B.commands()
    compiles = [c for c in cmds if "-c" in c]
    assert len(compiles) == 5 and len(cmds) == 6
    mine = [c for c in compiles if c[-1] == src]
    assert len(mine) == 1
    obj = mine[0][mine[0].index("-o") + 1]
    assert obj in cmds[-1] and "-shared" in cmds[-1]  # linked into the library
    # the solver's and the policy towers' code-generation settings, both
    for flag in B.EXACT_FLAGS + B.COLLECT_FLAGS:
        assert flag in mine[0]
    # every file of the new directory is a source, and each includes only files of csrc/ itself
    for f in os.listdir(os.path.dirname(src)):
        p = os.path.join(os.path.dirname(src), f)
        assert p in B.sources()
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(p).read(), flags=re.M):
            assert os.path.isfile(os.path.join(csrc, inc)) or inc == "rocket_hip.h", inc


def test_the_solver_is_compiled_without_contraction_and_the_policy_outside_it():
    """The order of the translation unit: the policy / rollout includes come before `#pragma clang fp
    contract(off)`, the exact solver and the kernel after it."""
    text = open(B.SRC_EVAL_EXACT).read()
    off = re.search(r"^#pragma clang fp contract\(off\)", text, flags=re.M).start()
    for inc in ("rocket_policy.inc", "rocket_rollout.inc", "rocket_eval.inc"):
        assert 0 <= text.index('#include "%s"' % inc) < off
    assert text.index('#include "rocket_dopri5.inc"') > off
    assert text.index("__global__") > off
