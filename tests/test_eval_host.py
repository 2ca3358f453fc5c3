"""rr_policy_evaluate's host side (no GPU): the C declaration, its ctypes mirror and the ABI
number agree; the call refuses bad arguments before any HIP call; EvalResult.stats() reduces
hand-made CPU tensors to SB3's evaluate_policy figures and the reference EpisodeAnalyzer's
statistics, leaving unfinished rows out of every mean."""
import ctypes
import math
import os
import re
import subprocess

import pytest

from rl_rocket_amd import _lib


def _header():
    with open(_lib.HEADER) as f:
        return f.read()


def test_declared_in_header_and_signatures_abi_14():
    text = _header()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text)
    assert _lib.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+rr_policy_evaluate\s*\(([^;]*)\)\s*;", code)
    assert m, "rr_policy_evaluate is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 and args[0].startswith("rr_env*") and "rr_eval_out" in args[5]
    res, argtypes = _lib.SIGNATURES["rr_policy_evaluate"]
    assert res is ctypes.c_int and len(argtypes) == 8
    assert argtypes[2:5] == [ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    assert argtypes[5] is ctypes.POINTER(_lib.RrEvalOut)
    # the flag bits of the header, of _lib and of the Python layer
    from rl_rocket_amd import rollout

    for name in ("EVENT", "BOUNDS", "TRUNCATED", "NONFINITE", "LANDED"):
        bit = int(re.search(r"#define\s+RR_EVAL_%s\s+(0x[0-9a-fA-F]+)" % name, text).group(1), 16)
        assert getattr(_lib, "RR_EVAL_" + name) == bit == getattr(rollout, "EVAL_" + name)


def test_eval_out_layout_matches_header(tmp_path):
    names = [f[0] for f in _lib.RrEvalOut._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rocket_hip.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(rr_eval_out));\n'
    for f in names:
        src += 'printf("%%zu\\n", offsetof(rr_eval_out, %s));\n' % f
    src += "return 0;}\n"
    c, exe = tmp_path / "l.c", tmp_path / "l"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.dirname(_lib.HEADER), str(c), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert ctypes.sizeof(_lib.RrEvalOut) == vals[0]
    assert [getattr(_lib.RrEvalOut, n).offset for n in names] == vals[1:]
    assert names == ["episodes", "ep_return", "ep_length", "flags", "used_mass", "final_state"]


def test_library_exports_it_and_refuses_a_null_handle():
    lib = _lib.load()
    assert lib.rr_abi_version() == 14
    out = _lib.RrEvalOut()
    assert lib.rr_policy_evaluate(None, None, 0, 5, 0, ctypes.byref(out), None, None) == _lib.RR_EINVAL
    assert b"rr_policy_evaluate" in lib.rr_last_error()


def _result():
    """3 envs x 2 episodes. Env 0 finished both, env 1 one, env 2 none: rows (1, 1), (0, 2) and
    (1, 2) are unfinished and hold values that would wreck every mean if they were counted."""
    import torch
    from rl_rocket_amd.params import STATE_NAMES_3DOF
    from rl_rocket_amd.rollout import (EVAL_BOUNDS, EVAL_EVENT, EVAL_LANDED, EVAL_NONFINITE, EVAL_TRUNCATED,
                                       EvalResult)

    junk = 1.0e30
    episodes = torch.tensor([2, 1, 0], dtype=torch.int32)
    ep_return = torch.tensor([[10.0, -2.0, junk], [4.0, junk, float("nan")]])
    ep_length = torch.tensor([[7, 80, 10 ** 6], [9, 10 ** 6, 10 ** 6]], dtype=torch.int32)
    flags = torch.tensor([[EVAL_EVENT | EVAL_LANDED, EVAL_TRUNCATED, EVAL_LANDED],
                          [EVAL_BOUNDS, EVAL_LANDED | EVAL_NONFINITE, 0xFF]], dtype=torch.uint8)
    used_mass = torch.tensor([[100.0, 400.0, junk], [250.0, junk, junk]])
    final_state = torch.full((2, 7, 3), junk)
    for k in range(7):  # final_state[ep][k][env]
        final_state[0, k, 0] = -(k + 1.0)
        final_state[0, k, 1] = 2.0 * (k + 1.0)
        final_state[1, k, 0] = 3.0 * (k + 1.0)
    return EvalResult(episodes, ep_return, ep_length, flags, used_mass, final_state, STATE_NAMES_3DOF)


def test_stats_on_cpu_tensors_excludes_unfinished_rows():
    from rl_rocket_amd.params import STATE_NAMES_3DOF

    res = _result()
    assert res.finished().tolist() == [[True, True, False], [True, False, False]]
    s = res.stats()
    rets = [10.0, -2.0, 4.0]
    mean = sum(rets) / 3
    assert s["mean_reward"] == pytest.approx(mean, rel=1e-12)
    assert s["std_reward"] == pytest.approx(math.sqrt(sum((r - mean) ** 2 for r in rets) / 3), rel=1e-12)  # np.std
    assert s["mean_ep_length"] == pytest.approx((7 + 80 + 9) / 3, rel=1e-12)
    assert s["episodes"] == 3 and s["unfinished"] == 3
    # the success rate is the RR_EVAL_LANDED bit of the finished rows: one of three
    assert s["ep_statistic/landing_success"] == pytest.approx(1 / 3, rel=1e-12)
    assert s["ep_statistic/used_mass"] == pytest.approx(250.0, rel=1e-12)
    assert (s["n_event"], s["n_bounds"], s["n_truncated"], s["n_nonfinite"]) == (1, 1, 1, 0)
    # final_errors/<name>: mean |terminal state| over the finished rows, in state_names order
    keys = [k for k in s if k.startswith("final_errors/")]
    assert keys == ["final_errors/" + n for n in STATE_NAMES_3DOF]
    for k, name in enumerate(STATE_NAMES_3DOF):
        assert s["final_errors/" + name] == pytest.approx((1 + 2 + 3) * (k + 1.0) / 3, rel=1e-6)


def test_stats_names_follow_the_6dof_state_names():
    import torch
    from rl_rocket_amd.params import STATE_NAMES_6DOF
    from rl_rocket_amd.rollout import EVAL_LANDED, EvalResult

    n = 4
    res = EvalResult(torch.ones(n, dtype=torch.int32), torch.ones(1, n), torch.full((1, n), 5, dtype=torch.int32),
                     torch.full((1, n), EVAL_LANDED, dtype=torch.uint8), torch.zeros(1, n),
                     torch.arange(14.0)[None, :, None].expand(1, 14, n).contiguous(), STATE_NAMES_6DOF)
    s = res.stats()
    assert s["ep_statistic/landing_success"] == 1.0 and s["unfinished"] == 0 and s["std_reward"] == 0.0
    assert [s["final_errors/" + name] for name in STATE_NAMES_6DOF] == [float(k) for k in range(14)]
