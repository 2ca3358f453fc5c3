"""rr_rollout_collect_stats's host side (no GPU): the block-to-dict function on hand-written blocks,
the C declarations and their ctypes mirrors, the refusals that come before any HIP call, and the
build's sixth translation unit."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from rl_rocket_amd import _lib
from rl_rocket_amd import build as B
from rl_rocket_amd import rollout_stats as S

NAMES = ("rr_rollout_stats_rows", "rr_rollout_collect_stats")


def test_dict_of_a_block_without_episodes():
    b = S.make_block(ints={_lib.RR_RSTAT_SAMPLES: 4},
                     floats={_lib.RR_RSTAT_Y_SUM: 10.0, _lib.RR_RSTAT_Y_SQ: 30.0,   # y = 1, 2, 3, 4
                             _lib.RR_RSTAT_D_SUM: 0.0, _lib.RR_RSTAT_D_SQ: 1.0})    # d = .5, -.5, .5, -.5
    d = S.stats_dict(b)
    # SB3 logs no episode figure without an episode
    assert sorted(d) == ["rollout/episodes", "train/explained_variance"]
    assert d["rollout/episodes"] == 0
    assert d["train/explained_variance"] == pytest.approx(1.0 - 0.25 / 1.25, rel=1e-15)
    e = S.stats_dict(S.empty_block())  # no sample either
    assert e["rollout/episodes"] == 0 and math.isnan(e["train/explained_variance"]) and len(e) == 2


def test_dict_where_the_returns_do_not_vary():
    b = S.make_block(ints={_lib.RR_RSTAT_SAMPLES: 4},
                     floats={_lib.RR_RSTAT_Y_SUM: 8.0, _lib.RR_RSTAT_Y_SQ: 16.0,    # y = 2, 2, 2, 2
                             _lib.RR_RSTAT_D_SUM: 1.0, _lib.RR_RSTAT_D_SQ: 1.0})
    assert math.isnan(S.stats_dict(b)["train/explained_variance"])  # Var(y) = 0: NaN, as SB3


def test_dict_of_an_ordinary_block():
    rets = np.array([-3.0, 1.0, 2.0, 8.0])
    b = S.make_block(ints={_lib.RR_RSTAT_EPISODES: 4, _lib.RR_RSTAT_LEN_SUM: 50, _lib.RR_RSTAT_LANDED: 1,
                           _lib.RR_RSTAT_END_EVENT: 2, _lib.RR_RSTAT_END_BOUNDS: 1, _lib.RR_RSTAT_END_TRUNCATED: 1,
                           _lib.RR_RSTAT_END_NONFINITE: 0, _lib.RR_RSTAT_SAMPLES: 8},
                     floats={_lib.RR_RSTAT_RET_SUM: rets.sum(), _lib.RR_RSTAT_RET_SQ: (rets * rets).sum(),
                             _lib.RR_RSTAT_RET_MIN: -3.0, _lib.RR_RSTAT_RET_MAX: 8.0,
                             _lib.RR_RSTAT_Y_SUM: 8.0, _lib.RR_RSTAT_Y_SQ: 40.0,     # Var(y) = 4
                             _lib.RR_RSTAT_D_SUM: 8.0, _lib.RR_RSTAT_D_SQ: 16.0})    # Var(d) = 1
    d = S.stats_dict(b)
    assert d == {"rollout/episodes": 4, "rollout/ep_rew_mean": 2.0, "rollout/ep_rew_std": pytest.approx(rets.std()),
                 "rollout/ep_rew_min": -3.0, "rollout/ep_rew_max": 8.0, "rollout/ep_len_mean": 12.5,
                 "rollout/success_rate": 0.25, "rollout/end_event": 0.5, "rollout/end_bounds": 0.25,
                 "rollout/end_truncated": 0.25, "rollout/end_nonfinite": 0.0, "train/explained_variance": 0.75}
    # a block may arrive as float64 words too
    assert S.stats_dict(b.view(np.float64)) == d
    with pytest.raises(ValueError):
        S.stats_dict(np.zeros(15, dtype=np.int64))


def test_fold_of_blocks():
    a = S.make_block(ints={0: 2, 15: 8}, floats={7: 1.5, 9: -1.0, 10: 2.0})
    b = S.make_block(ints={0: 3, 15: 8}, floats={7: 2.5, 9: 0.5, 10: 7.0})
    f = S.fold_blocks([a, S.empty_block(), b])
    assert np.array_equal(f, S.make_block(ints={0: 5, 15: 16}, floats={7: 4.0, 9: -1.0, 10: 7.0}))
    assert np.array_equal(S.fold_blocks([]), S.empty_block())


def test_header_declares_the_entry_points_and_signatures_mirror_them_abi_14():
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES
    m = re.search(r"int64_t\s+rr_rollout_stats_rows\s*\(\s*int64_t\s+n\s*\)\s*;", code)
    assert m and _lib.SIGNATURES["rr_rollout_stats_rows"] == (ctypes.c_int64, [ctypes.c_int64])
    m = re.search(r"int\s+rr_rollout_collect_stats\s*\(([^;]*)\)\s*;", code)
    plain = re.search(r"int\s+rr_rollout_collect\s*\(([^;]*)\)\s*;", code)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    pargs = [" ".join(a.split()) for a in plain.group(1).split(",")]
    # rr_rollout_collect's arguments, then the statistics, then the stream
    assert args[:-2] == pargs[:-1] and args[-1] == pargs[-1] == "void* stream"
    assert args[-2] == "const rr_rollout_stats* stats"
    res, argtypes = _lib.SIGNATURES["rr_rollout_collect_stats"]
    pres, pargtypes = _lib.SIGNATURES["rr_rollout_collect"]
    assert res is pres is ctypes.c_int and len(argtypes) == len(args) == 26
    assert argtypes[:-2] == pargtypes[:-1] and argtypes[-2] == ctypes.POINTER(_lib.RrRolloutStats)
    # the struct and the slot enum
    body = re.search(r"typedef\s+struct\s+rr_rollout_stats\s*\{(.*?)\}\s*rr_rollout_stats\s*;", code, re.S).group(1)
    assert re.findall(r"void\s*\*\s*(\w+)\s*;", body) == [f[0] for f in _lib.RrRolloutStats._fields_]
    assert ctypes.sizeof(_lib.RrRolloutStats) == 24
    enum = re.findall(r"\b(RR_RSTAT_[A-Z_]+)\b", code[code.index("RR_RSTAT_EPISODES = 0"):code.index("RR_RSTAT_SLOTS") + 20])
    assert len(enum) == 17 and [getattr(_lib, k) for k in enum] == list(range(17))
    assert _lib.RR_RSTAT_INT_SLOTS == (0, 1, 2, 3, 4, 5, 6, 15)


def test_library_exports_the_symbols_and_keeps_the_launcher_hidden():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out)
    assert not re.search(r"rrc_launch_collect_stats", out)
    assert lib.rr_abi_version() == 14
    assert [lib.rr_rollout_stats_rows(n) for n in (-3, 0, 1, 64, 65, 300, 65536)] == [0, 0, 1, 1, 2, 5, 1024]


def test_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    V = ctypes.c_void_p
    h = V(0x80000)  # never dereferenced: the checks below come before anything reads it
    ok = _lib.RrRolloutStats(partials=0x10080, out=0x20008, accum=0x30008)

    def call(e=h, T=16, adv=V(0x40000), ret=V(0x50000), st=ok):
        p = V(0x70000)
        return lib.rr_rollout_collect_stats(e, p, 0, 1, p, T, 0.99, 0.95, p, p, p, p, p, p, adv, ret, p, p, p, p, p, p, p, p,
                                            None if st is None else ctypes.byref(st), None)

    def refused(rc, word):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(b"rr_rollout_collect_stats: ") and word in msg, msg

    refused(call(e=None), b"handle")
    refused(call(T=0), b"n_steps")
    refused(call(st=None), b"stats")
    refused(call(st=_lib.RrRolloutStats(partials=0, out=0x20008)), b"partials")
    refused(call(st=_lib.RrRolloutStats(partials=0x10080, out=0)), b"out")
    refused(call(st=_lib.RrRolloutStats(partials=0x10040, out=0x20008)), b"128-B")
    refused(call(st=_lib.RrRolloutStats(partials=0x10080, out=0x20004)), b"8-B")
    refused(call(st=_lib.RrRolloutStats(partials=0x10080, out=0x20008, accum=0x30004)), b"8-B")
    refused(call(adv=None), b"buf_advantage")
    refused(call(ret=None), b"buf_advantage")


def test_build_compiles_the_translation_unit_of_its_own():
    src = B.SRC_COLLECT_STATS
    csrc = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc")
    assert os.path.dirname(src) == os.path.join(csrc, "collect_stats") and os.path.isfile(src)
    assert src in B.sources() and B.sources() == sorted(B.sources())
    cmds = B.commands()
    # the last step compiles the unit and links the library: the five earlier steps' objects go in
    mine = [c for c in cmds if c[-1] == src]
    assert mine == [cmds[-1]] and "-shared" in cmds[-1] and "-c" not in cmds[-1]
    assert cmds[-1][cmds[-1].index("-o") + 1] == B.OUT
    for c in cmds[:-1]:
        assert "-c" in c and c[c.index("-o") + 1] in cmds[-1]
    for flag in B.COLLECT_FLAGS:  # the collect translation unit's code-generation setting
        assert flag in mine[0]
    assert not any(f in mine[0] for f in B.EXACT_FLAGS if f != "-mllvm")
    text = open(src).read()
    assert re.search(r"^#define RR_POL_PREFETCH_A 1$", text, flags=re.M)
    assert text.index("#define RR_POL_PREFETCH_A 1") < text.index('#include "rocket_policy.inc"')
    # every file of the new directory is a source; each includes only sources (files of csrc/, the
    # C-ABI header, or its own directory)
    names = os.listdir(os.path.dirname(src))
    assert sorted(names) == ["rocket_collect_stats.hip", "rocket_collect_stats.inc"]
    for f in names:
        p = os.path.join(os.path.dirname(src), f)
        assert p in B.sources()
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(p).read(), flags=re.M):
            found = [q for q in (os.path.join(os.path.dirname(p), inc), os.path.join(csrc, inc),
                                 os.path.join(os.path.dirname(_lib.HEADER), inc)) if os.path.isfile(q)]
            assert found and found[0] in B.sources(), inc
            assert not inc.endswith(".hip")


def test_stats_kernels_use_no_scratch_and_the_existing_kernels_are_all_there():
    """From the built library: the 12 instantiations of the statistics collect and the reduction use
    no scratch (private_segment_fixed_size, bytes 4..8 of the kernel descriptor), and the plain
    collect's 12 instantiations are still in the library beside them."""
    import struct
    import tempfile

    from test_eval_trace_host import _code_objects

    kds = {}
    with tempfile.TemporaryDirectory() as d:
        for co in _code_objects(B.OUT, d):
            kds.update({n[:-3]: v for n, v in B._elf_symbols(open(co, "rb").read()).items() if n.endswith(".kd")})
    names = sorted(kds)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    by_name = {p: kds[m] for m, p in zip(names, plain)}
    mine = [k for k in by_name if "rollout_collect_stats_kernel<" in k]
    assert len(mine) == 12 and len([k for k in by_name if "rollout_stats_reduce_kernel" in k]) == 1
    for k in by_name:
        if "rollout_collect_stats_kernel<" in k or "rollout_stats_reduce_kernel" in k:
            assert struct.unpack_from("<I", by_name[k], 4)[0] == 0, k
    assert len([k for k in by_name if re.search(r"rollout_step_kernel<\d, \d, \d, true, 2>", k)]) == 12
