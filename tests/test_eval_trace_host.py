"""rr_policy_evaluate_trace's host side (no GPU): the C declaration, its ctypes mirror and the
unchanged ABI number; the call refuses bad arguments before any HIP call; EvalTrace /
EpisodeRecord give the reference's per-episode views on hand-made CPU tensors."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

from rl_rocket_amd import _lib

FIELDS = ["slot", "n_slots", "steps", "state", "action", "terms", "length"]


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)


# ---- 1. header, ctypes and library agree ----------------------------------------------------------------

def test_header_declares_the_entry_point_and_the_struct():
    code = _header_code()
    m = re.search(r"int\s+rr_policy_evaluate_trace\s*\(([^;]*)\)\s*;", code)
    assert m, "rr_policy_evaluate_trace is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[0].startswith("rr_env*")
    assert "rr_eval_out" in args[5] and "rr_eval_trace" in args[6]
    assert re.search(r"typedef\s+struct\s+rr_eval_trace\s*\{", code)
    res, argtypes = _lib.SIGNATURES["rr_policy_evaluate_trace"]
    assert res is ctypes.c_int and len(argtypes) == 9
    assert argtypes[5] == ctypes.POINTER(_lib.RrEvalOut) and argtypes[6] == ctypes.POINTER(_lib.RrEvalTrace)
    assert argtypes[2:5] == [ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    # the plain entry point is declared as before
    assert _lib.SIGNATURES["rr_policy_evaluate"][1][5] == ctypes.POINTER(_lib.RrEvalOut)
    assert len(_lib.SIGNATURES["rr_policy_evaluate"][1]) == 8


def test_ctypes_mirror_has_the_header_layout(tmp_path):
    assert [f[0] for f in _lib.RrEvalTrace._fields_] == FIELDS
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"rocket_hip.h\"\nint main(void){\n"
    src += 'printf("%zu\\n", sizeof(rr_eval_trace));\n'
    for f in FIELDS:
        src += 'printf("%%zu\\n", offsetof(rr_eval_trace, %s));\n' % f
    src += "return 0;}\n"
    c, exe = tmp_path / "l.c", tmp_path / "l"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.dirname(_lib.HEADER), str(c), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert ctypes.sizeof(_lib.RrEvalTrace) == vals[0]
    assert [getattr(_lib.RrEvalTrace, f).offset for f in FIELDS] == vals[1:]


def test_library_exports_the_symbol_and_the_abi_number_stays():
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT rr_policy_evaluate_trace\b", out)
    assert not re.search(r"rrc_launch_eval_trace", out)  # the cross-TU launcher stays hidden
    assert lib.rr_abi_version() == 14 and _lib.ABI_VERSION == 14
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", open(_lib.HEADER).read())


# ---- 2. argument checks, before any HIP call ------------------------------------------------------------

def _trace(null=None, n_slots=4, steps=8):
    """An rr_eval_trace of fake non-null device pointers (never dereferenced: every call below is
    refused before it launches)."""
    vals = dict(slot=0x10000, state=0x20000, action=0x30000, terms=0x40000, length=0x50000)
    if null:
        vals[null] = None
    return _lib.RrEvalTrace(n_slots=n_slots, steps=steps, **vals)


def test_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    V = ctypes.c_void_p
    out = _lib.RrEvalOut(episodes=0x60000)
    params = V(0x70000)  # 16-B aligned
    handle = V(0x80000)  # never dereferenced: the checks below come before anything reads it

    def refused(rc):
        assert rc == _lib.RR_EINVAL
        msg = lib.rr_last_error()
        assert msg.startswith(b"rr_policy_evaluate_trace: ") and len(msg) > 36, msg

    tr = _trace()
    refused(lib.rr_policy_evaluate_trace(None, params, 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None))
    assert b"handle" in lib.rr_last_error()
    h = handle
    refused(lib.rr_policy_evaluate_trace(h, params, 0, 1, 10, ctypes.byref(out), None, None, None))
    assert b"trace" in lib.rr_last_error()
    for null in ("slot", "state", "length"):
        tr = _trace(null=null)
        refused(lib.rr_policy_evaluate_trace(h, params, 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None))
        assert null.encode() in lib.rr_last_error()
    for kw in (dict(n_slots=0), dict(steps=0)):
        tr = _trace(**kw)
        refused(lib.rr_policy_evaluate_trace(h, params, 0, 1, 10, ctypes.byref(out), ctypes.byref(tr), None, None))
        assert list(kw)[0].encode() in lib.rr_last_error()
    # the plain call's messages keep their own prefix
    assert lib.rr_policy_evaluate(None, params, 0, 1, 10, ctypes.byref(out), None, None) == _lib.RR_EINVAL
    assert lib.rr_last_error().startswith(b"rr_policy_evaluate: ")


# ---- 3. EvalTrace / EpisodeRecord on hand-made CPU tensors ----------------------------------------------

def _cfg(model):
    from rl_rocket_amd.params import config_3dof, config_6dof

    return config_6dof() if model == 6 else config_3dof()


def _hand_made(model, lengths=((5, 3), (4, 6)), cap=6, episodes=None):
    """K = 2 recorded envs (ids 9 and 2), 2 episodes, capacity 6, filled with a smooth made-up
    descent: x / z falls from above the waypoint to below it, so v_targ takes both branches."""
    import torch
    from rl_rocket_amd.eval_trace import EvalTrace

    cfg = _cfg(model)
    ns, na, nt = cfg.state_dim, cfg.action_dim, len(cfg.term_names)
    g = torch.Generator().manual_seed(7)
    K, ne = 2, 2
    state = torch.rand((K, ne, cap + 1, ns), generator=g) - 0.5
    alt = 0 if model == 6 else 1
    wp = float(cfg.extra["waypoint"])
    state[..., alt] = torch.linspace(wp + 40.0, max(wp - 40.0, 1.0), cap + 1)
    state[..., -1] = torch.linspace(40e3, 39e3, cap + 1)  # mass
    action = torch.rand((K, ne, cap, na), generator=g) * 2 - 1
    terms = torch.rand((K, ne, cap, nt + 1), generator=g)
    length = torch.tensor(lengths, dtype=torch.int32).T.contiguous()  # [ne, K]
    tr = EvalTrace(cfg, state, action, terms, length, torch.tensor([9, 2]), episodes=episodes)
    return cfg, tr


@pytest.mark.parametrize("model", [6, 3])
def test_episode_record_views(model):
    from rl_rocket_amd import envs
    from rl_rocket_amd.params import (ACTION_NAMES_3DOF, ACTION_NAMES_6DOF, MAX_GIMBAL, MAX_THRUST, STATE_NAMES_3DOF,
                                      STATE_NAMES_6DOF)

    cfg, tr = _hand_made(model)
    ns, na, nt = cfg.state_dim, cfg.action_dim, len(cfg.term_names)
    snames = STATE_NAMES_6DOF if model == 6 else STATE_NAMES_3DOF
    anames = ACTION_NAMES_6DOF if model == 6 else ACTION_NAMES_3DOF
    rec = tr.episode(2, k=1)  # slot 1, episode 1: 6 steps
    L = 6
    assert len(rec) == L and rec.length == L and rec.complete and rec.env_id == 2 and rec.episode == 1
    assert rec.states.shape == (L + 1, ns) and rec.states.dtype == np.float32
    assert np.array_equal(rec.states, tr.state[1, 1, :L + 1].numpy())
    assert np.array_equal(rec.rewards, tr.terms[1, 1, :L, nt].numpy()) and rec.rewards.shape == (L,)
    rd = rec.rewards_dict
    assert len(rd) == L and all(list(d) == list(cfg.term_names) for d in rd)
    assert rd[3][cfg.term_names[1]] == float(tr.terms[1, 1, 3, 1])
    assert rec.used_mass() == tr.state[1, 1, 0, -1].numpy() - tr.state[1, 1, L, -1].numpy()
    sdf = rec.states_to_dataframe()
    assert sdf.shape == (L + 1, ns) and list(sdf.columns) == list(snames)
    adf = rec.actions_to_dataframe()
    assert adf.shape == (L + 1, na) and list(adf.columns) == list(anames)
    assert (adf.iloc[0] == 0).all()
    a = tr.action[1, 1, :L].numpy()
    want = np.stack([a[:, j] * np.float32(1) * MAX_GIMBAL for j in range(na - 1)] + [(a[:, -1] + 1) / 2.0 * MAX_THRUST],
                    axis=1).astype(np.float32)
    assert np.array_equal(adf.iloc[1:].to_numpy(dtype=np.float32), want)
    rdf = rec.rewards_to_dataframe()
    assert rdf.shape == (L, nt) and list(rdf.columns) == list(cfg.term_names)
    # v_targ: the single-env shim's _compute_vtarg on the same float32 states
    shim_cls = envs.Rocket6DOF if model == 6 else envs.Rocket
    shim = types.SimpleNamespace(SIM=types.SimpleNamespace(states=[s for s in rec.states]),
                                 waypoint=cfg.extra["waypoint"])
    want_vt = np.array([shim_cls._compute_vtarg(shim, np.asarray(s, np.float32)) for s in rec.states[1:]])
    vdf = rec.vtarg_to_dataframe()
    assert vdf.shape == (L, 3 if model == 6 else 2)
    assert list(vdf.columns) == (["v_x", "v_y", "v_z"] if model == 6 else ["v_x", "v_y"])
    assert np.array_equal(vdf.to_numpy(), want_vt)
    alt = rec.states[1:, 0 if model == 6 else 1]
    assert (alt > cfg.extra["waypoint"]).any() and (alt <= cfg.extra["waypoint"]).any()  # both branches
    # a shorter episode: only its rows
    short = tr.episode(9, k=1)
    assert len(short) == 3 and short.states.shape == (4, ns) and short.actions_to_dataframe().shape == (4, na)


@pytest.mark.parametrize("model", [6, 3])
def test_analyzer_log_has_the_reference_keys(model):
    from rl_rocket_amd.eval_trace import ANALYZER_KEYS
    from rl_rocket_amd.params import STATE_NAMES_3DOF, STATE_NAMES_6DOF

    cfg, tr = _hand_made(model)
    rec = tr.episode(9, k=0)
    log = rec.analyzer_log()
    names = STATE_NAMES_6DOF if model == 6 else STATE_NAMES_3DOF
    # wrappers.py:216-226
    assert set(log) == {"ep_history/states", "ep_history/actions", "ep_history/vtarg", "ep_history/rewards",
                        "plots3d/vtarg_trajectory", "plots3d/trajectory", "ep_statistic/landing_success",
                        "ep_statistic/used_mass"} | {"final_errors/" + n for n in names}
    assert set(ANALYZER_KEYS) <= set(log)
    assert log["ep_statistic/landing_success"] == rec.rewards_dict[-1]["rew_goal"]
    assert log["ep_statistic/used_mass"] == rec.used_mass()
    assert log["final_errors/mass"] == abs(rec.states[-1][-1])
    pytest.importorskip("plotly")
    import plotly.graph_objects as go

    assert isinstance(log["ep_history/states"], go.Figure) and len(log["ep_history/states"].data) == cfg.state_dim
    if model == 6:
        assert isinstance(log["plots3d/trajectory"], go.Figure)
        assert isinstance(rec.get_vtarg_trajectory(), go.Figure) and isinstance(rec.get_attitude_trajectory(), go.Figure)
    else:
        with pytest.raises(NotImplementedError):
            rec.get_trajectory_plotly()


def test_episode_refuses_unfinished_and_clipped_records():
    import torch

    # env 9 (slot 0) finished one episode, env 2 (slot 1) none; episode 1 of env 2 ran 9 > 6 steps
    episodes = torch.zeros(16, dtype=torch.int32)
    episodes[9] = 1
    cfg, tr = _hand_made(6, lengths=((5, 3), (4, 9)), episodes=episodes)
    assert len(tr.episode(9, k=0)) == 5
    with pytest.raises(ValueError, match="did not finish"):
        tr.episode(9, k=1)
    part = tr.episode(9, k=1, partial=True)
    assert len(part) == 3 and not part.complete
    with pytest.raises(ValueError, match="did not finish"):
        tr.episode(2, k=0)
    with pytest.raises(ValueError, match="did not finish"):
        tr.episode(2, k=1, partial=True)  # not even begun
    with pytest.raises(KeyError):
        tr.episode(3)
    episodes[2] = 2
    with pytest.raises(ValueError, match="record holds 6"):
        tr.episode(2, k=1)
    clip = tr.episode(2, k=1, clipped=True)
    assert len(clip) == 6 and clip.length == 9 and not clip.complete and clip.states.shape == (7, 14)


def test_record_indices_are_validated():
    import torch
    from rl_rocket_amd.rollout import PolicyEvaluator

    cfg = _cfg(3)
    env = types.SimpleNamespace(num_envs=16, device=torch.device("cpu"), cfg=cfg, state_dim=7, action_dim=2, n_terms=6,
                                params=types.SimpleNamespace(max_episode_steps=8))
    ev = types.SimpleNamespace(env=env, n_episodes=2, episodes=torch.zeros(16, dtype=torch.int32))
    make = PolicyEvaluator._make_trace
    with pytest.raises(ValueError, match="twice"):
        make(ev, [3, 5, 3], None)
    with pytest.raises(ValueError, match="outside"):
        make(ev, [3, 16], None)
    with pytest.raises(ValueError, match="outside"):
        make(ev, torch.tensor([-1, 2]), None)
    env.params.max_episode_steps = 0
    with pytest.raises(ValueError, match="record_steps"):
        make(ev, [3], None)
    assert make(ev, None, None) is None
    tr = make(ev, torch.tensor([15, 0, 7]), 5)  # any order
    assert tr.state.shape == (3, 2, 6, 7) and tr.action.shape == (3, 2, 5, 2) and tr.terms.shape == (3, 2, 5, 7)
    assert tr.length.shape == (2, 3) and tr.length.dtype == torch.int32 and tr.env_ids.tolist() == [15, 0, 7]
    slot = ev._slot
    assert slot.dtype == torch.int32 and slot.tolist() == [1, -1, -1, -1, -1, -1, -1, 2, -1, -1, -1, -1, -1, -1, -1, 0]


# ---- 4. the recording kernel's register budget, from the built library's kernel descriptors ------------

def _code_objects(lib, d):
    """The gfx950 code objects of `lib` (one per translation unit), unbundled into directory `d`."""
    from rl_rocket_amd import build as B

    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    fat = os.path.join(d, "fat.bin")
    subprocess.check_call([B._llvm("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, lib, os.path.join(d, "x")])
    blob = open(fat, "rb").read()
    starts, k = [], blob.find(magic)
    while k >= 0:
        starts.append(k)
        k = blob.find(magic, k + len(magic))
    out = []
    for i, k0 in enumerate(starts):
        part, co = os.path.join(d, "b%d.bin" % i), os.path.join(d, "b%d.co" % i)
        open(part, "wb").write(blob[k0:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.check_call([B._llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                               "--targets=hipv4-amdgcn-amd-amdhsa--%s" % B.ARCH, "--output=" + co])
        out.append(co)
    return out


def _kernel_descriptors(lib):
    """{demangled kernel name: its 64-byte kernel descriptor} of every gfx950 code object in `lib`."""
    import tempfile
    from rl_rocket_amd import build as B

    kds = {}
    with tempfile.TemporaryDirectory() as d:
        for co in _code_objects(lib, d):
            kds.update({n[:-3]: v for n, v in B._elf_symbols(open(co, "rb").read()).items() if n.endswith(".kd")})
    names = sorted(kds)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return {p: kds[m] for m, p in zip(names, plain.splitlines())}


def test_trace_arguments_sit_where_the_kernel_reads_them(tmp_path):
    """eval_trace_kernel reads its trace arguments from the kernel-argument segment at kTraceArgOff,
    computed as if the parameters were the members of a C struct (rocket_eval.inc). The code
    object's metadata must lay them out that way: every explicit argument at the previous one's end
    rounded up to 8 bytes, the last one (EvalTraceIO, 48 bytes) included."""
    from rl_rocket_amd import build as B

    seen = 0
    for co in _code_objects(B.OUT, str(tmp_path)):
        notes = subprocess.run([B._llvm("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
        for blk in re.findall(r"\.args:(.*?)\.group_segment_fixed_size:(?:.*?)\.name:\s+(\S+)", notes, re.S):
            body, name = blk
            if "eval_trace_kernel" not in name:
                continue
            args = [(int(o), int(sz)) for o, sz, kind in
                    re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+(\w+)", body)
                    if not kind.startswith("hidden")]
            assert len(args) == 7 and args[0] == (0, 8) and args[-1][1] == ctypes.sizeof(_lib.RrEvalTrace), (name, args)
            for (o0, s0), (o1, _s1) in zip(args[2:], args[3:]):  # the four structs after the three leading words
                assert o1 == (o0 + s0 + 7) // 8 * 8, (name, args)
            seen += 1
    assert seen == 12


def test_recording_kernel_keeps_two_waves_per_simd_and_no_scratch():
    """eval_trace_kernel<6, RK4, fp32> against eval_kernel<6, RK4, fp32>: no scratch, and at most 256
    unified registers (two waves per SIMD), as the plain kernel. From the kernel descriptors:
    private_segment_fixed_size (bytes 4..8) and compute_pgm_rsrc1's granulated VGPR count (bits 0..5
    of the word at byte 48; gfx90a and later: blocks of 8 registers, AGPRs included)."""
    import struct
    from rl_rocket_amd import build as B

    kds = _kernel_descriptors(B.OUT)

    def budget(prefix):
        kd, = [v for k, v in kds.items() if prefix in k]
        scratch, = struct.unpack_from("<I", kd, 4)
        rsrc1, = struct.unpack_from("<I", kd, 48)
        return scratch, ((rsrc1 & 0x3F) + 1) * 8

    plain, trace = budget("::eval_kernel<6, 0, 0>("), budget("::eval_trace_kernel<6, 0, 0>(")
    assert plain == (0, 256)  # 254 VGPRs, allocated in blocks of 8
    assert trace[0] == 0 and trace[1] <= 256
    for k in kds:
        if "eval_trace_kernel<" in k:
            assert struct.unpack_from("<I", kds[k], 4)[0] == 0, k  # no instantiation uses scratch
