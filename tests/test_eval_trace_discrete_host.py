"""The host side of the Categorical policy's recording evaluation, rr_policy_evaluate_discrete_trace (no GPU):
the C declaration, its ctypes mirror, the export and the unchanged ABI number; every refusal of the call is
reached with fake pointers before the handle is read; EvalTrace / EpisodeRecord / Demonstrations.from_trace with
a `choice` plane on hand-made CPU tensors; and the constructor's messages on stub batches."""
import ctypes
import re
import subprocess
import types

import numpy as np
import pytest

from rl_rocket_amd import _lib

NAME, TWIN = "rr_policy_evaluate_discrete_trace", "rr_policy_evaluate_discrete"


def test_declared_in_header_abi_14():
    with open(_lib.HEADER) as f:
        text = f.read()
    assert re.search(r"#define\s+RR_ABI_VERSION\s+14\b", text) and _lib.ABI_VERSION == 14
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = {}
    for name in (NAME, TWIN, "rr_policy_evaluate_trace"):
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name + " is not declared"
        decl[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    args, twin = decl[NAME], decl[TWIN]
    # rr_policy_evaluate_discrete's arguments plus (trace, choice) after out
    k = twin.index("const rr_eval_out* out") + 1
    assert args == twin[:k] + ["const rr_eval_trace* trace", "int32_t* choice"] + twin[k:]
    # and rr_policy_evaluate_trace's with (n_choices, table) after params and choice after trace
    tr = decl["rr_policy_evaluate_trace"]
    assert args == tr[:2] + ["int n_choices", "const float* table"] + tr[2:7] + ["int32_t* choice"] + tr[7:]
    res, argtypes = _lib.SIGNATURES[NAME]
    targtypes = _lib.SIGNATURES[TWIN][1]
    assert res is ctypes.c_int and len(argtypes) == len(args) == 12
    assert argtypes == targtypes[:k] + [ctypes.POINTER(_lib.RrEvalTrace), ctypes.c_void_p] + targtypes[k:]
    # rr_eval_trace itself is unchanged
    assert [f[0] for f in _lib.RrEvalTrace._fields_] == ["slot", "n_slots", "steps", "state", "action", "terms",
                                                         "length"]
    m = re.search(r"typedef\s+struct\s+rr_eval_trace\s*\{(.*?)\}\s*rr_eval_trace\s*;", code, flags=re.S)
    assert m and "choice" not in m.group(1) and len([x for x in m.group(1).split(";") if x.strip()]) == 7


def test_library_exports_it_and_keeps_the_launcher_hidden():
    lib = _lib.load()
    assert lib.rr_abi_version() == 14
    assert getattr(lib, NAME) is not None
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r"\bT %s\b" % NAME, out)
    assert not re.search(r"rrc_launch_eval_discrete_trace", out)


def test_unit_is_a_source_and_is_linked():
    from rl_rocket_amd import build as B

    assert B.SRC_EVAL_TRACE_DISCRETE in B.sources()
    assert B.SRC_EVAL_TRACE_DISCRETE in B.commands()[-1]


def test_c_abi_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    V = ctypes.c_void_p
    fake = V(0x10000)
    table = (ctypes.c_float * 8)(0, -1, -1, 1, 0, 1, 1, 1)
    out = _lib.RrEvalOut(0x20000, None, None, None, None, None)

    def trace(null=None, n_slots=4, steps=8):
        vals = dict(slot=0x30000, state=0x40000, action=0x50000, terms=0x60000, length=0x70000)
        if null:
            vals[null] = None
        return _lib.RrEvalTrace(n_slots=n_slots, steps=steps, **vals)

    def refused(rc, word):
        msg = lib.rr_last_error().decode()
        assert rc == _lib.RR_EINVAL and msg.startswith(NAME + ": ") and word in msg, (rc, msg)

    def call(h=None, params=fake, k=4, tab=table, prec=0, ne=1, o=out, tr=trace(), choice=V(0x80000)):
        return getattr(lib, NAME)(h, params, k, tab, prec, ne, 0, ctypes.byref(o) if o else None,
                                  ctypes.byref(tr) if tr else None, choice, None, None)

    # what rr_policy_evaluate_discrete refuses
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
    refused(call(ne=0), "n_episodes")
    refused(call(o=None), "out")
    refused(call(o=_lib.RrEvalOut()), "episodes")
    # what rr_policy_evaluate_trace refuses
    refused(call(tr=None), "trace")
    for null in ("slot", "state", "length"):
        refused(call(tr=trace(null=null)), null)
    refused(call(tr=trace(n_slots=0)), "n_slots")
    refused(call(tr=trace(steps=0)), "steps")
    # the choice plane
    refused(call(choice=V(0x80002)), "4-B aligned")
    # with a non-null handle that is never read: the same refusals
    refused(call(h=fake, tr=None), "trace")
    refused(call(h=fake, k=1), "2 .. 4")
    refused(call(h=fake, tr=trace(steps=0)), "steps")
    # and with everything in order, the handle; action, terms and choice are optional
    refused(call(), "null handle")
    refused(call(choice=None), "null handle")
    refused(call(tr=trace(null="action")), "null handle")
    refused(call(tr=trace(null="terms")), "null handle")


# ---- EvalTrace / EpisodeRecord / Demonstrations with a choice plane, on CPU tensors ----

def _hand_made(lengths=((5, 3), (4, 6)), cap=6, episodes=None, choice=True):
    """K = 2 recorded envs (ids 9 and 2), 2 episodes, capacity 6 of the 3DOF env; the action rows are the table
    rows of the choice plane. lengths[s][k]: steps of episode k of slot s."""
    import torch
    from rl_rocket_amd.eval_trace import EvalTrace
    from rl_rocket_amd.params import config_3dof
    from rl_rocket_amd.policy import DISCRETE_TABLE_3DOF

    cfg = config_3dof()
    ns, nt = cfg.state_dim, len(cfg.term_names)
    g = torch.Generator().manual_seed(7)
    K, ne = 2, 2
    state = torch.rand((K, ne, cap + 1, ns), generator=g) - 0.5
    state[..., 1] = torch.linspace(float(cfg.extra["waypoint"]) + 40.0, 1.0, cap + 1)
    state[..., -1] = torch.linspace(40e3, 39e3, cap + 1)
    ch = torch.randint(0, 4, (K, ne, cap), generator=g, dtype=torch.int32)
    table = torch.tensor(DISCRETE_TABLE_3DOF, dtype=torch.float32)
    action = table[ch.long()]
    terms = torch.rand((K, ne, cap, nt + 1), generator=g)
    length = torch.tensor(lengths, dtype=torch.int32).T.contiguous()  # [ne, K]
    kw = dict(choice=ch) if choice else {}
    return cfg, EvalTrace(cfg, state, action, terms, length, torch.tensor([9, 2]), episodes=episodes, **kw), table


def test_choice_is_a_trailing_keyword_and_none_for_a_gaussian_trace():
    import inspect

    from rl_rocket_amd.eval_trace import EpisodeRecord, EvalTrace

    assert list(inspect.signature(EvalTrace.__init__).parameters)[-1] == "choice"
    assert inspect.signature(EvalTrace.__init__).parameters["choice"].default is None
    assert list(inspect.signature(EpisodeRecord.__init__).parameters)[-1] == "choices"
    _, tr, _ = _hand_made(choice=False)
    assert tr.choice is None
    rec = tr.episode(9, 0)
    assert rec.choices is None and len(rec) == 5


def test_episode_returns_choices():
    _, tr, table = _hand_made()
    for env_id, s in ((9, 0), (2, 1)):
        for k in range(2):
            rec = tr.episode(env_id, k)
            L = int(tr.length[k, s])
            assert len(rec) == L == rec.length and rec.complete
            assert rec.choices.dtype == np.int32 and rec.choices.shape == (L,)
            assert rec.choices.tolist() == tr.choice[s, k, :L].tolist()
            assert np.array_equal(rec.actions, table.numpy()[rec.choices])  # the rows the env stepped with
            assert rec.states.shape == (L + 1, 7)
    # the frames of the reference's analyzer take a 3DOF record as before
    rec = tr.episode(9, 0)
    assert rec.actions_to_dataframe().shape == (6, 2) and len(rec.rewards_dict) == 5


def test_partial_and_clipped_episodes_behave_as_the_other_planes():
    import torch

    # env 9 finished one episode and took 3 steps of its second; env 2 finished both
    episodes = torch.zeros(10, dtype=torch.int32)
    episodes[9], episodes[2] = 1, 2
    _, tr, _ = _hand_made(episodes=episodes)
    with pytest.raises(ValueError, match="partial=True"):
        tr.episode(9, 1)
    rec = tr.episode(9, 1, partial=True)
    assert not rec.complete and len(rec) == 3 and rec.choices.tolist() == tr.choice[0, 1, :3].tolist()
    # an episode of 9 steps in a record of 6
    _, tr, _ = _hand_made(lengths=((9, 3), (4, 6)))
    with pytest.raises(ValueError, match="clipped=True"):
        tr.episode(9, 0)
    rec = tr.episode(9, 0, clipped=True)
    assert not rec.complete and rec.length == 9 and len(rec) == 6
    assert rec.choices.tolist() == tr.choice[0, 0].tolist() and rec.actions.shape == (6, 2)


def test_demonstrations_from_a_trace_with_choices():
    import torch
    from rl_rocket_amd.bc import Demonstrations, _check_indices

    episodes = torch.zeros(10, dtype=torch.int32)
    episodes[9], episodes[2] = 1, 2  # slot 0's second episode is partial: left out whole
    cfg, tr, _ = _hand_made(lengths=((5, 3), (9, 6)), episodes=episodes)  # slot 1's first episode is clipped
    batch = types.SimpleNamespace(cfg=cfg)
    demos = Demonstrations.from_trace(tr, batch)
    # slot, episode, step order: slot 0 episode 0 (5 steps), slot 1 episode 1 (6 steps)
    want = torch.cat([tr.choice[0, 0, :5], tr.choice[1, 1, :6]]).float()[:, None]
    assert demos.acts.shape == (11, 1) and demos.acts.dtype == torch.float32 and demos.acts.is_contiguous()
    assert torch.equal(demos.acts, want)
    _check_indices(demos.acts, 4)
    inv = torch.tensor((1.0 / np.asarray(cfg.state_normalizer, dtype=np.float64)).astype(np.float32))[:7]
    assert torch.equal(demos.obs, torch.cat([tr.state[0, 0, :5], tr.state[1, 1, :6]]) * inv)
    # a Gaussian trace (choice=None) gives what it gives today: the action rows, same mask and order
    _, tg, _ = _hand_made(lengths=((5, 3), (9, 6)), episodes=episodes, choice=False)
    dg = Demonstrations.from_trace(tg, batch)
    assert torch.equal(dg.acts, torch.cat([tg.action[0, 0, :5], tg.action[1, 1, :6]])) and dg.acts.shape == (11, 2)
    assert torch.equal(dg.obs, demos.obs)


# ---- the constructor ----

def _stub_batch(dof=3, device="cpu"):
    ns, na = (7, 2) if dof == 3 else (14, 3)
    return types.SimpleNamespace(num_envs=8, state_dim=ns, action_dim=na, device=device, model=dof)


def test_constructor_messages_on_stub_batches():
    """record= first asks for a real batch (one with params), before the device and the integrator."""
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic, PolicyEvaluator

    pol = MlpCategoricalActorCritic(7, 4)
    for dev in ("cpu", "cuda:0"):
        b = _stub_batch(device=dev)
        for kw in (dict(), dict(fused=True), dict(fused=False)):
            with pytest.raises(ValueError, match="record=.*RocketBatch"):
                PolicyEvaluator(b, pol, record=[0], **kw)
        with pytest.raises(ValueError, match="3DOF"):
            PolicyEvaluator(_stub_batch(6, dev), pol, record=[0], fused=True)
        with pytest.raises(ValueError, match="policy_dtype='bf16'"):
            real = _stub_batch(device=dev)
            real.params = types.SimpleNamespace(integrator=0, flags=0x1, max_episode_steps=8)
            PolicyEvaluator(real, pol, record=[0], fused=True, policy_dtype="bf16")
    # with params, the fused launch's own conditions follow in their order: the device, the integrator
    cpu = _stub_batch()
    cpu.params = types.SimpleNamespace(integrator=0, flags=0x1, max_episode_steps=8)
    with pytest.raises(ValueError, match="fused=True.*CUDA"):
        PolicyEvaluator(cpu, pol, record=[0], fused=True)
    dop = _stub_batch(device="cuda:0")
    dop.params = types.SimpleNamespace(integrator=2, flags=0x1, max_episode_steps=8)
    with pytest.raises(ValueError, match="fused=True.*dopri5"):
        PolicyEvaluator(dop, pol, record=[0], fused=True)
