"""Every arm of the host side's kernel choice launches the kernel it names.

The library picks a kernel instantiation from the handle's model, integrator and policy precision in
one dispatcher (csrc/rocket_device.h: dispatch_env / dispatch_env_prec), called from six launch
sites. A wrong arm launches a wrong kernel, which no machine-code comparison can see, so each case
here compares, bit for bit, two paths that reach their kernels through different launch sites, over
all 12 (model, integrator, precision) combinations and, for the step kernel, its three launch shapes
and both action layouts. n = 70 is one full and one ragged wave of one workgroup: the choice of arm
does not depend on n beyond the step kernel's shape thresholds."""
import pytest

import test_gpu_eval as E
from test_gpu_rollout import three_rollout_paths_agree
from test_gpu_step_entry import _bits, _kw, _same

pytestmark = pytest.mark.gpu

DEV = E.DEV
N = 70
MODELS, INTEGRATORS, PRECS = (6, 3), ("rk4", "euler"), ("fp32", "bf16", "fp16x3")
TL_EVAL = 6      # with E.NE = 2 episodes: 12 steps, every env truncates twice at the latest
STEP_TL, STEPS = 3, 8
WIDE = 16384 + N  # above kNarrowMaxN: four main waves per workgroup


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("model", MODELS)
def test_rollout_paths(model, integrator, prec):
    """rr_policy_act + rr_step (step_kernel), rr_rollout_step and rr_rollout_collect (the main and the
    collect unit's rollout_step_kernel): every buffer, env output, terminal row and the state, over
    two collects of 8 steps under TimeLimit 6."""
    three_rollout_paths_agree(model, prec, 8, n=N, integrator=integrator)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("model", MODELS)
def test_evaluation_paths(model, integrator, prec):
    """eval_kernel against a twin handle stepped with rr_rollout_step (tests/test_gpu_eval.py's
    comparison), and eval_trace_kernel recording envs 0 and 69 against eval_kernel (as
    tests/test_gpu_eval_trace.py::test_recording_does_not_disturb_the_evaluation): 2 episodes under
    TimeLimit 6."""
    import torch

    over = dict(max_episode_steps=TL_EVAL, integrator=integrator)
    steps = E.NE * TL_EVAL
    ref = E._reference(model, prec, N, tl=TL_EVAL, integrator=integrator)
    assert int(ref["episodes"].min()) == E.NE
    b, _, plain = E._evaluate(model, prec, N, max_steps=steps, **over)
    assert plain.trace is None
    E._compare(b, plain, ref, model)
    c, ev, res = E._evaluate(model, prec, N, max_steps=steps, record=[0, N - 1], **over)
    assert ev.fused and res.trace.env_ids.tolist() == [0, N - 1]
    for name in ("episodes", "ep_return", "ep_length", "flags", "used_mass", "final_state"):
        assert torch.equal(getattr(res, name), getattr(plain, name)), name
    for x, y in zip(E._aux(c), E._aux(b)):
        assert torch.equal(x, y)
    assert torch.equal(c.obs, b.obs)
    assert torch.equal(res.trace.length, res.ep_length[:, res.trace.env_ids])
    b.close()
    c.close()


def _step_handles(model, integrator, n, help_max, monkeypatch):
    """(row-major, action_soa, row-major without auto-reset) handles of one launch shape, reset."""
    from rl_rocket_amd.batch import RocketBatch

    if help_max is None:
        monkeypatch.delenv("RR_HELP_MAX_N", raising=False)
    else:
        monkeypatch.setenv("RR_HELP_MAX_N", help_max)  # read by rr_create
    hs = [RocketBatch(n, model=model, device=DEV, max_episode_steps=STEP_TL, integrator=integrator, episode_stats=True,
                      compute_terms=True, auto_reset=auto_reset, action_soa=soa, **_kw(model))
          for soa, auto_reset in ((False, True), (True, True), (False, False))]
    monkeypatch.delenv("RR_HELP_MAX_N", raising=False)
    for h in hs:
        h.seed(11)
        h.reset()
    return hs


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("model", MODELS)
def test_step_kernel_shapes_and_action_layouts(model, integrator, monkeypatch):
    """step_kernel's three launch shapes (helper waves with one main wave per workgroup, with four,
    and the plain kernel), 8 steps under TimeLimit 3. In each shape an action_soa handle fed the
    transposed actions equals the row-major one: outputs, terms, state, counter words, running returns
    and terminal rows. The shapes agree with each other on envs 0..69, whose trajectories depend on
    the seed, the env id, the counter word and the action only: without auto-reset (one kernel, no
    reset draw) and with it (the helper kernels against the plain one, as tests/test_gpu_step_entry.py
    at equal n)."""
    import torch

    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    na = 3 if model == 6 else 2
    acts = [torch.rand((WIDE, na), device=DEV, generator=g) * 2 - 1 for _ in range(STEPS)]
    runs = {}
    for shape, n, help_max in (("helper-narrow", N, None), ("helper-wide", WIDE, None), ("plain", N, "0")):
        row, soa, fixed = _step_handles(model, integrator, n, help_max, monkeypatch)
        seen, done_rows = [], 0
        for k, act in enumerate(acts):
            a = act[:n].contiguous()
            out_r, out_s = row.step(a), soa.step(a.T.contiguous())
            for name, x, y in zip(("obs", "reward", "done", "truncated"), out_r, out_s):
                _same(x, y, "%s: %s after step %d" % (shape, name, k))
            _same(row.terms, soa.terms, "%s: terms after step %d" % (shape, k))
            cr, cs = row.checkpoint(), soa.checkpoint()
            for key in ("state", "v0", "counter", "ep_return"):
                _same(cr[key], cs[key], "%s: %s after step %d" % (shape, key, k))
            for name, x, y in zip(("terminal obs", "return", "length"), row.copy_terminal(), soa.copy_terminal()):
                _same(x, y, "%s: %s after step %d" % (shape, name, k))
            done_rows += int(out_r[2].sum())
            out_f = fixed.step(a)
            seen.append([_bits(t[:N]).clone() for t in (*out_r, row.terms[:, :N].T, cr["state"][:, :N].T,
                                                        *out_f, fixed.terms[:, :N].T,
                                                        fixed.checkpoint()["state"][:, :N].T)])
        assert done_rows >= 2 * n  # TimeLimit 3 over 8 steps: every env was reset twice
        runs[shape] = seen
        for h in (row, soa, fixed):
            h.close()
    names = ["%s%s" % (name, tail) for tail in ("", " without auto-reset")
             for name in ("obs", "reward", "done", "truncated", "terms", "state")]
    for shape in ("helper-wide", "plain"):
        for k in range(STEPS):
            for name, x, y in zip(names, runs["helper-narrow"][k], runs[shape][k]):
                assert torch.equal(x, y), "helper-narrow vs %s: %s after step %d" % (shape, name, k)
