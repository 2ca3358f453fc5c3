"""The helper-wave step kernels (N <= RR_HELP_MAX_N) against the plain kernel of the same library, bitwise,
in waves that hold done and live lanes side by side: the done tail of a main wave (terminal rows, the
done word, the wait on its helper's flag, the candidate row, the second obs) next to lanes that just go
on. tests/test_gpu_step_entry.py runs TimeLimit 3, where every lane of every wave ends together and no
ground event fires; here the state is injected (set_state) so that, of env i,

  * i % 3 == 0 sits 2 m above the ground descending at 60 m/s: it crosses the ground inside step 0
    (0.1 s: 6 m of descent against at most +0.06 m from full thrust; the CPU oracle, oracle.oracle.step,
    reports status 1 and done for 4096 of 4096 such rows drawn from the reset distribution with random
    actions, 6DOF on x / vx and 3DOF on z / vz alike: the crossing lies a third into the step, certain,
    not marginal);
  * i % 3 == 1 has elapsed = max_steps - 1 - (i % 5) under TimeLimit 8: it truncates at step i % 5;
  * the rest stay aloft with elapsed = 2, so they truncate at step 5 (without them no env would be due
    at the sixth step: the lanes above are done by step 4 and their next episodes last until step 8);
  * the last full wave is made "rest" lanes only, so it has no done lane at step 0 (where N has a single
    full wave, N = 65, that wave stays mixed and the ragged wave's one lane, not due before step 4, is
    the wave without a done lane).

The preconditions (a mixed wave at every step, a ground event and a wave without a done lane at step 0,
truncated and non-truncated dones) are asserted on the plain twin, not on the kernel under test."""
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_STEPS = 8
STEPS = 6
WAVE = 64
# (altitude plane, vertical-velocity plane) of the state
ALT = {6: (0, 3), 3: (1, 4)}


def _kw(model):
    from rl_rocket_amd.params import ENV_CONFIG_6DOF

    return ENV_CONFIG_6DOF if model == 6 else {}


def _twins(model, n, monkeypatch):
    """(helper-wave env, plain env) of the same configuration and seed, both in the same mixed state."""
    import numpy as np
    import torch

    from rl_rocket_amd.batch import RocketBatch

    mk = lambda: RocketBatch(n, model=model, device=DEV, max_episode_steps=MAX_STEPS, auto_reset=True,  # noqa: E731
                             episode_stats=True, compute_terms=True, **_kw(model))
    monkeypatch.delenv("RR_HELP_MAX_N", raising=False)
    h = mk()
    monkeypatch.setenv("RR_HELP_MAX_N", "0")
    p = mk()
    monkeypatch.delenv("RR_HELP_MAX_N", raising=False)
    for e in (h, p):
        e.seed(11)
        e.reset()
    st = h.get_state()[0].cpu().numpy().copy()
    i = np.arange(n)
    ground, due = i % 3 == 0, i % 3 == 1
    full = n // WAVE
    if full >= 2:  # the last full wave: no done lane at step 0
        calm = (i >= (full - 1) * WAVE) & (i < full * WAVE)
        ground &= ~calm
        due &= ~calm
    alt, vel = ALT[model]
    st[alt, ground] = 2.0
    st[vel, ground] = -60.0
    el = np.where(due, MAX_STEPS - 1 - (i % 5), 2).astype(np.int32)
    el[ground] = 0
    for e in (h, p):
        e.set_state(torch.from_numpy(st), elapsed=torch.from_numpy(el))
    return h, p


def _actions(n, na, steps, seed):
    import torch

    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return [torch.rand((n, na), device=DEV, generator=g) * 2 - 1 for _ in range(steps)]


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(x, y, what):
    import torch

    assert torch.equal(_bits(x), _bits(y)), what


def _same_state(h, p, step):
    ch, cp = h.checkpoint(), p.checkpoint()
    for k in ("state", "v0", "counter", "ep_return"):
        _same(ch[k], cp[k], "%s after step %d" % (k, step))


def _same_done_rows(h, p, step):
    for name, x, y in zip(("idx", "terminal_obs", "episode_return", "episode_len"), h.fetch_done(), p.fetch_done()):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "done list %s after step %d" % (name, step)
    for name, x, y in zip(("terminal_obs", "episode_return", "episode_len"), h.copy_terminal(), p.copy_terminal()):
        _same(x, y, "copy_terminal %s after step %d" % (name, step))


class _Seen:
    """The preconditions, gathered from the PLAIN twin's outputs step by step."""

    def __init__(self, n):
        self.n, self.mixed, self.trunc, self.not_trunc = n, [], 0, 0
        self.ground0 = self.calm0 = None

    def step(self, k, p, done, truncated):
        import numpy as np

        n = self.n
        pad = (-n) % WAVE
        valid = np.pad(np.ones(n, bool), (0, pad)).reshape(-1, WAVE)
        d = np.pad(done.cpu().numpy() != 0, (0, pad)).reshape(-1, WAVE)
        self.mixed.append(bool(((d & valid).any(axis=1) & (~d & valid).any(axis=1)).any()))
        t = truncated.cpu().numpy() != 0
        self.trunc += int((t & d.reshape(-1)[:n]).sum())
        self.not_trunc += int((~t & d.reshape(-1)[:n]).sum())
        if k == 0:
            self.ground0 = int((p.terms[-1] == 1.0).sum())
            self.calm0 = int((~d.any(axis=1)).sum())

    def check(self):
        # the first STEPS steps (the graph test runs two more, in which no env is due)
        assert len(self.mixed) >= STEPS and all(self.mixed[:STEPS]), \
            "no wave with done and live lanes at some step: %s" % self.mixed
        assert self.ground0 >= 1, "no ground event at step 0"
        assert self.calm0 >= 1, "every wave has a done lane at step 0"
        assert self.trunc >= 1 and self.not_trunc >= 1, (self.trunc, self.not_trunc)


def _run_steps(model, n, monkeypatch):
    h, p = _twins(model, n, monkeypatch)
    seen = _Seen(n)
    for k, act in enumerate(_actions(n, h.action_dim, STEPS, 5)):
        oh, op = h.step(act), p.step(act)
        seen.step(k, p, op[2], op[3])
        for name, x, y in zip(("obs", "reward", "done", "truncated"), oh, op):
            _same(x, y, "%s after step %d" % (name, k))
        _same(h.terms, p.terms, "terms after step %d" % k)
        _same_state(h, p, k)
        _same_done_rows(h, p, k)
    seen.check()
    h.close()
    p.close()


# WPB = 1 (N <= 16 384): a full and a ragged wave; several workgroups. WPB = 4: a workgroup whose last main
# waves are empty (16 385) or full, full, full, ragged (16 384 + 64 * 3 + 5)
@pytest.mark.parametrize("n", [65, 257, 16385, 16384 + 64 * 3 + 5])
def test_6dof_mixed_waves_are_bitwise_plain(n, monkeypatch):
    _run_steps(6, n, monkeypatch)


# 7 state planes, the event on z
@pytest.mark.parametrize("n", [65, 16385])
def test_3dof_mixed_waves_are_bitwise_plain(n, monkeypatch):
    _run_steps(3, n, monkeypatch)


def test_graph_replays_from_a_mixed_state_are_bitwise_plain(monkeypatch):
    """8 captured steps from the mixed state, replayed twice from the restored checkpoint: both replays
    equal each other and the eager plain twin (a candidate row read before its helper wrote it, or a flag
    left over from the previous launch, shows here)."""
    import torch

    n, K = 16385, 8
    h, p = _twins(6, n, monkeypatch)
    acts = _actions(n, h.action_dim, K, 8)
    ck = {k: v.clone() for k, v in h.checkpoint().items()}
    outs = [h.alloc_outputs() for _ in range(K)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for act, out in zip(acts, outs):
                h.step(act, out=out)
    torch.cuda.current_stream().wait_stream(s)
    seen = _Seen(n)
    ref = []
    for k, act in enumerate(acts):
        ref.append([x.clone() for x in p.step(act)])
        seen.step(k, p, ref[-1][2], ref[-1][3])
    seen.check()
    ref_state = p.checkpoint()
    replays = []
    for _ in range(2):
        h.restore(ck)
        for out in outs:
            out.block.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        replays.append(([o.block.clone() for o in outs], h.checkpoint()))
        for k in range(K):
            for name, x, y in zip(("obs", "reward", "done", "truncated"), outs[k], ref[k]):
                _same(x, y, "%s of captured step %d" % (name, k))
        for key in ("state", "v0", "counter", "ep_return"):
            _same(replays[-1][1][key], ref_state[key], key)
        _same_done_rows(h, p, K - 1)
    for b0, b1 in zip(replays[0][0], replays[1][0]):
        assert torch.equal(b0, b1)
    h.close()
    p.close()


def test_rows_entry_point_from_a_mixed_state_is_bitwise_plain(monkeypatch):
    """rr_step_rows (obs, reward, done as one fp32 row per env) from the same mixed state."""
    import torch

    n = 16385
    h, p = _twins(6, n, monkeypatch)
    rh = torch.empty((n, h.state_dim + 2), device=DEV)
    rp = torch.empty((n, h.state_dim + 2), device=DEV)
    seen = _Seen(n)
    for k, act in enumerate(_actions(n, h.action_dim, STEPS, 6)):
        h.step_rows(act, rh)
        p.step_rows(act, rp)
        seen.step(k, p, rp[:, -1], p.truncated)
        _same(rh, rp, "rows after step %d" % k)
        _same(h.truncated, p.truncated, "truncated after step %d" % k)
        _same(h.terms, p.terms, "terms after step %d" % k)
        _same_state(h, p, k)
        _same_done_rows(h, p, k)
    seen.check()
    h.close()
    p.close()
