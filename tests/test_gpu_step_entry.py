"""The helper-wave step kernels (N <= RR_HELP_MAX_N) against the plain kernel of the same library,
bitwise: their entry issues every load ahead of the flag clear and the workgroup barrier. The plain
kernel (RR_HELP_MAX_N=0 at rr_create) has no such barrier, so it is the reference. Every case runs TimeLimit 3 with
auto-reset for 6 steps: every lane truncates and resets inside the run."""
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_STEPS = 3
STEPS = MAX_STEPS + 3


def _kw(model):
    from rl_rocket_amd.params import ENV_CONFIG_6DOF

    return ENV_CONFIG_6DOF if model == 6 else {}


def _twins(model, n, monkeypatch):
    """(helper-wave env, plain env) of the same configuration and seed, both reset."""
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


def _same_done_list(h, p, step):
    for name, x, y in zip(("idx", "terminal_obs", "episode_return", "episode_len"), h.fetch_done(), p.fetch_done()):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "done list %s after step %d" % (name, step)


def _run_steps(model, n, monkeypatch):
    h, p = _twins(model, n, monkeypatch)
    seen_done = 0
    for k, act in enumerate(_actions(n, h.action_dim, STEPS, 5)):
        oh, op = h.step(act), p.step(act)
        for name, x, y in zip(("obs", "reward", "done", "truncated"), oh, op):
            _same(x, y, "%s after step %d" % (name, k))
        _same(h.terms, p.terms, "terms after step %d" % k)
        _same_state(h, p, k)
        _same_done_list(h, p, k)
        seen_done += int(oh[2].sum())
    assert seen_done >= n  # every lane ended an episode (TimeLimit 3) and was reset inside the run
    h.close()
    p.close()


# WPB = 1 (N <= 16 384): one env; a ragged wave; a full wave; a full and a ragged wave; several workgroups.
# WPB = 4: a workgroup whose last main waves are empty (16 385) or full, full, full, ragged (16 384 + 64 * 3 + 5)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 16385, 16384 + 64 * 3 + 5])
def test_6dof_helper_kernel_is_bitwise_plain(n, monkeypatch):
    _run_steps(6, n, monkeypatch)


# 7 state planes, 8-B action rows
@pytest.mark.parametrize("n", [65, 16385])
def test_3dof_helper_kernel_is_bitwise_plain(n, monkeypatch):
    _run_steps(3, n, monkeypatch)


def test_rows_entry_point_is_bitwise_plain(monkeypatch):
    """rr_step_rows (obs, reward, done as one fp32 row per env; ShardGather's send rows): done travels in
    the row, truncated as flags."""
    import torch

    n = 16385
    h, p = _twins(6, n, monkeypatch)
    rh = torch.empty((n, h.state_dim + 2), device=DEV)
    rp = torch.empty((n, h.state_dim + 2), device=DEV)
    for k, act in enumerate(_actions(n, h.action_dim, STEPS, 6)):
        h.step_rows(act, rh)
        p.step_rows(act, rp)
        _same(rh, rp, "rows after step %d" % k)
        _same(h.truncated, p.truncated, "truncated after step %d" % k)
        _same(h.terms, p.terms, "terms after step %d" % k)
        _same_state(h, p, k)
        _same_done_list(h, p, k)
    h.close()
    p.close()


@pytest.mark.parametrize("offset", [0, 1, 2, 3, 4])
def test_flag_pointer_alignment(offset, monkeypatch):
    """Caller-owned done / truncated rows at byte offsets 0..4 of a 4-B aligned buffer, 64 guard bytes of
    0xA5 on both sides: the flags equal the plain kernel's and no byte outside the rows is written,
    whatever the pointers' alignment."""
    import torch

    n, guard = 320, 64
    h, p = _twins(6, n, monkeypatch)

    def flags():
        buf = torch.full((guard + offset + n + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 4 == 0
        return buf, buf[guard + offset:guard + offset + n]

    dbuf, done = flags()
    tbuf, trunc = flags()
    assert done.data_ptr() % 4 == offset % 4 and trunc.data_ptr() % 4 == offset % 4
    obs = torch.empty((n, h.state_dim), device=DEV)
    rew = torch.empty((n,), device=DEV)
    for k, act in enumerate(_actions(n, h.action_dim, STEPS, 7)):
        done.fill_(0xA5)
        trunc.fill_(0xA5)
        h.step(act, out=(obs, rew, done, trunc))
        po, pr, pd, pt = p.step(act)
        _same(done, pd, "done after step %d" % k)
        _same(trunc, pt, "truncated after step %d" % k)
        _same(obs, po, "obs after step %d" % k)
        _same(rew, pr, "reward after step %d" % k)
        for buf in (dbuf, tbuf):
            assert bool((buf[:guard + offset] == 0xA5).all()) and bool((buf[guard + offset + n:] == 0xA5).all()), \
                "guard bytes touched at step %d" % k
    _same_state(h, p, STEPS - 1)
    h.close()
    p.close()


def test_graph_replays_are_bitwise_plain(monkeypatch):
    """8 captured steps of the helper-wave env, replayed twice from a restored checkpoint: both replays
    equal each other and the eager plain twin (a flag left set in LDS by the previous launch would let a
    main wave read a candidate row before its helper has written it)."""
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
    ref = []
    for act in acts:
        ref.append([x.clone() for x in p.step(act)])
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
    for b0, b1 in zip(replays[0][0], replays[1][0]):
        assert torch.equal(b0, b1)
    h.close()
    p.close()
