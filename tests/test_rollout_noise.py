"""The rollout's action-noise keying, on the CPU: the statistics of its NumPy restatement
(tests/rollout_ref.py noise_ref, which tests/test_gpu_rollout_replay.py pins the kernels to element
by element) and the independence of the streams of different user seeds.

Every statistic is held within 6 of its own standard errors under the null hypothesis of
independent N(0, 1) draws (M samples per component): mean 1/sqrt(M), variance sqrt(2/M), third
moment sqrt(15/M), fourth moment sqrt(96/M), KS distance 1/sqrt(M) (the Kolmogorov statistic
sqrt(M) D exceeds 6 with probability 2 exp(-72)), each Pearson correlation 1/sqrt(M).
Measured with the seed mix: at most 2.0 standard errors on any statistic, largest |draw| 5.14."""
import numpy as np
import pytest

from rollout_ref import noise_ref

N, T, ITERS = 4096 + 37, 16, 4
SIGMAS = 6.0


@pytest.fixture(scope="module", params=[(3, 123), (3, 11), (3, (7 << 32) | 5), (2, 123), (2, 11), (2, (7 << 32) | 5)],
                ids=lambda p: "act%d-seed%x" % p)
def draws(request):
    """[ITERS, T, N, act_dim] draws of one (act_dim, seed)."""
    na, seed = request.param
    return np.stack([np.stack([noise_ref(N, 0, seed, it, t, na) for t in range(T)]) for it in range(ITERS)])


def _z(stat, se):
    return abs(stat) / se


def test_marginal_moments_and_ks(draws):
    import torch

    na = draws.shape[-1]
    for a in range(na):
        x = draws[..., a].ravel()
        m = x.size
        zs = {"mean": _z(x.mean(), 1 / np.sqrt(m)), "var": _z(x.var() - 1, np.sqrt(2 / m)),
              "m3": _z((x ** 3).mean(), np.sqrt(15 / m)), "m4": _z((x ** 4).mean() - 3, np.sqrt(96 / m))}
        xs = np.sort(x)
        cdf = torch.special.ndtr(torch.from_numpy(xs)).numpy()
        i = np.arange(m)
        zs["ks"] = _z(max((cdf - i / m).max(), ((i + 1) / m - cdf).max()), 1 / np.sqrt(m))
        print("component", a, {k: round(float(v), 2) for k, v in zs.items()}, "max |z|", np.abs(x).max())
        assert np.isfinite(x).all()
        for k, v in zs.items():
            assert v < SIGMAS, (a, k, v)


def test_no_dependence_between_components_steps_iterations_and_envs(draws):
    def corr(a, b):
        a, b = a.ravel(), b.ravel()
        return abs(np.corrcoef(a, b)[0, 1]) * np.sqrt(a.size)

    z = draws
    na = z.shape[-1]
    worst = {}
    for a in range(na):
        for b in range(a + 1, na):
            worst["comp %d-%d" % (a, b)] = corr(z[..., a], z[..., b])
        worst["t lag 1 [%d]" % a] = corr(z[:, :-1, :, a], z[:, 1:, :, a])
        worst["iter lag 1 [%d]" % a] = corr(z[:-1, ..., a], z[1:, ..., a])
        worst["env e, e+1 [%d]" % a] = corr(z[:, :, :-1, a], z[:, :, 1:, a])
        worst["env e, e+64 [%d]" % a] = corr(z[:, :, :-64, a], z[:, :, 64:, a])
    print({k: round(float(v), 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v < SIGMAS, (k, v)


def _stream(seed, **kw):
    return np.concatenate([noise_ref(4096, 0, seed, it, t, 3, **kw).ravel() for it in (0, 1) for t in (0, 1)])


def test_seeds_draw_independent_streams():
    """Different user seeds share (almost) no draws: for each pair of {0, 1, 5, 2^32} at n = 4096,
    T = 2, *iter 0 and 1, fewer than 1 % of one seed's draws occur among the other's (accidental
    fp64 matches of 24-bit uniforms: ~1e-4). Without the host-side splitmix64 of the seed this is
    100 %: seed 1 gives env e the stream seed 0 gives env e ^ 1, seed 2^32 at iteration 0 is seed 0
    at iteration 1 (measured: 1.0, 1.0, 0.5 shared)."""
    seeds = (0, 1, 5, 1 << 32)
    streams = {s: _stream(s) for s in seeds}
    for i, a in enumerate(seeds):
        for b in seeds[i + 1:]:
            shared = np.isin(streams[a], streams[b]).mean()
            print("seeds", a, b, "shared", shared)
            assert shared < 0.01, (a, b, shared)


def test_unmixed_seed_would_share_streams():
    """The check above has teeth: the same key without the seed mix fails it."""
    raw = {s: _stream(s, mix_seed=False) for s in (0, 1, 1 << 32)}
    assert np.isin(raw[1], raw[0]).mean() > 0.99          # env e <-> e ^ 1
    assert np.isin(raw[1 << 32], raw[0]).mean() >= 0.49   # iteration 0 <-> iteration 1
