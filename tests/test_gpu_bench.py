"""GPU: a plain bench.py run carries the headline only, times exactly --steps steps and, with
--dump-outputs, writes the outputs of its last timed step (checked against the same seeded steps
taken one rr_step at a time)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL_ONLY = ("n_sweep", "cpu_baseline", "sb3_legs", "allgather")
N = 5000 + 3


def _bench(monkeypatch, capsys, argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def _stepped(schedule):
    """The step outputs after the bench's seeded inputs taken one rr_step at a time: `schedule`
    lists the runs of consecutive steps, each starting at action batch 0 of the pool."""
    import torch

    from bench import POOL
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF, MAX_EPISODE_STEPS

    env = RocketBatch(N, model=6, device="cuda:0", max_episode_steps=MAX_EPISODE_STEPS, auto_reset=True,
                      episode_stats=False, **ENV_CONFIG_6DOF)
    env.reset()
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(42)
    pool = torch.rand((POOL, N, env.action_dim), device="cuda:0", generator=gen) * 2 - 1
    for run in schedule:
        for k in range(run):
            env.step(pool[k % POOL])
    torch.cuda.synchronize()
    out = {k: getattr(env, k).cpu().numpy().astype(np.float32) for k in ("obs", "reward", "done", "truncated")}
    env.close()
    return out


# direct launches below 8 timed steps: W warm-up steps, then the K timed ones; hipGraph replays from
# 8 on: W eager warm-up steps, one warming replay of the K-launch graph, then the timed replay
@pytest.mark.parametrize("steps,warmup,schedule", [(5, 3, (3, 5)), (11, 4, (4, 11, 11))])
def test_plain_run_dumps_the_last_timed_step(monkeypatch, capsys, tmp_path, steps, warmup, schedule):
    argv = ["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--n", str(N)]
    line = _bench(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "a")])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N * 1e3 / line["ms_per_step"])
    for k in ("metric", "unit", "higher_is_better", "dtype", "roofline"):
        assert k in line
    assert not [k for k in FULL_ONLY if k in line]
    ref = _stepped(schedule)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in ref)
    for k, want in ref.items():
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, want), k
    # the same arguments again: the same arrays
    _bench(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / "b")])
    for k in ref:
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))), k
