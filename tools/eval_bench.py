#!/usr/bin/env python
"""Timings of the on-device policy evaluation (rr_policy_evaluate), HIP events, one JSON record.

    python tools/eval_bench.py [--n 65536] [--out profiles/eval_bench.json] [--no-unfused]

  fixed   the evaluation against the collect on the same work: 6DOF, fp32, TimeLimit 800,
          max_steps = 16 with n_episodes = 16 (no env can finish 16 episodes in 16 steps, so every
          wave runs exactly 16 steps) against rr_rollout_collect with n_steps = 16. Both calls are
          one launch plus the policy pack launch. Blocks of `--calls` calls are timed alternately,
          `--blocks` blocks each; the record holds every block and the medians, in us per call.
  real    6DOF, TimeLimit 800, n_episodes = 1 from a fresh reset: us per evaluation, the wave-steps
          executed (sum over 64-env waves of the longest episode in the wave), env-steps and
          env-steps per second; `--reps` evaluations, each from a new reset.
  unfused the same evaluation through PolicyEvaluator(fused=False), once (it runs all 800
          iterations: it cannot leave early without a synchronise).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / calls  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-unfused", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rl_rocket_amd import build
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import DeviceRollout, MlpActorCritic, PolicyEvaluator

    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    n = args.n
    torch.manual_seed(0)
    pol = MlpActorCritic(14, 3).to(dev)
    rec = {"n": n, "model": "6DOF", "policy_dtype": "fp32", "max_episode_steps": 800,
           "device": torch.cuda.get_device_name(0), "source_hash": build.source_hash()}

    def env():
        return RocketBatch(n, model=6, device=dev, max_episode_steps=800, **ENV_CONFIG_6DOF)

    # ---- fixed work: 16 steps of every env, evaluation vs collect, alternating blocks ----
    ro = DeviceRollout(env(), pol, n_steps=16, policy_dtype="fp32")
    eb = env()
    eb.reset()
    ev = PolicyEvaluator(eb, pol, n_episodes=16, max_steps=16)
    for _ in range(20):  # warm-up: code objects loaded, episodes spread over their lengths
        ro.collect()
        ev.run()
    torch.cuda.synchronize()
    t_ev, t_co = [], []
    for _ in range(args.blocks):
        t_co.append(timed(ro.collect, args.calls))
        t_ev.append(timed(ev.run, args.calls))
    rec["fixed"] = {"steps": 16, "calls_per_block": args.calls, "collect_us": t_co, "evaluate_us": t_ev,
                    "collect_us_median": statistics.median(t_co), "evaluate_us_median": statistics.median(t_ev),
                    "collect_us_min": min(t_co), "evaluate_us_min": min(t_ev)}
    ro.env.close()
    eb.close()

    # ---- the real workload: one whole episode per env under TimeLimit 800 ----
    def real(fused, reps):
        b = env()
        e = PolicyEvaluator(b, pol, n_episodes=1, fused=fused)
        runs = []
        for r in range(reps + 1):  # run 0 is the warm-up
            b.reset()
            us = timed(e.run, 1)
            res = e.result
            ln = res.ep_length[0].long()
            pad = (-n) % 64
            waves = torch.nn.functional.pad(ln, (0, pad)).view(-1, 64).max(dim=1).values
            s = res.stats()
            if r:
                runs.append({"us": us, "wave_steps": int(waves.sum()), "env_steps": int(ln.sum()),
                             "env_steps_per_s": float(ln.sum()) / (us * 1e-6), "mean_ep_length": s["mean_ep_length"],
                             "mean_reward": s["mean_reward"], "episodes": s["episodes"],
                             "unfinished": s["unfinished"]})
        b.close()
        return runs

    rec["real"] = real(True, args.reps)
    if not args.no_unfused:
        rec["real_unfused"] = real(False, 1)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
