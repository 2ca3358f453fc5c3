#!/usr/bin/env python
"""What the Categorical policy's one-launch collect and one-launch evaluation cost beside the paths they
replace and beside the Gaussian 3DOF collect, HIP events, one JSON record.

    python tools/rollout_discrete_ab.py [--envs 65536] [--steps 16] [--runs 7] [--collects 4]
                                        [--time-limit 800] [--out FILE]

3DOF, fp32, RK4, 4 choices. Collect legs, each a DeviceRollout on a batch of its own from one seed:
  a_two_launch   the default Categorical collect: rr_policy_act_discrete + the env step per step, then
                 rr_policy_bootstrap and rr_gae (2 T + 2 launches)
  b_one_launch   one_launch=True: rr_rollout_collect_discrete (1 launch)
  c_gaussian     the Gaussian policy's rr_rollout_collect at (7, 2) (1 launch)
  d_per_step     one_launch=True, per_step=True: rr_rollout_step_discrete per step, then
                 rr_policy_bootstrap and rr_gae (T + 2 launches)
A sample is `--collects` whole collect() calls between two events, the second one synchronised, in us per
collect. Evaluation legs, under TimeLimit `--time-limit` with one episode per env, each sample one
batch.reset() (not timed) and one run() between two events, in us per run:
  e_unfused      PolicyEvaluator(fused=False): PyTorch ops around rr_step
  f_fused        PolicyEvaluator(fused=True): rr_policy_evaluate_discrete (1 launch)
The legs alternate in one process, `--runs` samples of each; the record holds every sample, the medians,
each leg's range (min, max) and spread (max - min), and the ratios b/a, b/c, d/a and f/e of the medians.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--collects", type=int, default=4)
    ap.add_argument("--time-limit", type=int, default=800)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be at least 5")

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.rollout import DeviceRollout, MlpActorCritic, MlpCategoricalActorCritic, PolicyEvaluator

    if not torch.cuda.is_available():
        raise SystemExit("rollout_discrete_ab.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    n, T, k = args.envs, args.steps, 4

    def policy(cls, heads):
        torch.manual_seed(0)
        pol = cls(7, heads).to(dev)
        with torch.no_grad():  # off SB3's small-gain init, so that the choices spread
            for prm in pol.parameters():
                prm.add_(0.3 * torch.randn_like(prm))
        return pol

    cat, gau = policy(MlpCategoricalActorCritic, k), policy(MlpActorCritic, 2)

    def batch(tl):
        return RocketBatch(n, model=3, device=dev, max_episode_steps=tl, seed=7)

    ros = {"a_two_launch": DeviceRollout(batch(args.time_limit), cat, n_steps=T, seed=3),
           "b_one_launch": DeviceRollout(batch(args.time_limit), cat, n_steps=T, seed=3, one_launch=True),
           "c_gaussian": DeviceRollout(batch(args.time_limit), gau, n_steps=T, seed=3),
           "d_per_step": DeviceRollout(batch(args.time_limit), cat, n_steps=T, seed=3, one_launch=True,
                                       per_step=True)}
    assert not ros["a_two_launch"].one_launch and ros["b_one_launch"].one_launch and not ros["b_one_launch"].per_step
    assert ros["c_gaussian"].one_launch and not ros["c_gaussian"].per_step and ros["d_per_step"].per_step
    evs = {"e_unfused": PolicyEvaluator(batch(args.time_limit), cat, n_episodes=1, fused=False),
           "f_fused": PolicyEvaluator(batch(args.time_limit), cat, n_episodes=1, fused=True)}

    def timed(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / calls

    def evaluate(ev):
        ev.env.reset()
        torch.cuda.synchronize()
        return timed(ev.run, 1)

    for ro in ros.values():  # warm-up: module load, the packed image
        ro.collect()
    for ev in evs.values():
        evaluate(ev)
    torch.cuda.synchronize()
    samples = {name: [] for name in list(ros) + list(evs)}
    for _ in range(args.runs):
        for name, ro in ros.items():
            samples[name].append(timed(ro.collect, args.collects))
        for name, ev in evs.items():
            samples[name].append(evaluate(ev))
    med = {name: statistics.median(v) for name, v in samples.items()}
    same = all(torch.equal(getattr(ros["a_two_launch"], f), getattr(ros[o], f))
               for o in ("b_one_launch", "d_per_step") for f in ("actions", "log_probs", "rewards", "advantages"))
    rec = {"envs": n, "n_steps": T, "model": "3DOF", "integrator": "rk4", "n_choices": k,
           "time_limit": args.time_limit, "runs": args.runs, "collects_per_sample": args.collects,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "source_hash": build.source_hash(),
           "unit": "us per collect() (a-d: HIP events around whole collect() calls, the second event synchronised) "
                   "and us per run() (e, f: one evaluation of one episode per env from a fresh reset)",
           "categorical_paths_bitwise_equal_after": same,
           "episodes_evaluated": {name: int(ev.episodes.sum()) for name, ev in evs.items()},
           "b_over_a": med["b_one_launch"] / med["a_two_launch"], "b_over_c": med["b_one_launch"] / med["c_gaussian"],
           "d_over_a": med["d_per_step"] / med["a_two_launch"], "f_over_e": med["f_fused"] / med["e_unfused"]}
    for name, v in samples.items():
        rec[name] = {"us": v, "median": med[name], "range": [min(v), max(v)], "spread": max(v) - min(v)}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
