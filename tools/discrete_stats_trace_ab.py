#!/usr/bin/env python
"""What the Categorical policy's collect statistics and recorded evaluation episodes cost over its plain
one-launch calls, beside what the Gaussian policy's statistics cost over its plain collect, HIP events, one
JSON record. A sibling of tools/rollout_discrete_ab.py, in its style.

    python tools/discrete_stats_trace_ab.py [--envs 65536] [--steps 16] [--runs 7] [--collects 4]
                                            [--time-limit 800] [--recorded 64] [--out FILE]

3DOF, fp32, RK4, 4 choices. Collect legs, each a DeviceRollout on a batch of its own (episode_stats and
auto_reset on) from one seed:
  a_discrete        one_launch=True: rr_rollout_collect_discrete (1 launch)
  b_discrete_stats  one_launch=True, stats=True: rr_rollout_collect_discrete_stats (the collect and the
                    one-workgroup reduction, 2 launches)
  c_gaussian        the Gaussian policy's rr_rollout_collect at (7, 2) (1 launch)
  d_gaussian_stats  stats=True: rr_rollout_collect_stats (2 launches)
A sample is `--collects` whole collect() calls between two events, the second one synchronised, in us per
collect. Evaluation legs, under TimeLimit `--time-limit` with one episode per env, each sample one
batch.reset() (not timed) and one run() between two events, in us per run:
  e_eval            PolicyEvaluator(fused=True): rr_policy_evaluate_discrete (1 launch)
  f_eval_rec_some   the same with `--recorded` envs recorded, spread evenly over the batch:
                    rr_policy_evaluate_discrete_trace (1 launch)
  g_eval_rec_all    the same with every env recorded
The legs alternate in one process, `--runs` samples of each; the record holds every sample, the medians,
each leg's range (min, max) and spread (max - min), the differences b - a and d - c of the medians with the
larger of the legs' spreads beside them, and the ratios f/e and g/e.
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
    ap.add_argument("--recorded", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 5:
        raise SystemExit("--runs must be at least 5")

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.rollout import DeviceRollout, MlpActorCritic, MlpCategoricalActorCritic, PolicyEvaluator

    if not torch.cuda.is_available():
        raise SystemExit("discrete_stats_trace_ab.py measures on the GPU; no HIP device found")
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

    tl = args.time_limit
    ros = {"a_discrete": DeviceRollout(batch(tl), cat, n_steps=T, seed=3, one_launch=True),
           "b_discrete_stats": DeviceRollout(batch(tl), cat, n_steps=T, seed=3, one_launch=True, stats=True),
           "c_gaussian": DeviceRollout(batch(tl), gau, n_steps=T, seed=3),
           "d_gaussian_stats": DeviceRollout(batch(tl), gau, n_steps=T, seed=3, stats=True)}
    for name, ro in ros.items():
        assert ro.one_launch and not ro.per_step and (ro.stats is not None) == name.endswith("_stats")
    some = torch.linspace(0, n - 1, min(args.recorded, n)).long().unique().tolist()
    evs = {"e_eval": PolicyEvaluator(batch(tl), cat, n_episodes=1, fused=True),
           "f_eval_rec_some": PolicyEvaluator(batch(tl), cat, n_episodes=1, fused=True, record=some),
           "g_eval_rec_all": PolicyEvaluator(batch(tl), cat, n_episodes=1, fused=True, record=list(range(n)))}

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
    spread = {name: max(v) - min(v) for name, v in samples.items()}
    fields = ("actions", "log_probs", "rewards", "advantages")
    same = {"discrete": all(torch.equal(getattr(ros["a_discrete"], f), getattr(ros["b_discrete_stats"], f)) for f in fields),
            "gaussian": all(torch.equal(getattr(ros["c_gaussian"], f), getattr(ros["d_gaussian_stats"], f)) for f in fields)}
    names = ("episodes", "ep_return", "ep_length", "flags", "used_mass", "final_state")
    eval_same = all(torch.equal(getattr(evs["e_eval"], f), getattr(evs[o], f)) for o in ("f_eval_rec_some", "g_eval_rec_all")
                    for f in names)
    tr = evs["g_eval_rec_all"].trace
    rec = {"envs": n, "n_steps": T, "model": "3DOF", "integrator": "rk4", "n_choices": k, "time_limit": tl,
           "runs": args.runs, "collects_per_sample": args.collects, "recorded_some": len(some),
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "source_hash": build.source_hash(),
           "unit": "us per collect() (a-d: HIP events around whole collect() calls, the second event synchronised) "
                   "and us per run() (e-g: one evaluation of one episode per env from a fresh reset)",
           "stats_and_plain_rollouts_bitwise_equal_after": same,
           "recorded_and_plain_evaluations_bitwise_equal_after": eval_same,
           "episodes_evaluated": {name: int(ev.episodes.sum()) for name, ev in evs.items()},
           "trace_bytes_all_recorded": sum(t.numel() * t.element_size() for t in (tr.state, tr.action, tr.terms,
                                                                                   tr.length, tr.choice)),
           "discrete_stats_minus_plain_us": med["b_discrete_stats"] - med["a_discrete"],
           "discrete_pair_spread_us": max(spread["a_discrete"], spread["b_discrete_stats"]),
           "gaussian_stats_minus_plain_us": med["d_gaussian_stats"] - med["c_gaussian"],
           "gaussian_pair_spread_us": max(spread["c_gaussian"], spread["d_gaussian_stats"]),
           "f_over_e": med["f_eval_rec_some"] / med["e_eval"], "g_over_e": med["g_eval_rec_all"] / med["e_eval"]}
    for name, v in samples.items():
        rec[name] = {"us": v, "median": med[name], "range": [min(v), max(v)], "spread": spread[name]}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
