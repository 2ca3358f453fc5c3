#!/usr/bin/env python
"""What the episode statistics cost the one-launch collect (rr_rollout_collect_stats against
rr_rollout_collect), HIP events over graph replays, one JSON record.

    python tools/collect_stats_ab.py [--n 65536] [--runs 5] [--replays 40] [--out FILE]
                                     [--plain-only] [--parent FILE]

6DOF, fp32 policy, n_steps 16, TimeLimit 800. Two batches with the same seed, one collected by the
plain call and one by the statistics call (two launches: the collect and the one-workgroup
reduction), each captured once in a graph. A run times `--replays` replays between two events and
reports the mean per replay; the runs alternate plain / stats in one session, `--runs` of each. Both
batches take the same number of collects, so run k of either covers the same episodes. The record
holds every run, the medians, the plain call's spread (max - min) and the statistics call's overhead
over the plain median, in us and in units of that spread.

--plain-only times only the plain call (a library without the new entry point, e.g. a build of the
parent commit selected with RR_LIB_PATH); --parent FILE embeds such a record as "parent".
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import DeviceRollout, MlpActorCritic

    if not torch.cuda.is_available():
        raise SystemExit("collect_stats_ab.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    n, T, tl = args.n, 16, 800
    torch.manual_seed(0)
    pol = MlpActorCritic(14, 3).to(dev)

    def arm(stats):
        b = RocketBatch(n, **dict(ENV_CONFIG_6DOF, model=6, device=dev, max_episode_steps=tl, seed=7))
        ro = DeviceRollout(b, pol, n_steps=T, seed=3, stats=stats)
        for _ in range(3):  # warm-up: code objects loaded, buffers touched
            ro.collect()
        g, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            with torch.cuda.graph(g, stream=st):
                ro.collect()
        torch.cuda.current_stream().wait_stream(st)
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        return ro, g

    arms = {"plain": arm(False)}
    if not args.plain_only:
        arms["stats"] = arm(True)

    def timed(g):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.replays):
            g.replay()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.replays  # us per replay

    samples = {k: [] for k in arms}
    for _ in range(args.runs):
        for k, (_ro, g) in arms.items():
            samples[k].append(timed(g))
    med = {k: statistics.median(v) for k, v in samples.items()}
    rec = {"n": n, "model": "6DOF", "policy_dtype": "fp32", "n_steps": T, "max_episode_steps": tl,
           "runs": args.runs, "replays_per_run": args.replays, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(_lib.LIB_PATH), "source_hash": build.source_hash(),
           "plain_us": samples["plain"], "plain_us_median": med["plain"],
           "plain_us_spread": max(samples["plain"]) - min(samples["plain"])}
    if "stats" in arms:
        ro_p, ro_s = arms["plain"][0], arms["stats"][0]
        over = med["stats"] - med["plain"]
        rec.update({"stats_us": samples["stats"], "stats_us_median": med["stats"],
                    "stats_us_spread": max(samples["stats"]) - min(samples["stats"]), "overhead_us": over,
                    "overhead_over_plain_spread": over / rec["plain_us_spread"] if rec["plain_us_spread"] else None,
                    "same_rollout": bool(torch.equal(ro_p.returns, ro_s.returns) and torch.equal(ro_p.obs, ro_s.obs)),
                    "last": ro_s.stats.last()})
    if args.parent:
        with open(args.parent) as f:
            rec["parent"] = json.load(f)
    for ro, _g in arms.values():
        ro.env.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
