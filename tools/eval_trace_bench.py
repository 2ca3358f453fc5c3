#!/usr/bin/env python
"""What recording costs the one-launch evaluation (rr_policy_evaluate_trace against
rr_policy_evaluate), HIP events, one JSON record.

    python tools/eval_trace_bench.py [--n 65536] [--reps 5] [--k 64 4096 65536] [--out FILE]
                                     [--plain-only] [--parent FILE]

6DOF, TimeLimit 800, one episode per env, fp32 policy. The batch is reset once and checkpointed;
every timed call starts from that checkpoint, so all calls run the same episodes. One round times the
plain call and then the recording call at each K (the K recorded envs are spread evenly over the
batch, record_steps = 800); `--reps` rounds in one session. The record holds every sample, the
medians, the spread (max - min) of the plain call, and for each K the overhead over the plain median,
the recorded env-steps and bytes (92 B per 6DOF env-step: 14 state + 3 action + 6 term floats) and,
where the overhead exceeds the plain call's spread, bytes per second of overhead.

--plain-only times only the plain call (a library without the recording entry point, e.g. a build
of the parent commit selected with RR_LIB_PATH); --parent FILE embeds such a record as "parent".
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROW_BYTES = (14 + 3 + 6) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, nargs="*", default=[64, 4096, 65536])
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import MlpActorCritic, PolicyEvaluator

    if not torch.cuda.is_available():
        raise SystemExit("eval_trace_bench.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    n, tl = args.n, 800
    torch.manual_seed(0)
    pol = MlpActorCritic(14, 3).to(dev)
    b = RocketBatch(n, model=6, device=dev, max_episode_steps=tl, **ENV_CONFIG_6DOF)
    b.reset()
    ck = b.checkpoint()
    evs = {0: PolicyEvaluator(b, pol, n_episodes=1)}
    for k in ([] if args.plain_only else args.k):
        k = min(k, n)
        evs[k] = PolicyEvaluator(b, pol, n_episodes=1, record=(torch.arange(k) * n) // k, record_steps=tl)

    def timed(ev):
        b.restore(ck)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ev.run()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0  # us

    for ev in evs.values():  # warm-up: code objects loaded, trace buffers touched
        timed(ev)
    samples = {k: [] for k in evs}
    for _ in range(args.reps):
        for k, ev in evs.items():
            samples[k].append(timed(ev))
    res = evs[0].result
    steps = int(res.ep_length[0].sum())
    rec = {"n": n, "model": "6DOF", "policy_dtype": "fp32", "max_episode_steps": tl, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "source_hash": build.source_hash(), "env_steps": steps, "episodes": int(res.episodes.sum()),
           "plain_us": samples[0], "plain_us_median": statistics.median(samples[0]),
           "plain_us_spread": max(samples[0]) - min(samples[0]), "trace": {}}
    for k, ev in evs.items():
        if not k:
            continue
        ln = ev.trace.length[0].long()
        med = statistics.median(samples[k])
        over = med - rec["plain_us_median"]
        row_steps = int(ln.sum())
        nbytes = row_steps * ROW_BYTES + k * 14 * 4  # + row 0 of every recorded episode
        rec["trace"][str(k)] = {"us": samples[k], "us_median": med, "overhead_us": over,
                                "overhead_over_plain_spread": over / rec["plain_us_spread"],
                                "recorded_env_steps": row_steps, "recorded_bytes": nbytes,
                                "bytes_per_s_of_overhead": nbytes / (over * 1e-6) if over > rec["plain_us_spread"] else None,
                                "lengths_equal_ep_length": bool(torch.equal(ev.trace.length[0],
                                                                            res.ep_length[0, ev.trace.env_ids]))}
    if args.parent:
        with open(args.parent) as f:
            rec["parent"] = json.load(f)
    b.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
