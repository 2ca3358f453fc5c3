#!/usr/bin/env python
"""What the learner's SB3 options cost an epoch (rr_ppo_update_opts against rr_ppo_update), HIP
events over replays of GraphedPPOUpdate's one-epoch graph, one JSON record.

    python tools/ppo_opts_ab.py [--n 65536] [--runs 7] [--replays 20] [--out FILE]

6DOF, fp32 policy, n_steps 16, batch 65 536 (16 chained minibatches at the default n). One collected
rollout, four learners on copies of the policy, each with its epoch captured once:
  existing   GraphedPPOUpdate with its defaults: rr_ppo_update
  opts_off   train_stats=True: rr_ppo_update_opts with every option off, the control block on
  vclip      clip_range_vf=0.2
  stopped    target_kl set and the control block's stop word already 1: every kernel returns at
             entry, the epoch costs its launches only
A run times `--replays` replays of one arm's graph between two events and reports the mean per
replay; the runs alternate between the arms in one session, `--runs` of each. The record holds every
run, the medians, each arm's spread (max - min) and its difference from the existing path's median in
us and in units of the existing path's spread.
"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import DeviceRollout, GraphedPPOUpdate, MlpActorCritic

    if not torch.cuda.is_available():
        raise SystemExit("ppo_opts_ab.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    n, T, bs = args.n, 16, 65536
    torch.manual_seed(0)
    pol = MlpActorCritic(14, 3).to(dev)
    env = RocketBatch(n, **dict(ENV_CONFIG_6DOF, model=6, device=dev, max_episode_steps=800, seed=7))
    ro = DeviceRollout(env, pol, n_steps=T, seed=3)
    ro.collect()
    torch.cuda.synchronize()

    def arm(**kw):
        p = copy.deepcopy(pol)
        opt = torch.optim.Adam(p.parameters(), lr=3e-4, eps=1e-5, capturable=True)
        upd = GraphedPPOUpdate(p, opt, ro, batch_size=min(bs, n * T), **kw)
        upd.perm.copy_(torch.randperm(n * T, device=dev))
        for _ in range(3):
            upd.graph.replay()
        torch.cuda.synchronize()
        return upd

    arms = {"existing": arm(), "opts_off": arm(train_stats=True), "vclip": arm(clip_range_vf=0.2),
            "stopped": arm(target_kl=0.01)}
    ctl = arms["stopped"]._update.ctl
    ctl.zero_()
    ctl[_lib.RR_PPO_CTL_STOP] = 1.0
    ctl[_lib.RR_PPO_CTL_DECIDE] = 1.0
    assert arms["existing"]._update.opts is None and arms["opts_off"]._update.opts is not None

    def timed(g):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.replays):
            g.replay()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.replays  # us per replay

    frozen = [p.detach().clone() for p in arms["stopped"].policy.parameters()]
    samples = {k: [] for k in arms}
    for _ in range(args.runs):
        for k, upd in arms.items():
            samples[k].append(timed(upd.graph))
    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = {k: max(v) - min(v) for k, v in samples.items()}
    rec = {"n": n, "model": "6DOF", "n_steps": T, "batch_size": min(bs, n * T), "minibatches_per_epoch": arms["existing"].n_mb,
           "runs": args.runs, "replays_per_run": args.replays, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(_lib.LIB_PATH), "source_hash": build.source_hash(), "unit": "us per epoch replay",
           "stopped_arm_left_the_parameters": all(torch.equal(a, b) for a, b in
                                                  zip(frozen, arms["stopped"].policy.parameters()))}
    for k in arms:
        rec[k] = {"us": samples[k], "median": med[k], "spread": spread[k], "minus_existing_us": med[k] - med["existing"],
                  "minus_existing_over_existing_spread": ((med[k] - med["existing"]) / spread["existing"]
                                                          if spread["existing"] else None)}
    env.close()
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
