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

    python tools/eval_bench.py --integrator dopri5 [--tl 800] [--reps 5] [--out profiles/eval_exact/eval_exact_bench.json]

  the exact mode's evaluation (rr_policy_evaluate_exact) against the step-by-step path on the same
  work: 6DOF, fp32 towers, the scaled test policy (tests/rollout_ref.py), one episode per env from a
  fresh reset under TimeLimit `--tl`. Two batches with the same seed, one evaluated with
  PolicyEvaluator(fused=True), one with fused=False (evaluate.py's _run_unfused: `--tl` iterations of
  a PyTorch policy forward, two exact steps and the state round trips), alternating, `--reps` timed
  runs each after a warm-up run, HIP events around run(). The record holds every run, the medians
  and spreads, env-steps per second, the ratio, and `--tl` x the committed rocprofv3 time of one
  step_exact_kernel launch (profiles/r06/r06h/: 25.9 us) as the "launch overhead removed, slowest
  wave of every step kept" yardstick. `fixed`: 64 steps of every env in one launch against 64 x
  (rr_policy_act + rr_step), the same work bit for bit (exact_fixed_work).

    python tools/eval_bench.py --integrator dopri5 --record [--out profiles/eval_exact_trace/eval_exact_trace_bench.json]

  the recording one-launch exact evaluation (rr_policy_evaluate_exact_trace) on the same workload,
  four legs alternating in one session, each on a batch of its own with the same seed and from the
  same reset, `--reps` timed runs each after a warm-up run (the three one-launch legs in rotating
  order, then the step-by-step leg): (a) `plain`, rr_policy_evaluate_exact;
  (b) `record_64`, the new call with 64 envs recorded, one per wave spread over the grid (env
  j * n / 64 + j); (c) `record_all`, every env recorded, with the bytes of rows it wrote; (d)
  `stepwise_64`, PolicyEvaluator(fused=False, record=) of the same 64 envs.

    python tools/eval_bench.py --integrator dopri5 --policy categorical [--out profiles/eval_exact_discrete/eval_exact_discrete_bench.json]

  the Categorical policy's one-launch exact evaluation (rr_policy_evaluate_exact_discrete) and its three
  neighbours, all 3DOF, one episode per env from a fresh reset under TimeLimit `--tl`, four legs alternating
  in one session as above (the one-launch legs in rotating order, then the step-by-step leg), `--reps` >= 5
  timed runs each after a warm-up run: (1) `exact_discrete`, the new call with tests/discrete_ref.cat_policy(4, 1);
  (2) `stepwise`, PolicyEvaluator(fused=False) with the same policy on a batch with the same seed;
  (3) `exact_gaussian`, rr_policy_evaluate_exact with tests/rollout_ref.scaled_policy(7, 2, seed=5);
  (4) `rk4_discrete`, rr_policy_evaluate_discrete on an RK4 batch with the policy of (1).

    python tools/eval_bench.py --sampled [--reps 7] [--out profiles/eval_sampled/eval_sampled_bench.json]

  the sampled-action evaluation (rr_policy_evaluate_sampled, PolicyEvaluator(deterministic=False)), 6DOF, fp32,
  RK4, tests/rollout_ref.scaled_policy(14, 3, seed=5, head_scale=1.0) at log_std = -1, `--reps` >= 7 samples of
  every leg, the legs alternating in rotating order in one process, medians with min .. max.
  `per_step`: n_episodes = max_steps = 64 under TimeLimit 800 (no env ends 64 episodes in 64 steps, so every env
  steps 64 times in every call), the sampled call beside rr_policy_evaluate and beside a 64-step
  rr_rollout_collect with the same (seed, iter) on twin batches; a sample is a block of `--calls` calls, in us
  per call and per step. The collect and the sampled evaluation draw the same noise, so their batches must end
  in the same state (`same_state_as_collect`). `whole`: one episode per env from a fresh reset, sampled beside
  deterministic, and sampled with 64 envs recorded (one per wave spread over the grid) and with every env
  recorded; a sample is one call.
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
    ap.add_argument("--integrator", choices=("rk4", "dopri5"), default="rk4")
    ap.add_argument("--tl", type=int, default=800, help="TimeLimit of the dopri5 leg")
    ap.add_argument("--record", action="store_true", help="the dopri5 leg's recording comparison")
    ap.add_argument("--policy", choices=("gaussian", "categorical"), default="gaussian",
                    help="categorical: the dopri5 leg's comparison of the Categorical policy's one-launch evaluation")
    ap.add_argument("--sampled", action="store_true", help="the sampled-action evaluation's comparison (RK4)")
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

    def write(rec):
        print(json.dumps(rec))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(rec, indent=1) + "\n")

    if args.sampled:
        if args.integrator != "rk4" or args.record or args.policy != "gaussian":
            raise SystemExit("--sampled goes alone")
        write(sampled_leg(args, rec, dev))
        return
    if args.policy == "categorical":
        if args.integrator != "dopri5" or args.record:
            raise SystemExit("--policy categorical goes with --integrator dopri5 and without --record")
        write(exact_discrete_leg(args, rec, dev))
        return
    if args.integrator == "dopri5":
        write(exact_trace_leg(args, rec, dev) if args.record else exact_leg(args, rec, dev))
        return

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
    write(rec)


# rocprofv3 kernel time of one step_exact_kernel launch at N = 65 536, 6DOF (profiles/r06/r06h/)
STEP_EXACT_US = 25.9


def exact_leg(args, rec, dev):
    """The --integrator dopri5 record (see the module docstring)."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import PolicyEvaluator

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from rollout_ref import scaled_policy

    n, tl = args.n, args.tl
    pol = scaled_policy(14, 3, seed=5, head_scale=1.0).to(dev)
    rec.update(integrator="dopri5", max_episode_steps=tl, policy="tests/rollout_ref.scaled_policy(14, 3, seed=5, "
               "head_scale=1.0)", n_episodes=1, reps=args.reps)
    legs = {}
    for name, fused in (("fused", True), ("unfused", False)):
        b = RocketBatch(n, model=6, device=dev, max_episode_steps=tl, integrator="dopri5",
                        **dict(ENV_CONFIG_6DOF, seed=1234))
        legs[name] = (b, PolicyEvaluator(b, pol, n_episodes=1, fused=fused), [])
    for r in range(args.reps + 1):  # run 0 is the warm-up; the two legs alternate, each from the same reset
        for name, (b, e, runs) in legs.items():
            b.reset()
            torch.cuda.synchronize()
            us = timed(e.run, 1)
            ln = e.result.ep_length[0].long()
            waves = torch.nn.functional.pad(ln, (0, (-n) % 64)).view(-1, 64).max(dim=1).values
            s = e.result.stats()
            if r:
                runs.append({"us": us, "env_steps": int(ln.sum()), "wave_steps": int(waves.sum()),
                             "wave_steps_max": int(waves.max()),
                             "env_steps_per_s": float(ln.sum()) / (us * 1e-6), "mean_ep_length": s["mean_ep_length"],
                             "mean_reward": s["mean_reward"], "landing_success": s["ep_statistic/landing_success"],
                             "episodes": s["episodes"], "unfinished": s["unfinished"]})
    for name, (b, e, runs) in legs.items():
        us = [x["us"] for x in runs]
        rec[name] = {"runs": runs, "us_median": statistics.median(us), "us_min": min(us), "us_max": max(us),
                     "env_steps_per_s_median": statistics.median(x["env_steps_per_s"] for x in runs)}
        b.close()
    f, u = rec["fused"], rec["unfused"]
    yard = tl * STEP_EXACT_US
    # the longest wave of the one-launch call: the launches a step-by-step loop that could leave early would need
    longest = statistics.median(x["wave_steps_max"] for x in f["runs"])
    rec.update(longest_wave_steps_median=longest, yardstick_longest_wave_us=longest * STEP_EXACT_US,
               fused_us_per_step_of_longest_wave=f["us_median"] / longest)
    rec.update(ratio_unfused_over_fused=u["us_median"] / f["us_median"],
               spreads_overlap=bool(f["us_max"] >= u["us_min"]),
               yardstick_us=yard, yardstick="%d x %.1f us (one step_exact_kernel launch, profiles/r06/r06h/)"
               % (tl, STEP_EXACT_US), yardstick_over_fused=yard / f["us_median"])
    rec["fixed"] = exact_fixed_work(args, dev, pol)
    return rec


def exact_trace_leg(args, rec, dev):
    """The --integrator dopri5 --record record (see the module docstring)."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import PolicyEvaluator

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from rollout_ref import scaled_policy

    n, tl = args.n, args.tl
    if n % 64 or args.reps < 5:
        raise SystemExit("--record needs n a multiple of 64 and --reps >= 5")
    pol = scaled_policy(14, 3, seed=5, head_scale=1.0).to(dev)
    ids64 = [j * (n // 64) + j for j in range(64)]  # lane j of every (n / 4096)-th wave
    rec.update(integrator="dopri5", max_episode_steps=tl, policy="tests/rollout_ref.scaled_policy(14, 3, seed=5, "
               "head_scale=1.0)", n_episodes=1, reps=args.reps, recorded_64=ids64)
    legs = {}
    for name, kw in (("plain", dict(fused=True)),
                     ("record_64", dict(fused=True, record=ids64, record_in_launch=True)),
                     ("record_all", dict(fused=True, record=torch.arange(n), record_in_launch=True)),
                     ("stepwise_64", dict(fused=False, record=ids64))):
        b = RocketBatch(n, model=6, device=dev, max_episode_steps=tl, integrator="dopri5",
                        **dict(ENV_CONFIG_6DOF, seed=1234))
        legs[name] = (b, PolicyEvaluator(b, pol, n_episodes=1, **kw), [])
    one = ["plain", "record_64", "record_all"]
    for r in range(args.reps + 1):  # run 0 is the warm-up; the legs alternate, each from the same reset
        # the one-launch legs rotate, so that each of them follows the long step-by-step leg in turn
        order = one[r % 3:] + one[:r % 3] + ["stepwise_64"]
        for pos, name in enumerate(order):
            b, e, runs = legs[name]
            b.reset()
            torch.cuda.synchronize()
            us = timed(e.run, 1)
            ln = e.result.ep_length[0].long()
            waves = torch.nn.functional.pad(ln, (0, (-n) % 64)).view(-1, 64).max(dim=1).values
            row = {"us": us, "position_in_round": pos, "env_steps": int(ln.sum()), "wave_steps_max": int(waves.max()),
                   "unfinished": int((e.result.episodes < 1).sum())}
            if e.trace is not None:  # rows written: length + 1 state rows, length action and terms rows, the length word
                tr = e.trace
                L = tr.length[0].long().clamp(max=tr.steps)
                per_step = 4 * (tr.state.shape[-1] + tr.action.shape[-1] + tr.terms.shape[-1])
                row.update(recorded_env_steps=int(L.sum()),
                           trace_bytes=int(L.sum()) * per_step + L.numel() * (4 * tr.state.shape[-1] + 4),
                           lengths_equal_ep_length=bool(torch.equal(tr.length[0].long(), ln[tr.env_ids])))
            if r:
                runs.append(row)
    for name, (b, e, runs) in legs.items():
        us = [x["us"] for x in runs]
        rec[name] = {"runs": runs, "us_median": statistics.median(us), "us_min": min(us), "us_max": max(us)}
        b.close()
    a = rec["plain"]
    spread = a["us_max"] - a["us_min"]
    rec["plain_spread_us"] = spread
    for name in ("record_64", "record_all", "stepwise_64"):
        x = rec[name]
        x["over_plain_median_us"] = x["us_median"] - a["us_median"]
        x["median_over_plain_max_us"] = x["us_median"] - a["us_max"]
        x["exceeds_plain_max_by_more_than_its_spread"] = bool(x["us_median"] - a["us_max"] > spread)
    rec["stepwise_over_record_64"] = rec["stepwise_64"]["us_median"] / rec["record_64"]["us_median"]
    return rec


def exact_discrete_leg(args, rec, dev):
    """The --integrator dopri5 --policy categorical record (see the module docstring)."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.rollout import PolicyEvaluator

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from discrete_ref import cat_policy
    from rollout_ref import scaled_policy

    n, tl = args.n, args.tl
    if args.reps < 5:
        raise SystemExit("--policy categorical needs --reps >= 5")
    cat = cat_policy(4, 1).to(dev)
    gauss = scaled_policy(7, 2, seed=5, head_scale=1.0).to(dev)
    rec.update(model="3DOF", integrator="dopri5 (rk4_discrete: rk4)", max_episode_steps=tl, n_episodes=1, reps=args.reps,
               policy="tests/discrete_ref.cat_policy(4, 1); exact_gaussian: tests/rollout_ref.scaled_policy(7, 2, "
               "seed=5, head_scale=1.0)")
    legs = {}
    for name, pol, integ, fused in (("exact_discrete", cat, "dopri5", True), ("exact_gaussian", gauss, "dopri5", True),
                                    ("rk4_discrete", cat, "rk4", True), ("stepwise", cat, "dopri5", False)):
        b = RocketBatch(n, model=3, device=dev, max_episode_steps=tl, integrator=integ, seed=1234)
        e = PolicyEvaluator(b, pol, n_episodes=1, fused=fused)
        assert e.fused == fused
        legs[name] = (b, e, [])
    one = ["exact_discrete", "exact_gaussian", "rk4_discrete"]
    for r in range(args.reps + 1):  # run 0 is the warm-up; the legs alternate, each from the same reset
        # the one-launch legs rotate, so that each of them follows the long step-by-step leg in turn
        order = one[r % 3:] + one[:r % 3] + ["stepwise"]
        for pos, name in enumerate(order):
            b, e, runs = legs[name]
            b.reset()
            torch.cuda.synchronize()
            us = timed(e.run, 1)
            ln = e.result.ep_length[0].long()
            waves = torch.nn.functional.pad(ln, (0, (-n) % 64)).view(-1, 64).max(dim=1).values
            s = e.result.stats()
            if r:
                runs.append({"us": us, "position_in_round": pos, "env_steps": int(ln.sum()),
                             "wave_steps": int(waves.sum()), "wave_steps_max": int(waves.max()),
                             "env_steps_per_s": float(ln.sum()) / (us * 1e-6), "mean_ep_length": s["mean_ep_length"],
                             "mean_reward": s["mean_reward"], "episodes": s["episodes"], "unfinished": s["unfinished"]})
    for name, (b, e, runs) in legs.items():
        us = [x["us"] for x in runs]
        rec[name] = {"runs": runs, "us_median": statistics.median(us), "us_min": min(us), "us_max": max(us)}
        b.close()
    x = rec["exact_discrete"]
    rec["stepwise_over_exact_discrete"] = rec["stepwise"]["us_median"] / x["us_median"]
    rec["stepwise_min_over_exact_discrete_max"] = rec["stepwise"]["us_min"] / x["us_max"]
    rec["exact_discrete_over_exact_gaussian"] = x["us_median"] / rec["exact_gaussian"]["us_median"]
    rec["exact_discrete_over_rk4_discrete"] = x["us_median"] / rec["rk4_discrete"]["us_median"]
    rec["gate_10x"] = bool(rec["stepwise_over_exact_discrete"] >= 10.0)
    return rec


def sampled_leg(args, rec, dev, k=64):
    """The --sampled record (see the module docstring)."""
    import torch
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import DeviceRollout, PolicyEvaluator

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from rollout_ref import scaled_policy

    n, reps = args.n, max(args.reps, 7)
    if n % 64:
        raise SystemExit("--sampled needs n a multiple of 64")
    pol = scaled_policy(14, 3, seed=5, head_scale=1.0)
    with torch.no_grad():
        pol.log_std.fill_(-1.0)
    pol = pol.to(dev)
    rec.update(integrator="rk4", policy="tests/rollout_ref.scaled_policy(14, 3, seed=5, head_scale=1.0), log_std = -1",
               reps=reps, seed=11)

    def env():
        b = RocketBatch(n, model=6, device=dev, max_episode_steps=800, **dict(ENV_CONFIG_6DOF, seed=1234))
        b.reset()
        return b

    def summary(us):
        return {"us": us, "us_median": statistics.median(us), "us_min": min(us), "us_max": max(us)}

    # ---- (a) the cost of a step: k steps of every env in every call ----
    ro = DeviceRollout(env(), pol, n_steps=k, policy_dtype="fp32", seed=11)
    legs = {"collect": (ro.env, ro.collect),
            "sampled": None, "deterministic": None}
    start = ro.env.checkpoint()  # (DeviceRollout reset its batch once more: the twins start where it starts)
    for name, kw in (("sampled", dict(deterministic=False, seed=11)), ("deterministic", {})):
        b = env()
        b.restore(start)
        legs[name] = (b, PolicyEvaluator(b, pol, n_episodes=k, max_steps=k, **kw).run)
    order = list(legs)
    for _ in range(10):  # warm-up: code objects loaded, episodes spread over their lengths
        for name in order:
            legs[name][1]()
    torch.cuda.synchronize()
    t = {name: [] for name in order}
    for r in range(reps):
        for name in order[r % 3:] + order[:r % 3]:
            t[name].append(timed(legs[name][1], args.calls))
    same = all(torch.equal(x, y) for x, y in zip(legs["collect"][0].get_state(), legs["sampled"][0].get_state()))
    per = {"steps": k, "calls_per_sample": args.calls, "same_state_as_collect": bool(same)}
    for name in order:
        per[name] = summary(t[name])
        per[name]["us_per_step_median"] = per[name]["us_median"] / k
        legs[name][0].close()
    per["sampled_below_collect"] = bool(per["sampled"]["us_median"] < per["collect"]["us_median"])
    per["sampled_max_below_collect_min"] = bool(per["sampled"]["us_max"] < per["collect"]["us_min"])
    per["sampled_over_deterministic"] = per["sampled"]["us_median"] / per["deterministic"]["us_median"]
    per["sampled_over_collect"] = per["sampled"]["us_median"] / per["collect"]["us_median"]
    rec["per_step"] = per

    # ---- (b) whole evaluations: one episode per env from a fresh reset ----
    ids64 = [j * (n // 64) + j for j in range(64)]  # lane j of every (n / 4096)-th wave
    rec["recorded_64"] = ids64
    sam = dict(deterministic=False, seed=11)
    whole = {}
    for name, kw in (("deterministic", {}), ("sampled", sam), ("sampled_record_64", dict(sam, record=ids64)),
                     ("sampled_record_all", dict(sam, record=torch.arange(n)))):
        b = env()
        whole[name] = (b, PolicyEvaluator(b, pol, n_episodes=1, **kw), [])
    order = list(whole)
    for r in range(reps + 1):  # run 0 is the warm-up; the legs alternate in rotating order
        for name in order[r % 4:] + order[:r % 4]:
            b, e, runs = whole[name]
            b.reset()
            torch.cuda.synchronize()
            us = timed(e.run, 1)
            ln = e.result.ep_length[0].long()
            waves = ln.view(-1, 64).max(dim=1).values
            row = {"us": us, "env_steps": int(ln.sum()), "wave_steps": int(waves.sum()), "wave_steps_max": int(waves.max()),
                   "unfinished": int((e.result.episodes < 1).sum())}
            if e.trace is not None:  # rows written: length + 1 state rows, length action and terms rows, the length word
                tr = e.trace
                L = tr.length[0].long().clamp(max=tr.steps)
                per_row = 4 * (tr.state.shape[-1] + tr.action.shape[-1] + tr.terms.shape[-1])
                row["trace_bytes"] = int(L.sum()) * per_row + L.numel() * (4 * tr.state.shape[-1] + 4)
            if r:
                runs.append(row)
    out = {}
    for name, (b, e, runs) in whole.items():
        out[name] = dict(summary([x["us"] for x in runs]), runs=runs,
                         us_per_wave_step_of_longest_wave=statistics.median(x["us"] / x["wave_steps_max"] for x in runs))
        b.close()
    out["sampled_over_deterministic"] = out["sampled"]["us_median"] / out["deterministic"]["us_median"]
    for name in ("sampled_record_64", "sampled_record_all"):
        out[name]["over_sampled_median_us"] = out[name]["us_median"] - out["sampled"]["us_median"]
    rec["whole"] = out
    return rec


def exact_fixed_work(args, dev, pol, k=64):
    """The same `k` steps of every env, once in one launch (n_episodes = max_steps = k: no env ends k
    episodes in k steps, so every wave runs k iterations with all lanes stepping) and once as k times
    rr_policy_act + rr_step, from the same reset, alternating. log_std = -60 makes rr_policy_act's
    action the mean, and the stepped batch starts from the exact mode's obs rows, so both paths do the
    same arithmetic: `same_state` records that they end in the same fp64 state bit for bit. What
    differs is where the waves meet: never, or after every step."""
    import copy
    import ctypes

    import numpy as np
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import RocketBatch, _ptr
    from rl_rocket_amd.params import ENV_CONFIG_6DOF
    from rl_rocket_amd.rollout import PolicyEvaluator, PolicyPack

    n = args.n
    pol = copy.deepcopy(pol)
    with torch.no_grad():
        pol.log_std.fill_(-60.0)
    bf, bs = [RocketBatch(n, model=6, device=dev, max_episode_steps=args.tl, integrator="dopri5",
                          **dict(ENV_CONFIG_6DOF, seed=1234)) for _ in range(2)]
    ev = PolicyEvaluator(bf, pol, n_episodes=k, max_steps=k, fused=True)
    pack = PolicyPack(pol, 14, 3, dev)
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=dev)
    it = torch.zeros(1, dtype=torch.int64, device=dev)
    act_env, act, val, lp = torch.zeros((n, 3), **f32), torch.zeros((n, 3), **f32), torch.zeros(n, **f32), torch.zeros(n, **f32)
    norm = torch.tensor(np.asarray(bs.cfg.state_normalizer, dtype=np.float64), device=dev)

    def stepwise():
        params = pack.pack()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for t in range(k):
            _lib.check(lib.rr_policy_act(_ptr(params), 14, 3, pack.prec, n, 0, _ptr(bs.obs), 11, _ptr(it), t,
                                         _ptr(act_env), _ptr(act), _ptr(val), _ptr(lp), None, None, None, None, 0.0,
                                         None, None, None, stream), "rr_policy_act")
            bs.step(act_env)

    one, many, same, ends = [], [], True, 0
    for r in range(args.reps + 1):  # run 0 is the warm-up
        bf.reset()
        torch.cuda.synchronize()
        t1 = timed(ev.run, 1)
        bs.reset()
        bs.obs.copy_((bs.get_state64()[0] / norm[:, None]).float().T)
        torch.cuda.synchronize()
        tk = timed(stepwise, 1)
        same = same and torch.equal(bf.get_state64()[0], bs.get_state64()[0])
        ends = int(ev.result.episodes.sum())
        if r:
            one.append(t1)
            many.append(tk)
    bf.close()
    bs.close()
    m1, mk = statistics.median(one), statistics.median(many)
    return {"steps": k, "one_launch_us": one, "stepwise_us": many, "one_launch_us_median": m1, "stepwise_us_median": mk,
            "one_launch_us_per_step": m1 / k, "stepwise_us_per_step": mk / k, "step_exact_kernel_us": STEP_EXACT_US,
            "same_state": bool(same), "episode_ends_in_the_last_run": ends,
            "stepwise": "k x (rr_policy_act + rr_step), direct launches from Python, HIP events around the loop"}


if __name__ == "__main__":
    main()
