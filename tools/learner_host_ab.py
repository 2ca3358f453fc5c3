#!/usr/bin/env python
"""Host overhead of the fused learner calls in this tree beside another tree (the parent commit,
exported and built somewhere), measured in one session with the trees alternating.

    python tools/learner_host_ab.py --parent DIR [--rounds 3] [--eager-only] [--out FILE]

The kernels of the two trees are the same machine code (tools/isa_diff.py), so what can differ is the
Python and C++ host path of a call. Every round runs, in each tree in turn (the parent first), three
children with that tree as working directory:
  bench     bench.py --mode rollout --full: the eager, graphed and fused-graphed PPO epoch and the
            training iteration (ms)
  bc_ab     tools/bc_ab.py: the chained 65 536-row rr_bc_update / rr_ppo_update minibatch in a graph
            replay (us)
  eager     this file with --child: PPOUpdate.__call__, BCUpdate.__call__ and, for the Categorical policy
            (3DOF, 4 choices), PPOUpdateDiscrete.__call__ and BCUpdate.__call__, called eagerly at batch
            64, where the host path dominates: 7 runs of 2000 calls between two synchronises on the host
            clock, the median run (us per call)
--eager-only runs the third child alone (a change that touches only the C++ host path of a call).
The bar is the parent's own run-to-run spread (max - min over its rounds): this tree's median over
the rounds may not lie above the parent's median by more than that. The record holds every raw
number. A child that fails or exceeds its time limit ends the measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ["bench.py", "--gpus", "1", "--mode", "rollout", "--full", "--steps", "256", "--warmup", "16",
         "--no-cpu-baseline", "--no-sb3-legs", "--no-gather-leg", "--n-sweep", ""]


def child():
    """us per eager call of PPOUpdate, BCUpdate and the Categorical policy's two at batch 64, from the tree
    in the working directory."""
    sys.path.insert(0, os.getcwd())
    import types

    import torch
    from rl_rocket_amd.bc import BCUpdate, Demonstrations
    from rl_rocket_amd.rollout import MlpActorCritic, MlpCategoricalActorCritic, PPOUpdate, PPOUpdateDiscrete

    dev = torch.device("cuda", 0)
    m, bs, ns, na = 256, 64, 14, 3
    g = torch.Generator(dev).manual_seed(0)
    f = dict(device=dev, dtype=torch.float32, generator=g)
    torch.manual_seed(0)
    obs, acts = 0.7 * torch.randn((m, ns), **f), torch.randn((m, na), **f).clamp(-1.0, 1.0)
    ro = types.SimpleNamespace(n_steps=1, env=types.SimpleNamespace(num_envs=m, state_dim=ns, action_dim=na),
                               obs=obs.view(1, m, ns), actions=acts.view(1, m, na), log_probs=torch.randn((1, m), **f),
                               advantages=torch.randn((1, m), **f), returns=torch.randn((1, m), **f))
    idx = torch.randperm(m, device=dev, generator=g)[:bs].contiguous()
    # the Categorical arm: a 3DOF rollout whose actions are one of 4 indices, as floats
    ro_d = types.SimpleNamespace(n_steps=1, env=types.SimpleNamespace(num_envs=m, state_dim=7, action_dim=2),
                                 obs=obs[:, :7].contiguous().view(1, m, 7),
                                 actions=torch.randint(0, 4, (1, m, 1), device=dev, generator=g).float(),
                                 log_probs=ro.log_probs, advantages=ro.advantages, returns=ro.returns)
    out = {}
    for name in ("ppo_update_call_us", "bc_update_call_us", "ppo_update_discrete_call_us", "bc_update_discrete_call_us"):
        pol = (MlpCategoricalActorCritic(7, 4) if "discrete" in name else MlpActorCritic(ns, na)).to(dev)
        opt = torch.optim.Adam(pol.parameters(), lr=1e-4, capturable=True)
        step = (PPOUpdateDiscrete(pol, opt, ro_d, bs) if name.startswith("ppo_update_d") else
                PPOUpdate(pol, opt, ro, bs) if name.startswith("ppo") else
                BCUpdate(pol, opt, Demonstrations(ro_d.obs[0], ro_d.actions[0]), bs) if "discrete" in name else
                BCUpdate(pol, opt, Demonstrations(obs, acts), bs))
        runs = []
        for _ in range(8):  # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2000):
                step(idx)
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / 2000 * 1e6)
        out[name] = {"us": runs[1:], "median": statistics.median(runs[1:])}
    print(json.dumps(out))


def run(cmd, cwd, limit):
    """The last JSON line a child printed; anything else ends the measurement."""
    env = dict(os.environ, PYTHONPATH=cwd)
    p = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, timeout=limit, stdout=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit("%s in %s exited with %d: stopping" % (cmd[0], cwd, p.returncode))
    return json.loads([line for line in p.stdout.splitlines() if line.startswith("{")][-1])


def measure(tree, eager_only=False):
    e = run([os.path.abspath(__file__), "--child"], tree, 300)
    eager = {"eager_" + k: v["median"] for k, v in e.items()}
    if eager_only:
        return dict(eager, raw={"eager": e})
    b = run(BENCH, tree, 300)
    a = run([os.path.join("tools", "bc_ab.py"), "--runs", "5"], tree, 300)
    upd = b["ppo_update"]
    return {"bench_eager_epoch_ms": upd["eager_epoch_ms"], "bench_graphed_epoch_ms": upd["graphed_epoch_ms"],
            "bench_fused_graphed_epoch_ms": upd["fused_graphed_epoch_ms"],
            "bench_train_iteration_ms": b["train_iteration"]["ms_per_iteration"],
            "bc_ab_bc_minibatch_us": a["bc"]["median"], "bc_ab_ppo_minibatch_us": a["ppo"]["median"],
            **eager,
            "raw": {"bench_ppo_update": upd, "bench_train_iteration": b["train_iteration"]["ms_per_iteration"],
                    "bc_ab": {k: a[k] for k in ("bc", "ppo")}, "eager": e}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the other tree: an export of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eager-only", action="store_true", help="only the eager calls' host cost")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()
    if not args.parent or args.rounds < 2:
        raise SystemExit("--parent DIR and at least 2 rounds (the bar is the parent's spread)")
    trees = {"parent": os.path.abspath(args.parent), "this": ROOT}
    rounds = {k: [] for k in trees}
    rec = {"rounds": args.rounds, "order": "parent, this, parent, this, ...", "runs": rounds}

    def write():
        print(json.dumps(rec), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(rec, indent=1) + "\n")

    for _ in range(args.rounds):
        for k, tree in trees.items():
            rounds[k].append(measure(tree, args.eager_only))
            write()  # what has been measured so far, should a later child end the run
    verdict = {}
    for m in [k for k in rounds["this"][0] if k != "raw"]:
        par, new = [r[m] for r in rounds["parent"]], [r[m] for r in rounds["this"]]
        spread = max(par) - min(par)
        verdict[m] = {"parent": par, "this": new, "parent_median": statistics.median(par),
                      "this_median": statistics.median(new), "parent_spread": spread, "parent_max": max(par),
                      "this_range": [min(new), max(new)], "below_parent_max": statistics.median(new) <= max(par),
                      "within": statistics.median(new) - statistics.median(par) <= spread}
    rec["metrics"] = verdict
    rec["verdict"] = "within the parent's spread" if all(v["within"] for v in verdict.values()) else \
        "slower than the parent's spread allows: " + ", ".join(k for k, v in verdict.items() if not v["within"])
    write()


if __name__ == "__main__":
    main()
