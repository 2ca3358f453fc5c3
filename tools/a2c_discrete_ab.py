#!/usr/bin/env python
"""What a Categorical A2C update and a whole Categorical A2C iteration cost on the device, HIP events, one
JSON record.

    python tools/a2c_discrete_ab.py [--envs 65536] [--steps 5] [--choices 4] [--runs 7] [--replays 100] [--out FILE]

3DOF, fp32, one real rollout of --envs x --steps rows collected once with the Categorical policy
(DeviceRollout(one_launch=True)); the update legs run on its rows, on copies of one policy:
  a2c_discrete       rr_a2c_update_discrete on the whole rollout with RMSpropTFLike (A2CUpdateDiscrete), one
                     call captured in a graph: four launches
  ppo_discrete_opts  rr_ppo_update_discrete_opts on the same rows as ONE minibatch, normalize_advantage=False,
                     no value clip, unchained (PPOUpdate), one call captured in a graph: four launches, the
                     same towers and one softmax, with the probability ratio. The yardstick: this call
                     exists without the new unit
  a2c_gauss          rr_a2c_update at (7, 2) on a Gaussian 3DOF rollout of the same size (A2CUpdate), one call
                     captured in a graph: the same towers with the Gaussian head
  autograd           the same loss through a2c_update_discrete(fused=False): forward, loss, backward,
                     clip_grad_norm_, RMSpropTFLike.step(), eager, one synchronise at the end
  iteration          one GraphedA2CDiscrete.step() on a batch of its own: the policy's packing, the one-launch
                     Categorical collect and the update in one graph replay, with env-steps/s end to end
A run times --replays replays (autograd: --replays eager calls) between two events and reports us per call;
the runs alternate between the legs in one session, --runs of each. The record holds every run, the medians
and min .. max.
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
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--choices", type=int, default=4)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.a2c import A2CUpdate, RMSpropTFLike
    from rl_rocket_amd.a2c_discrete import A2CUpdateDiscrete, GraphedA2CDiscrete, a2c_update_discrete
    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.rollout import DeviceRollout, MlpActorCritic, MlpCategoricalActorCritic, PPOUpdate

    if not torch.cuda.is_available():
        raise SystemExit("a2c_discrete_ab.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    n_envs, T, K = args.envs, args.steps, args.choices
    rows = n_envs * T
    tables = {4: ((0.0, -1.0), (-1.0, 1.0), (0.0, 1.0), (1.0, 1.0)), 3: ((0.0, -1.0), (-0.5, 0.25), (0.75, 1.0)),
              2: ((0.0, -1.0), (0.0, 1.0))}

    def batch(seed):
        return RocketBatch(n_envs, model=3, device=dev, max_episode_steps=400, seed=seed)

    torch.manual_seed(0)
    pol = MlpCategoricalActorCritic(7, K, tables[K]).to(dev)
    env = batch(1)
    ro = DeviceRollout(env, pol, n_steps=T, gae_lambda=1.0, seed=1, one_launch=True)
    ro.collect()
    torch.cuda.synchronize()
    coef = dict(ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)

    def graphed(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        return graph

    p_a, p_b, p_c = (copy.deepcopy(pol) for _ in range(3))
    a2c = A2CUpdateDiscrete(p_a, RMSpropTFLike(p_a.parameters(), lr=7e-4), ro, **coef)
    g_a = graphed(a2c)
    ppo = PPOUpdate(p_b, torch.optim.Adam(p_b.parameters(), lr=7e-4, capturable=True), ro, rows, ent_coef=0.01,
                    normalize_advantage=False)
    assert ppo._call == "rr_ppo_update_discrete_opts"
    every = torch.arange(rows, device=dev)
    g_b = graphed(lambda: ppo(every))
    o_c = RMSpropTFLike(p_c.parameters(), lr=7e-4)

    def autograd():
        a2c_update_discrete(p_c, o_c, ro, fused=False, **coef)

    autograd()
    # the Gaussian call at (7, 2) on a rollout of its own
    p_g = MlpActorCritic(7, 2).to(dev)
    env_g = batch(3)
    ro_g = DeviceRollout(env_g, p_g, n_steps=T, gae_lambda=1.0, seed=3)
    ro_g.collect()
    gauss = A2CUpdate(p_g, RMSpropTFLike(p_g.parameters(), lr=7e-4), ro_g, **coef)
    g_g = graphed(gauss)
    env_d = batch(2)
    p_d = copy.deepcopy(pol)
    ro_d = DeviceRollout(env_d, p_d, n_steps=T, gae_lambda=1.0, seed=2, one_launch=True)
    it = GraphedA2CDiscrete(p_d, RMSpropTFLike(p_d.parameters(), lr=7e-4), ro_d, **coef)
    for _ in range(2):
        it.step()
    torch.cuda.synchronize()
    arms = {"a2c_discrete": g_a.replay, "ppo_discrete_opts": g_b.replay, "a2c_gauss": g_g.replay,
            "autograd": autograd, "iteration": it.step}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.replays):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / args.replays  # us per call

    samples = {a: [] for a in arms}
    for _ in range(args.runs):
        for a, fn in arms.items():
            samples[a].append(timed(fn))
    med = {a: statistics.median(v) for a, v in samples.items()}
    finite = all(bool(torch.isfinite(t).all()) for p in (p_a, p_b, p_c, p_d, p_g) for t in p.parameters())
    rec = {"model": "3DOF", "envs": n_envs, "n_steps": T, "rows": rows, "n_choices": K, "runs": args.runs,
           "replays_per_run": args.replays, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(_lib.LIB_PATH), "source_hash": build.source_hash(),
           "unit": "us per call (HIP events; a2c_discrete / ppo_discrete_opts / a2c_gauss / iteration: graph "
                   "replays; autograd: eager)",
           "parameters_finite_after": finite, "a2c_discrete_last_stats": a2c.last_stats(),
           "a2c_discrete_over_ppo_discrete_opts": med["a2c_discrete"] / med["ppo_discrete_opts"],
           "a2c_discrete_over_a2c_gauss": med["a2c_discrete"] / med["a2c_gauss"],
           "autograd_over_a2c_discrete": med["autograd"] / med["a2c_discrete"],
           "a2c_discrete_fastest_run_above_ppo_discrete_opts_slowest_run":
               min(samples["a2c_discrete"]) > max(samples["ppo_discrete_opts"]),
           "iteration_env_steps_per_s": rows / (med["iteration"] * 1e-6),
           "update_share_of_iteration": med["a2c_discrete"] / med["iteration"]}
    for a in arms:
        rec[a] = {"us": samples[a], "median": med[a], "min": min(samples[a]), "max": max(samples[a])}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
