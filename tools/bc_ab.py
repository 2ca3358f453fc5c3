#!/usr/bin/env python
"""What a behaviour-cloning minibatch costs on the device (rr_bc_update, rr_bc_update_discrete) beside the
same minibatch in PyTorch autograd and beside a PPO minibatch of the same policy, HIP events, one JSON record.

    python tools/bc_ab.py [--policy gaussian|categorical] [--rows 1048576] [--batch 65536] [--runs 7]
                          [--replays 10] [--out FILE]

fp32, synthetic rows (the kernels' time does not depend on the values; the Categorical policy's indices are
valid), one permutation cut into rows / batch minibatches. The arms, on copies of one policy:
  --policy gaussian: 6DOF shapes (14 observations, 3 actions)
    bc            rows / batch CHAINED rr_bc_update calls captured in one graph (an eager call before the
                  capture leaves the packed image the first one uses): 3 launches per minibatch
    ppo           the same for rr_ppo_update with its defaults, each call handing the next one its
                  advantage statistics: 3 launches per minibatch, two towers on separate workgroups
    autograd      the same minibatches through bc_train's PyTorch path (index, forward, loss, backward,
                  Adam(capturable).step()), eager, one synchronise at the end
  --policy categorical: 3DOF shapes (7 observations), K = 4 choices
    bc_discrete   as bc, for rr_bc_update_discrete
    bc_gauss      as bc, for rr_bc_update on an MlpActorCritic(7, 2) and the same observations
    ppo_discrete  as ppo, for rr_ppo_update_discrete
    autograd      as above, for the Categorical policy
A run times `--replays` graph replays (the fused arms) or one pass over the minibatches (autograd) between
two events and reports us per minibatch; the runs alternate between the arms in one session,
`--runs` of each. The record holds every run, the medians and each arm's spread (max - min).
"""
import argparse
import copy
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", choices=("gaussian", "categorical"), default="gaussian")
    ap.add_argument("--rows", type=int, default=1048576)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.bc import BCUpdate, Demonstrations, _bc_loss
    from rl_rocket_amd.rollout import MlpActorCritic, MlpCategoricalActorCritic, PPOUpdate

    if not torch.cuda.is_available():
        raise SystemExit("bc_ab.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    cat = args.policy == "categorical"
    m, bs, k = args.rows, args.batch, 4
    ns, na = (7, 2) if cat else (14, 3)
    if m % bs or m // bs < 2:
        raise SystemExit("--rows must be a multiple (>= 2) of --batch")
    g = torch.Generator(dev).manual_seed(0)
    f = dict(device=dev, dtype=torch.float32, generator=g)
    torch.manual_seed(0)
    pol = (MlpCategoricalActorCritic(ns, k) if cat else MlpActorCritic(ns, na)).to(dev)
    gauss = MlpActorCritic(ns, 2).to(dev) if cat else None
    obs = 0.7 * torch.randn((m, ns), **f)
    if cat:
        acts = torch.randint(0, k, (m, 1), device=dev, generator=g).float()
    cont = torch.randn((m, na), **f).clamp(-1.0, 1.0)  # the Gaussian arm's actions
    if not cat:
        acts = cont
    with torch.no_grad():
        old_lp = pol.log_prob(pol(obs)[0], acts) + 0.1 * torch.randn((m,), **f)
    adv, ret = torch.randn((m,), **f), torch.randn((m,), **f)
    perm = torch.randperm(m, device=dev, generator=g)
    mbs = [perm[s:s + bs] for s in range(0, m, bs)]
    ro = types.SimpleNamespace(n_steps=1, env=types.SimpleNamespace(num_envs=m, state_dim=ns, action_dim=na),
                               obs=obs.view(1, m, ns), actions=acts.view(1, m, -1), log_probs=old_lp.view(1, m),
                               advantages=adv.view(1, m), returns=ret.view(1, m))

    def adam(p):
        return torch.optim.Adam(p.parameters(), lr=1e-3, capturable=True)

    def graphed(first, rest):
        """`first()` eagerly (it packs), then `rest()` captured: the chained minibatches of one pass."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            first()
            rest()  # warm-up of every shape
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rest()
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        return graph

    def bc_arm(p, a):
        step = BCUpdate(p, adam(p), Demonstrations(obs, a), bs)
        return step, graphed(lambda: step(mbs[-1]), lambda: [step(idx, chained=True) for idx in mbs])

    sfx = "_discrete" if cat else ""
    p_bc, p_ppo, p_ag = (copy.deepcopy(pol) for _ in range(3))
    bc, g_bc = bc_arm(p_bc, acts)
    arms = {"bc" + sfx: (g_bc.replay, args.replays)}
    if cat:
        bc_g, g_bcg = bc_arm(gauss, cont)  # bc_g owns the workspace the graph writes: it stays alive
        assert bc_g._call == "rr_bc_update"
        arms["bc_gauss"] = (g_bcg.replay, args.replays)
    ppo = PPOUpdate(p_ppo, adam(p_ppo), ro, bs)
    assert bc._call == "rr_bc_update" + sfx and ppo._call == "rr_ppo_update" + sfx
    nxt = mbs[1:] + mbs[:1]  # the last call of a pass prepares the first of the next replay
    g_ppo = graphed(lambda: ppo(mbs[-1], mbs[0]),
                    lambda: [ppo(idx, n, chained=True) for idx, n in zip(mbs, nxt)])
    arms["ppo" + sfx] = (g_ppo.replay, args.replays)
    o_ag = adam(p_ag)

    def autograd_pass():
        for idx in mbs:
            loss, _ = _bc_loss(p_ag, obs[idx], acts[idx], 1e-3, 0.0)
            o_ag.zero_grad(set_to_none=True)
            loss.backward()
            o_ag.step()

    autograd_pass()
    torch.cuda.synchronize()
    arms["autograd"] = (autograd_pass, 1)

    def timed(fn, passes):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(passes):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / (passes * len(mbs))  # us per minibatch

    samples = {a: [] for a in arms}
    for _ in range(args.runs):
        for a, (fn, passes) in arms.items():
            samples[a].append(timed(fn, passes))
    med = {a: statistics.median(v) for a, v in samples.items()}
    pols = [p_bc, p_ppo, p_ag] + ([gauss] if cat else [])
    finite = all(bool(torch.isfinite(t).all()) for p in pols for t in p.parameters())
    rec = {"rows": m, "batch": bs, "model": "3DOF" if cat else "6DOF"}
    if cat:
        rec["n_choices"] = k
    rec.update({"minibatches_per_pass": len(mbs), "runs": args.runs,
                "replays_per_run": args.replays, "device": torch.cuda.get_device_name(0),
                "library": os.path.basename(_lib.LIB_PATH), "source_hash": build.source_hash(),
                "unit": "us per minibatch (HIP events; the fused arms: chained calls in a graph replay; autograd: eager)",
                "parameters_finite_after": finite, "bc%s_last_stats" % sfx: bc.last_stats(),
                "bc%s_over_ppo%s" % (sfx, sfx): med["bc" + sfx] / med["ppo" + sfx]})
    if cat:
        rec["bc_discrete_over_bc_gauss"] = med["bc_discrete"] / med["bc_gauss"]
    rec["autograd_over_bc" + sfx] = med["autograd"] / med["bc" + sfx]
    for a in arms:
        rec[a] = {"us": samples[a], "median": med[a], "spread": max(samples[a]) - min(samples[a])}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
