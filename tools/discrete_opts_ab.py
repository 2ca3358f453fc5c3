#!/usr/bin/env python
"""What SB3's options and the control block cost the Categorical policy's fused learner, HIP events, one
JSON record.

    python tools/discrete_opts_ab.py [--rows 1048576] [--batch 65536] [--runs 7] [--replays 10] [--out FILE]

3DOF (7 observations), 4 choices, fp32, synthetic rows (the kernels' time does not depend on the values).
One permutation cut into rows / batch minibatches, CHAINED calls captured in one graph per leg (3 launches
per minibatch), each leg on a copy of one policy:
  discrete   rr_ppo_update_discrete
  opts_off   rr_ppo_update_discrete_opts with the options off and the control block on (train_stats)
  opts_on    the same with clip_range_vf = 0.2, normalize_advantage = 0 and a target_kl never reached
  stopped    opts_on's graph with the block as a stop leaves it (RR_PPO_CTL_STOP and RR_PPO_CTL_DECIDE set):
             every launch returns at entry
  autograd   opts_on's loss (value clip, raw advantages) through ppo_update's PyTorch ops (index, forward,
             loss, backward, clip_grad_norm_, Adam(capturable).step()), eager, one synchronise at the end
A run times `--replays` graph replays (or one eager pass) between two events; the runs alternate between
the legs in one process, `--runs` of each. The record holds every run, the medians, each leg's spread
(max - min) and opts_off / discrete and opts_on / discrete, in us per minibatch.
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
    ap.add_argument("--rows", type=int, default=1048576)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.learner import _ppo_loss
    from rl_rocket_amd.rollout import MlpCategoricalActorCritic, PPOUpdateDiscrete

    if not torch.cuda.is_available():
        raise SystemExit("discrete_opts_ab.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    m, bs, ns, k = args.rows, args.batch, 7, 4
    if m % bs or m // bs < 2:
        raise SystemExit("--rows must be a multiple (>= 2) of --batch")
    g = torch.Generator(dev).manual_seed(0)
    f = dict(device=dev, dtype=torch.float32, generator=g)
    torch.manual_seed(0)
    cat = MlpCategoricalActorCritic(ns, k).to(dev)
    obs = 0.7 * torch.randn((m, ns), **f)
    adv, ret = torch.randn((m,), **f), torch.randn((m,), **f)
    with torch.no_grad():
        logits, value = cat(obs)
        acts = torch.multinomial(torch.softmax(logits, -1), 1, generator=g).float()
        lp = cat.log_prob(logits, acts) + 0.1 * torch.randn((m,), **f)
        old_v = value.reshape(m) + 0.3 * torch.randn((m,), **f)
    perm = torch.randperm(m, device=dev, generator=g)
    mbs = [perm[s:s + bs] for s in range(0, m, bs)]
    nxt = mbs[1:] + mbs[:1]  # the last call of a pass prepares the first of the next replay
    ro = types.SimpleNamespace(n_steps=1, env=types.SimpleNamespace(num_envs=m, state_dim=ns, action_dim=2),
                               obs=obs.view(1, m, ns), actions=acts.view(1, m, 1), log_probs=lp.view(1, m),
                               advantages=adv.view(1, m), returns=ret.view(1, m), values=old_v.view(1, m))

    def adam(pol):
        return torch.optim.Adam(pol.parameters(), lr=1e-3, capturable=True)

    def graphed(upd):
        """One eager call (it packs), then the pass of chained calls captured."""
        kw = (lambda j: dict(epoch_start=j == 0)) if upd.opts is not None else (lambda j: {})

        def rest():
            for j, (i, n) in enumerate(zip(mbs, nxt)):
                upd(i, n, chained=True, **kw(j))

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            upd(mbs[-1], mbs[0])
            rest()  # warm-up of every shape
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rest()
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        return graph

    on = dict(clip_range_vf=0.2, normalize_advantage=False, target_kl=1e6)
    legs_kw = {"discrete": {}, "opts_off": dict(train_stats=True), "opts_on": on, "stopped": on}
    pols = {name: copy.deepcopy(cat) for name in list(legs_kw) + ["autograd"]}
    upds = {name: PPOUpdateDiscrete(pols[name], adam(pols[name]), ro, bs, **kw) for name, kw in legs_kw.items()}
    graphs = {name: graphed(u) for name, u in upds.items()}
    # the block as a stop leaves it: the decision and the committed stop (the optimizer launch reads the former)
    upds["stopped"].ctl[_lib.RR_PPO_CTL_STOP] = 1.0
    upds["stopped"].ctl[_lib.RR_PPO_CTL_DECIDE] = 1.0
    torch.cuda.synchronize()
    stopped_before = [t.detach().clone() for t in pols["stopped"].parameters()]
    o_a = adam(pols["autograd"])

    def autograd_pass():
        p_a = pols["autograd"]
        for idx in mbs:
            loss = _ppo_loss(p_a, obs[idx], acts[idx], lp[idx], adv[idx], ret[idx], old_v[idx], bs, 0.2, 0.01, 0.5, 0.2,
                             False)[0]
            o_a.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(p_a.parameters(), 0.5)
            o_a.step()

    autograd_pass()
    torch.cuda.synchronize()

    def timed(fn, passes):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(passes):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / (passes * len(mbs))

    legs = {name: (graphs[name].replay, args.replays) for name in legs_kw}
    legs["autograd"] = (autograd_pass, 1)
    samples = {name: [] for name in legs}
    for _ in range(args.runs):
        for name, (fn, passes) in legs.items():
            samples[name].append(timed(fn, passes))
    med = {name: statistics.median(v) for name, v in samples.items()}
    finite = all(bool(torch.isfinite(t).all()) for pol in pols.values() for t in pol.parameters())
    unmoved = all(torch.equal(a, b) for a, b in zip(stopped_before, pols["stopped"].parameters()))
    rec = {"rows": m, "batch": bs, "model": "3DOF", "n_choices": k, "minibatches_per_pass": len(mbs), "runs": args.runs,
           "replays_per_run": args.replays, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(_lib.LIB_PATH), "source_hash": build.source_hash(),
           "unit": "us per minibatch (chained calls in a graph replay; autograd: eager); HIP events",
           "parameters_finite_after": finite, "stopped_leg_left_the_parameters": unmoved,
           "opts_on_train_stats": upds["opts_on"].train_stats(),
           "opts_off_over_discrete": med["opts_off"] / med["discrete"],
           "opts_on_over_discrete": med["opts_on"] / med["discrete"],
           "stopped_over_discrete": med["stopped"] / med["discrete"],
           "autograd_over_opts_on": med["autograd"] / med["opts_on"]}
    for name in legs:
        rec[name] = {"us": samples[name], "median": med[name], "spread": max(samples[name]) - min(samples[name])}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
