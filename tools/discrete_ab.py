#!/usr/bin/env python
"""What the Categorical policy of the discrete 3DOF actions costs on the device beside the Gaussian one,
HIP events, one JSON record.

    python tools/discrete_ab.py [--rows 1048576] [--batch 65536] [--envs 65536] [--runs 7] [--replays 10]
                                [--out FILE]

3DOF shapes (7 observations), fp32, synthetic rows (the kernels' time does not depend on the values).
Learner, one permutation cut into rows / batch minibatches, on copies of one policy each:
  discrete  rows / batch CHAINED rr_ppo_update_discrete calls (4 choices) captured in one graph, each call
            handing the next one its advantage statistics: 3 launches per minibatch
  gaussian  the same for rr_ppo_update at (7, 2)
  autograd  the discrete minibatches through ppo_update's PyTorch loss (index, forward, loss, backward,
            clip_grad_norm_, Adam(capturable).step()), eager, one synchronise at the end
Act, N = --envs rows of obs, 16 launches captured in a graph:
  act_discrete  rr_policy_act_discrete            act_gaussian  rr_policy_act at (7, 2)
A run times `--replays` graph replays (or one eager pass) between two events; the runs alternate between
the arms in one session, `--runs` of each. The record holds every run, the medians and each arm's spread
(max - min), in us per minibatch (learner) and us per launch (act).
"""
import argparse
import copy
import ctypes
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
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from rl_rocket_amd import _lib, build
    from rl_rocket_amd.batch import _ptr as p
    from rl_rocket_amd.learner import _ppo_loss
    from rl_rocket_amd.rollout import (MlpActorCritic, MlpCategoricalActorCritic, PolicyPack, PPOUpdate,
                                       PPOUpdateDiscrete)

    if not torch.cuda.is_available():
        raise SystemExit("discrete_ab.py measures on the GPU; no HIP device found")
    dev = torch.device("cuda", 0)
    m, bs, ns, k = args.rows, args.batch, 7, 4
    if m % bs or m // bs < 2:
        raise SystemExit("--rows must be a multiple (>= 2) of --batch")
    g = torch.Generator(dev).manual_seed(0)
    f = dict(device=dev, dtype=torch.float32, generator=g)
    torch.manual_seed(0)
    cat, gau = MlpCategoricalActorCritic(ns, k).to(dev), MlpActorCritic(ns, 2).to(dev)
    obs = 0.7 * torch.randn((m, ns), **f)
    adv, ret = torch.randn((m,), **f), torch.randn((m,), **f)
    with torch.no_grad():
        logits = cat(obs)[0]
        a_cat = torch.multinomial(torch.softmax(logits, -1), 1, generator=g).float()
        lp_cat = cat.log_prob(logits, a_cat) + 0.1 * torch.randn((m,), **f)
        a_gau = torch.randn((m, 2), **f).clamp(-1.0, 1.0)
        lp_gau = gau.log_prob(gau(obs)[0], a_gau) + 0.1 * torch.randn((m,), **f)
    perm = torch.randperm(m, device=dev, generator=g)
    mbs = [perm[s:s + bs] for s in range(0, m, bs)]
    nxt = mbs[1:] + mbs[:1]  # the last call of a pass prepares the first of the next replay

    def rollout(acts, lp, na):
        return types.SimpleNamespace(n_steps=1, env=types.SimpleNamespace(num_envs=m, state_dim=ns, action_dim=na),
                                     obs=obs.view(1, m, ns), actions=acts.view(1, m, -1), log_probs=lp.view(1, m),
                                     advantages=adv.view(1, m), returns=ret.view(1, m))

    def adam(pol):
        return torch.optim.Adam(pol.parameters(), lr=1e-3, capturable=True)

    def graphed(first, rest):
        """`first()` eagerly (it packs), then `rest()` captured."""
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

    p_d, p_g, p_a = copy.deepcopy(cat), copy.deepcopy(gau), copy.deepcopy(cat)
    ro_d, ro_g = rollout(a_cat, lp_cat, 2), rollout(a_gau, lp_gau, 2)
    upd_d = PPOUpdateDiscrete(p_d, adam(p_d), ro_d, bs)
    g_d = graphed(lambda: upd_d(mbs[-1], mbs[0]), lambda: [upd_d(i, n, chained=True) for i, n in zip(mbs, nxt)])
    upd_g = PPOUpdate(p_g, adam(p_g), ro_g, bs)
    g_g = graphed(lambda: upd_g(mbs[-1], mbs[0]), lambda: [upd_g(i, n, chained=True) for i, n in zip(mbs, nxt)])
    o_a = adam(p_a)

    def autograd_pass():
        for idx in mbs:
            loss = _ppo_loss(p_a, obs[idx], a_cat[idx], lp_cat[idx], adv[idx], ret[idx], None, bs, 0.2, 0.01, 0.5, 0.0,
                             True)[0]
            o_a.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(p_a.parameters(), 0.5)
            o_a.step()

    autograd_pass()
    torch.cuda.synchronize()

    # the act launches: 16 per replay, t = 0 .. 15
    lib, n = _lib.load(), args.envs
    acts_per_replay = 16
    o_act = obs[:n].contiguous()
    it = torch.zeros(1, dtype=torch.int64, device=dev)
    pk_d, pk_g = PolicyPack(cat, ns, k, dev), PolicyPack(gau, ns, 2, dev)
    pk_d.pack(), pk_g.pack()
    table = (ctypes.c_float * (2 * k))(*cat.table.reshape(-1).tolist())
    z = dict(device=dev, dtype=torch.float32)
    env_a, val, lp = torch.zeros((n, 2), **z), torch.zeros(n, **z), torch.zeros(n, **z)
    act_d, act_g = torch.zeros(n, **z), torch.zeros((n, 2), **z)

    def act_discrete():
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for t in range(acts_per_replay):
            _lib.check(lib.rr_policy_act_discrete(p(pk_d.buf), ns, k, table, 0, n, 0, p(o_act), 1, p(it), t, p(env_a),
                                                  p(act_d), p(val), p(lp), None, None, None, None, 0.99, None, None, None,
                                                  stream), "rr_policy_act_discrete")

    def act_gaussian():
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for t in range(acts_per_replay):
            _lib.check(lib.rr_policy_act(p(pk_g.buf), ns, 2, 0, n, 0, p(o_act), 1, p(it), t, p(env_a), p(act_g), p(val),
                                         p(lp), None, None, None, None, 0.99, None, None, None, stream), "rr_policy_act")

    g_ad, g_ag = graphed(lambda: None, act_discrete), graphed(lambda: None, act_gaussian)

    def timed(fn, passes, per):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(passes):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1000.0 / (passes * per)

    arms = {"discrete": (g_d.replay, args.replays, len(mbs)), "gaussian": (g_g.replay, args.replays, len(mbs)),
            "autograd": (autograd_pass, 1, len(mbs)), "act_discrete": (g_ad.replay, args.replays, acts_per_replay),
            "act_gaussian": (g_ag.replay, args.replays, acts_per_replay)}
    samples = {name: [] for name in arms}
    for _ in range(args.runs):
        for name, (fn, passes, per) in arms.items():
            samples[name].append(timed(fn, passes, per))
    med = {name: statistics.median(v) for name, v in samples.items()}
    finite = all(bool(torch.isfinite(t).all()) for pol in (p_d, p_g, p_a) for t in pol.parameters())
    rec = {"rows": m, "batch": bs, "envs": n, "model": "3DOF", "n_choices": k, "minibatches_per_pass": len(mbs),
           "act_launches_per_replay": acts_per_replay, "runs": args.runs, "replays_per_run": args.replays,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "source_hash": build.source_hash(),
           "unit": "us per minibatch (discrete / gaussian: chained calls in a graph replay; autograd: eager) and us "
                   "per launch (act_*: 16 launches in a graph replay); HIP events",
           "parameters_finite_after": finite, "discrete_last_stats": upd_d.stats.tolist(),
           "discrete_over_gaussian": med["discrete"] / med["gaussian"],
           "autograd_over_discrete": med["autograd"] / med["discrete"],
           "act_discrete_over_act_gaussian": med["act_discrete"] / med["act_gaussian"]}
    for name in arms:
        rec[name] = {"us": samples[name], "median": med[name], "spread": max(samples[name]) - min(samples[name])}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
