"""Per-wave phase clocks of the headline step BY WAVE CLASS, in the fresh and in the steady phase of an
episode, from the RR_DIAG_STAMPS build (rocket_stamps.h): the steady-state counterpart of
tools/step_stamps_graph.py.

    RR_LIB_PATH=<diag lib> python tools/step_stamps_steady.py OUT.json [--n 65536] [--reps 5]

For each phase (restored to step 5: no env ends an episode; restored to step 150: ~1.5 % of the envs end
one per step, the phase tools/step_ab.py calls steady) a 20-launch hipGraph is replayed from the same
checkpoint and the LAST launch's stamps are read from the reward slots of each main wave's first lanes:
lanes 0-3 cycles of the four phases (entry -> past the barrier, -> state landed, -> compute done, -> tail
issued), lanes 4 / 5 the wave's s_memrealtime at entry / end (100 MHz), lanes 6-8 the done tail's
sub-stamps in cycles after the compute stamp (terminal rows issued, helper flag seen, candidate row in
registers; 0 where the wave has no done lane). Every main wave is classified from that launch's own
outputs: the `done` plane, and the status plane of a twin env (compute_terms=True, same library, same
checkpoint and actions, stepped eagerly: the stamps overwrite only reward slots, so its states are
bitwise the stamped env's) for "a lane of the wave took the ground-event path" (status 1).
Classes: none (no done lane), done (done lane, no ground event), ground (done lane with a ground event).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ("none", "done", "ground")
PHASES = ("barrier", "loads_landed", "compute", "tail")
SUBS = ("terminal_rows_issued", "flag_seen", "candidate_landed")
K = 20


def pct(v, q):
    import numpy as np

    return float(np.percentile(v, q)) if len(v) else None


def classify(done, status):
    """Wave class index per wave from [W, 64] done flags and solve status (1 = ground event)."""
    import numpy as np

    any_done = done.any(axis=1)
    ground = ((status == 1.0) & done).any(axis=1)
    return np.where(ground, 2, np.where(any_done, 1, 0))


def summarise(r, cls):
    """One replay's record from the [W, 64] reward slots `r` and the wave classes `cls`."""
    import numpy as np

    bits = r[:, 4:6].copy().view(np.uint32).astype(np.int64)
    s0 = bits[:, 0].min()
    start_us, end_us = (bits[:, 0] - s0) / 100.0, (bits[:, 1] - s0) / 100.0
    last = np.argsort(end_us, kind="stable")[-16:]
    rec = {"waves": int(len(cls)), "end_max_us": float(end_us.max()), "start_spread_us": float(start_us.max()),
           "last16_by_class": {c: int((cls[last] == k).sum()) for k, c in enumerate(CLASSES)},
           "last16_end_us": [float(x) for x in np.sort(end_us[last])], "classes": {}}
    for k, c in enumerate(CLASSES):
        w = cls == k
        d = {"waves": int(w.sum())}
        if w.any():
            for j, p in enumerate(PHASES):
                d[p + "_cycles"] = {"median": pct(r[w, j], 50), "p90": pct(r[w, j], 90)}
            tot = r[w, :4].sum(axis=1)
            d["total_cycles"] = {"median": pct(tot, 50), "p90": pct(tot, 90)}
            for j, p in enumerate(SUBS):
                v = r[w, 6 + j]
                v = v[v > 0]
                d[p + "_cycles_after_compute"] = {"waves": int(len(v)), "median": pct(v, 50), "p90": pct(v, 90)}
            d["start_us"] = {"median": pct(start_us[w], 50), "p90": pct(start_us[w], 90)}
            d["end_us"] = {"median": pct(end_us[w], 50), "p90": pct(end_us[w], 90), "max": float(end_us[w].max())}
        rec["classes"][c] = d
    return rec


def median_of(recs):
    """Field-wise median over the replays' records (same structure)."""
    import statistics

    a = recs[0]
    if isinstance(a, dict):
        return {k: median_of([x[k] for x in recs]) for k in a}
    if isinstance(a, list):
        return [median_of([x[j] for x in recs]) for j in range(len(a))]
    if a is None or any(x is None for x in recs):
        return None
    return statistics.median(recs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch

    from rl_rocket_amd.batch import RocketBatch
    from rl_rocket_amd.params import ENV_CONFIG_6DOF, MAX_EPISODE_STEPS

    dev = torch.device("cuda", 0)
    n = a.n
    gen = torch.Generator(device=dev).manual_seed(42)
    pool = torch.rand((8, n, 3), device=dev, generator=gen) * 2 - 1

    def mk(terms):
        return RocketBatch(n, model=6, device=dev, max_episode_steps=MAX_EPISODE_STEPS, auto_reset=True,
                           episode_stats=False, compute_terms=terms, **ENV_CONFIG_6DOF)

    out = {"what": __doc__.strip().splitlines()[0], "lib": os.environ.get("RR_LIB_PATH", "in-tree"), "n": n,
           "graph_launches": K,
           "clock": "cycles: s_memtime (about 2.1 per ns, DESIGN.md section 3); us: s_memrealtime, 100 MHz",
           "phases": {}}
    for phase, warm in (("fresh", 5), ("steady", 150)):
        env, twin = mk(False), mk(True)
        env.reset()
        for t in range(warm):
            env.step(pool[t % 8])
        torch.cuda.synchronize(dev)
        ck = {k: v.clone() for k, v in env.checkpoint().items()}
        # the twin's last step: the status plane of the stamped launch
        twin.reset()
        twin.restore(ck)
        for t in range(K):
            twin.step(pool[(warm + t) % 8])
        torch.cuda.synchronize(dev)
        status = twin.terms[-1].cpu().numpy()
        twin_done = twin.done.cpu().numpy()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                for t in range(K):
                    env.step(pool[(warm + t) % 8])
        torch.cuda.current_stream(dev).wait_stream(s)
        recs = []
        for rep in range(a.reps + 2):
            env.restore(ck)
            torch.cuda.synchronize(dev)
            g.replay()
            torch.cuda.synchronize(dev)
            if rep < 2:  # the first replays warm the graph
                continue
            done = env.done.cpu().numpy()
            assert (done == twin_done).all(), "the twin's done plane differs from the stamped launch's"
            pad = (-n) % 64
            r = np.pad(env.reward.cpu().numpy(), (0, pad)).reshape(-1, 64)
            cls = classify(np.pad(done, (0, pad)).reshape(-1, 64) != 0, np.pad(status, (0, pad)).reshape(-1, 64))
            rec = summarise(r, cls)
            rec["done_envs"] = int(done.sum())
            rec["ground_event_envs"] = int(((status == 1.0) & (done != 0)).sum())
            recs.append(rec)
            print(phase, json.dumps({"end_max_us": rec["end_max_us"], "last16": rec["last16_by_class"],
                                     "waves": {c: rec["classes"][c]["waves"] for c in CLASSES}}), flush=True)
        out["phases"][phase] = {"restored_to_step": warm, "median_over_replays": median_of(recs), "replays": recs}
        env.close()
        twin.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    m = out["phases"]["steady"]["median_over_replays"]["classes"]
    for c in CLASSES:
        if m[c]["waves"]:
            print("steady %-6s waves %6.0f  cycles %s  end_us median %.2f p90 %.2f" % (
                c, m[c]["waves"], [m[c][p + "_cycles"]["median"] for p in PHASES], m[c]["end_us"]["median"],
                m[c]["end_us"]["p90"]), flush=True)


if __name__ == "__main__":
    main()
