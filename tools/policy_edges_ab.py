"""A/B of two builds of the library on the policy kernels' outputs: the check of a kernel change
that must keep every bit inside a stated input domain.

    RR_LIB_PATH=tools/ab/lib_parent.so python tools/policy_edges_ab.py dump ab_out/parent.npz
    RR_LIB_PATH=tools/ab/lib_new.so    python tools/policy_edges_ab.py dump ab_out/new.npz
    python tools/policy_edges_ab.py compare ab_out/parent.npz ab_out/new.npz

`dump` runs rr_policy_act (value, action, clipped action, log_prob) and rr_policy_bootstrap
(value_out, reward_out) on the in-range inputs of tests/test_gpu_policy_edges.py (2 sizes x 3
precisions x 4 weight sets x 7 obs classes of 257 rows, |obs| <= 255.875: tests/policy_bound.py) with
the library RR_LIB_PATH names (one library per process) and stores the raw bits. `compare` lists the
arrays whose bits differ; exit status 1 if any does."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dump(path):
    import torch
    import policy_bound as B
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr
    from rl_rocket_amd.rollout import POLICY_PRECISIONS, PolicyPack

    lib, dev, n = _lib.load(), torch.device("cuda:0"), B.N_ROWS
    out = {}
    trunc = (torch.arange(n, device=dev) % 3 == 0).to(torch.uint8)
    rew = torch.linspace(-3, 3, n, device=dev)
    it = torch.tensor([5], dtype=torch.int64, device=dev)
    for ns, na in B.SIZES:
        for ws in B.WEIGHT_SETS:
            pol = B.weight_set(ws, ns, na).to(dev)
            for prec, pc in POLICY_PRECISIONS.items():
                params = PolicyPack(pol, ns, na, dev, precision=prec).pack()
                for oc in B.OBS_CLASSES:
                    obs = torch.from_numpy(B.obs_class(oc, ns)).to(dev)
                    assert float(obs.abs().max()) <= B.F16_OBS_MAX
                    act_env, act = torch.zeros((n, na), device=dev), torch.zeros((n, na), device=dev)
                    val, lp, vout, rout = (torch.zeros((n,), device=dev) for _ in range(4))
                    _lib.check(lib.rr_policy_act(_ptr(params), ns, na, pc, n, 0, _ptr(obs), 123, _ptr(it), 3, _ptr(act_env),
                                                 _ptr(act), _ptr(val), _ptr(lp), None, None, None, None, 0.99, None, None,
                                                 None, None), "rr_policy_act")
                    _lib.check(lib.rr_policy_bootstrap(_ptr(params), ns, na, pc, n, _ptr(obs), _ptr(trunc), _ptr(rew), 0.99,
                                                       _ptr(rout), _ptr(obs), _ptr(vout), None), "rr_policy_bootstrap")
                    torch.cuda.synchronize()
                    for name, t in (("act_env", act_env), ("act", act), ("value", val), ("logp", lp), ("value_out", vout),
                                    ("reward_out", rout)):
                        out["%d/%s/%s/%s/%s" % (ns, ws, prec, oc, name)] = t.cpu().numpy().view(np.int32)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print("%s: %d arrays from %s" % (path, len(out), os.environ.get("RR_LIB_PATH", "the in-tree library")))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files)
    diff = [k for k in a.files if not np.array_equal(a[k], b[k])]
    print("%d arrays, %d differ" % (len(a.files), len(diff)))
    for k in diff:
        print("  %s: %d of %d elements" % (k, int((a[k] != b[k]).sum()), a[k].size))
    return 1 if diff else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
