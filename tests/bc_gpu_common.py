"""What tests/test_gpu_bc.py and tests/test_gpu_bc_discrete.py share: the helpers around one fused
behaviour-cloning call (BCUpdate over rr_bc_update or rr_bc_update_discrete), parameterised by the float64
reference module (bc_ref or bc_discrete_ref), the policy's tensor names and the C call's name. The bars are
the learner's own (tests/test_gpu_ppo_edges.py): per tensor max |fused - fp64| <= 1e-4 max |fp64| + 1e-7;
statistics 1e-5 relative + 1e-6."""
import copy

import numpy as np


class BcHelpers:
    def __init__(self, ref, names, vf_names, call, sweep_inputs):
        """ref: the reference module (reference, STATS, N_ROWS); names / vf_names: the policy's tensors in the
        call's order and its value half; call: the C entry point BCUpdate must pick; sweep_inputs: the
        zero-argument source of (policy, obs, acts) for `epoch`."""
        self.R, self.names, self.vf_names, self.call, self.sweep_inputs = ref, names, vf_names, call, sweep_inputs

    def minibatch(self, bs, extra=0, n=None):
        import torch

        g = torch.Generator().manual_seed(bs)
        return torch.randperm(self.R.N_ROWS if n is None else n, generator=g)[:bs + extra].contiguous().cuda()

    @staticmethod
    def adam(pol, lr=1e-3, **kw):
        import torch

        return torch.optim.Adam(pol.parameters(), lr=lr, capturable=True, **kw)

    def one_call(self, pol0, obs, acts, idx, ent_weight=1e-3, l2_weight=0.0):
        """A copy of pol0 after one fused call on idx: (policy, its gradients fp32, the 8 stats)."""
        import torch
        from rl_rocket_amd.bc import BCUpdate, Demonstrations
        from rl_rocket_amd.rollout import _policy_tensors

        pol = copy.deepcopy(pol0)
        step = BCUpdate(pol, self.adam(pol), Demonstrations(obs, acts), idx.numel(), ent_weight, l2_weight)
        assert step._call == self.call and len(step.params) == len(self.names)
        stats = step(idx).clone()
        torch.cuda.synchronize()
        return pol, [t.grad.clone() for t in _policy_tensors(pol)], stats

    def check_against_fp64(self, label, pol0, obs, acts, idx, grads, stats, ent_weight=1e-3, l2_weight=0.0):
        """The learner's bars on the gradients a call left and its statistics; pol0 holds the parameters
        the call started from. Returns the float64 figures."""
        import torch
        from rl_rocket_amd.rollout import _policy_tensors

        kw = dict(ent_weight=ent_weight, l2_weight=l2_weight)
        ref64, st64 = self.R.reference(pol0, obs, acts, idx, torch.float64, **kw)
        ref32, st32 = self.R.reference(pol0, obs, acts, idx, torch.float32, **kw)
        assert len(grads) == len(ref64) == len(self.names)
        for name, a, r, t, w in zip(self.names, grads, ref64, ref32, _policy_tensors(pol0)):
            a = a.double()
            scale = r.abs().max().item()
            err, err32 = (a - r).abs().max().item(), (t - r).abs().max().item()
            print("%s %-9s max|ref| %.3e  fused err %.2e  torch-fp32 err %.2e" % (label, name, scale, err, err32))
            assert a.shape == w.shape and bool(torch.isfinite(a).all()), name
            assert err <= 1e-4 * scale + 1e-7, (name, err, scale, err32)
            if name in self.vf_names:
                if l2_weight == 0.0:
                    assert torch.count_nonzero(a).item() == 0, name
                else:  # l2_weight (as the fp32 argument it is) times w, within one fp32 rounding
                    want = float(np.float32(l2_weight)) * w.detach().double()
                    assert bool(((a - want).abs() <= 2.0 ** -24 * want.abs()).all()), name
        st = stats.tolist()
        assert all(v == v and abs(v) != float("inf") for v in st), st
        assert st[7] == 0.0
        for name, a, r, t in zip(self.R.STATS, st, st64, st32):
            print("%s %-13s fp64 %.9e  fused err %.2e  torch-fp32 err %.2e" % (label, name, r, abs(a - r), abs(t - r)))
            assert abs(a - r) <= 1e-5 * abs(r) + 1e-6, (name, a, r)
        return st64

    @staticmethod
    def state(pol, opt):
        import torch
        from rl_rocket_amd.rollout import _policy_tensors

        torch.cuda.synchronize()
        out = []
        for t in _policy_tensors(pol):
            out += [t.detach().clone(), t.grad.clone(), opt.state[t]["exp_avg"].clone(),
                    opt.state[t]["exp_avg_sq"].clone(), opt.state[t]["step"].clone()]
        return out

    def epoch(self, mode, sizes=(4097, 4097, 130)):
        """One epoch of minibatches (the last shorter: 33, 33 and 2 workgroups) on a copy of the sweep
        policy: 'packed' every call packs for itself, 'chained' all but the first are chained, 'graph'
        the chained epoch captured once and replayed once."""
        import torch
        from rl_rocket_amd.bc import BCUpdate, Demonstrations
        from rl_rocket_amd.rollout import _policy_tensors

        pol0, obs, acts = self.sweep_inputs()
        pol = copy.deepcopy(pol0)
        opt = self.adam(pol)
        step = BCUpdate(pol, opt, Demonstrations(obs, acts), max(sizes), ent_weight=0.01, l2_weight=1e-3)
        perm = torch.randperm(self.R.N_ROWS, generator=torch.Generator().manual_seed(31)).cuda()
        cuts = np.cumsum((0,) + tuple(sizes))
        mbs = [perm[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        stats = []

        def run():
            for k, idx in enumerate(mbs):
                stats.append(step(idx, chained=mode != "packed" and k > 0).clone())

        if mode == "graph":
            start = self.state(pol, opt)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                run()  # warm-up outside the capture, then back to the start
            torch.cuda.current_stream().wait_stream(side)
            with torch.no_grad():
                it = iter(start)
                for t in _policy_tensors(pol):
                    for dst in (t, t.grad, opt.state[t]["exp_avg"], opt.state[t]["exp_avg_sq"], opt.state[t]["step"]):
                        dst.copy_(next(it))
            del stats[:]
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run()
            with torch.no_grad():  # the capture ran nothing: still the start
                for a, b in zip(self.state(pol, opt), start):
                    assert torch.equal(a, b)
            graph.replay()
        else:
            run()
        return self.state(pol, opt), [s.clone() for s in stats]
