"""On-device PPO rollouts: policy inference, env step and rollout buffer all in HBM.

SURVEY.md §8(f) rank 2 / BASELINE.json configs[4]: stock SB3 1.6 copies every observation
batch to a NumPy ``RolloutBuffer`` on the host; here the PyTorch policy consumes the obs
tensor the step kernel wrote, the sampled actions go straight back into ``rr_step``, and
the buffer, GAE and the PPO update stay on the GPU. One ``collect`` (n_steps × [policy
forward + sample + env step + buffer writes]) can be captured into a hipGraph.

``MlpActorCritic`` mirrors SB3 1.6 ``ActorCriticPolicy`` defaults for PPO with
``"MlpPolicy"`` (the reference's ``sb3_config["policy_type"]``, configuration_file.py:41):
separate pi / vf MLPs [64, 64] with tanh, diagonal Gaussian with state-independent
log_std (init 0), orthogonal init (gain sqrt(2) hidden, 0.01 policy head, 1 value head);
actions are clipped to the Box [-1, 1] before the env step, as SB3 does.
Timeouts are bootstrapped like SB3 1.6 ``collect_rollouts``:
reward += gamma * V(terminal_obs) where TimeLimit truncated the episode.
"""
import math

import torch
from torch import nn


class _LinearFn(torch.autograd.Function):
    """``F.linear`` whose bias gradient is a GEMM with a row of ones instead of a column sum.

    On PyTorch 2.10 / ROCm 7 a hipGraph that runs a GEMM and then a column sum (``sum(0)``) of a
    tensor produced in the same graph returns a wrong sum from its second replay on (the first
    replay and eager runs are right; the round-3 probe (profiles/r03/r03i/probe_graph_reduce.txt): errors of 10^2 on sums of
    ~10^3 at 8 192 and 65 536 rows, the GEMM output itself correct, the same sum as
    ``ones @ g`` correct). A Linear's bias gradient is exactly that column sum of the output
    gradient, so GraphedPPOUpdate's replays trained with wrong hidden-layer bias gradients."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = g @ w
        if ctx.needs_input_grad[1]:
            gw = g2.t() @ x.reshape(-1, x.shape[-1])
        if ctx.needs_input_grad[2]:
            gb = (g2.new_ones(1, g2.shape[0]) @ g2)[0]
        return gx, gw, gb


class _Linear(nn.Linear):
    """nn.Linear (same parameters, initialisation and packing) through _LinearFn."""

    def forward(self, x):
        return _LinearFn.apply(x, self.weight, self.bias)


class MlpActorCritic(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden=(64, 64), log_std_init=0.0):
        super().__init__()
        self.hidden = tuple(hidden)

        def mlp():
            layers, d = [], obs_dim
            for h in hidden:
                layers += [_Linear(d, h), nn.Tanh()]
                d = h
            return nn.Sequential(*layers)

        self.pi_net, self.vf_net = mlp(), mlp()
        self.action_net = _Linear(hidden[-1], act_dim)
        self.value_net = _Linear(hidden[-1], 1)
        self.log_std = nn.Parameter(torch.full((act_dim,), float(log_std_init)))
        for net in (self.pi_net, self.vf_net):
            for m in net:
                if isinstance(m, nn.Linear):
                    nn.init.orthogonal_(m.weight, gain=math.sqrt(2))
                    nn.init.zeros_(m.bias)
        nn.init.orthogonal_(self.action_net.weight, gain=0.01)
        nn.init.zeros_(self.action_net.bias)
        nn.init.orthogonal_(self.value_net.weight, gain=1.0)
        nn.init.zeros_(self.value_net.bias)

    def forward(self, obs):
        return self.action_net(self.pi_net(obs)), self.value_net(self.vf_net(obs)).squeeze(-1)

    def value(self, obs):
        return self.value_net(self.vf_net(obs)).squeeze(-1)

    def log_prob(self, mean, actions):
        std = self.log_std.exp()
        return (-((actions - mean) ** 2) / (2 * std * std) - self.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)

    def entropy(self, n):
        return (0.5 + 0.5 * math.log(2 * math.pi) + self.log_std).sum().expand(n)


POLICY_PRECISIONS = {"fp32": 0, "bf16": 1, "fp16x3": 2}  # RR_POLICY_FP32 / RR_POLICY_BF16 / RR_POLICY_FP16X3


# folded fp32 tanh of the rollout pack (rocket_policy.inc kPolFoldTanh): c = 2 log2 e
FOLD_C = 2.88539008177792681


def _rowsum(w):
    """Row sums of a [rows][cols] weight in fp64, column by column (the pack kernel's order)."""
    w = w.double()
    acc = torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
    for q in range(w.shape[1]):
        acc = acc + w[:, q]
    return acc


class PolicyPack:
    """Packs an ``MlpActorCritic``'s weights into the fragment-ordered buffer of the fused
    HIP policy kernel (layout: rl_rocket_amd/csrc/rocket_policy.inc, offsets from
    ``rr_policy_layout``). ``pack()`` is pure device tensor work on the live parameters,
    so it can sit inside a captured graph and always reflects the current weights.
    ``precision`` "fp32" (default, SB3-exact to fp32 rounding), "bf16" (tower weights
    as bf16 MFMA fragments, opt-in) or "fp16x3" (tower weights 2^8 W split into fp16
    hi / lo planes, biases 2^16 b: the split-fp16 MFMA path, fp32-level accuracy)."""

    def __init__(self, policy, obs_dim, act_dim, device, precision="fp32"):
        import ctypes

        from . import _lib

        if precision not in POLICY_PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(POLICY_PRECISIONS))
        self.precision, self.prec = precision, POLICY_PRECISIONS[precision]
        lib = _lib.load()
        off = (ctypes.c_int64 * 12)()
        size = _lib.check(lib.rr_policy_layout(obs_dim, act_dim, self.prec, off), "rr_policy_layout")
        self.off = dict(zip(("L1A", "B1", "L2A", "B2", "TOWER", "PI", "VF", "HA", "HV", "HB", "VB", "LS"), list(off)))
        self.size, self.obs_dim, self.act_dim, self.policy = size, obs_dim, act_dim, policy
        self.buf = torch.zeros(size + 4, dtype=torch.float32, device=device)  # +4: 16-B alignment slack
        if self.buf.data_ptr() % 16:
            raise RuntimeError("packed policy buffer not 16-B aligned")
        dev = device
        lane = torch.arange(64, device=dev)
        r, hh = lane & 31, lane >> 5
        reg = torch.arange(16, device=dev)

        def row(rg, h):  # D-layout row of register rg in lane half h
            return (rg & 3) + 8 * (rg >> 2) + 4 * h

        half = torch.arange(2, device=dev)
        m = torch.arange(2, device=dev)
        # B[m][half][reg] = b[32m + row(reg, half)]
        self.b_i = (32 * m[:, None, None] + row(reg[None, None, :], half[None, :, None])).reshape(-1)
        if self.prec:
            # bf16: L1A[m][s][lane][j] = W1[32m + r][16s + 8hh + j];
            # L2A[m][t][s][lane][j] = W2[32m + r][32t + 16s + 8(j>>2) + 4hh + (j&3)]
            kp1 = (obs_dim + 15) // 16
            s_ = torch.arange(kp1, device=dev)
            j = torch.arange(8, device=dev)
            shp1 = (2, kp1, 64, 8)
            self.l1_i = (32 * m.view(2, 1, 1, 1) + r.view(1, 1, 64, 1)).expand(shp1).reshape(-1)
            self.l1_k = (16 * s_.view(1, kp1, 1, 1) + 8 * hh.view(1, 1, 64, 1) + j.view(1, 1, 1, 8)).expand(shp1).reshape(-1)
            t = torch.arange(2, device=dev)
            shp2 = (2, 2, 2, 64, 8)
            self.l2_i = (32 * m.view(2, 1, 1, 1, 1) + r.view(1, 1, 1, 64, 1)).expand(shp2).reshape(-1)
            self.l2_k = (32 * t.view(1, 2, 1, 1, 1) + 16 * torch.arange(2, device=dev).view(1, 1, 2, 1, 1)
                         + 8 * (j.view(1, 1, 1, 1, 8) >> 2) + 4 * hh.view(1, 1, 1, 64, 1)
                         + (j.view(1, 1, 1, 1, 8) & 3)).expand(shp2).reshape(-1)
            self.kp1 = kp1
            return
        kp1 = (obs_dim + 1) // 2
        self.kp1 = kp1
        s_ = torch.arange(kp1, device=dev)
        # L1A[m][s][lane] = W1[32m + r][2s + hh]  (k >= obs_dim -> padded column)
        k1 = 2 * s_[None, :, None] + hh[None, None, :]
        self.l1_i = (32 * m[:, None, None] + r[None, None, :]).expand(2, kp1, 64).reshape(-1)
        self.l1_k = k1.expand(2, kp1, 64).reshape(-1)
        # L2A[m][t][g][lane][rr] = W2[32m + r][32t + row(4g + rr, hh)]
        t = torch.arange(2, device=dev)
        g = torch.arange(4, device=dev)
        rr = torch.arange(4, device=dev)
        shp = (2, 2, 4, 64, 4)
        self.l2_i = (32 * m.view(2, 1, 1, 1, 1) + r.view(1, 1, 1, 64, 1)).expand(shp).reshape(-1)
        self.l2_k = (32 * t.view(1, 2, 1, 1, 1) + row(4 * g.view(1, 1, 4, 1, 1) + rr.view(1, 1, 1, 1, 4),
                                                        hh.view(1, 1, 1, 64, 1))).expand(shp).reshape(-1)

    def _tower(self, net, base):
        o = self.off
        w1, b1, w2, b2 = net[0].weight, net[0].bias, net[2].weight, net[2].bias
        kpad = (16 if self.prec else 2) * self.kp1 - self.obs_dim
        w1p = torch.nn.functional.pad(w1, (0, kpad))  # zero columns past obs_dim
        l1, l2 = w1p[self.l1_i, self.l1_k], w2[self.l2_i, self.l2_k]
        bscale = 1.0
        if self.prec == 1:  # RNE to bf16; two bf16 per packed float, element 2q in the low half
            l1 = l1.to(torch.bfloat16).view(torch.float32)
            l2 = l2.to(torch.bfloat16).view(torch.float32)
        elif self.prec == 2:  # [hi, lo] fp16 planes of 2^8 W (RNE); biases at the 2^16 accumulator scale

            def split(w):
                w = w * 256.0
                hi = w.to(torch.float16)
                lo = (w - hi.float()).to(torch.float16)
                return torch.cat([hi.view(torch.float32), lo.view(torch.float32)])

            l1, l2, bscale = split(l1), split(l2), 65536.0
        if self.prec == 0:  # the folded fp32 tanh (rocket_policy.inc kPolFoldTanh), fp64 then one rounding
            c = FOLD_C
            self.buf[base + o["L1A"]: base + o["L1A"] + l1.numel()] = (c * l1.double()).float()
            self.buf[base + o["B1"]: base + o["B1"] + 64] = (c * b1.double()).float()[self.b_i]
            self.buf[base + o["L2A"]: base + o["L2A"] + l2.numel()] = (-2.0 * c * l2.double()).float()
            self.buf[base + o["B2"]: base + o["B2"] + 64] = (c * (b2.double() + _rowsum(w2))).float()[self.b_i]
            return
        self.buf[base + o["L1A"]: base + o["L1A"] + l1.numel()] = l1
        self.buf[base + o["B1"]: base + o["B1"] + 64] = b1[self.b_i] * bscale
        self.buf[base + o["L2A"]: base + o["L2A"] + l2.numel()] = l2
        self.buf[base + o["B2"]: base + o["B2"] + 64] = b2[self.b_i] * bscale

    def _sources(self):
        p = self.policy
        ts = [p.pi_net[0].weight, p.pi_net[0].bias, p.pi_net[2].weight, p.pi_net[2].bias,
              p.vf_net[0].weight, p.vf_net[0].bias, p.vf_net[2].weight, p.vf_net[2].bias,
              p.action_net.weight, p.action_net.bias, p.value_net.weight, p.value_net.bias, p.log_std]
        for t in ts:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.buf.device:
                raise ValueError("rr_policy_pack needs contiguous fp32 parameters on the rollout device")
        return ts

    @torch.no_grad()
    def pack(self):
        """One HIP launch (rr_policy_pack) from the live parameter tensors."""
        import ctypes

        from . import _lib

        ts = self._sources()
        src = (ctypes.c_void_p * 13)(*[t.data_ptr() for t in ts])
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.buf.device).cuda_stream)
        _lib.check(_lib.load().rr_policy_pack(self.obs_dim, self.act_dim, self.prec, src,
                                              ctypes.c_void_p(self.buf.data_ptr()), stream), "rr_policy_pack")
        return self.buf

    @torch.no_grad()
    def pack_reference(self):
        """The same layout with PyTorch index ops (test reference for rr_policy_pack)."""
        p, o, na = self.policy, self.off, self.act_dim
        self._tower(p.pi_net, o["PI"])
        self._tower(p.vf_net, o["VF"])
        wa, wv = p.action_net.weight, p.value_net.weight
        if self.prec == 0:  # folded: the heads read r2 with tanh = 1 - 2 r2
            self.buf[o["HA"]: o["HA"] + 64 * na] = (-2.0 * wa[:, self.b_i]).reshape(-1)
            self.buf[o["HV"]: o["HV"] + 64] = -2.0 * wv[0, self.b_i]
            self.buf[o["HB"]: o["HB"] + na] = (p.action_net.bias.double() + _rowsum(wa)).float()
            self.buf[o["VB"]: o["VB"] + 1] = (p.value_net.bias.double() + _rowsum(wv)).float()
        else:
            self.buf[o["HA"]: o["HA"] + 64 * na] = wa[:, self.b_i].reshape(-1)
            self.buf[o["HV"]: o["HV"] + 64] = wv[0, self.b_i]
            self.buf[o["HB"]: o["HB"] + na] = p.action_net.bias
            self.buf[o["VB"]: o["VB"] + 1] = p.value_net.bias
        self.buf[o["LS"]: o["LS"] + na] = p.log_std
        return self.buf


class DeviceRollout:
    """Collects ``n_steps`` transitions from a ``RocketBatch`` (auto-reset, TimeLimit)
    into device tensors [n_steps, N, ...] and computes GAE on device.

    ``fused=True`` (default for an ``MlpActorCritic`` with 64x64 towers): per step one
    fp32-MFMA HIP launch for policy forward + sampling + buffer writes (``rr_policy_act``),
    the fused env step, one launch for the timeout bootstrap (``rr_policy_bootstrap``);
    GAE in one launch (``rr_gae``). ``fused=False``: the same algorithm in PyTorch ops.
    ``one_launch=True`` (default where possible: fused, RK4 / Euler env) collapses the whole
    ``collect`` to ONE launch (``rr_rollout_collect``: every env runs policy, sample, env step,
    bootstrap and buffer writes for all ``n_steps`` with its state in registers, then V(last
    obs) and its GAE scan); ``per_step=True`` keeps one launch per step (``rr_rollout_step``)
    + bootstrap + GAE launches. All three paths produce bitwise the same rollout.
    ``policy_dtype="fp16x3"`` (fused only) runs the towers on fp16 MFMA with every operand
    split into fp16 hi + lo halves and three MFMAs per k step: fp32-level results (values
    within ~3e-6 of the PyTorch fp32 policy at obs of O(1), as the fp32 path; ~1e-5 at the envs'
    largest obs of +-90; obs components past +-255.875, the fp16 operand range, are read as
    +-255.875: INTEGRATION.md) at 1.44x the collection rate.
    ``policy_dtype="bf16"`` (fused only, opt-in) runs the towers on bf16 MFMA with fp32
    accumulation: actions / values / log-probs then differ from the fp32 policy by the bf16
    rounding of obs, weights and the first hidden layer (the stored log-probs are those of
    the bf16 mean; PPO's first-epoch ratio starts within ~1e-3 of 1 instead of at 1).
    ``stats=True`` (one-launch path only, a batch with ``episode_stats=True`` and auto-reset) makes
    ``collect`` account for every episode the rollout finishes and for the samples' explained
    variance in the same launch (``rr_rollout_collect_stats``; the rollout itself is bitwise
    unchanged): ``ro.stats.last()`` / ``ro.stats.window()`` return SB3's ``rollout/*`` figures and
    ``train/explained_variance`` (``rollout_stats.RolloutStats``)."""

    def __init__(self, batch, policy, n_steps=16, gamma=0.99, gae_lambda=0.95, generator=None, fused=None,
                 seed=0, policy_dtype="fp32", one_launch=None, per_step=False, stats=False):
        self.env, self.policy = batch, policy
        self.n_steps, self.gamma, self.lam = n_steps, gamma, gae_lambda
        n, ns, na = batch.num_envs, batch.state_dim, batch.action_dim
        dev = batch.device
        f = dict(device=dev, dtype=torch.float32)
        self.obs = torch.zeros((n_steps, n, ns), **f)
        self.actions = torch.zeros((n_steps, n, na), **f)
        self.rewards = torch.zeros((n_steps, n), **f)
        self.starts = torch.zeros((n_steps, n), **f)   # SB3 episode_starts
        self.values = torch.zeros((n_steps, n), **f)
        self.log_probs = torch.zeros((n_steps, n), **f)
        self.advantages = torch.zeros((n_steps, n), **f)
        self.returns = torch.zeros((n_steps, n), **f)
        self.last_obs = batch.reset().clone()
        self.last_start = torch.ones((n,), **f)
        self.last_value = torch.zeros((n,), **f)
        self.last_done = torch.zeros((n,), **f)
        self.gen = generator
        self._clipped = torch.zeros((n, na), **f)
        self._tobs = torch.zeros((n, ns), **f)
        self._r = torch.zeros((n,), **f)
        if fused is None:
            fused = isinstance(policy, MlpActorCritic) and policy.hidden == (64, 64) and (ns, na) in ((14, 3), (7, 2))
        self.fused = bool(fused)
        if policy_dtype not in POLICY_PRECISIONS:
            raise ValueError("policy_dtype must be one of %s" % sorted(POLICY_PRECISIONS))
        if policy_dtype != "fp32" and not self.fused:
            raise ValueError("policy_dtype=%r needs the fused HIP policy path" % policy_dtype)
        self.policy_dtype = policy_dtype
        dopri = self.fused and int(batch.params.integrator) == 2  # RR_INT_DOPRI5: two-launch path
        if one_launch is None:
            one_launch = self.fused and not dopri
        if one_launch and (not self.fused or dopri):
            raise ValueError("one_launch needs the fused policy and an RK4 / Euler env")
        self.one_launch = bool(one_launch)
        self.per_step = bool(per_step) or not self.one_launch  # one_launch + not per_step: rr_rollout_collect
        self.stats = None
        if stats:
            from . import _lib

            if not self.one_launch or self.per_step:
                raise ValueError("stats=True needs the one-launch collect (fused policy, RK4 / Euler env, not per_step)")
            flags = int(batch.params.flags)
            if not flags & _lib.RR_FLAG_EPISODE_STATS or not flags & _lib.RR_FLAG_AUTO_RESET:
                raise ValueError("stats=True needs a batch created with episode_stats=True and auto_reset=True")
        if self.fused:
            from . import _lib

            self._lib = _lib.load()
            self._pack = PolicyPack(policy, ns, na, dev, precision=policy_dtype)
            self.iter = torch.zeros((1,), dtype=torch.int64, device=dev)  # advanced by every collect (graph-safe)
            self.seed = int(seed) & (2 ** 64 - 1)
            self._ones = torch.ones((n,), dtype=torch.uint8, device=dev)
            self._zeros = torch.zeros((n,), **f)
            import ctypes

            from .batch import _ptr

            self._c, self._p = ctypes, _ptr
            bufs = _lib.RrBuffers()
            _lib.check(self._lib.rr_get_buffers(batch._h, ctypes.byref(bufs)), "rr_get_buffers")
            self._term_obs = ctypes.c_void_p(bufs.terminal_obs)
            batch.done.fill_(1)  # SB3: _last_episode_starts = ones before the first rollout
            if stats:
                from .rollout_stats import RolloutStats

                self.stats = RolloutStats(n, dev, self._lib)

    @torch.no_grad()
    def collect(self):
        if self.fused:
            return self._collect_fused()
        env, pol = self.env, self.policy
        for t in range(self.n_steps):
            obs = self.last_obs
            mean, value = pol(obs)
            noise = torch.randn(mean.shape, device=mean.device, generator=self.gen)
            act = mean + pol.log_std.exp() * noise
            self.obs[t].copy_(obs)
            self.actions[t].copy_(act)
            self.values[t].copy_(value)
            self.log_probs[t].copy_(pol.log_prob(mean, act))
            self.starts[t].copy_(self.last_start)
            torch.clamp(act, -1.0, 1.0, out=self._clipped)
            nobs, rew, done, trunc = env.step(self._clipped)
            # SB3 1.6: bootstrap timeouts with the value of the terminal observation
            env.copy_terminal(out=(self._tobs, None, None))
            # a select, as the fused kernels: terminal rows of envs that are not done are stale
            # (possibly non-finite), and NaN * 0 would leak into the reward
            torch.where(trunc.bool(), torch.addcmul(rew, pol.value(self._tobs), trunc.float(), value=self.gamma),
                        rew, out=self._r)
            self.rewards[t].copy_(self._r)
            self.last_obs.copy_(nobs)
            self.last_start.copy_(done.float())
        self.last_value.copy_(pol.value(self.last_obs))
        self.last_done.copy_(self.last_start)
        self._gae()

    def _collect_fused(self):
        """one_launch: the whole rollout + GAE in one rr_rollout_collect launch, or (per_step)
        one rr_rollout_step per step (the env's obs buffer is written on the last step only),
        then V(last obs). Otherwise two launches per step: rr_policy_act
        (forward + sample of step t, bootstrap of step t-1, episode-start flags) and the
        fused env step; obs are read in place from the env's output buffer."""
        env, lib, c, p = self.env, self._lib, self._c, self._p
        from . import _lib

        n, ns, na = env.num_envs, env.state_dim, env.action_dim
        params = p(self._pack.pack())
        stream = c.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        it, obs, done = p(self.iter), p(env.obs), p(env.done)
        prec = self._pack.prec
        if self.stats is not None:
            st = self.stats.struct()
            _lib.check(lib.rr_rollout_collect_stats(env._h, params, prec, self.seed, it, self.n_steps, self.gamma,
                                                    self.lam, p(self.obs), p(self.actions), p(self.values),
                                                    p(self.log_probs), p(self.starts), p(self.rewards),
                                                    p(self.advantages), p(self.returns), p(self.last_value),
                                                    p(self.last_done), p(self.last_start), obs, p(env.reward), done,
                                                    p(env.truncated), p(env.terms), c.byref(st), stream),
                       "rr_rollout_collect_stats")
            self.iter.add_(1)
            return
        if self.one_launch and not self.per_step:
            _lib.check(lib.rr_rollout_collect(env._h, params, prec, self.seed, it, self.n_steps, self.gamma, self.lam,
                                              p(self.obs), p(self.actions), p(self.values), p(self.log_probs),
                                              p(self.starts), p(self.rewards), p(self.advantages), p(self.returns),
                                              p(self.last_value), p(self.last_done), p(self.last_start), obs,
                                              p(env.reward), done, p(env.truncated), p(env.terms), stream),
                       "rr_rollout_collect")
            self.iter.add_(1)
            return
        if self.one_launch:
            T = self.n_steps
            for t in range(T):
                _lib.check(lib.rr_rollout_step(env._h, params, prec, self.seed, it, t, self.gamma, p(self.obs[t]),
                                               p(self.actions[t]), p(self.values[t]), p(self.log_probs[t]),
                                               p(self.starts[t]), p(self.rewards[t]), obs if t == T - 1 else None,
                                               p(env.reward), done, p(env.truncated), p(env.terms), stream),
                           "rr_rollout_step")
            _lib.check(lib.rr_policy_bootstrap(params, ns, na, prec, n, None, None, None, self.gamma, None, obs,
                                               p(self.last_value), stream), "rr_policy_bootstrap")
            self._finish(stream)
            return
        for t in range(self.n_steps):
            prev = t > 0
            _lib.check(lib.rr_policy_act(params, ns, na, prec, n, env.env_id_offset, obs, self.seed, it, t, p(self._clipped),
                                         p(self.actions[t]), p(self.values[t]), p(self.log_probs[t]), p(self.obs[t]),
                                         self._term_obs if prev else None, p(env.truncated) if prev else None,
                                         p(env.reward) if prev else None, self.gamma,
                                         p(self.rewards[t - 1]) if prev else None, done, p(self.starts[t]), stream),
                       "rr_policy_act")
            env.step(self._clipped)
        _lib.check(lib.rr_policy_bootstrap(params, ns, na, prec, n, self._term_obs, p(env.truncated), p(env.reward),
                                           self.gamma, p(self.rewards[self.n_steps - 1]), obs, p(self.last_value),
                                           stream), "rr_policy_bootstrap")
        self._finish(stream)

    def _finish(self, stream):
        """last_done / last_start from the env's done flags, GAE (rr_gae), advance the
        noise counter."""
        from . import _lib

        env, lib, p = self.env, self._lib, self._p
        n = env.num_envs
        self.last_done.copy_(env.done)
        self.last_start.copy_(env.done)
        _lib.check(lib.rr_gae(self.n_steps, n, p(self.rewards), p(self.values), p(self.starts), p(self.last_value),
                              p(self.last_done), self.gamma, self.lam, p(self.advantages), p(self.returns), stream),
                   "rr_gae")
        self.iter.add_(1)

    def _gae(self):
        """SB3 RolloutBuffer.compute_returns_and_advantage, on device. The scan runs in float64
        and each stored value is rounded once, as rr_gae's (an fp32 scan is ~5e-5 off at |A| ~ 150)."""
        rewards, values, starts = self.rewards.double(), self.values.double(), self.starts.double()
        last_gae = torch.zeros_like(self.last_value, dtype=torch.float64)
        for t in reversed(range(self.n_steps)):
            if t == self.n_steps - 1:
                nonterminal = 1.0 - self.last_done.double()
                next_values = self.last_value.double()
            else:
                nonterminal = 1.0 - starts[t + 1]
                next_values = values[t + 1]
            delta = rewards[t] + self.gamma * next_values * nonterminal - values[t]
            last_gae = delta + self.gamma * self.lam * nonterminal * last_gae
            self.advantages[t].copy_(last_gae)
            self.returns[t].copy_(last_gae + values[t])


def _allreduce_grads(params, group):
    """Average the gradients of `params` over the ranks of `group` with ONE all_reduce of a
    flat buffer (the 64x64 MlpPolicy is ~10.6 k parameters: a single 42 KB message per
    minibatch, RCCL over xGMI with the "nccl" backend)."""
    import torch.distributed as dist

    grads = [p.grad for p in params if p.grad is not None]
    flat = torch.cat([g.reshape(-1) for g in grads])
    if flat.is_cuda and dist.get_backend(group) == "gloo":  # CPU rehearsal of the N > 1 path
        host = flat.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        flat.copy_(host)
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat /= dist.get_world_size(group)
    k = 0
    for g in grads:
        g.copy_(flat[k:k + g.numel()].view_as(g))
        k += g.numel()


def _policy_tensors(policy):
    """The 13 parameter tensors in rr_policy_pack / rr_ppo_grad order."""
    p = policy
    return [p.pi_net[0].weight, p.pi_net[0].bias, p.pi_net[2].weight, p.pi_net[2].bias,
            p.vf_net[0].weight, p.vf_net[0].bias, p.vf_net[2].weight, p.vf_net[2].bias,
            p.action_net.weight, p.action_net.bias, p.value_net.weight, p.value_net.bias, p.log_std]


def fused_grad_supported(policy, obs_dim, act_dim):
    return (isinstance(policy, MlpActorCritic) and policy.hidden == (64, 64)
            and (obs_dim, act_dim) in ((14, 3), (7, 2)))


class PPOGrad:
    """The PPO minibatch loss + backward as ONE HIP pipeline (``rr_ppo_grad``: fp32 MFMA forward
    and backward of both towers over the gathered minibatch, fixed-order workgroup sums).

    ``__call__(idx)`` WRITES ``p.grad`` of the policy's 13 parameters (allocated here once and
    kept: the library holds their addresses, so do not set them to None — use
    ``zero_grad(set_to_none=False)`` or none at all, the call overwrites) for the minibatch
    ``idx`` (int64 device tensor of 2 .. ``batch_size`` rows of the flattened rollout) and fills
    ``stats`` = [policy_loss, value_loss, entropy, clip_fraction, approx_kl]. Same loss as
    ``ppo_update`` (SB3 1.6 PPO.train); gradients equal autograd's to fp32 rounding
    (``tests/test_gpu_ppo.py``). Stream-ordered on the current stream; graph-capturable."""

    def __init__(self, policy, ro, batch_size, clip_range=0.2, ent_coef=0.01, vf_coef=0.5):
        import ctypes

        from . import _lib

        n = ro.n_steps * ro.env.num_envs
        ns, na = ro.env.state_dim, ro.env.action_dim
        if not fused_grad_supported(policy, ns, na):
            raise ValueError("PPOGrad needs an MlpActorCritic with 64x64 towers and (obs, act) in ((14, 3), (7, 2))")
        if not 2 <= batch_size <= n:
            raise ValueError("batch_size must be in [2, n_steps * num_envs]")
        self._lib, self._c = _lib.load(), ctypes
        self.ns, self.na, self.bs = ns, na, int(batch_size)
        self.coef = (float(clip_range), float(ent_coef), float(vf_coef))
        dev = ro.obs.device
        self.data = [ro.obs.reshape(n, ns), ro.actions.reshape(n, na), ro.log_probs.reshape(n),
                     ro.advantages.reshape(n), ro.returns.reshape(n)]
        for t in self.data:
            if not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError("rollout tensors must be contiguous fp32")
        self.params = _policy_tensors(policy)
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("rr_ppo_grad needs contiguous fp32 parameters on the rollout device")
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        nbytes = ctypes.c_int64()
        _lib.check(self._lib.rr_ppo_workspace_size(ns, na, self.bs, ctypes.byref(nbytes)), "rr_ppo_workspace_size")
        self.ws = torch.empty((nbytes.value + 15) // 16 * 4, dtype=torch.float32, device=dev)
        self.stats = torch.zeros(5, dtype=torch.float32, device=dev)
        self._src = (ctypes.c_void_p * 13)(*[p.data_ptr() for p in self.params])
        self._grads = [p.grad for p in self.params]
        self._dst = (ctypes.c_void_p * 13)(*[g.data_ptr() for g in self._grads])
        self._nbytes = nbytes.value

    def __call__(self, idx):
        from . import _lib

        c = self._c
        if (idx.dtype != torch.int64 or not 2 <= idx.numel() <= self.bs or not idx.is_contiguous()
                or idx.device != self.ws.device):
            raise ValueError("idx must be a contiguous int64 device tensor of 2 .. batch_size rows")
        for p, g in zip(self.params, self._grads):
            if p.grad is not g:
                raise RuntimeError("a parameter's .grad was replaced; PPOGrad writes into the tensors it allocated")
        clip, ent, vf = self.coef
        o, a, lp, adv, ret = self.data
        stream = c.c_void_p(torch.cuda.current_stream(self.ws.device).cuda_stream)
        _lib.check(self._lib.rr_ppo_grad(self.ns, self.na, self._src, self._dst, o.data_ptr(), a.data_ptr(),
                                         lp.data_ptr(), adv.data_ptr(), ret.data_ptr(), idx.data_ptr(), idx.numel(),
                                         clip, ent, vf, self.stats.data_ptr(), self.ws.data_ptr(), self._nbytes,
                                         stream), "rr_ppo_grad")
        return self.stats


def clip_adam_supported(optimizer, params):
    if type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
        return False
    g = optimizer.param_groups[0]
    if {id(p) for p in g["params"]} != {id(p) for p in params} or len(params) > 16:
        return False
    return (g.get("capturable", False) and not g.get("amsgrad", False) and not g.get("maximize", False)
            and g.get("weight_decay", 0) == 0 and not torch.is_tensor(g["betas"][0])
            and all(p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda for p in params))


class ClipAdam:
    """``clip_grad_norm_(params, max_grad_norm)`` + ``optimizer.step()`` for a
    ``torch.optim.Adam(capturable=True)`` in two launches (``rr_clip_adam``), on the optimizer's own
    state tensors (created here, as Adam's first step would, if absent), so the optimizer object
    stays the source of truth (state_dict, later eager steps). The learning rate is read from a
    device scalar that ``__call__`` refreshes from ``param_groups[0]["lr"]`` when called eagerly;
    inside a captured graph call ``sync_lr()`` before replays (GraphedPPOUpdate.update does)."""

    def __init__(self, optimizer, params, max_grad_norm):
        import ctypes

        from . import _lib

        if not clip_adam_supported(optimizer, params):
            raise ValueError("ClipAdam needs a capturable torch.optim.Adam over exactly these fp32 CUDA parameters "
                             "(one group, no weight decay / amsgrad / maximize, <= 16 tensors)")
        self.opt, self.params = optimizer, list(params)
        self.max_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
        dev = self.params[0].device
        for p in self.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            st = optimizer.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not st["step"].is_cuda or st["step"].dtype != torch.float32:
                raise ValueError("ClipAdam needs the capturable Adam's device float32 step tensors")
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sync_lr()
        n = len(self.params)
        P = ctypes.c_void_p * n
        self._tensors = [(p, p.grad, optimizer.state[p]["exp_avg"], optimizer.state[p]["exp_avg_sq"],
                          optimizer.state[p]["step"]) for p in self.params]
        self._ptrs = [P(*[t[k].data_ptr() for t in self._tensors]) for k in range(5)]
        self._numel = (ctypes.c_int64 * n)(*[p.numel() for p in self.params])
        self._lib, self._c = _lib.load(), ctypes
        nbytes = ctypes.c_int64()
        _lib.check(self._lib.rr_clip_adam_workspace_size(sum(p.numel() for p in self.params), ctypes.byref(nbytes)),
                   "rr_clip_adam_workspace_size")
        self._ws = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)
        self._nbytes = nbytes.value

    def sync_lr(self):
        self.lr.fill_(float(self.opt.param_groups[0]["lr"]))

    def __call__(self):
        from . import _lib

        for p, g, m, v, s in self._tensors:
            st = self.opt.state[p]
            if p.grad is not g or st["exp_avg"] is not m or st["exp_avg_sq"] is not v or st["step"] is not s:
                raise RuntimeError("a gradient or Adam state tensor was replaced; ClipAdam holds their addresses")
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        grp = self.opt.param_groups[0]
        b1, b2 = grp["betas"]
        _lib.check(self._lib.rr_clip_adam(len(self.params), *self._ptrs, self._numel, self.max_norm,
                                          self.lr.data_ptr(), float(b1), float(b2), float(grp["eps"]),
                                          self._ws.data_ptr(), self._nbytes,
                                          self._c.c_void_p(torch.cuda.current_stream(self.lr.device).cuda_stream)),
                   "rr_clip_adam")


def _ppo_options(clip_range_vf, normalize_advantage, target_kl):
    """SB3's three PPO.__init__ options as (clip_range_vf or 0.0, bool, target_kl or 0.0); None
    switches the first and the last off, a number must be finite and > 0."""
    out = []
    for name, v in (("clip_range_vf", clip_range_vf), ("target_kl", target_kl)):
        if v is None:
            out.append(0.0)
            continue
        v = float(v)
        if not (0.0 < v < float("inf")):
            raise ValueError("%s must be None or a finite number > 0, not %r" % (name, v))
        out.append(v)
    return out[0], bool(normalize_advantage), out[1]


def _old_values(ro, n):
    v = getattr(ro, "values", None)
    if v is None:
        raise ValueError("clip_range_vf needs the rollout's values (ro.values)")
    v = v.reshape(n)
    if not v.is_contiguous() or v.dtype != torch.float32:
        raise ValueError("rollout tensors must be contiguous fp32")
    return v


def _train_stats(ctl):
    """SB3 PPO.train's log means from a control block read to the host (rocket_hip.h RR_PPO_CTL_*)."""
    from . import _lib as L

    n = max(ctl[L.RR_PPO_CTL_EVALS], 1.0)
    stopped = ctl[L.RR_PPO_CTL_STOP] != 0.0
    return {"train/policy_gradient_loss": ctl[L.RR_PPO_CTL_SUM_POLICY] / n,
            "train/value_loss": ctl[L.RR_PPO_CTL_SUM_VALUE] / n,
            "train/entropy_loss": -ctl[L.RR_PPO_CTL_SUM_ENTROPY] / n,
            "train/clip_fraction": ctl[L.RR_PPO_CTL_SUM_CLIP] / n,
            "train/approx_kl": ctl[L.RR_PPO_CTL_KL_SUM] / max(ctl[L.RR_PPO_CTL_KL_COUNT], 1.0),
            "train/n_minibatches": int(ctl[L.RR_PPO_CTL_STEPS]),
            "train/n_evaluated": int(ctl[L.RR_PPO_CTL_EVALS]),
            "train/early_stop": bool(stopped),
            "train/stop_epoch": int(ctl[L.RR_PPO_CTL_EPOCHS]) - 1 if stopped else None}


class PPOUpdate(PPOGrad):
    """A whole PPO minibatch step — ``PPOGrad`` then ``ClipAdam``'s clip + Adam step on the same 13
    tensors — as ONE library call (``rr_ppo_update``). Without a gradient all_reduce between the
    two halves, the clip's norm is summed by the gradient finish. The optimizer launch also repacks
    the towers for the next call and sums the next minibatch's advantage statistics. A chain of
    minibatches therefore takes three launches each instead of five; the first takes four.

    ``__call__(idx, next_idx=None, chained=False)``:
      * ``chained=True`` says that the previous call on this object was given ``next_idx=idx`` and
        that nothing else has written the parameters since.
      * The optimizer is the source of truth, as with ``ClipAdam``: its exp_avg / exp_avg_sq /
        step tensors are updated in place.
      * ``lr`` is read from a device scalar. ``sync_lr()`` refreshes it, and eager calls do so
        themselves.

    SB3's ``clip_range_vf``, ``normalize_advantage=False`` and ``target_kl`` (None / True / None:
    today's ``rr_ppo_update`` calls, unchanged), or ``train_stats=True``, take the same step through
    ``rr_ppo_update_opts``. That call carries a control block on the device (``self.ctl``):
      * ``reset()`` clears it; call it before the first minibatch of a ``train()``-like pass and pass
        ``epoch_start=True`` with every epoch's first minibatch.
      * With ``target_kl``, the minibatch whose ``approx_kl > 1.5 target_kl`` takes no optimizer
        step, and every later call is a no-op until ``reset()``. That is SB3's ``break``, without a
        host read.
      * ``train_stats()`` reads the block (one copy, which waits for the stream) and returns SB3's
        ``train/*`` means over the pass."""

    def __init__(self, policy, optimizer, ro, batch_size, clip_range=0.2, ent_coef=0.01, vf_coef=0.5,
                 max_grad_norm=0.5, clip_range_vf=None, normalize_advantage=True, target_kl=None, train_stats=False):
        import ctypes

        from . import _lib

        super().__init__(policy, ro, batch_size, clip_range, ent_coef, vf_coef)
        cvf, norm, tkl = _ppo_options(clip_range_vf, normalize_advantage, target_kl)
        self.opts = (_lib.RrPpoOptions(cvf, tkl, int(norm), int(bool(train_stats)))
                     if cvf or tkl or not norm or train_stats else None)
        if not clip_adam_supported(optimizer, list(policy.parameters())):
            raise ValueError("PPOUpdate needs a capturable torch.optim.Adam over the policy's parameters "
                             "(one group, no weight decay / amsgrad / maximize)")
        self.opt, self.max_norm = optimizer, float(max_grad_norm) if max_grad_norm is not None else 0.0
        dev = self.ws.device
        for p in self.params:
            st = optimizer.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not st["step"].is_cuda or st["step"].dtype != torch.float32:
                raise ValueError("PPOUpdate needs the capturable Adam's device float32 step tensors")
        self._state = [(optimizer.state[p]["exp_avg"], optimizer.state[p]["exp_avg_sq"], optimizer.state[p]["step"])
                       for p in self.params]
        P = ctypes.c_void_p * 13
        self._params_w = P(*[p.data_ptr() for p in self.params])
        self._m, self._v, self._s = (P(*[st[k].data_ptr() for st in self._state]) for k in range(3))
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.sync_lr()
        nbytes = ctypes.c_int64()
        size = "rr_ppo_update_workspace_size" if self.opts is None else "rr_ppo_update_opts_workspace_size"
        _lib.check(getattr(self._lib, size)(self.ns, self.na, self.bs, ctypes.byref(nbytes)), size)
        self.ws = torch.empty((nbytes.value + 15) // 16 * 4, dtype=torch.float32, device=dev)
        self._nbytes = nbytes.value
        self._next = None  # (address, rows) of the last call's next_idx: what chained=True may follow
        self.ctl = self.old_values = None
        if self.opts is not None:
            self.ctl = torch.zeros(_lib.RR_PPO_CTL_SLOTS, dtype=torch.float32, device=dev)
            if cvf:
                self.old_values = _old_values(ro, self.data[0].shape[0])

    def reset(self):
        """Clear the control block (stream-ordered, no wait): a new ``train()`` pass begins."""
        if self.ctl is None:
            raise ValueError("this PPOUpdate has no control block (no option and no train_stats)")
        self.ctl.zero_()

    def train_stats(self):
        if self.ctl is None:
            raise ValueError("train_stats() needs PPOUpdate(train_stats=True) or one of the options")
        return _train_stats(self.ctl.tolist())

    def sync_lr(self):
        self.lr.fill_(float(self.opt.param_groups[0]["lr"]))

    def __call__(self, idx, next_idx=None, chained=False, epoch_start=False):
        from . import _lib

        c = self._c
        if epoch_start and self.opts is None:
            raise ValueError("epoch_start belongs to the control block (no option and no train_stats here)")
        for t in (idx,) if next_idx is None else (idx, next_idx):
            if (t.dtype != torch.int64 or not 2 <= t.numel() <= self.bs or not t.is_contiguous()
                    or t.device != self.ws.device):
                raise ValueError("idx / next_idx must be contiguous int64 device tensors of 2 .. batch_size rows")
        if next_idx is not None and next_idx.numel() > idx.numel():
            raise ValueError("next_idx may not be longer than idx")
        if chained and self._next != (idx.data_ptr(), idx.numel()):
            raise ValueError("chained=True needs the previous call on this PPOUpdate to have had next_idx=idx")
        for p, g, (m, v, s) in zip(self.params, self._grads, self._state):
            st = self.opt.state[p]
            if p.grad is not g or st["exp_avg"] is not m or st["exp_avg_sq"] is not v or st["step"] is not s:
                raise RuntimeError("a gradient or Adam state tensor was replaced; PPOUpdate holds their addresses")
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        grp = self.opt.param_groups[0]
        b1, b2 = grp["betas"]
        clip, ent, vf = self.coef
        o, a, lp, adv, ret = self.data
        nxt = None if next_idx is None else next_idx.data_ptr()
        if self.opts is not None:
            flags = (_lib.RR_PPO_CHAINED if chained else 0) | (_lib.RR_PPO_EPOCH_START if epoch_start else 0)
            _lib.check(self._lib.rr_ppo_update_opts(
                self.ns, self.na, self._params_w, self._dst, self._m, self._v, self._s, o.data_ptr(), a.data_ptr(),
                lp.data_ptr(), adv.data_ptr(), ret.data_ptr(),
                None if self.old_values is None else self.old_values.data_ptr(), idx.data_ptr(), idx.numel(), nxt,
                0 if next_idx is None else next_idx.numel(), clip, ent, vf, self.max_norm, self.lr.data_ptr(),
                float(b1), float(b2), float(grp["eps"]), c.byref(self.opts), self.ctl.data_ptr(),
                self.stats.data_ptr(), flags, self.ws.data_ptr(), self._nbytes,
                c.c_void_p(torch.cuda.current_stream(self.ws.device).cuda_stream)), "rr_ppo_update_opts")
            self._next = None if next_idx is None else (next_idx.data_ptr(), next_idx.numel())
            return self.stats
        _lib.check(self._lib.rr_ppo_update(
            self.ns, self.na, self._params_w, self._dst, self._m, self._v, self._s, o.data_ptr(), a.data_ptr(),
            lp.data_ptr(), adv.data_ptr(), ret.data_ptr(), idx.data_ptr(), idx.numel(), nxt,
            0 if next_idx is None else next_idx.numel(), clip, ent, vf, self.max_norm, self.lr.data_ptr(), float(b1),
            float(b2), float(grp["eps"]), self.stats.data_ptr(), 1 if chained else 0, self.ws.data_ptr(),
            self._nbytes, c.c_void_p(torch.cuda.current_stream(self.ws.device).cuda_stream)), "rr_ppo_update")
        self._next = None if next_idx is None else (next_idx.data_ptr(), next_idx.numel())
        return self.stats


def _epoch_perms(n, n_epochs, dev, generator=None):
    """The epochs' permutations for the fused updates, each later one drawn on a side stream
    while the caller runs the previous epoch on the current stream (torch's randperm at 1 M rows
    is a ~0.25 ms chain of small sort launches). Same draws, same order, same generator as a
    sequential loop of torch.randperm calls; each yielded tensor is ready on the current stream."""
    if n_epochs <= 0:
        return
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    nxt = torch.randperm(n, device=dev, generator=generator)
    for e in range(n_epochs):
        perm, ready = nxt, None
        if e + 1 < n_epochs:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                nxt = torch.randperm(n, device=dev, generator=generator)
                ready = side.record_event()
        yield perm
        if ready is not None:
            main.wait_event(ready)
            nxt.record_stream(main)  # drawn on the side stream, read on this one


def ppo_update(policy, optimizer, ro, n_epochs=10, batch_size=65536, clip_range=0.2, ent_coef=0.01,
               vf_coef=0.5, max_grad_norm=0.5, generator=None, group=None, fused=False, clip_range_vf=None,
               normalize_advantage=True, target_kl=None):
    """SB3 1.6 PPO.train on the device-resident rollout (advantage normalisation per
    minibatch, clipped surrogate, unclipped value loss, entropy bonus, grad-norm clip).
    ent_coef 0.01 as main_6DOF.py:68.

    Multi-GPU (one policy replica per GPU): with a torch.distributed `group`
    every rank collects from its own env shard and updates on its own rollout; the
    minibatch gradients are averaged over the ranks (one all_reduce) before the grad-norm
    clip and the optimizer step, so replicas that start equal stay equal. Ranks must run
    the same number of minibatches (equal shard sizes); advantages are normalised per
    rank's minibatch.

    ``fused=True``: the loss + backward of every minibatch is ``PPOGrad`` (one HIP pipeline)
    instead of PyTorch autograd, and for a capturable Adam the clip + optimizer step is
    ``ClipAdam`` (one launch) on the optimizer's own state; the all_reduce is unchanged.

    ``clip_range_vf`` / ``normalize_advantage`` / ``target_kl`` are SB3's (None / True / None: its
    defaults, and this function's behaviour without them). The autograd path implements all three,
    ``target_kl`` with SB3's ``break``. ``fused=True`` takes them on the one-replica path with a
    capturable Adam (``PPOUpdate``: ``rr_ppo_update_opts``, the stop carried on the device) and
    refuses them elsewhere. ``target_kl`` with a ``group`` is refused everywhere: every rank would
    decide on its own minibatch's KL."""
    n = ro.n_steps * ro.env.num_envs
    cvf, norm, tkl = _ppo_options(clip_range_vf, normalize_advantage, target_kl)
    if tkl and group is not None:
        raise ValueError("target_kl with a group is not supported: the ranks would stop at different minibatches")
    if fused and (cvf or tkl or not norm) and (group is not None
                                               or not clip_adam_supported(optimizer, list(policy.parameters()))):
        raise ValueError("fused=True takes clip_range_vf / normalize_advantage=False / target_kl only on the "
                         "one-replica path with a capturable torch.optim.Adam (rr_ppo_update_opts), not with a "
                         "group or another optimizer")
    if fused:
        perms = _epoch_perms(n, n_epochs, ro.obs.device, generator)
        if n % min(batch_size, n) == 1:
            # checked before the first minibatch: a 1-row remainder cannot be normalised (PPOGrad
            # refuses it) and failing there would leave the epoch's earlier Adam steps applied
            raise ValueError("n_steps * num_envs = %d leaves a 1-row last minibatch at batch_size %d (rr_ppo_grad "
                             "needs >= 2 rows); choose another batch_size" % (n, batch_size))
        params = list(policy.parameters())
        stats = None
        if group is None and clip_adam_supported(optimizer, params):
            # the whole minibatch step in one call, chained: each call sums the next one's statistics
            step = PPOUpdate(policy, optimizer, ro, min(batch_size, n), clip_range, ent_coef, vf_coef, max_grad_norm,
                             clip_range_vf, normalize_advantage, target_kl)
            kw = {}
            for perm in perms:
                for s in range(0, n, step.bs):
                    nxt = perm[s + step.bs:s + 2 * step.bs] if s + step.bs < n else None
                    if step.opts is not None:
                        kw = dict(epoch_start=s == 0)
                    stats = step(perm[s:s + step.bs], nxt, chained=s > 0, **kw)
            return {} if stats is None else dict(zip(("policy_loss", "value_loss", "entropy"), stats[:3].tolist()))
        grad = PPOGrad(policy, ro, min(batch_size, n), clip_range, ent_coef, vf_coef)
        adam = ClipAdam(optimizer, params, max_grad_norm) if clip_adam_supported(optimizer, params) else None
        for perm in perms:
            for s in range(0, n, grad.bs):
                stats = grad(perm[s:s + grad.bs])
                if group is not None:
                    _allreduce_grads(params, group)
                if adam is not None:
                    adam()
                else:
                    torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
                    optimizer.step()
        return {} if stats is None else dict(zip(("policy_loss", "value_loss", "entropy"), stats[:3].tolist()))
    obs = ro.obs.reshape(n, -1)
    act = ro.actions.reshape(n, -1)
    old_lp = ro.log_probs.reshape(n)
    adv_all = ro.advantages.reshape(n)
    ret = ro.returns.reshape(n)
    old_v = ro.values.reshape(n) if cvf else None
    stats = {}
    stop = False
    for _ in range(n_epochs):
        if stop:
            break
        perm = torch.randperm(n, device=obs.device, generator=generator)
        for s in range(0, n, batch_size):
            idx = perm[s:s + batch_size]
            mean, value = policy(obs[idx])
            lp = policy.log_prob(mean, act[idx])
            adv = adv_all[idx]
            if norm:
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            ratio = torch.exp(lp - old_lp[idx])
            pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
            if cvf:
                value = old_v[idx] + torch.clamp(value - old_v[idx], -cvf, cvf)
            vf = torch.nn.functional.mse_loss(ret[idx], value)
            ent = -policy.entropy(len(idx)).mean()
            loss = pg + ent_coef * ent + vf_coef * vf
            if tkl:
                with torch.no_grad():
                    log_ratio = lp - old_lp[idx]
                    kl = float(((torch.exp(log_ratio) - 1) - log_ratio).mean())
                if kl > 1.5 * tkl:  # SB3: the minibatch's losses are logged, its step is not taken
                    stats = {"policy_loss": pg.detach(), "value_loss": vf.detach(), "entropy": -ent.detach()}
                    stop = True
                    break
            optimizer.zero_grad(set_to_none=True)
            loss.backward()
            if group is not None:
                _allreduce_grads(list(policy.parameters()), group)
            torch.nn.utils.clip_grad_norm_(policy.parameters(), max_grad_norm)
            optimizer.step()
            stats = {"policy_loss": pg.detach(), "value_loss": vf.detach(), "entropy": -ent.detach()}
    return {k: float(v) for k, v in stats.items()}


class GraphedPPOUpdate:
    """``ppo_update``'s minibatch step — gather, forward, clipped-surrogate / value / entropy
    loss, backward, (multi-GPU gradient all_reduce), grad-norm clip, Adam step — captured ONCE
    into a hipGraph — one graph per EPOCH: the minibatch steps of one pass over the rollout,
    each reading its rows from a static permutation buffer that ``update`` refills with
    ``torch.randperm`` before every replay (no per-minibatch index copy or graph launch).

    ``fused`` (default: wherever ``PPOGrad`` supports the policy) takes the loss + backward from
    ``PPOGrad`` (rr_ppo_grad: one fp32-MFMA HIP pipeline) instead of PyTorch autograd, whose
    tall-skinny GEMMs over the 65 536-row minibatch run far below the GPU's rate (the weight
    gradient dW = g^T x alone ~190 us per layer: profiles/r03/r03i); the gradients then
    match the eager update's to fp32 rounding instead of bitwise. ``fused=False`` captures the
    PyTorch ops themselves (bitwise the eager ``ppo_update``).

    Needs an optimizer created with ``capturable=True`` (``torch.optim.Adam(..., capturable=True)``:
    its step count lives on the device) and ``n_steps * num_envs`` divisible by ``batch_size``.
    The warm-up steps the capture requires run on the real parameters and are undone (parameters
    and optimizer state restored in place), so the first ``update`` starts from the same state
    as the eager ``ppo_update`` would, and computes the same minibatch steps (``fused=False``: same
    kernels, same order; ``tests/test_gpu_rollout.py``). Multi-GPU: ``group`` must be an RCCL ("nccl") group —
    the all_reduce is captured with the rest.

    ``clip_range_vf`` / ``normalize_advantage`` / ``target_kl`` / ``train_stats`` (SB3's defaults and
    False: exactly the calls described above) put the fused one-replica path on
    ``rr_ppo_update_opts`` (``PPOUpdate``). ``update`` then clears the control block, every epoch's
    first minibatch is captured with the epoch-start flag, and a KL stop needs no host decision: the
    epochs after it replay as no-ops, and ``update`` still never waits for the device on their
    account. ``train_stats()`` returns SB3's ``train/*`` means over the last ``update`` with one
    copy. ``fused=False`` captures ``clip_range_vf`` and ``normalize_advantage`` as PyTorch ops and
    refuses ``target_kl`` (a ``break`` cannot be captured); the split multi-GPU path refuses all."""

    def __init__(self, policy, optimizer, ro, batch_size=65536, clip_range=0.2, ent_coef=0.01, vf_coef=0.5,
                 max_grad_norm=0.5, group=None, fused=None, clip_range_vf=None, normalize_advantage=True,
                 target_kl=None, train_stats=False):
        if not all(g.get("capturable", False) for g in optimizer.param_groups):
            raise ValueError("GraphedPPOUpdate needs an optimizer with capturable=True")
        cvf, norm, tkl = _ppo_options(clip_range_vf, normalize_advantage, target_kl)
        self._opt = (cvf, norm, tkl)
        if tkl and group is not None:
            raise ValueError("target_kl with a group is not supported: the ranks would stop at different minibatches")
        n = ro.n_steps * ro.env.num_envs
        if n % batch_size:
            raise ValueError("n_steps * num_envs (%d) must be a multiple of batch_size (%d)" % (n, batch_size))
        if group is not None:
            import torch.distributed as dist
            if dist.get_backend(group) != "nccl":
                raise ValueError("a captured gradient all_reduce needs the nccl (RCCL) backend")
        self.policy, self.optimizer, self.ro, self.group = policy, optimizer, ro, group
        self.n, self.bs = n, batch_size
        dev = ro.obs.device
        self.obs = ro.obs.reshape(n, -1)
        self.act = ro.actions.reshape(n, -1)
        self.old_lp = ro.log_probs.reshape(n)
        self.adv_all = ro.advantages.reshape(n)
        self.ret = ro.returns.reshape(n)
        self.coef = (clip_range, ent_coef, vf_coef, max_grad_norm)
        self.perm = torch.arange(n, device=dev)  # refilled per epoch; minibatch k = perm[k bs : (k + 1) bs]
        self._perm_bufs = self._perm_stream = None  # update(): the next epoch's permutation, drawn aside
        self._first = None  # prepare(): the event of the next update's first draw
        self.n_mb = n // batch_size
        params = list(policy.parameters())
        # state to restore after the warm-up steps (in place: the graph keeps these tensors)
        saved_p = [p.detach().clone() for p in params]
        saved_s = {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in optimizer.state[p].items()}
                   for p in params if p in optimizer.state}
        # static gradient buffers (allocated outside the graph): the captured step copies
        # torch.autograd.grad's results into them, so no accumulation into .grad is captured. The
        # policy's Linear layers must take their bias gradient as a GEMM (_LinearFn): a column sum
        # after a GEMM in the same graph is wrong from the second replay on (profiles/r03/r03i/probe_graph_reduce.txt)
        self.params = params
        for p in params:
            p.grad = torch.zeros_like(p)
        if fused is None:
            fused = fused_grad_supported(policy, ro.env.state_dim, ro.env.action_dim)
        self.fused = bool(fused)
        one_call = self.fused and group is None and clip_adam_supported(optimizer, params)
        if not one_call and (train_stats or tkl or (self.fused and (cvf or not norm))):
            raise ValueError("clip_range_vf / normalize_advantage=False on the fused path, target_kl and train_stats "
                             "need the fused one-replica update with a capturable torch.optim.Adam "
                             "(rr_ppo_update_opts); fused=False takes clip_range_vf and normalize_advantage only")
        self.old_v = _old_values(ro, n) if cvf and not self.fused else None
        # fused, one replica, capturable Adam: the chained whole-minibatch call (rr_ppo_update, or
        # rr_ppo_update_opts with an option or train_stats)
        self._update = (PPOUpdate(policy, optimizer, ro, batch_size, clip_range, ent_coef, vf_coef, max_grad_norm,
                                  clip_range_vf, normalize_advantage, target_kl, train_stats)
                        if one_call else None)
        self._grad = (PPOGrad(policy, ro, batch_size, clip_range, ent_coef, vf_coef)
                      if self.fused and self._update is None else None)
        self._adam = (ClipAdam(optimizer, params, max_grad_norm)
                      if self._grad is not None and clip_adam_supported(optimizer, params) else None)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for k in range(3):
                self._step(self._mb(k % self.n_mb), k % self.n_mb)
        torch.cuda.current_stream(dev).wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for k in range(self.n_mb):
                self.stats = self._step(self._mb(k), k)
        with torch.no_grad():
            for p, v in zip(params, saved_p):
                p.copy_(v)
            for p in params:
                st = optimizer.state.get(p)
                if not st:
                    continue
                old = saved_s.get(id(p))
                for k, v in st.items():
                    if torch.is_tensor(v):
                        if old is not None and k in old:
                            v.copy_(old[k])
                        else:
                            v.zero_()  # state the warm-up created: back to a fresh optimizer's
        if self._update is not None and self._update.opts is not None:
            self._update.reset()  # what the warm-up and the capture's eager side counted
        torch.cuda.synchronize(dev)

    def _mb(self, k):
        return self.perm[k * self.bs:(k + 1) * self.bs]

    def _step(self, i, k=0):
        clip_range, ent_coef, vf_coef, max_grad_norm = self.coef
        pol = self.policy
        if self._update is not None:
            kw = dict(epoch_start=k == 0) if self._update.opts is not None else {}
            st = self._update(i, self._mb(k + 1) if k + 1 < self.n_mb else None, chained=k > 0, **kw)
            self._more = (st[3], st[4])
            return {"policy_loss": st[0], "value_loss": st[1], "entropy": st[2]}
        if self.fused:
            st = self._grad(i)
            self._more = (st[3], st[4])
            if self.group is not None:
                _allreduce_grads(self.params, self.group)
            if self._adam is not None:
                self._adam()
            else:
                torch.nn.utils.clip_grad_norm_(self.params, max_grad_norm)
                self.optimizer.step()
            return {"policy_loss": st[0], "value_loss": st[1], "entropy": st[2]}
        cvf, norm, _ = self._opt
        mean, value = pol(self.obs[i])
        lp = pol.log_prob(mean, self.act[i])
        adv = self.adv_all[i]
        if norm:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(lp - self.old_lp[i])
        pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
        if cvf:
            value = self.old_v[i] + torch.clamp(value - self.old_v[i], -cvf, cvf)
        vf = torch.nn.functional.mse_loss(self.ret[i], value)
        ent = -pol.entropy(self.bs).mean()
        loss = pg + ent_coef * ent + vf_coef * vf
        for p, g in zip(self.params, torch.autograd.grad(loss, self.params)):
            p.grad.copy_(g)
        if self.group is not None:
            _allreduce_grads(self.params, self.group)
        torch.nn.utils.clip_grad_norm_(pol.parameters(), max_grad_norm)
        self.optimizer.step()
        with torch.no_grad():  # SB3 1.6 PPO.train's clip_fraction and approx_kl, as rr_ppo_grad's stats[3:5]
            log_ratio = lp - self.old_lp[i]
            self._more = ((torch.abs(ratio - 1) > clip_range).float().mean(), ((ratio - 1) - log_ratio).mean())
        return {"policy_loss": pg.detach(), "value_loss": vf.detach(), "entropy": -ent.detach()}

    def last_stats(self):
        """The last minibatch step's five figures as ``train/*`` keys: ``update``'s three and the
        ``clip_fraction`` / ``approx_kl`` the step computes beside them. One iteration's log dict is
        ``ro.stats.last() | upd.last_stats()``."""
        out = {"train/" + k: float(v) for k, v in self.stats.items()}
        out["train/clip_fraction"], out["train/approx_kl"] = (float(v) for v in self._more)
        return out

    def train_stats(self):
        """SB3 PPO.train's log figures over the last ``update``, from the control block with one copy:
        ``train/policy_gradient_loss``, ``train/value_loss``, ``train/entropy_loss``,
        ``train/clip_fraction`` (means over every evaluated minibatch), ``train/approx_kl`` (mean
        over the last, possibly partial, epoch), ``train/n_minibatches`` (optimizer steps applied),
        ``train/n_evaluated``, ``train/early_stop`` and ``train/stop_epoch`` (None without a stop)."""
        if self._update is None or self._update.opts is None:
            raise ValueError("train_stats() needs GraphedPPOUpdate(train_stats=True) or one of the options on the "
                             "fused one-replica path")
        return self._update.train_stats()

    def _perm_streams(self):
        dev = self.obs.device
        if self._perm_bufs is None:
            self._perm_bufs = (torch.empty_like(self.perm), torch.empty_like(self.perm))
            self._perm_stream = torch.cuda.Stream(dev)
        return torch.cuda.current_stream(dev), self._perm_bufs, self._perm_stream

    def prepare(self, generator=None):
        """Draw the next ``update``'s first-epoch permutation now, on the side stream: called
        before the rollout collect, the draw runs beside it instead of ahead of the first
        epoch. It is the draw ``update`` would make first; pass ``update`` the same generator
        and draw nothing else from it in between."""
        main, bufs, side = self._perm_streams()
        side.wait_stream(main)  # the previous update's readers of bufs[0] are done
        with torch.cuda.stream(side):
            torch.randperm(self.n, out=bufs[0], generator=generator)
            self._first = side.record_event()

    def update(self, n_epochs=10, generator=None):
        """n_epochs passes over the rollout in shuffled minibatches (ppo_update's order:
        one torch.randperm per epoch).

        Each later epoch's permutation is drawn on a side stream while the previous epoch's graph
        replays: torch's randperm is a ~0.25 ms chain of small sort launches at 1 M rows, and the
        learner's kernels leave most of each SIMD's wave slots free. The draws are issued in the
        same order from the same generator, so the permutations are the sequential loop's. After
        ``prepare`` the first epoch uses the permutation drawn there."""
        for o in (self._adam, self._update):
            if o is not None:
                o.sync_lr()  # the graph reads lr from the device: follow param_groups[0]["lr"]
        if self._update is not None and self._update.opts is not None:
            self._update.reset()  # a new train() pass: stop state and running sums cleared, stream-ordered
        main, bufs, side = self._perm_streams()
        ready, self._first = self._first, None
        if ready is None:  # no prepare(): the first epoch's draw in line
            torch.randperm(self.n, out=bufs[0], generator=generator)
        for e in range(n_epochs):
            cur = bufs[e % 2]
            if ready is not None:
                main.wait_event(ready)
            self.perm.copy_(cur)
            if e + 1 < n_epochs:
                side.wait_stream(main)  # the other buffer's last reader (the previous copy) is done
                with torch.cuda.stream(side):
                    torch.randperm(self.n, out=bufs[(e + 1) % 2], generator=generator)
                    ready = side.record_event()
            self.graph.replay()
        return {k: float(v) for k, v in self.stats.items()}


# ---- deterministic policy evaluation (SB3 EvalCallback / evaluate_policy + EpisodeAnalyzer) ----

from ._lib import (RR_EVAL_BOUNDS as EVAL_BOUNDS, RR_EVAL_EVENT as EVAL_EVENT, RR_EVAL_LANDED as EVAL_LANDED,  # noqa: E402
                   RR_EVAL_NONFINITE as EVAL_NONFINITE, RR_EVAL_TRUNCATED as EVAL_TRUNCATED)
from .eval_trace import EpisodeRecord, EvalTrace  # noqa: E402,F401


class EvalResult:
    """The per-episode outputs of one evaluation, as tensors on the evaluator's device (views of
    its buffers: the next ``run()`` overwrites them): ``episodes`` [n] (episodes env i completed),
    ``ep_return`` / ``ep_length`` / ``flags`` / ``used_mass`` [n_episodes, n] and ``final_state``
    [n_episodes, state_dim, n] (the terminal state, un-normalised). Row [k, i] is valid where
    ``k < episodes[i]``; ``finished()`` is that mask. ``trace`` is the ``EvalTrace`` of the envs the
    evaluator records (``PolicyEvaluator(record=...)``), else None."""

    def __init__(self, episodes, ep_return, ep_length, flags, used_mass, final_state, state_names, trace=None):
        self.episodes, self.ep_return, self.ep_length, self.flags = episodes, ep_return, ep_length, flags
        self.used_mass, self.final_state, self.state_names = used_mass, final_state, list(state_names)
        self.trace = trace

    def finished(self):
        k = torch.arange(self.ep_return.shape[0], device=self.episodes.device)
        return k[:, None] < self.episodes[None, :]

    def stats(self):
        """One synchronise (a single device-to-host copy). SB3 ``evaluate_policy``'s
        ``mean_reward`` / ``std_reward`` (population std) and ``mean_ep_length``; the reference
        EpisodeAnalyzer's ``ep_statistic/landing_success`` (here the rate of episodes whose last
        step paid the landing reward), ``ep_statistic/used_mass`` and ``final_errors/<state name>``
        (mean |terminal state|, wrappers.py:210-224); the counts of each way an episode ended
        (``n_event`` / ``n_bounds`` / ``n_truncated`` / ``n_nonfinite``), ``episodes`` and
        ``unfinished`` (rows not completed within max_steps, excluded from every mean)."""
        m = self.finished()
        w = m.double()
        cnt = w.sum()
        ret = torch.where(m, self.ep_return.double(), torch.zeros_like(w))
        mean = ret.sum() / cnt
        var = (torch.where(m, (self.ep_return.double() - mean) ** 2, torch.zeros_like(w))).sum() / cnt
        fl = torch.where(m, self.flags.to(torch.int64), torch.zeros_like(m, dtype=torch.int64))
        fe = torch.where(m[:, None, :], self.final_state.double().abs(), torch.zeros_like(w)[:, None, :])
        vals = [mean, var.sqrt(),
                torch.where(m, self.ep_length.double(), torch.zeros_like(w)).sum() / cnt,
                (fl & EVAL_LANDED).ne(0).double().sum() / cnt,
                torch.where(m, self.used_mass.double(), torch.zeros_like(w)).sum() / cnt]
        vals += [(fl & bit).ne(0).double().sum() for bit in (EVAL_EVENT, EVAL_BOUNDS, EVAL_TRUNCATED, EVAL_NONFINITE)]
        vals += [cnt, m.numel() - cnt]
        host = torch.cat([torch.stack(vals), fe.sum(dim=(0, 2)) / cnt]).cpu().tolist()
        out = dict(zip(("mean_reward", "std_reward", "mean_ep_length", "ep_statistic/landing_success",
                        "ep_statistic/used_mass"), host[:5]))
        for k, v in zip(("n_event", "n_bounds", "n_truncated", "n_nonfinite", "episodes", "unfinished"), host[5:11]):
            out[k] = int(v)
        for name, v in zip(self.state_names, host[11:]):
            out["final_errors/" + name] = v
        return out


class PolicyEvaluator:
    """Deterministic evaluation of ``policy`` on every env of a ``RocketBatch`` (auto-reset, with
    a TimeLimit or ``max_steps``): each env runs ``n_episodes`` episodes under the policy's mean
    action, starting from the batch's CURRENT state (reset first for whole episodes), and rests at
    the first state of a fresh episode afterwards. ``run()`` launches and returns an ``EvalResult``
    without synchronising; ``batch.obs`` holds the post-call observation.

    ``fused=True`` (default for an ``MlpActorCritic`` with 64x64 towers on an RK4 / Euler env): ONE
    launch (``rr_policy_evaluate``: the collect kernel's step loop with only the pi tower, state in
    registers, nothing stored per step), capturable in a graph. On an ``integrator="dopri5"`` batch
    ``fused=True`` must be asked for and is ``rr_policy_evaluate_exact``: the same loop around the exact
    solver, one launch where the step-by-step path takes two exact steps and a dozen small launches
    per iteration, bit for bit the episodes of ``rr_policy_act`` + ``rr_step`` (it does not record:
    ``record=`` with it raises). ``fused=False`` (any policy whose
    ``policy(obs)[0]`` is the action mean, and the default for ``integrator="dopri5"``): the same algorithm in
    PyTorch ops, one ``batch.step`` per iteration for ``max_steps`` iterations; the un-reset terminal
    state and the reward terms of each step come from a shadow batch without auto-reset stepped
    from the same state, and envs that have finished are put back after every step.
    ``max_steps`` (default ``n_episodes * max_episode_steps``) caps the steps of each env; episodes
    not completed by then leave their rows untouched (``EvalResult.episodes`` counts).

    ``record`` (a sequence or tensor of env indices local to the batch, unique, any order) records
    whole episodes of those envs: ``EvalResult.trace`` is then an ``EvalTrace`` with, per recorded
    env and episode, the un-normalised state before the episode's first step and after every step,
    the clipped mean actions, the reward terms and rewards, and the episode's length; its
    ``episode(env_id, k)`` gives the dataframes and figures of the reference's ``EpisodeAnalyzer``.
    The fused path does it in the same single launch (``rr_policy_evaluate_trace``); the evaluation
    itself is bit for bit the unrecorded one. ``record_steps`` is the recorded steps per episode
    (default ``max_episode_steps``; required without a TimeLimit): longer episodes are clipped, their
    ``length`` still counts every step. An episode's step count starts at the call, and the v_targ
    history takes v_0 from the first recorded state: reset first, as for whole episodes.
    ``record=None`` is the plain evaluation (``rr_policy_evaluate``)."""

    def __init__(self, batch, policy, n_episodes=5, max_steps=None, policy_dtype="fp32", fused=None, record=None,
                 record_steps=None):
        from . import _lib
        from .params import STATE_NAMES_3DOF, STATE_NAMES_6DOF

        self.env, self.policy = batch, policy
        n, ns, na = batch.num_envs, batch.state_dim, batch.action_dim
        dev = batch.device
        p = batch.params
        if not p.flags & _lib.RR_FLAG_AUTO_RESET:
            raise ValueError("PolicyEvaluator needs a RocketBatch with auto_reset=True")
        self.n_episodes = int(n_episodes)
        if self.n_episodes < 1:
            raise ValueError("n_episodes must be at least 1")
        self.max_steps = int(max_steps) if max_steps else self.n_episodes * int(p.max_episode_steps)
        if self.max_steps <= 0:
            raise ValueError("an env without a TimeLimit needs max_steps")
        dopri = int(p.integrator) == _lib.RR_INT_DOPRI5
        if fused is None:  # an exact-mode batch keeps the step-by-step path unless asked (fused=True)
            fused = fused_grad_supported(policy, ns, na) and not dopri
        if fused and not fused_grad_supported(policy, ns, na):
            raise ValueError("fused evaluation needs an MlpActorCritic with 64x64 towers")
        if fused and dopri and record is not None:
            raise ValueError("record= on an integrator=\"dopri5\" batch needs fused=False (the one-launch exact "
                             "evaluation does not record)")
        self.fused = bool(fused)
        self._exact = self.fused and dopri
        if policy_dtype not in POLICY_PRECISIONS:
            raise ValueError("policy_dtype must be one of %s" % sorted(POLICY_PRECISIONS))
        if policy_dtype != "fp32" and not self.fused:
            raise ValueError("policy_dtype=%r needs the fused HIP policy path" % policy_dtype)
        self.policy_dtype = policy_dtype
        ne = self.n_episodes
        self.episodes = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.ep_return = torch.zeros((ne, n), dtype=torch.float32, device=dev)
        self.ep_length = torch.zeros((ne, n), dtype=torch.int32, device=dev)
        self.flags = torch.zeros((ne, n), dtype=torch.uint8, device=dev)
        self.used_mass = torch.zeros((ne, n), dtype=torch.float32, device=dev)
        self.final_state = torch.zeros((ne, ns, n), dtype=torch.float32, device=dev)
        self.trace = self._make_trace(record, record_steps)
        self.result = EvalResult(self.episodes, self.ep_return, self.ep_length, self.flags, self.used_mass,
                                 self.final_state, STATE_NAMES_6DOF if batch.model == 6 else STATE_NAMES_3DOF,
                                 trace=self.trace)
        self._lib = _lib.load()
        if self.fused:
            self._pack = PolicyPack(policy, ns, na, dev, precision=policy_dtype)
            self._out = _lib.RrEvalOut(*[t.data_ptr() for t in (self.episodes, self.ep_return, self.ep_length,
                                                                 self.flags, self.used_mass, self.final_state)])
            if self.trace is not None:
                tr = self.trace
                self._trace_io = _lib.RrEvalTrace(self._slot.data_ptr(), tr.state.shape[0], tr.steps,
                                                  tr.state.data_ptr(), tr.action.data_ptr(), tr.terms.data_ptr(),
                                                  tr.length.data_ptr())
            return
        from .batch import RocketBatch
        from .params import INTEGRATORS

        integ = {v: k for k, v in INTEGRATORS.items()}
        self._dopri = dopri
        self._stats = bool(p.flags & _lib.RR_FLAG_EPISODE_STATS)
        # the same env without auto-reset, TimeLimit or Monitor: stepped from the batch's pre-step
        # state, it leaves the un-reset terminal state and the reward terms of the step
        self._shadow = RocketBatch(n, model=batch.model, device=dev, max_episode_steps=0, auto_reset=False,
                                   episode_stats=False, reward_annealing=bool(p.flags & _lib.RR_FLAG_REWARD_ANNEALING),
                                   integrator=integ[int(p.integrator)], env_id_offset=batch.env_id_offset,
                                   compute_terms=True, scipy_h0_clamp=bool(p.flags & _lib.RR_FLAG_SCIPY_H0_CLAMP),
                                   **batch.cfg.kwargs)
        self._none = torch.zeros((n,), dtype=torch.uint8, device=dev)
        self._tlen = torch.zeros((n,), dtype=torch.int32, device=dev)

    def _make_trace(self, record, record_steps):
        """The slot plane ([n] int32: the trace slot of env i, -1 = not recorded) and the trace
        buffers of ``record``, allocated once; None without ``record``."""
        if record is None:
            if record_steps is not None:
                raise ValueError("record_steps needs record")
            return None
        env = self.env
        n, dev = env.num_envs, env.device
        ids = torch.as_tensor(record).reshape(-1).to(torch.int64).cpu()
        if ids.numel() < 1:
            raise ValueError("record must name at least one env")
        if int(ids.min()) < 0 or int(ids.max()) >= n:
            raise ValueError("record holds an env index outside [0, %d)" % n)
        if ids.unique().numel() != ids.numel():
            raise ValueError("record holds an env index twice")
        steps = int(record_steps) if record_steps else int(env.params.max_episode_steps)
        if steps < 1:
            raise ValueError("an env without a TimeLimit needs record_steps")
        k, ne = ids.numel(), self.n_episodes
        slot = torch.full((n,), -1, dtype=torch.int32)
        slot[ids] = torch.arange(k, dtype=torch.int32)
        self._slot = slot.to(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        return EvalTrace(env.cfg, torch.zeros((k, ne, steps + 1, env.state_dim), **f32),
                         torch.zeros((k, ne, steps, env.action_dim), **f32),
                         torch.zeros((k, ne, steps, env.n_terms + 1), **f32),
                         torch.zeros((ne, k), dtype=torch.int32, device=dev), ids.to(dev), episodes=self.episodes)

    @torch.no_grad()
    def run(self):
        if not self.fused:
            return self._run_unfused()
        import ctypes

        from . import _lib
        from .batch import _ptr

        env = self.env
        stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        if self.trace is not None:
            _lib.check(self._lib.rr_policy_evaluate_trace(env._h, _ptr(self._pack.pack()), self._pack.prec,
                                                          self.n_episodes, self.max_steps, ctypes.byref(self._out),
                                                          ctypes.byref(self._trace_io), _ptr(env.obs), stream),
                       "rr_policy_evaluate_trace")
            return self.result
        call, name = ((self._lib.rr_policy_evaluate_exact, "rr_policy_evaluate_exact") if self._exact else
                      (self._lib.rr_policy_evaluate, "rr_policy_evaluate"))
        _lib.check(call(env._h, _ptr(self._pack.pack()), self._pack.prec, self.n_episodes, self.max_steps,
                        ctypes.byref(self._out), _ptr(env.obs), stream), name)
        return self.result

    # -- fused=False: the kernel's algorithm in PyTorch ops ---------------------------------------------------
    def _snap(self, env):
        import ctypes

        from . import _lib
        from .batch import _ptr

        st, v0, _ = env.get_state64() if self._dopri else env.get_state()
        cw = torch.empty((env.num_envs,), dtype=torch.int32, device=env.device)
        ret = torch.empty((env.num_envs,), dtype=torch.float32, device=env.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        _lib.check(self._lib.rr_get_aux(env._h, _ptr(cw), _ptr(ret), stream), "rr_get_aux")
        return st, v0, cw, ret

    def _put(self, env, st, v0, cw, ret):
        import ctypes

        from . import _lib
        from .batch import _ptr

        (env.set_state64 if self._dopri else env.set_state)(st, v0=v0, elapsed=cw)
        self._keep = (cw, ret)
        stream = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        _lib.check(self._lib.rr_set_aux(env._h, _ptr(cw), _ptr(ret), stream), "rr_set_aux")

    def _mean(self, obs):
        pol = self.policy
        if isinstance(pol, MlpActorCritic):
            return pol.action_net(pol.pi_net(obs))  # the pi tower only
        return pol(obs)[0]

    def _run_unfused(self):
        env, sh, ne = self.env, self._shadow, self.n_episodes
        n, nt = env.num_envs, env.n_terms
        el_mask = (1 << env.counter_bits) - 1

        def put_row(plane, ep, mask, val):  # plane[ep[i], ..., i] = val[..., i] where mask[i]
            idx = ep.clamp(max=ne - 1).long().expand(val.shape)[None]
            plane.scatter_(0, idx, torch.where(mask, val, plane.gather(0, idx)[0])[None])

        obs = env.reset(mask=self._none)  # no env is reset: the obs of the current state
        pre = self._snap(env)
        ep = torch.zeros_like(self.episodes)
        tr = self.trace
        if tr is not None:  # the kernel's records of the recorded envs, same rows, same tensors
            ids, cap = tr.env_ids, tr.steps
            ks = torch.arange(ids.numel(), device=ids.device)
            t_rec = torch.zeros_like(ids)  # steps of the running episode taken in this call
            tr.state[ks, 0, 0] = pre[0].float()[:, ids].T
        ret = pre[3].clone() if self._stats else torch.zeros_like(pre[3])
        m0 = pre[0][-1].float()
        for _ in range(self.max_steps):
            active = ep < ne
            act = torch.clamp(self._mean(obs), -1.0, 1.0)
            (sh.set_state64 if self._dopri else sh.set_state)(pre[0], v0=pre[1], elapsed=pre[2] & el_mask)
            sh.step(act)
            y1 = (sh.get_state64() if self._dopri else sh.get_state())[0].float()
            terms = sh.terms
            obs, rew, done, trunc = env.step(act)
            env.copy_terminal(out=(None, None, self._tlen))
            post = self._snap(env)
            ret = torch.where(active, ret + rew, ret)
            end = active & done.bool()
            status = terms[nt + 1]
            fl = ((status > 0) * EVAL_EVENT + (terms[nt] > 0) * EVAL_BOUNDS + trunc.bool() * EVAL_TRUNCATED
                  + (status < 0) * EVAL_NONFINITE + (terms[nt - 1] != 0) * EVAL_LANDED).to(torch.uint8)
            put_row(self.ep_return, ep, end, ret)
            put_row(self.ep_length, ep, end, self._tlen)
            put_row(self.flags, ep, end, fl)
            put_row(self.used_mass, ep, end, m0 - y1[-1])
            put_row(self.final_state, ep, end, y1)
            if tr is not None:
                act_r, end_r, ep_r = active[ids], end[ids], ep[ids].long()
                w = act_r & (t_rec < cap)  # steps past the capacity are counted, not written
                kw, ew, tw = ks[w], ep_r[w], t_rec[w]
                tr.state[kw, ew, tw + 1] = y1[:, ids].T[w]
                tr.action[kw, ew, tw] = act[ids][w]
                tr.terms[kw, ew, tw] = torch.cat([terms[:nt, ids].T, rew[ids, None]], dim=1)[w]
                t_rec = t_rec + act_r.to(t_rec.dtype)
                tr.length[ep_r[end_r], ks[end_r]] = t_rec[end_r].to(torch.int32)
                t_rec = torch.where(end_r, torch.zeros_like(t_rec), t_rec)
                nxt = end_r & (ep_r + 1 < ne)  # row 0 of the next episode: the auto-reset state
                tr.state[ks[nxt], ep_r[nxt] + 1, 0] = post[0].float()[:, ids].T[nxt]
            ret = torch.where(end, torch.zeros_like(ret), ret)
            m0 = torch.where(end, post[0][-1].float(), m0)
            ep = ep + end.to(ep.dtype)
            # envs that had finished before this step stay where they were
            pre = tuple(torch.where(active, b, a) for a, b in zip(pre, post))
            self._put(env, *pre)
        self.episodes.copy_(ep)
        if tr is not None:  # episodes cut by max_steps: the steps they took so far
            cut = ep[ids] < ne
            tr.length[ep[ids].long()[cut], ks[cut]] = t_rec[cut].to(torch.int32)
        env.reset(mask=self._none)  # env.obs of the final state
        return self.result


def evaluate_policy(policy, batch, n_eval_episodes=5, return_episode_rewards=False, **kw):
    """SB3 ``evaluate_policy(model, env, n_eval_episodes, deterministic=True)`` on a ``RocketBatch``:
    resets every env, runs a ``PolicyEvaluator`` (``**kw``: max_steps, policy_dtype, fused) and
    returns ``(mean_reward, std_reward)`` or, with ``return_episode_rewards``, ``(episode_rewards,
    episode_lengths)`` as lists over the finished episodes.

    ``n_eval_episodes`` is PER ENV here: every env runs that many episodes, N * n_eval_episodes in
    all. SB3 splits a total over the envs of a vec env, which would leave all but n_eval_episodes of
    thousands of envs idle."""
    batch.reset()
    res = PolicyEvaluator(batch, policy, n_episodes=n_eval_episodes, **kw).run()
    if return_episode_rewards:
        m = res.finished().cpu()
        return res.ep_return.cpu()[m].tolist(), res.ep_length.cpu()[m].tolist()
    s = res.stats()
    return s["mean_reward"], s["std_reward"]


from .bc import BCUpdate, Demonstrations, bc_train  # noqa: E402,F401  (behaviour cloning, beside PPOUpdate)
