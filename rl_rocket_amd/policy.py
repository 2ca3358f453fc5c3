"""The policy module and its packer for the fused HIP policy kernels.

``MlpActorCritic`` mirrors SB3 1.6 ``ActorCriticPolicy`` defaults for PPO with
``"MlpPolicy"`` (the reference's ``sb3_config["policy_type"]``, configuration_file.py:41):
separate pi / vf MLPs [64, 64] with tanh, diagonal Gaussian with state-independent
log_std (init 0), orthogonal init (gain sqrt(2) hidden, 0.01 policy head, 1 value head).
``MlpCategoricalActorCritic`` is the policy SB3 builds behind the reference's ``DiscreteActions3DOF``
(wrappers.py:24-35, a ``Discrete(K)`` action space): the same towers and initialisation, an action
head of K logits, no log_std (SB3 ``CategoricalDistribution``). Both derive from ``_MlpTowers``, which
builds and initialises the four nets and holds ``forward`` / ``value``; a class adds its distribution
(``log_std``, or ``table`` and ``n_choices``) and ``log_prob`` / ``entropy``.
"""
import math

import torch
from torch import nn

from .params import DISCRETE_TABLE_3DOF


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


class _MlpTowers(nn.Module):
    """What the two policies share: the pi / vf towers, ``action_net`` with ``out`` rows and ``value_net``,
    initialised in this order (the draws of a seeded generator follow it), and the two forward passes."""

    def __init__(self, obs_dim, out, hidden):
        super().__init__()
        self.hidden = tuple(hidden)

        def mlp():
            layers, d = [], obs_dim
            for h in hidden:
                layers += [_Linear(d, h), nn.Tanh()]
                d = h
            return nn.Sequential(*layers)

        self.pi_net, self.vf_net = mlp(), mlp()
        self.action_net = _Linear(hidden[-1], out)
        self.value_net = _Linear(hidden[-1], 1)
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


class MlpActorCritic(_MlpTowers):
    def __init__(self, obs_dim, act_dim, hidden=(64, 64), log_std_init=0.0):
        super().__init__(obs_dim, act_dim, hidden)
        self.log_std = nn.Parameter(torch.full((act_dim,), float(log_std_init)))

    def log_prob(self, mean, actions):
        std = self.log_std.exp()
        return (-((actions - mean) ** 2) / (2 * std * std) - self.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)

    def entropy(self, n):
        return (0.5 + 0.5 * math.log(2 * math.pi) + self.log_std).sum().expand(n)



class MlpCategoricalActorCritic(_MlpTowers):
    """SB3 1.6 ``MlpPolicy`` over ``Discrete(n_choices)``: ``MlpActorCritic``'s towers and
    initialisation (``action_net`` gain 0.01), ``action_net`` giving ``n_choices`` logits, no
    ``log_std``. ``table`` ([n_choices][2], rows of [gimbal, thrust]) turns an index into the 3DOF
    env's action, as ``DiscreteActions3DOF.action`` does; it is a buffer, not a parameter.
    ``forward`` returns ``(logits, value)``; ``log_prob`` / ``entropy`` / ``mode`` are
    ``CategoricalDistribution``'s, from a log-softmax (a probability that underflows to 0 leaves its
    log finite and its entropy term 0)."""

    def __init__(self, obs_dim, n_choices, table=DISCRETE_TABLE_3DOF, hidden=(64, 64)):
        table = torch.as_tensor(table, dtype=torch.float32)
        if table.dim() != 2 or table.shape != (n_choices, 2) or not bool(torch.isfinite(table).all()):
            raise ValueError("table must be [n_choices][2] finite numbers (rows of [gimbal, thrust])")
        if n_choices < 2:
            raise ValueError("n_choices must be at least 2")
        super().__init__(obs_dim, int(n_choices), hidden)
        self.n_choices = int(n_choices)
        self.register_buffer("table", table.clone())

    def log_prob(self, logits, actions):
        """log p of ``actions`` (indices as floats or integers, [...] or [..., 1]) under ``logits`` [..., K]."""
        a = actions.reshape(logits.shape[:-1]).long()
        return torch.log_softmax(logits, dim=-1).gather(-1, a.unsqueeze(-1)).squeeze(-1)

    def entropy(self, logits):
        lp = torch.log_softmax(logits, dim=-1)
        p = lp.exp()
        return -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(-1)

    def mode(self, logits):
        return logits.argmax(dim=-1)

    def continuous(self, index):
        """The table rows of ``index`` ([...] integers or floats holding them): [..., 2]."""
        return self.table[index.long()]


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
        # a Categorical policy: the 4-head image of rr_policy_layout_discrete, heads >= n_choices zero
        self.discrete = isinstance(policy, MlpCategoricalActorCritic)
        if self.discrete:
            if self.prec:
                raise ValueError("a Categorical policy packs in fp32 only, not %r" % precision)
            if act_dim != policy.n_choices:
                raise ValueError("act_dim is the policy's n_choices for a Categorical policy")
            size = _lib.check(lib.rr_policy_layout_discrete(obs_dim, off), "rr_policy_layout_discrete")
            self._pack = ("rr_policy_pack_discrete", (obs_dim, act_dim))
        else:
            size = _lib.check(lib.rr_policy_layout(obs_dim, act_dim, self.prec, off), "rr_policy_layout")
            self._pack = ("rr_policy_pack", (obs_dim, act_dim, self.prec))  # pack()'s call and its shape arguments
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
        ts = _policy_tensors(self.policy)
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
        src = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.buf.device).cuda_stream)
        call, shape = self._pack
        _lib.check(getattr(_lib.load(), call)(*shape, src, ctypes.c_void_p(self.buf.data_ptr()), stream), call)
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
        if not self.discrete:  # (a Categorical policy's heads past n_choices and its LS slots stay zero)
            self.buf[o["LS"]: o["LS"] + na] = p.log_std
        return self.buf


def _policy_tensors(policy):
    """The 13 parameter tensors in rr_policy_pack / rr_ppo_grad order (12 for a Categorical policy:
    there is no log_std)."""
    p = policy
    ts = [p.pi_net[0].weight, p.pi_net[0].bias, p.pi_net[2].weight, p.pi_net[2].bias,
          p.vf_net[0].weight, p.vf_net[0].bias, p.vf_net[2].weight, p.vf_net[2].bias,
          p.action_net.weight, p.action_net.bias, p.value_net.weight, p.value_net.bias]
    return ts + [p.log_std] if hasattr(p, "log_std") else ts


def fused_grad_supported(policy, obs_dim, act_dim):
    return (isinstance(policy, MlpActorCritic) and policy.hidden == (64, 64)
            and (obs_dim, act_dim) in ((14, 3), (7, 2)))


def fused_discrete_supported(policy, obs_dim):
    """The Categorical policy the discrete HIP calls take: 64x64 towers on the 3DOF env, 2 .. 4 choices."""
    return (isinstance(policy, MlpCategoricalActorCritic) and policy.hidden == (64, 64) and obs_dim == 7
            and 2 <= policy.n_choices <= 4)
