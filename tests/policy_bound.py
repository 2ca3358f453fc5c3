"""A worst-case forward error bound for the rollout policy kernels, the inputs that probe their
domain edges, and NumPy restatements of the two reduced-precision tower paths (tests only; plain
NumPy / PyTorch on the CPU, float64; no kernels here).

``forward_bound(pol, obs, precision)`` returns per row the fp64 action mean and value
(rollout_ref.policy64) and an absolute bound on what a kernel of that precision may differ by.
The bound runs through the layers (tanh is 1-Lipschitz):

    dz1 = (K1 + 2) u (|W1| |x| + |b1|)                 K1 = obs_dim products and sums per unit
    dh1 = dz1 + tau
    dz2 = |W2| dh1 + 66 u f (rowsum |W2| + |b2|)       64 products, 64 sums, the bias, one spare
    dh2 = dz2 + tau
    dy  = |Wh| dh2 + 66 u32 f (rowsum |Wh| + |bh|)     the heads are fp32 on every path

* u: the unit roundoff of the tower products, 2^-24 for "fp32" and 2^-21 for "fp16x3" (operands
  carried as two fp16 halves of v 2^8 keep 22 significant bits: rocket_policy.inc, head comment).
* f = 3 on the fp32 path and 1 elsewhere: the fp32 rollout pack folds the tanh's affine part into
  the next layer (kPolFoldTanh), which evaluates c (b2 + sum W2) - 2c W2 r1 and so carries the
  cancellation of the row sum: the rounded folded bias, the rounded -2c W2 and the products each
  cost one u of rowsum |W2| + |b2|.
* tau = 8 * 2^-24: the absolute error of the kernels' tanh, 1 - 2 / (1 + 2^(2 x log2 e)), given its
  argument: the argument's rounding (|x| sech^2 x <= 0.45, below half a unit), v_exp_f32 and
  v_rcp_f32 at 1 ulp each (the project's kernel guides give these instructions' issue costs but not
  their accuracy; "1 ULP" is what AMD's public CDNA3 / CDNA4 instruction set guides state for
  V_EXP_F32 and V_RCP_F32, and LLVM's AMDGPU backend relies on the same figure when it lowers
  exp2 / the 1 ulp reciprocal to them), the rounding of e + 1 and the final fma: near x = 0, where
  the error is largest (e = 1, d = 2, r = 1/2), these come to 2 (2^-24 + 2^-24 + 2^-25) + 2^-25
  = 5.5 * 2^-24.
* "bf16" gets no analytic bound: it is compared with ``emulate_bf16`` (the kernel's roundings: obs,
  tower weights and the first hidden layer RNE to bf16, everything else exact) under the suite's
  bar (test_gpu_rollout._check_close: max < 1e-2, q99 < 1e-4).

``emulate_fp16x3`` restates the split-fp16 path rounding by rounding (tests/test_policy_bound_cpu.py
holds it, and torch's fp32 forward, against the bound, and shows that the bound notices a dropped
product term)."""
import numpy as np

from rollout_ref import policy64, scaled_policy

U32 = 2.0 ** -24
U16X3 = 2.0 ** -21
TAU = 8 * U32
UNIT = {"fp32": (U32, 3.0), "fp16x3": (U16X3, 1.0)}
F16_OBS_MAX = 255.875          # 65504 / 2^8: the last obs magnitude inside the fp16x3 operand range
SIZES = [(14, 3), (7, 2)]
N_ROWS = 257
WEIGHT_SETS = ("suite", "scaled", "saturated", "constant")
OBS_CLASSES = ("zero", "signed_zero", "tiny", "randn", "randn8", "uniform90", "f16_edge")
BEYOND = (256.0, 300.0, 1e4, 1e6)


def weight_set(name, ns, na):
    """The four seeded policies (CPU, fp32):
    suite      SB3 init + 0.3 N(0, 1) on every parameter (test_gpu_rollout._policy's distribution);
    scaled     rollout_ref.scaled_policy (the same with the action head at 0.05);
    saturated  suite with the tower weights x 8 and biases x 4: most hidden units saturate;
    constant   suite with the tower weights zero (biases kept) and a value head of |w| in [27, 33]:
               the output is a constant of the fold's row sums at the +-60-return scale."""
    import torch

    seed = 40 + ns
    if name not in WEIGHT_SETS:
        raise ValueError(name)
    if name == "scaled":
        return scaled_policy(ns, na, seed)
    pol = scaled_policy(ns, na, seed, head_scale=1.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for net in (pol.pi_net, pol.vf_net):
            for lin in (net[0], net[2]):
                if name == "saturated":
                    lin.weight.mul_(8.0)
                    lin.bias.mul_(4.0)
                elif name == "constant":
                    lin.weight.zero_()
        if name == "constant":
            sign = torch.randint(0, 2, (1, 64), generator=g).float() * 2 - 1
            pol.value_net.weight.copy_(sign * (27.0 + 6.0 * torch.rand((1, 64), generator=g)))
    return pol


def obs_class(name, ns, n=N_ROWS):
    """One seeded fp32 batch [n][ns] of an obs class (OBS_CLASSES)."""
    rng = np.random.default_rng(OBS_CLASSES.index(name) * 100 + ns)
    sign = np.where(rng.random((n, ns)) < 0.5, -1.0, 1.0)
    if name == "zero":
        x = np.zeros((n, ns))
    elif name == "signed_zero":
        x = sign * 0.0
    elif name == "tiny":  # 1e-30 and the fp32 subnormal 1e-40, alternating along a row
        x = sign * np.where((np.arange(ns)[None, :] + np.arange(n)[:, None]) % 2 == 0, 1e-30, 1e-40)
    elif name == "randn":
        x = rng.standard_normal((n, ns))
    elif name == "randn8":
        x = 8.0 * rng.standard_normal((n, ns))
    elif name == "uniform90":  # the envs' own worst case (a lateral ic of mean 0: normalizer 1)
        x = rng.uniform(-90.0, 90.0, (n, ns))
    elif name == "f16_edge":  # one component at +-255.875, the rest N(0, 1)
        x = rng.standard_normal((n, ns))
        r = np.arange(n)
        x[r, r % ns] = np.where(r % 2 == 0, F16_OBS_MAX, -F16_OBS_MAX)
    else:
        raise ValueError(name)
    return x.astype(np.float32)


def beyond_obs(ns, n=N_ROWS):
    """N(0, 1) rows with one component at +-256, +-300, +-1e4, +-1e6 (past the fp16x3 operand
    range), every magnitude, sign and column in turn."""
    rng = np.random.default_rng(900 + ns)
    x = rng.standard_normal((n, ns))
    r = np.arange(n)
    mag = np.asarray(BEYOND)[(r // 2) % len(BEYOND)]
    x[r, (r // (2 * len(BEYOND))) % ns] = np.where(r % 2 == 0, mag, -mag)
    return x.astype(np.float32)


def _np64(t):
    return t.detach().cpu().double().numpy()


def _tower_bound(net, x, u, f):
    w1, b1, w2, b2 = (_np64(t) for t in (net[0].weight, net[0].bias, net[2].weight, net[2].bias))
    k1 = w1.shape[1]
    dz1 = (k1 + 2) * u * (np.abs(x) @ np.abs(w1).T + np.abs(b1))
    dh1 = dz1 + TAU
    dz2 = dh1 @ np.abs(w2).T + 66 * u * f * (np.abs(w2).sum(1) + np.abs(b2))
    return dz2 + TAU, (dz1, dz2)


def _head_bound(lin, dh2, f):
    w, b = _np64(lin.weight), _np64(lin.bias)
    return dh2 @ np.abs(w).T + 66 * U32 * f * (np.abs(w).sum(1) + np.abs(b))


def reference(pol, obs):
    """(mean [n][act], value [n]) of the policy in float64 on the fp32 obs."""
    import torch

    with torch.no_grad():
        mean, value = policy64(pol)(torch.from_numpy(np.asarray(obs, np.float32).astype(np.float64)))
    return mean.numpy(), value.numpy()


def forward_bound(pol, obs, precision):
    """(mean64 [n][act], value64 [n], dmean [n][act], dvalue [n]) for "fp32" or "fp16x3"."""
    u, f = UNIT[precision]
    x = np.asarray(obs, np.float32).astype(np.float64)
    mean, value = reference(pol, obs)
    dmean = _head_bound(pol.action_net, _tower_bound(pol.pi_net, x, u, f)[0], f)
    dvalue = _head_bound(pol.value_net, _tower_bound(pol.vf_net, x, u, f)[0], f)[:, 0]
    return mean, value, dmean, dvalue


def stage_bound(pol, obs, precision):
    """The bound's own stages on the value tower: (z1, z2, dz1, dz2), the fp64 pre-activations
    [n][64] of the two hidden layers and the bounds forward_bound propagates for them."""
    import torch

    u, f = UNIT[precision]
    x = np.asarray(obs, np.float32).astype(np.float64)
    net = policy64(pol).vf_net
    with torch.no_grad():
        z1 = net[0](torch.from_numpy(x))
        z2 = net[2](torch.tanh(z1))
    dz1, dz2 = _tower_bound(pol.vf_net, x, u, f)[1]
    return z1.numpy(), z2.numpy(), dz1, dz2


def worst_ratio(got, ref, bound):
    """max err / bound; inf if an element of `got` is not finite (a NaN must never pass)."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


def _bf16(x):
    import torch

    return torch.as_tensor(x).float().to(torch.bfloat16).double()


def emulate_bf16(pol, obs):
    """(mean, value) float64 with the bf16 kernel's roundings (test_gpu_rollout._emulated_bf16 with
    everything that the kernel keeps in fp32 exact)."""
    import torch

    p = policy64(pol)
    x = _bf16(torch.from_numpy(np.asarray(obs, np.float32)))

    def tower(net):
        h1 = torch.tanh(x @ _bf16(net[0].weight).T + net[0].bias)
        return torch.tanh(_bf16(h1) @ _bf16(net[2].weight).T + net[2].bias)

    with torch.no_grad():
        return p.action_net(tower(p.pi_net)).numpy(), p.value_net(tower(p.vf_net)).squeeze(-1).numpy()


def check_bf16_close(got, ref, tag):
    """The suite's bf16 bar (test_gpu_rollout._check_close): max < 1e-2 and q99 < 1e-4."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), tag
    err = np.abs(got - ref).ravel()
    q99 = float(np.quantile(err, 0.99))
    print(tag, "max err %.3e q99 %.3e" % (err.max(), q99))
    assert err.max() < 1e-2 and q99 < 1e-4, (tag, err.max(), q99)
    return float(err.max()), q99


# ---- the split-fp16 path, rounding by rounding ----------------------------------------------
f32 = np.float32
F16_MAX = 65504.0


def _split(w):
    """fp16 halves of the fp32 array w (already at the 2^8 operand scale), as float32 arrays."""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = w.astype(np.float16).astype(f32)
        lo = (w - hi).astype(np.float16).astype(f32)
    return hi, lo


def _mfma3(acc, a, b, drop_lo_hi):
    """acc [n][64] += b [n][K] . a [64][K] as the kernel's k steps of 16: per step lo_A hi_B, hi_A
    lo_B, hi_A hi_B, each product exact in fp32 (11 x 11 bits) and each sum rounded to fp32 in turn
    (at least as many roundings as the MFMA's own accumulation)."""
    (ahi, alo), (bhi, blo) = a, b
    k_all = ahi.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, k_all, 16):
            for wa, xb in ((alo, bhi), (ahi, blo), (ahi, bhi)):
                if drop_lo_hi and wa is alo:
                    continue
                for k in range(k0, min(k0 + 16, k_all)):
                    acc = (acc + xb[:, k:k + 1] * wa[None, :, k]).astype(f32)
    return acc


def _tanh_scaled(acc, out):
    """tanh_tile_scaled: out (1 - 2 / (1 + 2^(acc 2^-16 2 log2 e))) in fp32 steps (exp2 and the
    reciprocal correctly rounded here; the hardware's are within 1 ulp)."""
    c = f32(f32(2.88539008177792681) * f32(2.0 ** -16))
    with np.errstate(over="ignore"):
        y = (acc * c).astype(f32)
        d = (np.exp2(y.astype(np.float64)).astype(f32) + f32(1.0)).astype(f32)
        r = (1.0 / d.astype(np.float64)).astype(f32)
    return (out - (2.0 * out) * r.astype(np.float64)).astype(f32)  # one fma


def emulate_fp16x3(pol, obs, drop_lo_hi=False, saturate=True, stages=None):
    """(mean, value) float32 of the fp16x3 path: operands fp16(v 2^8) hi and lo, three products per
    k step accumulated in fp32 at the 2^16 scale (biases packed at 2^16), the scaled fp32 tanh, fp32
    heads. saturate: the obs operand clamped to +-65504 before the split (f16_operand).
    drop_lo_hi: the lo_A hi_B product left out of both layers (the sabotage of the sensitivity
    check). stages: a dict that receives the value tower's pre-activations z1, z2 (float64, the
    accumulators times 2^-16)."""
    x = (np.asarray(obs, f32) * f32(256.0)).astype(f32)
    if saturate:
        x = np.clip(x, -F16_MAX, F16_MAX)

    def t32(t):
        return t.detach().cpu().float().numpy()

    def tower(net, keep=None):
        w1, b1, w2, b2 = (t32(t) for t in (net[0].weight, net[0].bias, net[2].weight, net[2].bias))
        acc = np.broadcast_to((b1 * f32(65536.0)).astype(f32), (x.shape[0], 64))
        acc1 = _mfma3(acc, _split((w1 * f32(256.0)).astype(f32)), _split(x), drop_lo_hi)
        h1 = _tanh_scaled(acc1, 256.0)
        acc = np.broadcast_to((b2 * f32(65536.0)).astype(f32), (x.shape[0], 64))
        acc2 = _mfma3(acc, _split((w2 * f32(256.0)).astype(f32)), _split(h1), drop_lo_hi)
        if keep is not None:
            keep["z1"], keep["z2"] = acc1.astype(np.float64) / 65536.0, acc2.astype(np.float64) / 65536.0
        return _tanh_scaled(acc2, 1.0)

    def head(lin, h2):
        w, b = t32(lin.weight), t32(lin.bias)
        s = np.zeros((h2.shape[0], w.shape[0]), f32)
        for k in range(64):  # an fp32 fma chain
            s = (s.astype(np.float64) + h2[:, k:k + 1].astype(np.float64) * w[None, :, k]).astype(f32)
        return (s + b).astype(f32)

    return head(pol.action_net, tower(pol.pi_net)), head(pol.value_net, tower(pol.vf_net, stages))[:, 0]
