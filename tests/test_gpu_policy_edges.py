"""The policy forward, bootstrap and GAE kernels (rr_policy_act, rr_policy_bootstrap, rr_gae:
rl_rocket_amd/csrc/rocket_policy.inc) at the edges of their domain, against float64 references
(tests/policy_bound.py, tests/rollout_ref.py). tests/test_gpu_rollout.py holds them to a flat 2e-5 at
one input scale and one size; here

a. every row of 2 sizes x 4 weight sets x 7 obs classes (zeros, signed zeros, 1e-30 / subnormal,
   N(0, 1), 8 N(0, 1), uniform +-90, one component at +-255.875) stays inside the worst-case
   forward bound of policy_bound.forward_bound (fp32, fp16x3) or the suite's emulated-rounding bar
   (bf16): value, action mean (the sample at log_std = -30), the bootstrap's value_out and reward_out
   (bound x gamma) and log_prob (the fp64 log-density of the stored action);
b. obs components past the fp16 operand range (+-256 .. +-1e6): fp32 and bf16 as in (a); fp16x3
   finite and bitwise the call with the obs clamped to +-255.875;
c. a row's outputs do not depend on its position in the wave or on its neighbours (zeros, large,
   NaN / inf rows), bitwise;
d. n = 1 .. 257: nothing outside rows < n of any output is written, rows < n are bitwise those of the
   n = 257 call;
e. obs / obs_copy off 16-B alignment (stage_obs's element-wise path on full waves): same bits;
f. truncation patterns of the bootstrap, stand-alone and fused into rr_policy_act: same bits,
   untruncated rows return their reward bit for bit whatever the terminal row holds;
g. rr_gae at T around its 16-step chunk and n around a wave against rollout_ref.gae64, 1 fp32 ulp.

Measured (MI355X): in each test's docstring. The whole file runs in 4 s."""
import copy
import math

import numpy as np
import pytest

import policy_bound as B
import rollout_ref as R

pytestmark = pytest.mark.gpu

PREC = {"fp32": 0, "bf16": 1, "fp16x3": 2}
CASES = [(ns, na, prec) for ns, na in B.SIZES for prec in PREC]
N = B.N_ROWS
PAD = 64            # rows of sentinel before and after every output (64 rows keep 16-B alignment)
SENT = -12345.678
GAMMA = 0.99
U32 = B.U32
_packs, _refs = {}, {}


def _dev():
    import torch

    return torch.device("cuda:0")


def _pack(ns, na, ws, prec):
    """(CPU policy, packed params with log_std = -30, packed params as they are), built once."""
    import torch
    from rl_rocket_amd.rollout import PolicyPack

    key = (ns, ws, prec)
    if key not in _packs:
        pol = B.weight_set(ws, ns, na)
        packs = []
        for mean_only in (True, False):
            p = copy.deepcopy(pol).to(_dev())
            if mean_only:
                with torch.no_grad():
                    p.log_std.fill_(-30.0)
            pk = PolicyPack(p, ns, na, _dev(), precision=prec)
            pk.pack()
            packs.append(pk)
        torch.cuda.synchronize()
        _packs[key] = (pol, packs[0], packs[1])
    pol, a, b = _packs[key]
    return pol, a.buf, b.buf


def _bound(ns, na, ws, tag, obs, prec):
    """policy_bound.forward_bound of a named obs batch, computed once per unit roundoff."""
    key = (ns, ws, tag, prec)
    if key not in _refs:
        _refs[key] = B.forward_bound(B.weight_set(ws, ns, na), obs, prec)
    return _refs[key]


def _padded(n, cols):
    """(whole, rows): a [PAD + n + PAD][cols] buffer of the sentinel and its rows PAD .. PAD + n."""
    import torch

    shape = (n + 2 * PAD,) + ((cols,) if cols else ())
    whole = torch.full(shape, SENT, dtype=torch.float32, device=_dev())
    return whole, whole[PAD:PAD + n]


def _pads_untouched(whole, n):
    import torch

    ref = torch.full_like(whole[:PAD], SENT)
    return torch.equal(whole[:PAD].view(torch.int32), ref.view(torch.int32)) and \
        torch.equal(whole[PAD + n:].view(torch.int32), ref.view(torch.int32))


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _act(params, ns, na, prec, n, obs, ocopy=False, boot=None, done=None, obs_copy_view=None):
    """rr_policy_act on rows < n of `obs` into sentinel-padded outputs. boot = (term_obs, truncated,
    reward): the fused bootstrap; done: the start flags. Returns {name: (whole, rows)}."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr

    out = {"act_env": _padded(n, na), "act": _padded(n, na), "value": _padded(n, 0), "logp": _padded(n, 0)}
    if ocopy:
        out["obs_copy"] = _padded(n, ns)
    if obs_copy_view is not None:
        out["obs_copy"] = (obs_copy_view, obs_copy_view)
    if boot is not None:
        out["reward_out"] = _padded(n, 0)
    if done is not None:
        out["start_out"] = _padded(n, 0)
    it = torch.tensor([5], dtype=torch.int64, device=_dev())
    g = lambda k: _ptr(out[k][1]) if k in out else None  # noqa: E731
    tobs, trunc, rew = boot if boot is not None else (None, None, None)
    _lib.check(_lib.load().rr_policy_act(
        _ptr(params), ns, na, PREC[prec], n, 0, _ptr(obs), 123, _ptr(it), 3, g("act_env"), g("act"), g("value"), g("logp"),
        g("obs_copy"), _ptr(tobs), _ptr(trunc), _ptr(rew), GAMMA, g("reward_out"), _ptr(done), g("start_out"), None),
        "rr_policy_act")
    torch.cuda.synchronize()
    return out


def _bootstrap(params, ns, na, prec, n, tobs=None, trunc=None, rew=None, obs=None):
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr

    out = {}
    if tobs is not None:
        out["reward_out"] = _padded(n, 0)
    if obs is not None:
        out["value_out"] = _padded(n, 0)
    g = lambda k: _ptr(out[k][1]) if k in out else None  # noqa: E731
    _lib.check(_lib.load().rr_policy_bootstrap(_ptr(params), ns, na, PREC[prec], n, _ptr(tobs), _ptr(trunc), _ptr(rew),
                                               GAMMA, g("reward_out"), _ptr(obs), g("value_out"), None),
               "rr_policy_bootstrap")
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _cuda(x, dtype=None):
    import torch

    return torch.as_tensor(x, dtype=dtype).to(_dev()).contiguous()


def _logp_check(pol, act, logp, mean64, dmean):
    """err / bar of log_prob as the float64 log-density of the stored action. The kernel forms
    lp = sum(-eps^2 / 2 - log_std - log(2 pi) / 2) from its own fp32 draw eps and stores
    act = fl(mean + fl(std) eps); eps is recovered as (act - mean64) / std, off by at most
    d = (dmean + u |act|) / std + 4 u |eps| (the mean's bound, act's rounding, std through a 1 ulp
    exp2 of a rounded argument), which moves a term by |eps| d + d^2 / 2; the fp32 evaluation of the
    sum adds at most 8 u of the terms' magnitudes."""
    ls = pol.log_std.detach().double().numpy()
    std = np.exp(ls)
    eps = (act - mean64) / std
    lp64 = (-0.5 * eps ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(-1)
    d = (dmean + U32 * np.abs(act)) / std + 4 * U32 * np.abs(eps)
    bar = (np.abs(eps) * d + 0.5 * d * d).sum(-1) + 8 * U32 * (0.5 * eps ** 2 + np.abs(ls) + 0.919).sum(-1)
    return B.worst_ratio(logp, lp64, bar), eps


@pytest.mark.parametrize("ns,na,prec", CASES)
def test_forward_stays_inside_the_fp64_bound(ns, na, prec):
    """(a) Every row of every weight set x obs class against float64. fp32 / fp16x3: err <= the
    forward bound for value, mean, value_out, reward_out (x gamma; untruncated rows bitwise their
    reward) and the log_prob bar of _logp_check; bf16: the emulated-rounding bar (max < 1e-2, q99 <
    1e-4; log_prob max < 5e-2, q99 < 1e-3 as tests/test_gpu_rollout.py). Prints the largest
    err / bound per (weight set, obs class).

    Measured (MI355X), largest err / bound over the obs classes and both sizes, as value / mean /
    reward_out / log_prob:
      fp32    suite 6.1e-4 / 1.3e-3 / 5.6e-4 / 7.3e-4    scaled    6.1e-4 / 1.2e-3 / 5.6e-4 / 6.6e-3
              saturated 2.4e-4 / 2.1e-4 / 2.2e-4 / 1.6e-4  constant 1.5e-3 / 1.5e-3 / 1.5e-3 / 6.3e-3
      fp16x3  suite 9.3e-5 / 1.4e-4 / 7.0e-5 / 1.5e-4    scaled    9.3e-5 / 1.4e-4 / 7.0e-5 / 2.9e-3
              saturated 2.6e-5 / 4.3e-5 / 2.2e-5 / 2.1e-5  constant 8.8e-4 / 1.5e-3 / 8.9e-4 / 7.2e-3
    By obs class at the suite weights (value / mean): fp32 zeros, signed zeros and tiny 3.7e-4 /
    6.5e-4, N(0, 1) 6.1e-4 / 1.3e-3, 8 N(0, 1) 4.2e-4 / 7.6e-4, +-90 1.5e-4 / 2.3e-4, +-255.875
    1.0e-4 / 1.7e-4; fp16x3 1.1e-5 / 6.6e-5, 9.3e-5 / 1.4e-4, 5.3e-5 / 7.1e-5, 3.2e-5 / 5.8e-5, 7.3e-6 /
    8.7e-6. The errors themselves at the suite weights, max |kernel - fp64| (value / mean): fp32
    2.7e-6 / 4.8e-6 at N(0, 1) and 3.2e-6 / 8.0e-6 at +-90; fp16x3 1.3e-6 / 1.5e-6 and 5.3e-6 / 9.9e-6;
    at the saturated weights and +-90 fp32 3.5e-5 / 1.5e-4, fp16x3 1.2e-4 / 1.4e-4. The worst-case
    bound is three orders above the kernels (tests/test_policy_bound_cpu.py: a split path that lost
    one of its three products would sit near 0.2 here, still inside).
    bf16 against its emulation: max err 3.8e-3 (value, +-90), q99 <= 1.8e-5 in every case."""
    import torch

    rng = np.random.default_rng(7)
    trunc_np = (np.arange(N) % 3 == 0)
    trunc, rew_np = _cuda(trunc_np.astype(np.uint8)), rng.standard_normal(N).astype(np.float32)
    rew = _cuda(rew_np)
    for ws in B.WEIGHT_SETS:
        pol, p30, preal = _pack(ns, na, ws, prec)
        for oc in B.OBS_CLASSES:
            obs_np = B.obs_class(oc, ns)
            obs = _cuda(obs_np)
            o30 = _act(p30, ns, na, prec, N, obs)
            orl = _act(preal, ns, na, prec, N, obs)
            bo = _bootstrap(preal, ns, na, prec, N, tobs=obs, trunc=trunc, rew=rew, obs=obs)
            value, mean, act, logp = _np(o30["value"][1]), _np(o30["act"][1]), _np(orl["act"][1]), _np(orl["logp"][1])
            vout, rout = _np(bo["value_out"][1]), _np(bo["reward_out"][1])
            assert torch.equal(o30["value"][1], orl["value"][1]) and torch.equal(o30["value"][1], bo["value_out"][1])
            assert np.array_equal(_bits(bo["reward_out"][1])[~trunc_np], rew_np.view(np.int32)[~trunc_np])
            tag = "%s (%d,%d) %-9s %-11s" % (prec, ns, na, ws, oc)
            if prec == "bf16":
                m_e, v_e = B.emulate_bf16(pol, obs_np)
                B.check_bf16_close(value, v_e, tag + " value")
                B.check_bf16_close(mean, m_e, tag + " mean")
                B.check_bf16_close(rout, rew_np.astype(np.float64) + GAMMA * v_e * trunc_np, tag + " reward_out")
                _, eps = _logp_check(pol, act, logp, m_e, 0.0)
                ls = pol.log_std.detach().double().numpy()
                lp_err = np.abs(logp - (-0.5 * eps ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(-1))
                print(tag, "log_prob max err %.3e q99 %.3e" % (lp_err.max(), np.quantile(lp_err, 0.99)))
                assert lp_err.max() < 5e-2 and np.quantile(lp_err, 0.99) < 1e-3, tag
                continue
            m64, v64, dm, dv = _bound(ns, na, ws, oc, obs_np, prec)
            r = {"value": B.worst_ratio(value, v64, dv), "mean": B.worst_ratio(mean, m64, dm),
                 "reward_out": B.worst_ratio(rout[trunc_np], (rew_np + GAMMA * v64)[trunc_np], GAMMA * dv[trunc_np]),
                 "log_prob": _logp_check(pol, act, logp, m64, dm)[0]}
            print(tag, "err/bound " + " ".join("%s %.2e" % kv for kv in r.items()),
                  "| max |err| value %.2e mean %.2e" % (np.abs(value - v64).max(), np.abs(mean - m64).max()))
            for k, v in r.items():
                assert v <= 1.0, (tag, k, v)


@pytest.mark.parametrize("ns,na,prec", CASES)
def test_obs_beyond_the_fp16_operand_range(ns, na, prec):
    """(b) Rows with one component at +-256, +-300, +-1e4, +-1e6, every weight set. fp32: inside the
    bound (which a NaN or inf never is); bf16: the emulated-rounding bar; fp16x3: every output finite
    and bitwise that of the same rows clamped to +-255.875 (rr_policy_act and rr_policy_bootstrap):
    before the operand was saturated, every output of such a row was NaN.

    Measured (MI355X), largest err / bound: fp32 1.5e-3 (constant weights), 1.1e-4 on the other
    weight sets; fp16x3 against fp64 at the clamped obs 1.5e-3 (constant), 9.9e-6 elsewhere; bf16
    max err 1.8e-5."""
    import torch

    obs_np = B.beyond_obs(ns)
    obs = _cuda(obs_np)
    trunc = _cuda((np.arange(N) % 2 == 0).astype(np.uint8))
    rew = _cuda(np.linspace(-3, 3, N).astype(np.float32))
    for ws in B.WEIGHT_SETS:
        pol, p30, preal = _pack(ns, na, ws, prec)
        o30 = _act(p30, ns, na, prec, N, obs)
        tag = "%s (%d,%d) %-9s beyond" % (prec, ns, na, ws)
        value, mean = _np(o30["value"][1]), _np(o30["act"][1])
        assert np.isfinite(value).all() and np.isfinite(mean).all(), tag
        if prec == "fp32":
            m64, v64, dm, dv = _bound(ns, na, ws, "beyond", obs_np, prec)
            r = (B.worst_ratio(value, v64, dv), B.worst_ratio(mean, m64, dm))
            print(tag, "err/bound value %.2e mean %.2e" % r)
            assert max(r) <= 1.0, (tag, r)
        elif prec == "bf16":
            m_e, v_e = B.emulate_bf16(pol, obs_np)
            B.check_bf16_close(value, v_e, tag + " value")
            B.check_bf16_close(mean, m_e, tag + " mean")
        else:
            clamped = _cuda(np.clip(obs_np, -B.F16_OBS_MAX, B.F16_OBS_MAX))
            for params in (p30, preal):
                a = _act(params, ns, na, prec, N, obs)
                b = _act(params, ns, na, prec, N, clamped)
                for k in ("value", "act", "act_env", "logp"):
                    assert torch.isfinite(a[k][1]).all(), (tag, k)
                    assert np.array_equal(_bits(a[k][1]), _bits(b[k][1])), (tag, k)
            a = _bootstrap(preal, ns, na, prec, N, tobs=obs, trunc=trunc, rew=rew, obs=obs)
            b = _bootstrap(preal, ns, na, prec, N, tobs=clamped, trunc=trunc, rew=rew, obs=clamped)
            for k in ("reward_out", "value_out"):
                assert torch.isfinite(a[k][1]).all(), (tag, k)
                assert np.array_equal(_bits(a[k][1]), _bits(b[k][1])), (tag, k)
            m64, v64, dm, dv = _bound(ns, na, ws, "beyond_clamped", np.clip(obs_np, -B.F16_OBS_MAX, B.F16_OBS_MAX), prec)
            r = (B.worst_ratio(value, v64, dv), B.worst_ratio(mean, m64, dm))
            print(tag, "bitwise the clamped rows; against fp64 at the clamped obs err/bound value %.2e mean %.2e" % r)
            assert max(r) <= 1.0, (tag, r)


def _probe_row(ns, na, pol):
    """An N(0, 1) obs row whose fp64 means are all above 1e-4 in magnitude, so that the sample at
    log_std = -30 (mean + 9.4e-14 eps, |eps| < 6) is the fp32 mean itself whatever the row's draw."""
    rng = np.random.default_rng(50 + ns)
    for _ in range(100):
        row = rng.standard_normal((1, ns)).astype(np.float32)
        if np.abs(B.reference(pol, row)[0]).min() > 1e-4:
            return row[0]
    raise AssertionError("no probe row")


@pytest.mark.parametrize("ns,na,prec", CASES)
def test_row_outputs_do_not_depend_on_position_or_neighbours(ns, na, prec):
    """(c) One obs row at rows 0, 31, 32 and 256 of a 257-row batch whose other rows are zeros,
    8 N(0, 1), or hold NaN / +inf / -inf: its value, mean (the sample at log_std = -30) and the
    bootstrap's value_out have the same bits in all twelve places. The rows that hold a NaN give NaN
    value and means in fp32. fp16x3 saturates its operand with v_med3_f32, which returns the smallest
    operand when one is NaN: a NaN component reads as -255.875 and +-inf as +-255.875, pinned here
    as the whole batch being bitwise the batch with those substitutions."""
    import torch

    where = [0, 31, 32, 256]
    for ws in ("suite", "saturated"):
        pol, p30, _ = _pack(ns, na, ws, prec)
        probe = _probe_row(ns, na, pol)
        rng = np.random.default_rng(60 + ns)
        bad = rng.standard_normal((N, ns)).astype(np.float32)
        r = np.arange(N)
        bad[r, r % ns] = np.asarray([np.nan, np.inf, -np.inf], np.float32)[r % 3]
        bad[r[r % 5 == 4], (r[r % 5 == 4] + 3) % ns] = np.nan  # some rows hold a NaN and an inf
        has_nan = np.isnan(bad).any(1)
        batches = {"zeros": np.zeros((N, ns), np.float32), "randn8": (8 * rng.standard_normal((N, ns))).astype(np.float32),
                   "nonfinite": bad}
        got = {}
        for name, x in batches.items():
            x = x.copy()
            x[where] = probe
            obs = _cuda(x)
            o = _act(p30, ns, na, prec, N, obs)
            vo = _bootstrap(p30, ns, na, prec, N, obs=obs)["value_out"][1]
            assert torch.equal(o["value"][1].view(torch.int32), vo.view(torch.int32)), name
            got[name] = (_bits(o["value"][1]), _bits(o["act"][1]), x)
        v0, m0 = got["zeros"][0][0], got["zeros"][1][0]
        assert np.isfinite(v0.view(np.float32)) and np.isfinite(m0.view(np.float32)).all()
        for name, (vb, mb, _) in got.items():
            for w in where:
                assert vb[w] == v0 and np.array_equal(mb[w], m0), (ws, name, w)
        vb, mb, x = got["nonfinite"]
        rows = has_nan.copy()
        rows[where] = False
        assert rows.sum() > 60
        if prec == "fp32":
            assert np.isnan(vb.view(np.float32)[rows]).all() and np.isnan(mb.view(np.float32)[rows]).all()
        if prec == "fp16x3":
            sub = np.where(np.isnan(x), np.float32(-B.F16_OBS_MAX), np.clip(x, -B.F16_OBS_MAX, B.F16_OBS_MAX))
            o = _act(p30, ns, na, prec, N, _cuda(sub.astype(np.float32)))
            assert np.isfinite(vb.view(np.float32)).all() and np.isfinite(mb.view(np.float32)).all()
            assert np.array_equal(_bits(o["value"][1]), vb) and np.array_equal(_bits(o["act"][1]), mb)


def _edge_inputs(ns, seed=3):
    """Inputs of N rows inside allocations padded by PAD finite rows on both sides."""
    import torch

    g = torch.Generator().manual_seed(seed + ns)
    tot = N + 2 * PAD
    obs = (2 * torch.randn((tot, ns), generator=g)).to(_dev())
    tobs = torch.randn((tot, ns), generator=g).to(_dev())
    trunc = (torch.rand((tot,), generator=g) < 0.3).to(torch.uint8).to(_dev())
    done = (torch.rand((tot,), generator=g) < 0.3).to(torch.uint8).to(_dev())
    rew = torch.randn((tot,), generator=g).to(_dev())
    return tuple(t[PAD:PAD + N] for t in (obs, tobs, trunc, rew, done))


OUTS = ("act_env", "act", "value", "logp", "obs_copy", "reward_out", "start_out")


@pytest.mark.parametrize("ns,na,prec", CASES)
def test_shape_edges_write_nothing_outside_their_rows(ns, na, prec):
    """(d) n = 1, 31, 32, 33, 255, 256, 257 (below a wave's 32 envs, around it, around a workgroup's
    256): rr_policy_act with every optional output and rr_policy_bootstrap write into allocations
    with 64 sentinel rows before and after; the sentinels keep their bits, and rows < n have the bits
    of the n = 257 call (inputs sit inside padded allocations too)."""
    import torch

    _, _, params = _pack(ns, na, "suite", prec)
    obs, tobs, trunc, rew, done = _edge_inputs(ns)
    full = _act(params, ns, na, prec, N, obs, ocopy=True, boot=(tobs, trunc, rew), done=done)
    fullb = _bootstrap(params, ns, na, prec, N, tobs=tobs, trunc=trunc, rew=rew, obs=obs)
    assert torch.equal(full["obs_copy"][1], obs) and torch.equal(full["start_out"][1], done.float())
    assert torch.equal(full["act_env"][1], full["act"][1].clamp(-1, 1))
    assert torch.equal(full["reward_out"][1].view(torch.int32), fullb["reward_out"][1].view(torch.int32))
    assert torch.equal(full["value"][1].view(torch.int32), fullb["value_out"][1].view(torch.int32))
    for k in OUTS:
        assert torch.isfinite(full[k][1]).all(), k
    for n in (1, 31, 32, 33, 255, 256, 257):
        o = _act(params, ns, na, prec, n, obs, ocopy=True, boot=(tobs, trunc, rew), done=done)
        ob = _bootstrap(params, ns, na, prec, n, tobs=tobs, trunc=trunc, rew=rew, obs=obs)
        for name, res, ref in [(k, o, full) for k in OUTS] + [("reward_out", ob, fullb), ("value_out", ob, fullb)]:
            whole, rows = res[name]
            assert _pads_untouched(whole, n), (n, name)
            assert np.array_equal(_bits(rows), _bits(ref[name][1][:n])), (n, name)


@pytest.mark.parametrize("ns,na,prec", CASES)
def test_unaligned_obs_pointers_give_the_same_bits(ns, na, prec):
    """(e) obs, then obs_copy, then the bootstrap's term_obs / obs start 4 bytes past a 16-B boundary,
    n = 257 and 256 (eight full waves: stage_obs leaves its 16-B path for the element-wise one): every
    output has the bits of the aligned call, and the sentinels around the unaligned obs_copy hold."""
    import torch

    _, _, params = _pack(ns, na, "suite", prec)
    obs, tobs, trunc, rew, done = _edge_inputs(ns, seed=4)

    def off4(t):
        flat = torch.full((t.numel() + 8,), SENT, device=_dev())
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return flat, v

    for n in (257, 256):
        ref = _act(params, ns, na, prec, n, obs, ocopy=True, boot=(tobs, trunc, rew), done=done)
        refb = _bootstrap(params, ns, na, prec, n, tobs=tobs, trunc=trunc, rew=rew, obs=obs)
        assert obs.data_ptr() % 16 == 0 and ref["obs_copy"][1].data_ptr() % 16 == 0
        _, obs_u = off4(obs[:n])
        a = _act(params, ns, na, prec, n, obs_u, ocopy=True, boot=(tobs, trunc, rew), done=done)
        flat, oc_u = off4(torch.full((n, ns), SENT, device=_dev()))
        b = _act(params, ns, na, prec, n, obs, boot=(tobs, trunc, rew), done=done, obs_copy_view=oc_u)
        assert flat[0].item() == np.float32(SENT) and bool((flat[1 + n * ns:] == np.float32(SENT)).all())
        for res in (a, b):
            for k in OUTS:
                assert np.array_equal(_bits(res[k][1]), _bits(ref[k][1])), (n, k)
        _, tobs_u = off4(tobs[:n])
        c = _bootstrap(params, ns, na, prec, n, tobs=tobs_u, trunc=trunc, rew=rew, obs=obs_u)
        for k in ("reward_out", "value_out"):
            assert np.array_equal(_bits(c[k][1]), _bits(refb[k][1])), (n, k)


@pytest.mark.parametrize("ns,na,prec", CASES)
def test_bootstrap_truncation_patterns(ns, na, prec):
    """(f) n = 300 (nine full waves and one of 12 envs), truncated all 0, all 1, only env 0, only
    env n - 1, every third env: rr_policy_bootstrap and the bootstrap fused into rr_policy_act give
    the same bits; untruncated rows return their reward bit for bit although their terminal rows are
    NaN; truncated rows are r + gamma V64(terminal obs) within gamma x the forward bound (fp32,
    fp16x3).

    Measured (MI355X), largest err / bound on truncated rows: fp32 7.7e-4, fp16x3 9.4e-5; bf16
    against its emulation max err 2.1e-3."""
    import torch

    n = 300
    pol, _, params = _pack(ns, na, "scaled", prec)
    rng = np.random.default_rng(80 + ns)
    tobs_np = rng.standard_normal((n, ns)).astype(np.float32)
    rew_np = (3 * rng.standard_normal(n)).astype(np.float32)
    obs, rew = _cuda(rng.standard_normal((n, ns)).astype(np.float32)), _cuda(rew_np)
    patterns = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": np.arange(n) == 0,
                "last": np.arange(n) == n - 1, "third": np.arange(n) % 3 == 1}
    if prec != "bf16":
        _, v64, _, dv = _bound(ns, na, "scaled", "terminal", tobs_np, prec)
    for name, tr in patterns.items():
        t_np = tobs_np.copy()
        t_np[~tr] = np.nan
        tobs, trunc = _cuda(t_np), _cuda(tr.astype(np.uint8))
        alone = _bootstrap(params, ns, na, prec, n, tobs=tobs, trunc=trunc, rew=rew)
        fused = _act(params, ns, na, prec, n, obs, boot=(tobs, trunc, rew))
        for res in (alone, fused):
            assert _pads_untouched(res["reward_out"][0], n), name
        a, b = _bits(alone["reward_out"][1]), _bits(fused["reward_out"][1])
        assert np.array_equal(a, b), name
        assert np.array_equal(a[~tr], rew_np.view(np.int32)[~tr]), name
        out = _np(alone["reward_out"][1])
        assert np.isfinite(out).all(), name
        if prec != "bf16" and tr.any():
            r = B.worst_ratio(out[tr], (rew_np + GAMMA * v64)[tr], GAMMA * dv[tr])
            print("%s (%d,%d) truncated %-5s reward_out err/bound %.2e" % (prec, ns, na, name, r))
            assert r <= 1.0, (name, r)
        elif tr.any():
            v_e = B.emulate_bf16(pol, tobs_np)[1]
            B.check_bf16_close(out[tr], (rew_np + GAMMA * v_e)[tr], "bf16 (%d,%d) truncated %s" % (ns, na, name))


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 33])
def test_gae_matches_fp64_to_one_ulp(T, n):
    """(g) rr_gae against rollout_ref.gae64: T below, at and past the scan's 16-step chunk (33 = two
    chunks and one step), n below and past a wave; rewards N(0, 1) with +-60 spikes on 5 %, values
    uniform +-150; starts all 0, all 1 and random, last_done all 0, all 1 and random; outputs with
    sentinel rows around them. The device scan runs in fp64 and rounds each stored value once, so
    every advantage and return is within 1 fp32 ulp of the fp64 reference (a derived bar: the two
    fp64 evaluations differ by ~1e-13, which moves a value across an fp32 rounding boundary at most
    to the neighbouring float).

    Measured (MI355X): 757 184 of the 757 188 stored values are the rounded fp64 reference itself
    (99.9995 %); the other four are its neighbouring float."""
    import torch
    from rl_rocket_amd import _lib
    from rl_rocket_amd.batch import _ptr

    rng = np.random.default_rng(1000 * T + n)
    exact = total = 0
    for starts_mode in ("zeros", "ones", "random"):
        for done_mode in ("zeros", "ones", "random"):
            r = rng.standard_normal((T, n))
            spike = rng.random((T, n)) < 0.05
            r[spike] = np.where(rng.random(int(spike.sum())) < 0.5, -60.0, 60.0) + r[spike]
            v = rng.uniform(-150, 150, (T, n))
            flag = {"zeros": lambda s: np.zeros(s), "ones": lambda s: np.ones(s),
                    "random": lambda s: (rng.random(s) < 0.3).astype(np.float64)}
            s, ld = flag[starts_mode]((T, n)), flag[done_mode]((n,))
            lv = rng.uniform(-150, 150, n)
            r, v, s, lv, ld = (x.astype(np.float32) for x in (r, v, s, lv, ld))
            adv_w, adv = _padded(T * n, 0)
            ret_w, ret = _padded(T * n, 0)
            d = [_cuda(x) for x in (r, v, s, lv, ld)]
            _lib.check(_lib.load().rr_gae(T, n, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), _ptr(d[4]), 0.99, 0.95,
                                          _ptr(adv), _ptr(ret), None), "rr_gae")
            torch.cuda.synchronize()
            assert _pads_untouched(adv_w, T * n) and _pads_untouched(ret_w, T * n)
            a64, r64 = R.gae64(r, v, s, lv, ld, 0.99, 0.95)
            for got, ref in ((adv, a64), (ret, r64)):
                got = got.cpu().numpy().reshape(T, n)
                ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
                err = np.abs(got.astype(np.float64) - ref)
                assert (err <= ulp).all(), (starts_mode, done_mode, float((err / ulp).max()))
                exact += int((got == ref.astype(np.float32)).sum())
                total += got.size
    print("rr_gae T=%d n=%d: %d of %d values are the rounded fp64 reference (%.4f %%)" % (T, n, exact, total,
                                                                                        100.0 * exact / total))

