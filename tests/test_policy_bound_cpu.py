"""tests/policy_bound.py checked with references alone (no GPU): the forward error bound that
tests/test_gpu_policy_edges.py holds the policy kernels to is sound for two independent fp32-level
forwards on every case of that file (2 sizes x 4 weight sets x 7 obs classes of 257 rows), and it
notices a dropped product term of the split-fp16 path."""
import numpy as np
import pytest

import policy_bound as B

_cache = {}


def _case(ns, na, ws, oc):
    """(policy, obs, fp16x3 emulation outputs and stages) of one case, computed once."""
    key = (ns, ws, oc)
    if key not in _cache:
        if (ns, ws) not in _cache:
            _cache[ns, ws] = B.weight_set(ws, ns, na)
        pol = _cache[ns, ws]
        obs = B.obs_class(oc, ns)
        st = {}
        mean, value = B.emulate_fp16x3(pol, obs, stages=st)
        _cache[key] = (pol, obs, mean, value, st)
    return _cache[key]


@pytest.mark.parametrize("ns,na", B.SIZES)
def test_bound_holds_for_torch_fp32(ns, na):
    """Soundness, fp32: PyTorch's fp32 CPU forward (unfolded tanh, its own summation order) stays
    inside the u = 2^-24, f = 3 bound on every case.
    Largest err / bound: 4.4e-4 at (14, 3), 4.7e-4 at (7, 2)."""
    import torch

    worst = 0.0
    for ws in B.WEIGHT_SETS:
        for oc in B.OBS_CLASSES:
            pol, obs = _case(ns, na, ws, oc)[:2]
            mean, value, dmean, dvalue = B.forward_bound(pol, obs, "fp32")
            with torch.no_grad():
                m32, v32 = pol(torch.from_numpy(obs))
            r = max(B.worst_ratio(m32.numpy(), mean, dmean), B.worst_ratio(v32.numpy(), value, dvalue))
            print("fp32 (%d,%d) %-9s %-11s err/bound %.2e" % (ns, na, ws, oc, r))
            assert r <= 1.0, (ws, oc, r)
            worst = max(worst, r)
    print("fp32 (%d,%d) largest err/bound %.2e" % (ns, na, worst))


@pytest.mark.parametrize("ns,na", B.SIZES)
def test_bound_holds_for_split_fp16_emulation(ns, na):
    """Soundness, fp16x3: the NumPy restatement of the split path (fp16(v 2^8) hi and lo operands,
    three products per k step summed in fp32 one by one, biases at 2^16, fp32 tanh and heads) stays
    inside the u = 2^-21 bound on every case, at the outputs and at the bound's own stages (the
    value tower's pre-activations against dz1, dz2).
    Largest err / bound: outputs 1.3e-3 at (14, 3) and 1.4e-3 at (7, 2) (both on the 'constant'
    weights, one fp32 rounding of a +-60 value against the |w| ~ 30 head's 66 u rowsum |w|; 2e-4 on the
    other weight sets); stages z1 4.7e-2 / 7.7e-2, z2 3.2e-3 / 4.3e-3."""
    worst = {"out": 0.0, "z1": 0.0, "z2": 0.0}
    for ws in B.WEIGHT_SETS:
        for oc in B.OBS_CLASSES:
            pol, obs, m16, v16, st = _case(ns, na, ws, oc)
            mean, value, dmean, dvalue = B.forward_bound(pol, obs, "fp16x3")
            z1, z2, dz1, dz2 = B.stage_bound(pol, obs, "fp16x3")
            r = {"out": max(B.worst_ratio(m16, mean, dmean), B.worst_ratio(v16, value, dvalue)),
                 "z1": B.worst_ratio(st["z1"], z1, dz1), "z2": B.worst_ratio(st["z2"], z2, dz2)}
            print("fp16x3 (%d,%d) %-9s %-11s err/bound out %.2e z1 %.2e z2 %.2e" % (ns, na, ws, oc, r["out"], r["z1"],
                                                                                   r["z2"]))
            for k, v in r.items():
                assert v <= 1.0, (ws, oc, k, v)
                worst[k] = max(worst[k], v)
    print("fp16x3 (%d,%d) largest err/bound" % (ns, na), worst)


@pytest.mark.parametrize("ns,na", B.SIZES)
def test_bound_notices_a_dropped_split_term(ns, na):
    """Sensitivity: the same emulation without the lo_A hi_B products (the weights' low halves: a
    relative error of up to 2^-12 per product) breaks the bound on every weight set that has tower
    products, on each of the classes randn, randn8, uniform90 and f16_edge: the layer-1
    pre-activations leave dz1 by a factor of 35 - 110 (measured; the true emulation is at 0.08).

    Where it shows. The violation is at the bound's pre-activation stage, not at the outputs: there
    the sabotaged emulation reaches 0.25 of the bound at most (randn, 7 obs). The output bound
    carries the input-independent floor |Wh| 66 u rowsum |W2| (every rounding of all 64 x 64
    products with one sign, ~1.2e-2 here), while the dropped halves have random signs, sum like
    sqrt(64) and pass through tanh' < 1; reaching that floor needs 64 hidden activations aligned
    with the signs of one row's low halves, which a 7- or 14-component obs cannot produce for the
    64 rows at once. So the outputs alone cannot expose this term with these weights; the stage
    check does. tests/test_gpu_policy_edges.py reports the kernels' err / bound: they sit at 1e-4 to
    1.5e-3 of the output bound, two orders below where a kernel without the term would.

    'constant' has zero tower weights: no lo_A exists and the sabotaged emulation is bitwise the
    true one; asserted as such."""
    for ws in B.WEIGHT_SETS:
        pol = _case(ns, na, ws, "randn")[0]
        for oc in ("randn", "randn8", "uniform90", "f16_edge"):
            _, obs, m16, v16, st = _case(ns, na, ws, oc)
            sb = {}
            ms, vs = B.emulate_fp16x3(pol, obs, drop_lo_hi=True, stages=sb)
            if ws == "constant":
                assert np.array_equal(ms, m16) and np.array_equal(vs, v16)
                continue
            mean, value, dmean, dvalue = B.forward_bound(pol, obs, "fp16x3")
            z1, _, dz1, _ = B.stage_bound(pol, obs, "fp16x3")
            r1 = B.worst_ratio(sb["z1"], z1, dz1)
            rout = max(B.worst_ratio(ms, mean, dmean), B.worst_ratio(vs, value, dvalue))
            print("sabotaged fp16x3 (%d,%d) %-9s %-9s err/bound z1 %.1f out %.3f" % (ns, na, ws, oc, r1, rout))
            assert r1 > 1.0, (ws, oc, r1)


def test_split_fp16_emulation_saturates_like_the_kernel():
    """The restated path past the operand range: without the clamp of f16_operand a component at
    256 makes every output NaN (hi = inf, lo = -inf); with it the row is the row at 255.875."""
    pol = B.weight_set("suite", 7, 2)
    obs = B.beyond_obs(7, 16)
    with np.errstate(all="ignore"):
        m_raw, v_raw = B.emulate_fp16x3(pol, obs, saturate=False)
    assert np.isnan(m_raw).all() and np.isnan(v_raw).all()
    m, v = B.emulate_fp16x3(pol, obs)
    mc, vc = B.emulate_fp16x3(pol, np.clip(obs, -B.F16_OBS_MAX, B.F16_OBS_MAX))
    assert np.isfinite(m).all() and np.isfinite(v).all()
    assert np.array_equal(m, mc) and np.array_equal(v, vc)
