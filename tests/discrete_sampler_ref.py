"""Inputs of the Categorical sampler's and act kernel's edge tests (tests only; no kernels here, and nothing that
calls one): tests/test_discrete_sampler_inputs.py checks every condition on the CPU,
tests/test_gpu_discrete_sampler.py feeds the same inputs to rr_policy_act_discrete, rr_rollout_step_discrete,
rr_rollout_collect_discrete and rr_policy_evaluate_discrete_sampled. Every draw comes from a CPU generator.

* ``const_policy``: an ``MlpCategoricalActorCritic(7, K, table)`` whose ``action_net.weight`` is zero and whose
  ``action_net.bias`` holds the given logits. The packed head weights are -2 W = -0 and the packed head bias is
  fl(b + rowsum(W)) = fl(b + 0) = b (rr_policy_pack_discrete; policy.PolicyPack.pack_reference), so the kernel's
  logit is (a sum of +-0 products) + b = b: every row's logits are exactly the fp32 biases whatever the obs. (The
  GPU test launches on two different obs batches and requires equal bits.) The towers keep discrete_ref.cat_policy's
  perturbed weights, so the value still depends on the obs.
* ``ACT_DRAWS`` / ``COLLECT_DRAWS``: where the uniform draw u = r 2^-24, r = mix32(key) >> 8, takes a chosen 24-bit
  value: rows (id_off, t, r) at discrete_ref's ACT_SEED, ACT_ITER, ACT_T for the act and per-step kernels, and rows
  (seed, env, t, r) of a 64-env, 8-step call at iter 0 for the one-launch collect and the sampled evaluation. The
  values are the ends r = 0, 2^24 - 1, 2^24 - 2, 2^24 - 3 and the ties 2^22, 2^23, 3 2^22 (u = 0.25, 0.5, 0.75).
  ``search_id_offsets`` / ``search_seeds`` found them once, offline (2^27 ids in ~15 s, 400 000 seeds in ~40 s);
  the literals below are their first 4 rows per end value and 2 per tie value.
* ``sampler32``: the kernels' sampler text in numpy float32, the running sum of ex / sum compared with <=, with an
  optional +-1 ulp nudge on the ex values that are neither 0 nor 1 (the device's expf). guard=False is the text
  before the dead-choice guard, guard=True the present one (a step past choice q counts only if some ex beyond q is
  positive). It chooses inputs and proves that they discriminate; it is never a reference for the GPU.
* ``SHORTFALL``: logit sets with dead choices (a bias of -120: ex = 0 in fp32, p ~ e^-120 in float64) on which the
  unguarded text draws a dead choice at r = 2^24 - 1 under all three nudges: the fp32 running sum over the live
  choices stops short of 1 - 2^-24. ``find_shortfall`` found the x values on a 0.05 grid.
* ``live_ref``: the float64 inverse-CDF index (discrete_ref.act_ref's rule) over the probabilities with the dead
  ones (below DEAD = 1e-30) set to exactly 0. It is discrete_ref.act_ref's index on every committed draw but
  one kind: a dead LEADING choice at r = 0, where u = 0 lies inside float64's [0, e^-120) and act_ref names the
  dead choice itself; the kernels' documented rule (c_0 = 0 <= u: the boundary goes to the next choice) skips it.
* ``cat_weight_set`` / ``EDGE_OBS`` / ``logp_bar`` / ``knife_mask``: the act kernel's domain-edge cases, built like
  policy_bound.weight_set on the Categorical class, with the bars of tests/test_gpu_discrete_sampler.py part b.
"""
import numpy as np
import torch

import discrete_ref as D
import policy_bound as B
import rollout_ref as R

f32 = np.float32
R_TOP = 2 ** 24 - 1
R_ENDS = (0, R_TOP, R_TOP - 1, R_TOP - 2)
R_TIES = (2 ** 22, 2 ** 23, 3 * 2 ** 22)
R_WANTED = R_ENDS + R_TIES
N_ENVS, N_STEPS = 64, 8   # the collect's and the evaluation's call
DEAD = 1e-30
DEAD_LOGIT = -120.0


# ---- constant-logit policies ------------------------------------------------------------------------------------
def const_policy(logits, device="cpu"):
    k = len(logits)
    pol = D.cat_policy(k, 300 + k)
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.copy_(torch.tensor(logits, dtype=torch.float32))
    return pol.to(device)


# ---- extreme draws ----------------------------------------------------------------------------------------------
def _bits(e, s, it, t):
    """r = mix32(key) >> 8 for env ids e (uint64 array) under the mixed seed s (int, or uint64 arrays that
    broadcast against e), rollout_ref.noise_key's three stages."""
    lo, hi = (np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)) if isinstance(s, int) else s
    key = R.mix32((e & R.M32) ^ lo)
    key = R.mix32(key ^ R._u(it) ^ hi)
    key = R.mix32(key ^ R._u(int(it) >> 32) ^ (np.asarray(t, np.uint64) * np.uint64(0x9E3779B9) & R.M32))
    return R.mix32(key) >> np.uint64(8)


def _keep(rows, col):
    """The first 4 rows per end value and 2 per tie value, in R_WANTED's order."""
    out = []
    for r in R_WANTED:
        out += [x for x in rows if x[col] == r][:4 if r in R_ENDS else 2]
    return tuple(out)


def search_id_offsets(limit=2 ** 27, chunk=2 ** 22):
    """(id_off, t, r) of every env id below `limit` whose draw at (ACT_SEED, ACT_ITER, ACT_T) is in R_WANTED."""
    s, rows = R.splitmix64(D.ACT_SEED), []
    want = np.array(R_WANTED, np.uint64)
    for e0 in range(0, limit, chunk):
        e = np.arange(e0, e0 + chunk, dtype=np.uint64)
        r = _bits(e, s, D.ACT_ITER, D.ACT_T)
        for i in np.nonzero(np.isin(r, want))[0]:
            rows.append((int(e[i]), D.ACT_T, int(r[i])))
    return _keep(rows, 2)


def search_seeds(limit=400000, chunk=4096):
    """(seed, env, t, r) of every draw in R_WANTED of a N_ENVS x N_STEPS call at iter 0, id_off 0, seeds < limit."""
    rows = []
    want = np.array(R_WANTED, np.uint64)
    e = np.arange(N_ENVS, dtype=np.uint64)[None, :, None]
    t = np.arange(N_STEPS, dtype=np.uint64)[None, None, :]
    for s0 in range(0, limit, chunk):
        mixed = [R.splitmix64(s) for s in range(s0, s0 + chunk)]
        lo = np.array([m & 0xFFFFFFFF for m in mixed], np.uint64)[:, None, None]
        hi = np.array([m >> 32 for m in mixed], np.uint64)[:, None, None]
        r = _bits(e, (lo, hi), 0, t)
        for i, j, k in zip(*np.nonzero(np.isin(r, want))):
            rows.append((s0 + int(i), int(j), int(k), int(r[i, j, k])))
    return _keep(rows, 3)


# (id_off, t, r)
ACT_DRAWS = (
    (38134933, 5, 0), (47476682, 5, 0), (50907929, 5, 0), (62402570, 5, 0),
    (29785947, 5, 16777215), (34346289, 5, 16777215), (35163036, 5, 16777215), (58255919, 5, 16777215),
    (2942730, 5, 16777214), (53371611, 5, 16777214), (100627947, 5, 16777214), (104234343, 5, 16777214),
    (6291383, 5, 16777213), (45806519, 5, 16777213), (48497198, 5, 16777213), (49424961, 5, 16777213),
    (1723504, 5, 4194304), (4982467, 5, 4194304), (67014831, 5, 8388608), (82347964, 5, 8388608),
    (13142818, 5, 12582912), (57438034, 5, 12582912),
)
# (seed, env, t, r)
COLLECT_DRAWS = (
    (57692, 1, 4, 0), (122741, 31, 5, 0), (151826, 58, 4, 0), (187742, 48, 5, 0),
    (12301, 43, 7, 16777215), (28292, 19, 1, 16777215), (37146, 38, 4, 16777215), (44595, 53, 5, 16777215),
    (32812, 0, 0, 16777214), (62905, 39, 5, 16777214), (79394, 29, 4, 16777214), (133918, 43, 2, 16777214),
    (20626, 46, 6, 16777213), (23251, 11, 3, 16777213), (35737, 19, 1, 16777213), (55254, 56, 1, 16777213),
    (8750, 60, 1, 4194304), (46091, 33, 4, 4194304), (16753, 41, 0, 8388608), (31207, 13, 4, 8388608),
    (526, 10, 2, 12582912), (118446, 37, 3, 12582912),
)


def act_u(n, id_off, t=D.ACT_T):
    return D.uniform_ref(n, id_off, D.ACT_SEED, D.ACT_ITER, t)


def collect_u(seed):
    """[N_STEPS][N_ENVS] float64: the draws of the call under `seed`."""
    return np.stack([D.uniform_ref(N_ENVS, 0, seed, 0, t) for t in range(N_STEPS)])


# ---- the sampler text in float32 ----------------------------------------------------------------------------------
def sampler32(logits, u, nudge=0, guard=True):
    """index [n] of the kernels' text on logits [n][K] (or [K]: one set for every row) and u [n]."""
    u = np.asarray(u, np.float64).astype(f32)
    z = np.broadcast_to(np.asarray(logits, f32), (len(u), np.shape(logits)[-1]))
    k = z.shape[1]
    with np.errstate(under="ignore"):
        ex = np.exp((z - z.max(1, keepdims=True)).astype(f32)).astype(f32)
    if nudge:
        m = (ex != 0) & (ex != 1)
        ex[m] = np.nextafter(ex[m], f32(np.inf * nudge))
    total = np.zeros(len(u), f32)
    for q in range(k):
        total = (total + ex[:, q]).astype(f32)
    c, index = np.zeros(len(u), f32), np.zeros(len(u), np.int64)
    for q in range(k - 1):
        c = (c + (ex[:, q] / total).astype(f32)).astype(f32)
        step = c <= u
        if guard:
            step &= (ex[:, q + 1:] > 0).any(1)
        index += step
    return index


# ---- float64 ----------------------------------------------------------------------------------------------------
def probs64(logits):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def live_ref(logits, u):
    """index [n]: the number of k in 0 .. K - 2 with p_0 + .. + p_k <= u, the dead p_k exactly 0."""
    p = np.broadcast_to(probs64(logits), (len(u), np.shape(logits)[-1]))
    p = np.where(p < DEAD, 0.0, p)
    c = np.cumsum(p, axis=1)[:, :-1]
    return (c <= np.asarray(u)[:, None]).sum(1)


def act_ref_index(logits, u):
    """discrete_ref.act_ref's index on constant logits."""
    lp = np.log(np.broadcast_to(probs64(logits), (len(u), np.shape(logits)[-1])))
    return D.act_ref(lp, np.asarray(u))[0]


# ---- the cases --------------------------------------------------------------------------------------------------
X = DEAD_LOGIT
LIVE_ENDS = {4: (0.0, -0.5, 0.25, -1.0), 3: (0.5, 0.0, -0.75), 2: (0.0, -0.375)}  # every choice live
TIES = {2: (0.0, 0.0), 4: (1.5, 1.5, 1.5, 1.5)}   # running sums k / K, exact in fp32 and float64
TIES_DEAD = ((0.0, X, 0.0, X), (X, 0.0, X, 0.0), (X, 0.0, 0.0, X))  # running sums 0, 0.5, 1 around dead choices
EQUAL3 = (0.25, 0.25, 0.25)
KNIFE3 = 2.0 ** -22
KNIFE3_ROWS = 4
N_BITS = 65536

SHORTFALL_SHAPES = {
    "two_tails": lambda x: (0.0, -x, X, X),
    "one_tail": lambda x: (0.0, -x, -1.0, X),
    "k3_tail": lambda x: (0.0, -x, X),
    "middle": lambda x: (0.0, X, -x, X),
    "leading": lambda x: (X, 0.0, -x, X),
}


def draws_dead(logits, r=R_TOP, guard=False):
    """True if the float32 text draws a dead choice at u = r 2^-24 under all three nudges."""
    u = np.array([r * 2.0 ** -24])
    dead = probs64(logits) < DEAD
    return all(dead[sampler32(logits, u, nudge, guard)[0]] for nudge in (-1, 0, 1))


def find_shortfall(shape, grid=np.arange(0.5, 6.0001, 0.05)):
    return tuple(round(float(x), 2) for x in grid if draws_dead(SHORTFALL_SHAPES[shape](round(float(x), 2))))


# the x of find_shortfall that are used (it returns 1.8, 3.15, 3.25, 3.55, 3.8, 4.4, 4.65, 4.7, 4.75, 5.3 for every
# shape but one_tail, whose third live choice at -1 leaves 4.65 alone)
SHORTFALL_X = {"two_tails": (1.8, 3.55, 4.7), "one_tail": (4.65,), "k3_tail": (3.15, 5.3), "middle": (3.25, 4.4),
               "leading": (3.8, 4.75)}
SHORTFALL = tuple((shape, SHORTFALL_SHAPES[shape](x)) for shape, xs in SHORTFALL_X.items() for x in xs)


# ---- the act kernel's domain edges (part b) ------------------------------------------------------------------------
WEIGHT_SETS = ("suite", "saturated", "constant")
EDGE_OBS = ("zero", "signed_zero", "tiny", "randn", "randn8", "uniform90")
EDGE_K = (4, 2)
PEAKED = ((80.0, 0.0, -80.0, -120.0), (-60.0, -60.5, -61.0, -61.5), (80.0, 80.0, 80.0, 80.0), (-80.0, -80.0, -80.0, -80.0))
EDGE_N = B.N_ROWS
EDGE_ID_OFF = 1000


def cat_weight_set(name, k):
    """policy_bound.weight_set's suite / saturated / constant on an MlpCategoricalActorCritic(7, k)."""
    if name not in WEIGHT_SETS:
        raise ValueError(name)
    pol = D.cat_policy(k, 47, head_scale=1.0)
    g = torch.Generator().manual_seed(48)
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


def logp_bar(z64, dz, index):
    """Per row: 2 max_k dz_k + 2^-24 (2 |z_a - z_max| + 2 |lse| + 12), lse = log sum exp(z - z_max): one rounding
    each on z - z_max, on exp's argument, on the sum and its log, and on the last subtraction, over the logits'
    own bound (d(z_a - lse) <= 2 max |dz|)."""
    zm = z64.max(1)
    lse = np.log(np.exp(z64 - zm[:, None]).sum(1))
    za = z64[np.arange(len(index)), index]
    return 2 * dz.max(1) + B.U32 * (2 * np.abs(za - zm) + 2 * np.abs(lse) + 12)


def knife_mask(lp64, dz, u):
    """Rows where u is within max(discrete_ref.KNIFE, 2 max_k dz_k) of a float64 running sum (a running sum moves
    by at most 2 max |dz| when every logit moves by dz: d p_k <= 2 p_k max |dz|, and the p_k sum to at most 1)."""
    c = np.cumsum(np.exp(lp64), axis=1)[:, :-1]
    width = np.maximum(D.KNIFE, 2 * dz.max(1))
    return (np.abs(u[:, None] - c) < width[:, None]).any(1)


EDGE_CASES = tuple((k, ws, oc) for k in EDGE_K for ws in WEIGHT_SETS for oc in EDGE_OBS)
# The index of a case is compared with float64 only where knife_mask flags at most discrete_ref.KNIFE_CAP (1 %) of
# the 257 rows. forward_bound is a worst-case bound, three orders above the kernels' error, so 2 max dz is 8e-3 at
# the suite weights and above 0.06 at the saturated ones, and the rule admits: every obs class at the constant
# weights (1 row of 257 at K = 4 and at K = 2), and zero, signed_zero and tiny at the suite weights with K = 2
# (2 rows). Not admitted, and so compared on value and log-prob only: suite x randn, randn8, uniform90 at K = 2
# (1.2 %, 1.9 %, 5.8 %), suite x every class at K = 4 (4.7 % .. 15.6 %), saturated x every class at both K
# (11 % .. 100 %). (tests/test_discrete_sampler_inputs.py asserts that this literal is what the rule gives.)
INDEX_ADMITTED = frozenset((k, "constant", oc) for k in EDGE_K for oc in EDGE_OBS) | frozenset(
    (2, "suite", oc) for oc in ("zero", "signed_zero", "tiny"))
_edge = {}


def edge_case(k, ws, oc):
    """One (K, weight set, obs class) case on the CPU, cached and read-only: pol, obs [257][7] fp32, the float64
    logits, values and log-softmax, forward_bound's dz [257][K] and dv [257], the draws u, the knife-edge mask
    and the float64 index."""
    import types

    key = (k, ws, oc)
    if key not in _edge:
        pol = cat_weight_set(ws, k)
        obs = B.obs_class(oc, 7)
        z64, v64, dz, dv = B.forward_bound(pol, obs, "fp32")
        lp64 = D.forward64(pol, obs)[2]
        u = act_u(EDGE_N, EDGE_ID_OFF)
        _edge[key] = types.SimpleNamespace(k=k, ws=ws, oc=oc, pol=pol, obs=obs, z64=z64, v64=v64, dz=dz, dv=dv, lp64=lp64,
                                           u=u, knife=knife_mask(lp64, dz, u), ref=D.act_ref(lp64, u)[0])
    return _edge[key]
