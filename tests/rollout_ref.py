"""Plain fp64 references for the on-device PPO rollout (tests only; no kernels here).

* ``noise_ref``: the documented action-noise key (include/rocket_hip.h, rr_policy_act) restated in
  NumPy uint64 arithmetic masked to 32 bits, the Box-Muller draw in float64.
* ``policy64``: a float64 copy of an ``MlpActorCritic``.
* ``replay_collect``: every row of a collected rollout restarted from the collect's own
  ``obs[t]`` and stepped by the CPU oracle (fp64 scipy-RK45 restatement), so that what the rollout
  stores next to ``obs[t]`` -- next obs, reward with the timeout bootstrap, episode-start flags,
  values, log-probs, actions, GAE -- is compared with an independent computation.
* ``CpuRollout``: the same collect computed on the CPU from these references (oracle step, fp64
  policy, ``noise_ref``), the replay's own check: a faithful collect replays clean and a mis-wired
  one does not (tests/test_rollout_replay_cpu.py)."""
import copy
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
M64 = (1 << 64) - 1
GAE_REL_BAR = 96 * 2.0 ** -24


def _u(x):
    return np.uint64(int(x) & 0xFFFFFFFF)


def splitmix64(x):
    """One splitmix64 step on a Python int (the host-side seed mix of rr_seed and the noise key)."""
    z = (int(x) + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix32(x):
    """lowbias32 on uint64 arrays holding 32-bit values."""
    x = x.astype(np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def noise_key(n, id_off, seed, it, t, mix_seed=True):
    """The three-stage 32-bit key of env id_off + e (e < n) at rollout `it`, step `t`.
    mix_seed=False: the key without the host-side seed mix (the keying before it existed)."""
    s = splitmix64(seed) if mix_seed else int(seed) & M64
    e = (np.arange(n, dtype=np.uint64) + np.uint64(int(id_off) & M64)) & M32  # (uint32_t)(id_off + e)
    key = mix32(e ^ _u(s))
    key = mix32(key ^ _u(it) ^ _u(s >> 32))
    return mix32(key ^ _u(int(it) >> 32) ^ _u(int(t) * 0x9E3779B9))


def noise_ref(n, id_off, seed, it, t, act_dim, mix_seed=True):
    """float64 [n, act_dim]: the standard-normal draws of envs id_off .. id_off + n - 1."""
    key = noise_key(n, id_off, seed, it, t, mix_seed)
    out = np.empty((n, act_dim))
    for a in range(0, act_dim, 2):
        k = (key + _u(a * 0x632BE5AB)) & M32
        h1, h2 = mix32(k), mix32(k ^ np.uint64(0x68E31DA4))
        u1 = ((h1 >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24  # (0, 1]
        u2 = (h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
        out[:, a] = r * np.cos(ang)
        if a + 1 < act_dim:
            out[:, a + 1] = r * np.sin(ang)
    return out


def policy64(pol):
    """A float64 CPU deep copy of an MlpActorCritic."""
    return copy.deepcopy(pol).double().cpu()


def scaled_policy(ns, na, seed, head_scale=0.05, device="cpu"):
    """The suite's perturbed policy (test_gpu_rollout._policy: SB3 init + 0.3 N(0, 1) on every
    parameter, so every weight matters) with the action head scaled so the means stay O(0.1) and
    episodes last long enough to end in every way."""
    import torch
    from rl_rocket_amd.rollout import MlpActorCritic

    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    pol = MlpActorCritic(ns, na)
    with torch.no_grad():
        for prm in pol.parameters():
            prm.add_(0.3 * torch.randn(prm.shape, generator=gen))
        pol.action_net.weight.mul_(head_scale)
        pol.action_net.bias.mul_(head_scale)
    return pol.to(device)


def snapshot(ro):
    """Host copies of a DeviceRollout's last collect (float32 as stored) + the post-step obs."""
    import torch

    torch.cuda.synchronize()
    out = {k: getattr(ro, k).detach().cpu().numpy().copy() for k in (
        "obs", "actions", "rewards", "starts", "values", "log_probs", "advantages", "returns", "last_value",
        "last_done")}
    out["next_obs"] = ro.env.obs.detach().cpu().numpy().copy()
    return out


def new_carry(n, ns):
    """Per env: the running episode's initial condition (float32) and its elapsed steps."""
    return {"ic": np.zeros((n, ns), np.float32), "elapsed": np.zeros(n, np.int64)}


def gae64(rewards, values, starts, last_value, last_done, gamma, lam):
    """SB3 RolloutBuffer.compute_returns_and_advantage in float64."""
    r, v, s = (np.asarray(x, np.float64) for x in (rewards, values, starts))
    T = r.shape[0]
    adv, last = np.empty_like(r), np.zeros(r.shape[1])
    for t in reversed(range(T)):
        nt = 1.0 - (np.asarray(last_done, np.float64) if t == T - 1 else s[t + 1])
        nv = np.asarray(last_value, np.float64) if t == T - 1 else v[t + 1]
        last = r[t] + gamma * nv * nt - v[t] + gamma * lam * nt * last
        adv[t] = last
    return adv, adv + v


def _obs_err(model, got, ref):
    """floored_rel(got, ref, 1.0) per row; 3DOF obs[2] = theta / 2 pi compared on the circle."""
    e = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    if model == 3:
        d = np.abs(got[:, 2] - ref[:, 2])
        e[:, 2] = np.minimum(d, np.abs(1.0 - d))
    return e.max(1)


def replay_collect(oracle_mod, cfg, ro, carry, pol64, time_limit, gamma=0.99, lam=0.95, ic_low=None, ic_high=None,
                   noise=None, nthreads=8, probe_seed=0):
    """Replay one collect (`ro`: snapshot()) row by row through the oracle.

    Every row (t, e) restarts from obs[t, e] * normalizer in float64 and is stepped by
    oracle.step with clip(actions[t, e]), t_in = elapsed * dt and the carried episode ic. `carry`
    (new_carry) is rebuilt from the collect's own starts flags and updated in place for the next
    collect. `noise` = (id_off, seed, it) checks actions = mean64 + std * noise_ref, None skips it.

    Returns a dict: per-row errors [T, n] (obs, reward, reward_bar, value, logp, action, adv, ret,
    adv_rel, ret_rel),
    last_value error [n], the flag comparison (mismatch rows, how many of them are marginal), the
    reset-row check and the event counts."""
    import torch

    model = cfg.model
    ns = 14 if model == 6 else 7
    norm = np.array(cfg.normalizer[:ns])
    dt = cfg.dt
    obs = ro["obs"].astype(np.float64)
    T, n = obs.shape[:2]
    act = ro["actions"].astype(np.float64)
    a_env = np.clip(ro["actions"], -1.0, 1.0).astype(np.float32)
    starts = ro["starts"] != 0
    nxt_obs = np.concatenate([obs[1:], ro["next_obs"].astype(np.float64)[None]])
    nxt_start = np.concatenate([starts[1:], (ro["last_done"] != 0)[None]])

    # the episode's ic and elapsed steps of every row, from the collect's own flags
    ic = np.empty((T, n, ns), np.float32)
    el = np.empty((T, n), np.int64)
    for t in range(T):
        s = starts[t]
        carry["ic"][s] = (obs[t][s] * norm).astype(np.float32)
        carry["elapsed"][s] = 0
        ic[t], el[t] = carry["ic"], carry["elapsed"]
        carry["elapsed"] += 1
    s_in = (obs * norm).reshape(T * n, ns)
    o = oracle_mod.step(cfg, ic.reshape(T * n, ns), (el * dt).reshape(-1), s_in, a_env.reshape(T * n, -1),
                        nthreads=nthreads)
    done = o["done"].reshape(T, n)
    trunc = ~done & (el + 1 == time_limit)
    end = done | trunc
    o_obs = (o["state_out"] / norm).reshape(T, n, ns)
    mism = end != nxt_start
    ok = ~mism

    # flags that differ: marginal if one of 8 re-steps perturbed by <= 1e-6 relative gives the GPU's
    rows = np.argwhere(mism)
    marginal = 0
    rng = np.random.default_rng(probe_seed)
    for t, e in rows:
        k = 8
        sp = np.tile(obs[t, e] * norm, (k, 1)) * (1.0 + 1e-6 * rng.uniform(-1, 1, (k, ns)))
        ap = np.clip(np.tile(a_env[t, e].astype(np.float64), (k, 1)) * (1.0 + 1e-6 * rng.uniform(-1, 1, (k, a_env.shape[2]))),
                     -1.0, 1.0).astype(np.float32)
        o2 = oracle_mod.step(cfg, np.tile(ic[t, e], (k, 1)), np.full(k, el[t, e] * dt), sp, ap)
        end2 = o2["done"] | (~o2["done"] & (el[t, e] + 1 == time_limit))
        marginal += bool((end2 == nxt_start[t, e]).any())

    res = {"rows": T * n, "mismatch_rows": rows, "marginal": marginal,
           "events": int((o["status"] == 1).sum()), "bounds": int(o["bounds_violation"].sum()),
           "natural": int(done.sum()), "truncated": int(trunc.sum())}

    # next obs on the rows that go on
    go = ok & ~end
    e_obs = np.zeros((T, n))
    e_obs[go] = _obs_err(model, nxt_obs[go], o_obs[go])
    res["obs"] = e_obs

    # reset rows: the new episode's state inside the init space. The fp32 state s lies in
    # [ic_low, ic_high] up to one rounding of fma(span, u, low); obs = fl(s * fl(1 / norm)) adds two
    # roundings, so obs * norm is within 3 * 2^-24 |s| of it: slack 2.5e-7 max(|low|, |high|)
    res["reset_bad"] = 0
    if ic_low is not None:
        st = nxt_obs[nxt_start] * norm
        lo, hi = np.asarray(ic_low, np.float64), np.asarray(ic_high, np.float64)
        slack = 2.5e-7 * np.maximum(np.abs(lo), np.abs(hi))
        inside = (st >= lo - slack) & (st <= hi + slack)
        if model == 6:  # the drawn quaternion is normalised: unit within 1e-5 instead of inside the box
            inside[:, 6:10] = (np.abs(np.linalg.norm(st[:, 6:10], axis=1) - 1.0) <= 1e-5)[:, None]
        res["reset_bad"] = int((~inside.all(1)).sum())
        res["reset_rows"] = int(nxt_start.sum())

    # policy outputs in fp64
    with torch.no_grad():
        o_t = torch.from_numpy(obs.reshape(T * n, ns))
        mean64, v64 = (x.numpy().reshape(T, n, -1) for x in pol64(o_t))
        v64 = v64.reshape(T, n)
        lv64 = pol64.value(torch.from_numpy(ro["next_obs"].astype(np.float64))).numpy()
        log_std = pol64.log_std.numpy()
    std = np.exp(log_std)
    res["value"] = np.abs(ro["values"] - v64)
    res["last_value"] = np.abs(ro["last_value"] - lv64)
    lp64 = (-0.5 * ((act - mean64) / std) ** 2 - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    res["logp"] = np.abs(ro["log_probs"] - lp64)
    if noise is not None:
        id_off, seed, it = noise
        z = np.stack([noise_ref(n, id_off, seed, it, t, act.shape[2]) for t in range(T)])
        res["action"] = np.abs(act - (mean64 + std * z)).max(-1)

    # rewards: the oracle's reward + gamma V64(oracle terminal obs) on truncated rows and only those
    r_ref = o["reward"].reshape(T, n).copy()
    grad = 0.0
    if trunc.any():
        tob = torch.from_numpy(o_obs[trunc]).requires_grad_(True)
        vt = pol64.value(tob)
        g, = torch.autograd.grad(vt.sum(), tob)
        grad = float(g.abs().sum(1).max())  # G: how far an obs error within TOL_STATE can move V
        r_ref[trunc] += gamma * vt.detach().numpy()
    from gpu_util import TOL_REWARD, TOL_STATE

    bar = TOL_REWARD * np.maximum(np.abs(r_ref), 1.0) + trunc * gamma * (2e-5 + grad * TOL_STATE)
    e_rew = np.abs(ro["rewards"] - r_ref)
    e_rew[mism] = 0.0
    res["reward"], res["reward_bar"], res["G"] = e_rew, bar, grad
    res["reward_over"] = int((e_rew > bar).sum())
    # the bootstrap term on its own: rows the oracle ends naturally carry none (their |reward - r|
    # is inside the plain reward bar above); truncated rows carry one of the size gamma |V|
    res["trunc_mask"], res["done_mask"] = trunc & ok, done & ok

    adv64, ret64 = gae64(ro["rewards"], ro["values"], ro["starts"], ro["last_value"], ro["last_done"], gamma, lam)
    res["adv"] = np.abs(ro["advantages"] - adv64)
    res["ret"] = np.abs(ro["returns"] - ret64)
    # the same two errors over the env's own scale S = max(1, max_t |A| + |V| + |r|): one step of an
    # fp32 scan rounds at most six times (gamma V', + r, - V, gamma lambda A', the sum, A + V) at
    # magnitudes <= S and gamma lambda <= 1 does not amplify, so T = 16 steps stay within
    # GAE_REL_BAR = 96 * 2^-24 = 5.7e-6 of S (the bar holds for an fp32 scan; the fp64 scan of
    # gae_env sits at one rounding). Terminal rewards of +-60 make |A| reach ~170.
    scale = np.maximum(1.0, (np.abs(adv64) + np.abs(ro["values"]) + np.abs(ro["rewards"])).max(0))
    res["adv_rel"], res["ret_rel"] = res["adv"] / scale, res["ret"] / scale
    res["adv_abs_max"] = float(np.abs(adv64).max())
    return res


class CpuRollout:
    """DeviceRollout's collect computed on the CPU from the references of this module: fp64
    policy, noise_ref, the oracle's step on the float32-rounded state, uniform resets inside the
    init space, TimeLimit truncation, SB3's timeout bootstrap and GAE. `wiring` injects one of the
    errors a replay must notice: "bootstrap_natural" (bootstrap on natural ends too),
    "bootstrap_reset_obs" (V of the reset obs instead of the terminal obs), "starts_shifted"
    (starts[t] holds step t's done instead of step t-1's), "same_noise" (one draw for every t)."""

    def __init__(self, oracle_mod, cfg, pol64, n, n_steps, time_limit, ic_low, ic_high, seed=0, gamma=0.99,
                 lam=0.95, wiring=None):
        self.o, self.cfg, self.pol, self.n, self.T, self.tl = oracle_mod, cfg, pol64, n, n_steps, time_limit
        self.model = cfg.model
        self.ns = 14 if self.model == 6 else 7
        self.norm = np.array(cfg.normalizer[:self.ns])
        self.lo, self.hi = np.asarray(ic_low, np.float64), np.asarray(ic_high, np.float64)
        self.seed, self.gamma, self.lam, self.wiring = seed, gamma, lam, wiring
        self.rng = np.random.default_rng(seed)
        self.it = 0
        self.state = self._sample(n)
        self.ic = self.state.astype(np.float32)
        self.el = np.zeros(n, np.int64)
        self.start = np.ones(n, bool)

    def _sample(self, k):
        s = self.lo + (self.hi - self.lo) * self.rng.random((k, self.ns))
        if self.model == 6:
            s[:, 6:10] /= np.linalg.norm(s[:, 6:10], axis=1, keepdims=True)
        return s.astype(np.float32).astype(np.float64)

    def _obs(self, s):
        return (s / self.norm).astype(np.float32)

    def collect(self):
        import torch

        T, n, ns, pol = self.T, self.n, self.ns, self.pol
        na = pol.log_std.numel()
        f = np.float32
        ro = {"obs": np.zeros((T, n, ns), f), "actions": np.zeros((T, n, na), f)}
        for k in ("rewards", "starts", "values", "log_probs"):
            ro[k] = np.zeros((T, n), f)
        std = pol.log_std.detach().exp().numpy()
        for t in range(T):
            obs = self._obs(self.state)
            with torch.no_grad():
                mean, v = (x.numpy() for x in pol(torch.from_numpy(obs.astype(np.float64))))
            z = noise_ref(n, 0, self.seed, self.it, 0 if self.wiring == "same_noise" else t, na)
            a = (mean + std * z).astype(f)
            ro["obs"][t], ro["actions"][t], ro["values"][t] = obs, a, v
            ro["log_probs"][t] = (-0.5 * z ** 2 - np.log(std) - 0.5 * math.log(2 * math.pi)).sum(-1)
            ro["starts"][t] = self.start
            out = self.o.step(self.cfg, self.ic, self.el * self.cfg.dt, obs.astype(np.float64) * self.norm,
                              np.clip(a, -1, 1), nthreads=8)
            done = out["done"]
            trunc = ~done & (self.el + 1 == self.tl)
            end = done | trunc
            s1 = out["state_out"].astype(f).astype(np.float64)
            tobs = self._obs(s1)
            self.el += 1
            if end.any():
                s1[end] = self._sample(int(end.sum()))
                self.ic[end] = s1[end].astype(f)
                self.el[end] = 0
            boot = end if self.wiring == "bootstrap_natural" else trunc
            src = self._obs(s1) if self.wiring == "bootstrap_reset_obs" else tobs
            with torch.no_grad():
                vt = pol.value(torch.from_numpy(src.astype(np.float64))).numpy()
            ro["rewards"][t] = out["reward"] + np.where(boot, self.gamma * vt, 0.0)
            if self.wiring == "starts_shifted":
                ro["starts"][t] = end
            self.state, self.start = s1, end
        ro["next_obs"] = self._obs(self.state)
        with torch.no_grad():
            ro["last_value"] = pol.value(torch.from_numpy(ro["next_obs"].astype(np.float64))).numpy().astype(f)
        ro["last_done"] = self.start.astype(f)
        adv, ret = gae64(ro["rewards"], ro["values"], ro["starts"], ro["last_value"], ro["last_done"], self.gamma,
                         self.lam)
        ro["advantages"], ro["returns"] = adv.astype(f), ret.astype(f)
        self.it += 1
        return ro
