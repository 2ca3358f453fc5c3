"""The inputs of tests/test_gpu_discrete_sampler.py (tests/discrete_sampler_ref.py), checked on the CPU before any
of them reaches a kernel.

* Every committed (id_off, t, r) and (seed, env, t, r) reproduces its r through discrete_ref.uniform_ref, and the
  tables hold at least 4 rows per end value and 2 per tie value.
* Every shortfall case draws a dead choice under the float32 restatement of the unguarded sampler text at the top
  draw, under all three expf nudges; the guarded text and the float64 reference draw no dead choice at any
  committed draw. The float64 reference is discrete_ref.act_ref's index everywhere but on a dead leading choice
  at r = 0 (discrete_sampler_ref.live_ref's docstring), and those rows are counted here.
* Every row of every 64-row launch of the GPU file (the special row and its 63 neighbours) has the same index
  under the float64 reference and under the guarded float32 text with all three nudges: the GPU test needs no
  knife-edge exclusions on them.
* Equal logits at K = 2 and 4 have exactly representable running sums: float64 and float32 agree on every row of
  the 65 536-row case with no row left out, and both are floor(K u). At K = 3 at most KNIFE3_ROWS = 4 of the
  65 536 rows lie within 2^-22 of a running sum (2 x 2^-21 x 65 536 = 0.06 rows expected; counted: 0).
* The act kernel's edge cases: the knife-edge mask comes from the reference alone and INDEX_ADMITTED is exactly
  the set the 1 % rule admits; torch's fp32 log_softmax stays within half of the log-prob bar on every case."""
import numpy as np
import pytest
import torch

import discrete_ref as D
import discrete_sampler_ref as S
import policy_bound as B

LANES = (0, 31, 32, 63)
ALL_LOGITS = (tuple(S.LIVE_ENDS.values()) + tuple(z for _, z in S.SHORTFALL) + tuple(S.TIES.values()) + S.TIES_DEAD)


def test_committed_draws_reproduce_their_bits():
    for id_off, t, r in S.ACT_DRAWS:
        assert t == D.ACT_T
        assert D.uniform_ref(1, id_off, D.ACT_SEED, D.ACT_ITER, t)[0] == r * 2.0 ** -24, (id_off, r)
    for seed, env, t, r in S.COLLECT_DRAWS:
        assert 0 <= env < S.N_ENVS and 0 <= t < S.N_STEPS
        assert D.uniform_ref(S.N_ENVS, 0, seed, 0, t)[env] == r * 2.0 ** -24, (seed, env, t, r)
        assert S.collect_u(seed)[t, env] == r * 2.0 ** -24
    for table in (S.ACT_DRAWS, S.COLLECT_DRAWS):
        got = [row[-1] for row in table]
        assert all(got.count(r) >= 4 for r in S.R_ENDS) and all(got.count(r) >= 2 for r in S.R_TIES)
        assert set(got) == set(S.R_WANTED) and len(set(table)) == len(table)
    assert S.R_ENDS == (0, 2 ** 24 - 1, 2 ** 24 - 2, 2 ** 24 - 3) and S.R_TIES == (2 ** 22, 2 ** 23, 3 * 2 ** 22)


def test_search_finds_the_committed_rows():
    """The search functions on the slices that hold the first committed row of each table."""
    id_off, t, r = min(S.ACT_DRAWS)
    e0 = id_off - id_off % 2 ** 16
    e = np.arange(e0, e0 + 2 ** 16, dtype=np.uint64)
    bits = S._bits(e, S.R.splitmix64(D.ACT_SEED), D.ACT_ITER, D.ACT_T)
    assert np.array_equal(bits.astype(np.float64) * 2.0 ** -24, S.act_u(2 ** 16, e0)) and bits[id_off - e0] == r
    seed, env, t, r = min(S.COLLECT_DRAWS)
    found = S.search_seeds(limit=seed + 1, chunk=seed + 1)
    assert (seed, env, t, r) in found and all(row in S.COLLECT_DRAWS for row in found)


def test_shortfall_cases_discriminate():
    assert len(S.SHORTFALL) >= 6
    shapes = [s for s, _ in S.SHORTFALL]
    assert {"two_tails", "one_tail", "k3_tail", "middle", "leading"} == set(shapes)
    us = np.array([r * 2.0 ** -24 for r in S.R_WANTED])
    leading_at_zero = 0
    for shape, z in S.SHORTFALL:
        p = S.probs64(z)
        dead = p < S.DEAD
        assert dead.any() and p[~dead].min() > 1e-4 and p[dead].max() < 1e-50, z  # nothing near the line
        assert np.array_equal(np.asarray(z) == S.DEAD_LOGIT, dead)
        assert S.draws_dead(z), (shape, z)                      # the text before the guard, all three nudges
        ref, plain = S.live_ref(z, us), S.act_ref_index(z, us)
        assert not dead[ref].any(), z
        for nudge in (-1, 0, 1):
            assert np.array_equal(S.sampler32(z, us, nudge, guard=True), ref), (z, nudge)
        differ = ref != plain
        if shape == "leading":  # u = 0 lies in float64's [0, e^-120): act_ref names the dead choice, the rule skips it
            assert differ.tolist() == [r == 0 for r in S.R_WANTED] and plain[0] == 0 and ref[0] == 1
            leading_at_zero += 1
        else:
            assert not differ.any(), z
    assert leading_at_zero == 2
    # every row on which the unguarded text draws a live choice keeps its index under the guarded one
    u = S.act_u(S.N_BITS, 0)
    for _, z in S.SHORTFALL:
        a, b = S.sampler32(z, u, guard=False), S.sampler32(z, u, guard=True)
        live = ~(S.probs64(z) < S.DEAD)[a]
        assert np.array_equal(a[live], b[live]) and live.all()


def test_dead_choices_at_ties_and_at_zero():
    us = np.array([r * 2.0 ** -24 for r in S.R_WANTED])
    want = {(0.0, S.X, 0.0, S.X): [0, 2, 2, 2, 0, 2, 2], (S.X, 0.0, S.X, 0.0): [1, 3, 3, 3, 1, 3, 3],
            (S.X, 0.0, 0.0, S.X): [1, 2, 2, 2, 1, 2, 2]}
    assert set(want) == set(S.TIES_DEAD)
    for z, idx in want.items():
        assert S.live_ref(z, us).tolist() == idx, z
        for nudge in (-1, 0, 1):  # nothing to nudge: every ex is 0 or 1
            assert S.sampler32(z, us, nudge).tolist() == idx and S.sampler32(z, us, nudge, guard=False).tolist() == idx


def test_every_row_of_every_sampler_launch_has_one_answer():
    """The 64 rows of each act / per-step launch (the special row at lane LANES[i % 4]) and the 64 x 8 rows of
    each collect / evaluation call, for every logit set: float64 and the guarded float32 text under all three
    nudges agree, so the GPU test compares whole launches."""
    rows = 0
    for z in ALL_LOGITS:
        for i, (id_off, t, r) in enumerate(S.ACT_DRAWS):
            lane = LANES[i % 4]
            u = S.act_u(64, id_off - lane)
            assert u[lane] == r * 2.0 ** -24
            ref = S.live_ref(z, u)
            for nudge in (-1, 0, 1):
                assert np.array_equal(S.sampler32(z, u, nudge), ref), (z, id_off, nudge)
            rows += 64
        for seed, env, t, r in S.COLLECT_DRAWS:
            u = S.collect_u(seed).reshape(-1)
            ref = S.live_ref(z, u)
            for nudge in (-1, 0, 1):
                assert np.array_equal(S.sampler32(z, u, nudge), ref), (z, seed, nudge)
    lanes = {r: {LANES[i % 4] for i, row in enumerate(S.ACT_DRAWS) if row[2] == r} for r in S.R_ENDS}
    assert all(v == set(LANES) for v in lanes.values())  # every end value sits at every lane once
    print("%d logit sets, %d act rows each" % (len(ALL_LOGITS), rows // len(ALL_LOGITS)))


def test_ends_of_the_range_with_every_choice_live():
    for k, z in S.LIVE_ENDS.items():
        assert len(z) == k and S.probs64(z).min() > 0.05
        us = np.array([r * 2.0 ** -24 for r in S.R_ENDS])
        assert S.live_ref(z, us).tolist() == [0, k - 1, k - 1, k - 1]
        assert S.act_ref_index(z, us).tolist() == [0, k - 1, k - 1, k - 1]


@pytest.mark.parametrize("k", [2, 4])
def test_equal_logits_have_exact_running_sums(k):
    z = S.TIES[k]
    u = S.act_u(S.N_BITS, 0)
    want = np.floor(k * u).astype(np.int64)
    assert np.array_equal(S.live_ref(z, u), want) and np.array_equal(S.act_ref_index(z, u), want)
    for nudge in (-1, 0, 1):
        assert np.array_equal(S.sampler32(z, u, nudge), want)
    assert sorted(set(want.tolist())) == list(range(k))
    ties = np.array([r * 2.0 ** -24 for r in S.R_TIES])  # the boundary value goes to the next choice
    assert S.live_ref(z, ties).tolist() == np.floor(k * ties).tolist() == ([1, 2, 3] if k == 4 else [0, 1, 1])
    assert np.array_equal(S.sampler32(z, ties), S.live_ref(z, ties))
    # what the 65 536-row launch tells apart: a comparator turned round (c < u: the tie rows, here) fails nothing
    # on random rows, so the committed ties carry it; a u of 23 bits over half the range and a swapped key stage
    # fail thousands of rows; a u with only its last bit dropped, (x >> 9) 2^-23, changes no floor(K u) at all and
    # is within one ulp of u everywhere: no float64 reference can tell it from the kernel's own rounding
    assert (S.sampler32(z, np.floor(u * 2 ** 23) * 2.0 ** -23) != want).sum() == 0
    assert (S.sampler32(z, np.floor(u * 2 ** 23) * 2.0 ** -24) != want).sum() > 1000
    swapped = D.uniform_ref(S.N_BITS, 0, D.ACT_SEED, D.ACT_T, D.ACT_ITER)
    assert (np.floor(k * swapped) != want).sum() > 1000


def test_equal_logits_at_three_choices_knife_rows():
    u = S.act_u(S.N_BITS, 0)
    c = np.cumsum(S.probs64(S.EQUAL3))[:-1]
    knife = (np.abs(u[:, None] - c[None, :]) < S.KNIFE3).any(1)
    print("K = 3: %d knife rows of %d" % (knife.sum(), S.N_BITS))
    assert knife.sum() <= S.KNIFE3_ROWS
    ref = S.live_ref(S.EQUAL3, u)
    for nudge in (-1, 0, 1):
        got = S.sampler32(S.EQUAL3, u, nudge)
        assert np.array_equal(got[~knife], ref[~knife])
    assert sorted(set(ref.tolist())) == [0, 1, 2]


def test_edge_case_admission():
    admitted = set()
    for k, ws, oc in S.EDGE_CASES:
        c = S.edge_case(k, ws, oc)
        assert c.obs.shape == (S.EDGE_N, 7) and c.obs.dtype == np.float32 and c.dz.shape == (S.EDGE_N, k)
        assert np.isfinite(c.dz).all() and np.isfinite(c.dv).all() and (c.dz > 0).all()
        share = c.knife.mean()
        if share <= D.KNIFE_CAP:
            admitted.add((k, ws, oc))
        # the log-prob bar: torch's fp32 log_softmax of the fp32 module stays within half of it, on every index
        with torch.no_grad():
            lp32 = torch.log_softmax(c.pol(torch.from_numpy(c.obs))[0], -1).double().numpy()
        worst = 0.0
        for a in range(k):
            bar = S.logp_bar(c.z64, c.dz, np.full(S.EDGE_N, a))
            worst = max(worst, float((np.abs(lp32[:, a] - c.lp64[:, a]) / bar).max()))
        print("K %d %-9s %-11s knife %.4f max dz %.2e fp32 log_softmax / bar %.4f" % (k, ws, oc, share, c.dz.max(), worst))
        assert worst <= 0.5, (k, ws, oc, worst)
    assert admitted == set(S.INDEX_ADMITTED)
    assert len(S.EDGE_CASES) == 36 and S.WEIGHT_SETS == ("suite", "saturated", "constant")


def test_peaked_logits_log_prob_admission():
    """Constant peaked logits: dz = 0, the bar is 2^-24 (2 |z_a - z_max| + 2 |lse| + 12); torch's fp32 log_softmax
    stays within half of it for every choice."""
    for z in S.PEAKED:
        z64 = np.asarray(z, np.float64)[None, :]
        lp64 = np.log(S.probs64(z))
        lp32 = torch.log_softmax(torch.tensor(z, dtype=torch.float32), -1).double().numpy()
        for a in range(len(z)):
            bar = S.logp_bar(z64, np.zeros((1, len(z))), np.array([a]))[0]
            assert abs(lp32[a] - lp64[a]) <= 0.5 * bar, (z, a, abs(lp32[a] - lp64[a]) / bar)


def test_const_policy_logits_are_the_biases():
    z = S.SHORTFALL[0][1]
    pol = S.const_policy(z)
    g = torch.Generator().manual_seed(1)
    for obs in (torch.randn((5, 7), generator=g), 90 * torch.randn((5, 7), generator=g)):
        with torch.no_grad():
            logits, value = pol(obs)
        assert torch.equal(logits, torch.tensor(z).expand(5, 4)) and value.unique().numel() == 5
    assert B.U32 == 2.0 ** -24
