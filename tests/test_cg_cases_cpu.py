"""The cases of tests/cg_cases.py through the traced numpy restatement of the CG minimiser (tests/cg_oracle.py), on the CPU: every
case reaches the stop reason and the branches it is listed for, and together the cases reach every branch counter and every
reachable stop reason.  This is what keeps tests/test_cg_gpu_branches.py from silently testing nothing."""

from collections import Counter

import numpy as np
import pytest

import cg_cases as cc
from cg_oracle import BRANCHES, cg_minimize

# branches the seed search could not reach (at most proj_rejected and not_downhill_reset may ever stand here): none
UNREACHED = frozenset()
# reason 6 (zero force) cannot occur: f.h > 0 implies max|h| > 0
REACHABLE_REASONS = {1, 2, 3, 4, 5, 7, 8}


@pytest.fixture(scope="module")
def traced(golden, oracle_mod):
    """{case name: (case, counter, (pos, e, n_iter, n_eval, reason, energies))} -- every case once."""
    out = {}
    for c in cc.all_cases(golden):
        tr = Counter()
        out[c.name] = (c, tr, cc.run_restatement(c, golden, oracle_mod, trace=tr))
    return out


def test_case_names_are_unique_and_small(golden):
    cases = cc.all_cases(golden)
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.kind in ("tersoff", "pair") and c.klass in ("exact", "noise")
        assert 1 <= len(c.types) <= 9 or c.name == "tersoff:gan_slab_36"
        if not c.pbc.any():      # the box is wider than the cutoff and holds the cluster
            assert c.pos.min() > 0.0 and c.pos.max() < cc.BOX
        if c.klass == "noise":
            assert c.params["etol"] == 0.0 and c.params["ftol"] == 0.0 and 200 <= c.params["max_iter"] <= 500


def test_every_case_reaches_what_it_is_listed_for(traced):
    for name, (c, tr, res) in traced.items():
        why = res[4]
        if c.reason is not None:
            assert why == c.reason, (name, why, dict(tr))
        for b in c.branches:
            assert tr[b] > 0, (name, b, dict(tr))
        if c.klass == "noise":
            assert why in (7, 8) and tr["reset_to_start"] == 1, (name, why)
        assert set(tr) <= set(BRANCHES)


def test_the_cases_cover_every_branch_and_reason(traced):
    assert UNREACHED <= {"proj_rejected", "not_downhill_reset"}
    for kind in ("tersoff", "pair", None):      # the union; the per-kind unions are printed (the lock-step driver serves both kinds)
        total, reasons = Counter(), set()
        for c, tr, res in traced.values():
            if kind is None or c.kind == kind:
                total.update(tr)
                reasons.add(res[4])
        print(kind or "all", {b: total[b] for b in BRANCHES}, sorted(reasons))
    assert {b for b in BRANCHES if total[b] == 0} == set(UNREACHED), {b: total[b] for b in BRANCHES}
    assert reasons >= REACHABLE_REASONS and 6 not in reasons
    # ... and in exact cases alone (those are compared count for count on the device) every branch but the return to x0
    exact = Counter()
    for c, tr, _ in traced.values():
        if c.klass == "exact":
            exact.update(tr)
    assert {b for b in BRANCHES if exact[b] == 0} <= {"reset_to_start"} | set(UNREACHED)
    # Tersoff alone (the only kind the chain-resident kernel serves) reaches every branch as well
    ters = Counter()
    for c, tr, _ in traced.values():
        if c.kind == "tersoff":
            ters.update(tr)
    assert {b for b in BRANCHES if ters[b] == 0} == set(UNREACHED)


def test_exact_cases_stop_far_from_round_off(traced, golden, oracle_mod):
    """What "exact" means: a start perturbed by 1e-12 A -- orders of magnitude more than the device's summation order can change
    -- gives the same (n_iter, n_eval, stop_reason), and final positions within 1e-9 A: the run amplifies a perturbation less than
    1000 times, so differences of the size of fp64 round-off (1e-15 .. 1e-14) stay two orders below the 1e-9 bounds of the device
    comparison.  (Free, floppy clusters that run for 50 .. 100 iterations amplify 1e5 .. 1e7 times; they are no exact cases.)"""
    rng = np.random.default_rng(5)
    for name, (c, _, res) in traced.items():
        if c.klass != "exact":
            continue
        for _ in range(3):
            pos = c.pos + rng.uniform(-1e-12, 1e-12, c.pos.shape)
            pos[c.fixed] = c.pos[c.fixed]
            got = cc.run_restatement(c, golden, oracle_mod, pos=pos)
            assert got[2:5] == res[2:5], (name, got[2:5], res[2:5])
            assert np.abs(got[0] - res[0]).max() < 1e-9 and abs(got[1] - res[1]) < 1e-9, (name, np.abs(got[0] - res[0]).max())
        # ... and so do energies and forces that carry relative noise of 1e-13 in EVERY evaluation (the device's arithmetic differs
        # from numpy's in every evaluation, not only at the start; a run that contracts forgets a perturbed start)
        fn = cc.force_fn(c, golden, oracle_mod)
        for _ in range(3):
            def noisy(p):
                E, F = fn(p)
                return E * (1.0 + 1e-13 * rng.uniform(-1, 1)), F * (1.0 + 1e-13 * rng.uniform(-1, 1, F.shape))
            got = cg_minimize(noisy, c.pos, fixed=c.fixed, **c.params)
            assert got[2:5] == res[2:5], (name, got[2:5], res[2:5])
            assert np.abs(got[0] - res[0]).max() < 1e-9 and abs(got[1] - res[1]) < 1e-9, (name, np.abs(got[0] - res[0]).max())


def test_tracing_changes_nothing(golden, oracle_mod):
    c = [c for c in cc.all_cases(golden) if c.name == "tersoff:dmax10_7"][0]
    a = cc.run_restatement(c, golden, oracle_mod)
    b = cc.run_restatement(c, golden, oracle_mod, trace=Counter())
    assert np.array_equal(a[0], b[0]) and a[1:5] == b[1:5] and a[5] == b[5]
    # dmax stays a keyword of its own with LAMMPS' default (0.1): the existing callers pass none of the two new arguments
    fn = cc.force_fn(c, golden, oracle_mod)
    d, e = cg_minimize(fn, c.pos, max_iter=5), cg_minimize(fn, c.pos, max_iter=5, dmax=0.1, trace=None)
    assert np.array_equal(d[0], e[0]) and d[1:5] == e[1:5] and not np.array_equal(d[0], cg_minimize(fn, c.pos, max_iter=5, dmax=0.05)[0])


def test_batches_hold_every_case_once_and_chains_that_stop_at_once(golden):
    orig = {c.name: c for c in cc.all_cases(golden)}
    for kind in ("tersoff", "pair"):
        seen = []
        for klass in ("exact", "noise"):
            for params, cs in cc.batches(kind, klass, golden):
                assert all(c.params == params and c.kind == kind for c in cs)
                seen += [c.name for c in cs if orig[c.name].params == params]      # (not the companions re-issued under other parameters)
                if klass == "exact":
                    assert {c.name.split(":")[1] for c in cs} >= {"all_held_5", "far_apart_3", "one_atom"}
        assert sorted(seen) == sorted(n for n, c in orig.items() if c.kind == kind)


def test_noise_bound_is_the_measured_one():
    assert cc.NOISE_ENERGY_BOUND == max(10.0 * cc.NOISE_SPREAD_MAX, 1e-8)


def test_size_cases_sit_on_the_limits_of_the_chain_resident_kernel(golden):
    sizes = [len(c.types) for c in cc.size_cases(golden, with_257=True)]
    assert sizes == [1, 63, 64, 65, 255, 256, 257]
    g = golden.structure("GaN_3x3_pristine").repeat((7, 1, 1))
    assert len(g.numbers) == 252
    for c in cc.size_cases(golden, with_257=True):
        assert c.params["max_iter"] == 5 and len(c.fixed) < len(c.types)
