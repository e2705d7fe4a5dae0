"""The cases of tests/relax_cases.py through the traced numpy restatements of FIRE and BFGS (tests/fire_oracle.py, bfgs_oracle.py), on
the CPU: every case reaches the branches it is listed for, together they reach every branch of k_fire_step and k_bfgs_step, no
decision of any run is a near tie, a start perturbed by 1e-12 A stays within the committed spread, and forcing the other branch at
a listed step moves the next positions by 100 bounds or more.  This is what keeps tests/test_relax_gpu_branches.py from passing with
a branch wrong, or from silently testing nothing."""

import numpy as np
import pytest

import bfgs_oracle
import fire_oracle
import relax_cases as rc

REQUIRED = {"FIRE": set(fire_oracle.BRANCHES) | {"stride"}, "BFGS": set(bfgs_oracle.BRANCHES) | {"stride"}}
# branches that have no other branch in a dense restatement (relax_cases.mutation_of says why)
NO_MUTATION = {("FIRE", "stride"), ("BFGS", "stride"), ("BFGS", "first"), ("BFGS", "dropped_column")}


@pytest.fixture(scope="module")
def traces():
    """{case name: (case, (pos, trace, n_steps, converged), records)} -- every case and every batch's companions once."""
    out = {}
    for opt in ("FIRE", "BFGS"):
        for _, cases in rc.batches(opt):
            for c in cases:
                out[(c.name, rc._key(c.params))] = (c,) + rc.traced(c)
    return out


def _own(traces):
    names = {c.name for c in rc.all_cases()}
    return [v for (name, _), v in traces.items() if name in names]


def test_case_names_are_unique_and_shapes_are_the_smallest_that_reach_the_code():
    cases = rc.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert c.opt in ("FIRE", "BFGS") and c.pos.min() > 0.0 and c.pos.max() < rc.cc.BOX, c.name
        assert set(c.params) == set(rc.FIRE_DEFAULTS if c.opt == "FIRE" else rc.BFGS_DEFAULTS)
        assert all(v == rc.f32(v) for k, v in c.params.items() if k not in rc.INT_FIELDS)      # the C floats the ABI carries
        assert len(c.types) in (2, 3, 7, 40, 257), c.name
        if len(c.types) == 257:
            assert c.params["max_steps"] <= 15
    for opt in ("FIRE", "BFGS"):
        sizes = {(len(c.types), len(c.fixed)) for c in cases if c.opt == opt}
        assert sizes >= {(2, 0), (2, 1), (3, 2), (7, 0), (7, 2)} and any(n == 257 for n, _ in sizes)
        assert {c.params["max_steps"] for c in cases if c.opt == opt} >= {0, 1, 3, 4, 5}
    cap = [c for c in cases if "full_basis" in c.branches]
    assert len(cap) == 1 and len(cap[0].types) - len(cap[0].fixed) >= 40 and 3 * 40 > rc.mmax_of(cap[0])


def test_the_sizing_rule_of_the_factored_hessian():
    assert [bfgs_oracle.device_mmax(k) for k in (0, 20, 47, 48, 108, 1000)] == [2, 42, 96, 98, 98, 98]
    lds = lambda m: 8 * (2 * m * (m | 1) + 5 * m + 8)
    assert lds(98) <= 160 * 1024 - 4096 < lds(100)


def test_every_case_reaches_what_it_is_listed_for_and_together_they_reach_every_branch(traces):
    total = {"FIRE": set(), "BFGS": set()}
    for c, res, rec in _own(traces):
        got = rc.reached(c, rec)
        assert set(c.branches) <= got, (c.name, sorted(set(c.branches) - got))
        assert got <= REQUIRED[c.opt]
        total[c.opt] |= set(c.branches)
    for opt in total:                                            # ... as LISTED branches: those are the ones the mutation test covers
        assert total[opt] == REQUIRED[opt], (opt, sorted(REQUIRED[opt] - total[opt]))
    # nsteps_pos <= nmin and > nmin, the enlarged dt clipped in the same step, both BFGS step scalings: named branches above.  Stops:
    for opt in ("FIRE", "BFGS"):
        ends = {}
        for (name, _), (c, res, rec) in traces.items():
            if c.opt != opt:
                continue
            n, conv = res[2], res[3]
            kind = ("before_step_0" if n == 0 else "on_a_poll_iteration" if (n + 1) % rc.POLL == 0 else "inside_a_poll_window") if conv else "never"
            ends.setdefault(kind, []).append(name)
            assert n <= c.params["max_steps"] and (conv or n == c.params["max_steps"])
        print(opt, {k: len(v) for k, v in ends.items()})
        assert set(ends) >= {"before_step_0", "inside_a_poll_window", "never"}, (opt, ends)


def test_every_batch_mixes_chains_that_leave_at_step_0_with_chains_that_run(traces):
    orig = {c.name for c in rc.all_cases()}
    for opt in ("FIRE", "BFGS"):
        seen = []
        for params, cases in rc.batches(opt):
            assert all(c.params == params and c.opt == opt for c in cases)
            steps = [traces[(c.name, rc._key(params))][1][2] for c in cases]
            assert steps[-3:] == [0, 0, 0] and [c.name.split(":")[1] for c in cases[-3:]] == ["all_held_5", "far_apart_3", "one_atom"]
            assert max(steps) > 0 or params["max_steps"] == 0
            seen += [c.name for c in cases if c.name in orig]
        assert sorted(seen) == sorted(c.name for c in rc.all_cases() if c.opt == opt)


def test_no_decision_is_a_near_tie(traces):
    """vf away from 0 by 1e-6 |v||f|, max|F| from fmax by 1e-4, normdr / longest from maxstep and dt finc from dtmax by 1e-6, max|dr|
    from 1e-7 by a factor 10, a and b of the BFGS update from 0 by 1e-8 |dr||df|, the smallest eigenvalue of H from 0 by 1e-6 eV/A^2:
    inside those bands fp64 summation order could decide a branch."""
    for c, res, rec in traces.values():
        assert rc.near_ties(c, rec) == [], c.name


def test_the_rank_of_the_update_vectors_is_never_a_close_call_where_the_basis_fills(traces):
    """The capacity case.  Every residual of an update vector against the span of the earlier ones is a new direction (> 1e-6 of its
    norm) or what the rounding of r = r0 + step leaves of an exactly dependent H dr: below 1e-9 of its norm AND below alpha x half an
    ulp of the coordinates, the most that rounding can put there.  (1e-13 is out of reach for any run that contracts: the rounding is
    alpha x 2e-15 A whatever the step, so it measures 1e-13 of |H dr| only while |H dr| > 0.05 alpha.)  One column per update after
    the first: the basis of 98 fills at update 96, not at 46, and the run has more than 8 steps with a skipped update behind it."""
    (c, res, rec), = [v for v in _own(traces) if "full_basis" in v[0].branches]
    assert rc.mmax_of(c) == 98 and not res[3] and res[2] == c.params["max_steps"]
    lo, hi = [], []
    for r in rec:
        if "residuals" not in r:
            continue
        for x in r["residuals"]:
            (lo if x < bfgs_oracle.RANK_TOL else hi).append(x)
        if r["residuals"][1] < bfgs_oracle.RANK_TOL:
            assert r["dg_noise_ratio"] < 1.0, (r["it"], r["dg_noise_ratio"])
        else:
            assert r["dg_noise_ratio"] > 1e6, (r["it"], r["dg_noise_ratio"])
    print(f"capacity: {len(lo)} dependent vectors, residual <= {max(lo):.2e}; {len(hi)} new directions, residual >= {min(hi):.2e}")
    assert max(lo) < bfgs_oracle.RANK_LO and min(hi) > bfgs_oracle.RANK_HI
    m = [r["m"] for r in rec]                                    # (a record holds m behind its iteration's update)
    assert m[1] == 2 and all(m[k] == k + 1 for k in range(2, 97)), m
    full = [r["it"] for r in rec if "full_basis" in r["branches"]]
    assert full == list(range(97, c.params["max_steps"])) and len(full) >= 8 and m[-1] == 97
    assert all("update" in rec[k]["branches"] for k in range(1, 97))      # ... through steps 46 and 50, which the old limit cut off


def test_a_start_perturbed_by_1e_12_stays_within_the_committed_spread():
    """relax_cases.SPREAD is what this measures (restatement only), and every bound is max(1e-7, 10 spread) <= 1e-5 A."""
    for c in rc.all_cases():
        s, same = rc.sensitivity(c)
        print(f"{c.name}: spread {s:.3e} A, bound {rc.bound(c):.3e} A")
        assert same, c.name
        assert s <= rc.SPREAD.get(c.name, rc.SPREAD_FLOOR), (c.name, s)
        assert rc.BOUND_FLOOR <= rc.bound(c) <= rc.BOUND_CEILING
        assert rc.bound(c) == max(1e-7, 10.0 * rc.SPREAD.get(c.name, 1e-9))
    assert set(rc.SPREAD) <= {c.name for c in rc.all_cases()} | {"fire:gan_5_seed23"}


def test_the_tersoff_fragments_reset_uphill_within_20_steps(golden, oracle_mod):
    """The batch of the second fp64 kind, held to the same standards: listed branches reached, no near tie, spread, mutation."""
    params, cases = rc.tersoff_fire_batch(golden)
    assert params["max_steps"] <= 20 and [len(c.types) for c in cases] == [7, 5, 3, 5, 3, 1]
    for c in cases:
        fn = rc.tersoff_force_fn(c, golden, oracle_mod)
        res, rec = rc.traced(c, fn=fn)
        assert set(c.branches) <= rc.reached(c, rec) and rc.near_ties(c, rec) == [], c.name
        assert (res[2] == 0 and res[3]) if not c.branches else "uphill_reset" in rc.reached(c, rec)
        s, same = rc.sensitivity(c, fn=fn)
        assert same and s <= rc.SPREAD.get(c.name, rc.SPREAD_FLOOR) and rc.bound(c) == 1e-7, (c.name, s)
        for b in c.branches:
            it, which, shift = rc.mutation_shift(c, rec, b, fn=fn)
            print(f"{c.name}: {b} at iteration {it}: shift {shift:.3e} A")
            assert shift >= 100.0 * rc.bound(c)


def test_the_other_branch_at_a_listed_step_moves_the_next_positions_by_100_bounds(traces):
    n = 0
    for c, res, rec in _own(traces):
        for b in c.branches:
            it, which, shift = rc.mutation_shift(c, rec, b)
            if which is None:
                assert (c.opt, b) in NO_MUTATION, (c.name, b)
                continue
            print(f"{c.name}: {b} at iteration {it}, {which} flipped: shift {shift:.3e} A = {shift / rc.bound(c):.1e} bounds")
            assert shift >= 100.0 * rc.bound(c), (c.name, b, it, shift)
            n += 1
    assert n >= 40


def test_the_new_arguments_change_nothing_unless_used():
    """Existing tests call the restatements without them: same bits with and without a record, fp64 forces unless f32 is set, no cap
    unless mmax is set."""
    c = [c for c in rc.all_cases() if c.name == "bfgs:run_7"][0]
    fn = rc.force_fn(c)
    for relax, kw in ((bfgs_oracle.bfgs_relax, dict(max_steps=8)), (fire_oracle.fire_relax, dict(max_steps=8))):
        a, b = relax(fn, c.pos, **kw), relax(fn, c.pos, record=[], **kw)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        assert not np.array_equal(a[0], relax(fn, c.pos, f32=True, **kw)[0])
    a, b = bfgs_oracle.bfgs_relax(fn, c.pos, max_steps=8), bfgs_oracle.bfgs_relax(fn, c.pos, max_steps=8, mmax=4)
    assert not np.array_equal(a[0], b[0])
