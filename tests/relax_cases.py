"""Inputs that steer the lock-step FIRE and BFGS step kernels (csrc/relax.hip::k_fire_step, k_bfgs_step) into every branch: ``lj/cut``
clusters of tests/cg_cases.py (its terms, its non-periodic 30 A box, its builders) on a pair handle, the cheapest fp64 kind.  TEST
INFRASTRUCTURE shared by tests/test_relax_cases_cpu.py (is every case what it claims to be?) and tests/test_relax_gpu_branches.py.

A case names its geometry, held atoms, optimizer, the full parameter set of its call (``FireParams`` / ``BfgsParams`` fields, each
already the C float the ABI carries) and the branches it is there for (names of fire_oracle.BRANCHES / bfgs_oracle.BRANCHES, plus
``stride``: a chain longer than the 256 threads of the step kernels' loops).  The parameters belong to a call, not to a chain:
``batches(opt)`` groups the cases by parameter set and gives every batch the three chains that stop before their first step (all atoms
held, all atoms beyond the cutoff, a one-atom chain), so each launch mixes chains that leave at step 0 with chains that run.

Steering.  Geometry reaches most branches in a few dozen steps; parameters reach the rest quickly: dtmax = 0.115 clamps dt after its
second growth, maxstep = 0.02 clips a step in the very iteration that enlarges dt, alpha = 7e8 makes the first BFGS step ~1e-8 A so
that the next update is skipped far from round-off, and alpha = 200 on the settled 40-atom cluster makes a run that contracts for
108 steps without ever converging to fmax = 1e-6.  fmax is chosen per batch so that some chain converges inside a 4-iteration poll
window of the driver and some on a poll iteration itself.

Bounds.  ``bound(case)`` = max(1e-7 A, 10 x spread), where spread is the largest per-step position difference among 8 runs of the
RESTATEMENT from starts perturbed by 1e-12 A (tools/relax_branch_report.py sensitivity; table in profiles/r24/NOTES_relax_branches.md).
1e-7 A is the bound of tests/test_pair_gpu_relax.py for these drivers.  Nothing here was measured on the device."""

from collections import namedtuple

import numpy as np

import cg_cases as cc

Case = namedtuple("Case", "name opt types pos cell pbc fixed params branches")


def f32(x):
    return float(np.float32(x))


FIRE_DEFAULTS = dict(max_steps=20, fmax=0.01, dt=0.1, maxstep=0.2, dtmax=1.0, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, nmin=5)
BFGS_DEFAULTS = dict(max_steps=20, fmax=0.01, alpha=70.0, maxstep=0.2)
INT_FIELDS = ("max_steps", "nmin")
POLL = 4                                      # the driver reads its counters every 4 iterations (csrc/relax.hip::relax_lockstep)

# SPREAD: the cases whose measured spread exceeds 1e-9 A -- table "sensitivity" of profiles/r24/NOTES_relax_branches.md, measured on the
# restatement (CPU) by tools/relax_branch_report.py; every other case: below 1e-9 A, so its bound is the 1e-7 A floor.
SPREAD = {"bfgs:run_7": 2.27e-8, "bfgs:run_7_two_held": 5.20e-8, "bfgs:stride_257": 5.94e-9, "bfgs:capacity_40": 1.78e-9,
          "fire:gan_5_seed23": 1.73e-9}      # (the Tersoff fragment of tersoff_fire_batch)
SPREAD_FLOOR, BOUND_FLOOR, BOUND_CEILING = 1e-9, 1e-7, 1e-5


def bound(case):
    return max(BOUND_FLOOR, 10.0 * SPREAD.get(case.name, SPREAD_FLOOR))


def _params(opt, **over):
    p = dict(FIRE_DEFAULTS if opt == "FIRE" else BFGS_DEFAULTS)
    p.update(over)
    return {k: (int(v) if k in INT_FIELDS else f32(v)) for k, v in p.items()}


def _key(params):
    return tuple(sorted(params.items()))


def c_params(case_or_params, backend):
    """The ctypes struct of a case's (or a batch's) parameter set."""
    p = case_or_params.params if isinstance(case_or_params, Case) else case_or_params
    return (backend.FireParams if "dt" in p else backend.BfgsParams)(**p)


def _centred(n, seed, sigma):
    """lj_cluster with the middle of its bounding box, not its centroid, in the middle of the box (a 257-atom cluster is 28.6 A wide)."""
    _, x = cc.lj_cluster(n, seed, sigma, centre=0.0)
    return cc.lj_cluster(n, seed, sigma, centre=cc.BOX / 2 - (x.max(axis=0) + x.min(axis=0)) / 2)


def settled_cluster(n, seed, sigma, settle=300):
    """lj_cluster let down by ``settle`` steps of the FIRE restatement (fp64 forces), then rattled by ``sigma``: a start inside one
    basin.  The rattled random trees of lj_cluster are floppy and far from any minimum; 100 BFGS steps on 40 of their atoms wander and
    amplify a 1e-12 A change of the start to 1e-3 A, whatever alpha and maxstep.  From inside a basin and with alpha above every
    curvature the run contracts, never scales a step and forgets such a change (spread 2e-9 A over 108 steps)."""
    from fire_oracle import fire_relax
    import pair_oracle

    types, pos = _centred(n, seed, 0.0)
    cell, pbc = np.eye(3) * cc.BOX, np.zeros(3, np.uint8)

    def fn(p):
        E, _, F = pair_oracle.pair(cc.LJ_TERMS, None, types, p, cell, pbc)
        return E, F
    pos = fire_relax(fn, pos, max_steps=settle, fmax=1e-3)[0]
    return types, pos + np.random.default_rng(seed + 6).normal(0.0, sigma, pos.shape)


def axis_dimer(r):
    """cg_cases.dimer turned onto the x axis.  Along (0.6, 0.8, 0) the float32 rounding of the force components turns the force
    direction by ~2e-8 from step to step, which the Gram-Schmidt of k_bfgs_step rightly takes for new columns; on an axis the forces
    are parallel to the bit and the basis of a dimer with one atom held keeps one column for the whole run."""
    types, pos = cc.dimer("pair", r)
    pos[1] = pos[0] + np.array([r, 0.0, 0.0])
    return types, pos


# the capacity case: the basis of 98 is full behind the update of iteration 96 (one column per update after the first), 11 more steps
CAPACITY_STEPS = 108


def _all_cases():
    cell, pbc = np.eye(3) * cc.BOX, np.zeros(3, np.uint8)
    none = np.zeros(0, np.int64)

    def mk(opt, name, geom, fixed, params, branches=()):
        types, pos = geom
        return Case(f"{opt.lower()}:{name}", opt, np.asarray(types, np.int32), np.asarray(pos, float), cell, pbc,
                    np.asarray(fixed, np.int64), params, tuple(branches))

    c7a, c7b, c3 = cc.lj_cluster(7, 34, 0.08), cc.lj_cluster(7, 26, 0.08), cc.lj_cluster(3, 14, 0.10)
    b7a, b7b = cc.lj_cluster(7, 11, 0.08), cc.lj_cluster(7, 39, 0.08)
    near, far = axis_dimer(2.75), axis_dimer(3.6)                   # inside r_min = 2.918 A; beyond the inflection at 3.235 A
    big, c40 = _centred(257, 42, 0.05), settled_cluster(40, 1, 0.05)
    out = []
    # ---- FIRE ----------------------------------------------------------------------------------------------------------------
    F = lambda **kw: _params("FIRE", **kw)
    run = F(max_steps=60, fmax=0.05)
    out += [mk("FIRE", "run_7", c7a, none, run, ("first", "downhill_hold", "downhill_grow", "uphill_reset", "clip", "noclip")),
            mk("FIRE", "run_7_two_held", c7b, [0, 4], run, ("first", "downhill_hold", "downhill_grow", "uphill_reset")),
            mk("FIRE", "run_dimer_near", near, none, run, ("first", "downhill_hold", "uphill_reset")),
            mk("FIRE", "run_dimer_far_one_held", far, [0], run, ("first", "downhill_hold", "downhill_grow", "uphill_reset")),
            mk("FIRE", "run_trimer_two_held", c3, [0, 1], run, ("first", "downhill_hold"))]
    clamp = F(max_steps=24, fmax=1e-4, dtmax=0.115)
    out += [mk("FIRE", "dtmax_7", c7a, none, clamp, ("dtmax_clamp", "downhill_grow")),
            mk("FIRE", "dtmax_dimer_far", far, none, clamp, ("dtmax_clamp",))]
    small = F(max_steps=16, fmax=1e-4, maxstep=0.02)
    out += [mk("FIRE", "maxstep_7", c7b, none, small, ("clip", "clip_and_grow")),
            mk("FIRE", "maxstep_7_two_held", c7a, [1, 5], small, ("clip", "clip_and_grow"))]
    out += [mk("FIRE", "stride_257", big, np.arange(0, 257, 16), F(max_steps=15, fmax=1e-4), ("stride", "clip"))]
    for k in (0, 1, 3, 4, 5):
        out += [mk("FIRE", f"steps{k}_7", c7a, none, F(max_steps=k, fmax=1e-4)), mk("FIRE", f"steps{k}_dimer", far, [1], F(max_steps=k, fmax=1e-4))]
    # ---- BFGS ----------------------------------------------------------------------------------------------------------------
    B = lambda **kw: _params("BFGS", **kw)
    run = B(max_steps=20, fmax=0.05)
    out += [mk("BFGS", "run_7", b7a, none, run, ("first", "update", "neg_eig", "scaled", "unscaled")),
            mk("BFGS", "run_7_two_held", b7b, [0, 4], run, ("first", "update", "unscaled")),
            mk("BFGS", "run_dimer_far", far, none, run, ("first", "update", "neg_eig", "dropped_column", "scaled")),
            mk("BFGS", "run_dimer_near_one_held", near, [0], run, ("first", "update", "dropped_column", "unscaled")),
            mk("BFGS", "run_trimer_two_held", c3, [0, 1], run, ("first", "update", "dropped_column"))]
    tiny = B(max_steps=6, fmax=1e-4, alpha=7e8)
    out += [mk("BFGS", "alpha7e8_7", c7a, none, tiny, ("first", "skipped_update", "unscaled")),
            mk("BFGS", "alpha7e8_dimer", far, [0], tiny)]      # (df rounds to 0 in float32 there: no other branch to compute)
    out += [mk("BFGS", "stride_257", big, np.arange(0, 257, 16), B(max_steps=10, fmax=1e-4), ("first", "stride", "update", "scaled"))]
    out += [mk("BFGS", "capacity_40", c40, none, B(max_steps=CAPACITY_STEPS, fmax=1e-6, alpha=200.0), ("update", "dropped_column", "full_basis"))]
    for k in (0, 1, 3, 4, 5):
        out += [mk("BFGS", f"steps{k}_7", c7a, none, B(max_steps=k, fmax=1e-4)), mk("BFGS", f"steps{k}_dimer", far, [1], B(max_steps=k, fmax=1e-4))]
    return out


_CACHE = []


def all_cases():
    if not _CACHE:
        _CACHE.extend(_all_cases())
    return list(_CACHE)


def companions(opt, params):
    """The three chains that stop before their first step under any parameters: all held, beyond the cutoff, one atom."""
    cell, pbc = np.eye(3) * cc.BOX, np.zeros(3, np.uint8)
    t5, p5 = cc.lj_cluster(5, 14, 0.10)
    tf, pf = cc._far_apart("pair")
    t1, p1 = cc._far_apart("pair", 1)
    mk = lambda name, t, p, fx: Case(f"{opt.lower()}:{name}", opt, t, p, cell, pbc, np.asarray(fx, np.int64), params, ())
    return [mk("all_held_5", t5, p5, np.arange(5)), mk("far_apart_3", tf, pf, []), mk("one_atom", t1, p1, [])]


def batches(opt):
    """[(params, [cases])]: the cases of an optimizer grouped by parameter set, each group with the ``companions`` behind its own cases."""
    groups = {}
    for c in all_cases():
        if c.opt == opt:
            groups.setdefault(_key(c.params), []).append(c)
    return [(cs[0].params, cs + companions(opt, cs[0].params)) for cs in groups.values()]


# ---- a second fp64 kind: Tersoff GaN fragments of cg_cases.gan_fragment, one short FIRE batch with an uphill reset in it, so that the
# branch tests do not rest on one evaluator's force layout (seeds of cg_cases; each run resets uphill at iteration 3) ------
TERSOFF_FRAGMENTS = ((7, 22, 0.08, ()), (5, 23, 0.10, (1,)), (3, 14, 0.10, ()))


def tersoff_fire_batch(golden):
    """(params, [cases]): three rattled GaN fragments and the three Tersoff chains that stop at once, 20 FIRE steps."""
    params = _params("FIRE", max_steps=20, fmax=0.05)
    cell, pbc = np.eye(3) * cc.BOX, np.zeros(3, np.uint8)
    out = []
    for n, seed, sigma, held in TERSOFF_FRAGMENTS:
        t, p = cc.gan_fragment(golden, n, seed, sigma)
        out.append(Case(f"fire:gan_{n}_seed{seed}", "FIRE", t, p, cell, pbc, np.asarray(held, np.int64), params, ("first", "uphill_reset")))
    for c in cc.companions("tersoff", golden):
        out.append(Case("fire:gan_" + c.name.split(":")[1], "FIRE", c.types, c.pos, c.cell, c.pbc, c.fixed, params, ()))
    return params, out


def tersoff_force_fn(case, golden, oracle_mod):
    def fn(p):
        E, _, F = oracle_mod.tersoff(golden.tersoff_params, case.types, p, case.cell, case.pbc)
        return E, F
    return fn


def force_fn(case):
    """force_fn(pos) -> (E, F) of the case's potential from the fp64 restatement tests/pair_oracle.py."""
    import pair_oracle

    def fn(p):
        E, _, F = pair_oracle.pair(cc.LJ_TERMS, None, case.types, p, case.cell, case.pbc)
        return E, F
    return fn


def mmax_of(case):
    from bfgs_oracle import device_mmax

    return device_mmax(case.params["max_steps"])


def run_restatement(case, pos=None, record=None, mutate=None, fn=None):
    """The case through its restatement as the device runs it: forces rounded to float32, the ABI's float parameters, and for BFGS the
    capacity of the factored Hessian.  Returns (pos, energies | trace, n_steps, converged)."""
    from bfgs_oracle import bfgs_relax
    from fire_oracle import fire_relax

    fn = fn or force_fn(case)
    x = case.pos if pos is None else pos
    if case.opt == "FIRE":
        return fire_relax(fn, x, fixed=case.fixed, f32=True, record=record, mutate=mutate, **case.params)
    return bfgs_relax(fn, x, fixed=case.fixed, f32=True, record=record, mutate=mutate, mmax=mmax_of(case), **case.params)


# ---- what tests/test_relax_cases_cpu.py asserts and tools/relax_branch_report.py prints -------------------------------------------
STRUCTURAL = ("stride",)                      # no decision of the optimizer: the chain's size


def mutation_of(case, branch):
    """The decision to flip for a branch, or None where the restatement has no other branch to take: ``stride`` is a size; BFGS has no
    Hessian to update at its first step; a dependent update vector changes nothing in a dense matrix whether it is dropped or not
    (what dropping buys is capacity, and the capacity case pins that through the step at which the basis fills)."""
    import bfgs_oracle
    import fire_oracle

    return (fire_oracle.MUTATIONS if case.opt == "FIRE" else bfgs_oracle.MUTATIONS).get(branch)


def traced(case, pos=None, mutate=None, fn=None):
    rec = []
    res = run_restatement(case, pos=pos, record=rec, mutate=mutate, fn=fn)
    return res, rec


def reached(case, rec):
    got = set().union(*[r["branches"] for r in rec]) if rec else set()
    if len(case.types) > 256:
        got.add("stride")
    return got


def near_ties(case, rec):
    """Every decision of the run whose margin is inside the band in which fp64 summation order could decide it."""
    bad = []
    fmax = case.params["fmax"]
    for r in rec:
        def chk(key, ok):
            if r.get(key) is not None and not ok(r[key]):
                bad.append((r["it"], key, r[key]))
        chk("fm", lambda x: abs(x / fmax - 1.0) > 1e-4)
        chk("vf_rel", lambda x: abs(x) > 1e-6)
        chk("dt_rel", lambda x: abs(x - 1.0) > 1e-6)
        chk("normdr_rel", lambda x: abs(x - 1.0) > 1e-6)
        chk("longest_rel", lambda x: abs(x - 1.0) > 1e-6)
        chk("max_dr", lambda x: not (1e-8 <= x <= 1e-6))
        chk("a_rel", lambda x: abs(x) > 1e-8)
        chk("b_rel", lambda x: abs(x) > 1e-8)
        chk("omega_min", lambda x: abs(x) > 1e-6)          # eV/A^2: the sign of an eigenvalue, where |L|^-1 turns the step around
        # the rank of the basis decides something only where the basis can fill: in the capacity case
        for x in r.get("residuals", ()) if "full_basis" in case.branches else ():
            from bfgs_oracle import RANK_HI, RANK_LO
            if RANK_LO <= x <= RANK_HI:
                bad.append((r["it"], "residual", x))
    return bad


def sensitivity(case, n_starts=8, eps=1e-12, fn=None):
    """(spread, same_counts): the largest per-step position difference among runs of the restatement from ``n_starts`` starts perturbed
    by ``eps`` A (held atoms stay), and whether all of them took the same number of steps and ended alike."""
    import zlib

    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    runs, counts = [], set()
    for _ in range(n_starts):
        pos = case.pos + rng.uniform(-eps, eps, case.pos.shape)
        pos[case.fixed] = case.pos[case.fixed]
        res, rec = traced(case, pos=pos, fn=fn)
        runs.append(np.array([r["pos"] for r in rec]))
        counts.add((res[2], res[3], len(rec)))
    if len(counts) > 1:
        return float("inf"), False
    runs = np.array(runs)
    return float((runs.max(axis=0) - runs.min(axis=0)).max()), True


def first_step_of(rec, branch):
    for r in rec:
        if branch in r["branches"]:
            return r["it"]
    return None


def mutation_shift(case, rec, branch, fn=None):
    """(iteration, decision, shift): the other branch of ``branch`` forced at the first iteration that takes it moves the positions of
    the next iteration by ``shift`` A."""
    which, it = mutation_of(case, branch), first_step_of(rec, branch)
    if which is None or it is None:
        return it, which, None
    _, mut = traced(case, mutate=(it, which), fn=fn)
    return it, which, float(np.abs(mut[it + 1]["pos"] - rec[it + 1]["pos"]).max())


def pack(cases):
    """(structs for backend.pack_batch, fixed mask [sum N] uint8) of a list of cases."""
    return cc.pack(cases)
