"""Inputs that steer BFGSLineSearch (tests/bfgsls_oracle.py, csrc/bfgsls_dev.h) into its stop reasons and line-search branches, in
the manner of tests/cg_cases.py (whose geometries they reuse): small Tersoff GaN fragments and ``lj/cut`` clusters of 1 .. 9 atoms in
the non-periodic 30 A box, and the periodic 36-atom GaN slab plus two adatoms with its bulk held.  TEST INFRASTRUCTURE shared by
tests/test_bfgsls_cpu.py (does every case reach what it is listed for, far from round-off?) and tests/test_bfgsls_gpu.py.

Classes:
  exact   every comparison the run decides has a relative margin above 1e-7 (the restatement's tracer), and a start perturbed by
          1e-12 A ends with the same counts within 1e-9 A: the device must reproduce (n_steps, n_eval, stop_reason);
  noise   runs to the bottom (fmax far below what fp64 energies resolve): the last comparisons happen at the 1e-16 level.  CPU only,
          no count parity; they show the branches that exist only there (the floor on |p|, the rounding WARNs).
The parameters belong to a vssr_batch_relax_bfgs_linesearch call, not to a chain: ``batches(kind, golden)`` groups the exact cases by
parameter set, each group with the three ``companions`` that stop at their first evaluation (all atoms held, all atoms beyond the
cutoff, a one-atom chain), so every launch mixes chains that leave with chains that run.

The seeds of the bisection, ``no_update`` and skipped-update cases come from a CPU search with the tracer over rattled clusters and
parameter variants (tools/bfgsls_branch_report.py search; profiles/r19/NOTES_bfgs_linesearch.md has the search and what it did not
reach)."""

from collections import namedtuple

import numpy as np

import cg_cases as cc

DEFAULTS = dict(max_steps=20, fmax=0.01, max_eval=None, alpha=10.0, maxstep=0.2, c1=0.23, c2=0.46, stpmax=50.0)
KEYS = tuple(DEFAULTS)
EXACT_MARGIN = 1e-7

Case = namedtuple("Case", "name kind klass types pos cell pbc fixed params reason branches")


def _params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


def _key(params):
    return tuple(params[k] for k in KEYS)


def max_eval_of(params):
    return 20 * params["max_steps"] + 20 if params["max_eval"] is None else params["max_eval"]


def _kind_cases(kind, golden):
    cell, pbc = np.eye(3) * cc.BOX, np.zeros(3, np.uint8)
    none, three = np.zeros(0, np.int64), np.arange(3)
    S = cc.SEEDS[kind]

    def mk(name, klass, geom, fixed, params, reason, branches=()):
        types, pos = geom
        return Case(f"{kind}:{name}", kind, klass, np.asarray(types, np.int32), np.asarray(pos, float), cell, pbc,
                    np.asarray(fixed, np.int64), params, reason, tuple(branches))

    def rattled(n, seed, soft=0):     # the clusters of the search: sigma 0.1, atom 0 held when there are more than two
        t, p = cc.cluster(kind, golden, n, seed, 0.1)
        return (t + soft, p), ([0] if n > 2 else none)

    c7 = cc.cluster(kind, golden, 7, S["c7"], 0.08)
    c9 = cc.cluster(kind, golden, 9, S["c9"] or 12, 0.05 if S["c9"] is None else 0.08)
    c5 = cc.cluster(kind, golden, 5, S["c5"], 0.10)
    c3 = cc.cluster(kind, golden, 3, 14, 0.10)
    c4 = cc.cluster(kind, golden, 4, 15, 0.10)
    t = kind == "tersoff"
    out = [
        mk("defaults_7_three_held", "exact", c7, three, _params(), 1 if t else 2, ("cap", "dcstep3")),
        mk("defaults_5_one_held", "exact", c5, [1], _params(), 1, ("cap", "dcstep1")),   # (lj/cut: converged when step 20 opens)
        mk("defaults_4", "exact", c4, none, _params(), 1, ("dcstep1", "dcstep2", "dcstep3")),
        mk("defaults_3", "exact", c3, none, _params(), 1, ("dcstep1", "dcstep2")),
        mk("maxsteps0_7", "exact", c7, three, _params(max_steps=0), 2),
        mk("maxsteps3_9", "exact", c9, [0, 4], _params(max_steps=3), 2),
        mk("maxeval1_7", "exact", c7, three, _params(max_eval=1), 4),
        mk("maxeval5_7", "exact", c7, three, _params(max_eval=5), 4),
        mk("maxeval5_4", "exact", c4, none, _params(max_eval=5), 4),
        mk("stpmax1_7", "exact", c7, three, _params(stpmax=1.0), 3, ("warn_stpmax",)),
        mk("stpmax1_4", "exact", c4, none, _params(stpmax=1.0), 3, ("warn_stpmax",)),
        mk("all_held_5", "exact", c5, np.arange(5), _params(), 1),
        mk("far_apart_3", "exact", cc._far_apart(kind), none, _params(), 1),
        mk("one_atom", "exact", cc._far_apart(kind, 1), none, _params(), 1),
    ]
    if t:
        # SEARCH: H0 = I / alpha far too soft (alpha 0.3) and a long leash (maxstep 2): the first trials overshoot, the bracket
        # shrinks slowly and dcsrch bisects; a strict curvature test (c2 0.05) does the same with more trials per search
        g, f = rattled(4, 3)
        out.append(mk("bisect_4_seed3", "exact", g, f, _params(alpha=0.3, maxstep=2.0), 1, ("bisection", "dcstep1")))
        g, f = rattled(4, 14)
        out.append(mk("bisect_4_seed14", "exact", g, f, _params(alpha=1.0, c2=0.05, maxstep=1.0), 1, ("bisection",)))
        g, f = rattled(2, 100)
        out.append(mk("noise_dimer", "noise", g, f, _params(fmax=1e-13, max_steps=60), None, ("p_floor",)))
    else:
        out.append(mk("defaults_9_two_held", "exact", c9, [0, 4], _params(), 2, ("dcstep4",)))
        # SEARCH: the soft type (curvature far below alpha) under a strict curvature test (c2 0.1): the search extrapolates to
        # stpmax, stays there (no_update) and the next step skips its H update
        g, f = rattled(3, 1, soft=1)
        out.append(mk("noupdate_soft_3_seed1", "exact", g, f, _params(c2=0.1), 1, ("no_update", "skip_update", "dcstep3")))
        g, f = rattled(3, 100, soft=1)
        out.append(mk("stpmax1_soft_3", "exact", g, f, _params(stpmax=1.0), 3, ("warn_stpmax",)))
        g, f = rattled(2, 101)
        out.append(mk("noise_dimer", "noise", g, f, _params(fmax=1e-13, max_steps=60), None, ("p_floor",)))
    return out


def gan_slab_adatoms(golden, seed=41):
    """The periodic 36-atom GaN slab plus two adatoms, rattled, the layers more than 3 A below the top held."""
    c = cc._slab_with_adatoms(golden, 1, 2, seed)
    return Case("tersoff:gan_slab_38", "tersoff", "exact", c.types, c.pos, c.cell, c.pbc, c.fixed, _params(max_steps=8), 2, ("cap",))


def all_cases(golden):
    return _kind_cases("tersoff", golden) + _kind_cases("pair", golden) + [gan_slab_adatoms(golden)]


def companions(kind, golden):
    names = {f"{kind}:all_held_5", f"{kind}:far_apart_3", f"{kind}:one_atom"}
    return [c for c in all_cases(golden) if c.name in names]


def batches(kind, golden):
    """[(params, [cases])]: the exact cases of a kind grouped by parameter set, each group with the ``companions`` behind its own
    cases, re-issued under the group's parameters (no force acts on them and convergence is tested first: reason 1 under any)."""
    groups = {}
    for c in all_cases(golden):
        if c.kind == kind and c.klass == "exact":
            groups.setdefault(_key(c.params), []).append(c)
    out = []
    for cs in groups.values():
        p = cs[0].params
        have = {c.name for c in cs}
        cs = cs + [c._replace(params=p) for c in companions(kind, golden) if c.name not in have]
        out.append((p, cs))
    return out


force_fn = cc.force_fn
pack = cc.pack


def run_restatement(case, golden, oracle_mod, trace=None, pos=None, record_interval=0):
    from bfgsls_oracle import bfgs_linesearch

    return bfgs_linesearch(force_fn(case, golden, oracle_mod), case.pos if pos is None else pos, fixed=case.fixed, trace=trace,
                           record_interval=record_interval, **case.params)
