"""Inputs that steer the LAMMPS-style CG minimiser (tests/cg_oracle.py, csrc/cg_dev.h) into every stop reason and line-search
branch: small Tersoff (GaN parameter set of tests/golden) and ``lj/cut`` clusters of 1 .. 9 atoms in a non-periodic box wider than
the cutoff, one periodic 36-atom GaN slab, and the slabs at the size limits of the chain-resident kernel.  TEST INFRASTRUCTURE
shared by tests/test_cg_cases_cpu.py (does every case reach what it is listed for?) and tests/test_cg_gpu_branches.py.

A case names its engine kind, geometry, held atoms, CG parameters, class and what it is there for (``reason`` / ``branches``).
Classes:
  exact   the run stops far from round-off: the device must reproduce (n_iter, n_eval, stop_reason) of the numpy restatement;
  noise   etol = ftol = 0: the run goes to the bottom and ends with reason 7 or 8 through the return to x0; its last comparisons
          happen at the 1e-16 level, where iteration counts depend on summation order -- no count parity, the energy bound below.
The CG parameters belong to a vssr_batch_relax_cg call, not to a chain: ``batches(kind, klass)`` groups the cases by parameter set,
and every exact batch also carries the three chains that stop at once (``companions``: all atoms held, all atoms beyond the cutoff, a
one-atom chain), so each launch holds chains that leave at the first iteration next to chains that keep running.

The seeds of ``proj_rejected`` and ``not_downhill_reset`` come from a CPU search over rattled clusters with the restatement's tracer
(profiles/r18/NOTES_cg_branches.md has the search and its outcome)."""

from collections import namedtuple

import numpy as np

DEFAULTS = dict(max_iter=100, max_eval=10000, etol=1e-5, ftol=1e-5, dmax=0.1)
BOX = 30.0                                   # non-periodic cube; clusters sit in its middle
# lj/cut, two types that never share a chain: type 0 stiff (eps 1 eV: curvature ~ 57 eps / sigma^2 = 8 eV/A^2, the line search projects
# and clamps at dmax), type 1 soft (eps 0.05 eV: curvature < 1 eV/A^2, alphamax = 1 is too short a step and the Armijo gain falls below
# EMACH long before the forces vanish -- "linesearch alpha is zero" far from round-off).  (type_a, type_b, style, (eps, sigma), rc, shift)
LJ_TERMS = [(0, 0, "lj/cut", (1.0, 2.6), 8.0, 0), (1, 1, "lj/cut", (0.05, 2.6), 8.0, 0), (0, 1, "lj/cut", (0.2, 2.6), 8.0, 0)]
LJ_NTYPES = 2
LJ_R0 = 2.0 ** (1.0 / 6.0) * 2.6

Case = namedtuple("Case", "name kind klass types pos cell pbc fixed params reason branches")

# |E_device - E_restatement| of the noise cases: 10 x the largest spread of the restatement's final energy over 8 starts perturbed by
# 1e-12 A (measured on the CPU, tools/cg_branch_report.py noise; table in profiles/r18/NOTES_cg_branches.md), floored at the line search's
# EMACH.  The largest measured spread is far below the floor, so the floor is the bound.
NOISE_SPREAD_MAX = 6.217e-14    # eV (tersoff:noise_4_seed103 and noise_6_seed102; the lj/cut dimers: 0)
NOISE_ENERGY_BOUND = max(10.0 * NOISE_SPREAD_MAX, 1e-8)


def _params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


def _key(params):
    return tuple(params[k] for k in ("max_iter", "max_eval", "etol", "ftol", "dmax"))


def gan_fragment(golden, n, seed, sigma, centre=BOX / 2):
    """n atoms of the GaN slab around one of its atoms (the nearest ones, so the fragment is bonded), rattled, in the box."""
    g = golden.structure("GaN_3x3_pristine")
    rng = np.random.default_rng(seed)
    c = int(rng.integers(len(g.numbers)))
    d = np.linalg.norm(g.positions - g.positions[c], axis=1)
    idx = np.argsort(d, kind="stable")[:n]
    pos = g.positions[idx] - g.positions[idx].mean(axis=0) + centre + rng.normal(0.0, sigma, (n, 3))
    types = np.array([0 if z == 31 else 1 for z in g.numbers[idx]], np.int32)
    return types, pos


def lj_cluster(n, seed, sigma, centre=BOX / 2):
    """n atoms grown one by one at ~r_min from an earlier atom and no closer than 0.85 r_min to any, rattled, in the box."""
    rng = np.random.default_rng(seed)
    pts = [np.zeros(3)]
    while len(pts) < n:
        v = rng.normal(size=3)
        cand = pts[int(rng.integers(len(pts)))] + LJ_R0 * v / np.linalg.norm(v)
        if min(np.linalg.norm(cand - p) for p in pts) > 0.85 * LJ_R0:
            pts.append(cand)
    pos = np.array(pts)
    pos = pos - pos.mean(axis=0) + centre + rng.normal(0.0, sigma, (n, 3))
    return np.zeros(n, np.int32), pos


def cluster(kind, golden, n, seed, sigma, centre=BOX / 2):
    return gan_fragment(golden, n, seed, sigma, centre) if kind == "tersoff" else lj_cluster(n, seed, sigma, centre)


def _far_apart(kind, n=3):
    """n atoms 10 A apart: beyond the cutoff of either potential (Tersoff <= 3.1 A, lj/cut 8 A), so no force acts."""
    pos = np.array([[5.0 + 10.0 * k, 5.0, 5.0 + 0.3 * k] for k in range(n)])
    return (np.array([0, 1, 0], np.int32)[:n] if kind == "tersoff" else np.zeros(n, np.int32)), pos


def dimer(kind, r):
    pos = np.array([[BOX / 2, BOX / 2, BOX / 2], [BOX / 2 + 0.6 * r, BOX / 2 + 0.8 * r, BOX / 2]])
    return (np.array([0, 1], np.int32) if kind == "tersoff" else np.zeros(2, np.int32)), pos


# SEARCH: tools/cg_branch_report.py search looked for proj_rejected and not_downhill_reset over rattled clusters of both kinds.  Both
# branches turn out to be common once dmax stops clamping the first trial point (dmax = 10): halved alphas, rejected projections and
# directions that are no longer downhill within a dozen iterations.  The winners are the dmax10 cases below.
#
# Seeds of the exact cases.  A free, floppy cluster that runs for 50 .. 100 iterations amplifies a 1e-12 A change of its start to
# 1e-7 .. 1e-5 A at its end (rigid-body and soft modes): no 1e-9 A comparison can be made there whatever the arithmetic.  So the
# longer exact runs hold three atoms, and every seed below was picked on the CPU by the restatement alone: a start perturbed by
# 1e-12 A gives the same counts and final positions within 3e-10 A (tests/test_cg_cases_cpu.py asserts 1e-9).
SEEDS = {"tersoff": dict(c7=22, c9=15, c5=23, ftol7=None, dmax002=12, dmax10_7=37, dmax10_5=16),
         "pair": dict(c7=34, c9=None, c5=14, ftol7=39, dmax002=11, dmax10_7=26, dmax10_5=21)}


def _kind_cases(kind, golden):
    cell, pbc = np.eye(3) * BOX, np.zeros(3, np.uint8)
    none, three = np.zeros(0, np.int64), np.arange(3)
    S = SEEDS[kind]

    def mk(name, klass, geom, fixed, params, reason, branches=()):
        types, pos = geom
        return Case(f"{kind}:{name}", kind, klass, np.asarray(types, np.int32), np.asarray(pos, float), cell, pbc,
                    np.asarray(fixed, np.int64), params, reason, tuple(branches))

    c7 = cluster(kind, golden, 7, S["c7"], 0.08)
    c9 = cluster(kind, golden, 9, S["c9"] or 12, 0.05 if S["c9"] is None else 0.08)
    c5 = cluster(kind, golden, 5, S["c5"], 0.10)
    c3 = cluster(kind, golden, 3, 14, 0.10)
    c4 = cluster(kind, golden, 4, 15, 0.10)
    r_far = 2.6 if kind == "tersoff" else 4.4          # a stretched bond: many dmax-limited line searches back to the minimum
    dmax10 = _params(dmax=10.0, etol=0.0, ftol=1e-3, max_iter=12)
    out = [
        mk("defaults_7_three_held", "exact", c7, three, _params(), 1, ("proj", "proj_accepted")),
        mk("defaults_4", "exact", c4, none, _params(), 1),
        mk("ftol_5_one_held", "exact", c5, [1], _params(etol=0.0, ftol=1e-3), 2),
        mk("ftol_3", "exact", c3, none, _params(etol=0.0, ftol=1e-3), 2),
        mk("maxiter0_7", "exact", c7, none, _params(max_iter=0), 3),
        mk("maxiter1_7", "exact", c7, none, _params(max_iter=1), 3),
        mk("maxiter3_9", "exact", c9, none, _params(max_iter=3), 3),
        mk("maxeval0_7", "exact", c7, none, _params(max_eval=0, etol=0.0, ftol=0.0), 4),
        mk("maxeval7_7", "exact", c7, none, _params(max_eval=7, etol=0.0, ftol=0.0), 4),
        mk("maxeval7_3", "exact", c3, none, _params(max_eval=7, etol=0.0, ftol=0.0), 4),
        mk("all_held_5", "exact", c5, np.arange(5), _params(), 5),
        mk("far_apart_3", "exact", _far_apart(kind), none, _params(), 5),
        mk("one_atom", "exact", _far_apart(kind, 1), none, _params(), 5),
        mk("dmax002_7_three_held", "exact", cluster(kind, golden, 7, S["dmax002"], 0.08), three,
           _params(dmax=0.02, etol=0.0, ftol=1e-2, max_iter=40), 3, ("dmax_clamp",)),
        mk("dmax10_7", "exact", cluster(kind, golden, 7, S["dmax10_7"], 0.08), none, dmax10, 3,
           ("alpha_one", "halve", "proj_rejected", "not_downhill_reset")),
        mk("dmax10_5", "exact", cluster(kind, golden, 5, S["dmax10_5"], 0.10), none, dmax10, 3,
           ("alpha_one", "halve", "proj_rejected", "not_downhill_reset")),
        mk("dimer_one_held", "exact", dimer(kind, r_far), [0], _params(etol=0.0, ftol=1e-3), 2, ("ndof_restart", "beta_zero")),
    ]
    if S["c9"] is not None:
        out.append(mk("defaults_9_two_held", "exact", c9, [0, 4], _params(), 1))
    if S["ftol7"] is not None:
        out.append(mk("ftol_7_three_held", "exact", cluster(kind, golden, 7, S["ftol7"], 0.08), three, _params(etol=0.0, ftol=1e-3), 2))
    # noise: clusters (n, seed, centre) whose run to the bottom ends through the return to x0 within max_iter = 400 on the CPU.  Most
    # rattled clusters do not: at the bottom every projection changes the energy by < EMACH and is "accepted" until max_iter.  These
    # ended with reason 7 / 8 from 9 starts perturbed by 1e-12 A and in 16 runs with relative noise of 1e-15 / 1e-14 in every
    # evaluation (a 5-atom fragment and a dimer that ran into max_iter once in those 16 were left out).  The lj/cut dimers sit near
    # the origin of the box, where an ulp of a coordinate is 4x smaller and f.h falls below EPS_QUAD (reason 7).
    noisy = ((4, 103, BOX / 2), (4, 133, BOX / 2), (6, 102, BOX / 2)) if kind == "tersoff" else ((2, 110, 4.0), (2, 116, 4.0))
    for n, seed, centre in noisy:
        out.append(mk(f"noise_{n}_seed{seed}", "noise", cluster(kind, golden, n, seed, 0.1, centre), none,
                      _params(etol=0.0, ftol=0.0, max_iter=400), None, ("reset_to_start",)))
    if kind == "pair":      # the soft type: the line search gives up (reason 8) when the Armijo gain of a full step falls below EMACH.  The
        for n, seed in ((2, 100), (3, 100), (3, 106)):      # iteration at which that happens moves with 1e-13 of noise: noise class
            t, p = cluster(kind, golden, n, seed, 0.1)
            out.append(mk(f"noise_soft_{n}_seed{seed}", "noise", (t + 1, p), none, _params(etol=0.0, ftol=0.0, max_iter=400), 8, ("reset_to_start",)))
    return out


def gan_slab(golden, sigma=0.05, seed=4):
    """The periodic 36-atom GaN slab of tests/test_cg.py, rattled; bulk layers (atoms 12 .. 35 there) held."""
    g = golden.structure("GaN_3x3_pristine")
    rng = np.random.default_rng(seed)
    types = np.array([0 if z == 31 else 1 for z in g.numbers], np.int32)
    return types, g.positions + rng.normal(0, sigma, g.positions.shape), np.array(g.cell, float), np.ones(3, np.uint8)


def all_cases(golden):
    out = _kind_cases("tersoff", golden) + _kind_cases("pair", golden)
    t, p, c, b = gan_slab(golden)
    out.append(Case("tersoff:gan_slab_36", "tersoff", "exact", t, p, c, b, np.arange(12, 36), _params(), 1, ("proj",)))
    return out


def companions(kind, golden):
    """The three chains that stop in their first iteration (reason 5; reason 3 with max_iter = 0) under any parameters."""
    names = {f"{kind}:all_held_5", f"{kind}:far_apart_3", f"{kind}:one_atom"}
    return [c for c in all_cases(golden) if c.name in names]


def batches(kind, klass, golden):
    """[(params, [cases])]: the cases of a kind and class grouped by parameter set, each exact group with the ``companions`` (re-issued
    under the group's parameters) behind its own cases."""
    groups = {}
    for c in all_cases(golden):
        if c.kind == kind and c.klass == klass:
            groups.setdefault(_key(c.params), []).append(c)
    out = []
    for cs in groups.values():
        p = cs[0].params
        if klass == "exact":
            have = {c.name for c in cs}
            cs = cs + [c._replace(params=p, reason=None) for c in companions(kind, golden) if c.name not in have]
        out.append((p, cs))
    return out


def force_fn(case, golden, oracle_mod):
    """force_fn(pos) -> (E, F) of the case's potential from the fp64 CPU oracles."""
    if case.kind == "tersoff":
        def fn(p):
            E, _, F = oracle_mod.tersoff(golden.tersoff_params, case.types, p, case.cell, case.pbc)
            return E, F
    else:
        import pair_oracle

        def fn(p):
            E, _, F = pair_oracle.pair(LJ_TERMS, None, case.types, p, case.cell, case.pbc)
            return E, F
    return fn


def run_restatement(case, golden, oracle_mod, trace=None, pos=None):
    from cg_oracle import cg_minimize

    return cg_minimize(force_fn(case, golden, oracle_mod), case.pos if pos is None else pos, fixed=case.fixed, trace=trace, **case.params)


# ---- the size limits of the chain-resident kernel (CM_MAX_ATOMS = 256, 64-centre site tiles) -------------------------------------
def _slab_with_adatoms(golden, reps, n_ads, seed, n_keep=None):
    g = golden.structure("GaN_3x3_pristine").repeat((reps, 1, 1))
    rng = np.random.default_rng(seed)
    types = np.array([0 if z == 31 else 1 for z in g.numbers], np.int32)
    pos = g.positions + rng.normal(0, 0.03, g.positions.shape)
    ztop = g.positions[:, 2].max()
    fixed = g.positions[:, 2] < ztop - 3.0
    if n_ads:
        ads = np.array([(rng.uniform(), rng.uniform(), 0.0) for _ in range(n_ads)]) @ g.cell
        ads[:, 2] = ztop + rng.uniform(1.6, 2.4, n_ads)
        pos, types, fixed = np.vstack([pos, ads]), np.concatenate([types, np.arange(n_ads, dtype=np.int32) % 2]), np.concatenate([fixed, np.zeros(n_ads, bool)])
    if n_keep is not None:       # drop atoms from the end: a slab with vacancies (still periodic)
        pos, types, fixed = pos[:n_keep], types[:n_keep], fixed[:n_keep]
    return Case(f"tersoff:slab_{len(types)}", "tersoff", "size", types, pos, np.array(g.cell, float), np.ones(3, np.uint8),
                np.flatnonzero(fixed), _params(max_iter=5), None, ())


def size_cases(golden, with_257=False):
    """GaN chains of 1, 63, 64, 65, 255 and exactly 256 atoms (7 x 36 = 252 slab atoms + 4 adatoms); with_257: one more of 257."""
    one = [c for c in all_cases(golden) if c.name == "tersoff:one_atom"][0]._replace(params=_params(max_iter=5), klass="size")
    out = [one, _slab_with_adatoms(golden, 2, 0, 31, n_keep=63), _slab_with_adatoms(golden, 2, 0, 32, n_keep=64),
           _slab_with_adatoms(golden, 2, 0, 33, n_keep=65), _slab_with_adatoms(golden, 7, 3, 34), _slab_with_adatoms(golden, 7, 4, 35)]
    if with_257:
        out.append(_slab_with_adatoms(golden, 7, 5, 36))
    return out


def pack(cases):
    """(structs for backend.pack_batch, fixed mask [sum N] uint8) of a list of cases."""
    structs = [(c.types, c.pos, c.cell, c.pbc) for c in cases]
    mask = []
    for c in cases:
        m = np.zeros(len(c.types), np.uint8)
        m[c.fixed] = 1
        mask.append(m)
    return structs, np.concatenate(mask)
