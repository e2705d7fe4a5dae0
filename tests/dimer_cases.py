"""Inputs of tests/test_dimer_gpu.py and their CPU rehearsal in tests/test_dimer_cpu.py (test infrastructure).  A structure is
``(types, positions, cell, pbc)``; a case is one dimer: a structure, its held mask [n], a starting mode [n, 3] (None: drawn from the
seed of its parameters) and the parameters of ``dimer_oracle.run``.  In a batch every structure stands twice (chains 2 g, 2 g + 1)."""
from collections import namedtuple

import numpy as np

import cg_cases as cc
import dimer_oracle as do
import neb_cases as nc
import pair_oracle as po

Case = namedtuple("Case", "name struct held mode params terms")

# ---- the physics anchor: the free lj/cut atom of neb_cases above the held triangle, started off the axis -------------------------------
ANCHOR_START = (0.10, -0.05, 0.40)
ANCHOR = dict(delta=0.01, phi_tol=np.pi / 180.0, fmax=0.01, max_steps=200)
ANCHOR_ROTATIONS = ((8, 1), (8, 2), (1, 1))          # (max_rot_first, max_rot)
ANCHOR_SEEDS = tuple(range(6))


def triangle_energy():
    """The three held-held pairs of the triangle under the restated lj/cut: the part of E0 the closed-form barrier does not count."""
    T, X, cell, pbc = nc.anchor_image(0.0, 0.0, 0.0)
    return float(po.pair(cc.LJ_TERMS, None, T[:3], X[:3], cell, pbc)[0])


def anchor_case(seed, max_rot_first, max_rot, **over):
    return Case(f"anchor_s{seed}_r{max_rot_first}{max_rot}", nc.anchor_image(*ANCHOR_START), nc.ANCHOR_HELD, None,
                dict(ANCHOR, seed=seed, max_rot_first=max_rot_first, max_rot=max_rot, **over), cc.LJ_TERMS)


def anchor_cases(seeds=ANCHOR_SEEDS):
    return [anchor_case(s, a, b) for s in seeds for a, b in ANCHOR_ROTATIONS]


def anchor_hessian_at(offset, h=1e-3):
    """3 x 3 Hessian of the free atom at `offset` from the triangle's centre, by central differences of the restated forces."""
    s = nc.anchor_image(*offset)
    fn = nc.lj_batch_fn([s])
    H = np.zeros((3, 3))
    for c in range(3):
        p, m = s[1].copy(), s[1].copy()
        p[3, c] += h
        m[3, c] -= h
        H[c] = -(fn(p)[1][3] - fn(m)[1][3]) / (2 * h)
    return 0.5 * (H + H.T)


def anchor_third_derivatives(offset, h=1e-2):
    """T[i, j, k] = d^3 E / dx_i dx_j dx_k of the free atom at `offset`, by central differences of the Hessian."""
    T = np.zeros((3, 3, 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        T[:, :, k] = (anchor_hessian_at(np.asarray(offset) + e) - anchor_hessian_at(np.asarray(offset) - e)) / (2 * h)
    return T


def anchor_third_derivative_along(N, offset, delta, h=1e-3, samples=9):
    """max over the dimer's segment x0 .. x0 + delta N of |d^3 E / ds^3| along N, by central differences of the restated forces."""
    N = np.asarray(N, np.float64)
    s = nc.anchor_image(*offset)
    fn = nc.lj_batch_fn([s])

    def g(t):                                # dE / ds at x0 + t N
        x = s[1].copy()
        x[3] += t * N
        return -float(fn(x)[1][3] @ N)
    return max(abs((g(t + h) - 2.0 * g(t) + g(t - h)) / (h * h)) for t in np.linspace(0.0, delta, samples))


def anchor_curvature_bound(N, offset, H, delta, fmax):
    """What the dimer's curvature C at the midpoint x0 = centre + `offset` with mode N may differ by from the lowest eigenvalue of the
    saddle's Hessian H:
      forward difference over delta along N:  |C - N.H(x0).N| <= delta / 2 max |d^3 E / ds^3| over the segment x0 .. x0 + delta N
        (the mean-value form of the error.  At the saddle itself the third derivative along z vanishes by symmetry, so the maximum over
        the segment, where it has grown to delta times the fourth derivative, is what counts);
      x0 off the saddle by dx = H^-1 F, |F| < fmax:  |N.(H(x0) - H).N| <= 2 |T(N, N, .)| fmax / min |lambda|, T the third derivatives
        at x0 (they vanish at the saddle by symmetry and grow linearly towards x0; the factor 2 covers the curvature of that growth);
      N off the lowest eigenvector v:  N.H.N - lambda_min <= (1 - (N.v)^2) (lambda_max - lambda_min)."""
    lam, vec = np.linalg.eigh(H)
    T = anchor_third_derivatives(offset)
    N = np.asarray(N, np.float64)
    tnn = np.einsum("ijk,i,j->k", T, N, N)
    return (0.5 * delta * anchor_third_derivative_along(N, offset, delta) + 2.0 * np.linalg.norm(tnn) * fmax / np.abs(lam).min()
            + (1.0 - (N @ vec[:, 0]) ** 2) * (lam[-1] - lam[0]))


# ---- the census cases -----------------------------------------------------------------------------------------------------------------
# a free atom between two held ones on a line, the mode along the line: every force is along x to the bit (the other components of
# every distance are exact zeros), so F_perp = Fd - (Fd.N) N is an exact zero: no rotation, f = 0.  The curvature along the line is
# positive (the atom is caged), the dimer walks against the force along N and never meets a negative curvature: reason 2.
def line_case():
    T = np.zeros(3, np.int32)
    X = np.array([[14.0, 16.0, 16.0], [18.0, 16.0, 16.0], [16.25, 16.0, 16.0]])
    mode = np.zeros((3, 3))
    mode[2, 0] = 1.0
    return Case("line_f_zero", (T, X, nc.BOX, nc.OPEN), np.array([1, 1, 0], np.uint8), mode,
                dict(ANCHOR, max_steps=4, max_rot_first=3, max_rot=1, maxstep=0.05), cc.LJ_TERMS)


# ---- non-finite evaluations: the wall term of neb_cases (overflows everywhere inside its 0.6 A cutoff, absent outside) -----------------
# The free type-1 atom stands 2.4 A from a held type-1 atom (36 eV / A towards +x) and 0.7 A from the held type-0 wall atom.  With the
# mode along y the curvature is negative (a repulsive pair seen sideways) and F0.N = 0, so G = F0: the first FIRE step is clamped to
# maxstep = 0.2 A and lands inside the wall: non-finite at evaluation E of step 1, back to the input, 0 steps.
WALL_TYPES = np.array([1, 1, 0], np.int32)
WALL_HELD = nc.WALL_HELD


def wall_case_E():
    X = np.array([[10.0, 10.0, 10.0], [12.4, 10.0, 10.0], [13.1, 10.0, 10.0]])
    mode = np.zeros((3, 3))
    mode[1, 1] = 1.0
    return Case("wall_at_E", (WALL_TYPES, X, nc.BOX, nc.OPEN), WALL_HELD, mode, dict(ANCHOR, max_steps=12, max_rot_first=0, max_rot=0),
                nc.WALL_TERMS)


# Evaluation R: the wall atom now stands 0.6065 A beside the free atom (along y), the mode between x and y.  The first translation
# (no rotation allowed before it, maxstep = 0.001 A) moves the midpoint by 1e-3 A along the mode; midpoint and dimer end stay
# outside the wall's cutoff.  The first trial rotation then turns the end towards y and into the wall: non-finite at an evaluation
# R after one step, back to the input x0 and N bit for bit, 0 steps counted.
def wall_case_R():
    X = np.array([[10.0, 10.0, 10.0], [12.4, 10.0, 10.0], [12.4, 10.6065, 10.0]])
    mode = np.zeros((3, 3))
    mode[1] = [0.8, 0.6, 0.0]
    return Case("wall_at_R", (WALL_TYPES, X, nc.BOX, nc.OPEN), WALL_HELD, mode,
                dict(ANCHOR, max_steps=40, max_rot_first=0, max_rot=1, maxstep=0.001), nc.WALL_TERMS)


def census_cases():
    return [anchor_case(0, 8, 1), anchor_case(2, 8, 2), anchor_case(4, 1, 1),
            anchor_case(1, 8, 1, maxstep=0.02, max_steps=12),       # a binding maxstep clamp, and reason 2
            line_case(), wall_case_E(), wall_case_R()]


REQUIRED = ("rotate", "no_rotate_phi_tol", "no_rotate_counter", "no_rotate_f_zero", "phi_plus_half_pi", "translate_convex",
            "translate_saddle", "uphill_reset", "downhill_grow", "clip", "reason1", "reason2", "reason3_at_E", "reason3_at_R")
# cases whose comparisons are exact ties by construction (f = 0 against 0): device and restatement agree to the bit there
EXACT = ("line_f_zero",)


# ---- the parity batches of tests/test_dimer_gpu.py: one structure each of 3, 65 and 257 atoms (one, two and five strides of the 256-thread
# workgroup and the tail of its reduction), the first two atoms of every chain held, modes drawn; tests/test_neb_gpu.py's grids ----------
PARITY_KINDS = ("pair_lj", "sw", "eam_alloy", "tersoff", "vashishta", "ewald")
PARITY_SIZES = (3, 65, 257)
EXTRA_SHAPE = {"tersoff": (2, 1.95), "vashishta": (2, 1.9), "ewald": (2, 2.7)}      # (types in use, grid spacing in A)
PARITY_JITTER = 0.05
PARITY = dict(max_steps=10, max_rot_first=3, max_rot=1, delta=0.01, phi_tol=np.pi / 180.0, fmax=1e-4, seed=7)
MARGIN = 1e-6        # the smallest relative margin a comparison of a parity case may have (an ulp of trigonometry must not flip a branch)


def parity_structs(kind):
    import cg_resident_cases as rc
    import pair_cases as pc

    out = []
    for k, n in enumerate(PARITY_SIZES):
        pbc = [1, 1, 1] if kind == "ewald" else ([1, 1, 0] if n == 257 else [0, 0, 0])
        if kind in EXTRA_SHAPE:
            nt, spacing = EXTRA_SHAPE[kind]
            out.append(pc.grid_chain(n, 80 + k, pbc, n_types=nt, spacing=spacing, jitter=PARITY_JITTER))
        else:
            out.append(rc.grid(kind, n, 80 + k, pbc, jitter=PARITY_JITTER))
    return out


def parity_batch(kind):
    """(structures: every one twice, held mask [sum N])."""
    structs = [s for s in parity_structs(kind) for _ in (0, 1)]
    return structs, np.concatenate([(np.arange(len(s[0])) < 2) for s in structs]).astype(np.uint8)


def cpu_force_fn(kind, golden=None, oracle_mod=None):
    """structs -> force callback of a whole batch under the CPU restatement of the potential behind the parity engine of `kind`."""
    import cg_resident_cases as rc

    if kind == "pair_lj":
        one = lambda s, x: po.pair(cc.LJ_TERMS, None, s[0], x, s[2], s[3])
    elif kind == "sw":
        import sw_oracle as so

        P = so.si_params()
        one = lambda s, x: so.sw(P, s[0], x, s[2], s[3])
    elif kind == "eam_alloy":
        import eam_alloy_oracle as ao

        tab = rc.eam_tables("eam_alloy")
        one = lambda s, x: ao.eam_typed(tab, s[0], x, s[2], s[3])
    elif kind == "tersoff":
        one = lambda s, x: oracle_mod.tersoff(golden.tersoff_params, s[0], x, s[2], s[3])
    elif kind == "vashishta":
        import vashishta_oracle as vo

        P = vo.sic_params()[1]
        one = lambda s, x: vo.vashishta(P, s[0], x, s[2], s[3])
    elif kind == "ewald":
        import ewald_cases as ec
        import ewald_oracle as eo
        from surface_sampling_amd import pair

        terms, charges, kspace = eo.model_of(pair.parse(ec.RAGGED_MODEL, 3))
        one = lambda s, x: eo.ewald(terms, charges, kspace, s[0], x, s[2])
    else:
        raise ValueError(kind)

    def make(structs):
        start = start_of(structs)

        def fn(pos):
            # the two chains of a dimer differ in a few rows only, but the restatements know nothing of that: every chain is evaluated
            E, F = [], []
            for s, a0, a1 in zip(structs, start[:-1], start[1:]):
                e, _, f = one(s, pos[a0:a1])[:3]
                E.append(e)
                F.append(f)
            return np.array(E), np.vstack(F)
        return fn
    return make


# ---- packing and running --------------------------------------------------------------------------------------------------------------
def pack(cases):
    """(structures of the batch: every case's twice, held mask [sum N], modes [sum N, 3] or None when every case draws its own)."""
    structs = [c.struct for c in cases for _ in (0, 1)]
    held = np.concatenate([np.tile(np.asarray(c.held, np.uint8), 2) for c in cases])
    drawn = [c.mode is None for c in cases]
    assert all(drawn) or not any(drawn)
    modes = None if all(drawn) else np.vstack([np.vstack([c.mode, np.zeros_like(c.mode)]) for c in cases])
    return structs, held, modes


def start_of(structs):
    return np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])]).astype(np.int64)


def pair_batch_fn(structs, terms):
    """tests/pair_oracle.py over a batch (overflows are the point of the wall term: no warnings)."""
    start = start_of(structs)

    def fn(pos):
        E, F = [], []
        with np.errstate(all="ignore"):
            for s, a0, a1 in zip(structs, start[:-1], start[1:]):
                e, _, f = po.pair(terms, None, s[0], pos[a0:a1], s[2], s[3])
                E.append(e)
                F.append(f)
        return np.array(E), np.vstack(F)
    return fn


def run_case(case, force_fn=None, record=None, **over):
    structs, held, modes = pack([case])
    fn = force_fn or pair_batch_fn(structs, case.terms)
    return do.run(fn, np.vstack([s[1] for s in structs]), start_of(structs), fixed=held, modes=modes, record=record,
                  **{**case.params, **over})


def census(cases=None):
    """({branch: set of case names that visit it}, {case name: {comparison: smallest relative margin}})."""
    seen = {b: set() for b in do.BRANCHES}
    margins = {}
    for c in cases or census_cases():
        rec = []
        run_case(c, record=rec)
        margins[c.name] = smallest_margins(rec)
        for r in rec:
            for b in r["branches"]:
                seen[b].add(c.name)
    return seen, margins


def smallest_margins(record):
    out = {}
    for r in record:
        for k, v in r["margins"].items():
            out[k] = min(out.get(k, np.inf), v)
    return out
