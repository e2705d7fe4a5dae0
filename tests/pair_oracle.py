"""CPU restatement of LAMMPS ``pair_style lj/cut``, ``morse``, ``buck``, ``born`` and ``coul/dsf`` (and sums of them per type pair) in
numpy fp64 (test infrastructure, not the thing shipped; nothing shared with the C code).

Neighbors come from ``cell_cases.brute_neighbors`` (every image enumerated).  A model is a list of terms ``(type_a, type_b, style, c,
rc, shift)`` on unordered type pairs -- the names or the codes 1 .. 5 of ``STYLE`` -- and per-type charges.  For r < rc:

    lj/cut    4 eps [(sig/r)^12 - (sig/r)^6]                        c = eps sig
    morse     D0 [exp(-2 alpha (r - r0)) - 2 exp(-alpha (r - r0))]  c = D0 alpha r0
    buck      A exp(-r/rho) - C/r^6                                 c = A rho C
    born      A exp((sig - r)/rho) - C/r^6 + D/r^8                  c = A rho sig C D
    coul/dsf  qqrd2e q_a q_b [erfc(alpha r)/r - erfc(alpha rc)/rc + B (r - rc)]        c = alpha
              B = erfc(alpha rc)/rc^2 + 2 alpha/sqrt(pi) exp(-alpha^2 rc^2)/rc

``shift`` subtracts E(rc) from the first four.  pe/atom: half of every pair energy to either atom, and the coul/dsf self term
-(erfc(alpha rc)/(2 rc) + alpha/sqrt(pi)) qqrd2e q_i^2 to every atom whose type carries a coul/dsf term.  The formulas are those of
the LAMMPS documentation (coul/dsf: Fennell & Gezelter, J. Chem. Phys. 124, 234104 (2006)); no LAMMPS binary was executed.
"""

from __future__ import annotations

import math

import numpy as np

from cell_cases import brute_neighbors

QQRD2E = 14.399645
STYLE = {1: "lj/cut", 2: "morse", 3: "buck", 4: "born", 5: "coul/dsf"}
_erfc = np.frompyfunc(math.erfc, 1, 1)


def erfc(x):
    return np.asarray(_erfc(np.asarray(x, np.float64)), np.float64)


def term_energy(style, c, rc, r, qq=0.0, shift=0):
    """(E, dE/dr) of one term at distances ``r`` (all below rc)."""
    style = STYLE.get(style, style)
    r = np.asarray(r, np.float64)

    def raw(x):
        if style == "lj/cut":
            s6 = (c[1] / x) ** 6
            return 4 * c[0] * (s6 * s6 - s6), -24 * c[0] * (2 * s6 * s6 - s6) / x
        if style == "morse":
            u = np.exp(-c[1] * (x - c[2]))
            return c[0] * (u * u - 2 * u), -2 * c[1] * c[0] * (u * u - u)
        if style == "buck":
            u = c[0] * np.exp(-x / c[1])
            return u - c[2] / x ** 6, -u / c[1] + 6 * c[2] / x ** 7
        if style == "born":
            u = c[0] * np.exp((c[2] - x) / c[1])
            return u - c[3] / x ** 6 + c[4] / x ** 8, -u / c[1] + 6 * c[3] / x ** 7 - 8 * c[4] / x ** 9
        raise ValueError(style)

    if style == "coul/dsf":
        a = c[0]
        B = math.erfc(a * rc) / rc ** 2 + 2 * a / math.sqrt(math.pi) * math.exp(-a * a * rc * rc) / rc
        e = QQRD2E * qq * (erfc(a * r) / r - math.erfc(a * rc) / rc + B * (r - rc))
        de = QQRD2E * qq * (-erfc(a * r) / r ** 2 - 2 * a / math.sqrt(math.pi) * np.exp(-a * a * r * r) / r + B)
        return e, de
    e, de = raw(r)
    if shift:
        e = e - raw(np.float64(rc))[0]
    return e, de


def cutoff(terms) -> float:
    return max(float(t[4]) for t in terms)


def pair(terms, charges, types, pos, cell, pbc):
    """Returns (E, e_atom [N], forces [N, 3])."""
    types = np.asarray(types, np.int64)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = len(pos)
    q = np.zeros(int(types.max()) + 1 if n else 1) if charges is None else np.asarray(charges, np.float64)
    i, j, _, rv = brute_neighbors(pos, cell, pbc, cutoff(terms))
    i, j = i.astype(np.int64), j.astype(np.int64)
    d = np.sqrt((rv * rv).sum(axis=1))
    ti, tj = types[i], types[j]
    e_edge, de_edge = np.zeros(len(d)), np.zeros(len(d))
    e_atom = np.zeros(n)
    dsf_types = set()
    for a, b, style, c, rc, shift in terms:
        name = STYLE.get(style, style)
        if name == "coul/dsf":
            dsf_types |= {a, b}
            self_c = -(math.erfc(c[0] * rc) / (2 * rc) + c[0] / math.sqrt(math.pi)) * QQRD2E
        m = (((ti == a) & (tj == b)) | ((ti == b) & (tj == a))) & (d < rc)
        if m.any():
            e, de = term_energy(name, c, rc, d[m], qq=q[a] * q[b] if name == "coul/dsf" else 0.0, shift=shift)
            e_edge[m] += e
            de_edge[m] += de
    for t in dsf_types:
        e_atom[types == t] += self_c * q[t] ** 2
    np.add.at(e_atom, i, 0.5 * e_edge)                 # every pair is two directed edges: half to either atom
    F = np.zeros((n, 3))
    np.add.at(F, i, (de_edge / d)[:, None] * rv)       # r = x_j - x_i: F_i = E'(r) r / |r| summed over the atom's own edges
    return float(e_atom.sum()), e_atom, F


def model_of(pair_model):
    """(terms, charges) of a ``surface_sampling_amd.pair.PairModel``."""
    return [tuple(t) for t in pair_model.terms], pair_model.charges


def rocksalt(a=5.64, reps=1):
    """Conventional 8-atom rocksalt cell (times reps^3): (types [0 = cation, 1 = anion], positions, cell)."""
    cat = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    frac = np.concatenate([cat, cat + [.5, .5, .5]]) % 1.0
    types = np.array([0] * 4 + [1] * 4, np.int32)
    shifts = np.array([[x, y, z] for x in range(reps) for y in range(reps) for z in range(reps)], float)
    frac = (frac[None] + shifts[:, None]).reshape(-1, 3) / reps
    return np.tile(types, len(shifts)), frac @ (np.eye(3) * a * reps), np.eye(3) * a * reps


MADELUNG_NACL = 1.7475646

# Born-Mayer-Huggins-like numbers for a +-1 rocksalt (tests only; not a fitted potential) + damped-shifted Coulomb
ROCKSALT_COMMANDS = [
    "pair_style hybrid/overlay born 8.0 coul/dsf 0.2 12.0",
    "pair_coeff 1 1 born 0.2637 0.317 2.340 1.0486 -0.4993",
    "pair_coeff 1 2 born 0.2110 0.317 2.755 6.9906 -8.6758",
    "pair_coeff 2 2 born 0.1582 0.317 3.170 72.4022 -145.4285",
    "pair_coeff * * coul/dsf",
    "set type 1 charge 1.0",
    "set type 2 charge -1.0",
]
