"""CPU restatement of an Ewald sum (LAMMPS ``pair_style coul/long`` + ``kspace_style ewald``, units metal) in numpy fp64 (test
infrastructure, not the thing shipped; nothing shared with the C code: images are enumerated by ``cell_cases.brute_neighbors``, the
reciprocal vectors in an explicit loop over the FULL sphere -- no half space, no phase tables, no recurrences).

For damping g (1 / A), real-space cutoff rc and reciprocal cutoff k_cut, a cell of volume V with charges q_i and total charge Q:

    E_real = sum over pairs with r < rc of qqrd2e q_a q_b erfc(g r) / r                       (no shift)
    E_k    = sum over k != 0, |k| <= k_cut of u(k) |S(k)|^2,   u(k) = qqrd2e (2 pi / V) exp(-k^2 / 4 g^2) / k^2,
             S(k) = sum_j q_j exp(i k.r_j),   k = h b1 + k b2 + l b3
    E_self = -qqrd2e g / sqrt(pi) sum q_i^2,   E_bg = -qqrd2e pi Q^2 / (2 g^2 V)
    F_i    = q_i sum_k 2 u(k) k [sin(k.r_i) Re S(k) - cos(k.r_i) Im S(k)]  (+ the real-space pair forces)
    e_i    = q_i sum_k u(k) Re(exp(-i k.r_i) S(k)) - qqrd2e g q_i^2 / sqrt(pi) - qqrd2e pi q_i Q / (2 g^2 V) + half of every pair

The formulas are those of the LAMMPS documentation and of Allen & Tildesley; no LAMMPS binary was executed.  The other terms of a
model (lj/cut, morse, buck, born) go through tests/pair_oracle.py.
"""

from __future__ import annotations

import math

import numpy as np

import pair_oracle as po
from cell_cases import brute_neighbors

QQRD2E = po.QQRD2E
COUL_LONG = 6


def recip(cell):
    """Rows b_a with b_a . a_c = 2 pi delta_ac."""
    return 2.0 * np.pi * np.linalg.inv(np.asarray(cell, np.float64).reshape(3, 3)).T


def bounds(cell, k_cut):
    """Per-axis index bounds floor(k_cut |a_i| / 2 pi): |h| = |k . a_1| / 2 pi <= |k| |a_1| / 2 pi."""
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    return [int(math.floor(k_cut * np.linalg.norm(cell[a]) / (2.0 * np.pi))) for a in range(3)]


def k_indices(cell, k_cut):
    """Integer triples (h, k, l) != 0 of the full sphere |k| <= k_cut, [n, 3], and the k vectors [n, 3]."""
    B = recip(cell)
    m = [n + 1 for n in bounds(cell, k_cut)]
    g = np.array([[h, k, l] for h in range(-m[0], m[0] + 1) for k in range(-m[1], m[1] + 1) for l in range(-m[2], m[2] + 1)
                  if (h, k, l) != (0, 0, 0)], np.int64)
    K = g @ B
    keep = (K * K).sum(axis=1) <= k_cut * k_cut
    return g[keep], K[keep]


def sphere_margin(cell, k_cut):
    """Smallest | |k|^2 / k_cut^2 - 1 | over the lattice vectors near the sphere: how far the k set is from changing."""
    B = recip(cell)
    m = [n + 2 for n in bounds(cell, k_cut)]
    g = np.array([[h, k, l] for h in range(-m[0], m[0] + 1) for k in range(-m[1], m[1] + 1) for l in range(-m[2], m[2] + 1)], np.int64)
    k2 = ((g @ B) ** 2).sum(axis=1)
    return float(np.abs(k2 / (k_cut * k_cut) - 1.0).min())


def split(terms):
    """(the model's other terms, rc of its coul/long terms or None)."""
    rest = [t for t in terms if po.STYLE.get(t[2], t[2]) not in (COUL_LONG, "coul/long")]
    rcs = {float(t[4]) for t in terms if po.STYLE.get(t[2], t[2]) in (COUL_LONG, "coul/long")}
    assert len(rcs) <= 1
    return rest, (rcs.pop() if rcs else None)


def coulomb(charges, g, rc, k_cut, types, pos, cell, hkl=None):
    """The Ewald sum alone: (E, e_atom [N], forces [N, 3]).  ``hkl``: integer triples to use instead of the sphere of this cell (the
    strain derivative at a fixed k set)."""
    types = np.asarray(types, np.int64)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    q = np.asarray(charges, np.float64)[types]
    n, V = len(pos), abs(np.linalg.det(cell))
    e_atom, F = np.zeros(n), np.zeros((n, 3))
    # real space
    i, j, _, rv = brute_neighbors(pos, cell, np.ones(3, np.uint8), rc)
    i, j = i.astype(np.int64), j.astype(np.int64)
    d = np.sqrt((rv * rv).sum(axis=1))
    qq = QQRD2E * q[i] * q[j]
    e = qq * po.erfc(g * d) / d
    de = qq * (-po.erfc(g * d) / d ** 2 - 2.0 * g / math.sqrt(math.pi) * np.exp(-g * g * d * d) / d)
    np.add.at(e_atom, i, 0.5 * e)
    np.add.at(F, i, (de / d)[:, None] * rv)
    # reciprocal space, one k vector after the other
    K = k_indices(cell, k_cut)[1] if hkl is None else np.asarray(hkl, np.int64) @ recip(cell)
    for kv in K:
        k2 = float(kv @ kv)
        u = QQRD2E * (2.0 * np.pi / V) * math.exp(-k2 / (4.0 * g * g)) / k2
        ph = pos @ kv
        c, s = np.cos(ph), np.sin(ph)
        Sre, Sim = float((q * c).sum()), float((q * s).sum())
        e_atom += q * u * (c * Sre + s * Sim)
        F += (q * 2.0 * u * (s * Sre - c * Sim))[:, None] * kv[None, :]
    Q = float(q.sum())
    e_atom += -QQRD2E * g * q * q / math.sqrt(math.pi) - QQRD2E * np.pi * q * Q / (2.0 * g * g * V)
    return float(e_atom.sum()), e_atom, F


def ewald(terms, charges, kspace, types, pos, cell, hkl=None):
    """A whole model (``pair.PairModel`` terms, charges, ``kspace`` with g_ewald / k_cut) on a fully periodic cell:
    (E, e_atom [N], forces [N, 3])."""
    rest, rc = split(terms)
    g, k_cut = (kspace.g_ewald, kspace.k_cut) if hasattr(kspace, "g_ewald") else kspace[-2:]
    E, ea, F = coulomb(charges, g, rc, k_cut, types, pos, cell, hkl=hkl)
    if rest:
        E2, ea2, F2 = po.pair(rest, charges, types, pos, cell, np.ones(3, np.uint8))
        E, ea, F = E + E2, ea + ea2, F + F2
    return E, ea, F


def model_of(pair_model):
    """(terms, charges, kspace) of a ``surface_sampling_amd.pair.PairModel``."""
    return [tuple(t) for t in pair_model.terms], pair_model.charges, pair_model.kspace
