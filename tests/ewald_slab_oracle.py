"""CPU restatement of the Ewald sum for slabs (LAMMPS ``kspace_style ewald`` + ``kspace_modify slab F`` under ``boundary p p f``, units
metal) in numpy fp64, and an exact two-dimensional Ewald sum to measure it against (test infrastructure, not the thing shipped;
nothing shared with the C code).  Restated from Yeh & Berkowitz, J. Chem. Phys. 111, 3155 (1999), Ballenegger, Arnold & Cerda,
J. Chem. Phys. 131, 094107 (2009) for cells with net charge, and Heyes, Barber & Clarke (1977) / de Leeuw & Perram (1979) for the
two-dimensional sum; no LAMMPS binary was executed.

(a) ``coulomb`` / ``ewald``: for cell rows a, b, c with open axis c and slab factor F

    real space            pairs of the in-plane images only (pbc 1 1 0)
    E_k, E_self, E_bg     the formulas of tests/ewald_oracle.py in the extended cell (a, b, F c): V' = F V, its reciprocal vectors
    E_slab = qqrd2e (2 pi / V') (M^2 - Q R2 - Q^2 L'^2 / 12),   Q = sum q, M = sum q z, R2 = sum q z^2,
             z_i = r_i . n, n = a x b / |a x b| (the general normal, so that tests/strain_fd.py may shear the cell), L' = F |c . n|
    e_i   += qqrd2e (2 pi / V') q_i (z_i M - (R2 + Q z_i^2) / 2 - Q L'^2 / 12),     F_i += -qqrd2e (4 pi / V') q_i (M - Q z_i) n

(b) ``ewald_2d``: the exact sum of a neutral cell periodic in a and b only, in e^2 / A (no qqrd2e), A = |a x b|, double sums over
    ordered pairs with i = j included:

    1/2 sum_ij sum'_n q_i q_j erfc(g |r_ij + n|) / |r_ij + n|                                               (in-plane images n)
    + (pi / 2 A) sum_{k != 0} sum_ij q_i q_j cos(k . rho_ij) / k [e^{k z_ij} erfc(k / 2 g + g z_ij) + e^{-k z_ij} erfc(k / 2 g - g z_ij)]
    - (pi / A) sum_ij q_i q_j [z_ij erf(g z_ij) + e^{-g^2 z_ij^2} / (g sqrt(pi))]  -  (g / sqrt(pi)) sum q_i^2
"""

from __future__ import annotations

import math

import numpy as np

import ewald_oracle as eo
import pair_oracle as po
from cell_cases import brute_neighbors

QQRD2E = eo.QQRD2E
PBC_SLAB = np.array([1, 1, 0], np.uint8)
_erf = np.frompyfunc(math.erf, 1, 1)


def extended(cell, F):
    """The cell (a, b, F c)."""
    ext = np.array(cell, np.float64).reshape(3, 3)
    ext[2] *= F
    return ext


def normal(cell):
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    n = np.cross(cell[0], cell[1])
    return n / np.linalg.norm(n)


def slab_term(q, pos, cell, F):
    """The dipole correction alone for per-atom charges ``q``: (E_slab, e_atom [N], forces [N, 3])."""
    q = np.asarray(q, np.float64)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    n = normal(cell)
    z = pos @ n
    Vx = F * abs(np.linalg.det(cell))
    Lx = F * abs(cell[2] @ n)
    Q, M, R2 = float(q.sum()), float((q * z).sum()), float((q * z * z).sum())
    c = QQRD2E * 2.0 * np.pi / Vx
    E = c * (M * M - Q * R2 - Q * Q * Lx * Lx / 12.0)
    e = c * q * (z * M - 0.5 * (R2 + Q * z * z) - Q * Lx * Lx / 12.0)
    f = (-2.0 * c * q * (M - Q * z))[:, None] * n[None, :]
    return E, e, f


def k_indices(cell, k_cut, F):
    """(h, k, l) and k vectors of the full sphere of the extended cell (the fixed k set of a strain derivative)."""
    return eo.k_indices(extended(cell, F), k_cut)


def coulomb(charges, g, rc, k_cut, F, types, pos, cell, hkl=None, correct=True):
    """(a): (E, e_atom [N], forces [N, 3]).  ``hkl``: integer triples of the extended cell to use instead of its sphere;
    ``correct=False`` leaves the dipole correction out (the plain 3-D sum of the extended cell with in-plane real-space images)."""
    types = np.asarray(types, np.int64)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    ext = extended(cell, F)
    q = np.asarray(charges, np.float64)[types]
    n, Vx = len(pos), abs(np.linalg.det(ext))
    e_atom, Fo = np.zeros(n), np.zeros((n, 3))
    i, j, _, rv = brute_neighbors(pos, cell, PBC_SLAB, rc)
    i, j = i.astype(np.int64), j.astype(np.int64)
    d = np.sqrt((rv * rv).sum(axis=1))
    qq = QQRD2E * q[i] * q[j]
    e = qq * po.erfc(g * d) / d
    de = qq * (-po.erfc(g * d) / d ** 2 - 2.0 * g / math.sqrt(math.pi) * np.exp(-g * g * d * d) / d)
    np.add.at(e_atom, i, 0.5 * e)
    np.add.at(Fo, i, (de / d)[:, None] * rv)
    K = eo.k_indices(ext, k_cut)[1] if hkl is None else np.asarray(hkl, np.int64) @ eo.recip(ext)
    # the full sphere at once: [atoms, k vectors] phases (no half space, no phase tables, no recurrences)
    k2 = (K * K).sum(axis=1)
    u = QQRD2E * (2.0 * np.pi / Vx) * np.exp(-k2 / (4.0 * g * g)) / k2
    ph = pos @ K.T
    c, s = np.cos(ph), np.sin(ph)
    Sre, Sim = q @ c, q @ s
    e_atom += q * ((c * Sre + s * Sim) @ u)
    Fo += 2.0 * q[:, None] * (((s * Sre - c * Sim) * u) @ K)
    Q = float(q.sum())
    e_atom += -QQRD2E * g * q * q / math.sqrt(math.pi) - QQRD2E * np.pi * q * Q / (2.0 * g * g * Vx)
    if correct:
        _, es, fs = slab_term(q, pos, cell, F)
        e_atom += es
        Fo += fs
    return float(e_atom.sum()), e_atom, Fo


def ewald(terms, charges, kspace, types, pos, cell, hkl=None):
    """A whole model (``pair.PairModel`` terms, charges, ``kspace`` with g_ewald / k_cut / slab) on a slab: (E, e_atom, forces)."""
    rest, rc = eo.split(terms)
    E, ea, F = coulomb(charges, kspace.g_ewald, rc, kspace.k_cut, kspace.slab, types, pos, cell, hkl=hkl)
    if rest:
        E2, ea2, F2 = po.pair(rest, charges, types, pos, cell, PBC_SLAB)
        E, ea, F = E + E2, ea + ea2, F + F2
    return E, ea, F


def ewald_2d(q, g, rc, k_cut, pos, cell):
    """(b): the energy in e^2 / A of per-atom charges ``q`` (neutral) in a cell periodic along a and b only (both in the xy plane)."""
    q = np.asarray(q, np.float64)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    assert abs(q.sum()) < 1e-12 and cell[0, 2] == 0.0 and cell[1, 2] == 0.0
    A = abs(np.cross(cell[0], cell[1])[2])
    i, j, _, rv = brute_neighbors(pos, cell, PBC_SLAB, rc)
    d = np.sqrt((rv * rv).sum(axis=1))
    E = 0.5 * float((q[i] * q[j] * po.erfc(g * d) / d).sum())
    qq = q[:, None] * q[None, :]
    dz = pos[:, None, 2] - pos[None, :, 2]
    B = 2.0 * np.pi * np.linalg.inv(cell[:2, :2]).T          # rows: in-plane reciprocal vectors
    m = [int(k_cut * np.linalg.norm(cell[a]) / (2.0 * np.pi)) + 1 for a in range(2)]
    for h in range(-m[0], m[0] + 1):
        for k in range(-m[1], m[1] + 1):
            kv = h * B[0] + k * B[1]
            kk = math.hypot(kv[0], kv[1])
            if (h == 0 and k == 0) or kk > k_cut:
                continue
            ph = pos[:, :2] @ kv
            cosij = np.cos(ph[:, None] - ph[None, :])
            f = np.exp(kk * dz) * po.erfc(kk / (2.0 * g) + g * dz) + np.exp(-kk * dz) * po.erfc(kk / (2.0 * g) - g * dz)
            E += np.pi / (2.0 * A) * float((qq * cosij / kk * f).sum())
    erf = np.asarray(_erf(g * dz), np.float64)
    E -= np.pi / A * float((qq * (dz * erf + np.exp(-g * g * dz * dz) / (g * math.sqrt(math.pi)))).sum())
    E -= g / math.sqrt(math.pi) * float((q * q).sum())
    return E
