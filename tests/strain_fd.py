"""Stress as the strain derivative of an energy function (test infrastructure: the checker of the device virials of the analytic
potentials, tests/test_analytic_stress_cpu.py and tests/test_gpu_analytic_stress.py).

ASE's convention: sigma_ab = (1 / V) dE / d eps_ab under x -> (1 + eps) x for positions and cell rows, V = |det cell| (also for a
slab with a vacuum axis), Voigt order xx yy zz yz xz xy, tensile positive.  The derivative is a central difference at two steps,
Richardson-extrapolated, and comes with its own uncertainty, so that a comparison needs no tolerance picked by hand.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
H = 1e-4                       # the smaller of the two steps (2 H the larger; 4 H only for the uncertainty)
EPS64 = 2.0 ** -52

FdStress = namedtuple("FdStress", "sigma virial unc volume")


def strained(structure, eps):
    """``structure`` = (positions [N, 3], cell [3, 3]); returns both multiplied by (1 + eps): x -> x (1 + eps)^T."""
    pos, cell = structure
    D = np.eye(3) + np.asarray(eps, np.float64)
    return np.asarray(pos, np.float64).reshape(-1, 3) @ D.T, np.asarray(cell, np.float64).reshape(3, 3) @ D.T


def voigt_strain(k, delta):
    """The symmetric strain tensor of Voigt component k with magnitude delta (off-diagonal: delta / 2 on either side)."""
    i, j = VOIGT[k]
    eps = np.zeros((3, 3))
    eps[i, j] += 0.5 * delta
    eps[j, i] += 0.5 * delta
    return eps


def fd_stress(energy_fn, pos, cell, h=H):
    """``energy_fn(positions, cell) -> E``.  Returns FdStress(sigma [6] eV / A^3, virial [6] = V sigma = dE / d eps in eV, unc [6] in eV,
    volume).  Per component: central differences D at h, 2 h and 4 h; the value is the Richardson extrapolate
    (4 D(h) - D(2 h)) / 3; ``unc`` = |Richardson(h, 2 h) - Richardson(2 h, 4 h)| (the remainder of the coarser extrapolate, sixteen
    times that of the finer one for a smooth energy) + 4 * 2^-52 * |E| / h (the rounding floor of a central difference of energies
    that are each good to a few units in the last place)."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    vol = abs(np.linalg.det(cell))
    e0 = abs(float(energy_fn(pos, cell)))
    virial, unc = np.zeros(6), np.zeros(6)
    for k in range(6):
        D = []
        for step in (h, 2 * h, 4 * h):
            ep = float(energy_fn(*strained((pos, cell), voigt_strain(k, step))))
            em = float(energy_fn(*strained((pos, cell), voigt_strain(k, -step))))
            D.append((ep - em) / (2 * step))
        fine, coarse = (4 * D[0] - D[1]) / 3, (4 * D[1] - D[2]) / 3
        virial[k] = fine
        unc[k] = abs(fine - coarse) + 4 * EPS64 * e0 / h
    return FdStress(virial / vol, virial, unc, vol)


def voigt_to_tensor(v):
    v = np.asarray(v, np.float64)
    return np.array([[v[0], v[5], v[4]], [v[5], v[1], v[3]], [v[4], v[3], v[2]]])


def tensor_to_voigt(t):
    return np.array([t[i, j] for i, j in VOIGT])


def rotated_voigt(v, R):
    """Voigt components of R sigma R^T (positions and cell rows mapped as x -> x R^T)."""
    return tensor_to_voigt(R @ voigt_to_tensor(v) @ R.T)
