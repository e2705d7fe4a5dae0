"""Harmonic vibrations restated in numpy (test infrastructure; the contract of csrc/vib.hip and ``vssr_batch_vibrations``).

ASE's ``Vibrations.read`` as remembered: rows of the Hessian from central (nfree = 2) or five-point (nfree = 4) differences of the
forces, the optional Frederiksen correction, ``H += H.T``, then the eigen-decomposition of ``D H D`` with ``D = diag(mass^-1/2)``,
and the harmonic zero-point and Helmholtz energies.  Dense numpy and LAPACK; nothing here follows the device's loop order."""
import numpy as np

HBAR, E_CHARGE, AMU = 1.054571817e-34, 1.602176634e-19, 1.66053906660e-27     # CODATA 2018
S_UNIT = HBAR * 1e10 / np.sqrt(E_CHARGE * AMU)                                # eV per sqrt(eV / A^2 / amu) = 0.0646541513...
KB = 8.617333262e-5                                                           # eV / K
EV_PER_INV_CM = 1.239841984e-4


def dof(vib_idx):
    """(atom, component) of every degree of freedom, in order."""
    return [(int(a), c) for a in vib_idx for c in range(3)]


def displaced(pos, a, c, k, delta):
    p = np.array(pos, dtype=np.float64).reshape(-1, 3).copy()
    p[a, c] = p[a, c] + k * delta
    return p


def rows(force_fn, pos, vib_idx, delta=0.01, nfree=2, method="standard"):
    """The rows before ``H += H.T``: [m, m].  ``force_fn(pos [N, 3]) -> forces [N, 3]``."""
    if nfree not in (2, 4) or method not in ("standard", "frederiksen"):
        raise ValueError("nfree is 2 or 4, method 'standard' or 'frederiksen'")
    vib_idx = np.asarray(vib_idx, dtype=np.int64)
    m = 3 * len(vib_idx)
    K = np.zeros((m, m))

    def F(a, c, k):
        f = np.array(force_fn(displaced(pos, a, c, k, delta)), dtype=np.float64).reshape(-1, 3)
        if method == "frederiksen":
            tot = np.zeros(3)
            for i in range(len(f)):                      # in atom order
                tot = tot + f[i]
            f[a] = f[a] - tot
        return f[vib_idx].ravel()

    for r, (a, c) in enumerate(dof(vib_idx)):
        if nfree == 2:
            row = 0.5 * (F(a, c, -1) - F(a, c, +1))
        else:
            row = (-F(a, c, -2) + 8 * F(a, c, -1) - 8 * F(a, c, +1) + F(a, c, +2)) / 12.0
        K[r] = row / (2 * delta)
    return K


def hessian(force_fn, pos, vib_idx, delta=0.01, nfree=2, method="standard"):
    """H [m, m] in eV / A^2 (m = 3 len(vib_idx))."""
    K = rows(force_fn, pos, vib_idx, delta, nfree, method)
    return K + K.T


def mass_weighted(H, mass):
    """D H D; ``mass`` [m / 3]: the masses of the vib atoms."""
    im = np.repeat(np.asarray(mass, dtype=np.float64) ** -0.5, 3)
    return im[:, None] * H * im


def signed(v):
    """A vector with its largest-magnitude entry (the first on ties) made positive."""
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def modes(H, mass):
    """(energies [m] eV ascending, negative = imaginary; modes [m, m], rows = signed unit eigenvectors of D H D)."""
    if len(H) == 0:
        return np.zeros(0), np.zeros((0, 0))
    w2, V = np.linalg.eigh(mass_weighted(H, mass))
    return np.sign(w2) * S_UNIT * np.sqrt(np.abs(w2)), np.array([signed(v) for v in V.T])


def thermo(energies, T=0.0, e_min=0.0):
    """(zpe, f_vib, n_imag, n_left_out) over the modes with energy > e_min."""
    e = np.asarray(energies, dtype=np.float64)
    keep = e[e > e_min]
    zpe = 0.5 * keep.sum()
    f = zpe if T == 0 else float(np.sum(keep / 2 + KB * T * np.log1p(-np.exp(-keep / (KB * T)))))
    return float(zpe), float(f), int((e < 0).sum()), int(len(e) - len(keep))
