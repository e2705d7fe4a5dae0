"""Inputs of the slab Ewald tests (test infrastructure), shared by the device tests (tests/test_ewald_slab_gpu.py) and their CPU
rehearsal (tests/test_ewald_slab_cpu.py).  Structures are ``(types, positions, cell, pbc)`` with pbc (1, 1, 0), a and b in the xy
plane and c along z; models are command lines for ``surface_sampling_amd.pair.parse``.  Types: 0 = cation +1, 1 = anion -1,
2 = cation +2 (tests/ewald_cases.py)."""
import numpy as np

import ewald_cases as ec
import pair_oracle as po

PBC = np.array([1, 1, 0], np.uint8)
F = 3.0
HEAD = ["units metal", "boundary p p f"]


def slab_lines(lines, factor=F):
    """The commands of a 3-D Ewald model of tests/ewald_cases.py as a slab model: boundary p p f in front, kspace_modify slab F."""
    out = HEAD + list(lines)
    k = next(n for n, ln in enumerate(out) if ln.startswith("kspace_style"))
    return out[:k + 1] + [f"kspace_modify slab {factor}"] + out[k + 1:]


# the model of the parity, invariance and reproducibility cases: bare Coulomb, rc = 10 A, A = 1e-8 -> g = 0.4292, k_cut = 3.684 1/A,
# below 63 * 2 pi / 101.52 = 3.899 1/A, the largest k_cut the thin tall cell admits at F = 3
MODEL = slab_lines(ec.coul(10.0, 1e-8))


def dipolar8():
    """Eight ions of a rocksalt cell under vacuum (5.64 x 5.64 x 12 A), rattled, every cation 0.35 A above its plane: neutral, M != 0."""
    T, X, _ = po.rocksalt(5.64)
    X = X + [0.0, 0.0, 4.0] + np.random.default_rng(41).normal(0, 0.05, X.shape)
    X[T == 0, 2] += 0.35
    return T.copy(), X, np.diag([5.64, 5.64, 12.0]), PBC


def charged8():
    """dipolar8 with its first cation of type 2 (+2): total charge +1."""
    T, X, C, pbc = dipolar8()
    T[0] = 2
    return T, X, C, pbc


SKEW_CELL = np.array([[6.0, 0.0, 0.0], [1.5, 5.5, 0.0], [0.0, 0.0, 11.0]])


def skewed8():
    """Eight ions on rocksalt-like sites of a cell skewed in the plane, z in [2.5, 8], the first one +2: total charge +1."""
    T, X, _ = po.rocksalt(1.0)
    X = X @ np.array([[6.0, 0.0, 0.0], [1.5, 5.5, 0.0], [0.0, 0.0, 5.5]]) + [0.0, 0.0, 2.5]
    X = X + np.random.default_rng(42).uniform(-0.25, 0.25, X.shape)
    T = T.copy()
    T[0] = 2
    return T, X, SKEW_CELL.copy(), PBC


def single():
    """One +1 ion in a 6 x 7 x 12 A cell."""
    return np.array([0], np.int32), np.array([[1.0, 2.0, 3.0]]), np.diag([6.0, 7.0, 12.0]), PBC


def big(n):
    """The first n of: rocksalt 2 x 2 x 2 (64 ions) with six adsorbed ions (4 cations, 2 anions) on top, in a cell with 8 A of vacuum."""
    T, X, C, _ = ec.slab70()
    return T[:n].copy(), X[:n] + [0.0, 0.0, 1.0], C, PBC


def thin32():
    """32 ions (rocksalt 1 x 1 x 4, 22.6 A tall) in a 5.64 x 5.64 x 33.84 A cell: extended to 101.5 A, many l rows, a small atom tile."""
    T, X, _ = po.rocksalt(5.64)
    T = np.concatenate([T] * 4).astype(np.int32)
    X = np.concatenate([X + [0, 0, 5.64 * k] for k in range(4)]) + [0.0, 0.0, 3.0]
    return T, X + np.random.default_rng(43).normal(0, 0.05, X.shape), np.diag([5.64, 5.64, 33.84]), PBC


SHIFT_Z = 0.9


def in_plane_shift(cell):
    return 2.3 * cell[0] - 1.7 * cell[1]


def below_and_outside():
    """charged8 moved down to negative z and out of the cell in the plane (nothing wrapped)."""
    T, X, C, pbc = charged8()
    return T, X + in_plane_shift(C) + [0.0, 0.0, -7.5], C, pbc


def lefthanded8():
    """charged8 in the same cell with rows a and b exchanged: det cell < 0, the kernels' normal a x b / det points along -z."""
    T, X, C, pbc = charged8()
    return T, X, C[[1, 0, 2]].copy(), pbc


# the ragged batch of the device tests: name, builder
RAGGED = [("dipolar8", dipolar8), ("charged8", charged8), ("skewed8", skewed8), ("single", single), ("big63", lambda: big(63)),
          ("big64", lambda: big(64)), ("big65", lambda: big(65)), ("big70", lambda: big(70)), ("thin32", thin32),
          ("below_and_outside", below_and_outside), ("lefthanded8", lefthanded8)]


def ext_bounds(cell, k_cut, factor=F):
    """Per-axis bounds of the extended cell, as csrc/ewald_dev.h takes them."""
    cell = np.asarray(cell, np.float64)
    return tuple(int(k_cut * np.linalg.norm(cell[a]) * (factor if a == 2 else 1.0) / (2.0 * np.pi)) for a in range(3))


# stress: born/coul/long at A = 1e-12; the cutoffs keep every pair 0.01 A away (asserted in both test files)
STRESS = [("neutral", dipolar8, 8.05), ("charged", skewed8, 8.42)]


def relax16():
    """Two rocksalt layers of 8 ions (11.28 x 5.64 A in the plane) under vacuum, rattled; the bottom layer (the first 8) is held."""
    T, X, _ = po.rocksalt(5.64)
    keep = X[:, 2] < 2.0
    T1, X1 = T[keep], X[keep]
    T2, X2 = T[~keep], X[~keep]
    Tl = np.concatenate([T1, T1, T2, T2]).astype(np.int32)
    Xl = np.concatenate([X1, X1 + [5.64, 0, 0], X2, X2 + [5.64, 0, 0]]) + [0.0, 0.0, 3.0]
    Xl[8:] += np.random.default_rng(44).normal(0, 0.08, (8, 3))
    fixed = np.arange(16) < 8
    return (Tl, Xl, np.diag([11.28, 5.64, 14.0]), PBC), fixed
