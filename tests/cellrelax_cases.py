"""Inputs of tests/test_cellrelax_cpu.py and tests/test_cellrelax_gpu.py (test infrastructure): 8- to 32-atom periodic cells for the
variable-cell relaxation, every one chosen with tests/cellrelax_oracle.py on the CPU (the CPU test rehearses the lj/cut ones under the
exact pair virial: which stop reason each ends with, and that reason 4 occurs only where it is wanted).

Two one-type lj/cut models (eps 0.1 eV, sigma 2.6 A, unshifted): ``LJ`` with rc = 6.5 A for everything but the thin cell, and
``LJ_THIN`` with rc = 7.9 A, under which the 4.03 A high fcc cell scans 2 images along its short axes and a third one as soon as a
height falls below 3.95 A -- 2 % of compression."""

import numpy as np

import pair_cases as pc

LJ = [(0, 0, "lj/cut", (0.1, 2.6), 6.5, 0)]
LJ_THIN = [(0, 0, "lj/cut", (0.1, 2.6), 7.9, 0)]
LJ_A0 = 4.029                    # A: near the fcc minimum of the rc = 6.5 A model (rehearsed in tests/test_cellrelax_cpu.py)
PBC3 = np.ones(3, np.uint8)
SKEW = np.array([[1.0, 0.0, 0.0], [0.06, 1.0, 0.0], [0.03, -0.05, 1.0]])   # lower triangular: a skewed, right-handed triclinic cell

FCC = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])


def fcc(reps, a=LJ_A0, sigma=0.0, seed=0, skew=False):
    """fcc ``reps`` = (nx, ny, nz) conventional cells: (types, positions, cell, pbc); ``sigma``: rattle in A; ``skew``: the cell sheared."""
    reps = np.asarray(reps)
    shifts = np.array([[x, y, z] for x in range(reps[0]) for y in range(reps[1]) for z in range(reps[2])], float)
    frac = (FCC[None] + shifts[:, None]).reshape(-1, 3) / reps
    cell = np.diag(a * reps.astype(float))
    if skew:
        cell = cell @ SKEW
    X = frac @ cell + np.random.default_rng(seed).normal(0, sigma, frac.shape)
    return np.zeros(len(X), np.int32), X, cell, PBC3.copy()


def mixed_batch():
    """Three different chains: 8, 16 and 32 atoms, skewed, rattled, off their lattice constant."""
    return [fcc((2, 1, 1), 4.10, 0.05, 1, True), fcc((2, 2, 1), 3.95, 0.08, 2, True), fcc((2, 2, 2), 4.06, 0.05, 3, True)]


def pressure_case():
    """16 atoms, skewed and rattled, under p = 0.02 eV / A^3 (3.2 GPa): compresses by about 1.5 % in length."""
    return fcc((2, 2, 1), LJ_A0, 0.03, 4, True), 0.02


def compressing_cube():
    """32 atoms at a = 4.20 A: 54 neighbors within 6.5 A; the fifth shell (24 more) enters at a < 4.11 A on the way to 4.0 A."""
    return fcc((2, 2, 2), 4.20, 0.02, 5)


COMPRESS_SLOTS = 60              # slots per atom of the tight handle: above the 56 of the start, below the 80 of the end
ROOMY_SLOTS = 128                # and of the handle that never regrows


THIN_STEPS = 6


def thin_case():
    """(the thin 8-atom cell under LJ_THIN, a neighbour, pressure): the first leaves its image range after three steps; the neighbour,
    the same cell started at a = 4.25 A, is still above 3.95 A after THIN_STEPS steps (every fcc cell crosses under this pressure in the end)."""
    return fcc((2, 1, 1), LJ_A0, 0.02, 6), fcc((2, 1, 1), 4.25, 0.03, 7), 0.1


WALL_STEPS = 4                   # the wall chain's fourth step is the one it takes back; its neighbour takes all four


def wall_case():
    """(structure, held mask, terms, cutoff): eight type-1 atoms, fcc at a = 4.25 A, and one type-0 atom 0.62 A from the first of them,
    both held, under neb_cases.WALL_TERMS: the 0 - 1 term overflows below 0.6 A.  The cell shrinks towards a = 4.03 A and carries the
    held pair along; at 3.3 % of compression an evaluation is not finite -- before any height reaches the 5.9 % that would need
    another image under the 8 A cutoff."""
    import neb_cases as nc

    T, X, C, pbc = fcc((2, 1, 1), 4.25, 0.02, 10)
    X = np.vstack([X, X[0] + [0.62, 0.0, 0.0]])
    held = np.zeros(9, np.uint8)
    held[0] = held[8] = 1
    return (np.concatenate([np.ones(8, np.int32), np.zeros(1, np.int32)]), X, C, pbc), held, nc.WALL_TERMS, 8.0


SLAB_MASK = (1, 1, 0, 0, 0, 1)


def slab():
    """fcc (100), 2 x 2 lateral cells and three layers (24 atoms), stretched in plane to 4.15 A, open along z in a 20 A cell."""
    a = 4.15
    pts = [[(i + bx) * a, (j + by) * a, 5.0 + k * 0.5 * LJ_A0] for k in range(3) for i in range(2) for j in range(2)
           for bx, by in (((0, 0), (.5, .5)) if k % 2 == 0 else ((.5, 0), (0, .5)))]
    X = np.array(pts) + np.random.default_rng(8).normal(0, 0.02, (24, 3))
    return np.zeros(24, np.int32), X, np.diag([2 * a, 2 * a, 20.0]), np.array([1, 1, 0], np.uint8)


# ---- step-for-step parity: one case per handle kind, three chains of 8, 12 and 27 atoms on the jittered grid of pair_cases.grid_chain in
# its skewed triclinic cell, at a spacing near the kind's nearest-neighbor distance ------------------------------------------------------
PARITY_KINDS = ("pair_lj", "sw", "tersoff", "eam_alloy", "adp", "vashishta")
PARITY_SHAPE = {"pair_lj": (2, 2.9), "sw": (1, 2.5), "tersoff": (2, 1.95), "eam_alloy": (2, 2.7), "adp": (2, 2.7), "vashishta": (2, 1.9)}
PARITY_SIZES = (8, 12, 27)
PARITY = dict(max_steps=8, fmax=1e-4)
PARITY_JITTER = 0.1


def parity_structs(kind):
    nt, spacing = PARITY_SHAPE[kind]
    return [pc.grid_chain(n, 60 + k, [1, 1, 1], n_types=nt, spacing=spacing, jitter=PARITY_JITTER) for k, n in enumerate(PARITY_SIZES)]


def parity_engine(kind, golden):
    import adp_oracle as adp
    import cg_resident_cases as rc
    import vib_cases as vc
    from surface_sampling_amd import backend, eam

    if kind == "adp":
        return backend.EAMEngine(eam.tables_from_adp(eam.parse_adp(eam.write_adp(adp.cuau_adp(*rc._funcfl()))), ["Cu", "Au"]), device=0)
    if kind == "vashishta":
        import vashishta_oracle as vo

        return backend.VashishtaEngine(vo.sic_params()[1], device=0)
    return vc.engine(kind, golden)


def parity_cutoff(kind, golden):
    """The cutoff the handle of ``parity_engine`` searches neighbors with (what decides the image counts)."""
    import cg_resident_cases as rc

    if kind == "pair_lj":
        return 8.0
    if kind == "tersoff":
        P = golden.tersoff_params
        return float((P[..., 10] + P[..., 11]).max())
    if kind == "vashishta":
        import vashishta_oracle as vo

        return float(vo.cutoff(vo.sic_params()[1]))
    if kind == "adp":
        return float(rc.eam_tables("eam_alloy").cutoff)
    return rc.cutoff(kind)


def painn_struct():
    """Cubic SrTiO3, 2 x 2 x 1 cells of a = 3.905 A (20 atoms), sheared and rattled."""
    a = 3.905
    base = [(38, (0, 0, 0)), (22, (.5, .5, .5)), (8, (.5, .5, 0)), (8, (.5, 0, .5)), (8, (0, .5, .5))]
    Z, frac = [], []
    for i in range(2):
        for j in range(2):
            for z, f in base:
                Z.append(z)
                frac.append(((f[0] + i) / 2, (f[1] + j) / 2, f[2]))
    cell = np.diag([2 * a, 2 * a, a]) @ SKEW
    X = np.array(frac) @ cell + np.random.default_rng(9).normal(0, 0.05, (20, 3))
    return np.array(Z, np.int32), X, cell, PBC3.copy()


def permuted(struct, seed):
    """(the structure with its atoms in another order, the permutation): row k of the result is row perm[k] of the input."""
    T, X, C, pbc = struct
    perm = np.random.default_rng(seed).permutation(len(T))
    return (T[perm], X[perm], C, pbc), perm
