"""Inputs of tests/test_vib_gpu.py and their CPU rehearsal in tests/test_vib_cpu.py (test infrastructure).  Structures are
``(types, positions, cell, pbc)``; masks are per-structure index lists of the atoms that vibrate."""
import numpy as np

import cg_cases as cc
import cg_resident_cases as rc
import pair_cases as pc
import pair_oracle as po
import vib_oracle as vo

TYPE_MASS = np.array([26.9815385, 63.546, 107.8682])
WANT = 1 | 2 | 16   # energy, forces, per-atom energies
BOX = np.eye(3) * 40.0
OPEN = np.zeros(3, np.uint8)

# ---- the Morse dimer of the physics anchor ---------------------------------------------------------------------------------------------
MORSE_D, MORSE_A, MORSE_R0 = 0.5, 1.8, 2.2
MORSE_MASS = np.array([15.999, 1.008])
MORSE_TERMS = [(0, 1, "morse", (MORSE_D, MORSE_A, MORSE_R0), 8.0, 0)]
MORSE_COMMANDS = ["pair_style morse 8.0", f"pair_coeff * * {MORSE_D} {MORSE_A} {MORSE_R0}"]


def morse_top_mode():
    """s sqrt(2 D a^2 / mu): 0.11951050758 eV."""
    mu = MORSE_MASS[0] * MORSE_MASS[1] / MORSE_MASS.sum()
    return vo.S_UNIT * np.sqrt(2 * MORSE_D * MORSE_A ** 2 / mu)


def morse_dimer():
    """O - H at the Morse minimum along (1, 0.2, 0.12).  The truncation error of Cartesian displacements depends on the bond's
    orientation (relative error of the top mode at nfree = 2, delta = 0.01: 1.89e-4 along an axis, 1.5e-5 along the body diagonal);
    this orientation gives the 1.63e-4, 4.08e-5 (delta = 0.005) and -4.2e-8 (nfree = 4) the tests pin."""
    u = np.array([1.0, 0.2, 0.12])
    pos = np.array([[15.0, 15.2, 14.9], [15.0, 15.2, 14.9] + MORSE_R0 * u / np.linalg.norm(u)])
    return np.array([0, 1], np.int32), pos, BOX, OPEN


def pair_force_fn(terms, struct):
    """The numpy restatement of a pair handle (tests/pair_oracle.py) as force function of one structure."""
    T, _, cell, pbc = struct
    return lambda p: po.pair(terms, None, T, p, cell, pbc)[2]


def masses(structs):
    return np.concatenate([TYPE_MASS[np.asarray(s[0]) % 3] for s in structs])


def start(structs):
    return np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])]).astype(np.int64)


def mask_of(structs, idx):
    """uint8 [sum N] from the per-structure index lists."""
    out = [np.zeros(len(s[0]), np.uint8) for s in structs]
    for m, ix in zip(out, idx):
        m[np.asarray(ix, dtype=np.int64)] = 1
    return np.concatenate(out)


def repeat(structs, idx, n_rep):
    """The batch with structure g present n_rep[g] times: (structures, index lists)."""
    S, I = [], []
    for s, ix, n in zip(structs, idx, n_rep):
        S += [s] * n
        I += [ix] * n
    return S, I


# ---- A: assembly -------------------------------------------------------------------------------------------------------------------------
ASSEMBLY_KINDS = ("pair_lj", "tersoff", "sw", "eam_alloy")
ASSEMBLY_SIZES = (1, 2, 3, 65, 2)
ASSEMBLY_MASK65 = (0, 7, 31, 32, 64)


def engine(kind, golden=None):
    from surface_sampling_amd import backend

    if kind == "tersoff":
        return backend.TersoffEngine(golden.tersoff_params, device=0)
    return rc.engine(kind)


def assembly_batch(kind):
    """Chains of 1, 2, 3 and 65 atoms (the last periodic in x and y) and a 2-atom chain whose mask is empty: m = 3, 6, 9, 15, 0."""
    def grid(n, seed, pbc):
        if kind == "tersoff":
            return pc.grid_chain(n, seed, pbc, n_types=2, spacing=1.95, jitter=0.1)
        return rc.grid(kind, n, seed, pbc)

    structs = [grid(n, 60 + k, [1, 1, 0] if n == 65 else [0, 0, 0]) for k, n in enumerate(ASSEMBLY_SIZES)]
    idx = [[0], [0, 1], [0, 1, 2], list(ASSEMBLY_MASK65), []]
    return structs, idx


def restatement_force_fn(kind, struct, golden=None, oracle_mod=None):
    """The numpy / CPU restatement of the kind's potential as force function of one structure (the rehearsal of the assembly cases)."""
    T, _, cell, pbc = struct
    if kind == "pair_lj":
        return lj_force_fn(struct)
    if kind == "tersoff":
        return lambda p: oracle_mod.tersoff(golden.tersoff_params, T, p, cell, pbc)[2]
    if kind == "sw":
        import sw_oracle as so

        P = so.si_params()
        return lambda p: so.sw(P, T, p, cell, pbc)[2]
    import eam_alloy_oracle as ao

    tab = rc.eam_tables(kind)
    return lambda p: ao.eam_typed(tab, T, p, cell, pbc)[2]


# ---- B: replicas -------------------------------------------------------------------------------------------------------------------------
LJ00 = (1.0, 2.6, 8.0)       # the type 0 - type 0 term of cg_cases.LJ_TERMS
REPLICA_MASK = (0, 5, 13, 26)
REPLICA_COUNTS = (1, 5, 12, 16)


def lj_cluster(n, seed, spacing=2.95, jitter=0.03):
    """n type-0 atoms of a jittered simple cubic grid near the lj/cut minimum, in an open box."""
    side = int(np.ceil(n ** (1 / 3) - 1e-9))
    g = np.array([[x, y, z] for z in range(side) for y in range(side) for x in range(side)], float)[:n] * spacing
    pos = g + np.random.default_rng(seed).normal(0, jitter, g.shape) + 12.0
    return np.zeros(n, np.int32), pos, BOX, OPEN


def replica_structs():
    """The 27-atom cluster with its 4-atom mask, and a second, different structure (16 atoms, 2 vib atoms) for the (3, 2) batch."""
    return [lj_cluster(27, 3), lj_cluster(16, 4, spacing=3.05)], [list(REPLICA_MASK), [2, 9]]


def idle_replicas(m, n_rep):
    """Ranks that never get a degree of freedom."""
    return [k for k in range(n_rep) if k >= m]


def evaluations(ms, n_rep, nfree):
    """Lock-step evaluations the call needs: nfree (largest share of a replica) + 1."""
    return nfree * max([-(-m // n) for m, n in zip(ms, n_rep) if m] + [0]) + 1


# ---- C: eigen-solve ----------------------------------------------------------------------------------------------------------------------
EIGEN_SIZES = (1, 2, 3, 32, 85)        # m = 3, 6, 9 (odd: the tournament plays with an idle seat), 96, 255


def eigen_batch():
    structs = [lj_cluster(n, 20 + k) for k, n in enumerate(EIGEN_SIZES)]
    return structs, [list(range(n)) for n in EIGEN_SIZES]


def too_many():
    """86 atoms: 258 degrees of freedom, the smallest count beyond the 256 of the eigen-solver."""
    return lj_cluster(86, 29)


# ---- F: robustness -----------------------------------------------------------------------------------------------------------------------
TIGHT_SLOTS_PER_ATOM = 5
TIGHT_DELTA = 0.3


def tight_cluster():
    """27 atoms on a 4.0 A grid under the 8 A cutoff: second neighbors along the axes sit at the cutoff, so displacements of 0.3 A
    move pairs across it, and 5 slots per atom hold none of it."""
    return lj_cluster(27, 11, spacing=4.0, jitter=0.05)


def slots(pos, rc_=8.0):
    """(padded slots, real edges) of an open chain: every row padded to a multiple of 4."""
    d = pos[None] - pos[:, None]
    deg = ((d * d).sum(axis=2) < rc_ * rc_).sum(axis=1) - 1
    return int(((deg + 3) & ~3).sum()), int(deg.sum())


COLLIDE_DELTA = 0.25


def colliding_dimer():
    """Two atoms COLLIDE_DELTA apart along x and 1e-150 A apart along y: the +delta displacement of atom 0 along x (and the -delta
    one of atom 1) leaves them 1e-150 A apart -- exactly coincident atoms are no neighbors, these are, and lj/cut overflows."""
    pos = np.array([[15.0, 0.0, 15.0], [15.0 + COLLIDE_DELTA, 1e-150, 15.0]])
    return np.zeros(2, np.int32), pos, BOX, OPEN


def collide_batch():
    """The colliding dimer between two harmless chains."""
    return [lj_cluster(8, 31), colliding_dimer(), lj_cluster(3, 32)], [[0, 3], [0, 1], [0, 1, 2]]


def lj_force_fn(struct):
    return pair_force_fn(cc.LJ_TERMS, struct)
