"""Inputs of the pair-potential tests (test infrastructure), shared by the device tests (tests/test_pair_gpu*.py) and their CPU
rehearsals (tests/test_pair_cpu.py): every input is built here once, and what a device test presumes about it -- the degree of
every centre, the distance of every pair from every cutoff -- is asserted on the CPU from the same object.

Structures are ``(types, positions, cell, pbc)``; models are command lines for ``surface_sampling_amd.pair.parse``."""
import numpy as np

import cell_cases as cc

OPEN = np.zeros(3, np.uint8)

OVERLAY5 = ["pair_style hybrid/overlay lj/cut 6.0 morse 5.0 buck 7.0 born 6.5 coul/dsf 0.25 9.0",
            "pair_coeff 1 1 lj/cut 0.02 2.6", "pair_coeff 2 2 lj/cut 0.03 2.8", "pair_coeff 1 2 morse 0.2 1.4 2.6",
            "pair_coeff 1 3 buck 900.0 0.29 25.0", "pair_coeff 2 3 born 0.4 0.3 2.7 20.0 30.0", "pair_coeff 3 3 lj/cut 0.01 3.0",
            "pair_coeff * * coul/dsf", "pair_modify shift yes",
            "set type 1 charge 0.8", "set type 2 charge 0.4", "set type 3 charge -1.2"]


def grid_chain(n, seed, pbc, n_types=3, spacing=2.7, jitter=0.15):
    """n atoms on a jittered grid in a skewed cell; open axes get 12 A of vacuum: (types, positions, cell, pbc)."""
    rng = np.random.default_rng(seed)
    nx = int(np.ceil(n ** (1 / 3)))
    ny = int(np.ceil(np.sqrt(n / nx)))
    nz = int(np.ceil(n / (nx * ny)))
    pts = np.array([[x, y, z] for z in range(nz) for y in range(ny) for x in range(nx)], float)[:n]
    lens = np.array([nx, ny, nz], float) * spacing + np.where(np.asarray(pbc, bool), 0.0, 12.0)
    cell = np.diag(lens) + np.array([[0, 0, 0], [0.9, 0, 0], [0.4, -0.6, 0]]) * np.asarray(pbc, float)[:, None]
    X = (pts + 0.25) * spacing + rng.normal(0, jitter, (n, 3))
    return rng.permutation(np.arange(n) % n_types).astype(np.int32), X, cell, np.asarray(pbc, np.uint8)


def degrees(struct, rc):
    """Slots per centre: the directed edges (images included) within rc, from the brute-force enumeration."""
    T, X, C, pbc = struct
    i, _, _, _ = cc.brute_neighbors(X, C, pbc, rc)
    return np.bincount(i, minlength=len(T))


def cutoff_margin(model, struct):
    """Smallest | |r_ij| - rc | over the model's terms and the pairs of their types."""
    T, X, C, pbc = struct
    i, j, _, rv = cc.brute_neighbors(X, C, pbc, model.cutoff + 0.5)
    d, ti, tj = np.linalg.norm(rv, axis=1), T[i], T[j]
    out = np.inf
    for t in model.terms:
        on = ((ti == t.type_a) & (tj == t.type_b)) | ((ti == t.type_b) & (tj == t.type_a))
        if on.any():
            out = min(out, np.abs(d[on] - t.rc).min())
    return out


# -- 1: row shapes -------------------------------------------------------------------------------------------------------------------
ROWS_RC = 4.0
ROWS_MODEL = ["pair_style hybrid/overlay lj/cut 4.0 coul/dsf 0.25 4.0",
              "pair_coeff 1 1 lj/cut 0.02 2.3", "pair_coeff 2 2 lj/cut 0.03 2.1", "pair_coeff 1 2 lj/cut 0.025 2.2",
              "pair_coeff * * coul/dsf", "set type 1 charge 0.7", "set type 2 charge -0.5"]
ROWS_DEGREES = [0, 1, 1, 1, 2, 1, 3, 1, 1, 1, 4, 1, 1, 1, 1, 5, 4, 4, 4, 4, 5, 9, 6, 6, 6, 6, 3, 3, 3, 3, 5]


def rows_cluster():
    """31 atoms of two types in a 30 A open box, placed by hand 2.5 A apart in seven groups more than 4 A from each other: a lone
    atom, a dimer, a straight trimer, a planar and a tetrahedral star (leaves more than 4 A apart), a square pyramid about its
    centre and a flat 3 x 3 grid with an apex.  With the 4 A cutoff the rows have 0, 1, 2, 3, 4, 5, 6 and 9 slots (ROWS_DEGREES):
    rows shorter than, equal to and one longer than the four lanes of a centre, and one of two full passes and a rest."""
    a, t = 2.5, 2.5 / np.sqrt(3.0)
    x, y, z = np.eye(3) * a
    o = np.zeros(3)
    groups = [
        [o],
        [o, x],
        [-x, o, x],
        [o] + [a * np.array([np.cos(w), np.sin(w), 0.0]) for w in np.deg2rad([0.0, 120.0, 240.0])],
        [o] + [t * np.array(v, float) for v in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))],
        [o, x, -x, y, -y, z],
        [o, x, -x, y, -y, x + y, x - y, -x + y, -x - y, z],
    ]
    at = [(5, 5, 5), (15, 5, 5), (25, 5, 5), (5, 15, 5), (15, 15, 5), (25, 15, 5), (15, 25, 15)]
    X = np.concatenate([np.asarray(g) + np.asarray(c, float) for g, c in zip(groups, at)])
    return (np.arange(len(X)) % 2).astype(np.int32), X, np.eye(3) * 30.0, OPEN


def rows_batch():
    """The cluster, a 65-atom fully periodic chain and a 63-atom slab chain, in that order: the first 64-centre workgroup holds the
    cluster and the head of the 65-atom chain (two cells), the 65-atom chain spans two workgroups, and so does the last chain."""
    return [rows_cluster(), grid_chain(65, 51, [1, 1, 1], n_types=2), grid_chain(63, 52, [1, 1, 0], n_types=2)]


# -- 2: table addressing ---------------------------------------------------------------------------------------------------------------
def table_lines(nt):
    """hybrid/overlay commands for nt types in which the coefficients of every unordered pair (a, b) differ by a formula in (a, b)
    and the single-term pairs cycle through lj/cut, morse, buck and born; the pairs (1, nt), (nt, nt) and (4, 5) carry three terms
    -- lj/cut, morse and coul/dsf, each with its own cutoff.  All charges differ."""
    lines = ["pair_style hybrid/overlay lj/cut 5.5 morse 5.0 buck 6.0 born 5.8 coul/dsf 0.3 6.5"]
    triple = {(1, nt), (nt, nt), (4, 5)}
    for a in range(1, nt + 1):
        for b in range(a, nt + 1):
            u, v = 0.01 * a, 0.013 * b
            lj = f"pair_coeff {a} {b} lj/cut {0.01 + u + 0.5 * v:.4f} {2.3 + 3 * u + v:.4f} {5.1 + 3 * u + 2 * v:.4f}"
            mo = f"pair_coeff {a} {b} morse {0.05 + 2 * u + v:.4f} {1.2 + 2 * u + 3 * v:.4f} {2.5 + 3 * v + u:.4f} {4.4 + 2 * u + 3 * v:.4f}"
            if (a, b) in triple:
                lines += [lj, mo, f"pair_coeff {a} {b} coul/dsf"]
                continue
            lines.append([lj, mo,
                          f"pair_coeff {a} {b} buck {700 + 4000 * u + 3000 * v:.1f} {0.27 + 0.3 * u + 0.2 * v:.4f} {15 + 100 * u + 150 * v:.2f} {5.6 + 2 * u + v:.4f}",
                          f"pair_coeff {a} {b} born {0.3 + 2 * u + v:.4f} {0.29 + 0.2 * u + 0.3 * v:.4f} {2.5 + 2 * u + 3 * v:.4f} {12 + 100 * u + 80 * v:.2f}"
                          f" {20 + 150 * u + 100 * v:.2f} {5.3 + u + 3 * v:.4f}"][(a + 2 * b) % 4])
    lines += [f"set type {a} charge {(-1) ** a * (0.3 + 0.11 * a):.2f}" for a in range(1, nt + 1)]
    return lines


def table_chain(nt):
    """The 40-atom jittered grid, every type present, periodic in x and y (seeds that leave every pair more than 0.005 A from its
    terms' cutoffs, so that the strain derivative of the unshifted energy is defined)."""
    return grid_chain(40, {8: 64, 5: 68}[nt], [1, 1, 0], n_types=nt)


def swap_types(struct, a, b):
    T, X, C, pbc = struct
    T2 = T.copy()
    T2[T == a], T2[T == b] = b, a
    return T2, X, C, pbc


# -- 3: the cutoff decision ----------------------------------------------------------------------------------------------------------
CUT_BOX = np.eye(3) * 20.0
CUT_LJ = ["pair_style lj/cut 6.0", "pair_coeff 1 1 0.0104 3.4", "pair_modify shift no"]
CUT_OVERLAY = ["pair_style hybrid/overlay lj/cut 5.0 morse 6.0", "pair_coeff 1 1 lj/cut 0.0104 3.4", "pair_coeff 1 1 morse 0.3 1.0 2.4",
               "pair_modify shift no"]
CUT_DSF = ["pair_style coul/dsf 0.2 6.0", "pair_coeff * *", "set type 1 charge 1.0"]


def cutoff_dimers(rc):
    """Three dimers on the x axis of a 20 A open box, the first atom at x = 1, the second at x = 1 + rc and at its two fp64
    neighbours: separations one ulp inside rc, exactly rc and one ulp outside (rc = 5 or 6: the coordinates, their difference and
    the difference's neighbours are all exact in binary).  Returns (structures, separations)."""
    far = np.float64(1.0 + rc)
    xs = [np.nextafter(far, 0.0), far, np.nextafter(far, 100.0)]
    structs = [(np.zeros(2, np.int32), np.array([[1.0, 3.0, 3.0], [x, 3.0, 3.0]]), CUT_BOX, OPEN) for x in xs]
    return structs, np.array([x - 1.0 for x in xs])


# -- 4: relaxations --------------------------------------------------------------------------------------------------------------------
RELAX_SHAPES = ((7, [1, 1, 1]), (16, [1, 1, 0]), (23, [1, 0, 0]))
RELAX_SEEDS = (40, 41, 42)
STRESS_SEEDS = (52, 45, 41)      # after 12 FIRE steps no pair of these lies within 0.005 A of a cutoff (restated on the CPU)


def relax_batch(seeds=RELAX_SEEDS):
    """Three ragged, charged, three-type chains for OVERLAY5 and the mask holding the first two atoms of each."""
    chains = [grid_chain(n, seed, pbc) for seed, (n, pbc) in zip(seeds, RELAX_SHAPES)]
    return chains, held_mask(chains)


def held_mask(chains):
    return np.concatenate([(np.arange(len(c[0])) < 2) for c in chains]).astype(np.uint8)
