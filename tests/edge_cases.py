"""Inputs that sit where the fp64 many-body kernels have special code: cutoff and taper edges, the ``exp`` clamps of Tersoff, the
end of the EAM tables (tests/test_potential_edges_cpu.py asserts on the CPU what tests/test_potential_edges_gpu.py presumes).

TEST INFRASTRUCTURE ONLY.  Every input is built here once, from fixed numbers.  Structures are (types, positions, cell, pbc); every
chain has at most 100 atoms, every batch at most 8 chains.

Edge pairs are dimers, or a cluster centre and a neighbour, on the x or z axis with the first atom at x = z = 0, so that the
separation is one coordinate: the neighbour search (d^2 <= rc^2, csrc/nbr_dev.h), the kernels (sqrt(d . d) against the bound) and
the restatements all see exactly the distance written here -- sqrt(fl(d d)) = d in IEEE binary arithmetic.  The dimers and clusters
of one chain lie 25 A apart along y (beyond every cutoff), free boundaries.

The EAM restatement of this module (``eam_mut``) is tests/eam_alloy_oracle.py with the two places named in ``EAM_MUTATIONS`` made
switchable (the cutoff defects need no switch: ``with_cutoff``); unmutated it is compared with the existing oracles on the CPU, and
the device is compared with those oracles, never with this one.
"""

from __future__ import annotations

import dataclasses
import os

import numpy as np

import eam_alloy_oracle as ao
from eam_oracle import build_spline, spline_eval

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
APART = 25.0                     # spacing of the dimers / clusters of a chain: beyond every cutoff in this module
MIN_TERMS = 8                    # every named branch is entered by at least this many terms
FRAGMENT_A = 2.3                 # lattice constant of the free fcc fragments (Cu: 3.615): their cores sit beyond the F tables
SW_SEED = 11

# Bounds of the device tests of the same kernels, scaled by max|F| / max|pe| as tests/test_gpu_parity.py scales the Tersoff ones
# (compressed states have forces of hundreds of eV / A):  |dE| <= E (max(1, |E|)), |d pe/atom| <= EA max(1, max|pe|),
# |dF| <= F max(1, max|F|).
TERSOFF_TOL = {"E": 1e-9, "EA": 1e-9, "F": 1e-8}      # tests/test_gpu_parity.py
EAM_TOL = {"E": 1e-9, "EA": 1e-9, "F": 1e-8}          # tests/test_eam_alloy_gpu.py, tests/test_adp_gpu.py
SW_TOL = {"E": 1e-10, "EA": 1e-9, "F": 1e-8}          # tests/test_sw_gpu.py
VASHISHTA_TOL = {"E": 1e-10, "EA": 1e-9, "F": 1e-8}   # tests/test_vashishta_gpu.py


def up(x, k=1):
    """x moved k units in the last place towards +inf (k < 0: towards 0 for positive x)."""
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else 0.0)
    return float(x)


def dimer_chain(distances, types=(0, 0), copies=4, lone=0, lone_type=0):
    """``copies`` dimers at every distance of ``distances`` (first atom at x = 0, second at x = d, rows APART along y) and ``lone``
    isolated atoms, free boundaries.  Returns the structure and {distance: [(i, j), ...]}."""
    T, X, where = [], [], {}
    row = 0
    for d in distances:
        for _ in range(copies):
            where.setdefault(d, []).append((len(T), len(T) + 1))
            T += list(types)
            X += [[0.0, row * APART, 0.0], [d, row * APART, 0.0]]
            row += 1
    for _ in range(lone):
        T.append(lone_type)
        X.append([0.0, row * APART, 0.0])
        row += 1
    assert len(T) <= 100
    return (np.array(T, np.int32), np.array(X), np.eye(3) * (APART * (row + 2)), np.zeros(3, np.uint8)), where


# ======================================================================================================================================
# EAM (funcfl, typed alloy / fs / mixed funcfl) and ADP
# ======================================================================================================================================
EAM_EDGE_CUT = 4.5               # cutoff of the edge tables: exactly representable, in the middle of the shipped tables' range
EAM_MUTATIONS = ("no_linear", "fp_prev_interval")


def funcfl_pair():
    from surface_sampling_amd import eam

    return eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))


def edge_grid(nr, dr, cut=EAM_EDGE_CUT):
    """Points kept of an r table so that it ENDS 0.10 .. 0.12 A inside ``cut``: (nr' - 1) dr < cut, the clamped evaluation
    (m = nr' - 1, p = 1) serves the distances between the table end and the cutoff."""
    keep = int(np.floor((cut - 0.10) / dr)) + 1
    assert 5 <= keep < nr and (keep - 1) * dr < cut - 0.09
    return keep


def edge_funcfl(f, cut=EAM_EDGE_CUT):
    """The funcfl element with its r tables cut short and the cutoff at ``cut``: rho and r phi are far from zero at the cutoff
    (asserted in the rehearsal), and the cutoff lies beyond the last table point -- the host readers accept such a file."""
    keep = edge_grid(f.nr, f.dr, cut)
    return dataclasses.replace(f, nr=keep, cutoff=cut, zr=f.zr[:keep].copy(), rhor=f.rhor[:keep].copy())


def edge_tables(t, cut=EAM_EDGE_CUT):
    """The same cut of an eam.EamTables (u and w of an ADP set included)."""
    keep = edge_grid(t.nr, t.dr, cut)
    short = lambda a: None if a is None else np.ascontiguousarray(a[..., :keep])   # noqa: E731
    return dataclasses.replace(t, nr=keep, cutoff=cut, rhor=short(t.rhor), z2r=short(t.z2r), u=short(t.u), w=short(t.w))


def typed_forms():
    """{form: EamTables (Cu, Au)} through the file writers and readers -- the forms of tests/test_eam_alloy_gpu.py plus the ADP set of
    tests/test_adp_gpu.py."""
    import adp_oracle
    from surface_sampling_amd import eam

    cu, au = funcfl_pair()
    return {
        "alloy": eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au))), ["Cu", "Au"]),
        "fs": eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (0.7, 1.3))), fs=True), ["Cu", "Au"]),
        "funcfl": eam.tables_from_funcfl([cu, au]),
        "adp": eam.tables_from_adp(eam.parse_adp(eam.write_adp(adp_oracle.cuau_adp(cu, au))), ["Cu", "Au"]),
    }


def as_tables(f):
    """One funcfl element as EamTables (what ``eam_mut`` and ``eam_rho`` take)."""
    from surface_sampling_amd import eam

    if hasattr(f, "z2r"):
        return f
    return eam.EamTables(["X"], False, f.nrho, f.drho, f.nr, f.dr, f.cutoff, np.asarray(f.frho, float)[None, :].copy(),
                         np.asarray(f.rhor, float)[None, :].copy(), (eam.HARTREE_BOHR * np.asarray(f.zr, float) ** 2)[None, :])


def eam_edge_distances(t):
    """The named distances of a table with cutoff rc beyond its last point r_end = (nr - 1) dr."""
    rc, r_end = float(t.cutoff), (t.nr - 1) * t.dr
    return {"inside": up(rc, -1), "at": rc, "outside": up(rc, 1), "last_interval": r_end - 0.375 * t.dr,
            "beyond_table": 0.5 * (r_end + rc), "bulk": 2.5}


def eam_edge_chain(t, types=(0, 0)):
    """Four dimers at each named distance and eight isolated atoms (rho = 0: F(0), the lower end of the F table)."""
    d = eam_edge_distances(t)
    s, where = dimer_chain(list(d.values()), types=types, copies=4, lone=8, lone_type=types[1])
    return s, {k: where[v] for k, v in d.items()}


def compressed_slab(a=2.4, types_seed=None, sigma=0.03, seed=5):
    """fcc(100) slab at the lattice constant ``a`` (Cu: 3.615), 3 x 3 cells, 5 layers = 90 atoms, periodic in x and y, rattled.
    At a = 2.4 the inner layers sit above the end of the shipped F tables and the two surface layers below it."""
    pos, cell, pbc = ao.cu100_slab(3, 3, 5, a=a)
    pos = pos + np.random.default_rng(seed).normal(0, sigma, pos.shape)
    t = np.zeros(len(pos), np.int32) if types_seed is None else ao.random_alloy(pos, 0.3, types_seed)
    return t, pos, cell, pbc


def fcc_fragment(a=FRAGMENT_A, types_seed=None):
    """A free fcc fragment (pbc = 0): the 63 lattice points of 2 x 2 x 2 conventional cells.  Compressed, it expands under CG."""
    g = np.array([[i, j, k] for i in range(5) for j in range(5) for k in range(5) if (i + j + k) % 2 == 0], float)
    pos = g * (a / 2.0)
    t = np.zeros(len(pos), np.int32) if types_seed is None else ao.random_alloy(pos, 0.3, types_seed)
    return t, pos, np.eye(3) * 40.0, np.zeros(3, np.uint8)


def eam_rho(t, types, pos, cell, pbc):
    """Host electron density of every atom and the end of the F table."""
    return eam_mut(t, types, pos, cell, pbc)[3], (t.nrho - 1) * t.drho


def eam_mut(tab, types, pos, cell, pbc, mutate=None):
    """eam_alloy_oracle.eam_typed with switchable defects.  ``mutate``: None, "no_linear" (F clamped at the table end without the
    linear term), "fp_prev_interval" (F' of the continuation taken from the end of the interval before the last one).  Returns
    (E, e_atom, forces, rho)."""
    assert mutate is None or mutate in EAM_MUTATIONS
    types = np.asarray(types, np.int64)
    n_el = len(tab.frho)
    Fs = [build_spline(f, tab.drho) for f in tab.frho]
    Rs = [build_spline(f, tab.dr) for f in tab.rhor]
    Zs = [build_spline(f, tab.dr) for f in tab.z2r]
    ii, jj, rr = ao.neighbor_pairs(pos, cell, pbc, tab.cutoff)
    n = len(types)
    dist = np.sqrt((rr ** 2).sum(axis=1))
    ti, tj = types[ii], types[jj]
    r_ji, r_ij = (tj * n_el + ti, ti * n_el + tj) if tab.fs else (tj, ti)
    hi, lo = np.maximum(ti, tj), np.minimum(ti, tj)
    rho_e, drho_ji = ao._grouped(Rs, r_ji, dist, tab.dr, tab.nr)
    _, drho_ij = ao._grouped(Rs, r_ij, dist, tab.dr, tab.nr)
    z, dz = ao._grouped(Zs, hi * (hi + 1) // 2 + lo, dist, tab.dr, tab.nr)
    rho = np.zeros(n)
    np.add.at(rho, ii, rho_e)
    Fi, fp = np.zeros(n), np.zeros(n)
    rhomax = (tab.nrho - 1) * tab.drho
    for t in np.unique(types):
        m = types == t
        Fi[m], fp[m] = spline_eval(Fs[t], rho[m], tab.drho, tab.nrho, clamp_lo=True)
        if mutate == "fp_prev_interval":
            c = Fs[t][tab.nrho - 2]
            fp[m] = np.where(rho[m] > rhomax, c[0] + c[1] + c[2], fp[m])
    if mutate != "no_linear":
        Fi = Fi + np.where(rho > rhomax, fp * (rho - rhomax), 0.0)
    phi = z / dist
    phip = dz / dist - phi / dist
    e_atom = Fi.copy()
    np.add.at(e_atom, ii, 0.5 * phi)
    psip = fp[ii] * drho_ji + fp[jj] * drho_ij + phip
    forces = np.zeros((n, 3))
    np.add.at(forces, ii, (psip / dist)[:, None] * rr)
    return float(e_atom.sum()), e_atom, forces, rho


def with_cutoff(t, rc):
    """The table (or funcfl element) with another cutoff: the restatements use the cutoff only in ``dist < cutoff``, so
    ``with_cutoff(t, up(rc, -1))`` drops a pair one ulp inside and ``with_cutoff(t, up(rc, +2))`` keeps one one ulp outside."""
    return dataclasses.replace(t, cutoff=float(rc))


# ======================================================================================================================================
# clusters: one centre at (0, y0, 0), neighbours on the coordinate axes at exact distances, fillers around them
# ======================================================================================================================================
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1]], float)   # (not y: the clusters of a chain are stacked along y)
N_AXES = len(AXES)


def cluster(axis_d, axis_t, n_fill, fill_r, fill_t, centre_t, rng, min_sep=1.45):
    """Centre at the origin, one neighbour per entry of ``axis_d`` on the axes +x -x +z -z (its distance from the centre is EXACTLY
    axis_d[k]: one coordinate, the others zero), and ``n_fill`` fillers at radii drawn from ``fill_r`` = (lo, hi) with types
    drawn from ``fill_t``, no two atoms closer than ``min_sep``.  Returns (types, positions)."""
    X = [np.zeros(3)] + [AXES[k] * d for k, d in enumerate(axis_d)]
    T = [centre_t] + list(axis_t)
    while len(X) < 1 + len(axis_d) + n_fill:
        v = rng.normal(size=3)
        x = v / np.linalg.norm(v) * rng.uniform(*fill_r)
        if all(np.linalg.norm(x - y) >= min_sep for y in X):
            X.append(x)
            T.append(int(rng.choice(fill_t)))
    return np.array(T, np.int32), np.array(X)


def spread(places, c):
    """The N_AXES places cluster number c puts on its axes: consecutive clusters walk round the list, so every place is served
    equally often."""
    return [places[(c * N_AXES + a) % len(places)] for a in range(N_AXES)]


def cluster_chain(clusters):
    """Clusters stacked APART along y: the centres keep x = z = 0 and every axis neighbour shares its centre's y, so the separations
    stay the single coordinates written by ``cluster``."""
    T, X, centres = [], [], []
    for k, (t, x) in enumerate(clusters):
        centres.append(len(T))
        T += list(t)
        X += list(x + np.array([0.0, k * APART, 0.0]))
    assert len(T) <= 100
    return (np.array(T, np.int32), np.array(X), np.eye(3) * (APART * (len(clusters) + 2)), np.zeros(3, np.uint8)), centres


# ======================================================================================================================================
# Tersoff: a designed three-species table and clusters that enter both exp clamps, every ex path and both ends of the cutoff shell
# ======================================================================================================================================
TERSOFF_BOX_SEED = 2                 # found by search: see tersoff_clamp_box


def tersoff_edge_table():
    """P[i, j, k] in the field order of include/vssr_eval.h (m gamma lam3 c d h n beta lam2 B R D lam1 A).

    by the third species k   k = 0: m = 3, lam3 = 3.0  -> |arg| > 69.0776 once |rij - rik| > 1.368 A
                             k = 1: m = 1, lam3 = 80   -> |arg| > 69.0776 once |rij - rik| > 0.864 A
                             k = 2: lam3 = 0           (ex = 1 without exp)
    by the centre i          n = 1, 0.78734, 2.5       (the n == 1 branch of b_ij and the general one)
    by the neighbour j       beta = 1e-30, 1e-30, 1.0  with beta = 1e-30 a zeta of ~1e30 (the high clamp) gives beta zeta ~ 1: b_ij sits
                             in its n == 1 / general branch, so the VALUE 1e30 and dex = 0 both change E and F; with beta = 1 the clamp
                             only drives b_ij to 0
    R, D by the pair (i, k)  (0,0) 3.0 0.2 | (0,1) 2.7 0.15 | (1,1) 2.5 0.2 | (0,2) 2.4 0.1 | (1,2) 2.3 0.15 | (2,2) 2.1 0.1: a row
                             (every neighbour inside 3.2 A) holds neighbours beyond an entry's own cutoff
    """
    RD = {(0, 0): (3.0, 0.2), (0, 1): (2.7, 0.15), (1, 1): (2.5, 0.2), (0, 2): (2.4, 0.1), (1, 2): (2.3, 0.15), (2, 2): (2.1, 0.1)}
    P = np.zeros((3, 3, 3, 14))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                R, D = RD[min(i, k), max(i, k)]
                m, lam3 = ((3.0, 3.0), (1.0, 80.0), (3.0, 0.0))[k]
                P[i, j, k] = [m, 0.4 + 0.1 * i + 0.05 * k, lam3, 2.0 + 0.2 * j, 1.5 + 0.1 * k, -0.3 - 0.05 * i, (1.0, 0.78734, 2.5)[i],
                              (1e-30, 1e-30, 1.0)[j], 1.6 + 0.1 * min(i, j) + 0.05 * max(i, j), 300.0 + 20.0 * (i + j), R, D,
                              2.6 + 0.1 * min(i, j) + 0.05 * max(i, j), 1500.0 + 100.0 * (i + j)]
    return P


def tersoff_shell_places(P, i=0, j=0):
    """The six exact distances around the cutoff shell of the pair entry (i, j, j): one ulp inside / on / one ulp outside R - D and
    R + D, computed as the kernels compute the bounds (fl(R - D), fl(R + D))."""
    R, D = P[i, j, j, 10], P[i, j, j, 11]
    lo, hi = R - D, R + D
    return [up(lo, -1), lo, up(lo, 1), up(hi, -1), hi, up(hi, 1)]


def tersoff_edge_chains():
    """Eight chains.  Every cluster has a centre of type c with four neighbours of type a on the axes, at four of the six places of
    the shell of the entry (c, a, a) (the next cluster of the same kind takes the next four), and fillers of all three types at 1.5 .. 2.75 A.  (c, a) runs over (0, 0), (0, 1), (1, 0),
    (1, 1): for (0, 0) R + D = 3.2 A is also the row cutoff of the table, where the inclusive search meets the kernels' r > R + D (the
    pair one ulp beyond never enters the row); for the others the pair one ulp beyond its own cutoff sits IN the row and the kernel
    must skip it.  Chains 0, 1: 3 fillers (rows of <= 10 slots: the tile form), eight clusters each; chains 2 .. 7: 14 fillers
    (rows of 17 or 18: the long-row form), four clusters each.  The fillers 0.9 .. 1.7 A nearer than the axis neighbours put terms into both
    clamps through m = 1 and m = 3; centres of type 0 have n = 1, of type 1 n = 0.78734.
    Returns (P, [(structure, centres)])."""
    P = tersoff_edge_table()
    rng = np.random.default_rng(2024)
    kinds = ((0, 0), (0, 1), (1, 0), (1, 1))
    chains, c = [], 0
    for n_fill, n_chains, per_chain in ((3, 2, 8), (14, 6, 4)):
        for _ in range(n_chains):
            cl = []
            for _ in range(per_chain):
                ct, at = kinds[c % 4]
                places = tersoff_shell_places(P, ct, at)
                cl.append(cluster(spread(places, c // 4), [at] * N_AXES, n_fill, (1.5, 2.75), (0, 1, 2), ct, rng))
                c += 1
            chains.append(cluster_chain(cl))
    return P, chains


def tersoff_clamp_box(seed=TERSOFF_BOX_SEED, n=24, box=7.0, min_sep=1.5):
    """A periodic box on the edge table for the stress test: no pair on a shell end, and (asserted with the census over every
    strained copy the strain derivative evaluates) no term that changes its branch under a strain of up to 4e-4."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        x = rng.uniform(0, box, 3)
        if all(np.linalg.norm((x - y + box / 2) % box - box / 2) >= min_sep for y in pts):
            pts.append(x)
    return rng.integers(0, 3, n).astype(np.int32), np.array(pts), np.eye(3) * box, np.ones(3, np.uint8)


def strained_copies(structure, steps=(1e-4, 2e-4, 4e-4)):
    """Every structure strain_fd.fd_stress evaluates for ``structure`` (6 components, both signs, three steps)."""
    import strain_fd as sf

    T, X, Cl, pbc = structure
    out = []
    for k in range(6):
        for h in steps:
            for sgn in (1.0, -1.0):
                x, c = sf.strained((X, Cl), sf.voigt_strain(k, sgn * h))
                out.append((T, x, c, pbc))
    return out


# ======================================================================================================================================
# places: which directed pairs sit one ulp inside / on / one ulp outside a bound, by the kernel form of their centre
# ======================================================================================================================================
def place_of(r, bound):
    return "-" if r == up(bound, -1) else "0" if r == bound else "+" if r == up(bound, 1) else None


def place_tally(structure, row_cut, bounds_of, form_of):
    """{(form, bound name, place): directed pairs}.  ``bounds_of(ti, tj)`` -> {name: distance} of the pair entry (ti, tj, tj);
    ``form_of(distances of the centre's row)`` -> "tile" / "long"; a row is every neighbour with d^2 <= row_cut^2 (the device search).
    Also (form, "rows", "centres") and (form, "rows", "beyond own cutoff") = row members outside their pair's largest bound."""
    from collections import Counter

    from cell_cases import brute_neighbors

    T, X, Cl, pbc = structure
    ei, ej, _, er = brute_neighbors(X, Cl, pbc, row_cut)
    d = np.sqrt((er * er).sum(axis=1))
    start = np.searchsorted(ei, np.arange(len(T) + 1))
    out = Counter()
    for i in range(len(T)):
        a, b = start[i], start[i + 1]
        form = form_of(d[a:b])
        out[form, "rows", "centres"] += 1
        for e in range(a, b):
            bounds = bounds_of(int(T[i]), int(T[ej[e]]))
            for name, v in bounds.items():
                p = place_of(d[e], v)
                if p:
                    out[form, name, p] += 1
            out[form, "rows", "beyond own cutoff"] += d[e] > max(bounds.values())
    return out


def by_slots(limit=16):
    return lambda row: "tile" if len(row) <= limit else "long"


# ======================================================================================================================================
# Stillinger-Weber: the shipped Si set and the three-species set of tests/sw_oracle.py (different a sigma, every gamma > 1)
# ======================================================================================================================================
SW_SETS = {"Si": ((0, 0),), "three species": ((0, 0), (0, 2), (2, 0), (1, 1))}      # (centre, axis neighbour) kinds of the clusters


def sw_set(name):
    import sw_oracle

    return sw_oracle.si_params() if name == "Si" else sw_oracle.three_species()[1]


def sw_bounds(P):
    return lambda ti, tj: {"cut": float(P[ti, tj, tj, 2] * P[ti, tj, tj, 1])}


def sw_underflow_distance(P, ti, tj):
    """cut - gamma sigma / 760: gamma sigma x = -760 (exp = 0: ef has underflowed, and 0 x dlf with dlf ~ -1e5 must stay 0) while
    sigma x = -760 / gamma >= -724 for gamma >= 1.05 (exp is still a number, if a denormal one)."""
    p = P[ti, tj, tj]
    return float(p[2] * p[1] - p[4] * p[1] / 760.0)


def sw_edge_chains(P, kinds, seed):
    """Clusters as for Tersoff: centre type c, four axis neighbours of type a at cut-, cut, cut+ and the underflow
    distance (cut = a sigma of the entry (c, a, a)); 3 fillers (tile form) or 14 (long-row form: rows of 17 or 18) at 2.1 .. 3.2 A.
    Two tile chains of eight clusters, four long chains of four.  Returns [(structure, centres)]."""
    rng = np.random.default_rng(seed)
    nt = P.shape[0]
    chains, c = [], 0
    for n_fill, n_chains, per_chain in ((3, 2, 8), (14, 4, 4)):
        for _ in range(n_chains):
            cl = []
            for _ in range(per_chain):
                ct, at = kinds[c % len(kinds)]
                cut = float(P[ct, at, at, 2] * P[ct, at, at, 1])
                und = sw_underflow_distance(P, ct, at)
                cl.append(cluster([up(cut, -1), cut, up(cut, 1), und], [at] * N_AXES, n_fill, (2.1, 3.2), tuple(range(nt)), ct, rng,
                                  min_sep=1.8))
                c += 1
            chains.append(cluster_chain(cl))
    return chains


# ======================================================================================================================================
# Vashishta: the built-in SiC set
# ======================================================================================================================================
def vashishta_bounds(P):
    return lambda ti, tj: {"r0": float(P[ti, tj, tj, 11]), "rc": float(P[ti, tj, tj, 8])}


def vashishta_edge_chains(P, seed=77):
    """Clusters with a Si centre (type 1) and four C neighbours (type 0) on the axes at r0-, r0+, rc-, rc+ of the entry
    (Si, C, C), plus 15 or 16 fillers of both types at 1.75 .. 2.8 A (all short, r < r0): with the axis neighbour at r0- the centre has
    exactly 16 short slots (the LDS tile of csrc/vashishta_dev.h holds 16) or 17 (its long form).  Four chains of four clusters: chains
    0, 1 with 16 short slots, chains 2, 3 with 17.  Returns [(structure, centres)]."""
    rng = np.random.default_rng(seed)
    r0, rc = float(P[1, 0, 0, 11]), float(P[1, 0, 0, 8])
    places = [up(r0, -1), up(r0, 1), up(rc, -1), up(rc, 1)]
    chains = []
    for n_fill in (15, 15, 16, 16):
        cl = [cluster(places, [0] * N_AXES, n_fill, (1.75, 2.8), (0, 1), 1, rng, min_sep=1.6) for _ in range(4)]
        chains.append(cluster_chain(cl))
    return chains


def by_short_slots(r0max, limit=16):
    return lambda row: "tile" if int((row < r0max).sum()) <= limit else "long"
