"""CPU restatement of LAMMPS ``pair_style vashishta`` in vectorised numpy fp64 (test infrastructure, not the thing shipped).

Neighbors come from ``cell_cases.brute_neighbors`` (every image enumerated, nothing shared with the device neighbor list).  For an
entry (i, j, k) of ``params[nt, nt, nt, 14]`` (LAMMPS columns H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta):

    V(r)          = H / r^eta + qqr2e Zi Zj / r exp(-r / lambda1) - D / r^4 exp(-r / lambda4) - W / r^6
    phi2(r_ij)    = V(r) - V(rc) - (r - rc) V'(rc)                                     r < rc, entry (i, j, j)
    phi3(j, i, k) = B f_ij(r_ij) f_ik(r_ik) dc^2 / (1 + C dc^2),  dc = cos theta_jik - costheta    B, C, costheta: (i, j, k)
    f_ij(r)       = exp(gamma / (r - r0)) for r < r0, else 0, with entry (i, j, j)

E = sum over directed pairs 1/2 phi2 (= sum over pairs phi2: (i, j, j) and (j, i, i) agree in the two-body columns) + sum over
centres i and unordered neighbor pairs {j, k} phi3.  pe/atom: pair terms half / half, three-body terms in thirds (LAMMPS ev_tally3).
Forces are the analytic gradient; the virial is dE / d eps = sum over slots of G_a r_b.  No LAMMPS was executed: the SiC numbers of
the 2007 paper (cohesive energy, lattice constant, B, C11, C12) are what pins the form, qqr2e, the shift and the angular part.
"""

from __future__ import annotations

import numpy as np

from cell_cases import brute_neighbors

QQR2E = 14.399645
EV_A3_GPA = 160.21766208
SIC = "SiC_Vashishta_2007"
SIC_A0 = 4.3581


def cutoff(params) -> float:
    P = np.asarray(params, np.float64)
    n = np.arange(P.shape[0])
    return float(P[:, n, n, 8].max())


def r0max(params) -> float:
    P = np.asarray(params, np.float64)
    n = np.arange(P.shape[0])
    return float(P[:, n, n, 11].max())


def _v(p, r):
    """V(r), V'(r) with rows p[:, 14] of entries (i, j, j); terms with a zero coefficient are skipped (their lambda may be 0)."""
    H, eta, zz, l1, D, l4, W = p[:, 0], p[:, 1], QQR2E * p[:, 2] * p[:, 3], p[:, 4], p[:, 5], p[:, 6], p[:, 7]
    hr = H * r ** -eta
    v = hr - W / r ** 6
    dv = -eta * hr / r + 6.0 * W / r ** 7
    m = zz != 0.0
    c = np.zeros_like(r)
    c[m] = zz[m] / r[m] * np.exp(-r[m] / l1[m])
    v = v + c
    dv[m] -= c[m] * (1.0 / r[m] + 1.0 / l1[m])
    m = D != 0.0
    d = np.zeros_like(r)
    d[m] = D[m] / r[m] ** 4 * np.exp(-r[m] / l4[m])
    v = v - d
    dv[m] += d[m] * (4.0 / r[m] + 1.0 / l4[m])
    return v, dv


def pair_term(p, r):
    """phi2(r), phi2'(r) for rows p of entries (i, j, j) at distances r (zero at and beyond rc)."""
    p = np.atleast_2d(np.asarray(p, np.float64))
    r = np.atleast_1d(np.asarray(r, np.float64))
    rc = p[:, 8]
    v, dv = _v(p, r)
    vc, dvc = _v(p, rc.copy())
    inside = r < rc
    return np.where(inside, v - vc - (r - rc) * dvc, 0.0), np.where(inside, dv - dvc, 0.0)


def vashishta(params, types, pos, cell, pbc, virial=False):
    """Returns (E, e_atom [N], forces [N, 3]) and, with ``virial=True``, also dE / d eps [6] (Voigt xx yy zz yz xz xy, eV)."""
    P = np.asarray(params, np.float64)
    types = np.asarray(types, np.int64)
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = len(pos)
    i, j, _, rv = brute_neighbors(pos, cell, pbc, cutoff(P))
    i, j = i.astype(np.int64), j.astype(np.int64)
    d = np.sqrt((rv * rv).sum(axis=1))
    e_atom = np.zeros(n)
    F = np.zeros((n, 3))
    if len(i) == 0:
        out = (0.0, e_atom, F)
        return out + (np.zeros(6),) if virial else out
    ti, tj = types[i], types[j]
    Pij = P[ti, tj, tj]
    u = rv / d[:, None]
    phi2, dphi2 = pair_term(Pij, d)
    G = 0.5 * dphi2[:, None] * u                      # dE / d r_e of the directed halves
    np.add.at(e_atom, i, 0.25 * phi2)
    np.add.at(e_atom, j, 0.25 * phi2)
    E = 0.5 * phi2.sum()

    gam, r0 = Pij[:, 10], Pij[:, 11]
    short = np.flatnonzero(d < r0)                    # slots that take part in three-body terms
    x = 1.0 / (d[short] - r0[short])
    f = np.exp(gam[short] * x)
    dlf = -gam[short] * x * x
    si, sj, su, sd, stj = i[short], j[short], u[short], d[short], tj[short]
    e1s, e2s = [], []
    order = np.argsort(si, kind="stable")
    starts = np.searchsorted(si[order], np.arange(n + 1))
    for c in range(n):
        idx = order[starts[c]:starts[c + 1]]
        if len(idx) >= 2:
            a1, a2 = np.triu_indices(len(idx), 1)
            e1s.append(idx[a1]); e2s.append(idx[a2])
    if e1s:
        e1, e2 = np.concatenate(e1s), np.concatenate(e2s)
        c = si[e1]
        tri = P[types[c], stj[e1], stj[e2]]
        B, C, c0 = tri[:, 9], tri[:, 12], tri[:, 13]
        cs = (su[e1] * su[e2]).sum(axis=1)
        dc = cs - c0
        q = 1.0 / (1.0 + C * dc * dc)
        h, dh = dc * dc * q, 2.0 * dc * q * q
        w = B * f[e1] * f[e2]
        phi3 = w * h
        E += phi3.sum()
        np.add.at(e_atom, c, phi3 / 3.0)
        np.add.at(e_atom, sj[e1], phi3 / 3.0)
        np.add.at(e_atom, sj[e2], phi3 / 3.0)
        g1 = w[:, None] * (dh[:, None] * (su[e2] - cs[:, None] * su[e1]) / sd[e1][:, None] + (h * dlf[e1])[:, None] * su[e1])
        g2 = w[:, None] * (dh[:, None] * (su[e1] - cs[:, None] * su[e2]) / sd[e2][:, None] + (h * dlf[e2])[:, None] * su[e2])
        np.add.at(G, short[e1], g1)
        np.add.at(G, short[e2], g2)
    # r_e = x_j - x_i (+ shift): F_i = +G_e, F_j = -G_e
    np.add.at(F, i, G)
    np.add.at(F, j, -G)
    if not virial:
        return float(E), e_atom, F
    W = G.T @ rv
    W = 0.5 * (W + W.T)
    return float(E), e_atom, F, np.array([W[0, 0], W[1, 1], W[2, 2], W[1, 2], W[0, 2], W[0, 1]])


def energy(params, types, pos, cell, pbc):
    return vashishta(params, types, pos, cell, pbc)[0]


# -- parameter sets ------------------------------------------------------------------------------------------------------------------
def sic_params():
    """(species, params [2, 2, 2, 14]) of the built-in SiC set; type 0 = C, 1 = Si."""
    from surface_sampling_amd import vashishta as va

    sp = va.builtin_species(SIC)
    return sp, va.parse_vashishta(va.builtin_text(SIC), sp)


def text_of(sp, P, wrap=False):
    """A .vashishta text of the table (``wrap``: every entry spans two lines)."""
    n = len(sp)
    lines = ["# e1 e2 e3  H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta"]
    for i in range(n):
        for j in range(n):
            for k in range(n):
                v = [repr(float(x)) for x in P[i, j, k]]
                head = f"{sp[i]} {sp[j]} {sp[k]}  "
                lines.append(head + " ".join(v[:8]) + "\n        " + " ".join(v[8:]) if wrap else head + " ".join(v))
    return "\n".join(lines) + "\n"


def three_species():
    """A synthetic three-species set (species, params [3, 3, 3, 14], text): distinct numbers in every column, rc in {5.5, 6.0} and
    r0 in {3.2, 3.8} (symmetric in the pair, as rc must be; gamma is not), eta both integer (7, 9) and not (7.5); B, C and costheta
    depend on the centre and on the unordered pair {j, k}.  The two-body columns of the entries with j != k hold other numbers that
    nobody reads.  At the density of ``sw_oracle.dense_box`` the rows below r0max = 3.8 A lie on both sides of 16 slots."""
    sp = ["Si", "O", "Al"]
    nt = 3
    sym = lambda a, b, c, d, e, f: np.array([[a, b, c], [b, d, e], [c, e, f]], float)          # noqa: E731
    H = sym(23.7, 163.9, 47.1, 74.2, 120.3, 31.9)
    eta = sym(7.0, 9.0, 7.5, 7.0, 9.0, 7.0)
    Z = np.array([1.2, -0.6, 0.9])
    lam1 = sym(4.43, 4.60, 5.0, 4.43, 4.80, 5.2)
    D = sym(0.0, 3.46, 1.9, 1.73, 2.7, 0.8)
    lam4 = sym(2.5, 2.7, 3.0, 2.5, 2.9, 3.1)
    Wd = sym(0.0, 12.1, 3.3, 0.0, 20.5, 7.7)
    rc = sym(5.5, 6.0, 5.5, 6.0, 5.5, 6.0)
    r0 = sym(3.2, 3.8, 3.2, 3.8, 3.2, 3.8)
    gam = np.array([[1.00, 1.15, 0.90], [1.25, 0.80, 1.05], [0.95, 1.10, 1.30]])          # by (centre, neighbor): not symmetric
    P = np.zeros((nt, nt, nt, 14))
    for i in range(nt):
        for j in range(nt):
            for k in range(nt):
                s, m = j + k, abs(j - k)
                B = 4.0 + 1.1 * i + 0.7 * s + 0.45 * m
                C = 0.5 + 0.9 * i + 0.35 * s + 0.2 * m
                c0 = -1.0 / 3.0 + 0.03 * i - 0.02 * s + 0.01 * m
                if j == k:
                    P[i, j, k] = [H[i, j], eta[i, j], Z[i], Z[j], lam1[i, j], D[i, j], lam4[i, j], Wd[i, j], rc[i, j], B, gam[i, j],
                                  r0[i, j], C, c0]
                else:
                    P[i, j, k] = [0.1 * (i + 1), 0.0, 0.3, -0.2 * j, 0.0, 0.05 * k, 0.0, 0.01, 0.0, B, 0.5, 0.25, C, c0]
    return sp, P, text_of(sp, P, wrap=True)


def two_species_r0_zero():
    """A two-species set in which centre 0 has r0 = 0 (no three-body term on it) while centre 1 has r0 = 3.0 towards both species:
    (species, params [2, 2, 2, 14])."""
    sp = ["In", "P"]
    P = np.zeros((2, 2, 2, 14))
    H = np.array([[270.0, 450.0], [450.0, 1020.0]])
    eta = np.array([[7.0, 9.0], [9.0, 7.0]])
    Z = np.array([1.1, -1.1])
    Wd = np.array([[0.0, 55.0], [55.0, 0.0]])
    D = np.array([[0.0, 9.1], [9.1, 18.2]])
    for i in range(2):
        for j in range(2):
            for k in range(2):
                B, C, c0 = 6.0 + 2.0 * i + 0.5 * (j + k), 3.0 + i + 0.25 * (j + k), -1.0 / 3.0 + 0.05 * i
                if j == k:
                    P[i, j, k] = [H[i, j], eta[i, j], Z[i], Z[j], 4.5, D[i, j], 2.75, Wd[i, j], 5.0, B, 1.0 + 0.2 * j,
                                  0.0 if i == 0 else 3.0, C, c0]
                else:
                    P[i, j, k] = [0.0] * 8 + [5.0, B, 0.0, 0.0, C, c0]
    return sp, P


# -- structures -----------------------------------------------------------------------------------------------------------------------
def zincblende(a, reps=1):
    """Conventional 8-atom zincblende cell (times reps^3), C (type 0) on the fcc sites and Si (type 1) on the tetrahedral ones:
    (types, positions, cell)."""
    fcc = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    basis = np.concatenate([fcc, fcc + 0.25])
    t = np.array([0] * 4 + [1] * 4, np.int32)
    shifts = np.array([[x, y, z] for x in range(reps) for y in range(reps) for z in range(reps)], float)
    frac = (basis[None, :, :] + shifts[:, None, :]).reshape(-1, 3) / reps
    cell = np.eye(3) * a * reps
    return np.tile(t, len(shifts)), frac @ cell, cell


def elastic(energy_and_virial, a=SIC_A0, h=1e-3):
    """(C11, C12) in GPa from the xx and yy stresses of the 8-atom cell under +-h xx strain.  ``energy_and_virial(types, positions,
    cell) -> dE / d eps [6]`` in eV (zincblende under a uniaxial strain along a cube axis has no internal relaxation)."""
    T, X, Cl = zincblende(a)
    s = []
    for e in (h, -h):
        M = np.diag([1.0 + e, 1.0, 1.0])
        w = np.asarray(energy_and_virial(T, X @ M, Cl @ M))
        s.append(w / abs(np.linalg.det(Cl @ M)))
    d = (s[0] - s[1]) / (2 * h) * EV_A3_GPA
    return float(d[0]), float(d[1])


def rattled_sic(seed=1, sigma=0.08, reps=(1, 1, 1), n_fixed=0):
    """Zincblende SiC, 8 reps atoms, rattled (the first ``n_fixed`` atoms stay): (types, positions, cell, pbc)."""
    T, X, Cl = zincblende(SIC_A0)
    sh = [np.array([x, y, z]) * SIC_A0 for x in range(reps[0]) for y in range(reps[1]) for z in range(reps[2])]
    T, X, Cl = np.tile(T, len(sh)), np.concatenate([X + s for s in sh]), Cl * np.asarray(reps, float)[:, None]
    move = np.random.default_rng(seed).normal(0.0, sigma, X.shape)
    move[:n_fixed] = 0.0
    return T.astype(np.int32), X + move, Cl, np.ones(3, np.uint8)


def sic001_slab(nx=2, ny=2, layers=4, vacuum=12.0):
    """A small SiC(001) slab, C-terminated at the bottom and Si-terminated on top, periodic in x and y, with the C adsorption sites
    of the next layer: (numbers, positions, cell, pbc, ads_coords).  Conventional cell a x a in plane, ``layers`` double layers."""
    a = SIC_A0
    pos, num = [], []
    for l in range(2 * layers):                        # planes a / 4 apart: C, Si, C, Si, ...
        for ix in range(nx):
            for iy in range(ny):
                for bx, by in ((0.0, 0.0), (0.5, 0.5)):
                    off = [(0.0, 0.0), (0.25, 0.25), (0.5, 0.0), (0.75, 0.25)][l % 4]
                    pos.append([(ix + bx + off[0]) * a, (iy + by + off[1]) * a, l * a / 4])
                    num.append(6 if l % 2 == 0 else 14)
    pos = np.array(pos)
    cell = np.diag([nx * a, ny * a, pos[:, 2].max() + vacuum])
    lnext = 2 * layers
    off = [(0.0, 0.0), (0.25, 0.25), (0.5, 0.0), (0.75, 0.25)][lnext % 4]
    ads = np.array([[(ix + bx + off[0]) * a, (iy + by + off[1]) * a, lnext * a / 4]
                    for ix in range(nx) for iy in range(ny) for bx, by in ((0.0, 0.0), (0.5, 0.5))])
    return np.array(num, np.int32), pos, cell, np.array([1, 1, 0], np.uint8), ads
