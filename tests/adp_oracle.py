"""numpy restatement of LAMMPS ``pair_style adp`` (Mishin, Mehl, Papaconstantopoulos 2005) in fp64, synthetic ADP sets and the
states the ADP tests share.

TEST INFRASTRUCTURE ONLY (the checker of csrc/adp.hip).  Restated from the LAMMPS documentation of ``pair_style adp``; no LAMMPS
was executed:

    E = sum_i [F_{a(i)}(rho_i) + 1/2 sum_a mu_ia^2 + 1/2 sum_ab lambda_iab^2 - nu_i^2 / 6] + 1/2 sum_{i != j} phi_{a(i)a(j)}(r_ij),
    rho_i = sum_j rho_{a(j)}(r),  mu_i = sum_j u_{a(i)a(j)}(r) r,  lambda_i = sum_j w_{a(i)a(j)}(r) r (x) r,  nu_i = tr lambda_i,

r = x_j - x_i over every neighbour inside the file's cutoff, images included; pe/atom of i = the bracket + half of its pair
energies.  F, rho and r phi are the tables and splines of ``eam_alloy_oracle.eam_typed`` (alloy densities, F continued linearly
beyond its table); u and w take the same spline and grid rule and are not scaled by r.  The neighbour enumeration and the spline
helper are those of eam_alloy_oracle.

The gradient of one pair with respect to r = r_ij (the force on i is + g, on j - g; derived from the energy above, pinned by
tests/test_adp_cpu.py against central differences of ``adp(...)[0]``), with dm = mu_i - mu_j, L = lambda_i + lambda_j:

    g = [F'_i rho'_j + F'_j rho'_i + phi'] r_hat + u dm + u' (dm . r) r_hat + w' (r^T L r) r_hat + 2 w L r
        - (nu_i + nu_j) / 3 (w' r^2 r_hat + 2 w r)
"""

from __future__ import annotations

import os

import numpy as np

import eam_alloy_oracle as ao
from eam_oracle import build_spline, spline_eval

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def adp(tab, types, pos, cell, pbc, angular=True, virial=False):
    """``tab``: eam.EamTables with ``u`` / ``w`` (or any object with its fields); ``types`` [N] table indices.  Returns
    (E, e_atom [N], forces [N, 3]) and, with ``virial=True``, also dE / d eps [6] (Voigt xx yy zz yz xz xy, eV) of a homogeneous
    strain.  ``angular=False`` drops the dipole and quadrupole terms (the eam/alloy energy of the same tables)."""
    types = np.asarray(types, np.int64)
    pos = np.asarray(pos, float).reshape(-1, 3)
    n = len(types)
    assert not getattr(tab, "fs", False)
    Fs = [build_spline(f, tab.drho) for f in tab.frho]
    Rs = [build_spline(f, tab.dr) for f in tab.rhor]
    Zs = [build_spline(f, tab.dr) for f in tab.z2r]
    ii, jj, rr = ao.neighbor_pairs(pos, cell, pbc, tab.cutoff)
    dist = np.sqrt((rr ** 2).sum(axis=1))
    ti, tj = types[ii], types[jj]
    hi, lo = np.maximum(ti, tj), np.minimum(ti, tj)
    p_idx = hi * (hi + 1) // 2 + lo
    rho_e, drho_ji = ao._grouped(Rs, tj, dist, tab.dr, tab.nr)
    _, drho_ij = ao._grouped(Rs, ti, dist, tab.dr, tab.nr)
    z, dz = ao._grouped(Zs, p_idx, dist, tab.dr, tab.nr)
    if angular:
        u, du = ao._grouped([build_spline(f, tab.dr) for f in tab.u], p_idx, dist, tab.dr, tab.nr)
        w, dw = ao._grouped([build_spline(f, tab.dr) for f in tab.w], p_idx, dist, tab.dr, tab.nr)
    else:
        u = du = w = dw = np.zeros(len(dist))
    rho = np.zeros(n)
    np.add.at(rho, ii, rho_e)
    mu = np.zeros((n, 3))
    np.add.at(mu, ii, u[:, None] * rr)
    lam = np.zeros((n, 3, 3))
    np.add.at(lam, ii, w[:, None, None] * rr[:, :, None] * rr[:, None, :])
    nu = np.trace(lam, axis1=1, axis2=2)
    Fi, fp = np.zeros(n), np.zeros(n)
    for t in np.unique(types):
        m = types == t
        Fi[m], fp[m] = spline_eval(Fs[t], rho[m], tab.drho, tab.nrho, clamp_lo=True)
    rhomax = (tab.nrho - 1) * tab.drho
    Fi = Fi + np.where(rho > rhomax, fp * (rho - rhomax), 0.0)
    phi = z / dist
    phip = dz / dist - phi / dist
    e_atom = Fi + 0.5 * (mu ** 2).sum(axis=1) + 0.5 * (lam ** 2).sum(axis=(1, 2)) - nu ** 2 / 6.0
    np.add.at(e_atom, ii, 0.5 * phi)
    rhat = rr / dist[:, None]
    dm = mu[ii] - mu[jj]
    L = lam[ii] + lam[jj]
    Lr = np.einsum("eab,eb->ea", L, rr)
    nus = nu[ii] + nu[jj]
    radial = (fp[ii] * drho_ji + fp[jj] * drho_ij + phip + du * (dm * rr).sum(axis=1) + dw * (rr * Lr).sum(axis=1)
              - nus / 3.0 * dw * dist ** 2)
    g = radial[:, None] * rhat + u[:, None] * dm + 2.0 * w[:, None] * Lr - (2.0 / 3.0 * nus * w)[:, None] * rr
    forces = np.zeros((n, 3))
    np.add.at(forces, ii, g)
    out = (float(e_atom.sum()), e_atom, forces)
    if virial:
        W = 0.5 * np.einsum("ea,eb->ab", g, rr)
        W = 0.5 * (W + W.T)
        out += (np.array([W[a, b] for a, b in VOIGT]),)
    return out


# ---- synthetic ADP sets ----------------------------------------------------------------------------------------------------------
# amplitude of u [1 / A-ish: mu = sum u r is an energy^(1/2)] and w of every pair (0,0), (1,0), (1,1), (2,0), (2,1), (2,2): all
# distinct, both signs.  Chosen (and pinned by test_adp_cpu.py) so that the angular part changes E by more than 1e-2 eV on every
# rattled test state below.
U_AMP = (0.30, -0.22, 0.26, 0.18, -0.28, 0.24)
W_AMP = (0.050, 0.040, -0.060, 0.045, 0.055, -0.035)


def _uw(setfl, scale=1.0):
    """Smooth u_p = a_p (1 - r / rc)^3 and w_p = b_p (1 - r / rc)^4 exp(-r / 4): value and slope vanish at the cutoff."""
    r = np.arange(setfl.nr) * setfl.dr
    x = np.clip(1.0 - r / setfl.cutoff, 0.0, None)
    n_pairs = len(setfl.z2r)
    u = np.stack([scale * U_AMP[p] * x ** 3 for p in range(n_pairs)])
    w = np.stack([scale * W_AMP[p] * x ** 4 * np.exp(-r / 4.0) for p in range(n_pairs)])
    return u, w


def cuau_adp(cu, au, scale=1.0):
    """Two elements (Cu, Au): ``eam_alloy_oracle.cuau_setfl`` of the two golden funcfl files plus synthetic u, w (``scale`` = 0: an
    ADP file whose angular part is zero)."""
    s = ao.cuau_setfl(cu, au)
    s.u, s.w = _uw(s, scale)
    s.comments = ("synthetic ADP: Cu Au from Cu_u3 / Au_u3 + smooth u, w", "", "")
    return s


def cuauag_adp(cu, au, scale=1.0):
    """Three elements: Cu, Au and a scaled copy of Cu under the name Ag, so that the pairs (2,0), (2,1), (2,2) have tables of
    their own."""
    from surface_sampling_amd import eam

    s = ao.cuau_setfl(cu, au)
    frho = np.vstack([s.frho, 0.9 * s.frho[:1]])
    rhor = np.vstack([s.rhor, 1.1 * s.rhor[:1]])
    z2r = np.vstack([s.z2r, 0.95 * s.z2r[0:1], 1.05 * s.z2r[1:2], 0.9 * s.z2r[0:1]])
    out = eam.Setfl(["Cu", "Au", "Ag"], [29, 79, 47], [63.55, 196.97, 107.87], [3.615, 4.08, 4.09], ["fcc"] * 3, s.nrho, s.drho,
                    s.nr, s.dr, s.cutoff, frho, rhor, z2r, False, ("synthetic ADP: Cu Au + a scaled copy of Cu as Ag", "", ""))
    out.u, out.w = _uw(out, scale)
    return out


def permuted(setfl, order):
    """The same ADP potential with its elements listed in ``order`` (indices into setfl.elements)."""
    from surface_sampling_amd import eam

    o = list(order)
    out = ao.permuted(setfl, o)
    pairs = [eam.pair_index(o[a], o[b]) for a in range(len(o)) for b in range(a + 1)]
    out.u, out.w = setfl.u[pairs].copy(), setfl.w[pairs].copy()
    return out


# ---- the states the tests share ------------------------------------------------------------------------------------------------
def cu100_states():
    """Two types: Cu(100) with Au / Cu adatoms (9 .. 12 atoms) and rattled 192-atom Cu(100) slabs with random Au substitution --
    the states of tests/test_eam_alloy_gpu.py."""
    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    out = []
    for k, sub in enumerate(((3,), (2, 9), (0, 5, 11), (1, 4, 7, 12))):
        pos = np.vstack([d["positions"], d["ads_coords"][list(sub)]])
        t = np.concatenate([np.zeros(len(d["positions"]), np.int32), (np.arange(len(sub)) + k) % 2])
        out.append((t.astype(np.int32), pos, d["cell"], d["pbc"].astype(np.uint8)))
    for seed, frac in ((1, 0.1), (3, 0.5)):
        pos, cell, pbc = ao.cu100_slab(4, 4, 6)
        pos = pos + np.random.default_rng(seed).normal(0, 0.05, pos.shape)
        out.append((ao.random_alloy(pos, frac, seed), pos, cell, pbc))
    return out


def three_element_slab(pbc=(1, 1, 0)):
    """A rattled 4 x 4 x 3 fcc(100) slab (96 atoms) of three elements in random order."""
    pos, cell, _ = ao.cu100_slab(4, 4, 3)
    rng = np.random.default_rng(17)
    pos = pos + rng.normal(0, 0.05, pos.shape)
    return rng.integers(0, 3, len(pos)).astype(np.int32), pos, cell, np.array(pbc, np.uint8)


def skewed_thin_cell():
    """Three atoms (Ag, Au, Cu) on low-symmetry sites of a skewed cell whose three heights (3.4, 4.9 and 5.2 A) are below the
    cutoff of 5.55 A: every atom is a neighbour of its own images (24 of the 74 directed edges).  The images come in +- pairs, so
    they cancel in mu and add up in lambda."""
    cell = np.array([[3.4, 0.0, 0.0], [0.9, 4.9, 0.0], [0.5, -0.7, 5.2]])
    frac = np.array([[0.03, 0.05, -0.02], [0.45, 0.52, 0.30], [0.10, 0.48, 0.78]])
    return np.array([2, 1, 0], np.int32), frac @ cell, cell, np.ones(3, np.uint8)


def fcc_bulk(a=3.615):
    """One atom in the fcc primitive cell: a site of cubic symmetry."""
    return np.zeros(1, np.int32), np.zeros((1, 3)), np.array([[0, a / 2, a / 2], [a / 2, 0, a / 2], [a / 2, a / 2, 0]]), np.ones(3, np.uint8)


def rattled_states():
    """{name: (types, positions, cell, pbc)} of every rattled / low-symmetry state of the ADP tests (types of the three-element
    set; the two-type states use types 0 and 1 only)."""
    out = {f"cu100_{k}": s for k, s in enumerate(cu100_states())}
    out["slab3_TTF"] = three_element_slab((1, 1, 0))
    out["slab3_TFF"] = three_element_slab((1, 0, 0))
    out["skewed_thin"] = skewed_thin_cell()
    return out


def relax_case():
    """A rattled 32-atom Cu/Au fcc(100) slab (2 x 2 cells, 4 layers) and the mask that fixes its bottom layer."""
    pos, cell, pbc = ao.cu100_slab(2, 2, 4)
    pos = pos + np.random.default_rng(5).normal(0, 0.04, pos.shape)
    t = ao.random_alloy(pos, 0.3, 9)
    return (t, pos, cell, pbc), (np.arange(len(pos)) < 8).astype(np.uint8)
