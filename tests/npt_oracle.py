"""numpy restatement of the device's constant-pressure MD (csrc/md_npt.hip, the comment of vssr_batch_md_npt in include/vssr_eval.h; test
infrastructure): the step of tests/md_oracle.py with a Berendsen thermostat, a Berendsen barostat (isotropic / per axis) or stochastic
cell rescaling around it.  Restated from ASE (NVTBerendsen, NPTBerendsen, Inhomogeneous_NPTBerendsen) and from Bernetti & Bussi,
J. Chem. Phys. 153, 114107 (2020) as remembered; NOT pinned by an executed library.

Row vectors; cell rows are lattice vectors.  The callback is ``force_fn(pos [N, 3], cells [B, 3, 3]) -> (E [B], F [N, 3], sigma [B, 6])``
over the whole batch, sigma the virial stress in Voigt order xx yy zz yz xz xy, eV / A^3, ASE's sign (None without a barostat).

Per chain and evaluation, with n = step0 + steps completed:
  1. non-finite E, F or (barostat) sigma: positions, velocities and cell back to the last completed step, stop reason 2
  2. close the step in flight: v += (dt/2) a
  3. every thermo_interval steps the record (E_pot, E_kin, V = |det C|, P = tr Pi / 3), Pi = -sigma + (1/V) sum m v v^T / ACC
     (P is NaN without a barostat: no stress is evaluated)
  4. steps == n_steps: stop reason 1
  5. a. Berendsen thermostat: lambda = sqrt(1 + (dt/taut)(kB T_n / kT_kin - 1)) (0 for a negative argument) clamped to [0.9, 1.1],
        kT_kin = 2 E_kin / (3 N_free); 1 if E_kin = 0 or N_free = 0; v <- lambda v; the kinetic part of Pi times lambda^2
     b. Berendsen barostat: mu = 1 - (dt beta / (3 taup))(P0 - P), P the mean of Pi_kk over the masked axes (isotropic) or Pi_kk itself
        (per axis); C <- C D, x <- x D for every atom, D = diag(mu_k), 1 on unmasked axes.
        crescale: d eps = -(beta/taup)(P0 - tr Pi / 3) dt + sqrt(2 kB T_n beta dt / (V taup)) xi, mu = exp(d eps / 3), C <- mu C,
        x <- mu x, v <- v / mu; xi = first normal of Philox draw (n, atom 0, tag 3, pair 0) under the chain key
     c. new cell finite, det keeps its sign, image counts floor(cutoff / height) + 1 <= those the call began with along every periodic
        axis; else stop reason 3 at the evaluated state, nothing of a / b written
     d. v += (dt/2) a; x += dt v, or md_oracle's Langevin BAOAB; forces are those of this evaluation (not recomputed after the rescale)."""
import numpy as np

import md_oracle as mo

KB, ACC = mo.KB, mo.ACC
TAG_CRESCALE = 3
STOP_REASONS = {1: "all steps taken", 2: "non-finite energy, force or stress", 3: "cell left the image range it began with or degenerated"}
THERMOSTATS, BAROSTATS, COUPLINGS = ("none", "langevin", "berendsen"), ("none", "berendsen", "crescale"), ("isotropic", "per_axis")


def image_counts(cells, pbc, cutoff):
    """cell_dev.h over a batch: (floor(cutoff / height) + 1 per periodic axis, 0 on open axes) [B, 3] and ok [B] (False: periodic with
    |det| < 1e-12 or a non-finite count)."""
    cells, pbc = np.asarray(cells, np.float64).reshape(-1, 3, 3), np.asarray(pbc, bool).reshape(-1, 3)
    a, b, c = cells[:, 0], cells[:, 1], cells[:, 2]
    bc, ca, ab = np.cross(b, c), np.cross(c, a), np.cross(a, b)
    vol = (a * bc).sum(axis=1)
    with np.errstate(all="ignore"):
        h = np.abs(vol)[:, None] / np.stack([np.linalg.norm(bc, axis=1), np.linalg.norm(ca, axis=1), np.linalg.norm(ab, axis=1)], axis=1)
        cnt = np.floor(cutoff / h) + 1
    ok = (~pbc.any(axis=1)) | ((np.abs(vol) >= 1e-12) & np.isfinite(np.where(pbc, cnt, 0.0)).all(axis=1))
    ni = np.where(pbc & ok[:, None], np.where(np.isfinite(cnt), cnt, 0.0), 0.0).astype(np.int64)
    return ni, ok


def det3(m):
    """The determinant of [..., 3, 3] by the cofactor expression of the device (csrc/md_npt.hip npt_det3)."""
    m = np.asarray(m, np.float64)
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]) - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
            + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def crescale_normal(seed, chain_id, n):
    keys = mo.chain_keys(seed, chain_id)
    z0, _ = mo.normal_pairs(keys, n, np.zeros(len(keys), np.uint64), TAG_CRESCALE, 0)
    return z0


def run(pos, vel, cells, pbc, mass, cfg_start, force_fn, *, n_steps, dt, cutoff, thermostat="none", barostat="none", coupling="isotropic",
        temperature=0.0, temperature_end=None, friction=0.0, taut=100.0, taup=1000.0, pressure=0.0, compressibility=1.0, mask=(1, 1, 1),
        ramp_steps=0, step0=0, seed=0, chain_id=None, fixed=None, thermo_interval=1):
    """The device's vssr_batch_md_npt.  Returns dict(positions, velocities, cells, epot / ekin / volume / pressure
    [n_steps // thermo_interval + 1, B] (NaN where a chain never got), n_done [B], stop_reason [B], n_eval)."""
    assert thermostat in THERMOSTATS and barostat in BAROSTATS and coupling in COUPLINGS
    pos, vel = np.array(pos, np.float64).reshape(-1, 3), np.array(vel, np.float64).reshape(-1, 3)
    cells = np.array(cells, np.float64).reshape(-1, 3, 3)
    mass = np.asarray(mass, np.float64)
    cfg_start, atom_chain, atom_idx = mo._layout(cfg_start)
    B, N = len(cfg_start) - 1, len(pos)
    pbc = np.broadcast_to(np.asarray(pbc), (B, 3)).astype(bool)
    mask = np.asarray(mask, bool)
    held = np.zeros(N, bool) if fixed is None else np.asarray(fixed, bool)
    vel[held] = 0.0
    baro, langevin = barostat != "none", thermostat == "langevin"
    t_end = temperature if temperature_end is None else temperature_end
    if thermostat == "none":
        ramp_steps = 0
    ids = np.arange(B, dtype=np.uint64) if chain_id is None else np.asarray(chain_id, np.uint64)
    keys = mo.chain_keys(seed, ids)[atom_chain]
    c1 = float(np.exp(-friction * dt)) if langevin else 1.0
    c2 = 1.0 - c1 * c1
    hdt = 0.5 * dt
    nfree = np.bincount(atom_chain[~held], minlength=B).astype(np.float64)
    nimg0, _ = image_counts(cells, pbc, cutoff)
    steps, reason, opened = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, bool)
    nrec = n_steps // thermo_interval + 1
    rec = {k: np.full((nrec, B), np.nan) for k in ("epot", "ekin", "volume", "pressure")}
    r_prev, v_prev, c_prev = pos.copy(), vel.copy(), cells.copy()
    n_eval = 0
    while (reason == 0).any():
        with np.errstate(all="ignore"):
            E, F, sig = force_fn(pos, cells)
        E, F = np.atleast_1d(np.asarray(E, np.float64)), np.asarray(F, np.float64).reshape(-1, 3)
        sig = np.asarray(sig, np.float64).reshape(B, 6) if baro else None
        n_eval += 1
        live = reason == 0
        # 1. non-finite
        bad = ~np.isfinite(E)
        np.logical_or.at(bad, atom_chain, ~np.isfinite(F).all(axis=1))
        if baro:
            bad |= ~np.isfinite(sig).all(axis=1)
        bad &= live
        back = bad & opened
        pos[back[atom_chain]], vel[back[atom_chain]] = r_prev[back[atom_chain]], v_prev[back[atom_chain]]
        cells[back] = c_prev[back]
        reason[bad], opened[bad] = 2, False
        live &= ~bad
        free = live[atom_chain] & ~held
        with np.errstate(all="ignore"):
            acc = (F / mass[:, None]) * ACC
        # 2. close the step in flight
        c = free & opened[atom_chain]
        vel[c] += hdt * acc[c]
        steps[live & opened] += 1
        opened[live] = False
        # the sums of one pass over the atoms
        k = np.zeros(B)
        np.add.at(k, atom_chain, mass * (vel * vel).sum(axis=1))
        kd = np.zeros((B, 3))
        np.add.at(kd, atom_chain, mass[:, None] * (vel * vel))
        ekin = 0.5 * k / ACC
        vol = np.abs(det3(cells))
        # 3. thermo
        due = live & (steps % thermo_interval == 0)
        row, col = steps[due] // thermo_interval, np.nonzero(due)[0]
        rec["epot"][row, col], rec["ekin"][row, col], rec["volume"][row, col] = E[due], ekin[due], vol[due]
        if baro:
            with np.errstate(all="ignore"):
                Pi = -sig[:, :3] + (kd / ACC) / vol[:, None]
            rec["pressure"][row, col] = (Pi.sum(axis=1) / 3.0)[due]
        # 4. finished
        fin = live & (steps == n_steps)
        reason[fin] = 1
        live &= ~fin
        if not live.any():
            break
        # 5. open the next step
        n = step0 + steps
        T = np.where(n < ramp_steps, temperature + (t_end - temperature) * (n.astype(np.float64) / float(max(ramp_steps, 1))), t_end)
        kT = KB * T if thermostat != "none" else np.zeros(B)
        lam = np.ones(B)
        if thermostat == "berendsen":
            for b in np.nonzero(live & (ekin != 0.0) & (nfree != 0.0))[0]:
                arg = 1.0 + (dt / taut) * (kT[b] / (2.0 * ekin[b] / (3.0 * nfree[b])) - 1.0)
                lam[b] = min(max(np.sqrt(arg) if arg > 0.0 else 0.0, 0.9), 1.1)
        mu, vdiv = np.ones((B, 3)), np.ones(B)
        if baro:
            with np.errstate(all="ignore"):
                Pi = -sig[:, :3] + ((lam * lam)[:, None] * kd / ACC) / vol[:, None]
                if barostat == "crescale":
                    xi = crescale_normal(seed, ids, n)
                    deps = -(compressibility / taup) * (pressure - Pi.sum(axis=1) / 3.0) * dt + np.sqrt(2.0 * kT * compressibility * dt / (vol * taup)) * xi
                    mu[:] = np.exp(deps / 3.0)[:, None]
                    vdiv = mu[:, 0].copy()
                else:
                    g = dt * compressibility / (3.0 * taup)
                    if coupling == "per_axis":
                        mu[:, mask] = 1.0 - g * (pressure - Pi[:, mask])
                    else:
                        mu[:, mask] = (1.0 - g * (pressure - Pi[:, mask].mean(axis=1)))[:, None]
                new = cells * mu[:, None, :]
            # c. the cell check
            with np.errstate(all="ignore"):
                d0, d1 = det3(cells), det3(new)
                ni, ok = image_counts(new, pbc, cutoff)
                ok &= np.isfinite(new).all(axis=(1, 2)) & np.isfinite(d1) & (d0 * d1 > 0.0)
                ok &= (~pbc | ((ni >= 1) & (ni <= nimg0))).all(axis=1)
            reason[live & ~ok] = 3
            live &= ok
            if not live.any():
                continue
        la = live[atom_chain]
        r_prev[la], v_prev[la] = pos[la], vel[la]
        c_prev[live] = cells[live]
        if baro:
            cells[live] = new[live]
        pos[la] = pos[la] * mu[atom_chain[la]]
        free = la & ~held
        vel[free] = (vel[free] * lam[atom_chain[free], None]) / vdiv[atom_chain[free], None]
        if langevin:
            m = free
            nn = n[atom_chain[m]]
            z = mo.normals3(keys[m], nn, atom_idx[m], mo.TAG_LANGEVIN)
            sigma = np.sqrt(c2 * kT[atom_chain[m]] * ACC / mass[m])[:, None]
            v = vel[m] + hdt * acc[m]
            x = pos[m] + hdt * v
            v = c1 * v + sigma * z
            x = x + hdt * v
            vel[m], pos[m] = v, x
        else:
            vel[free] += hdt * acc[free]
            pos[free] += dt * vel[free]
        opened[live] = True
    return {"positions": pos, "velocities": vel, "cells": cells, **rec, "n_done": steps.astype(np.int32), "stop_reason": reason.astype(np.int32),
            "n_eval": n_eval}


# ---- cases the CPU rehearsals and the device tests share ----------------------------------------------------------------------------
def ideal_gas_case(n_chains=1024, n_atoms=8, seed=5):
    """The stochastic-cell-rescaling check: ``n_chains`` boxes of 10 A with ``n_atoms`` free particles that never interact (the device
    runs it on a pair handle with zero well depth and a 1 A cutoff, so no chain comes near the image-count stop).  Stationary density of
    the contract's Euler form: p(V) ~ V^N exp(-P0 V / kT), so <V> = (N + 1) kT / P0 and Var V = (N + 1)(kT / P0)^2.  P0 puts <V> at
    1500 A^3, half as much again as the boxes start with, so a barostat that does nothing fails by 32 standard errors.  With
    beta = 1 / P0 the mean volume relaxes as exp(-t / taup): 600 steps of 2 fs are 6 taup (500 A^3 exp(-6) = 1.2 A^3 left, 0.08 standard
    errors), and dt / taup = 0.01 keeps the time-step bias of the Euler form below one standard error (at 0.02 it is +1.3 of them);
    the Langevin friction equilibrates the particles within ~10 steps.  The last step is sampled: 1024 independent chains.
    Returns (positions [B n, 3], cells, masses, cfg_start, keywords of ``run``, (mean, standard error of the 1024-chain mean))."""
    T, L, v_mean = 300.0, 10.0, 1500.0
    kT = KB * T
    p0 = (n_atoms + 1) * kT / v_mean
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, L, (n_chains * n_atoms, 3))
    cells = np.tile(np.eye(3) * L, (n_chains, 1, 1))
    mass = np.full(n_chains * n_atoms, 39.948)
    kw = dict(n_steps=600, dt=2.0, thermostat="langevin", barostat="crescale", temperature=T, friction=0.05, taup=200.0, pressure=p0,
              compressibility=1.0 / p0, seed=seed, thermo_interval=600)
    se = np.sqrt((n_atoms + 1) * (kT / p0) ** 2 / n_chains)
    return pos, cells, mass, np.arange(n_chains + 1) * n_atoms, kw, (v_mean, se)


def no_forces(pos, cells):
    B = len(cells)
    return np.zeros(B), np.zeros_like(pos), np.zeros((B, 6))


FCC = dict(eps=0.0104, sigma=3.4, rc=8.5, a0=5.3)      # lj/cut argon in the 4-atom conventional cell, slightly expanded (minimum near 5.24 A:
FCC_P0 = 0.001                                         # the fifth shell stays inside rc, the sixth outside); target pressure, eV / A^3


def fcc_cell(a):
    frac = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]], float)
    return frac * a, np.eye(3) * a


def lj_fcc_energy(a, eps=0.0104, sigma=3.4, rc=8.5, **_):
    """Energy of the 4-atom fcc cell under lj/cut (unshifted) by a direct lattice sum."""
    pos, cell = fcc_cell(a)
    n = int(np.ceil(rc / a)) + 1
    sh = np.array([[i, j, k] for i in range(-n, n + 1) for j in range(-n, n + 1) for k in range(-n, n + 1)], float) * a
    d = pos[None, :, None, :] - pos[:, None, None, :] + sh[None, None, :, :]
    r2 = (d * d).sum(axis=3)
    m = (r2 < rc * rc) & (r2 > 1e-12)
    s6 = np.where(m, (sigma * sigma / np.where(m, r2, 1.0)) ** 3, 0.0)
    return 0.5 * (4 * eps * (s6 * s6 - s6)).sum()


def lj_fcc_pressure_and_modulus(a, h=1e-4, **kw):
    """P = -dE/dV and K = -V dP/dV of the static lattice by central differences in a (no pair crosses rc between a - 2h and a + 2h is the
    caller's to check: E(a) is smooth there)."""
    V = lambda x: x ** 3
    P = lambda x: -(lj_fcc_energy(x + h, **kw) - lj_fcc_energy(x - h, **kw)) / (V(x + h) - V(x - h))
    K = -V(a) * (P(a + h) - P(a - h)) / (V(a + h) - V(a - h))
    return P(a), K
