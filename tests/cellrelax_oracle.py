"""numpy restatement of the device variable-cell relaxation (vssr_batch_relax_cell, csrc/relax_cell.hip): ASE's ``UnitCellFilter`` under
ASE's ``FIRE``, one chain at a time, in fp64.  TEST INFRASTRUCTURE, and the contract of the device code.

Restated from ASE as remembered (ase/filters.py ``UnitCellFilter``, ase/optimize/fire.py); ASE is not installed where this was written,
so nothing here is pinned by an executed ASE.  What pins the filter algebra instead is tests/test_cellrelax_cpu.py: the N + 3 row force
below is the exact negative gradient of the enthalpy E + p V with respect to the N + 3 rows the optimizer sees.

Row vectors; the rows of a cell are the lattice vectors.  Fixed per chain at the start: C0 (the cell) and c (``cell_factor``, default:
the atom count).  State: s [N, 3] and the deformation gradient F [3, 3], from s = x, F = I.  Physical state: x = s F^T, C = C0 F^T.
The optimizer's N + 3 rows are s and c F.  Row forces, in this order:

    1. atoms   g_i = f_i F; rows of held atoms are zero (they ride the cell through x = s F^T)
    2. cell    W = -V (sigma + p I) F^-T,  V = |det C|, sigma the 3 x 3 of the Voigt stress (ASE's sign), p = scalar_pressure
    3. hydrostatic_strain:  W <- (tr W / 3) I
    4. W <- W o mask, the 3 x 3 of 0 / 1 from the Voigt-6 mask (xx yy zz yz xz xy)
    5. the three cell rows are W / c

Convergence is ASE's over all N + 3 rows: max_row |row| < fmax, tested when a step opens.  The step is ASE FIRE over the 3 N + 9
numbers in the form of csrc/fire_dev.h (v' = c1 v + c2 G, |dt v'| from the three sums v.v, v.G, G.G, clamped to maxstep as a whole);
the cell rows move F by (step of c F) / c.

Stops: 1 converged; 2 max_steps; 3 a non-finite energy, force or stress (the state goes back to where the step opened, that step is
not counted); 4 the step's new cell would need more periodic images along an axis than the starting cell (``image_counts``), or has
det F <= 0, or is not finite: the step is not taken, the chain stays at the state it was evaluated at.
"""

from __future__ import annotations

import numpy as np

import strain_fd as sf

STOP_REASONS = {1: "converged", 2: "max steps", 3: "non-finite energy, force or stress", 4: "cell left the image range or degenerated"}
FIRE_DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)


def mask33(mask6):
    """3 x 3 of 0 / 1 from a Voigt-6 mask; ``ValueError`` for an entry other than 0 or 1."""
    m = np.asarray(mask6, np.float64).reshape(6)
    if not np.isin(m, (0.0, 1.0)).all():
        raise ValueError(f"mask {mask6!r}: entries 0 or 1 wanted")
    return sf.voigt_to_tensor(m)


def image_counts(cell, pbc, cutoff):
    """floor(cutoff / height) + 1 per periodic axis, 0 on an open one: csrc/cell_dev.h."""
    C = np.asarray(cell, np.float64).reshape(3, 3)
    vol = abs(np.linalg.det(C))
    out = np.zeros(3, np.int64)
    for k in range(3):
        if pbc[k]:
            n = np.cross(C[(k + 1) % 3], C[(k + 2) % 3])
            out[k] = int(np.floor(cutoff / (vol / np.sqrt(np.vdot(n, n))))) + 1
    return out


def row_forces(f, sigma6, F, volume, scalar_pressure=0.0, mask=(1, 1, 1, 1, 1, 1), hydrostatic_strain=False, cell_factor=1.0, fixed=None):
    """The N + 3 row forces of the docstring from atom forces f [N, 3], the Voigt stress, F, V = |det C|."""
    f = np.asarray(f, np.float64).reshape(-1, 3)
    G = np.zeros((len(f) + 3, 3))
    G[:-3] = f @ F
    if fixed is not None:
        G[:-3][np.asarray(fixed, bool)] = 0.0
    W = -volume * (sf.voigt_to_tensor(sigma6) + scalar_pressure * np.eye(3)) @ np.linalg.inv(F).T
    if hydrostatic_strain:
        W = np.eye(3) * (np.trace(W) / 3.0)
    W = W * mask33(mask)
    G[-3:] = W / cell_factor
    return G


def enthalpy(energy_fn, rows, C0, cell_factor, scalar_pressure=0.0):
    """E + p V at the optimizer's rows [N + 3, 3] (s and c F); ``energy_fn(x, C) -> E``."""
    F = rows[-3:] / cell_factor
    C = C0 @ F.T
    return float(energy_fn(rows[:-3] @ F.T, C)) + scalar_pressure * abs(np.linalg.det(C))


def relax_chain(eval_fn, pos, cell, pbc, cutoff, fixed=None, max_steps=100, fmax=0.05, dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1,
                fdec=0.5, astart=0.1, fa=0.99, scalar_pressure=0.0, mask=(1, 1, 1, 1, 1, 1), hydrostatic_strain=False, cell_factor=0.0,
                record=None):
    """``eval_fn(x [N, 3], C [3, 3]) -> (E, f [N, 3], sigma [6])``; ``fixed``: bool / 0-1 mask [N] or None.  Returns a dict: positions,
    cell, n_steps, stop_reason, fmax, energy, volume (the last three as of the last convergence test), F."""
    C0 = np.array(cell, np.float64).reshape(3, 3)
    s = np.array(pos, np.float64).reshape(-1, 3)
    n = len(s)
    held = np.zeros(n, bool) if fixed is None else np.asarray(fixed).astype(bool).reshape(n)
    c = float(cell_factor) if cell_factor > 0 else float(n)
    mask33(mask)                                   # (ValueError before anything is evaluated)
    F = np.eye(3)
    nimg0 = image_counts(C0, pbc, cutoff)
    v = np.zeros((n + 3, 3))
    has_v, a, nsteps_pos, steps = False, astart, 0, 0
    s_open, F_open = s.copy(), F.copy()
    res = [np.nan, np.nan, np.nan]
    while True:
        x, C = s @ F.T, C0 @ F.T
        with np.errstate(all="ignore"):
            E, f, sig = eval_fn(x, C)
        f, sig = np.asarray(f, np.float64).reshape(n, 3), np.asarray(sig, np.float64).reshape(6)
        if not (np.isfinite(E) and np.isfinite(f).all() and np.isfinite(sig).all()):
            s, F = s_open, F_open
            steps = max(steps - 1, 0)
            reason = 3
            break
        V = abs(np.linalg.det(C))
        G = row_forces(f, sig, F, V, scalar_pressure, mask, hydrostatic_strain, c, held)
        fm2 = float((G * G).sum(axis=1).max())
        res = [np.sqrt(fm2), float(E), V]
        rec = None
        if record is not None:
            rec = dict(step=steps, positions=x.copy(), cell=C.copy(), F=F.copy(), fmax=res[0], energy=float(E), volume=V, branches=set())
            record.append(rec)
        if fm2 < fmax * fmax:
            reason = 1
            break
        if steps >= max_steps:
            reason = 2
            break
        vG, GG, vv = float(np.vdot(v, G)), float(np.vdot(G, G)), float(np.vdot(v, v))
        mix, mix_a, mix_s, c1 = False, 0.0, 0.0, 0.0
        if has_v:
            if vG > 0.0:
                mix, mix_a, mix_s = True, a, a * np.sqrt(vv / GG)
                c1 = 1.0 - mix_a
                if nsteps_pos > nmin:
                    dt, a = min(dt * finc, dtmax), a * fa
                nsteps_pos += 1
            else:
                a, dt, nsteps_pos = astart, dt * fdec, 0
        c2 = mix_s + dt
        normdr = dt * np.sqrt((c1 * c1) * vv + (2.0 * c1 * c2) * vG + (c2 * c2) * GG)
        scale = maxstep / normdr if normdr > maxstep else 1.0
        vn = ((1.0 - mix_a) * v + mix_s * G if mix else np.zeros_like(v)) + dt * G
        Fn = F + (scale * (dt * vn[-3:])) / c
        if rec is not None:
            rec["branches"] |= {"mix" if mix else ("first" if not has_v else "uphill"), "clip" if scale != 1.0 else "noclip"}
            rec["normdr_rel"] = float(normdr / maxstep)
        Cn = C0 @ Fn.T
        bad = not np.isfinite(Cn).all() or not np.linalg.det(Fn) > 0.0
        if not bad:
            ni = image_counts(Cn, pbc, cutoff)
            bad = bool(((ni > nimg0) | ((ni < 1) & np.asarray(pbc, bool))).any())
        if bad:
            reason = 4
            break
        s_open, F_open = s, F
        s = s + scale * (dt * vn[:-3])
        F, v, has_v = Fn, vn, True
        steps += 1
    return dict(positions=s @ F.T, cell=C0 @ F.T, n_steps=steps, stop_reason=reason, fmax=res[0], energy=res[1], volume=res[2], F=F)


def run(eval_fn, structs, fixed=None, record=None, **kw):
    """A batch: ``structs`` as backend.pack_batch takes them ((types, pos, cell, pbc), ...), ``eval_fn(b, x, C)``, ``fixed`` a mask
    [sum N] or None, ``cutoff`` in ``kw``.  Returns dict(positions [sum N, 3], cells [B, 3, 3], n_steps, stop_reason, result [B, 3])."""
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])]).astype(np.int64)
    out = dict(positions=[], cells=[], n_steps=[], stop_reason=[], result=[])
    for b, st in enumerate(structs):
        rec = None if record is None else []
        r = relax_chain(lambda x, C, b=b: eval_fn(b, x, C), st[1], st[2], st[3], fixed=None if fixed is None else fixed[start[b]:start[b + 1]],
                        record=rec, **kw)
        if record is not None:
            record.append(rec)
        out["positions"].append(r["positions"])
        out["cells"].append(r["cell"])
        out["n_steps"].append(r["n_steps"])
        out["stop_reason"].append(r["stop_reason"])
        out["result"].append([r["fmax"], r["energy"], r["volume"]])
    return dict(positions=np.vstack(out["positions"]), cells=np.array(out["cells"]), n_steps=np.array(out["n_steps"], np.int32),
                stop_reason=np.array(out["stop_reason"], np.int32), result=np.array(out["result"]))


# ---- stresses for the CPU restatements of the potentials, which return (E, e_atom, forces) only ------------------------------------
def pair_virial(terms, charges, types, pos, cell, pbc):
    """(E, forces, sigma [6]) of tests/pair_oracle.py's model with the exact virial: dE / d eps_ab = sum over pairs E'(r) r_a r_b / r."""
    import pair_oracle as po
    from cell_cases import brute_neighbors

    E, _, f = po.pair(terms, charges, types, pos, cell, pbc)
    types = np.asarray(types, np.int64)
    q = np.zeros(int(types.max()) + 1) if charges is None else np.asarray(charges, np.float64)
    i, j, _, rv = brute_neighbors(np.asarray(pos, np.float64).reshape(-1, 3), cell, pbc, po.cutoff(terms))
    d = np.sqrt((rv * rv).sum(axis=1))
    ti, tj = types[i.astype(np.int64)], types[j.astype(np.int64)]
    de = np.zeros(len(d))
    for a, b, style, c, rc, shift in terms:
        name = po.STYLE.get(style, style)
        m = (((ti == a) & (tj == b)) | ((ti == b) & (tj == a))) & (d < rc)
        if m.any():
            de[m] += po.term_energy(name, c, rc, d[m], qq=q[a] * q[b] if name == "coul/dsf" else 0.0, shift=shift)[1]
    W = 0.5 * np.einsum("e,ea,eb->ab", de / d, rv, rv)          # every pair is two directed edges
    return E, f, sf.tensor_to_voigt(W) / abs(np.linalg.det(np.asarray(cell, np.float64).reshape(3, 3)))


def isotropic_fd_eval(one, h=1e-4):
    """``one(x, C) -> (E, e_atom, forces)`` of a CPU restatement with a smooth cutoff -> ``eval_fn(x, C) -> (E, forces, sigma)`` for a run
    under ``hydrostatic_strain`` from an isotropic start, where only tr sigma is read: sigma = (dE / d eta) / (3 V) I under
    x -> (1 + eta) x, Richardson-extrapolated central differences at h and 2 h (four evaluations; strain_fd.fd_stress takes 36)."""
    def fn(x, C):
        E, _, f = one(x, C)[:3]
        D = [(one(x * (1 + k * h), C * (1 + k * h))[0] - one(x * (1 - k * h), C * (1 - k * h))[0]) / (2 * k * h) for k in (1, 2)]
        p = (4 * D[0] - D[1]) / 3.0 / (3.0 * abs(np.linalg.det(C)))
        return E, f, np.array([p, p, p, 0.0, 0.0, 0.0])
    return fn
