"""numpy restatement of the device nudged elastic band (``vssr_batch_neb``, csrc/neb.hip): the checker of the device code.
TEST INFRASTRUCTURE.  The improved tangent (Henkelman & Jonsson, J. Chem. Phys. 113, 9978 (2000)), ASE's ``aseneb`` method, the
climbing image (Henkelman, Uberuaga & Jonsson, J. Chem. Phys. 113, 9901 (2000)) and ASE's FIRE over the concatenated interior images of
a band, restated from the papers and from ASE's neb.py / fire.py as remembered.  ASE was NOT executed: this file is the contract, and it
is pinned by its own physics anchor (tests/test_neb_cpu.py).

A batch is ``pos`` [sum N, 3] with ``start`` [B + 1]; band g is ``n_img[g]`` consecutive chains.  ``force_fn(pos) -> (E [B], F [sum N, 3])``
evaluates the whole batch, as the device's lock-step evaluation does.  ``record``: a list that receives one dict per band and test
(the branches taken), for the census of tests/neb_cases.py."""
import numpy as np

METHODS = ("improvedtangent", "aseneb")
STOP_REASONS = {1: "converged", 2: "max steps", 3: "non-finite energy or force", 4: "zero tangent"}
FIRE_DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)
BRANCHES = ("tangent_up", "tangent_down", "tangent_extremum_rising", "tangent_extremum_falling", "tangent_tie",
            "ase_below", "ase_above", "ase_at", "climb", "noclimb",
            "first", "uphill_reset", "downhill_hold", "downhill_grow", "dtmax_clamp", "clip", "noclip", "clip_band_only")


def mic(d, cell, pbc):
    """Displacements [N, 3] to the nearest image along the periodic axes: whole lattice vectors rint(d cell^-1) taken off."""
    d = np.asarray(d, np.float64)
    pbc = np.asarray(pbc).astype(bool)
    if not pbc.any():
        return d.copy()
    cell = np.asarray(cell, np.float64)
    n = np.rint(d @ np.linalg.inv(cell))
    n[:, ~pbc] = 0.0
    return d - n @ cell


def first_max(e):
    """Index of the first interior image of maximal energy."""
    imax, emax = 1, e[1]
    for j in range(2, len(e) - 1):
        if e[j] > emax:
            imax, emax = j, e[j]
    return imax


def neb_forces(x, e, F, cell, pbc, held, k, climb, method, branches=None):
    """x [n, N, 3], e [n], F [n, N, 3] (raw) of one band -> (G [n, N, 3], imax, zero_tangent).  held: bool [N]."""
    n = len(x)
    Fz = np.where(held[None, :, None], 0.0, F)
    G = np.zeros_like(x)
    imax = first_max(e)
    zero = False
    for i in range(1, n - 1):
        t1 = mic(x[i] - x[i - 1], cell, pbc)
        t2 = mic(x[i + 1] - x[i], cell, pbc)
        climbing = bool(climb) and i == imax
        if branches is not None:
            branches.add("climb" if climbing else "noclimb")
        if method == "improvedtangent":
            if e[i + 1] > e[i] > e[i - 1]:
                al, be, name = 1.0, 0.0, "tangent_up"
            elif e[i + 1] < e[i] < e[i - 1]:
                al, be, name = 0.0, 1.0, "tangent_down"
            else:
                dp, dm = abs(e[i + 1] - e[i]), abs(e[i - 1] - e[i])
                dmax, dmin = max(dp, dm), min(dp, dm)
                if e[i + 1] > e[i - 1]:
                    al, be, name = dmax, dmin, "tangent_extremum_rising"
                else:
                    al, be, name = dmin, dmax, "tangent_tie" if e[i + 1] == e[i - 1] else "tangent_extremum_falling"
            t = al * t2 + be * t1
            tt = np.vdot(t, t)
            if not tt > 0.0:                        # two coincident images: G = F here, the band stops unless it has converged
                zero = True
                G[i] = Fz[i]
                continue
            t = t / np.sqrt(tt)
            fpar = np.vdot(Fz[i], t)
            if climbing:
                g = Fz[i] + (-2.0 * fpar) * t
            else:
                g = Fz[i] + (-fpar + k * (np.sqrt(np.vdot(t2, t2)) - np.sqrt(np.vdot(t1, t1)))) * t
        elif method == "aseneb":
            if i < imax:
                t, name = t2, "ase_below"
            elif i > imax:
                t, name = t1, "ase_above"
            else:
                t, name = t1 + t2, "ase_at"
            m = np.vdot(t, t)
            if not m > 0.0:
                zero = True
                G[i] = Fz[i]
                continue
            fpar = np.vdot(Fz[i], t)
            if climbing:
                g = Fz[i] + (-2.0 * (fpar / m)) * t
            else:
                g = Fz[i] + (-(fpar / m) - np.vdot(k * t1 - k * t2, t) / m) * t
        else:
            raise ValueError(f"NEB method {method!r}")
        if branches is not None:
            branches.add(name)
        G[i] = np.where(held[:, None], 0.0, g)
    return G, imax, zero


def run(force_fn, pos, start, n_img, cells, pbcs, fixed=None, k=0.1, climb=False, method="improvedtangent", fmax=0.05, max_steps=100,
        dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, record=None):
    """Returns dict(positions, energies [B], neb_forces, fmax / barrier_forward / barrier_reverse [G], n_steps / stop_reason / imax [G],
    n_eval).  cells [B, 3, 3], pbcs [B, 3] (those of a band's first image are used).  neb_forces, fmax, the barriers and imax of a
    band that stopped with reason 3 are not part of the contract."""
    pos = np.array(pos, np.float64).reshape(-1, 3)
    start = np.asarray(start, np.int64)
    n_img = [int(v) for v in n_img]
    B, nb = len(start) - 1, len(n_img)
    assert sum(n_img) == B and min(n_img) >= 3
    first = np.concatenate([[0], np.cumsum(n_img)])[:-1]
    held_all = np.zeros(len(pos), bool) if fixed is None else np.asarray(fixed).astype(bool).reshape(-1)
    S = [dict(dt=dt, a=astart, nsteps_pos=0, v=None, steps=0, reason=0, imax=0, fmax=0.0, ef=0.0, er=0.0, xprev=None) for _ in range(nb)]
    Gout = np.zeros_like(pos)
    n_eval = 0
    went_back = False
    E = None
    for it in range(max_steps + 1):
        if all(s["reason"] for s in S):
            break
        E, F = force_fn(pos)
        E, F = np.asarray(E, np.float64), np.asarray(F, np.float64).reshape(-1, 3)
        n_eval += 1
        for g in range(nb):
            s = S[g]
            if s["reason"]:
                continue
            f, n = first[g], n_img[g]
            a0, a1 = start[f], start[f + n]
            nat = start[f + 1] - start[f]
            x = pos[a0:a1].reshape(n, nat, 3)
            e = E[f:f + n]
            Fg = F[a0:a1].reshape(n, nat, 3)
            held = held_all[a0:a0 + nat]
            br = set()
            bad = not (np.isfinite(e).all() and np.isfinite(Fg).all())
            if not bad:
                G, imax, zero = neb_forces(x, e, Fg, cells[f], pbcs[f], held, k, climb, method, br)
                bad = not np.isfinite(G).all()       # (a non-finite position difference)
            if bad:      # back to the positions the step opened at; that step is not counted
                if s["v"] is not None:
                    pos[a0:a1] = s["xprev"]
                    s["steps"] -= 1
                    went_back = True
                s["reason"] = 3
                continue
            Gout[a0:a1] = G.reshape(-1, 3)
            fm2 = float((G * G).sum(axis=2).max())
            s["imax"], s["fmax"], s["ef"], s["er"] = imax, np.sqrt(fm2), e[imax] - e[0], e[imax] - e[-1]
            rec = None
            if record is not None:
                rec = dict(band=g, it=it, steps=s["steps"], branches=br, imax=imax, fmax=s["fmax"])
                record.append(rec)
            if fm2 < fmax * fmax:
                s["reason"] = 1
                continue
            if zero:
                s["reason"] = 4
                continue
            if s["steps"] >= max_steps:
                s["reason"] = 2
                continue
            # ASE FIRE over the interior images of the band
            Gi = G[1:-1]
            if s["v"] is None:
                v = np.zeros_like(Gi)
                br.add("first")
            else:
                v = s["v"]
                vf = np.vdot(Gi, v)
                if vf > 0.0:
                    v = (1.0 - s["a"]) * v + s["a"] * np.sqrt(np.vdot(v, v) / np.vdot(Gi, Gi)) * Gi
                    if s["nsteps_pos"] > nmin:
                        br.add("dtmax_clamp" if s["dt"] * finc > dtmax else "downhill_grow")
                        s["dt"] = min(s["dt"] * finc, dtmax)
                        s["a"] *= fa
                    else:
                        br.add("downhill_hold")
                    s["nsteps_pos"] += 1
                else:
                    br.add("uphill_reset")
                    v = np.zeros_like(Gi)
                    s["a"] = astart
                    s["dt"] *= fdec
                    s["nsteps_pos"] = 0
            v = v + s["dt"] * Gi
            dr = s["dt"] * v
            normdr = np.sqrt(np.vdot(dr, dr))
            if normdr > maxstep:
                br.add("clip")
                if max(np.sqrt(np.vdot(d, d)) for d in dr) <= maxstep:
                    br.add("clip_band_only")
                dr = (maxstep / normdr) * dr
            else:
                br.add("noclip")
            if rec is not None:
                rec["normdr_rel"] = float(normdr / maxstep)
            s["v"] = v
            s["xprev"] = pos[a0:a1].copy()
            x[1:-1] += dr                     # (x is a view of pos)
            s["steps"] += 1
    if went_back or E is None:
        E, F = force_fn(pos)
    return dict(positions=pos, energies=np.asarray(E, np.float64), neb_forces=Gout, fmax=np.array([s["fmax"] for s in S]),
                barrier_forward=np.array([s["ef"] for s in S]), barrier_reverse=np.array([s["er"] for s in S]),
                n_steps=np.array([s["steps"] for s in S], np.int32), stop_reason=np.array([s["reason"] for s in S], np.int32),
                imax=np.array([s["imax"] for s in S], np.int32), n_eval=n_eval)


def interpolate(x0, x1, n_images, cell, pbc, mic_=True):
    """n_images images from x0 to x1 (both included), linear in the (wrapped) displacement."""
    x0, x1 = np.asarray(x0, np.float64), np.asarray(x1, np.float64)
    d = mic(x1 - x0, cell, pbc) if mic_ else x1 - x0
    return [x0 + d * (i / (n_images - 1)) for i in range(n_images)]


def path(x, cell, pbc):
    """Cumulative |d(i)| along a band x [n, N, 3]."""
    out = [0.0]
    for i in range(len(x) - 1):
        d = mic(x[i + 1] - x[i], cell, pbc)
        out.append(out[-1] + float(np.sqrt(np.vdot(d, d))))
    return np.array(out)
