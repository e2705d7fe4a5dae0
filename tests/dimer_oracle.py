"""numpy restatement of the device dimer method (``vssr_batch_dimer``, csrc/dimer.hip): the checker of the device code.
TEST INFRASTRUCTURE.  Min-mode following from one structure: the dimer of Henkelman & Jonsson, J. Chem. Phys. 111, 7010 (1999), with the
one-gradient rotation of Heyden, Bell & Keil, J. Chem. Phys. 123, 224101 (2005) and the force extrapolation of Kaestner & Sherwood,
J. Chem. Phys. 128, 014106 (2008), translated by ASE's FIRE as csrc/neb.hip restates it.  Restated from the three papers; it is NOT ASE's
``MinModeTranslate`` and no library was executed: this file is the contract, pinned by its own physics anchor (tests/test_dimer_cpu.py).

A batch is ``pos`` [sum N, 3] with ``start`` [B + 1], B = 2 G; dimer g is chains 2 g (the midpoint x0) and 2 g + 1 (the moving end
x0 + delta N, whose input positions are ignored).  ``force_fn(pos) -> (E [B], F [sum N, 3])`` evaluates the whole batch, as the device's
lock-step evaluation does.  ``record``: a list that receives one dict per dimer and decision: ``branches`` (a set of names from
``BRANCHES``) and ``margins`` (name of the comparison -> its relative margin), for the census and the margins of tests/dimer_cases.py."""
import numpy as np

import md_oracle as mo

STOP_REASONS = {1: "converged", 2: "max steps", 3: "non-finite energy or force"}
FIRE_DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)
TAG_DIMER = 2        # the Philox draw tag of a starting mode (md_oracle: 0 Maxwell-Boltzmann, 1 Langevin), at draw index n = 0
BRANCHES = ("rotate", "no_rotate_phi_tol", "no_rotate_counter", "no_rotate_f_zero", "phi_plus_half_pi", "phi_kept",
            "translate_convex", "translate_saddle", "first", "uphill_reset", "downhill_hold", "downhill_grow", "dtmax_clamp",
            "clip", "noclip", "reason1", "reason2", "reason3_at_E", "reason3_at_R")
# the comparisons whose margins are recorded: phi1 against phi_tol, Cm against C, C against 0 (twice: the step test and the choice of
# G), fmax, FIRE's power against 0, |dt v| against maxstep
COMPARISONS = ("phi_tol", "cm_c", "c_zero", "fmax", "power", "maxstep")


def draw_modes(seed, dimer_id, sizes):
    """Standard normals [sum n, 3] of the dimers' starting modes, keyed by (seed, dimer id, atom, component); sizes [G]."""
    keys = mo.chain_keys(seed, dimer_id)
    out = []
    for g, n in enumerate(sizes):
        out.append(mo.normals3(np.broadcast_to(keys[g], (n, 2)), 0, np.arange(n), TAG_DIMER))
    return out


def _rel(a, b):
    s = max(abs(a), abs(b))
    return abs(a - b) / s if s > 0 else 0.0


def run(force_fn, pos, start, fixed=None, modes=None, dimer_id=None, seed=0, max_steps=100, max_rot_first=8, max_rot=1, delta=0.01,
        phi_tol=np.pi / 180.0, fmax=0.05, displace=0.0, dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99,
        record=None):
    """Returns dict(positions [sum N, 3], energies [B], modes [sum N, 3] (zero on the odd chains), fmax / curvature / e0 / f_perp [G],
    n_steps / stop_reason / n_rot / n_eval [G]).  fmax, curvature, e0 and f_perp of a dimer that stopped with reason 3 are those of its
    last complete test and not part of the contract."""
    pos = np.array(pos, np.float64).reshape(-1, 3)
    start = np.asarray(start, np.int64)
    B = len(start) - 1
    assert B % 2 == 0
    G = B // 2
    held_all = np.zeros(len(pos), bool) if fixed is None else np.asarray(fixed).astype(bool).reshape(-1)
    ids = np.arange(G) if dimer_id is None else np.asarray(dimer_id)
    sizes = [int(start[2 * g + 1] - start[2 * g]) for g in range(G)]
    drawn = draw_modes(seed, ids, sizes) if modes is None else None
    S = []
    for g in range(G):
        a0, n = start[2 * g], sizes[g]
        assert start[2 * g + 2] - start[2 * g + 1] == n
        held = held_all[a0:a0 + n]
        N = np.array(drawn[g] if modes is None else np.asarray(modes, np.float64).reshape(-1, 3)[a0:a0 + n], np.float64)
        N[held] = 0.0
        nn = np.vdot(N, N)
        if not (nn > 0.0 and np.isfinite(nn)):
            raise ValueError(f"dimer {g}: the mode has no length over the free atoms")
        N = N / np.sqrt(nn)
        x0 = pos[a0:a0 + n] + displace * N
        pos[a0:a0 + n] = x0
        pos[a0 + n:a0 + 2 * n] = x0 + delta * N
        S.append(dict(a0=a0, n=n, held=held, N=N, x0=x0.copy(), xopen=x0.copy(), Nopen=N.copy(), phase="E", rot=0, steps=0, reason=0,
                      n_rot=0, n_eval=0, v=None, dt=dt, a=astart, nsteps_pos=0, fmax=0.0, C=0.0, e0=0.0, f=0.0))

    def put(s):
        pos[s["a0"]:s["a0"] + s["n"]] = s["x0"]
        pos[s["a0"] + s["n"]:s["a0"] + 2 * s["n"]] = s["x0"] + delta * s["N"]

    def note(s, g, branches, margins, closed=None):
        if record is not None:
            record.append(dict(dimer=g, steps=s["steps"], rot=s["rot"], branches=set(branches), margins=dict(margins), closed=closed, fmax_atom=s["fmax"]))

    def trial(s):
        return s["N"] * np.cos(s["phi1"]) + s["theta"] * np.sin(s["phi1"])

    while not all(s["reason"] for s in S):
        E, F = force_fn(pos)
        E, F = np.asarray(E, np.float64), np.asarray(F, np.float64).reshape(-1, 3)
        for g, s in enumerate(S):
            if s["reason"]:
                continue
            a0, n, held, br, mg = s["a0"], s["n"], s["held"], set(), {}
            s["n_eval"] += 1
            closed = None
            Fa, Fb = F[a0:a0 + n], F[a0 + n:a0 + 2 * n]
            if not (np.isfinite(E[2 * g]) and np.isfinite(E[2 * g + 1]) and np.isfinite(Fa).all() and np.isfinite(Fb).all()):
                # back to the x0 and N the step opened at; that step is not counted
                br.add("reason3_at_" + s["phase"])
                s["x0"], s["N"] = s["xopen"].copy(), s["Nopen"].copy()
                if s["steps"] > 0:
                    s["steps"] -= 1
                s["reason"] = 3
                put(s)
                note(s, g, br, mg, closed)
                continue
            if s["phase"] == "E":
                s["F0"] = np.where(held[:, None], 0.0, Fa)
                s["F1"] = np.where(held[:, None], 0.0, Fb)
                s["e0"] = float(E[2 * g])
                s["C"] = (np.vdot(s["F0"], s["N"]) - np.vdot(s["F1"], s["N"])) / delta
                s["rot"] = 0
            else:
                F1s = np.where(held[:, None], 0.0, Fb)
                Ns, phi1, b1, C, F0 = trial(s), s["phi1"], s["b1"], s["C"], s["F0"]
                C1 = (np.vdot(F0, Ns) - np.vdot(F1s, Ns)) / delta
                a1 = (C - C1 + b1 * np.sin(2.0 * phi1)) / (1.0 - np.cos(2.0 * phi1))
                a0_ = 2.0 * (C - a1)
                with np.errstate(all="ignore"):
                    phim = 0.5 * np.arctan(np.float64(b1) / np.float64(a1))
                Cm = 0.5 * a0_ + a1 * np.cos(2.0 * phim) + b1 * np.sin(2.0 * phim)
                mg["cm_c"] = _rel(Cm, C)
                if Cm > C:
                    br.add("phi_plus_half_pi")
                    phim += 0.5 * np.pi
                    Cm = 0.5 * a0_ + a1 * np.cos(2.0 * phim) + b1 * np.sin(2.0 * phim)
                else:
                    br.add("phi_kept")
                s["F1"] = (np.sin(phi1 - phim) / np.sin(phi1)) * s["F1"] + (np.sin(phim) / np.sin(phi1)) * F1s \
                    + (1.0 - np.cos(phim) - np.sin(phim) * np.tan(0.5 * phi1)) * F0
                Nn = s["N"] * np.cos(phim) + s["theta"] * np.sin(phim)
                s["N"] = Nn / np.sqrt(np.vdot(Nn, Nn))
                s["C"] = float(Cm)
                hn = float(np.sqrt(np.vdot(F0 - F1s, F0 - F1s))) / delta
                closed = dict(f=s["f"], phi1=phi1, a1=float(a1), b1=b1, hn=hn)      # the conditioning of this rotation, for bounds
                s["rot"] += 1
                s["n_rot"] += 1
            # the rotation test
            F0, F1, N, C = s["F0"], s["F1"], s["N"], s["C"]
            Fd = 2.0 * (F1 - F0)
            Fp = Fd - np.vdot(Fd, N) * N
            f = float(np.sqrt(np.vdot(Fp, Fp)))
            s["f"] = f
            b1 = -f / (2.0 * delta)
            with np.errstate(all="ignore"):
                phi1 = float(0.5 * np.arctan(np.float64(f) / np.float64(2.0 * delta * abs(C))))
            limit = max_rot_first if s["steps"] == 0 else max_rot
            if not s["rot"] < limit:
                br.add("no_rotate_counter")
            elif not f > 0.0:
                br.add("no_rotate_f_zero")
            else:
                mg["phi_tol"] = _rel(phi1, phi_tol)
                if phi1 >= phi_tol:
                    br.add("rotate")
                    s["theta"], s["phi1"], s["b1"] = Fp / f, phi1, b1
                    pos[a0 + n:a0 + 2 * n] = s["x0"] + delta * trial(s)
                    s["phase"] = "R"
                    note(s, g, br, mg, closed)
                    continue
                br.add("no_rotate_phi_tol")
            # the step test, on F0 of the last evaluation E
            s["phase"] = "E"
            fm2 = float((F0 * F0).sum(axis=1).max())
            s["fmax"] = np.sqrt(fm2)
            f0n, f1n = np.vdot(F0, N), np.vdot(F1, N)
            mg["fmax"] = _rel(s["fmax"], fmax)
            mg["c_zero"] = abs(C) * delta / max(abs(f0n) + abs(f1n), 1e-300)
            if fm2 < fmax * fmax and C < 0.0:
                br.add("reason1")
                s["reason"] = 1
                put(s)
                note(s, g, br, mg, closed)
                continue
            if s["steps"] >= max_steps:
                br.add("reason2")
                s["reason"] = 2
                put(s)
                note(s, g, br, mg, closed)
                continue
            if C < 0.0:
                br.add("translate_saddle")
                Gv = F0 - (2.0 * f0n) * N
            else:
                br.add("translate_convex")
                Gv = (-f0n) * N
            if s["v"] is None:
                v = np.zeros_like(Gv)
                br.add("first")
            else:
                v = s["v"]
                vG, GG, vv = np.vdot(v, Gv), np.vdot(Gv, Gv), np.vdot(v, v)
                mg["power"] = abs(vG) / max(np.sqrt(vv * GG), 1e-300)
                if vG > 0.0:
                    v = (1.0 - s["a"]) * v + (s["a"] * np.sqrt(vv / GG)) * Gv
                    if s["nsteps_pos"] > nmin:
                        br.add("dtmax_clamp" if s["dt"] * finc > dtmax else "downhill_grow")
                        s["dt"] = min(s["dt"] * finc, dtmax)
                        s["a"] *= fa
                    else:
                        br.add("downhill_hold")
                    s["nsteps_pos"] += 1
                else:
                    br.add("uphill_reset")
                    v = np.zeros_like(Gv)
                    s["a"] = astart
                    s["dt"] *= fdec
                    s["nsteps_pos"] = 0
            v = v + s["dt"] * Gv
            dr = s["dt"] * v
            normdr = float(np.sqrt(np.vdot(dr, dr)))
            mg["maxstep"] = _rel(normdr, maxstep)
            if normdr > maxstep:
                br.add("clip")
                dr = (maxstep / normdr) * dr
            else:
                br.add("noclip")
            s["v"] = v
            s["xopen"], s["Nopen"] = s["x0"].copy(), N.copy()
            s["x0"] = s["x0"] + dr
            s["steps"] += 1
            put(s)
            note(s, g, br, mg, closed)
    E, F = force_fn(pos)
    modes_out = np.zeros_like(pos)
    for s in S:
        modes_out[s["a0"]:s["a0"] + s["n"]] = s["N"]
    arr = lambda k, t=np.float64: np.array([s[k] for s in S], t)
    return dict(positions=pos, energies=np.asarray(E, np.float64), modes=modes_out, fmax=arr("fmax"), curvature=arr("C"), e0=arr("e0"),
                f_perp=arr("f"), n_steps=arr("steps", np.int32), stop_reason=arr("reason", np.int32), n_rot=arr("n_rot", np.int32),
                n_eval=arr("n_eval", np.int32))
