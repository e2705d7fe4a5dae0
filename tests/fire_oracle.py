"""numpy restatement of ASE's FIRE (ase/optimize/fire.py) for tests: the checker of the device relaxation.
TEST INFRASTRUCTURE.  Parity status: the optimizer trajectory of the reference is not pinned by any stored output
(notebook BFGS traces are trajectory-level only), so this restatement is pinned by its
invariants (energy decrease, final fmax) and is used as a same-algorithm cross-check of the device code.

Three optional arguments serve tests/relax_cases.py (without them nothing changes): ``f32`` rounds the forces to float32 before use,
as the device's optimizer state does for the fp64 potentials (csrc/relax.hip::k_narrow_forces); ``record`` is a list that receives one
dict per iteration (positions before the step, the branches taken, the margins of every decision); ``mutate = (iteration, which)``
takes the OTHER branch of one decision at one iteration (``MUTATIONS``), to show that a trajectory comparison would notice."""

import numpy as np

# branch names of a record, and the decision whose flip leaves each of them
BRANCHES = ("first", "downhill_hold", "downhill_grow", "dtmax_clamp", "uphill_reset", "clip", "noclip", "clip_and_grow")
MUTATIONS = {"first": "first", "downhill_hold": "grow", "downhill_grow": "grow", "dtmax_clamp": "dtmax", "uphill_reset": "vf",
             "clip": "clip", "noclip": "clip", "clip_and_grow": "grow"}


def fire_relax(force_fn, pos, fixed=None, max_steps=20, fmax=0.01, dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1,
               fdec=0.5, astart=0.1, fa=0.99, f32=False, record=None, mutate=None):
    """force_fn(pos) -> (energy, forces[N,3]).  Returns (pos, energies list, n_steps, converged)."""
    pos = np.array(pos, dtype=np.float64)
    mask = np.ones(len(pos), bool)
    if fixed is not None:
        mask[np.asarray(fixed, dtype=np.int64)] = False
    v = None
    a, nsteps_pos, steps = astart, 0, 0
    energies = []
    converged = False
    for it in range(max_steps + 1):
        e, f = force_fn(pos)
        if f32:
            f = np.asarray(f, np.float64).astype(np.float32).astype(np.float64)
        f = np.where(mask[:, None], f, 0.0)
        energies.append(e)
        fm = np.linalg.norm(f, axis=1).max()
        rec = None
        if record is not None:
            rec = dict(it=it, pos=pos.copy(), energy=float(e), fm=float(fm), branches=set())
            record.append(rec)
        if fm < fmax:
            converged = True
            break
        if it == max_steps:
            break
        flip = mutate[1] if mutate is not None and mutate[0] == it else None
        first = v is None
        if first:
            v = np.zeros_like(pos)
            if flip == "first":                 # the other branch of the first step: the velocity taken as present (and zero)
                first = False
            elif rec is not None:
                rec["branches"].add("first")
        if not first:
            vf = np.vdot(f, v)
            if rec is not None:
                nv, nf = np.sqrt(np.vdot(v, v)), np.sqrt(np.vdot(f, f))
                rec["vf_rel"] = float(vf / (nv * nf)) if nv * nf > 0 else None
            if (vf > 0.0) != (flip == "vf"):
                v = (1.0 - a) * v + a * f / np.sqrt(np.vdot(f, f)) * np.sqrt(np.vdot(v, v))
                if (nsteps_pos > nmin) != (flip == "grow"):
                    clamp = dt * finc > dtmax
                    if rec is not None:
                        rec["branches"].add("dtmax_clamp" if clamp else "downhill_grow")
                        rec["dt_rel"] = float(dt * finc / dtmax)
                        rec["grew"] = min(dt * finc, dtmax) > dt
                    dt = min(dt * finc, dtmax) if flip != "dtmax" else (dt * finc if clamp else dtmax)
                    a *= fa
                elif rec is not None:
                    rec["branches"].add("downhill_hold")
                nsteps_pos += 1
            else:
                if rec is not None:
                    rec["branches"].add("uphill_reset")
                v[:] = 0.0
                a = astart
                dt *= fdec
                nsteps_pos = 0
        v = v + dt * f
        dr = dt * v
        normdr = np.sqrt(np.vdot(dr, dr))
        clip = normdr > maxstep
        if rec is not None:
            rec["normdr_rel"] = float(normdr / maxstep)
            rec["branches"].add("clip" if clip else "noclip")
            if clip and rec.get("grew"):
                rec["branches"].add("clip_and_grow")
        if clip != (flip == "clip"):
            dr = maxstep * dr / normdr
        pos = pos + dr
        steps += 1
    return pos, energies, steps, converged
