#!/usr/bin/env python3
"""Device dimer method: microseconds per lock-step evaluation spent beside the evaluation (wall time minus the evaluation's event time
from ``vssr_profile_read``) and in ``k_dimer_advance`` itself, next to what a lock-step FIRE relaxation of the same batch costs per step
in the same run; searches converged per second; the share of chain evaluations that were the idle midpoint of an evaluation R (one
JSON line per measurement).

  (a) the 192-atom Cu(100) slab (EAM alloy tables) with a Cu adatom started 0.4 A from its relaxed hollow towards the bridge, as
      4 / 32 / 96 dimers (two chains each) under dimer ids 0 .. n - 1;
  (b) 128 PaiNN dimers: 128 structures of the bench batch (bench.py's chains), 256 chains.

    python tools/bench_dimer.py [--reps 3] [--steps 30] [--dimers 4,32,96] [--painn-dimers 128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))   # (the restatements under tests/ import the oracle's spline helpers)

DIMER_CLASS = "dimer_advance"


def _timed(eng, fn, reps):
    """Best wall time of ``fn()`` over ``reps`` runs after one warm-up, and the profile of one more run."""
    out, best = None, np.inf
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if rep:
            best = min(best, time.perf_counter() - t0)
    eng.profile_enable(True)
    eng.profile_reset()
    fn()
    prof = eng.profile_read()
    eng.profile_enable(False)
    return out, best, prof


def _split(prof):
    ms = {k: v["total_ms"] for k, v in prof.items()}
    n = {k: v["launches"] for k, v in prof.items()}
    return sum(v for k, v in ms.items() if k != DIMER_CLASS), ms.get(DIMER_CLASS, 0.0), n.get(DIMER_CLASS, 0)


def measure(tag, eng, structs, held, steps, reps, want, converge):
    B = len(structs)
    G = B // 2
    kw = dict(max_steps=steps, max_rot_first=3, max_rot=1, delta=0.01, fmax=1e-6, seed=0, want=want)

    def dimer():
        eng.upload(structs)
        return eng.dimer(fixed=held, **kw)

    def fire():
        eng.upload(structs)
        return eng.relax_fire(fixed=held, max_steps=steps, fmax=1e-6, want=want)

    out, t_dim, prof = _timed(eng, dimer, reps)
    ev_ms, adv_ms, launches = _split(prof)
    evals, chain_evals = (int(v) for v in eng.last_relax_counts)
    _, t_fire, prof_f = _timed(eng, fire, reps)
    ev_f = _split(prof_f)[0]
    evals_f = int(eng.last_relax_counts[0])
    rec = {"bench": tag, "dimers": G, "chains": B, "atoms": int(sum(len(s[0]) for s in structs)), "steps": steps, "reps": reps,
           "lockstep_evaluations": evals, "dimer_wall_us_per_evaluation": round(1e6 * t_dim / evals, 2),
           "evaluation_us": round(1e3 * ev_ms / evals, 2), "dimer_advance_us_per_launch": round(1e3 * adv_ms / max(launches, 1), 2),
           "dimer_wall_minus_evaluation_us": round(1e6 * t_dim / evals - 1e3 * ev_ms / evals, 2),
           "fire_wall_us_per_step": round(1e6 * t_fire / evals_f, 2),
           "fire_wall_minus_evaluation_us": round(1e6 * t_fire / evals_f - 1e3 * ev_f / evals_f, 2),
           "rotations": int(out["n_rot"].sum()), "idle_midpoint_share_of_chain_evaluations": round(float(out["n_rot"].sum()) / chain_evals, 4),
           "stop_reasons": sorted(set(int(r) for r in out["stop_reason"]))}
    if converge:
        kw2 = dict(kw, fmax=0.01, max_steps=400, max_rot_first=8)
        best, conv, r = np.inf, 0, None
        for rep in range(2):
            t0 = time.perf_counter()
            eng.upload(structs)
            r = eng.dimer(fixed=held, **kw2)
            best = min(best, time.perf_counter() - t0)
            conv = int((r["stop_reason"] == 1).sum())
        evals2, chain2 = (int(v) for v in eng.last_relax_counts)
        rec.update({"converged_searches": conv, "steps_to_converge_max": int(r["n_steps"].max()), "lockstep_evaluations_to_converge": evals2,
                    "searches_converged_per_second": round(conv / best, 2),
                    "idle_midpoint_share_to_converge": round(float(r["n_rot"].sum()) / chain2, 4),
                    "saddle_energy_spread_eV": float(np.ptp(r["e0"][r["stop_reason"] == 1])) if conv else None})
    print(json.dumps(rec), flush=True)


def bench_eam(dimers, steps, reps):
    import cg_resident_cases as rc
    import eam_alloy_oracle as ao
    from surface_sampling_amd import backend

    pos, cell, pbc = ao.cu100_slab(4, 4, 6)
    assert len(pos) == 192
    top = pos[:, 2].max()
    a = 3.615
    ad = np.array([1.0 * a, 1.0 * a, top + 0.45 * a])      # a Cu adatom over a fourfold hollow
    T = np.zeros(193, np.int32)
    x0 = np.vstack([pos, ad])
    held1 = (x0[:, 2] < 0.5).astype(np.uint8)
    eng = backend.EAMEngine(rc.eam_tables("eam_alloy"), device=0)
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    eng.upload([(T, x0, cell, pbc)])
    x = eng.relax_fire(fixed=held1, max_steps=300, fmax=1e-3, want=want)["positions"].reshape(193, 3).copy()
    x[192] += 0.4 * np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)      # towards the bridge to the next hollow
    s = (T, x, cell, pbc)
    for g in dimers:
        measure("dimer_eam_cu100_193", eng, [s] * (2 * g), np.tile(held1, 2 * g), steps, reps, want, True)
    eng.close()


def bench_painn(n_dimers, steps, reps):
    import bench
    from surface_sampling_amd import backend, structures

    blobs, S, _ = bench.load_golden()
    slabs = bench.build_chains(S, 0, n_dimers)
    structs, held = [], []
    for s in slabs:
        T, X, cell, pbc = structures.as_arrays(s)
        structs += [(T, X, cell, pbc)] * 2
        held += [(X[:, 2] < X[:, 2].min() + 1.0).astype(np.uint8)] * 2
    eng = backend.PainnEngine(blobs, device=0)
    measure("dimer_painn_bench_batch", eng, structs, np.concatenate(held), steps, reps, backend.WANT_ENERGY | backend.WANT_FORCES, False)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--dimers", default="4,32,96")
    ap.add_argument("--painn-dimers", type=int, default=128, help="0: skip the PaiNN part")
    a = ap.parse_args()
    bench_eam([int(c) for c in a.dimers.split(",") if c], a.steps, a.reps)
    if a.painn_dimers:
        bench_painn(a.painn_dimers, a.steps, a.reps)


if __name__ == "__main__":
    main()
