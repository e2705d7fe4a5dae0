#!/usr/bin/env python3
"""Device nudged elastic band: microseconds per NEB step, split into evaluation / project / step (``vssr_profile_read``), against what a
lock-step FIRE relaxation of the same batch costs per step, and bands converged per second (one JSON line per measurement).

The batch shapes are those of tools/bench_vib.py:
  (a) the 192-atom Cu(100) slab (EAM alloy tables) with a Cu adatom as 1 / 8 / 24 bands of 8 images (the adatom hops from one
      fourfold hollow to the next; both end images are relaxed first);
  (b) 256 PaiNN chains: 64 structures of the bench batch (bench.py's chains) as bands of 4 images (the topmost atom moved 0.6 A).

    python tools/bench_neb.py [--reps 3] [--steps 30] [--bands 1,8,24] [--painn-bands 64]
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

NEB_CLASSES = ("neb_project", "neb_step")


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
    return sum(v for k, v in ms.items() if k not in NEB_CLASSES), ms.get("neb_project", 0.0), ms.get("neb_step", 0.0), n.get("neb_step", 0)


def measure(tag, eng, structs, n_img, held, steps, reps, want, extra):
    G, B = len(n_img), len(structs)
    kw = dict(k=0.1, climb=True, method="improvedtangent", fmax=1e-6, max_steps=steps, want=want)

    def neb():
        eng.upload(structs)
        return eng.neb(n_img, fixed=held, **kw)

    def fire():
        eng.upload(structs)
        return eng.relax_fire(fixed=held, max_steps=steps, fmax=1e-6, want=want)

    out, t_neb, prof = _timed(eng, neb, reps)
    ev_ms, proj_ms, step_ms, launches = _split(prof)
    evals = int(eng.last_relax_counts[0])
    _, t_fire, prof_f = _timed(eng, fire, reps)
    ev_f = _split(prof_f)[0]
    evals_f = int(eng.last_relax_counts[0])
    per = lambda ms, n: round(1e3 * ms / max(n, 1), 2)
    neb_over = per(proj_ms + step_ms, launches)
    fire_over = round(1e6 * t_fire / evals_f - 1e3 * ev_f / evals_f, 2)      # wall per step minus its evaluation (FIRE has no class of its own)
    rec = {"bench": tag, "bands": G, "chains": B, "atoms": int(sum(len(s[0]) for s in structs)), "steps": steps, "reps": reps,
           "neb_lockstep_evaluations": evals, "neb_wall_us_per_step": round(1e6 * t_neb / evals, 2),
           "evaluation_us_per_step": per(ev_ms, launches), "project_us_per_step": per(proj_ms, launches), "step_us_per_step": per(step_ms, launches),
           "neb_launches_us_per_step": neb_over, "neb_wall_minus_evaluation_us_per_step": round(1e6 * t_neb / evals - 1e3 * ev_ms / max(launches, 1), 2),
           "fire_wall_us_per_step": round(1e6 * t_fire / evals_f, 2), "fire_wall_minus_evaluation_us_per_step": fire_over,
           "stop_reasons": sorted(set(int(r) for r in out["stop_reason"]))}
    # bands converged per second: the same bands to fmax 0.05 eV / A
    kw2 = dict(kw, fmax=0.05, max_steps=400)
    best, conv = np.inf, 0
    for rep in range(2):
        t0 = time.perf_counter()
        eng.upload(structs)
        r = eng.neb(n_img, fixed=held, **kw2)
        best = min(best, time.perf_counter() - t0)
        conv = int((r["stop_reason"] == 1).sum())
    rec.update({"converged_bands": conv, "steps_to_converge_max": int(r["n_steps"].max()), "bands_converged_per_second": round(conv / best, 2)})
    rec.update(extra(r))
    print(json.dumps(rec), flush=True)


def bench_eam(bands, steps, reps):
    import cg_resident_cases as rc
    import eam_alloy_oracle as ao
    from surface_sampling_amd import backend

    pos, cell, pbc = ao.cu100_slab(4, 4, 6)
    assert len(pos) == 192
    top = pos[:, 2].max()
    a = 3.615
    ad = np.array([1.0 * a, 1.0 * a, top + 0.45 * a])      # (the top layer of six holds atoms at (i + 1/2, j) a and (i, j + 1/2) a)
    T = np.zeros(193, np.int32)                            # a Cu adatom over a fourfold hollow, hopping to the next one
    x0 = np.vstack([pos, ad])
    d = np.zeros_like(x0)
    d[192] = [0.5 * a, 0.5 * a, 0.0]
    held1 = (x0[:, 2] < 0.5).astype(np.uint8)
    eng = backend.EAMEngine(rc.eam_tables("eam_alloy"), device=0)
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    eng.upload([(T, x0, cell, pbc), (T, x0 + d, cell, pbc)])
    ends = eng.relax_fire(fixed=np.tile(held1, 2), max_steps=300, fmax=1e-3, want=want)["positions"].reshape(2, 193, 3)
    band = [(T, ends[0] + (ends[1] - ends[0]) * (i / 7), cell, pbc) for i in range(8)]
    for g in bands:
        measure("neb_eam_cu100_193", eng, band * g, [8] * g, np.tile(held1, 8 * g), steps, reps, want,
                lambda r: {"barrier_forward_eV": float(r["barrier_forward"][0]), "barrier_reverse_eV": float(r["barrier_reverse"][0])})
    eng.close()


def bench_painn(n_bands, steps, reps):
    import bench
    from surface_sampling_amd import backend, structures

    blobs, S, _ = bench.load_golden()
    slabs = bench.build_chains(S, 0, n_bands)
    structs, held = [], []
    for s in slabs:
        T, X, cell, pbc = structures.as_arrays(s)
        d = np.zeros_like(X)
        d[int(np.argmax(X[:, 2]))] = [0.5, 0.3, 0.1]
        structs += [(T, X + d * (i / 3), cell, pbc) for i in range(4)]
        held += [(X[:, 2] < X[:, 2].min() + 1.0).astype(np.uint8)] * 4
    eng = backend.PainnEngine(blobs, device=0)
    measure("neb_painn_bench_batch", eng, structs, [4] * n_bands, np.concatenate(held), steps, reps, backend.WANT_ENERGY | backend.WANT_FORCES,
            lambda r: {})
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--bands", default="1,8,24")
    ap.add_argument("--painn-bands", type=int, default=64, help="0: skip the PaiNN part")
    a = ap.parse_args()
    bench_eam([int(c) for c in a.bands.split(",") if c], a.steps, a.reps)
    if a.painn_bands:
        bench_painn(a.painn_bands, a.steps, a.reps)


if __name__ == "__main__":
    main()
