#!/usr/bin/env python3
"""Device constant-pressure MD against the fixed-cell lock-step MD it extends, chain-steps per second (one JSON line per batch).

On the same resident batch, in one process, in alternating order: ``backend.md`` (lock-step Langevin: the reference rate),
``backend.npt`` thermostat-only (Berendsen, no stress kernel) and ``backend.npt`` with the Berendsen barostat under Langevin.  Next to
the ratios the time of one ``stress()`` call on the evaluated batch (the stress kernels plus the copy-out of 12 B doubles: an upper
bound of the kernels' share), which is the cost a barostat cannot avoid.

  * the 48-atom GaN Tersoff chains of tools/bench_md.py at 256 and 4 096 chains;
  * the PaiNN bench batch (bench.py's chains).

Every timed window covers whole calls (they end in a synchronise and the copy-out of positions, cells and thermo records).

    python tools/bench_npt.py [--chains 256,4096] [--steps 200] [--reps 3] [--painn-chains 256] [--painn-steps 20]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

BARO = dict(barostat="berendsen", pressure=0.0, compressibility=0.005, taup=1000.0, mask=(1, 1, 0))


def measure(eng, name, packs, mass, fixed, steps, dt, reps, want):
    B = len(packs)
    common = dict(temperature=300.0, seed=1, fixed=fixed, thermo_interval=steps, want=want)
    runs = {
        "md_langevin": lambda: eng.md(mass, steps, dt, thermostat="langevin", friction=0.01, driver="lockstep", **common),
        "npt_berendsen_thermostat": lambda: eng.npt(mass, steps, dt, thermostat="berendsen", taut=100.0, **common),
        "npt_langevin_berendsen_barostat": lambda: eng.npt(mass, steps, dt, thermostat="langevin", friction=0.01, **BARO, **common),
    }
    best = {k: 0.0 for k in runs}
    for rep in range(reps + 1):          # rep 0 warms every path up (buffers, pools)
        order = list(runs) if rep % 2 == 0 else list(runs)[::-1]
        for k in order:
            eng.upload(packs)
            eng.draw_velocities(mass, 300.0, seed=1, fixed=fixed)
            t0 = time.perf_counter()
            out = runs[k]()
            el = time.perf_counter() - t0
            assert (out["stop_reason"] == 1).all(), (k, np.unique(out["stop_reason"]))
            if rep:
                best[k] = max(best[k], B * steps / el)
    # one stress() on the evaluated batch, best of a few
    eng.upload(packs)
    eng.run(want)
    eng.synchronize()
    eng.stress()
    t_stress = min(_timed(eng.stress) for _ in range(5))
    t_eval = min(_timed(lambda: (eng.run(want), eng.synchronize())) for _ in range(5))
    print(json.dumps({"bench": name, "chains": B, "atoms": int(len(mass)), "steps": steps, "reps": reps,
                      **{k + "_chain_steps_per_s": round(v, 1) for k, v in best.items()},
                      "thermostat_only_over_md": round(best["npt_berendsen_thermostat"] / best["md_langevin"], 3),
                      "barostat_over_md": round(best["npt_langevin_berendsen_barostat"] / best["md_langevin"], 3),
                      "stress_call_ms": round(1e3 * t_stress, 3), "evaluation_ms": round(1e3 * t_eval, 3)}), flush=True)


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def bench_gan(chains, steps, reps):
    import bench_md
    from surface_sampling_amd import backend

    for B in chains:
        golden, structs, mask, mass = bench_md.gan_chains(B)
        eng = backend.TersoffEngine(golden.tersoff_params, device=0)
        measure(eng, "npt_gan48", structs, mass, mask, steps, 1.0, reps, backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM)
        eng.close()


def bench_painn(n_chains, steps, reps):
    import bench
    from surface_sampling_amd import backend, structures

    blobs, S, _ = bench.load_golden()
    slabs = bench.build_chains(S, 0, n_chains)
    packs = [structures.as_arrays(s) for s in slabs]
    mass = np.concatenate([structures.masses_of(s) for s in slabs])
    fixed = np.concatenate([(s.positions[:, 2] < s.positions[:, 2].max() - 4.0) for s in slabs]).astype(np.uint8)
    eng = backend.PainnEngine(blobs, device=0)
    measure(eng, "npt_painn", packs, mass, fixed, steps, 0.5, reps, backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_STD)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="256,4096")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--painn-chains", type=int, default=256, help="0: skip the PaiNN part")
    ap.add_argument("--painn-steps", type=int, default=20)
    a = ap.parse_args()
    bench_gan([int(c) for c in a.chains.split(",") if c], a.steps, a.reps)
    if a.painn_chains:
        bench_painn(a.painn_chains, a.painn_steps, a.reps)


if __name__ == "__main__":
    main()
