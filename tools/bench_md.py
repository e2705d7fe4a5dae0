#!/usr/bin/env python3
"""Device molecular dynamics, chain-steps per second (one JSON line per measurement).

  * Langevin MD of the 48-atom GaN Tersoff chains (36-atom slab + 12 adatoms, CG-relaxed first, bulk held) at 256 / 1 024 / 4 096 / 16 384 chains: the
    lock-step driver against the chain-resident one, alternating in one run;
  * lock-step Langevin MD of the PaiNN bench batch (bench.py's chains) against the plain evaluation rate of the same batch, same run.

Every timed window covers whole ``backend.md`` calls (they end in a synchronise and the copy-out of positions and thermo records) or,
for the plain rate, ``run()`` calls closed by ``synchronize()``.

    python tools/bench_md.py [--chains 256,1024,4096,16384] [--steps 200] [--reps 3] [--painn-chains 256] [--painn-steps 20]
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


def gan_chains(n_chains):
    """n_chains 48-atom chains: 16 distinct slabs + adatoms (tests/cg_cases.py), CG-relaxed, repeated; (structs, held mask, masses)."""
    import cg_cases as cc
    from conftest import Golden

    from surface_sampling_amd import backend

    golden = Golden()
    cases = [cc._slab_with_adatoms(golden, 1, 12, 50 + k) for k in range(16)]
    # the adatoms are dropped at random: CG-relax the 16 chains once, so that the dynamics starts near a minimum
    base, base_mask = cc.pack(cases)
    eng = backend.TersoffEngine(golden.tersoff_params, device=0)
    relaxed = eng.relax_cg_f64(base, fixed=base_mask, max_iter=200)[3]
    eng.close()
    cases = [c._replace(pos=relaxed[48 * k:48 * (k + 1)]) for k, c in enumerate(cases)]
    structs, mask = cc.pack([cases[b % 16] for b in range(n_chains)])
    mass = np.concatenate([np.where(np.asarray(s[0]) == 0, 69.723, 14.007) for s in structs])
    return golden, structs, mask, mass


def bench_gan(chains, steps, reps):
    from surface_sampling_amd import backend

    for B in chains:
        golden, structs, mask, mass = gan_chains(B)
        eng = backend.TersoffEngine(golden.tersoff_params, device=0)
        kw = dict(thermostat="langevin", temperature=300.0, friction=0.01, seed=1, fixed=mask, thermo_interval=steps,
                  want=backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM)
        best = {"lockstep": 0.0, "resident": 0.0}
        ref = None
        for rep in range(reps + 1):          # rep 0 warms both drivers up (buffers, pools)
            for driver in ("lockstep", "resident"):
                eng.upload(structs)
                eng.draw_velocities(mass, 300.0, seed=1, fixed=mask)
                t0 = time.perf_counter()
                out = eng.md(mass, steps, 1.0, driver=driver, **kw)
                dt = time.perf_counter() - t0
                assert eng.last_md_driver == driver and (out["stop_reason"] == 1).all()
                if ref is None:
                    ref = out["positions"]
                assert np.array_equal(ref, out["positions"])      # the two drivers agree bit for bit
                if rep:
                    best[driver] = max(best[driver], B * steps / dt)
        n_free = 48 - mask.reshape(B, 48).sum(axis=1)
        T = 2 * out["ekin"][-1] / (3 * n_free * backend.KB_EV)
        print(json.dumps({"bench": "md_gan48_langevin", "chains": B, "atoms_per_chain": 48, "steps": steps, "reps": reps,
                          "lockstep_chain_steps_per_s": round(best["lockstep"], 1), "resident_chain_steps_per_s": round(best["resident"], 1),
                          "resident_over_lockstep": round(best["resident"] / best["lockstep"], 3),
                          "mean_kinetic_temperature_K": round(float(T.mean()), 1)}), flush=True)
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
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_STD
    md_rate = ev_rate = 0.0
    for rep in range(reps + 1):
        eng.upload(packs)
        eng.draw_velocities(mass, 300.0, seed=1, fixed=fixed)
        t0 = time.perf_counter()
        out = eng.md(mass, steps, 0.5, thermostat="langevin", temperature=300.0, friction=0.01, seed=1, fixed=fixed, thermo_interval=steps, want=want)
        dt = time.perf_counter() - t0
        assert (out["stop_reason"] == 1).all()
        eng.upload(packs)
        eng.run(want)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.run(want)
        eng.synchronize()
        de = time.perf_counter() - t0
        if rep:
            md_rate, ev_rate = max(md_rate, n_chains * steps / dt), max(ev_rate, n_chains * steps / de)
    print(json.dumps({"bench": "md_painn_langevin_lockstep", "chains": n_chains, "atoms": int(len(mass)), "steps": steps, "reps": reps,
                      "md_chain_steps_per_s": round(md_rate, 1), "plain_chain_evaluations_per_s": round(ev_rate, 1),
                      "md_over_plain": round(md_rate / ev_rate, 3)}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="256,1024,4096,16384")
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
