"""Secondary measurement (not the BASELINE metric): Stillinger-Weber on the reference's Si(111) 5x5 slab (100 atoms, the first 75
held as the bulk group, the top 25 free; tests/golden/si111_5x5.npz), fp64 on one GPU.
  * single-point evaluations/s at B chains (every chain the slab with its top 25 atoms rattled by its own seed): the resident batch
    re-evaluated (neighbor list + SW site / gather / energy kernels; vssr_batch_run + synchronize) and the whole call with upload
    and fp64 download (SWEngine.evaluate_arrays_f64);
  * batched semigrand MC proposals/s (mc.ChainEnsemble + SWSurfCalc, Si adatoms on a 4 x 4 site grid), every proposal relaxed
    with the LAMMPS-style CG minimiser before the Metropolis test; --cg-driver lockstep | resident | both selects its driver
    (both: the two drivers one after the other in this process, the A/B of profiles/r15/NOTES_chain_resident_kinds.md), with the
    chain-evaluations the relaxations dispatched and needed (vssr_batch_relax_counts, sum of n_eval + 1 per chain).
Prints one JSON line per measurement.  For the kernel table: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_si.py --quick
Usage: python tools/bench_si.py [--chains 256,1024,4096] [--mc-chains 256,1024] [--reps 20] [--mc-steps 3] [--relax-steps 50]
       [--cg-driver auto|lockstep|resident|both] [--no-single-point]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODEL = "SW_StillingerWeber_1985_Si__MO_405512056662_005"


def slab():
    d = np.load(os.path.join(ROOT, "tests", "golden", "si111_5x5.npz"))
    return d["numbers"], d["positions"], d["cell"], d["pbc"], d["fixed"]


def single_point(B, reps):
    from surface_sampling_amd import backend, sw as sw_io

    Z, X, Cl, pbc, fixed = slab()
    n = len(Z)
    P = sw_io.parse_sw(sw_io.builtin_text(MODEL), ["Si"])
    eng = backend.SWEngine(P, device=0)
    rng = np.random.default_rng(0)
    pos = np.concatenate([X + np.where(fixed[:, None], 0.0, rng.normal(0, 0.05, X.shape)) for _ in range(B)])
    n_atoms = np.full(B, n, np.int32)
    T = np.zeros(B * n, np.int32)
    cell = np.tile(Cl.reshape(1, 9), (B, 1))
    pb = np.tile(pbc.astype(np.uint8).reshape(1, 3), (B, 1))
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    for _ in range(3):
        eng.evaluate_arrays_f64(n_atoms, T, pos, cell, pb)
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.evaluate_arrays_f64(n_atoms, T, pos, cell, pb)
    dt_call = (time.perf_counter() - t0) / reps
    eng.upload_arrays(n_atoms, T, pos, cell, pb)
    eng.run(want)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.run(want)
    eng.synchronize()
    dt_run = (time.perf_counter() - t0) / reps
    eng.close()
    print(json.dumps({"metric": "SW single-point evaluations/s, Si(111) 5x5 slab (100 atoms, top 25 rattled)", "chains": B,
                      "evals_per_s_resident": round(B / dt_run, 1), "ms_per_batch_resident": round(1e3 * dt_run, 3),
                      "evals_per_s_call": round(B / dt_call, 1), "ms_per_batch_call": round(1e3 * dt_call, 3), "reps": reps}), flush=True)


CG_DRIVERS = ("auto", "lockstep", "resident", "both")


def drivers_of(choice):
    return ("lockstep", "resident") if choice == "both" else (choice,)


class RelaxCounter:
    """Sums over the CG relaxations of an engine: launches, dispatched chain-evaluations (vssr_batch_relax_counts) and the
    chain-evaluations the chains needed (n_eval + the setup evaluation of every chain)."""

    def __init__(self, eng):
        self.eng, self.launches, self.dispatched, self.needed, self.calls = eng, 0, 0, 0, 0
        inner = eng.relax_cg_arrays_f64

        def counted(*a, **kw):
            out = inner(*a, **kw)
            ls, ce = eng.last_relax_counts
            self.launches += int(ls); self.dispatched += int(ce); self.needed += int(out[5].sum()) + len(out[5]); self.calls += 1
            return out

        eng.relax_cg_arrays_f64 = counted

    def reset(self):
        self.launches = self.dispatched = self.needed = self.calls = 0

    def report(self):
        return {"cg_driver_used": self.eng.last_cg_driver, "relaxations": self.calls, "launches": self.launches,
                "chain_evals_dispatched": self.dispatched, "chain_evals_needed": self.needed,
                "dispatched_over_needed": round(self.dispatched / max(1, self.needed), 3)}


def mc_cg(B, steps, relax_steps, driver="auto"):
    from surface_sampling_amd import mc, structures
    from surface_sampling_amd.calculators import SWSurfCalc

    Z, X, Cl, pbc, fixed = slab()
    base = structures.Structure(Z, X, Cl, pbc)
    ztop = X[:, 2].max()
    sites = np.array([(i + 0.3) / 4 * Cl[0] + (j + 0.6) / 4 * Cl[1] for i in range(4) for j in range(4)], float)
    sites[:, 2] = ztop + 1.6
    calc = SWSurfCalc(MODEL, device="cuda:0")
    calc.set(relax_steps=relax_steps, cg_driver=driver)
    ens = mc.ChainEnsemble(base, sites, ("Si",), B, calc, seed=1, relax=True, relax_steps=relax_steps,
                           fixed_indices=np.flatnonzero(fixed), temperature=0.5, optimizer="LAMMPS")
    count = RelaxCounter(calc._get_engine())
    ens.initialize()
    ens.step_semigrand()                                           # warm-up
    count.reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        ens.step_semigrand()
    dt = time.perf_counter() - t0
    ls, ce = calc._get_engine().last_relax_counts
    print(json.dumps({"metric": "SW batched semigrand MC proposals/s, Si(111) 5x5 + Si adatoms, every proposal CG-relaxed "
                                "(<= %d iterations)" % relax_steps, "chains": B, "cg_driver": driver,
                      "proposals_per_s": round(B * steps / dt, 1), "s_per_step": round(dt / steps, 4), "steps": steps,
                      "mean_adatoms": float(ens.num_adsorbates().mean()), "last_relax_lockstep_evals": int(ls),
                      "last_relax_chain_evals": int(ce), **count.report()}), flush=True)
    calc._get_engine().close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="256,1024,4096")
    ap.add_argument("--mc-chains", default="256,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mc-steps", type=int, default=3)
    ap.add_argument("--relax-steps", type=int, default=50)
    ap.add_argument("--cg-driver", choices=CG_DRIVERS, default="auto", help="driver of the CG relaxations (both: lock-step, then chain-resident)")
    ap.add_argument("--no-single-point", action="store_true", help="the MC measurement only")
    ap.add_argument("--quick", action="store_true", help="one size of each (for the rocprofv3 kernel table)")
    args = ap.parse_args()
    chains = [1024] if args.quick else [int(x) for x in args.chains.split(",") if x]
    mc_chains = [256] if args.quick else [int(x) for x in args.mc_chains.split(",") if x]
    for B in ([] if args.no_single_point else chains):
        single_point(B, 5 if args.quick else args.reps)
    for B in mc_chains:
        for driver in drivers_of(args.cg_driver):
            mc_cg(B, 1 if args.quick else args.mc_steps, args.relax_steps, driver)


if __name__ == "__main__":
    main()
