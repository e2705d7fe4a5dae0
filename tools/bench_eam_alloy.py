"""Secondary measurement (not the BASELINE metric): several-element EAM (eam/alloy) on one GPU, fp64.
  * single-point evaluations/s at B chains of a generated 4 x 4 x 6 Cu(100) slab (192 atoms, rattled) with ~30 % random Au
    substitution, the Cu/Au setfl built from the shipped Cu_u3 / Au_u3 funcfl files: the resident batch re-evaluated (neighbor list
    + typed density / force / energy kernels; vssr_batch_run + synchronize) and the whole call with upload and fp64 download;
  * A/B: pure Cu through the typed kernels (a one-element setfl converted from Cu_u3) against the funcfl kernels, same slabs;
  * batched semigrand MC proposals/s (mc.ChainEnsemble + EAMSurfCalc, Cu / Au adatoms on the 16 sites of the Cu(100) fixture,
    static energies);
  * with --cg-driver lockstep | resident | both: the same MC on the Cu(100) toy with every proposal CG-relaxed (the fixture's first
    four atoms held), and CG relaxations/s of the 192-atom Cu/Au slabs (the device part of a relaxing proposal), each with the
    chain-evaluations dispatched and needed; both: the two drivers one after the other in this process.
Prints one JSON line per measurement.  For the kernel table: rocprofv3 --kernel-trace --stats -d <dir> -- python
tools/bench_eam_alloy.py --quick
Usage: python tools/bench_eam_alloy.py [--chains 1024,4096,16384] [--mc-chains 1024,4096] [--reps 20] [--mc-steps 5]
       [--cg-driver lockstep|resident|both] [--cg-only] [--relax-steps 20]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def potentials():
    import eam_alloy_oracle as ao
    from surface_sampling_amd import eam

    cu, au = eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))
    return cu, eam.tables_from_setfl(ao.cuau_setfl(cu, au), ["Cu", "Au"]), eam.tables_from_setfl(eam.funcfl_to_setfl(cu), ["Cu"])


def batch(B, frac):
    import eam_alloy_oracle as ao

    X, Cl, pbc = ao.cu100_slab(4, 4, 6)
    n = len(X)
    rng = np.random.default_rng(0)
    pos = np.concatenate([X + rng.normal(0, 0.05, X.shape) for _ in range(B)])
    T = np.concatenate([ao.random_alloy(X, frac, b) for b in range(B)]).astype(np.int32)
    return np.full(B, n, np.int32), T, pos, np.tile(Cl.reshape(1, 9), (B, 1)), np.tile(pbc.reshape(1, 3), (B, 1)), n


def time_engine(eng, arrays, reps):
    from surface_sampling_amd import backend

    n_atoms, T, pos, cell, pb = arrays
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
    return (time.perf_counter() - t0) / reps, dt_call


def single_point(B, reps, pots):
    from surface_sampling_amd import backend

    cu, cuau, cu1 = pots
    n_atoms, T, pos, cell, pb, n = batch(B, 0.3)
    eng = backend.EAMEngine(cuau, device=0)
    dt_run, dt_call = time_engine(eng, (n_atoms, T, pos, cell, pb), reps)
    eng.close()
    print(json.dumps({"metric": "EAM eam/alloy single-point evaluations/s, Cu(100) 4x4x6 slab (192 atoms, ~30 % Au, rattled)",
                      "chains": B, "evals_per_s_resident": round(B / dt_run, 1), "ms_per_batch_resident": round(1e3 * dt_run, 3),
                      "evals_per_s_call": round(B / dt_call, 1), "ms_per_batch_call": round(1e3 * dt_call, 3), "reps": reps}),
          flush=True)
    # A/B: pure Cu, typed kernels (one-element setfl) vs funcfl kernels, alternated
    zeros = np.zeros_like(T)
    res = {"typed": [], "funcfl": []}
    engs = {"typed": backend.EAMEngine(cu1, device=0), "funcfl": backend.EAMEngine(cu, device=0)}
    for _ in range(3):
        for k, e in engs.items():
            res[k].append(time_engine(e, (n_atoms, zeros, pos, cell, pb), reps)[0])
    for e in engs.values():
        e.close()
    t, f = float(np.median(res["typed"])), float(np.median(res["funcfl"]))
    print(json.dumps({"metric": "EAM A/B pure Cu: typed kernels (one-element setfl) vs funcfl kernels, resident batch, 192-atom slabs",
                      "chains": B, "ms_typed": round(1e3 * t, 3), "ms_funcfl": round(1e3 * f, 3), "typed_over_funcfl": round(t / f, 3),
                      "runs_ms_typed": [round(1e3 * x, 3) for x in res["typed"]],
                      "runs_ms_funcfl": [round(1e3 * x, 3) for x in res["funcfl"]], "reps": reps}), flush=True)


def mc_static(B, steps, path):
    from surface_sampling_amd import mc, structures
    from surface_sampling_amd.calculators import EAMSurfCalc

    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    base = structures.Structure(d["numbers"], d["positions"], d["cell"], d["pbc"])
    calc = EAMSurfCalc(files=[path], device="cuda:0")
    calc.set(pair_style="eam/alloy", pair_coeff=[f"* * {os.path.basename(path)} Cu Au"])
    ens = mc.ChainEnsemble(base, d["ads_coords"], ("Cu", "Au"), B, calc, seed=1, relax=False, temperature=0.5)
    ens.initialize()
    ens.step_semigrand()                                           # warm-up
    t0 = time.perf_counter()
    for _ in range(steps):
        ens.step_semigrand()
    dt = time.perf_counter() - t0
    print(json.dumps({"metric": "EAM eam/alloy batched semigrand MC proposals/s, Cu(100) 2x2 slab + Cu / Au adatoms on 16 sites, "
                                "static energies", "chains": B, "proposals_per_s": round(B * steps / dt, 1),
                      "s_per_step": round(dt / steps, 4), "steps": steps, "mean_adatoms": float(ens.num_adsorbates().mean())}),
          flush=True)


def mc_cg(B, steps, path, relax_steps, driver):
    import bench_si
    from surface_sampling_amd import mc, structures
    from surface_sampling_amd.calculators import EAMSurfCalc

    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    base = structures.Structure(d["numbers"], d["positions"], d["cell"], d["pbc"])
    calc = EAMSurfCalc(files=[path], device="cuda:0")
    calc.set(pair_style="eam/alloy", pair_coeff=[f"* * {os.path.basename(path)} Cu Au"], relax_steps=relax_steps, cg_driver=driver)
    ens = mc.ChainEnsemble(base, d["ads_coords"], ("Cu", "Au"), B, calc, seed=1, relax=True, relax_steps=relax_steps,
                           fixed_indices=np.arange(4), temperature=0.5, optimizer="LAMMPS")
    count = bench_si.RelaxCounter(calc._get_engine())
    ens.initialize()
    ens.step_semigrand()                                           # warm-up
    count.reset()
    t0 = time.perf_counter()
    for _ in range(steps):
        ens.step_semigrand()
    dt = time.perf_counter() - t0
    print(json.dumps({"metric": "EAM eam/alloy batched semigrand MC proposals/s, Cu(100) 2x2 slab + Cu / Au adatoms on 16 sites, every "
                                "proposal CG-relaxed (<= %d iterations)" % relax_steps, "chains": B, "cg_driver": driver,
                      "proposals_per_s": round(B * steps / dt, 1), "s_per_step": round(dt / steps, 4), "steps": steps,
                      "mean_adatoms": float(ens.num_adsorbates().mean()), **count.report()}), flush=True)
    calc._get_engine().close()


def relax_cg_slab(B, pots, relax_steps, driver, eng):
    import bench_pair
    import eam_alloy_oracle as ao

    X, Cl, pbc = ao.cu100_slab(4, 4, 6)
    bench_pair.relax_cg("Cu(100) 4x4x6 slab, eam/alloy, ~30 % Au", eng, (ao.random_alloy(X, 0.3, 0).astype(np.int32), X, Cl, pbc), B,
                        relax_steps, driver)


def main():
    import tempfile

    import eam_alloy_oracle as ao
    from surface_sampling_amd import eam

    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="1024,4096,16384")
    ap.add_argument("--mc-chains", default="1024,4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mc-steps", type=int, default=5)
    ap.add_argument("--cg-driver", choices=("none", "auto", "lockstep", "resident", "both"), default="none",
                    help="also measure the MC with a CG relaxation per proposal and CG relaxations of the 192-atom slabs")
    ap.add_argument("--cg-only", action="store_true", help="skip the single-point and static-MC figures")
    ap.add_argument("--relax-steps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="one size of each (for the rocprofv3 kernel table)")
    args = ap.parse_args()
    pots = potentials()
    chains = [4096] if args.quick else [int(x) for x in args.chains.split(",") if x]
    mc_chains = [1024] if args.quick else [int(x) for x in args.mc_chains.split(",") if x]
    for B in [] if args.cg_only else chains:
        single_point(B, 5 if args.quick else args.reps, pots)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "CuAu.eam.alloy")
        eam.write_setfl(ao.cuau_setfl(pots[0], eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))), path)
        for B in [] if args.cg_only else mc_chains:
            mc_static(B, 1 if args.quick else args.mc_steps, path)
        if args.cg_driver != "none":
            import bench_si
            from surface_sampling_amd import backend

            for B in mc_chains:
                for driver in bench_si.drivers_of(args.cg_driver):
                    mc_cg(B, 1 if args.quick else args.mc_steps, path, args.relax_steps, driver)
            eng = backend.EAMEngine(pots[1], device=0)
            for B in chains:
                for driver in bench_si.drivers_of(args.cg_driver):
                    relax_cg_slab(B, pots, args.relax_steps, driver, eng)
            eng.close()


if __name__ == "__main__":
    main()
