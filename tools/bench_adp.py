"""Secondary measurement (not the BASELINE metric): the angular-dependent potential (pair_style adp) on one GPU, fp64, against the
eam/alloy handle of the same tables.
  * single-point evaluations/s at B chains of a generated 4 x 4 x 6 Cu(100) slab (192 atoms, rattled) with ~30 % random Au
    substitution -- the slabs of tools/bench_eam_alloy.py -- through the ADP handle (the Cu/Au setfl built from the shipped Cu_u3 /
    Au_u3 funcfl files plus the synthetic u, w of tests/adp_oracle.py) and through the eam/alloy handle of the same F, rho and
    r phi tables, alternated: the resident batch re-evaluated (neighbor list + density / force / energy kernels; vssr_batch_run +
    synchronize) and the whole call with upload and fp64 download;
  * with --stress: the same with vssr_batch_stress after every evaluation.
Prints one JSON line per measurement.  For the kernel table: rocprofv3 --kernel-trace --stats -d <dir> -- python
tools/bench_adp.py --quick
Usage: python tools/bench_adp.py [--chains 1024] [--reps 20] [--rounds 3] [--stress]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def potentials():
    import adp_oracle
    from surface_sampling_amd import eam

    cu, au = eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))
    s = adp_oracle.cuau_adp(cu, au)
    return {"adp": eam.tables_from_adp(s, ["Cu", "Au"]), "eam/alloy": eam.tables_from_setfl(s, ["Cu", "Au"])}


def time_stress(eng, arrays, reps):
    from surface_sampling_amd import backend

    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    eng.upload_arrays(*arrays)
    for _ in range(2):
        eng.run(want)
        eng.stress()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.run(want)
        eng.stress()
    return (time.perf_counter() - t0) / reps


def main():
    import bench_eam_alloy
    from surface_sampling_amd import backend

    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two handles; the medians are reported")
    ap.add_argument("--stress", action="store_true")
    ap.add_argument("--quick", action="store_true", help="one round of five repetitions (for the rocprofv3 kernel table)")
    args = ap.parse_args()
    reps, rounds = (5, 1) if args.quick else (args.reps, args.rounds)
    pots = potentials()
    for B in [int(x) for x in args.chains.split(",") if x]:
        n_atoms, T, pos, cell, pb, n = bench_eam_alloy.batch(B, 0.3)
        arrays = (n_atoms, T, pos, cell, pb)
        engs = {k: backend.EAMEngine(t, device=0) for k, t in pots.items()}
        run = {k: [] for k in engs}
        call = {k: [] for k in engs}
        vir = {k: [] for k in engs}
        for _ in range(rounds):
            for k, e in engs.items():
                r, c = bench_eam_alloy.time_engine(e, arrays, reps)
                run[k].append(r)
                call[k].append(c)
                if args.stress:
                    vir[k].append(time_stress(e, arrays, reps))
        for e in engs.values():
            e.close()
        med = lambda v: float(np.median(v))   # noqa: E731
        out = {"metric": "ADP against eam/alloy single-point evaluations/s, Cu(100) 4x4x6 slab (192 atoms, ~30 % Au, rattled)",
               "chains": B, "atoms_per_chain": n, "reps": reps, "rounds": rounds}
        for k in engs:
            tag = k.replace("/", "_")
            out[f"evals_per_s_resident_{tag}"] = round(B / med(run[k]), 1)
            out[f"ms_per_batch_resident_{tag}"] = round(1e3 * med(run[k]), 3)
            out[f"evals_per_s_call_{tag}"] = round(B / med(call[k]), 1)
            out[f"runs_ms_resident_{tag}"] = [round(1e3 * x, 3) for x in run[k]]
            if args.stress:
                out[f"ms_per_batch_with_stress_{tag}"] = round(1e3 * med(vir[k]), 3)
        out["adp_over_eam_alloy_resident"] = round(med(run["adp"]) / med(run["eam/alloy"]), 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
