"""Secondary measurement (not the BASELINE metric): the Vashishta potential (pair_style vashishta) on one GPU, fp64, with a pair
potential of the same cutoff as the yardstick for the cost of the row walk.
  * single-point evaluations/s at B chains of a generated SiC(001) slab (3 x 3 cells in plane, 12 atomic planes: 216 atoms, rattled,
    periodic in x and y) through the Vashishta handle with the built-in SiC set (rc = 7.35 A: 128 slots per row on this slab; r0 = 2.9 A:
    about 4 short slots) and through a pair handle with a ``born`` term on every type pair at the same 7.35 A cutoff, alternated: the
    resident batch re-evaluated (neighbor list + site / gather / energy kernels; vssr_batch_run + synchronize) and the whole call
    with upload and fp64 download;
  * with --stress: the same with vssr_batch_stress after every evaluation (the gradient launch of the site kernel + the virial
    kernel).
Prints one JSON line per measurement.  For the per-launch times of k_vashishta_site<false>, k_vashishta_gather, k_vashishta_site<true>
and k_slot_stress: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_vashishta.py --quick --stress
Usage: python tools/bench_vashishta.py [--chains 1024,4096] [--reps 20] [--rounds 3] [--stress]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

RC = 7.35


def batch(B, seed=0):
    """B rattled copies of the 216-atom slab as the ABI's packed arrays: (n_atoms, types, pos, cell, pbc, atoms per chain)."""
    import vashishta_oracle as vo

    Z, X, Cl, pbc, _ = vo.sic001_slab(nx=3, ny=3, layers=6)
    n = len(Z)
    rng = np.random.default_rng(seed)
    T = np.tile(np.where(Z == 6, 0, 1).astype(np.int32), B)
    pos = np.tile(X, (B, 1)) + rng.normal(0.0, 0.05, (B * n, 3))
    return np.full(B, n, np.int32), T, pos, np.tile(Cl.reshape(1, 9), (B, 1)), np.tile(pbc, (B, 1)).astype(np.uint8), n


def engines():
    import vashishta_oracle as vo
    from surface_sampling_amd import backend

    born = [(a, b, "born", [900.0 + 100.0 * (a + b), 0.3, 1.6, 12.0, 4.0], RC, 1) for a in range(2) for b in range(a, 2)]
    return {"vashishta": backend.VashishtaEngine(vo.sic_params()[1], device=0),
            "born": backend.PairEngine(born, n_types=2, device=0)}


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

    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="1024,4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two handles; the medians are reported")
    ap.add_argument("--stress", action="store_true")
    ap.add_argument("--quick", action="store_true", help="1 024 chains, one round of five repetitions (for the rocprofv3 kernel table)")
    args = ap.parse_args()
    reps, rounds = (5, 1) if args.quick else (args.reps, args.rounds)
    chains = [1024] if args.quick else [int(x) for x in args.chains.split(",") if x]
    for B in chains:
        n_atoms, T, pos, cell, pb, n = batch(B)
        arrays = (n_atoms, T, pos, cell, pb)
        engs = engines()
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
        stats = engs["vashishta"].stats()   # atoms, neighbor edges and padded slots of the resident batch
        for e in engs.values():
            e.close()
        med = lambda v: float(np.median(v))   # noqa: E731
        out = {"metric": "Vashishta SiC against a born pair potential at the same 7.35 A cutoff, single-point evaluations/s, "
                         "SiC(001) 3x3 slab (216 atoms, rattled)",
               "chains": B, "atoms_per_chain": n, "reps": reps, "rounds": rounds}
        out["slots_per_atom"] = round(stats["slots"] / stats["atoms"], 1)
        for k in engs:
            out[f"evals_per_s_resident_{k}"] = round(B / med(run[k]), 1)
            out[f"ms_per_batch_resident_{k}"] = round(1e3 * med(run[k]), 3)
            out[f"evals_per_s_call_{k}"] = round(B / med(call[k]), 1)
            out[f"runs_ms_resident_{k}"] = [round(1e3 * x, 3) for x in run[k]]
            if args.stress:
                out[f"ms_per_batch_with_stress_{k}"] = round(1e3 * med(vir[k]), 3)
        out["vashishta_over_born_resident"] = round(med(run["vashishta"]) / med(run["born"]), 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
