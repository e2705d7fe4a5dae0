"""Secondary measurement: cost of the lock-step relaxation driver against the number of chain-evaluations it needs.
256 bench chains (BASELINE configs[3] workload), lower slab layers held fixed; for several convergence thresholds:
wall time of vssr_batch_relax_{bfgs,fire}, sum over chains of (steps + 1) = evaluations an ideal driver performs, and the
time per chain-evaluation -- constant if converged chains cost nothing.  Prints one JSON line per run.
--cg-driver lockstep | resident | both measures the CG minimiser of the fp64 potentials instead (vssr_batch_relax_cg with that driver):
--chains rattled Si(111) 5x5 slabs on Stillinger-Weber, wall time and dispatched / needed chain-evaluations per driver.
--linesearch measures the device BFGSLineSearch (vssr_batch_relax_bfgs_linesearch) next to device BFGS per handle kind: the PaiNN bench
batch, and --chains rattled GaN (Tersoff), Si(111) (Stillinger-Weber), Cu(100) + Au (eam/alloy) and rocksalt (Born + dsf) slabs with
their lower half held: steps, evaluations per step, lock-step evaluations and wall time of both optimizers.
Usage: python tools/bench_relax.py [--chains 256] [--relax-steps 20] [--cg-driver lockstep|resident|both] [--linesearch]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (golden loaders)


def cg_main(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_pair
    import bench_si
    from surface_sampling_amd import backend, sw as sw_io

    Z, X, Cl, pbc, fixed = bench_si.slab()
    # (bench_pair.relax_cg holds the atoms below the middle height: the lower layers of the slab)
    eng = backend.SWEngine(sw_io.parse_sw(sw_io.builtin_text(bench_si.MODEL), ["Si"]), device=0)
    for driver in bench_si.drivers_of(args.cg_driver):
        bench_pair.relax_cg("Si(111) 5x5 slab, Stillinger-Weber", eng, (np.zeros(len(Z), np.int32), X, Cl, pbc), args.chains,
                            args.relax_steps, driver, sigma=0.1)
    eng.close()


def _linesearch_pair(kind, name, eng, upload, mask, steps, fmax):
    """BFGS, then BFGSLineSearch, on the batch ``upload()`` makes resident: one warm-up and one timed call each."""
    rows = {}
    for opt in ("BFGS", "BFGSLineSearch"):
        fn = eng.relax_bfgs if opt == "BFGS" else eng.relax_bfgs_linesearch
        for timed in (False, True):
            upload()
            eng.synchronize()
            t0 = time.perf_counter()
            info = fn(fixed=mask, max_steps=steps, fmax=fmax)
            dt = time.perf_counter() - t0
        lockstep, dispatched = eng.relax_counts()
        n_eval = info["n_eval"] if "n_eval" in info else info["n_steps"] + 1
        rows[opt] = {"mean_steps": round(float(info["n_steps"].mean()), 2), "mean_n_eval": round(float(n_eval.mean()), 2),
                     "max_n_eval": int(n_eval.max()), "evaluations_per_step": round(float(n_eval.sum()) / max(1, int(info["n_steps"].sum())), 3),
                     "converged": int(info["converged"].sum()), "lockstep_evaluations": lockstep, "wall_s": round(dt, 4)}
        if "stop_reason" in info:
            rows[opt]["stop_reasons"] = {str(k): int((info["stop_reason"] == k).sum()) for k in np.unique(info["stop_reason"])}
    print(json.dumps({"metric": f"BFGSLineSearch next to BFGS, {name}", "kind": kind, "chains": int(eng._n_cfg), "relax_steps": steps,
                      "fmax": fmax, **{k: v for k, v in rows.items()},
                      "wall_ratio_linesearch_over_bfgs": round(rows["BFGSLineSearch"]["wall_s"] / rows["BFGS"]["wall_s"], 3)}), flush=True)


def linesearch_main(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench_eam_alloy
    import bench_pair
    import bench_si
    from surface_sampling_amd import backend, pair, sw as sw_io
    from surface_sampling_amd.calculators import stoich_offset_table

    B, steps, fmax = args.chains, args.relax_steps, 0.01
    blobs, S, offset_data = bench.load_golden()
    table, const = stoich_offset_table(offset_data)
    chains = bench.build_chains(S, 0, B)
    packs = [(s.numbers, s.positions, s.cell, s.pbc) for s in chains]
    mask = np.concatenate([(s.positions[:, 2] < s.positions[:240, 2].max() - 4.0).astype(np.uint8) for s in chains])
    eng = backend.PainnEngine(blobs, device=0, offset_per_z=table, offset_const=const)
    _linesearch_pair("painn", "PaiNN bench batch (SrTiO3 chains)", eng, lambda: eng.upload(packs), mask, steps, fmax)
    eng.close()

    def analytic(kind, name, eng, struct, sigma=0.05):
        T1, X, Cl, pbc = struct
        n = len(T1)
        rng = np.random.default_rng(0)
        held = X[:, 2] < 0.5 * (X[:, 2].min() + X[:, 2].max())
        pos = np.concatenate([X + np.where(held[:, None], 0.0, rng.normal(0, sigma, X.shape)) for _ in range(B)])
        arrays = (np.full(B, n, np.int32), np.tile(T1, B), pos, np.tile(np.asarray(Cl, float).reshape(1, 9), (B, 1)),
                  np.tile(np.asarray(pbc, np.uint8).reshape(1, 3), (B, 1)))
        _linesearch_pair(kind, f"{name} ({n} atoms, {int(held.sum())} held)", eng, lambda: eng.upload_arrays(*arrays),
                         np.tile(held.astype(np.uint8), B), steps, fmax)
        eng.close()

    with open(os.path.join(ROOT, "tests", "golden", "GaN_tersoff_params.json")) as fh:
        params = np.array(json.load(fh)["params_ijk"], dtype=np.float64)
    k = "GaN_3x3_pristine"
    gan = (np.array([0 if z == 31 else 1 for z in S[f"{k}.numbers"]], np.int32), S[f"{k}.positions"], S[f"{k}.cell"], S[f"{k}.pbc"])
    analytic("tersoff", "GaN(0001) 3x3 slab, Tersoff", backend.TersoffEngine(params, device=0), gan)
    Z, X, Cl, pbc, _ = bench_si.slab()
    analytic("sw", "Si(111) 5x5 slab, Stillinger-Weber", backend.SWEngine(sw_io.parse_sw(sw_io.builtin_text(bench_si.MODEL), ["Si"]), device=0),
             (np.zeros(len(Z), np.int32), X, Cl, pbc), sigma=0.1)
    import eam_alloy_oracle as ao
    _, alloy, _ = bench_eam_alloy.potentials()
    X, Cl, pbc = ao.cu100_slab(4, 4, 6)
    analytic("eam", "Cu(100) 4x4x6 slab, eam/alloy, ~30 % Au", backend.EAMEngine(alloy, device=0), (ao.random_alloy(X, 0.3, 0).astype(np.int32), X, Cl, pbc))
    analytic("pair", "rocksalt slab, Born + damped-shifted Coulomb", backend.PairEngine(pair.parse(bench_pair.BORN_DSF, 2), device=0),
             bench_pair.rocksalt_slab())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--linesearch", action="store_true", help="BFGSLineSearch next to BFGS on every handle kind")
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--relax-steps", type=int, default=20)
    ap.add_argument("--cg-driver", choices=("none", "auto", "lockstep", "resident", "both"), default="none")
    args = ap.parse_args()
    if args.linesearch:
        return linesearch_main(args)
    if args.cg_driver != "none":
        return cg_main(args)
    from surface_sampling_amd import backend
    from surface_sampling_amd.calculators import stoich_offset_table

    blobs, S, offset_data = bench.load_golden()
    table, const = stoich_offset_table(offset_data)
    chains = bench.build_chains(S, 0, args.chains)
    packs = [(s.numbers, s.positions, s.cell, s.pbc) for s in chains]
    mask = np.concatenate([(s.positions[:, 2] < s.positions[:240, 2].max() - 4.0).astype(np.uint8) for s in chains])
    eng = backend.PainnEngine(blobs, device=0, offset_per_z=table, offset_const=const)
    eng.upload(packs)
    eng.run(); eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        eng.run()
    eng.synchronize()
    t_eval = (time.perf_counter() - t0) / 5
    for opt in ("BFGS", "FIRE"):
        for fmax in (0.01, 0.3, 1.0, 3.0):
            eng.upload(packs)
            eng.synchronize()
            t0 = time.perf_counter()
            info = eng.relax(opt, fixed=mask, max_steps=args.relax_steps, fmax=fmax)
            dt = time.perf_counter() - t0
            need = int((info["n_steps"] + 1).sum())
            lockstep, dispatched = eng.relax_counts()
            print(json.dumps({"optimizer": opt, "fmax": fmax, "chains": args.chains, "relax_steps": args.relax_steps,
                              "converged": int(info["converged"].sum()), "mean_steps": float(info["n_steps"].mean()),
                              "chain_evaluations_needed": need, "lockstep_evaluations": lockstep,
                              "chain_evaluations_dispatched": dispatched, "dispatched_over_needed": round(dispatched / max(1, need), 4),
                              "wall_s": round(dt, 4),
                              "ms_per_256_chain_evaluations": round(1e3 * dt / need * 256, 3),
                              "full_batch_evaluation_ms": round(1e3 * t_eval, 3),
                              "wall_if_no_chain_dropped_s": round((args.relax_steps + 1) * t_eval, 4)}))
    eng.close()


if __name__ == "__main__":
    main()
