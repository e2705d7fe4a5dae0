"""Secondary measurement (not the BASELINE metric): PaiNN ensembles (3 models) of other widths on one GPU.
Evaluations/s with forces (neighbor list + forward + reverse + force assembly, resident batch: vssr_batch_run + synchronize) for
B chains of the BASELINE configs[3] workload (bench.build_chains, 248-272 atoms per chain) at
  F = 64,  R = 16   (general path)
  F = 128, R = 20   (general path, VSSR_PAINN_PATH=general)
  F = 128, R = 20   (the specialised 128 / 20 path)
  F = 256, R = 20   (general path)
Models other than 128 / 20: the shipped weights cut / padded (tests/painn_shapes.py).  One JSON line per (shape, B).
For the kernel table: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_painn_widths.py --shapes 128g --chains 256 --reps 5
Usage: python tools/bench_painn_widths.py [--chains 256,1024] [--reps 10] [--shapes 64,128g,128,256]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = {"64": (64, 16, False), "128g": (128, 20, True), "128": (128, 20, False), "256": (256, 20, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="256,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="64,128g,128,256")
    args = ap.parse_args()
    import bench
    from painn_shapes import reshape_ensemble
    from surface_sampling_amd import backend
    from surface_sampling_amd.calculators import stoich_offset_table

    blobs0, S, offset_data = bench.load_golden()
    table, const = stoich_offset_table(offset_data)
    for B in [int(x) for x in args.chains.split(",")]:
        chains = bench.build_chains(S, 0, B)
        structs = [(s.numbers, s.positions, s.cell, s.pbc) for s in chains]
        n_atoms = sum(len(s.numbers) for s in chains)
        for key in args.shapes.split(","):
            F, R, general = SHAPES[key]
            blobs, hp = (blobs0, {}) if (F, R) == (128, 20) else reshape_ensemble(blobs0, F, R)
            old = os.environ.get("VSSR_PAINN_PATH")
            if general:
                os.environ["VSSR_PAINN_PATH"] = "general"
            else:
                os.environ.pop("VSSR_PAINN_PATH", None)
            try:
                eng = backend.PainnEngine(blobs, device=0, offset_per_z=table, offset_const=const, hparams=hp)
            finally:   # the caller's setting, as it was
                if old is None:
                    os.environ.pop("VSSR_PAINN_PATH", None)
                else:
                    os.environ["VSSR_PAINN_PATH"] = old
            eng.upload(structs)
            for _ in range(2):
                eng.run(backend.WANT_ALL)
                eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                eng.run(backend.WANT_ALL)
                eng.synchronize()
            dt = (time.perf_counter() - t0) / args.reps
            res = eng.download()
            ok = bool(np.isfinite(res["energy"]).all() and np.isfinite(res["forces"]).all())
            eng.close()
            print(json.dumps({"feat_dim": F, "n_rbf": R, "path": "general" if (general or (F, R) != (128, 20)) else "fast_128_20",
                              "chains": B, "atoms": n_atoms, "ms_per_step": round(dt * 1e3, 3),
                              "evaluations_per_s": round(B / dt, 1), "finite": ok, "models": len(blobs), "reps": args.reps}),
                  flush=True)


if __name__ == "__main__":
    main()
