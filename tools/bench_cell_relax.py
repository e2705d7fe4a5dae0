"""Secondary measurement: lock-step steps per second of the variable-cell relaxation (vssr_batch_relax_cell) against the fixed-cell FIRE
(vssr_batch_relax_fire) on the same resident batch.  Per step the variable-cell driver adds the kind's stress kernels and one launch
(k_cell_step instead of k_fire_step); it never masks the evaluation.  fmax is set so low that no chain stops early: both drivers run
``--relax-steps`` steps, i.e. relax-steps + 1 lock-step evaluations.  The slabs are open along z: the in-plane mask (1, 1, 0, 0, 0, 1).
Runs --chains rattled Si(111) 5x5 slabs on Stillinger-Weber and the PaiNN bench chains (BASELINE configs[3] workload), each at every
chain count given, the two drivers alternating --repeats times (the first pair is a warm-up and is not reported).  One JSON line per
kind and chain count: median steps / s of either driver and their ratio.
Usage: python tools/bench_cell_relax.py [--chains 256 1024] [--relax-steps 20] [--repeats 4] [--kinds sw painn]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402  (golden loaders)

MASK = (1, 1, 0, 0, 0, 1)
FMAX = 1e-9


def _pair(kind, name, eng, upload, fixed, steps, repeats):
    rate = {"fire": [], "cell": []}
    for rep in range(repeats + 1):
        for driver in ("fire", "cell"):
            upload()
            eng.synchronize()
            t0 = time.perf_counter()
            if driver == "fire":
                info = eng.relax_fire(fixed=fixed, max_steps=steps, fmax=FMAX)
            else:
                info = eng.relax_cell(fixed=fixed, max_steps=steps, fmax=FMAX, mask=MASK)
            dt = time.perf_counter() - t0
            lockstep, _ = eng.relax_counts()
            assert (info["n_steps"] == steps).all(), (driver, info["n_steps"].min())
            if rep:
                rate[driver].append(lockstep / dt)
    fire, cell = float(np.median(rate["fire"])), float(np.median(rate["cell"]))
    print(json.dumps({"metric": f"variable-cell relaxation next to fixed-cell FIRE, {name}", "kind": kind, "chains": int(eng._n_cfg),
                      "relax_steps": steps, "repeats": repeats, "fire_steps_per_s": round(fire, 2), "cell_steps_per_s": round(cell, 2),
                      "fire_all": [round(r, 2) for r in rate["fire"]], "cell_all": [round(r, 2) for r in rate["cell"]],
                      "cell_over_fire": round(cell / fire, 4), "extra_ms_per_step": round(1e3 * (1.0 / cell - 1.0 / fire), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--relax-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--kinds", nargs="+", default=["sw", "painn"], choices=("sw", "painn"))
    args = ap.parse_args()
    from surface_sampling_amd import backend, sw as sw_io
    from surface_sampling_amd.calculators import stoich_offset_table

    for kind in args.kinds:
        for B in args.chains:
            if kind == "sw":
                import bench_si

                Z, X, Cl, pbc, fixed = bench_si.slab()
                n = len(Z)
                rng = np.random.default_rng(0)
                held = np.asarray(fixed, bool)
                pos = np.concatenate([X + np.where(held[:, None], 0.0, rng.normal(0, 0.1, X.shape)) for _ in range(B)])
                arrays = (np.full(B, n, np.int32), np.zeros(B * n, np.int32), pos, np.tile(np.asarray(Cl, float).reshape(1, 9), (B, 1)),
                          np.tile(np.asarray(pbc, np.uint8).reshape(1, 3), (B, 1)))
                eng = backend.SWEngine(sw_io.parse_sw(sw_io.builtin_text(bench_si.MODEL), ["Si"]), device=0)
                _pair(kind, f"Si(111) 5x5 slab, Stillinger-Weber ({n} atoms)", eng, lambda: eng.upload_arrays(*arrays), np.tile(held.astype(np.uint8), B),
                      args.relax_steps, args.repeats)
            else:
                blobs, S, offset_data = bench.load_golden()
                table, const = stoich_offset_table(offset_data)
                chains = bench.build_chains(S, 0, B)
                packs = [(s.numbers, s.positions, s.cell, s.pbc) for s in chains]
                mask = np.concatenate([(s.positions[:, 2] < s.positions[:240, 2].max() - 4.0).astype(np.uint8) for s in chains])
                eng = backend.PainnEngine(blobs, device=0, offset_per_z=table, offset_const=const)
                _pair(kind, "PaiNN bench chains (SrTiO3 slabs)", eng, lambda: eng.upload(packs), mask, args.relax_steps, args.repeats)
            eng.close()


if __name__ == "__main__":
    main()
