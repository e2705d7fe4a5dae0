"""Secondary measurement (not the BASELINE metric): the pair potentials (pair.hip), fp64 on one GPU.  Single-point evaluations/s at B
resident chains of two workloads, each chain rattled by its own seed:
  * lj      a 192-atom fcc(100) Lennard-Jones slab (4 x 4 x 3 cells, argon numbers), pair_style lj/cut 6.0, periodic in x and y;
  * born    the 8-atom rocksalt cell tiled 3 x 3 x 3 (216 atoms) as a slab, pair_style hybrid/overlay born 8.0 coul/dsf 0.2 12.0:
            rows of several hundred slots per centre, which is what bounds it;
  * sw      tools/bench_si.py's Stillinger-Weber single point on the Si(111) 5x5 slab at the same chain counts, for scale.
For each: the resident batch re-evaluated (neighbor list + site + energy kernels; vssr_batch_run + synchronize) and the whole call
with upload and fp64 download (evaluate_arrays_f64); mean slots per atom from vssr_batch_stats.  One JSON line per measurement.
--cg-driver lockstep | resident | both adds CG relaxations/s of the rocksalt slab (the device part of an MC proposal that relaxes:
B chains rattled by their own seeds, the lower half held, vssr_batch_relax_cg with that driver) with the chain-evaluations dispatched
and needed; both: the two drivers one after the other in this process.
Usage: python tools/bench_pair.py [--chains 1024,4096] [--reps 10] [--no-sw] [--cg-driver lockstep|resident|both] [--cg-only]
       [--relax-steps 20]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LJ = ["pair_style lj/cut 6.0", "pair_coeff 1 1 0.0104 3.4"]
BORN_DSF = ["pair_style hybrid/overlay born 8.0 coul/dsf 0.2 12.0",
            "pair_coeff 1 1 born 0.2637 0.317 2.340 1.0486 -0.4993", "pair_coeff 1 2 born 0.2110 0.317 2.755 6.9906 -8.6758",
            "pair_coeff 2 2 born 0.1582 0.317 3.170 72.4022 -145.4285", "pair_coeff * * coul/dsf",
            "set type 1 charge 1.0", "set type 2 charge -1.0"]


def lj_slab():
    a = 2.0 ** (1 / 6) * 3.4 * np.sqrt(2.0)
    basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    shifts = np.array([[x, y, z] for x in range(4) for y in range(4) for z in range(3)], float)
    X = (basis[None] + shifts[:, None]).reshape(-1, 3) * a
    return np.zeros(len(X), np.int32), X, np.diag([4 * a, 4 * a, 3 * a + 15.0]), np.array([1, 1, 0], np.uint8)


def rocksalt_slab(a=5.64, reps=3):
    cat = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    frac = np.concatenate([cat, cat + [.5, .5, .5]]) % 1.0
    shifts = np.array([[x, y, z] for x in range(reps) for y in range(reps) for z in range(reps)], float)
    X = (frac[None] + shifts[:, None]).reshape(-1, 3) * a
    return np.tile(np.array([0] * 4 + [1] * 4, np.int32), len(shifts)), X, np.diag([reps * a, reps * a, reps * a + 15.0]), np.array([1, 1, 0], np.uint8)


def single_point(name, lines, n_types, struct, B, reps):
    from surface_sampling_amd import backend, pair

    T1, X, Cl, pbc = struct
    n = len(T1)
    eng = backend.PairEngine(pair.parse(lines, n_types), device=0)
    rng = np.random.default_rng(0)
    pos = np.concatenate([X + rng.normal(0, 0.05, X.shape) for _ in range(B)])
    n_atoms = np.full(B, n, np.int32)
    T = np.tile(T1, B)
    cell = np.tile(Cl.reshape(1, 9), (B, 1))
    pb = np.tile(pbc.reshape(1, 3), (B, 1))
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    for _ in range(2):
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
    st = eng.stats()
    eng.close()
    print(json.dumps({"metric": f"pair single-point evaluations/s, {name} ({n} atoms, {lines[0]})", "chains": B,
                      "evals_per_s_resident": round(B / dt_run, 1), "ms_per_batch_resident": round(1e3 * dt_run, 3),
                      "evals_per_s_call": round(B / dt_call, 1), "ms_per_batch_call": round(1e3 * dt_call, 3),
                      "mean_slots_per_atom": round(st["edges"] / st["atoms"], 1), "reps": reps}), flush=True)


def relax_cg(name, eng, struct, B, max_iter, driver, sigma=0.05, reps=2):
    """CG relaxations/s of B rattled copies of ``struct`` (atoms below the middle height held) with one driver: the best of ``reps``
    timed calls behind a warm-up call (the chain-resident pools and the lock-step buffers have grown by then)."""
    import bench_si

    T1, X, Cl, pbc = struct
    n = len(T1)
    rng = np.random.default_rng(0)
    held = X[:, 2] < 0.5 * (X[:, 2].min() + X[:, 2].max())
    pos = np.concatenate([X + np.where(held[:, None], 0.0, rng.normal(0, sigma, X.shape)) for _ in range(B)])
    arrays = (np.full(B, n, np.int32), np.tile(T1, B), pos, np.tile(Cl.reshape(1, 9), (B, 1)), np.tile(np.asarray(pbc, np.uint8).reshape(1, 3), (B, 1)))
    mask = np.tile(held.astype(np.uint8), B)
    count = bench_si.RelaxCounter(eng)
    try:
        eng.relax_cg_arrays_f64(*arrays, fixed=mask, max_iter=max_iter, rerun=False, driver=driver)
        best = None
        for _ in range(reps):
            count.reset()
            t0 = time.perf_counter()
            out = eng.relax_cg_arrays_f64(*arrays, fixed=mask, max_iter=max_iter, rerun=False, driver=driver)
            dt = time.perf_counter() - t0
            if best is None or dt < best[0]:
                best = (dt, count.report())
    finally:
        del eng.relax_cg_arrays_f64          # (the counter's wrapper)
    print(json.dumps({"metric": f"CG relaxations/s, {name} ({n} atoms, {int(held.sum())} held, <= {max_iter} iterations)", "chains": B,
                      "cg_driver": driver, "relaxations_per_s": round(B / best[0], 1), "s_per_batch": round(best[0], 4),
                      "mean_n_eval": round(float(out[5].mean()), 2), "min_n_eval": int(out[5].min()), "max_n_eval": int(out[5].max()),
                      "regrows_last_call": eng.debug_capacity(), **best[1]}), flush=True)


def main():
    import bench_si

    ap = argparse.ArgumentParser()
    ap.add_argument("--cg-driver", choices=("none",) + bench_si.CG_DRIVERS, default="none", help="also measure CG relaxations of the rocksalt slab")
    ap.add_argument("--cg-only", action="store_true", help="skip the single-point figures")
    ap.add_argument("--relax-steps", type=int, default=20)
    ap.add_argument("--chains", default="1024,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-sw", action="store_true", help="skip the Stillinger-Weber figure of tools/bench_si.py")
    args = ap.parse_args()
    if args.cg_driver != "none":
        from surface_sampling_amd import backend, pair

        eng = backend.PairEngine(pair.parse(BORN_DSF, 2), device=0)
        for B in [int(x) for x in args.chains.split(",") if x]:
            for driver in bench_si.drivers_of(args.cg_driver):
                relax_cg("rocksalt slab, Born + damped-shifted Coulomb", eng, rocksalt_slab(), B, args.relax_steps, driver)
        eng.close()
    for B in [] if args.cg_only else [int(x) for x in args.chains.split(",") if x]:
        single_point("Lennard-Jones fcc(100) slab", LJ, 1, lj_slab(), B, args.reps)
        single_point("rocksalt slab, Born + damped-shifted Coulomb", BORN_DSF, 2, rocksalt_slab(), B, args.reps)
        if not args.no_sw:
            bench_si.single_point(B, args.reps)


if __name__ == "__main__":
    main()
