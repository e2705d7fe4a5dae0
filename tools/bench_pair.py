"""Secondary measurement (not the BASELINE metric): the pair potentials (pair.hip), fp64 on one GPU.  Single-point evaluations/s at B
resident chains of two workloads, each chain rattled by its own seed:
  * lj      a 192-atom fcc(100) Lennard-Jones slab (4 x 4 x 3 cells, argon numbers), pair_style lj/cut 6.0, periodic in x and y;
  * born    the 8-atom rocksalt cell tiled 3 x 3 x 3 (216 atoms) as a slab, pair_style hybrid/overlay born 8.0 coul/dsf 0.2 12.0:
            rows of several hundred slots per centre, which is what bounds it;
  * sw      tools/bench_si.py's Stillinger-Weber single point on the Si(111) 5x5 slab at the same chain counts, for scale.
For each: the resident batch re-evaluated (neighbor list + site + energy kernels; vssr_batch_run + synchronize) and the whole call
with upload and fp64 download (evaluate_arrays_f64); mean slots per atom from vssr_batch_stats.  One JSON line per measurement.
Usage: python tools/bench_pair.py [--chains 1024,4096] [--reps 10] [--no-sw]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="1024,4096")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-sw", action="store_true", help="skip the Stillinger-Weber figure of tools/bench_si.py")
    args = ap.parse_args()
    for B in [int(x) for x in args.chains.split(",") if x]:
        single_point("Lennard-Jones fcc(100) slab", LJ, 1, lj_slab(), B, args.reps)
        single_point("rocksalt slab, Born + damped-shifted Coulomb", BORN_DSF, 2, rocksalt_slab(), B, args.reps)
        if not args.no_sw:
            import bench_si

            bench_si.single_point(B, args.reps)


if __name__ == "__main__":
    main()
