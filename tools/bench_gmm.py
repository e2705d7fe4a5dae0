"""Secondary measurement (not the BASELINE metric): Gaussian-mixture uncertainty of the resident PaiNN embedding on one GPU.
B chains of the BASELINE configs[3] workload (bench.build_chains, 248-272 atoms per chain), 3-model ensemble, one evaluation; then
ms per call of
  device   vssr_gmm_score_batch on member 0 in place (rows = every atom or the structure means; order system_mean), synchronised
  host     the embedding downloaded (vssr_batch_embedding of member 0) and scored in numpy fp64 (the reference's formula)
for K in {5, 16} components, D = 128, full upper-triangular precision Cholesky factors (sklearn's form: the zero blocks below the
diagonal are skipped).  One JSON line per (B, K, rows).
For the kernel table: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_gmm.py --chains 256 --reps 5
Usage: python tools/bench_gmm.py [--chains 256,1024] [--components 5,16] [--reps 20] [--host-reps 2]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_nll(X, means, P, w, log2pi):
    n, D = X.shape
    lp = np.empty((n, len(means)))
    for k in range(len(means)):
        y = X @ P[k] - means[k] @ P[k]
        lp[:, k] = -0.5 * (D * log2pi + np.sum(y * y, axis=1)) + np.log(np.diagonal(P[k])).sum()
    wl = lp + np.log(w)
    m = wl.max(axis=1)
    return -(m + np.log(np.exp(wl - m[:, None]).sum(axis=1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="256,1024")
    ap.add_argument("--components", default="5,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    args = ap.parse_args()
    import bench
    import gmm_oracle as go
    from surface_sampling_amd import backend
    from surface_sampling_amd.calculators import stoich_offset_table

    blobs, S, offset_data = bench.load_golden()
    table, const = stoich_offset_table(offset_data)
    eng = backend.PainnEngine(blobs, device=0, offset_per_z=table, offset_const=const)
    D = 128
    for B in [int(x) for x in args.chains.split(",")]:
        chains = bench.build_chains(S, 0, B)
        eng.upload([(s.numbers, s.positions, s.cell, s.pbc) for s in chains])
        eng.run(backend.WANT_ALL)
        eng.synchronize()
        n_atoms = np.diff(eng._cfg_start)
        N = int(n_atoms.sum())
        emb = eng.embedding(0)
        scale = float(np.abs(emb).mean()) + 0.1
        for K in [int(x) for x in args.components.split(",")]:
            means, prec, w = go.random_gmm(K, D, "full", seed=K, scale=scale)
            means = means + emb.mean(axis=0)
            g = backend.GMMEngine(means, prec, w)
            for rows in ("atoms", "mean"):
                for _ in range(2):
                    nll, sysv = g.score_batch(eng, 0, rows, "system_mean")
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    g.score_batch(eng, 0, rows, "system_mean")
                dev_ms = (time.perf_counter() - t0) / args.reps * 1e3
                t0 = time.perf_counter()
                for _ in range(args.host_reps):
                    X = eng.embedding(0).astype(np.float64)
                    if rows == "mean":
                        X = np.add.reduceat(X, eng._cfg_start[:-1].astype(np.int64), axis=0) / n_atoms[:, None]
                    ref = host_nll(X, means, prec, w, 1.8378770351409912)
                host_ms = (time.perf_counter() - t0) / args.host_reps * 1e3
                err = float(np.max(np.abs(nll - ref) / (1 + np.abs(ref))))
                n_rows = N if rows == "atoms" else B
                flop = 2.0 * n_rows * K * D * (D + 16) / 2   # triangular factors: the upper block triangle of each P_k
                print(json.dumps({"chains": B, "atoms": N, "K": K, "D": D, "rows": rows, "n_rows": n_rows,
                                  "device_ms_per_call": round(dev_ms, 3), "host_ms_per_call": round(host_ms, 1),
                                  "speedup": round(host_ms / dev_ms, 1), "matrix_gflop": round(flop / 1e9, 3),
                                  "device_gflop_per_s": round(flop / dev_ms / 1e6, 1), "max_rel_dev_vs_host": err,
                                  "reps": args.reps}), flush=True)
            g.close()
    eng.close()


if __name__ == "__main__":
    main()
