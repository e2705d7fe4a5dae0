#!/usr/bin/env python3
"""Device clustering of embedding-like rows (D = 128): PCA(32, whiten) and Ward linkage on three whitened coordinates.

    bench_cluster.py [--rows 1000,16384,65536,262144] [--no-host] [--out profiles/r12/bench_cluster.jsonl]

One JSON line per size: milliseconds of the PCA and of the linkage (host clock around calls that end in a device synchronise, best
of --repeat after one warm-up), the rounds, and -- where the condensed distance matrix fits (<= 16 384 rows) and scikit-learn / SciPy
are importable -- the host path's times with identical partitions asserted (maxclust 200).  The share of the search kernel comes from
a separate run under rocprofv3 --kernel-trace --stats (k_ward_nn against the other k_ward_* kernels)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from surface_sampling_amd import backend, clustering as cl  # noqa: E402


def rows(n, D=128, seed=0, blobs=7):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    spectrum = 2.0 * np.exp(-np.arange(D) / 40.0) + 0.02
    centres = rng.normal(size=(blobs, D)) * spectrum * 2.5
    return (centres[rng.integers(0, blobs, size=n)] + rng.normal(size=(n, D)) * spectrum) @ Q.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000,16384,65536,262144")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import cluster_oracle as co

    for n in [int(v) for v in a.rows.split(",")]:
        X = rows(n)
        eng = backend.ClusterEngine(128, n_components=32, whiten=True, cluster_dims=3)
        eng.append_rows(X)
        t_pca, t_link = [], []
        for it in range(a.repeat + 1):
            t0 = time.perf_counter(); eng.pca(); t1 = time.perf_counter()
            Z, rounds = eng.linkage(); t2 = time.perf_counter()
            if it:
                t_pca.append(t1 - t0); t_link.append(t2 - t1)
        t0 = time.perf_counter(); y = cl.fcluster(Z, 200, "maxclust"); t_cut = time.perf_counter() - t0
        eng.close()
        rec = {"rows": n, "dim": 128, "cluster_dims": 3, "pca_ms": 1e3 * min(t_pca), "linkage_ms": 1e3 * min(t_link), "rounds": rounds,
               "fcluster_numpy_ms": 1e3 * t_cut, "clusters": int(len(np.unique(y)))}
        if not a.no_host and n <= 16384:
            try:
                from scipy.cluster.hierarchy import fcluster, linkage
                from sklearn.decomposition import PCA
            except ImportError:
                pass
            else:
                t0 = time.perf_counter(); Xr = PCA(n_components=32, whiten=True, svd_solver="full").fit(X).transform(X); t1 = time.perf_counter()
                Zh = linkage(Xr[:, :3], method="ward", metric="euclidean"); t2 = time.perf_counter()
                assert co.same_partition(y, fcluster(Zh, 200, "maxclust")), "device and host partitions differ"
                rec.update(host_pca_ms=1e3 * (t1 - t0), host_linkage_ms=1e3 * (t2 - t1), partitions_identical=True)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
