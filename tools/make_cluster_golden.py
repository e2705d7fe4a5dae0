#!/usr/bin/env python3
"""Write the reference fixtures of the device clustering: tests/golden/cluster_*.npz (data only).

Usage: make_cluster_golden.py            (build host only: needs scikit-learn, scipy and pandas)
Every array is produced by the calls the reference's mcmc/utils/clustering.py makes -- sklearn.decomposition.PCA(32, whiten=True),
scipy.cluster.hierarchy.linkage(X_r[:, :3], method="ward", metric="euclidean"), fcluster(Z, t, criterion, depth=2), the pandas
sort_values / groupby of select_data_and_save -- on seeded synthetic rows (float16 values, so the fp64 input is exact); seeds are
recorded in the files.  svd_solver="full" pins the PCA: with 1 000 x 128 rows sklearn's default resolves to the randomized solver
with an unseeded generator; `ref_spread` records how far the first three whitened coordinates of five seeded default fits lie from
the full solver's, which is the tolerance of the GPU test.

Asserted before anything is written, so that the reference alone satisfies what the tests demand: the numpy restatement
(tests/cluster_oracle.py) reproduces scipy's pair and size columns of Z exactly on the two sets without duplicates; every distance
cut is at least 1e-6 x the largest height away from any merge height; the pipeline's partitions do not depend on the solver or on
optimal_ordering."""
import os
import sys

import numpy as np
import pandas as pd
from scipy.cluster.hierarchy import fcluster, linkage
from sklearn.decomposition import PCA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_oracle as co  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def embedding_rows(n, D, seed, blobs=7):
    """Embedding-like rows: `blobs` Gaussian blobs whose spread decays along a random orthonormal basis, float16 values."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    spectrum = 2.0 * np.exp(-np.arange(D) / 40.0) + 0.02   # slow decay: the randomized solver of sklearn is visibly inexact on it
    centres = rng.normal(size=(blobs, D)) * spectrum * 2.5
    which = rng.integers(0, blobs, size=n)
    X = ((centres[which] + rng.normal(size=(n, D)) * spectrum) @ Q.T + rng.normal(size=D) * 0.5)
    return X.astype(np.float16).astype(np.float64)


def distance_cuts(Z, n_clusters=(5, 40, 300)):
    h = Z[:, 2]
    n = len(h) + 1
    cuts = []
    for k in n_clusters:
        i = n - 1 - k                        # heights h[0 .. i] merged -> k clusters
        t = 0.5 * (h[i] + h[i + 1])
        assert np.min(np.abs(h - t)) >= 1e-6 * h.max(), (k, t)
        cuts.append(t)
    return np.array(cuts)


def linkage_fixture(P, seed, with_Z=True):
    Z = linkage(P, method="ward", metric="euclidean")
    out = {"points": P, "seed": np.int64(seed)}
    cuts = distance_cuts(Z) if with_Z else distance_cuts(Z, (5, 40, 150))
    out["distance_cuts"] = cuts
    for k in co.MAXCLUST:
        if with_Z or k <= 200:
            out[f"labels_maxclust_{k}"] = fcluster(Z, t=k, criterion="maxclust", depth=2)
    for i, t in enumerate(cuts):
        out[f"labels_distance_{i}"] = fcluster(Z, t=t, criterion="distance", depth=2)
    if with_Z:
        out["Z"] = Z
        Zo, _ = co.ward_rnn(P)
        assert np.array_equal(Zo[:, [0, 1, 3]], Z[:, [0, 1, 3]]), "the restatement's tree differs from scipy's: draw another seed"
        assert np.max(np.abs(Zo[:, 2] - Z[:, 2])) <= 1e-12 * Z[:, 2].max()
    return out


def main():
    # PCA
    seed = 11
    X = embedding_rows(1000, 128, seed)
    full = PCA(n_components=32, whiten=True, svd_solver="full").fit(X)
    Xr = full.transform(X)
    default = PCA(n_components=32, whiten=True).fit(X)
    assert default._fit_svd_solver == "randomized"
    spread = 0.0
    for s in range(5):
        Xd = PCA(n_components=32, whiten=True, random_state=s).fit(X).transform(X)
        spread = max(spread, float(np.max(np.abs(Xd[:, :3] - Xr[:, :3]))))
    print(f"ref_spread = {spread:.3e}")
    np.savez_compressed(os.path.join(GOLDEN, "cluster_pca_d128_n1000.npz"), X=X.astype(np.float16), X_r=Xr,
                        explained_variance_=full.explained_variance_, explained_variance_ratio_=full.explained_variance_ratio_,
                        components_=full.components_, mean_=full.mean_, ref_spread=np.float64(spread), seed=np.int64(seed))
    # linkage
    np.savez_compressed(os.path.join(GOLDEN, "cluster_ward_n1000_d3.npz"), **linkage_fixture(np.ascontiguousarray(Xr[:, :3]), seed))
    seed3 = 12
    X3 = embedding_rows(3000, 128, seed3)
    P3 = PCA(n_components=32, whiten=True, svd_solver="full").fit(X3).transform(X3)[:, :3]
    np.savez_compressed(os.path.join(GOLDEN, "cluster_ward_n3000_d3.npz"), **linkage_fixture(np.ascontiguousarray(P3), seed3))
    # duplicates: 200 distinct points, each three times, shuffled
    seedd = 13
    rng = np.random.default_rng(seedd)
    Pd = np.repeat(P3[rng.choice(3000, 200, replace=False)], 3, axis=0)[rng.permutation(600)]
    fx = linkage_fixture(np.ascontiguousarray(Pd), seedd, with_Z=False)
    assert all(float(t) > 0 for t in fx["distance_cuts"])
    np.savez_compressed(os.path.join(GOLDEN, "cluster_ward_dups_n600.npz"), **fx)
    # whole pipeline
    seedp = 14
    Xp = embedding_rows(1000, 128, seedp)
    rng = np.random.default_rng(seedp)
    out = {"X": Xp.astype(np.float16), "seed": np.int64(seedp)}
    Xf = PCA(n_components=32, whiten=True, svd_solver="full").fit(Xp).transform(Xp)
    Xd = PCA(n_components=32, whiten=True, random_state=0).fit(Xp).transform(Xp)
    Z = linkage(Xf[:, :3], method="ward", metric="euclidean")
    Zd = linkage(Xd[:, :3], method="ward", metric="euclidean", optimal_ordering=True)      # the reference's own call
    t_dist = float(distance_cuts(Z, (25,))[0])
    for crit, t in (("distance", t_dist), ("maxclust", 50)):
        y = fcluster(Z, t=t, criterion=crit, depth=2)
        assert co.same_partition(y, fcluster(Zd, t=t, criterion=crit, depth=2)), "partition depends on the solver / leaf ordering"
        out[f"labels_{crit}"] = y
        out[f"t_{crit}"] = np.float64(t)
    metric = np.round(rng.uniform(0, 1, size=1000), 1)                                     # rounded: ties inside the clusters
    out["metric_values"] = metric
    y = out["labels_maxclust"]
    df = pd.DataFrame({"cluster": y, "metric_values": metric}).reset_index()
    sel = df.sort_values(["cluster", "metric_values"], ascending=[True, False]).groupby("cluster", as_index=False).first()
    out["selected"] = sel["index"].to_numpy()
    assert len(np.unique(metric[y == y[out["selected"][0]]])) < np.sum(y == y[out["selected"][0]]), "no tie in the first cluster"
    np.savez_compressed(os.path.join(GOLDEN, "cluster_pipeline_n1000.npz"), **out)
    for f in sorted(os.listdir(GOLDEN)):
        if f.startswith("cluster_"):
            print(f, os.path.getsize(os.path.join(GOLDEN, f)))


if __name__ == "__main__":
    main()
