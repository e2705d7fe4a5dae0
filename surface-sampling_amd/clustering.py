"""Clustering of latent embeddings (reference ``mcmc/utils/clustering.py``) on the MI355X backend.

The reference's ``perform_clustering`` runs ``PCA(n_components=32, whiten=True)`` on one mean-pooled embedding row per structure,
Ward linkage on the first three whitened coordinates and ``fcluster`` by distance or cluster count; ``select_data_and_save`` keeps
one structure per cluster.  Here the PCA and the linkage run on the GPU (``backend.ClusterEngine``, ``csrc/cluster.hip``): the
linkage needs no distance matrix, so a whole run is clustered at once in O(N) memory.  ``fcluster`` is restated in numpy (SciPy is
not needed), with the cluster numbers SciPy assigns for the same ``Z``.

One stated divergence: the reference passes ``optimal_ordering=True`` to ``linkage``.  That reorders the children inside the rows
of ``Z`` for the dendrogram plot and thereby permutes ``fcluster``'s cluster *numbers*; the partition is the same.  The optimal
leaf ordering is not built: labels are those of SciPy on the un-reordered tree ``linkage(P, "ward")``.

``device=None`` runs the same arithmetic in numpy on the host (eigen-decomposition PCA with sklearn's sign rule, Ward linkage by
rounds of reciprocal nearest neighbours): the checker of the device path, usable without a GPU.  Plots stay out of scope: they are
drawn only when the reference's ``mcmc.utils.plot`` is importable.
"""

from __future__ import annotations

import logging
import os
import pickle as pkl

import numpy as np

N_COMPONENTS = 32     # clustering.py:50
CLUSTER_DIMS = 3      # clustering.py:60


# ---- host restatement ------------------------------------------------------------------------------------------------------------
def pca_host(X, n_components=N_COMPONENTS, whiten=True):
    """sklearn's ``PCA(n_components, whiten).fit(X)`` by the eigen-decomposition of the covariance (denominator N - 1): components by
    decreasing eigenvalue, the largest-magnitude loading of every component positive (``svd_flip(u_based_decision=False)``).
    Returns ``(X_r, params)``."""
    X = np.asarray(X, dtype=np.float64)
    n, D = X.shape
    if not 1 <= n_components <= min(n, D):
        raise ValueError(f"n_components={n_components} must be between 0 and min(n_samples, n_features)={min(n, D)}")
    mean = X.mean(axis=0)
    Xc = X - mean
    lam, V = np.linalg.eigh(Xc.T @ Xc / (n - 1))
    order = np.argsort(-lam, kind="stable")
    lam, Vt = np.maximum(lam[order], 0.0), V[:, order].T
    sign = np.sign(Vt[np.arange(D), np.argmax(np.abs(Vt), axis=1)])
    sign[sign == 0] = 1.0
    Vt = Vt * sign[:, None]
    comp, ev = Vt[:n_components], lam[:n_components]
    X_r = Xc @ comp.T
    if whiten:
        X_r = X_r / np.maximum(np.sqrt(ev), np.finfo(np.float64).eps)
    return X_r, {"mean_": mean, "components_": comp, "explained_variance_": ev, "explained_variance_ratio_": ev / lam.sum()}


def ward_linkage_host(points, chunk=2048):
    """``scipy.cluster.hierarchy.linkage(points, "ward")`` without a distance matrix: clusters are (centroid, size), every round each
    live cluster finds its nearest live cluster (lowest position on ties) and all reciprocal pairs merge.  Returns ``(Z, rounds)``."""
    P = np.ascontiguousarray(points, dtype=np.float64)
    n = P.shape[0]
    cen, siz, cid = P.copy(), np.ones(n), np.arange(n)
    rec = np.zeros((n - 1, 4))
    n_rec = rounds = 0
    while len(cid) > 1:
        m = len(cid)
        nn = np.empty(m, dtype=np.int64)
        for a in range(0, m, chunk):
            b = min(m, a + chunk)
            d2 = np.zeros((b - a, m))
            for e in range(P.shape[1]):
                df = cen[a:b, e, None] - cen[None, :, e]
                d2 += df * df
            key = d2 * ((siz[a:b, None] * siz[None, :]) / (siz[a:b, None] + siz[None, :]))
            key[np.arange(b - a), np.arange(a, b)] = np.inf
            nn[a:b] = np.argmin(key, axis=1)
        idx = np.arange(m)
        lower = (nn[nn] == idx) & (idx < nn)
        i = idx[lower]
        j = nn[i]
        si, sj = siz[i], siz[j]
        st = si + sj
        df = cen[i] - cen[j]
        k = len(i)
        rec[n_rec:n_rec + k, 0], rec[n_rec:n_rec + k, 1] = cid[i], cid[j]
        rec[n_rec:n_rec + k, 2] = np.sqrt(2.0 * ((si * sj) / st)) * np.sqrt((df * df).sum(axis=1))
        rec[n_rec:n_rec + k, 3] = st
        cen[i] = (si[:, None] * cen[i] + sj[:, None] * cen[j]) / st[:, None]
        siz[i] = st
        cid[i] = n + n_rec + np.arange(k)
        keep = np.ones(m, dtype=bool)
        keep[j] = False
        cen, siz, cid = cen[keep], siz[keep], cid[keep]
        n_rec += k
        rounds += 1
    return records_to_Z(rec, n), rounds


def records_to_Z(rec, n):
    """Merge records in creation order (ids: leaves 0 .. n-1, record r = n + r) -> SciPy's ``Z``: sorted by height (stable), row r
    creates cluster n + r, the smaller id first."""
    order = np.argsort(rec[:, 2], kind="stable")
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    ids = rec[order][:, :2].astype(np.int64)
    big = ids >= n
    ids[big] = n + rank[ids[big] - n]
    Z = np.empty((len(order), 4))
    Z[:, 0], Z[:, 1] = ids.min(axis=1), ids.max(axis=1)
    Z[:, 2:] = rec[order][:, 2:]
    return Z


def fcluster(Z, t, criterion="distance", depth=2):
    """``scipy.cluster.hierarchy.fcluster(Z, t, criterion)`` for ``"distance"`` and ``"maxclust"``, with SciPy's cluster numbers
    (left-first traversal from the root; a cluster is numbered when its leader is first met).  ``depth`` only affects the
    ``inconsistent`` criterion and is accepted and ignored."""
    Z = np.asarray(Z, dtype=np.float64)
    n = Z.shape[0] + 1
    left, right = Z[:, 0].astype(np.int64), Z[:, 1].astype(np.int64)
    md = Z[:, 2].copy()                       # maximum merge height inside every subtree
    for i in range(n - 1):
        if left[i] >= n:
            md[i] = max(md[i], md[left[i] - n])
        if right[i] >= n:
            md[i] = max(md[i], md[right[i] - n])
    if criterion == "distance":
        cutoff = float(t)
    elif criterion == "maxclust":
        # SciPy bisects over the heights for the smallest threshold that leaves at most t clusters ("no merge at all" included)
        max_nc = max(int(t), 1)
        if max_nc >= n:                       # every observation alone: SciPy numbers them in row order
            return np.arange(1, n + 1, dtype=np.int32)
        cutoff = np.sort(md)[n - max_nc - 1]
    else:
        raise ValueError(f"criterion {criterion!r} is not supported (distance, maxclust)")
    T = np.zeros(n, dtype=np.int32)
    visited = np.zeros(n - 1, dtype=bool)
    stack, n_cluster, leader = [n - 2], 0, -1
    left_l, right_l, md_l = left.tolist(), right.tolist(), md.tolist()
    while stack:
        root = stack[-1]
        lc, rc = left_l[root], right_l[root]
        if leader == -1 and md_l[root] <= cutoff:
            leader = root
            n_cluster += 1
        if lc >= n and not visited[lc - n]:
            visited[lc - n] = True
            stack.append(lc - n)
            continue
        if rc >= n and not visited[rc - n]:
            visited[rc - n] = True
            stack.append(rc - n)
            continue
        if lc < n:
            if leader == -1:
                n_cluster += 1
            T[lc] = n_cluster
        if rc < n:
            if leader == -1:
                n_cluster += 1
            T[rc] = n_cluster
        if leader == root:
            leader = -1
        stack.pop()
    return T


# ---- the device flow -----------------------------------------------------------------------------------------------------------------
def _device_ordinal(device):
    if device is None:
        return None
    if isinstance(device, int):
        return device
    s = str(device)
    if s == "cpu":
        return None
    return int(s.split(":")[1]) if ":" in s else 0


class LatentClustering:
    """PCA + Ward linkage of embedding rows that stay on the GPU.

        lc = LatentClustering(dim=128, device=0)
        for batch in batches:
            painn_engine.evaluate(batch)                 # embeddings resident
            lc.append_resident(painn_engine, model=0)    # one mean row per structure, device to device
        y = lc.fit(clustering_cutoff=200, cutoff_criterion="maxclust")

    ``device=None`` keeps the rows on the host and runs the numpy restatement.  After ``fit``: ``Z_``, ``X_r_``, ``pca_`` (sklearn's
    attribute names), ``n_rounds_``, ``labels_``."""

    def __init__(self, dim, n_components=N_COMPONENTS, whiten=True, cluster_dims=CLUSTER_DIMS, device=0):
        self.dim, self.n_components, self.whiten, self.cluster_dims = int(dim), int(n_components), bool(whiten), int(cluster_dims)
        self.device = _device_ordinal(device)
        self._rows = []
        self._engine = None
        if self.device is not None:
            from . import backend

            self._engine = backend.ClusterEngine(self.dim, self.n_components, self.whiten, self.cluster_dims, self.device)

    @property
    def n_rows(self):
        return self._engine.n_rows if self._engine is not None else sum(len(r) for r in self._rows)

    def append_rows(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.dim)
        if self._engine is not None:
            self._engine.append_rows(x)
        else:
            if not np.all(np.isfinite(x)):
                raise ValueError("rows hold a non-finite value")
            self._rows.append(x.copy())

    def append_resident(self, painn_engine, model=0):
        if self._engine is None:
            raise ValueError("append_resident needs a device (device=None keeps rows on the host: use append_rows)")
        self._engine.append_resident(painn_engine, model)

    def clear(self):
        self._rows = []
        if self._engine is not None:
            self._engine.clear()

    def linkage(self):
        """PCA and linkage of the resident rows; returns ``Z``."""
        if self._engine is not None:
            self.pca_info_ = self._engine.pca()
            self.pca_ = self._engine.pca_params()
            self.X_r_ = self._engine.projected()
            self.Z_, self.n_rounds_ = self._engine.linkage()
        else:
            self.X_r_, self.pca_ = pca_host(np.concatenate(self._rows), self.n_components, self.whiten)
            self.Z_, self.n_rounds_ = ward_linkage_host(self.X_r_[:, :self.cluster_dims])
        return self.Z_

    def fit(self, clustering_cutoff, cutoff_criterion="distance"):
        self.linkage()
        crit = "distance" if cutoff_criterion == "distance" else "maxclust"
        self.labels_ = fcluster(self.Z_, clustering_cutoff, criterion=crit, depth=2)
        return self.labels_

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None


def _reference_plots():
    try:
        from mcmc.utils import plot_settings
        from mcmc.utils.plot import plot_clustering_results, plot_dendrogram

        return plot_settings, plot_clustering_results, plot_dendrogram
    except Exception:
        return None


def perform_clustering(embeddings, clustering_cutoff, cutoff_criterion="distance", save_folder="./", save_prepend="", logger=None,
                       **kwargs):
    """The reference's ``perform_clustering`` (``mcmc/utils/clustering.py:21-85``): PCA(32, whiten) on the embedding rows, Ward
    linkage on the first three whitened coordinates, ``fcluster`` by ``"distance"`` or (anything else) ``"maxclust"``.  Returns the
    cluster number of every row.  ``device`` (keyword, default 0) selects the GPU; ``device=None`` runs the numpy restatement.
    Labels are SciPy's for ``linkage(..., "ward")`` without ``optimal_ordering``: same partition as the reference, the numbers may
    be permuted (module docstring)."""
    logger = logger or logging.getLogger(__name__)
    device = kwargs.pop("device", 0)
    X = np.stack([np.asarray(e, dtype=np.float64).reshape(-1) for e in embeddings])
    lc = LatentClustering(X.shape[1], n_components=kwargs.pop("n_components", N_COMPONENTS), whiten=True,
                          cluster_dims=kwargs.pop("cluster_dims", CLUSTER_DIMS), device=device)
    try:
        lc.append_rows(X)
        y = lc.fit(clustering_cutoff, cutoff_criterion)
    finally:
        lc.close()
    logger.info("X_r has shape %s", lc.X_r_.shape)
    logger.info("X has shape %s", X.shape)
    logger.info("The first pca explained ratios are %s", lc.pca_["explained_variance_ratio_"][:5])
    num_clusters = len(np.unique(y))
    logger.info("There are %s clusters", num_clusters)
    plots = _reference_plots()
    if plots is not None:
        plot_settings, plot_clustering_results, plot_dendrogram = plots
        plot_dendrogram(lc.Z_, save_prepend=save_prepend, save_folder=save_folder)
        plot_clustering_results(lc.X_r_, num_clusters, y, cmap=plot_settings.cmap, save_prepend=save_prepend, save_folder=save_folder,
                                title=False)
    return y


def select_indices(y, metric_values, clustering_metric="force_std", rng=None):
    """One row index per cluster, clusters in ascending number: the row with the largest metric, the earliest row on ties (the
    reference's stable two-key ``sort_values`` followed by ``groupby().first()``); ``"random"``: a uniformly drawn row."""
    y = np.asarray(y).reshape(-1)
    mv = np.asarray(metric_values, dtype=np.float64).reshape(-1)
    order = np.lexsort((-mv, y))              # stable: cluster ascending, metric descending, then row order
    ys = y[order]
    first = np.flatnonzero(np.r_[True, ys[1:] != ys[:-1]])
    if clustering_metric in "random":         # (the reference's test: a substring of "random")
        rng = rng or np.random.default_rng()
        last = np.r_[first[1:], len(ys)]
        return order[rng.integers(first, last)]
    return order[first]


def select_data_and_save(atoms_batches, y, metric_values, clustering_metric="force_std", save_folder="./", save_prepend="",
                         logger=None):
    """The reference's ``select_data_and_save`` (``mcmc/utils/clustering.py:88-157``) without pandas: one structure per cluster by
    ``select_indices``, pickled to ``<save_prepend>clustered.pkl``.  Returns the selected row indices."""
    logger = logger or logging.getLogger(__name__)
    selected = select_indices(y, metric_values, clustering_metric)
    logger.info("Cluster: %s metric value: %s", np.asarray(y)[selected[0]], np.asarray(metric_values)[selected[0]])
    selected_atoms = [atoms_batches[i] for i in selected.tolist()]
    logger.info("Saving %d Atoms objects", len(selected_atoms))
    path = os.path.join(save_folder, save_prepend + "clustered.pkl")
    with open(path, "wb") as f:
        pkl.dump(selected_atoms.copy(), f)
    logger.info("Saved to %s", path)
    return selected


def get_cluster_centers(points, n_clusters, device=0):
    """The reference's ``get_cluster_centers`` (``:160-188``): Ward linkage of ``points`` (up to 32 columns on the device), cut into
    ``n_clusters``; returns ``(centers, labels)``."""
    points = np.asarray(points, dtype=np.float64)
    dev = _device_ordinal(device)
    if dev is None:
        Z, _ = ward_linkage_host(points)
    else:
        from . import backend

        eng = backend.ClusterEngine(points.shape[1], n_components=1, cluster_dims=points.shape[1], device=dev)
        try:
            eng.set_points(points)
            Z, _ = eng.linkage()
        finally:
            eng.close()
    labels = fcluster(Z, n_clusters, criterion="maxclust")
    centers = [np.mean(points[labels == i], axis=0) for i in range(1, n_clusters + 1)]
    return np.array(centers), labels


def find_closest_points_indices(points, centers, labels):
    """Index of the point of every cluster that is closest to the cluster's centre (the reference's function, ``:201-233``)."""
    out = []
    for i in range(1, len(centers) + 1):
        idx = np.where(labels == i)[0]
        out.append(idx[np.argmin(np.linalg.norm(points[idx] - centers[i - 1], axis=1))])
    return np.array(out)
