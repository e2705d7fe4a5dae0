"""Independent numpy statement of the latent-space clustering (csrc/cluster.hip, surface_sampling_amd/clustering.py), and the
fixture loader of its tests.  Deliberately written another way than the package's host path: the PCA through the SVD of the centred
rows (what sklearn's "full" solver does), the Ward linkage by rounds of reciprocal nearest neighbours over one dense key matrix,
flat clusters by union-find over the merges at or below the cut (a partition, no numbering)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAXCLUST = (2, 12, 200)


def load(name):
    with np.load(os.path.join(GOLDEN, f"cluster_{name}.npz")) as f:
        return {k: f[k] for k in f.files}


def pca_svd(X, n_components=32, whiten=True):
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    mean = X.mean(axis=0)
    U, S, Vt = np.linalg.svd(X - mean, full_matrices=False)
    sign = np.sign(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)])
    Vt, U = Vt * sign[:, None], U * sign[None, :]
    ev = S ** 2 / (n - 1)
    X_r = U[:, :n_components] * S[:n_components]
    if whiten:
        X_r = X_r / np.sqrt(ev[:n_components])
    return X_r, {"mean_": mean, "components_": Vt[:n_components], "explained_variance_": ev[:n_components],
                 "explained_variance_ratio_": ev[:n_components] / ev.sum()}


def pca_longdouble(X, n_components=32, whiten=True):
    """The PCA with the mean and the centred covariance accumulated in np.longdouble, the covariance then rounded to fp64 and solved
    by numpy.linalg.eigh; components by decreasing eigenvalue (clamped at 0), the largest-magnitude loading positive, whitening by
    max(sqrt(l), eps).  A second, equally valid solver: its distance from pca_svd says how far two correct answers lie apart."""
    Xl = np.asarray(X, dtype=np.float64).astype(np.longdouble)
    n, D = Xl.shape
    mean = Xl.sum(axis=0) / np.longdouble(n)
    Xc = Xl - mean
    cov = (Xc.T @ Xc) / np.longdouble(n - 1)
    lam, V = np.linalg.eigh(cov.astype(np.float64))
    order = np.argsort(-lam, kind="stable")
    lam, Vt = np.maximum(lam[order], 0.0), V[:, order].T
    sign = np.sign(Vt[np.arange(D), np.argmax(np.abs(Vt), axis=1)])
    sign[sign == 0] = 1.0
    comp, ev = (Vt * sign[:, None])[:n_components], lam[:n_components]
    X_r = (Xc @ comp.T.astype(np.longdouble)).astype(np.float64)
    if whiten:
        X_r = X_r / np.maximum(np.sqrt(ev), np.finfo(np.float64).eps)
    return X_r, {"mean_": mean.astype(np.float64), "components_": comp, "explained_variance_": ev,
                 "explained_variance_ratio_": ev / lam.sum()}


def ward_rnn(points, margin=False):
    """(Z, rounds): Ward linkage by rounds of reciprocal nearest neighbours, lowest position wins a tie.  With ``margin`` also the
    smallest relative gap (second - best) / second between the best and the second-best key of any cluster in any round (rounds with
    two live clusters have no second key and are skipped): how far the tree is from a decision that rounding could turn."""
    P = np.asarray(points, dtype=np.float64)
    n = len(P)
    cen, siz, cid = [p for p in P], [1.0] * n, list(range(n))
    rec, rounds, gap = [], 0, np.inf
    while len(cid) > 1:
        C, s = np.array(cen), np.array(siz)
        d2 = sum((C[:, None, e] - C[None, :, e]) ** 2 for e in range(C.shape[1]))
        key = d2 * (s[:, None] * s[None, :] / (s[:, None] + s[None, :]))
        np.fill_diagonal(key, np.inf)
        nn = key.argmin(axis=1)
        if margin and len(cid) > 2:
            two = np.partition(key, 1, axis=1)[:, :2]
            gap = min(gap, float(np.min(np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / np.where(two[:, 1] > 0, two[:, 1], 1.0), 0.0))))
        dead = set()
        for i in range(len(cid)):
            j = int(nn[i])
            if nn[j] == i and i < j:
                st = siz[i] + siz[j]
                h = np.sqrt(2.0 * siz[i] * siz[j] / st) * np.sqrt(((cen[i] - cen[j]) ** 2).sum())
                rec.append((cid[i], cid[j], h, st))
                cen[i] = (siz[i] * cen[i] + siz[j] * cen[j]) / st
                siz[i], cid[i] = st, n + len(rec) - 1
                dead.add(j)
        cen = [c for k, c in enumerate(cen) if k not in dead]
        siz = [c for k, c in enumerate(siz) if k not in dead]
        cid = [c for k, c in enumerate(cid) if k not in dead]
        rounds += 1
    rec = np.array(rec)
    order = np.argsort(rec[:, 2], kind="stable")
    rank = np.argsort(order, kind="stable")
    Z = np.zeros((n - 1, 4))
    for r, o in enumerate(order):
        a, b = (int(v) if v < n else n + int(rank[int(v) - n]) for v in rec[o, :2])
        Z[r] = (min(a, b), max(a, b), rec[o, 2], rec[o, 3])
    return (Z, rounds, gap) if margin else (Z, rounds)


def partition(Z, t, criterion):
    """Flat clusters as a canonical label vector (clusters numbered by their first row)."""
    Z = np.asarray(Z)
    n = len(Z) + 1
    h = Z[:, 2]
    if criterion == "maxclust":
        k = int(t)
        if k >= n:
            return np.arange(n)
        t = np.sort(h)[n - k - 1]
    parent = list(range(2 * n - 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for r in range(n - 1):      # (Ward heights are monotone: a node is inside a flat cluster exactly when its height is <= t)
        if h[r] <= t:
            parent[find(int(Z[r, 0]))] = n + r
            parent[find(int(Z[r, 1]))] = n + r
    return canonical(np.array([find(i) for i in range(n)]))


def canonical(labels):
    _, first, inv = np.unique(np.asarray(labels), return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inv]


def same_partition(a, b):
    return np.array_equal(canonical(a), canonical(b))


def cuts(fx):
    """Every recorded cut of a linkage fixture: (criterion, t, labels)."""
    out = [("maxclust", int(k), fx[f"labels_maxclust_{k}"]) for k in MAXCLUST if f"labels_maxclust_{k}" in fx]
    out += [("distance", float(t), fx[f"labels_distance_{i}"]) for i, t in enumerate(fx["distance_cuts"])]
    return out
