"""Independent numpy fp64 restatement of the Gaussian-mixture EM fit (reference mcmc/uncertainty/gmm.py, i.e. sklearn's
GaussianMixture / BaseMixture.fit): E step, M step in the centred form, precision Cholesky factors, the stopping rule; the seeded
initialisers of the device fit as include/vssr_eval.h defines them (Philox draws, "random_from_data", k-means++ and Lloyd); and the
loader of the reference fixtures tests/golden/gmm_fit_*.npz (written by tools/make_gmm_fit_golden.py)."""
import glob
import os

import numpy as np

import gmm_oracle as go

ILL_DEFINED = "ill-defined empirical covariance"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMPARED = ("weights_", "means_", "covariances_", "precisions_cholesky_", "lower_bounds_")
FLOOR, FACTOR = 1e-12, 16.0   # device / restatement bound: max(FACTOR x reference-vs-sklearn discrepancy, FLOOR), relative to max|ref|


def e_step(X, weights, means, prec_chol, cov_type):
    """(lower bound, responsibilities [n][K]) with the fp64 log 2 pi."""
    K, D = means.shape
    P = go.expand(prec_chol, cov_type, K, D)
    wlp = go.log_prob(X, means, P, go.LOG2PI_F64) + np.log(weights)
    m = wlp.max(axis=1, keepdims=True)
    lpn = m[:, 0] + np.log(np.exp(wlp - m).sum(axis=1))
    return float(np.mean(lpn)), np.exp(wlp - lpn[:, None])


def m_step(X, resp, reg_covar, cov_type):
    """(n_k, means, covariances in sklearn's shape): gmm.py:164-281."""
    n, D = X.shape
    nk = resp.sum(axis=0) + 10 * np.finfo(np.float64).eps
    means = resp.T @ X / nk[:, None]
    K = len(nk)
    if cov_type == "full":
        cov = np.empty((K, D, D))
        for k in range(K):
            diff = X - means[k]
            cov[k] = (resp[:, k] * diff.T) @ diff / nk[k]
            cov[k].flat[::D + 1] += reg_covar
    elif cov_type == "tied":
        cov = (X.T @ X - (nk * means.T) @ means) / nk.sum()
        cov.flat[::D + 1] += reg_covar
    else:
        cov = resp.T @ (X * X) / nk[:, None] - 2 * means * (resp.T @ X / nk[:, None]) + means ** 2 + reg_covar
        if cov_type == "spherical":
            cov = cov.mean(axis=1)
    return nk, means, cov


def precision_cholesky(cov, cov_type):
    def one(c):
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError(ILL_DEFINED)
        return np.linalg.solve(L, np.eye(len(c))).T   # (general solve of a triangular system: exact up to rounding)

    if cov_type == "full":
        return np.stack([one(c) for c in cov])
    if cov_type == "tied":
        return one(cov)
    if np.any(cov <= 0.0):
        raise ValueError(ILL_DEFINED)
    return 1.0 / np.sqrt(cov)


def init_precision_cholesky(precisions, cov_type):
    """gmm.py:657-664: LOWER Cholesky factors of the given precision matrices (sqrt for diag / spherical)."""
    p = np.asarray(precisions, dtype=np.float64)
    if cov_type == "full":
        return np.stack([np.linalg.cholesky(q) for q in p])
    if cov_type == "tied":
        return np.linalg.cholesky(p)
    return np.sqrt(p)


def one_hot(labels, K):
    labels = np.asarray(labels)
    r = np.zeros((len(labels), K))
    ok = labels >= 0
    r[np.nonzero(ok)[0], labels[ok]] = 1.0
    return r


def fit(X, K, cov_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, means_init=None, weights_init=None, precisions_init=None,
        labels=None):
    """One restart of BaseMixture.fit from explicit parameters and / or labels; returns the fitted attributes as a dict."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    if labels is not None:
        nk, means, cov = m_step(X, one_hot(labels, K), reg_covar, cov_type)
        weights = nk / n
        pc = None if precisions_init is not None else precision_cholesky(cov, cov_type)
    else:
        weights = means = pc = cov = None
    weights = weights if weights_init is None else np.asarray(weights_init, dtype=np.float64)
    means = means if means_init is None else np.asarray(means_init, dtype=np.float64)
    pc = pc if precisions_init is None else init_precision_cholesky(precisions_init, cov_type)
    lb, trace, converged, n_iter = -np.inf, [], False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lb
        lb, resp = e_step(X, weights, means, pc, cov_type)
        nk, means, cov = m_step(X, resp, reg_covar, cov_type)
        weights = nk / nk.sum()
        pc = precision_cholesky(cov, cov_type)
        trace.append(lb)
        if abs(lb - prev) < tol:
            converged = True
            break
    return {"weights_": weights, "means_": means, "covariances_": cov, "precisions_cholesky_": pc, "n_iter_": n_iter,
            "converged_": converged, "lower_bound_": lb, "lower_bounds_": np.array(trace)}


def em_iteration(X, weights, means, prec_chol, cov_type, reg_covar):
    """One E + M step from given parameters: (lower bound, weights, means, covariances, precisions_cholesky)."""
    lb, resp = e_step(X, weights, means, prec_chol, cov_type)
    nk, m, cov = m_step(X, resp, reg_covar, cov_type)
    return lb, nk / nk.sum(), m, cov, precision_cholesky(cov, cov_type)


# ---- the seeded initialisers (csrc/gmm_fit.hip: fit_uniform, fit_draw_rows, fit_kmeans; include/vssr_eval.h) -------------------------
KMEANS_ROUNDS = 300


def uniform(seed, restart, draw):
    """u(seed, restart, draw) in [0, 1): Philox4x32-10 on counter (draw, restart, 0x676d6d, 0), key = seed; 53 bits of words 0, 1."""
    from surface_sampling_amd import mc

    seed = int(seed) & (2 ** 64 - 1)
    c = mc.philox4x32(np.array([draw, restart, 0x676D6D, 0], np.uint64), np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    return float(((int(c[0]) << 32 | int(c[1])) >> 11) * 2.0 ** -53)


def random_from_data_labels(n, K, seed, restart):
    """Labels of the "random_from_data" start: K distinct rows (repeats rejected, draws numbered from 0) own one component each,
    every other row has none (-1)."""
    rows, draw = [], 0
    while len(rows) < K:
        r = min(n - 1, int(uniform(seed, restart, draw) * n))
        draw += 1
        if r not in rows:
            rows.append(r)
    labels = np.full(n, -1, np.int32)
    labels[rows] = np.arange(K)
    return labels


def _sqdist(X, c):
    return ((X - c) ** 2).sum(axis=1)


def kmeans(X, K, seed, restart):
    """The "kmeans" start: k-means++ seeding by D^2 sampling (one candidate per centre; the cumulative walk runs over the sums of
    256-row blocks, then inside the block; a row at distance zero is passed over while another is left), then Lloyd rounds (nearest
    centre, the first on ties; means of the members over n_k + 10 eps, so a centre without members moves to the origin) until the
    inertia repeats or 300 rounds.  Returns (labels, centres, margins): ``margins["walk"]`` is the smallest |cumulative sum - target|
    / total over every comparison of the seeding, ``margins["tie"]`` the smallest (d2 - d1) / d2 of the two nearest centres of a
    row over every Lloyd round -- where either is not far above rounding, another summation order may pick differently;
    ``margins["exact_ties"]`` counts the rows whose two nearest centres were exactly as far."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    n_blk = (n + 255) // 256
    walk, tie, exact = np.inf, np.inf, 0
    first = min(n - 1, int(uniform(seed, restart, 0) * n))
    cen = [X[first].copy()]
    mind2 = np.full(n, np.inf)
    for c in range(1, K):
        mind2 = np.minimum(mind2, _sqdist(X, cen[c - 1]))
        hp = [float(mind2[256 * b:256 * (b + 1)].sum()) for b in range(n_blk)]
        tot = 0.0
        for v in hp:
            tot += v
        target = uniform(seed, restart, c) * tot
        blk, run = 0, 0.0
        while blk < n_blk - 1:
            if tot > 0:
                walk = min(walk, abs(run + hp[blk] - target) / tot)
            if not run + hp[blk] <= target:
                break
            run += hp[blk]
            blk += 1
        hm = mind2[256 * blk:256 * (blk + 1)]
        pick = 0
        while pick < len(hm) - 1:
            if tot > 0:
                walk = min(walk, abs(run + hm[pick] - target) / tot)
            if not run + hm[pick] <= target:
                break
            run += hm[pick]
            pick += 1
        while pick < len(hm) - 1 and not hm[pick] > 0.0:
            pick += 1
        cen.append(X[256 * blk + pick].copy())
    cen = np.array(cen)
    prev, labels = -1.0, None
    for _ in range(KMEANS_ROUNDS):
        d2 = np.stack([_sqdist(X, cen[k]) for k in range(K)], axis=1)
        labels = np.argmin(d2, axis=1)           # (the first on ties)
        if K > 1:
            two = np.sort(d2, axis=1)[:, :2]
            apart = two[:, 1] > two[:, 0]          # (an exact tie is counted, not measured: identical centres tie on any hardware)
            exact += int((~apart).sum())
            if apart.any():
                tie = min(tie, float(((two[apart, 1] - two[apart, 0]) / two[apart, 1]).min()))
        inertia = float(d2[np.arange(n), labels].sum())
        if inertia == prev:
            break
        prev = inertia
        r = one_hot(labels, K)
        cen = r.T @ X / (r.sum(axis=0) + 10 * np.finfo(np.float64).eps)[:, None]
    return labels.astype(np.int32), cen, {"walk": walk, "tie": tie, "exact_ties": exact}


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def fixture_names():
    return sorted(os.path.basename(p)[len("gmm_fit_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "gmm_fit_*.npz"))
                  if not p.endswith("_ref.npz"))


def load_fixture(name):
    """dict of a fixture: X (fp64 of the stored float16 rows: exact), settings, initial values, the reference's results and the
    recorded reference-vs-sklearn discrepancies ``disc_<quantity>`` = (max abs, relative to max |reference|)."""
    d = dict(np.load(os.path.join(GOLDEN, f"gmm_fit_{name}.npz"), allow_pickle=False))
    ref = os.path.join(GOLDEN, f"gmm_fit_{name}_ref.npz")
    if os.path.exists(ref):
        d.update(np.load(ref, allow_pickle=False))
    d["X"] = d["X"].astype(np.float64)
    for k in ("cov_type",):
        d[k] = str(d[k])
    for k in ("K", "max_iter", "n_iter_"):
        if k in d:
            d[k] = int(d[k])
    for k in ("tol", "reg_covar"):
        d[k] = float(d[k])
    d["raises"] = bool(d["raises"])
    if "converged_" in d:
        d["converged_"] = bool(d["converged_"])
    return d


def init_kwargs(fx):
    return {k: fx[k] for k in ("means_init", "weights_init", "precisions_init", "labels") if k in fx}


def bound(fx, key):
    """Absolute bound for ``key``: max(FACTOR x recorded relative discrepancy, FLOOR) x max |reference|."""
    return max(FACTOR * float(fx["disc_" + key][1]), FLOOR) * float(np.max(np.abs(fx[key])))


def check(fx, got, who=""):
    """Assert a fit result (dict with the sklearn attribute names) against the fixture; prints every figure first."""
    worst = {}
    for key in COMPARED:
        err = float(np.max(np.abs(np.asarray(got[key]) - fx[key])))
        worst[key] = (err, bound(fx, key))
        print(f"{who} {key}: max abs error {err:.3e}  bound {bound(fx, key):.3e}  (reference-vs-sklearn {float(fx['disc_' + key][0]):.3e})")
    assert int(got["n_iter_"]) == fx["n_iter_"], (got["n_iter_"], fx["n_iter_"])
    assert bool(got["converged_"]) == fx["converged_"]
    for key, (err, b) in worst.items():
        assert err <= b, f"{who} {key}: {err:.3e} > {b:.3e}"
