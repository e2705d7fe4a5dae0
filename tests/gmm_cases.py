"""Inputs of the Gaussian-mixture tests beyond the fixture shapes (tests/test_gpu_gmm_shapes.py), each built once from fixed seeds,
with what a device test presumes about them; tests/test_gmm_cases_cpu.py asserts those presumptions against the numpy restatements
(tests/gmm_oracle.py, tests/gmm_fit_oracle.py) without a GPU."""
import functools

import numpy as np

import gmm_fit_oracle as fo
import gmm_oracle as go

COVS = ("full", "tied", "diag", "spherical")
cached = functools.lru_cache(maxsize=None)


def nb(D):
    """Number of 16-column blocks of the padded width: the template argument of k_gmm_logp."""
    return (D + 15) // 16


# ---- A. scoring of caller rows ------------------------------------------------------------------------------------------------------
# 16 NB - 15 for every NB (the largest pad of each instantiation), plus 15 and 255 (the smallest pad of the first and the last)
A_DIMS = (1, 15, 17, 33, 49, 65, 81, 97, 113, 129, 145, 161, 177, 193, 209, 225, 241, 255)
A_ROW_COUNTS = (1, 63, 64, 65, 128, 129)   # around the 64-row workgroup of k_gmm_logp


def score_rows_like_the_shape_test(means, rng, n_ordinary=150):
    """The rows of test_caller_rows_every_shape_and_covariance_type: the means themselves, ordinary rows, three 100 sigma outliers.
    One column carries a 100 sigma outlier to an NLL of a few thousand only, short of the 1e4 that test asks for (NLL ~ D z^2 / 2):
    the outliers of D = 1 lie at 1000 sigma, which puts them in the same 1e4 .. 1e6 range as the wider rows."""
    D = means.shape[1]
    far = 100.0 if D > 1 else 1000.0
    return np.concatenate([means + 0.0, rng.normal(size=(n_ordinary, D)), means[:1] + far * rng.normal(size=(3, D))])


@cached
def scoring_case(K, D, cov, n_ordinary=150):
    """(means, P [K][D][D], weights, rows) of a seeded random mixture of one covariance type."""
    means, prec, w = go.random_gmm(K, D, cov, seed=K + D)
    rows = score_rows_like_the_shape_test(means, np.random.default_rng(K * 1000 + D), n_ordinary)
    return means, go.expand(prec, cov, K, D), w, rows


def block_mask(P):
    """[NB][NB] 0/1: the 16 x 16 blocks of one factor that hold a non-zero entry (what gmm_upload finds and k_gmm_logp skips by)."""
    D = len(P)
    n = nb(D)
    pad = np.zeros((16 * n, 16 * n))
    pad[:D, :D] = P
    return (pad.reshape(n, 16, n, 16) != 0.0).any(axis=(1, 3)).astype(np.uint8)


MASK_KINDS = ("diagonal", "upper", "lower", "dense", "upper_with_hole", "block_diagonal")


@cached
def mask_case(D=80):
    """One mixture of six components whose zero-block patterns differ (MASK_KINDS, in this order): (means, P, weights, rows)."""
    rng = np.random.default_rng(480)
    K = len(MASK_KINDS)

    def upper():
        A = rng.normal(size=(D, D)) / np.sqrt(D)
        return np.linalg.inv(np.linalg.cholesky(A @ A.T + 0.5 * np.eye(D))).T

    P = np.zeros((K, D, D))
    P[0] = np.diag(1.0 / np.sqrt(rng.uniform(0.3, 2.0, D)))
    P[1] = upper()
    U = upper()
    P[2] = np.linalg.cholesky(U @ U.T)                    # what set_init(precisions=...) produces
    Q = np.linalg.qr(rng.normal(size=(D, D)))[0]          # a fixed orthogonal matrix
    dense = upper() @ Q
    P[3] = dense * np.where(np.diagonal(dense) < 0, -1.0, 1.0)[:, None]   # rows flipped so that the diagonal is positive
    P[4] = upper()
    P[4][16:32, 48:64] = 0.0                              # one off-diagonal block of exact zeros
    for a, b in ((0, 32), (32, 80)):                      # two dense diagonal blocks of 2 and 3 sixteens
        blk = upper()[a:b, a:b] @ np.linalg.qr(rng.normal(size=(b - a, b - a)))[0]
        P[5][a:b, a:b] = blk * np.where(np.diagonal(blk) < 0, -1.0, 1.0)[:, None]
    means = rng.normal(size=(K, D))
    w = rng.uniform(0.2, 1.0, K)
    return means, P, w / w.sum(), score_rows_like_the_shape_test(means, rng, 70)


@cached
def zero_weight_case(D=33, K=5):
    """(means, P, weights with w[1] = w[3] = 0, rows)."""
    means, P, w, rows = scoring_case(K, D, "full", 80)
    w = w.copy()
    w[[1, 3]] = 0.0
    return means, P, w / w.sum(), rows


# ---- B. chains of the resident embedding -----------------------------------------------------------------------------------------------
B_CHAINS = (1, 255, 256, 257, 540)   # one atom; around the 256 threads of k_gmm_reduce; the 60-atom slab repeated 3 x 3 x 1


def long_chains(golden):
    """The 60-atom SrTiO3 slab repeated 3 x 3 x 1 (540 atoms, the first 60 are the slab itself) and its first n atoms."""
    s = golden.structure("SrTiO3_2x2_pristine")
    Z, pos, cell, pbc = np.asarray(s.numbers), np.asarray(s.positions), np.asarray(s.cell), np.asarray(s.pbc)
    shifts = [i * cell[0] + j * cell[1] for i in range(3) for j in range(3)]
    Zr = np.concatenate([Z] * 9)
    posr = np.concatenate([pos + t for t in shifts])
    cellr = cell * np.array([3.0, 3.0, 1.0])[:, None]
    return [(Zr[:n], posr[:n], cellr, pbc) for n in B_CHAINS]


# ---- C. one EM iteration -----------------------------------------------------------------------------------------------------------------
C_CASES = ([("full", 256, 16, 24576), ("diag", 256, 16, 24576), ("tied", 256, 16, 24576), ("full", 2, 255, 2300)]
           + [("full", 3, 17, N) for N in (257, 258, 259, 260, 1025)] + [("tied", 5, 33, N) for N in (257, 258, 259, 260, 1025)]
           + [("spherical", 7, 15, 449), ("diag", 2, 1, 2)])


def precision_matrices(pc, cov):
    """Precision matrices (sklearn's precisions_init) of precision Cholesky factors."""
    if cov == "full":
        return np.einsum("kij,klj->kil", pc, pc)
    return pc @ pc.T if cov == "tied" else pc ** 2


def _start(K, D, cov, seed):
    means, pc, w = go.random_gmm(K, D, cov, seed=seed)
    return means, w, precision_matrices(pc, cov)


def _f32(X):
    return X.astype(np.float32).astype(np.float64)


@cached
def em_case(cov, K, D, N):
    """Start (means, weights, precisions), rows (balanced labels, unit noise), reg_covar and the restatement's iteration."""
    rng = np.random.default_rng(K * 100 + D + N)
    means, w, prec = _start(K, D, cov, seed=K + D)
    X = _f32(means[rng.permutation(N) % K] + rng.normal(size=(N, D)))
    reg = 1e-3 if N == 2 else 1e-6
    lb, w1, m1, cov1, pc1 = fo.em_iteration(X, w, means, fo.init_precision_cholesky(prec, cov), cov, reg)
    want = {"lower_bounds_": np.array([lb]), "weights_": w1, "means_": m1, "covariances_": cov1, "precisions_cholesky_": pc1}
    return {"means": means, "weights": w, "precisions": prec, "X": X, "reg_covar": reg, "want": want}


def covariance_condition(cov1, cov):
    """max_k cond(S_k) of covariances in sklearn's shape."""
    if cov == "full":
        return max(float(np.linalg.cond(c)) for c in cov1)
    if cov == "tied":
        return float(np.linalg.cond(cov1))
    if cov == "diag":
        return float((cov1.max(axis=1) / cov1.min(axis=1)).max())
    return 1.0


# ---- D. start-up paths -------------------------------------------------------------------------------------------------------------------
D_DIMS = (20, 33)
D_PARTIAL = (("means",), ("weights",), ("precisions",), ("means", "precisions"), ("weights", "means"))


@cached
def start_case(cov, D, N=600, K=3):
    """Overlapping clusters (so that the start decides the first E step), labels, and explicit values unlike what the labels give."""
    rng = np.random.default_rng(D * 10 + COVS.index(cov) + N)
    centres = 0.6 * rng.normal(size=(K, D))
    labels = (rng.permutation(N) % K).astype(np.int32)
    X = _f32(centres[labels] + rng.normal(size=(N, D)))
    means, w, prec = _start(K, D, cov, seed=D + 7)
    given = {"means": centres + 0.3 * means, "weights": np.array([0.2, 0.3, 0.5]), "precisions": prec}
    return {"X": X, "labels": labels, "given": given, "K": K}


def start_kwargs(case, names):
    return {n + "_init": case["given"][n] for n in names}


@cached
def start_want(cov, D, names):
    c = start_case(cov, D)
    return fo.fit(c["X"], c["K"], cov, tol=0.0, max_iter=1, labels=c["labels"], **start_kwargs(c, names))


@cached
def unlabelled_case(cov, D, N=1100):
    """Labels with -1 on a quarter of the rows: the whole 256-row block 256 .. 511 and 19 rows spread over the rest."""
    c = dict(start_case(cov, D, N))
    labels = c["labels"].copy()
    labels[256:512] = -1
    rest = np.concatenate([np.arange(256), np.arange(512, N)])
    labels[np.random.default_rng(D).choice(rest, N // 4 - 256, replace=False)] = -1
    c["labels"] = labels
    c["want"] = fo.fit(c["X"], c["K"], cov, tol=0.0, max_iter=1, labels=labels)
    return c


# ---- E. restarts ---------------------------------------------------------------------------------------------------------------------------
E_SEED, E_MAX_ITER, E_TOL, E_M = 5, 30, 1e-3, 4
E_GAP = 1e-3   # final bounds of two restarts further apart than this cannot change order between the device and the restatement


def separated(K=4, D=12, n_per=400, seed=0):
    """The rows of test_seeded_initialisers."""
    rng = np.random.default_rng(seed)
    centres = 12.0 * rng.normal(size=(K, D))
    labels = np.repeat(np.arange(K), n_per)
    X = centres[labels] + rng.normal(size=(K * n_per, D))
    perm = rng.permutation(len(X))
    return _f32(X[perm]), labels[perm]


@cached
def restart_bounds(init, cov, seed=E_SEED, m=E_M):
    """Final lower bounds of restarts 0 .. m-1 by the restatement."""
    X, _ = separated()
    out = []
    for r in range(m):
        labels = fo.kmeans(X, 4, seed, r)[0] if init == "kmeans" else fo.random_from_data_labels(len(X), 4, seed, r)
        out.append(fo.fit(X, 4, cov, tol=E_TOL, max_iter=E_MAX_ITER, labels=labels)["lower_bound_"])
    return np.array(out)


def best_init(bounds, m):
    """Index the driver reports for n_init = m: the first restart that reaches the largest bound."""
    return int(np.argmax(bounds[:m]))


# ---- F. k-means --------------------------------------------------------------------------------------------------------------------------------
F_CASES = ((4, 12, 1600, 1), (3, 33, 700, 2), (16, 5, 3000, 14))   # (K, D, N, seed)
F_EVERY_RESTART = (16, 5, 3000, 14)   # its restated restarts improve in order: n_init = 1, 2, 3 report restarts 0, 1, 2
F_GAP = 1e-6                           # relative gap of two one-iteration bounds that rounding (ONE_ITER_REL = 1e-8) cannot close
F_RESTARTS = 3
F_MARGIN = 1e-9


@cached
def kmeans_rows(K, D, N):
    if (K, D, N) == (4, 12, 1600):
        return separated()[0]
    rng = np.random.default_rng(K + D + N)
    centres = 4.0 * rng.normal(size=(K, D))
    return _f32(centres[rng.integers(0, K, N)] + rng.normal(size=(N, D)))


@cached
def kmeans_case(K, D, N, seed, restart):
    """Rows, the restated labels of one restart with their margins, and the restatement's one EM iteration from those labels."""
    X = kmeans_rows(K, D, N)
    labels, centres, margins = fo.kmeans(X, K, seed, restart)
    want = fo.fit(X, K, "full", tol=0.0, max_iter=1, labels=labels)
    return {"X": X, "labels": labels, "margins": margins, "want": want}


EMPTY_SEED, EMPTY_REG = 3, 1e-3


@cached
def empty_cluster_case(cov="full"):
    """Two distinct rows of small integers, 200 copies each, K = 3: every distance and every mean is exact in fp64, the third
    centre repeats one of the two, loses every tie to it and ends at the origin without members."""
    a, b = np.array([3.0, -4.0, 5.0, 3.0, -5.0, 4.0]), np.array([-4.0, 3.0, 4.0, -5.0, 3.0, 5.0])
    X = np.concatenate([np.tile(a, (200, 1)), np.tile(b, (200, 1))])[np.random.default_rng(9).permutation(400)]
    labels, centres, margins = fo.kmeans(X, 3, EMPTY_SEED, 0)
    want = fo.fit(X, 3, cov, tol=0.0, reg_covar=EMPTY_REG, max_iter=1, labels=labels)
    return {"X": X, "labels": labels, "centres": centres, "want": want}
