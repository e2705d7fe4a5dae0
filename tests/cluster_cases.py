"""Inputs of the shape sweep of the device clustering (csrc/cluster.hip), built once from seeds and formulas, in the manner of
tests/ewald_cases.py.  TEST INFRASTRUCTURE shared by tests/test_cluster_cpu.py (is every case what it is listed as, and does the
host path pass it?) and tests/test_gpu_cluster.py.

PCA cases (name, X, n_components, whiten, groups); ``groups`` lists the components that are compared: a tuple of one index is compared
singly (sign rule, vector, coordinate), a longer tuple only as a subspace (its eigenvalues are equal), a component in no group has a
zero eigenvalue and is only required to be finite with 0 <= explained variance <= 1e-12 l_0.
  shapes             D in 1 .. 256 around the padding (16), the dummy player (odd D) and the limit of the Jacobi kernel (256);
                     rows G diag(sigma) Q + mu, sigma geometric from 1 to 1e-3 (a non-degenerate population spectrum)
  rank_deficient     N <= D: N - 1 eigenvalues above zero, the rest clamped; n_components = min(N, D)
  degenerate         an exact spectrum (4, 4, 4, 2, 1, 1, 0.5, ...) by construction: X = sqrt(N - 1) U diag(s) V^T
  diagonal           the same with V = I: a covariance that is diagonal to rounding
  constant_column    two constant columns: zero rows and columns in the covariance
  offset             the D = 17 rows of ``shapes`` plus 1e6 in every column

Linkage cases: ``general`` (name, points) at every stored width (1, 2, 3, 4, 8, 16, 32 with and without zero padding) and at the
workgroup / tile edges; ``hierarchy(k)``: 2^k points on a line whose Ward tree is known in closed form (round b merges all sibling
blocks of 2^b points at height sqrt(2^b) g^b), exact in fp64 up to k = 17, with ``check_hierarchy_tree`` as its O(N) checker."""

import functools
from collections import namedtuple

import numpy as np

import cluster_oracle as co

PcaCase = namedtuple("PcaCase", "name X n_components whiten groups")
LinkCase = namedtuple("LinkCase", "name points")

# the bounds of tests/test_gpu_cluster.py's docstring
B_MEAN, B_EV, B_RATIO, B_VEC, B_SUB, B_XR, B_XR_WHITE = 1e-13, 1e-12, 1e-12, 1e-9, 1e-9, 1e-9, 1e-6
NULL_EV = 1e-9            # components with l_c <= NULL_EV * l_0 are not compared
WHITE_MIN = 1e-6          # whitened coordinates are compared for l_c >= WHITE_MIN * l_0
SINGLE_GAP, GROUP_EQ = 1e-3, 1e-12
# cases whose coordinate bound is max(project bound, 10 x |pca_svd - pca_longdouble|): the eigenvectors of the smallest components
# of a covariance of condition 1e6 and more are set by the solver to about eps l_0 / gap, whichever correct solver runs
# (profiles/r21/NOTES_cluster_shapes.md has both numbers per case); "offset" takes every bound that way
SPREAD_XR = ()


def _rows(D, N, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(N, D))
    Q = np.linalg.qr(rng.normal(size=(D, D)))[0]
    sigma = np.geomspace(1.0, 1e-3, D)
    mu = 2.0 * rng.normal(size=D)
    return (G * sigma) @ Q + mu + offset


def _singles(X, nc):
    """Every component above the null threshold of the oracle's spectrum, singly."""
    with np.errstate(all="ignore"):
        ev = co.pca_svd(X, nc, False)[1]["explained_variance_"]
    return tuple((c,) for c in range(nc) if ev[c] > NULL_EV * ev[0])


def _exact_spectrum(D, N, seed, diagonal):
    s2 = np.array([4, 4, 4, 2, 1, 1, 0.5, 0.4, 0.3, 0.25, 0.2, 0.15, 0.1, 0.08, 0.06, 0.05, 0.04][:D])
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(N, D))
    U = np.linalg.qr(A - A.mean(axis=0))[0]
    V = np.eye(D) if diagonal else np.linalg.qr(rng.normal(size=(D, D)))[0]
    X = np.sqrt(N - 1.0) * (U * np.sqrt(s2)) @ V.T
    groups = ((0, 1, 2), (3,), (4, 5)) + tuple((c,) for c in range(6, D))
    return X, groups


@functools.lru_cache(maxsize=None)
def pca_cases():
    out = []
    for D in (1, 2, 3, 15, 16, 17, 100, 255, 256):
        X = _rows(D, 257 if D <= 100 else 600, 1000 + D)
        nc = min(D, 32)
        for w in ((1, 0) if D in (17, 256) else (1,)):
            out.append(PcaCase(f"shapes_d{D}_w{w}", X, nc, w, _singles(X, nc)))
    for D, N in ((17, 10), (256, 2), (100, 100)):
        X = _rows(D, N, 2000 + D)
        nc = min(N, D)
        for w in (1, 0):
            out.append(PcaCase(f"rank_deficient_d{D}_n{N}_w{w}", X, nc, w, _singles(X, nc)))
    X, groups = _exact_spectrum(16, 200, 3000, False)
    out.append(PcaCase("degenerate", X, 16, 1, groups))
    X, groups = _exact_spectrum(17, 200, 3001, True)
    out.append(PcaCase("diagonal", X, 17, 1, groups))
    X = _rows(17, 257, 4000)
    X[:, 4], X[:, 11] = 2.5, 0.1
    out.append(PcaCase("constant_column", X, 17, 1, _singles(X, 17)))
    X = _rows(17, 257, 1017, offset=1e6)
    out.append(PcaCase("offset", X, 17, 1, _singles(X, 17)))
    return tuple(out)


def pca_case(name):
    return next(c for c in pca_cases() if c.name == name)


PCA_NAMES = ("shapes_d1_w1", "shapes_d2_w1", "shapes_d3_w1", "shapes_d15_w1", "shapes_d16_w1", "shapes_d17_w1", "shapes_d17_w0",
             "shapes_d100_w1", "shapes_d255_w1", "shapes_d256_w1", "shapes_d256_w0", "rank_deficient_d17_n10_w1",
             "rank_deficient_d17_n10_w0", "rank_deficient_d256_n2_w1", "rank_deficient_d256_n2_w0", "rank_deficient_d100_n100_w1",
             "rank_deficient_d100_n100_w0", "degenerate", "diagonal", "constant_column", "offset")


@functools.lru_cache(maxsize=None)
def pca_reference(name):
    """co.pca_svd of the case: the reference of every comparison (computed once, never written to)."""
    c = pca_case(name)
    with np.errstate(all="ignore"):        # zero eigenvalues: the oracle whitens by sqrt(0); those components are not compared
        Xr, p = co.pca_svd(c.X, c.n_components, bool(c.whiten))
    for a in (Xr, *p.values()):
        a.setflags(write=False)
    return Xr, p


def pca_figures(case, Xr, p, ref=None):
    """Every error figure of (Xr, p) against the case's reference (or ``ref``), each in the unit of its bound."""
    Xr0, p0 = pca_reference(case.name) if ref is None else ref
    lam = p0["explained_variance_"]
    l0 = lam[0] if lam[0] > 0 else 1.0
    V, V0 = p["components_"], p0["components_"]
    compared = [c for g in case.groups for c in g]
    null = [c for c in range(case.n_components) if c not in compared]
    f = {"mean": float(np.max(np.abs(p["mean_"] - p0["mean_"])) / max(1.0, float(np.max(np.abs(p0["mean_"]))))),
         "ev": float(np.max(np.abs(p["explained_variance_"] - lam)) / l0),
         "ratio": float(np.max(np.abs(p["explained_variance_ratio_"] - p0["explained_variance_ratio_"]))),
         "vec": 0.0, "sub": 0.0, "xr": 0.0, "sign_ok": True,
         "null_ev_ok": all(0.0 <= p["explained_variance_"][c] <= B_EV * l0 for c in null),
         "finite": bool(all(np.all(np.isfinite(a)) for a in (Xr, *p.values())))}
    for g in case.groups:
        g = list(g)
        if len(g) == 1:
            c = g[0]
            f["vec"] = max(f["vec"], float(1.0 - abs(V[c] @ V0[c])))
            f["sign_ok"] = f["sign_ok"] and bool(V[c, np.argmax(np.abs(V[c]))] > 0)
            want = Xr0[:, g]
        else:
            sv = np.linalg.svd(V[g] @ V0[g].T, compute_uv=False)
            f["sub"] = max(f["sub"], float(np.max(np.abs(sv - 1.0))))
            want = Xr0[:, g] @ (V0[g] @ V[g].T)       # the reference's coordinates in the other basis of the same subspace
        if case.whiten:
            if lam[g[-1]] >= WHITE_MIN * l0:
                f["xr"] = max(f["xr"], float(np.max(np.abs(Xr[:, g] - want))))
        else:
            f["xr"] = max(f["xr"], float(np.max(np.abs(Xr[:, g] - want)) / np.sqrt(l0)))
    return f


@functools.lru_cache(maxsize=None)
def pca_spread(name):
    """Figures of co.pca_longdouble against co.pca_svd on the case: how far two correct solvers lie apart."""
    c = pca_case(name)
    return pca_figures(c, *co.pca_longdouble(c.X, c.n_components, bool(c.whiten)))


def pca_bounds(case):
    b = {"mean": B_MEAN, "ev": B_EV, "ratio": B_RATIO, "vec": B_VEC, "sub": B_SUB, "xr": B_XR_WHITE if case.whiten else B_XR}
    keys = tuple(b) if case.name == "offset" else ("xr",) if case.name in SPREAD_XR else ()
    for k in keys:
        b[k] = max(b[k], 10.0 * pca_spread(case.name)[k])
    return b


def pca_check(case, f, what=""):
    """Print every figure next to its bound, then assert them all."""
    b = pca_bounds(case)
    print(f"{what}{case.name}: " + ", ".join(f"{k} {f[k]:.2e} (bound {b[k]:.2e})" for k in b)
          + f", sign {f['sign_ok']}, null ev {f['null_ev_ok']}, finite {f['finite']}")
    for k in b:
        assert f[k] <= b[k], (case.name, k, f[k], b[k])
    assert f["sign_ok"] and f["null_ev_ok"] and f["finite"], case.name


# ---- linkage -------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
MARGIN = 1e-6             # three orders above what fma-versus-sum ordering moves in fp64, one below the smallest measured gap


def _points(d, N):
    rng = np.random.default_rng(100 * d + N)
    return rng.normal(size=(N, d)) + 3.0 * rng.integers(0, 4, size=(N, 1))


GENERAL = tuple((d, N) for d in WIDTHS for N in (257, 513)) + tuple((d, N) for d in (3, 9) for N in (2, 3, 255, 256))
GENERAL_NAMES = tuple(f"d{d}_n{N}" for d, N in GENERAL)


@functools.lru_cache(maxsize=None)
def general(name):
    d, N = GENERAL[GENERAL_NAMES.index(name)]
    P = _points(d, N)
    P.setflags(write=False)
    return LinkCase(name, P)


@functools.lru_cache(maxsize=None)
def tree(name):
    """(Z, rounds, margin) of co.ward_rnn on a general case, computed once."""
    Z, rounds, gap = co.ward_rnn(general(name).points, margin=True)
    Z.setflags(write=False)
    return Z, rounds, gap


def tree_figures(Z, rounds, Zo, rounds_o):
    """(pairs and sizes identical, height error / largest height, rounds equal)"""
    same = bool(np.array_equal(Z[:, [0, 1, 3]], Zo[:, [0, 1, 3]]))
    return same, float(np.max(np.abs(Z[:, 2] - Zo[:, 2])) / Zo[:, 2].max()), rounds == rounds_o


def hierarchy(k, g=3, perm=None):
    """2^k points on a line, x_i = sum_b bit_b(i) g^b; ``perm`` (an index array) reorders them: point j is x[perm[j]]."""
    i = np.arange(1 << k)
    x = np.zeros(1 << k)
    for b in range(k):
        x += ((i >> b) & 1) * float(g) ** b
    if perm is not None:
        x = x[np.asarray(perm)]
    return x.reshape(-1, 1)


def hierarchy_heights(k, g=3):
    """Column 2 and 3 of the closed-form Z: N / 2^(b+1) rows of height sqrt(2^b) g^b and size 2^(b+1) for b = 0 .. k - 1."""
    h = np.concatenate([np.full(1 << (k - 1 - b), np.sqrt(2.0 ** b) * float(g) ** b) for b in range(k)])
    s = np.concatenate([np.full(1 << (k - 1 - b), 2.0 ** (b + 1)) for b in range(k)])
    return h, s


def check_hierarchy_tree(Z, k, perm=None):
    """Assert that Z is the closed-form tree of hierarchy(k, perm=perm) in its structure: every row joins two sibling blocks (leaf
    ranges [2 a 2^b, (2 a + 1) 2^b) and [(2 a + 1) 2^b, (2 a + 2) 2^b)) of equal level b, the smaller id first.  Leaf range and
    level are recorded per node; rows are taken level by level (the closed form has N / 2^(b+1) rows of level b, in this order),
    so a row that uses a node of another level, or one not yet made, fails.  O(N), numpy only."""
    n = 1 << k
    Z = np.asarray(Z)
    assert Z.shape == (n - 1, 4)
    a, b = Z[:, 0].astype(np.int64), Z[:, 1].astype(np.int64)
    assert np.all(a == Z[:, 0]) and np.all(b == Z[:, 1]) and np.all((0 <= a) & (a < b) & (b < 2 * n - 1))
    lo, level = np.full(2 * n - 1, -1, np.int64), np.full(2 * n - 1, -1, np.int64)
    lo[:n] = np.arange(n) if perm is None else np.asarray(perm)
    level[:n] = 0
    r0 = 0
    for lv in range(k):
        r1 = r0 + (1 << (k - 1 - lv))
        ca, cb = a[r0:r1], b[r0:r1]
        assert np.all(level[ca] == lv) and np.all(level[cb] == lv), f"level {lv}: a child of another level"
        first, second = np.minimum(lo[ca], lo[cb]), np.maximum(lo[ca], lo[cb])
        assert np.all(first % (2 << lv) == 0) and np.all(second == first + (1 << lv)), f"level {lv}: not a sibling pair"
        lo[n + r0:n + r1], level[n + r0:n + r1] = first, lv + 1
        r0 = r1
    used = np.bincount(np.concatenate([a, b]), minlength=2 * n - 1)
    assert np.all(used[:2 * n - 2] == 1) and used[2 * n - 2] == 0, "a node is merged twice or never"
