#!/usr/bin/env python3
"""Write the reference fixtures of the device Gaussian-mixture fit: tests/golden/gmm_fit_<case>.npz (+ _ref.npz for the large arrays).

Usage: make_gmm_fit_golden.py /path/to/reference/mcmc/uncertainty/gmm.py
Needs scikit-learn and scipy.  Every case is fitted with the reference's GaussianMixture (imported from the given file at generation
time; none of its text is stored) and with sklearn.mixture.GaussianMixture; the files hold data only: the rows (float16 values, so
the fp64 input is exact), the initial parameters or labels, the reference's fitted attributes, and per compared quantity the
reference-vs-sklearn discrepancy (max abs, relative to max |reference|) that sets the tolerance of the tests
(tests/gmm_fit_oracle.py: bound).  Asserted here: every fitted component keeps n_k >= 4 D, and at the stopping iteration |change| is
at least 10x away from tol on both sides (every earlier change is at least 2x tol, the unconverged case's changes 10x)."""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
COMPARED = ("weights_", "means_", "covariances_", "precisions_cholesky_", "lower_bounds_")

# name: cov_type, D, K, N, init ("params" | "labels"), tol, reg_covar, max_iter, seed
CASES = {
    "full_d20_k5_params": ("full", 20, 5, 2000, "params", 1e-3, 1e-6, 100, 1),
    "full_d64_k3_labels": ("full", 64, 3, 2000, "labels", 1e-3, 1e-6, 100, 2),
    "full_d128_k3_labels": ("full", 128, 3, 1800, "labels", 1e-3, 1e-6, 100, 3),
    "full_d20_k1_labels": ("full", 20, 1, 500, "labels", 1e-3, 1e-6, 100, 4),
    "tied_d20_k3_params": ("tied", 20, 3, 2000, "params", 1e-3, 1e-6, 100, 5),
    "diag_d64_k5_labels": ("diag", 64, 5, 2000, "labels", 1e-3, 1e-6, 100, 6),
    "spherical_d20_k3_labels": ("spherical", 20, 3, 2000, "labels", 1e-3, 1e-6, 100, 17),
    "full_d20_k5_maxiter": ("full", 20, 5, 2000, "params", 1e-9, 1e-6, 3, 8),
    "full_d20_k3_collapsed": ("full", 20, 3, 600, "collapsed", 1e-3, 0.0, 100, 9),
}


def make_case(cov, D, K, N, init, tol, reg, max_iter, seed):
    rng = np.random.default_rng(seed)
    centres = rng.normal(scale=1.5, size=(K, D))
    scales = rng.uniform(0.6, 1.4, size=(K, D))
    true = rng.integers(0, K, size=N)
    true[:K] = np.arange(K)
    mix = rng.normal(size=(K, D, D)) * 0.15
    X = centres[true] + np.einsum("nd,nde->ne", rng.normal(size=(N, D)) * scales[true], np.eye(D) + mix[true])
    X = X.astype(np.float16).astype(np.float64)
    kw = {}
    if init == "params":
        kw["means_init"] = centres + rng.normal(scale=0.7, size=(K, D))
        w = rng.uniform(0.5, 1.5, K)
        kw["weights_init"] = w / w.sum()
        if cov == "full":
            A = rng.normal(size=(K, D, D)) * 0.1
            kw["precisions_init"] = np.einsum("kij,klj->kil", A, A) + 0.5 * np.eye(D)
        elif cov == "tied":
            A = rng.normal(size=(D, D)) * 0.1
            kw["precisions_init"] = A @ A.T + 0.5 * np.eye(D)
        elif cov == "diag":
            kw["precisions_init"] = rng.uniform(0.3, 1.0, size=(K, D))
        else:
            kw["precisions_init"] = rng.uniform(0.3, 1.0, size=K)
    elif init == "labels":
        lab = true.copy()
        flip = rng.random(N) < 0.35   # noisy labels: the fit needs several iterations
        lab[flip] = rng.integers(0, K, size=int(flip.sum()))
        kw["labels"] = lab.astype(np.int32)
    else:   # a component without a single row and reg_covar = 0: its covariance is exactly zero
        kw["labels"] = (true % (K - 1)).astype(np.int32)
    return X, kw


def run(cls, X, cov, K, tol, reg, max_iter, kw):
    """Fit with ``cls``; label init is fed through the estimator's own _initialize (what it does with its k-means result)."""
    gm = cls(n_components=K, covariance_type=cov, tol=tol, reg_covar=reg, max_iter=max_iter, n_init=1,
             means_init=kw.get("means_init"), weights_init=kw.get("weights_init"), precisions_init=kw.get("precisions_init"))
    if "labels" in kw:
        resp = np.zeros((len(X), K))
        resp[np.arange(len(X)), kw["labels"]] = 1.0
        gm._initialize_parameters = lambda X_, random_state, xp=None: gm._initialize(X_, resp)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(X)
    return gm


def main(ref_path):
    from sklearn.mixture import GaussianMixture as SkGM

    spec = importlib.util.spec_from_file_location("reference_gmm", ref_path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    RefGM = mod.GaussianMixture
    for name, (cov, D, K, N, init, tol, reg, max_iter, seed) in CASES.items():
        X, kw = make_case(cov, D, K, N, init, tol, reg, max_iter, seed)
        small = {"X": X.astype(np.float16), "cov_type": np.array(cov), "K": K, "tol": tol, "reg_covar": reg, "max_iter": max_iter,
                 "raises": init == "collapsed"}
        small.update(kw)
        big = {}
        if init == "collapsed":
            for cls in (RefGM, SkGM):
                try:
                    run(cls, X, cov, K, tol, reg, max_iter, kw)
                except ValueError as e:
                    assert "ill-defined empirical covariance" in str(e)
                else:
                    raise AssertionError(f"{name}: {cls.__module__} did not raise")
        else:
            ref, sk = run(RefGM, X, cov, K, tol, reg, max_iter, kw), run(SkGM, X, cov, K, tol, reg, max_iter, kw)
            assert ref.n_iter_ == sk.n_iter_ and ref.converged_ == sk.converged_, name
            assert (N * ref.weights_).min() >= 4 * D, (name, N * ref.weights_, 4 * D)
            tr = np.array(ref.lower_bounds_)
            for t in (tr, np.array(sk.lower_bounds_)):
                ch = np.abs(np.diff(np.concatenate([[-np.inf], t])))
                if ref.converged_:
                    assert ch[-1] <= tol / 10 and (len(ch) < 2 or ch[:-1].min() >= 2 * tol), (name, ch, tol)
                else:
                    assert ch.min() >= 10 * tol, (name, ch, tol)
            for key in COMPARED:
                a, b = np.asarray(getattr(ref, key), dtype=np.float64), np.asarray(getattr(sk, key), dtype=np.float64)
                disc = float(np.max(np.abs(a - b)))
                (big if a.size > 4096 else small)[key] = a
                small["disc_" + key] = np.array([disc, disc / float(np.max(np.abs(a)))])
            small.update({"n_iter_": ref.n_iter_, "converged_": ref.converged_, "lower_bound_": ref.lower_bound_})
            print(name, "n_iter", ref.n_iter_, "converged", ref.converged_, "min n_k", (N * ref.weights_).min(),
                  {k: small["disc_" + k][1] for k in COMPARED})
        np.savez(os.path.join(GOLDEN, f"gmm_fit_{name}.npz"), **small)
        if big:
            np.savez(os.path.join(GOLDEN, f"gmm_fit_{name}_ref.npz"), **big)


if __name__ == "__main__":
    main(sys.argv[1])
