"""The Gaussian-mixture EM fit on the MI355X (csrc/gmm_fit.hip through vssr_gmm_fit_*): every reference fixture through
backend.GMMFitEngine and uncertainty.GaussianMixture at the bound the fixtures record (tests/gmm_fit_oracle.py: max(16 x the
reference-vs-sklearn discrepancy, 1e-12) relative to max |reference|), one EM iteration of shapes beyond the fixtures against the
numpy restatement, bit-reproducibility, the seeded initialisers, the resident PaiNN embedding, and the error paths."""
import numpy as np
import pytest

import gmm_fit_oracle as fo
import gmm_oracle as go
from surface_sampling_amd import backend, uncertainty as U
from test_gpu_uncertainty import _engine, _structs

pytestmark = pytest.mark.gpu


def _engine_result(eng):
    r, p = eng.fit(), eng.params()
    return dict(p, n_iter_=r["n_iter"], converged_=r["converged"], lower_bound_=r["lower_bound"], lower_bounds_=r["lower_bounds"])


@pytest.mark.parametrize("name", fo.fixture_names())
def test_reference_fixtures(name):
    fx = fo.load_fixture(name)
    K, D = fx["K"], fx["X"].shape[1]
    kw = fo.init_kwargs(fx)
    eng = backend.GMMFitEngine(K, D, covariance_type=fx["cov_type"], tol=fx["tol"], reg_covar=fx["reg_covar"],
                               max_iter=fx["max_iter"], init="given")
    eng.append_rows(fx["X"])
    eng.set_init(means=kw.get("means_init"), weights=kw.get("weights_init"), precisions=kw.get("precisions_init"),
                 labels=kw.get("labels"))
    gm = U.GaussianMixture(K, covariance_type=fx["cov_type"], tol=fx["tol"], reg_covar=fx["reg_covar"], max_iter=fx["max_iter"],
                           means_init=kw.get("means_init"), weights_init=kw.get("weights_init"),
                           precisions_init=kw.get("precisions_init"), device="cuda:0")
    if fx["raises"]:
        with pytest.raises(ValueError, match="ill-defined empirical covariance.*decrease the number of components, or increase reg_covar"):
            eng.fit()
        with pytest.raises(ValueError, match=fo.ILL_DEFINED):
            gm.fit(fx["X"], labels=kw.get("labels"))
        eng.close()
        return
    fo.check(fx, _engine_result(eng), f"{name} engine")
    eng.close()
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(fx["X"], labels=kw.get("labels"))
    fo.check(fx, {k: getattr(gm, k) for k in fo.COMPARED + ("n_iter_", "converged_")}, f"{name} GaussianMixture")
    assert gm.lower_bound_ == gm.lower_bounds_[-1]
    # score_samples of the fitted estimator (the scorer built from the device arrays) against the restatement
    P = go.expand(fx["precisions_cholesky_"], fx["cov_type"], K, D)
    want = -go.nll(fx["X"][:200], fx["means_"], P, fx["weights_"], go.LOG2PI_F64)
    assert np.max(np.abs(gm.score_samples(fx["X"][:200]) - want) / (1 + np.abs(want))) <= 1e-9


def _random_start(K, D, cov, seed):
    means, pc, w = go.random_gmm(K, D, cov, seed=seed)
    if cov == "full":
        prec = np.einsum("kij,klj->kil", pc, pc)
    elif cov == "tied":
        prec = pc @ pc.T
    else:
        prec = pc ** 2
    return means, w, prec


# bound of one EM iteration against the numpy restatement.  Both sides evaluate the same formulas in fp64; they differ in summation
# order over N rows and D columns.  A sum of n terms carries a relative rounding error of at most about n eps; the centred covariance
# and its Cholesky inverse amplify it by the condition number of S_k, which these well-populated random shapes (n_k >= 4 D rows of
# unit-scale noise, reg_covar 1e-6) keep below ~1e3: 2000 rows x 256 columns x 2.2e-16 x 1e3 ~ 1e-7 is the worst case, and the
# typical error is its square root.  1e-8 relative to the array's max |.| sits between the two.
ONE_ITER_REL = 1e-8


@pytest.mark.parametrize("cov", ["full", "tied", "diag", "spherical"])
@pytest.mark.parametrize("K,D,N", [(1, 1, 37), (16, 16, 1000), (3, 100, 1999), (64, 16, 5000), (2, 256, 2300), (1, 100, 50)])
def test_one_em_iteration_beyond_the_fixtures(cov, K, D, N):
    if cov in ("full", "tied") and N < 4 * D:
        N = 4 * D + 3   # the matrix types need a positive definite covariance
    rng = np.random.default_rng(K * 100 + D)
    means, w, prec = _random_start(K, D, cov, seed=K + D)
    X = (means[rng.integers(0, K, N)] + rng.normal(size=(N, D))).astype(np.float32).astype(np.float64)
    eng = backend.GMMFitEngine(K, D, covariance_type=cov, tol=0.0, reg_covar=1e-6, max_iter=1, init="given")
    eng.append_rows(X[: N // 2])
    eng.append_rows(X[N // 2:])      # two appends: the resident rows are kept when the buffer grows
    eng.set_init(means=means, weights=w, precisions=prec)
    got = _engine_result(eng)
    eng.close()
    lb, w1, m1, cov1, pc1 = fo.em_iteration(X, w, means, fo.init_precision_cholesky(prec, cov), cov, 1e-6)
    assert got["n_iter_"] == 1 and not got["converged_"]
    for key, want in (("lower_bounds_", np.array([lb])), ("weights_", w1), ("means_", m1), ("covariances_", cov1),
                      ("precisions_cholesky_", pc1)):
        err = float(np.max(np.abs(got[key] - want))) / float(np.max(np.abs(want)))
        print(f"{cov} K={K} D={D} N={N} {key}: relative error {err:.3e}")
        assert err <= ONE_ITER_REL, (key, err)


def test_two_runs_are_bit_identical():
    fx = fo.load_fixture("full_d64_k3_labels")
    out = []
    for _ in range(2):
        eng = backend.GMMFitEngine(3, 64, tol=fx["tol"], max_iter=fx["max_iter"], init="given")
        eng.append_rows(fx["X"])
        eng.set_init(labels=fx["labels"])
        out.append(_engine_result(eng))
        eng.close()
    for key in fo.COMPARED:
        assert np.array_equal(out[0][key], out[1][key]), key


def _separated(K=4, D=12, n_per=400, seed=0):
    rng = np.random.default_rng(seed)
    centres = 12.0 * rng.normal(size=(K, D))
    labels = np.repeat(np.arange(K), n_per)
    X = centres[labels] + rng.normal(size=(K * n_per, D))
    perm = rng.permutation(len(X))
    return X[perm].astype(np.float32).astype(np.float64), labels[perm]


@pytest.mark.parametrize("init", ["kmeans", "random_from_data"])
def test_seeded_initialisers(init):
    X, labels = _separated()
    K, D = 4, X.shape[1]

    def run(seed):
        eng = backend.GMMFitEngine(K, D, tol=1e-6, max_iter=200, init=init, seed=seed, n_init=1 if init == "kmeans" else 8)
        eng.append_rows(X)
        r = _engine_result(eng)
        eng.close()
        return r

    a, b = run(7), run(7)
    for key in fo.COMPARED:
        assert np.array_equal(a[key], b[key]), key                      # same seed: identical result
    tr = a["lower_bounds_"]
    # EM never lowers the bound; rounding floor: the bound is a mean of N log-likelihoods of size |lb|, each exact to a few eps
    floor = 64 * np.finfo(np.float64).eps * float(np.max(np.abs(tr)))
    print(init, "trace steps min", float(np.diff(tr).min()) if len(tr) > 1 else 0.0, "floor", floor)
    assert np.all(np.diff(tr) >= -floor)
    eng = backend.GMMFitEngine(K, D, tol=1e-6, max_iter=200, init="given")
    eng.append_rows(X)
    eng.set_init(labels=labels)
    ref = _engine_result(eng)
    eng.close()
    # both fits stop when the bound moves by less than tol per iteration: they agree on the optimum within a few tol
    print(init, "lower bound", a["lower_bound_"], "from the true labels", ref["lower_bound_"])
    assert abs(a["lower_bound_"] - ref["lower_bound_"]) <= 10 * 1e-6


def test_resident_embedding_two_batches(golden):
    eng = _engine(golden)
    structs = _structs(golden, n_synth=4)
    half = len(structs) // 2
    K, D = 3, 128
    fit = backend.GMMFitEngine(K, D, tol=1e-3, reg_covar=1e-4, max_iter=4, init="given")
    rows, Zall = [], []
    for part in (structs[:half], structs[half:]):
        eng.evaluate(part)
        fit.append_batch(eng, model=1, rows="atoms")
        rows.append(eng.embedding(1).astype(np.float64))
        Zall.append(np.concatenate([s[0] for s in part]))
    X, Zall = np.concatenate(rows), np.concatenate(Zall)
    labels = np.searchsorted(np.unique(Zall), Zall).astype(np.int32)     # one component per species (O, Ti, Sr)
    assert fit.n_rows == len(X) and labels.max() == K - 1
    fit.set_init(labels=labels)
    got = _engine_result(fit)
    want = fo.fit(X, K, "full", tol=1e-3, reg_covar=1e-4, max_iter=4, labels=labels)
    assert got["n_iter_"] == want["n_iter_"] and got["converged_"] == want["converged_"]
    for key in fo.COMPARED:
        err = float(np.max(np.abs(got[key] - want[key]))) / float(np.max(np.abs(want[key])))
        print(f"resident fit {key}: relative error {err:.3e}")
        # embedding clusters are far worse conditioned than the random shapes above (reg_covar 1e-4 against variances of order 1):
        # the factor entries carry the condition number; the lower bound and the moments do not
        assert err <= (1e-6 if key == "precisions_cholesky_" else ONE_ITER_REL), (key, err)
    # scoring the resident batch with the handle built on the device == scoring with an engine built from the downloaded parameters
    sc = fit.scorer(go.LOG2PI_F32)
    p = fit.params()
    host = backend.GMMEngine(p["means_"], p["precisions_cholesky_"], p["weights_"], log_2pi=go.LOG2PI_F32)
    a, b = sc.score_batch(eng, model=1, rows="atoms", order="system_mean"), host.score_batch(eng, model=1, rows="atoms", order="system_mean")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the same through GMMUncertainty(fit_device=...)
    u = U.GMMUncertainty(n_clusters=K, tol=1e-3, max_iter=4, init_params="random_from_data", device="cuda:0", fit_device="cuda:0")
    u.random_state = 3
    u.fit_resident(eng, model=1)
    assert u.is_fitted() and u.means.shape == (K, D)
    nll, unc = u.score_resident(eng, model=1)
    assert np.all(np.isfinite(nll.numpy()))
    for x in (sc, host, fit, eng):
        x.close()


def test_error_paths_return_codes(golden):
    eng = _engine(golden)
    fit = backend.GMMFitEngine(2, 128)
    s = _structs(golden, n_synth=0)[:2]
    eng.upload(s)
    with pytest.raises(backend.BackendError, match="vssr error -5: no completed PaiNN run"):
        fit.append_batch(eng)
    eng.run()
    fit.append_batch(eng)
    small = backend.GMMFitEngine(2, 64)
    with pytest.raises(backend.BackendError, match="vssr error -1: GMM dimension 64 differs from the PaiNN feat_dim 128"):
        small.append_batch(eng)
    with pytest.raises(backend.BackendError, match="vssr error -5: GMM fit: no completed fit"):
        fit.params()
    with pytest.raises(backend.BackendError, match="init = given needs labels"):
        fit.fit()
    with pytest.raises(backend.BackendError, match="Gaussian-mixture fit handle"):
        backend.PainnEngine.run(fit)
    with pytest.raises(backend.BackendError, match="not a GMM handle"):
        fit._check(fit._lib.vssr_gmm_score_rows(fit._h, 1, None, None, None))
    with pytest.raises(backend.BackendError, match="not a GMM fit handle"):
        eng._check(eng._lib.vssr_gmm_fit_clear(eng._h))
    for x in (small, fit, eng):
        x.close()
