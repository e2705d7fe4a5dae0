"""The Gaussian-mixture fit without a GPU: the numpy restatement (tests/gmm_fit_oracle.py) reproduces every reference fixture within
the bound the fixtures record, the library's argument checks of vssr_gmm_fit_* (no device is touched), the refusal of fit handles by
the other entry points, pickling of uncertainty.GaussianMixture through load_pickle, the unchanged host path of
GMMUncertainty.fit_gmm, and the ISA lint of csrc/gmm_fit.hip."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gmm_fit_oracle as fo
import gmm_oracle as go
from conftest import ROOT
from surface_sampling_amd import backend, uncertainty as U


def test_fixture_set_covers_what_the_fit_supports():
    names = fo.fixture_names()
    fxs = [fo.load_fixture(n) for n in names]
    assert {f["cov_type"] for f in fxs} == {"full", "tied", "diag", "spherical"}
    assert {20, 64, 128} <= {f["X"].shape[1] for f in fxs} and {1, 3, 5} <= {f["K"] for f in fxs}
    assert any("labels" in f for f in fxs) and any("precisions_init" in f for f in fxs)
    assert any(not f["raises"] and not f["converged_"] for f in fxs) and any(f["raises"] for f in fxs)
    for n in names:
        for suffix in ("", "_ref"):
            p = os.path.join(fo.GOLDEN, f"gmm_fit_{n}{suffix}.npz")
            assert not os.path.exists(p) or os.path.getsize(p) < 1 << 20


@pytest.mark.parametrize("name", fo.fixture_names())
def test_restatement_reproduces_the_reference(name):
    fx = fo.load_fixture(name)
    args = dict(K=fx["K"], cov_type=fx["cov_type"], tol=fx["tol"], reg_covar=fx["reg_covar"], max_iter=fx["max_iter"], **fo.init_kwargs(fx))
    if fx["raises"]:
        with pytest.raises(ValueError, match=fo.ILL_DEFINED):
            fo.fit(fx["X"], **args)
        return
    fo.check(fx, fo.fit(fx["X"], **args), name)


# ---- library checks (no device is touched) ----------------------------------------------------------------------------------------
def _create(K=2, D=4, cov=0, max_iter=10, n_init=1, init=0, tol=1e-3, reg=1e-6, size=None):
    L = backend.load_library()
    cfg = backend.GmmFitConfig(C.sizeof(backend.GmmFitConfig) if size is None else size, 0, K, D, cov, max_iter, n_init, init, tol,
                               reg, 0)
    h = C.c_void_p()
    rc = L.vssr_gmm_fit_create(C.byref(cfg), C.byref(h))
    return rc, (L.vssr_last_error(h if h else None) or b"").decode(), h


def test_create_refuses_bad_configurations_without_a_device():
    for kw, word in ((dict(K=0), "n_components"), (dict(K=257), "1..256"), (dict(D=0), "1..256"), (dict(D=257), "1..256"),
                     (dict(cov=4), "covariance_type"), (dict(init=3), "init"), (dict(tol=-1e-9), "tol"),
                     (dict(tol=float("nan")), "tol"), (dict(reg=-1.0), "reg_covar"), (dict(max_iter=0), "max_iter"),
                     (dict(n_init=0), "n_init"), (dict(size=8), "size mismatch")):
        rc, msg, h = _create(**kw)
        assert rc == -1 and word in msg and not h, (kw, msg)
    L = backend.load_library()
    assert L.vssr_gmm_fit_create(None, None) == -1


def test_rows_and_initial_values_are_checked_without_a_device():
    L = backend.load_library()
    rc, _, h = _create(K=2, D=4)
    assert rc == 0 and h
    err = lambda: L.vssr_last_error(h).decode()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    good = np.zeros((3, 4))
    assert L.vssr_gmm_fit_append_rows(h, 0, dp(good)) == -1 and L.vssr_gmm_fit_append_rows(h, 3, None) == -1
    bad = good.copy()
    bad[2, 1] = np.inf
    assert L.vssr_gmm_fit_append_rows(h, 3, dp(bad)) == -1 and "row 2" in err()
    nan = np.full((2, 4), np.nan)
    assert L.vssr_gmm_fit_set_init(h, dp(nan), None, None, None) == -1 and "mean" in err()
    assert L.vssr_gmm_fit_set_init(h, None, dp(np.array([0.5, -0.5])), None, None) == -1 and "weight 1" in err()
    assert L.vssr_gmm_fit_set_init(h, None, dp(np.zeros(2)), None, None) == -1
    notpd = np.stack([np.eye(4), -np.eye(4)])
    assert L.vssr_gmm_fit_set_init(h, None, None, dp(notpd), None) == -1 and "component 1 is not positive definite" in err()
    assert L.vssr_gmm_fit_set_init(h, dp(np.zeros((2, 4))), dp(np.array([0.5, 0.5])), dp(np.stack([np.eye(4)] * 2)), None) == 0
    # nothing resident: N < 2 is refused before a device is looked for; fitted state is required by params / scorer
    assert L.vssr_gmm_fit_run(h, None) == -1 and "at least 2 rows" in err()
    assert L.vssr_gmm_fit_params(h, None, None, None, None) == -5
    g = C.c_void_p()
    assert L.vssr_gmm_fit_scorer(h, 1.8, C.byref(g)) == -5 and not g
    assert L.vssr_gmm_fit_clear(h) == 0
    L.vssr_destroy(h)
    for f in (L.vssr_gmm_fit_clear, ):
        assert f(None) == -1
    assert L.vssr_gmm_fit_run(None, None) == -1 and L.vssr_gmm_fit_append_batch(None, None, 0, 0) == -1


def test_fit_handles_are_refused_by_the_other_entry_points():
    L = backend.load_library()
    rc, _, h = _create()
    assert rc == 0
    assert L.vssr_batch_run(h, 1) == -1 and b"fit handle serves the vssr_gmm_fit_* calls only" in L.vssr_last_error(h)
    assert L.vssr_synchronize(h) == -1
    assert L.vssr_gmm_score_rows(h, 1, None, None, None) == -1 and b"not a GMM handle" in L.vssr_last_error(h)
    assert L.vssr_gmm_score_batch(h, h, 0, 0, 0, None, None) == -1
    assert L.vssr_abi_version() == 1
    L.vssr_destroy(h)


def test_estimator_arguments_and_pickle_round_trip(tmp_path):
    with pytest.raises(NotImplementedError, match="host"):
        U.GaussianMixture(2, init_params="random").new_engine(4)
    with pytest.raises(NotImplementedError):
        U.GaussianMixture(2, init_params="k-means++").new_engine(4)
    with pytest.raises(ValueError, match="covariance_type"):
        U.GaussianMixture(2, covariance_type="banded").new_engine(4)
    fx = fo.load_fixture("tied_d20_k3_params")
    gm = U.GaussianMixture.from_dict({k: fx[k] for k in ("weights_", "means_", "covariances_", "precisions_cholesky_")}
                                     | {"covariance_type": "tied", "converged_": True, "n_iter_": fx["n_iter_"],
                                        "lower_bound_": float(fx["lower_bounds_"][-1]), "lower_bounds_": fx["lower_bounds_"]})
    assert gm.n_components == 3 and np.allclose(gm.precisions_, fx["precisions_cholesky_"] @ fx["precisions_cholesky_"].T)
    assert gm._n_parameters() == 20 * 21 // 2 + 3 * 20 + 2
    path = tmp_path / "gm.pkl"
    gm.save(str(path))
    d = U.load_pickle(str(path))
    assert isinstance(d, dict) and d["covariance_type"] == "tied" and np.array_equal(d["means_"], fx["means_"])
    # accepted wherever gm_model= is, as the object and as the saved dict
    X = fx["X"][:50]
    want = go.nll(X, fx["means_"], go.expand(fx["precisions_cholesky_"], "tied", 3, 20), fx["weights_"], go.LOG2PI_F32)
    for model in (gm, d):
        u = U.GMMUncertainty(device="cpu", covariance_type="tied", gm_model=model)
        assert np.max(np.abs(u.negative_log_likelihood(X).numpy() - want)) <= 1e-12 * np.max(np.abs(want))
    u = U.GMMUncertainty(device="cpu", gmm_path=str(path))
    assert np.max(np.abs(u.negative_log_likelihood(X).numpy() - want)) <= 1e-12 * np.max(np.abs(want))
    unc = tmp_path / "unc.pkl"
    U.GMMUncertainty(device="cpu", covariance_type="tied", gm_model=gm).save(str(unc))
    assert isinstance(U.load_pickle(str(unc))["unc_params"]["gm_model"], dict)


def test_fit_gmm_without_fit_device_still_runs_scikit_learn(monkeypatch):
    sk = pytest.importorskip("sklearn.mixture")
    calls = []
    orig = sk.GaussianMixture.fit

    def spy(self, X, y=None):
        calls.append(X.shape)
        return orig(self, X, y)

    monkeypatch.setattr(sk.GaussianMixture, "fit", spy)
    rng = np.random.default_rng(5)
    X = np.concatenate([rng.normal(loc=c, size=(60, 6)) for c in (-2.0, 3.0)])
    u = U.GMMUncertainty(device="cpu", n_clusters=2, covariance_type="diag", max_iter=200)
    assert u.fit_device is None
    u.fit_gmm(X)
    assert calls == [(120, 6)] and isinstance(u.gm_model, sk.GaussianMixture) and u.means.shape == (2, 6)
    with pytest.raises(ValueError, match="fit_device"):
        u._device_estimator()


def test_gmm_fit_kernels_pass_the_isa_lint():
    src = os.path.join(ROOT, "surface-sampling_amd", "csrc", "gmm_fit.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_mfma_loads.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 violations" in r.stdout
    text = open(src).read()
    assert "atomicAdd" not in text and "atomic_add" not in text   # the fixed-order promise: no floating-point atomics
    assert "mfma_f64_16x16x4f64" in text
