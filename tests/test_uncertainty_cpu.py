"""Gaussian-mixture / ensemble uncertainty on the host: the numpy path of surface_sampling_amd.uncertainty against the fp64
restatement (tests/gmm_oracle.py), the reference's quirks (float32 log 2 pi, zero padding of ragged batches), the restricted GMM
unpickler, the library's input checks of vssr_gmm_create (no device is touched), the ISA lint of csrc/gmm.hip and the launcher."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import gmm_oracle as go
from conftest import ROOT
from surface_sampling_amd import backend, launch, uncertainty as U


def _unc(gmm, cov="full", **kw):
    means, prec, w = gmm
    return U.GMMUncertainty(device="cpu", covariance_type=cov,
                            gm_model={"means_": means, "precisions_cholesky_": prec, "weights_": w, "covariance_type": cov}, **kw)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize("cov", ["full", "tied", "diag", "spherical"])
@pytest.mark.parametrize("order", go.ORDERS)
def test_cpu_path_matches_the_oracle_for_every_order(cov, order):
    K, D = 5, 24
    means, prec, w = go.random_gmm(K, D, cov, seed=3)
    P = go.expand(prec, cov, K, D)
    rng = np.random.default_rng(1)
    num_atoms = [7, 3, 11, 1]
    X = rng.normal(size=(sum(num_atoms), D)).astype(np.float32).astype(np.float64)   # (fp32 embeddings, scored in fp64)
    for umin, calibrate in ((None, False), (2.5, False), (1.5, True)):
        unc = _unc((means, prec, w), cov, order=order, min_uncertainty=umin, calibrate=calibrate, cp_alpha=0.1 if calibrate else None)
        qhat = None
        if calibrate:
            unc.CP.qhat = qhat = 1.7
        got = unc({"embedding": torch.from_numpy(X.astype(np.float32)).double()}, num_atoms=torch.tensor(num_atoms))
        want = go.uncertainty(X, (means, P, w), order, num_atoms, umin, qhat)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.device.type == "cpu"
        assert got.shape == np.shape(want)
        assert _rel(got.numpy(), want) <= 1e-13
    unc = _unc((means, prec, w), cov)
    lp = unc.estimate_log_prob(X).numpy()
    assert _rel(lp, go.log_prob(X, means, P, go.LOG2PI_F32)) <= 1e-13
    assert _rel(unc.estimate_weighted_log_prob(X).numpy(), lp + np.log(w)) <= 1e-13
    nll = go.nll(X, means, P, w, go.LOG2PI_F32)
    assert _rel(unc.log_likelihood(X).numpy(), -nll) <= 1e-13
    assert _rel(unc.negative_log_likelihood(X).numpy(), nll) <= 1e-13
    Y = 0.01 * X[:3]
    assert _rel(unc.probability(Y).numpy(), np.exp(-go.nll(Y, means, P, w, go.LOG2PI_F32))) <= 1e-12


def test_log2pi_is_the_float32_value_of_the_reference_expression():
    ref = torch.log(torch.tensor([2 * torch.pi]))   # GMMUncertainty.estimate_log_prob's constant
    assert ref.dtype == torch.float32
    assert U.LOG2PI_F32 == float(ref.item()) == 1.8378770351409912
    assert U.GMMUncertainty.log2pi == U.LOG2PI_F32
    assert U.LOG2PI_F64 == float(np.log(2 * np.pi)) and U.LOG2PI_F64 != U.LOG2PI_F32
    # D = 128: the two constants move the NLL by 0.5 D (F64 - F32), about 2.0e-6
    means, prec, w = go.random_gmm(2, 128, seed=4)
    X = np.random.default_rng(0).normal(size=(3, 128))
    a = _unc((means, prec, w)).negative_log_likelihood(X).numpy()
    u = _unc((means, prec, w))
    u.log2pi = U.LOG2PI_F64
    b = u.negative_log_likelihood(X).numpy()
    assert np.allclose(b - a, 64 * (U.LOG2PI_F64 - U.LOG2PI_F32), rtol=1e-6, atol=0)
    assert 1.9e-6 < float(np.mean(b - a)) < 2.1e-6


def test_get_system_val_pads_ragged_batches_with_zeros():
    val = torch.tensor([3.0, 4.0, 5.0, -2.0, -1.0, 6.0], dtype=torch.float64)   # structures of 3, 2, 1 rows
    n = [3, 2, 1]
    assert U.get_system_val(val, n, "system_max").tolist() == [5.0, 0.0, 6.0]        # -2, -1 padded: max(., 0) = 0
    assert U.get_system_val(val, n, "system_min").tolist() == [3.0, -2.0, 0.0]       # the longest is not padded; 6 is: min(6, 0)
    assert U.get_system_val(val, n, "system_mean").tolist() == [4.0, -1.5, 6.0]     # means are not affected
    assert U.get_system_val(val, n, "system_sum").tolist() == [12.0, -3.0, 6.0]
    assert torch.equal(U.get_system_val(val[:3], [1, 1, 1], "system_max"), val[:3])   # already per system: unchanged
    for order in go.ORDERS[1:]:
        got = U.get_system_val(val, n, order).numpy()
        assert np.allclose(got, go.system_val(val.numpy(), n, order), rtol=1e-15)
    # the device returns TRUE reductions; the Python layer turns them into the same values
    true_max, true_min = np.array([5.0, -1.0, 6.0]), np.array([3.0, -2.0, 6.0])
    assert U.apply_padding_rule(true_max, n, "system_max").tolist() == [5.0, 0.0, 6.0]
    assert U.apply_padding_rule(true_min, n, "system_min").tolist() == [3.0, -2.0, 0.0]


@pytest.mark.parametrize("order", ["atomic", "system_mean", "system_max"])
@pytest.mark.parametrize("std_or_var", ["std", "var"])
def test_ensemble_uncertainty_matches_the_oracle(order, std_or_var):
    rng = np.random.default_rng(2)
    n = [4, 2, 5]
    res = {"forces_std": rng.uniform(size=(sum(n), 3)).astype(np.float32), "energy_std": rng.uniform(size=3),
           "energy_var": rng.uniform(size=3)}
    for q in ("forces_std", "energy_std"):
        u = U.EnsembleUncertainty(q, order, std_or_var, min_uncertainty=0.1)
        got = u(res, num_atoms=n)
        assert got.dtype == torch.float64
        assert np.allclose(got.numpy(), go.ensemble(res, q, order, std_or_var, n, 0.1), rtol=1e-12, atol=0)


def test_conformal_prediction_quantile():
    cp = U.ConformalPrediction(alpha=0.1)
    r, h = np.linspace(1, 3, 19), np.full(19, 2.0)
    cp.fit(torch.from_numpy(r), torch.from_numpy(h))
    ref = torch.quantile(torch.from_numpy(np.abs(r / h)), float(np.ceil(20 * 0.9) / 19)).item()
    assert cp.qhat == pytest.approx(ref, rel=1e-15)
    assert cp.predict(2.0) == (2.0 * cp.qhat, cp.qhat)


def test_sklearn_score_samples_with_the_fp64_constant():
    sk = pytest.importorskip("sklearn.mixture")
    rng = np.random.default_rng(5)
    X = np.concatenate([rng.normal(loc=c, size=(60, 6)) for c in (-2.0, 0.0, 3.0)])
    Y = rng.normal(scale=2.0, size=(25, 6))
    for cov in ("full", "tied", "diag", "spherical"):
        gm = sk.GaussianMixture(n_components=3, covariance_type=cov, random_state=0).fit(X)
        u = U.GMMUncertainty(device="cpu", covariance_type=cov, gm_model=gm)
        u.log2pi = U.LOG2PI_F64
        assert _rel(u.negative_log_likelihood(Y).numpy(), -gm.score_samples(Y)) <= 1e-10
        assert _rel(u.estimate_log_prob(Y).numpy(), gm._estimate_log_prob(Y)) <= 1e-10
    # fit_gmm on the host (EM stays there), saved as arrays behind gmm_path
    u = U.GMMUncertainty(device="cpu", n_clusters=2, covariance_type="diag", max_iter=200)
    u.fit_gmm(torch.from_numpy(X))
    assert u.is_fitted() and u.means.shape == (2, 6)


# ---- pickles ----------------------------------------------------------------------------------------------------------------------
def _stand_in_reference(monkeypatch):
    """A stand-in for the reference's mcmc.uncertainty.gmm module with a GaussianMixture class whose instances pickle the way the
    reference's do (every fitted attribute in the instance dict)."""
    import types

    mods = {n: types.ModuleType(n) for n in ("mcmc", "mcmc.uncertainty", "mcmc.uncertainty.gmm")}

    class GaussianMixture:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    GaussianMixture.__module__ = "mcmc.uncertainty.gmm"
    GaussianMixture.__qualname__ = "GaussianMixture"
    mods["mcmc.uncertainty.gmm"].GaussianMixture = GaussianMixture
    for n, m in mods.items():
        monkeypatch.setitem(sys.modules, n, m)
    return GaussianMixture


def test_pickles_round_trip_and_foreign_globals_are_refused(tmp_path, monkeypatch):
    GM = _stand_in_reference(monkeypatch)
    means, prec, w = go.random_gmm(3, 8, "full", seed=7)
    gm = GM(n_components=3, covariance_type="full", means_=means, precisions_cholesky_=prec, weights_=w, tol=1e-3,
            converged_=True, n_iter_=12, lower_bound_=np.float64(-3.5), random_state=None)
    X = np.random.default_rng(0).normal(size=(9, 8))
    want = go.nll(X, means, prec, w, go.LOG2PI_F32)
    # a bare GaussianMixture.save pickle behind gmm_path
    bare = tmp_path / "gmm.pkl"
    bare.write_bytes(pickle.dumps(gm))
    u = U.GMMUncertainty(device="cpu", gmm_path=str(bare))
    assert isinstance(u.gm_model, U.GaussianMixtureParams) and not hasattr(u.gm_model, "tol")
    assert _rel(u.negative_log_likelihood(X).numpy(), want) <= 1e-13
    # an Uncertainty.save dict of the reference (calibrated, GMM object inside)
    ref = tmp_path / "unc.pkl"
    params = {"train_embed_key": "embedding", "test_embed_key": "embedding", "n_clusters": 3, "order": "system_mean",
              "covariance_type": "full", "tol": 1e-3, "max_iter": 100000, "n_init": 1, "verbose": 0, "calibrate": True,
              "cp_alpha": 0.05, "min_uncertainty": np.float64(0.25), "gm_model": gm, "qhat": 1.25}
    ref.write_bytes(pickle.dumps({"uncertainty_type": "gmm", "unc_params": params}))
    v = U.Uncertainty.load(str(ref))
    v.device = "cpu"
    assert isinstance(v, U.GMMUncertainty) and v.CP.qhat == 1.25 and v.umin == 0.25 and v.order == "system_mean"
    got = v({"embedding": X}, num_atoms=[4, 5])
    assert _rel(got.numpy(), go.uncertainty(X, (means, prec, w), "system_mean", [4, 5], 0.25, 1.25)) <= 1e-13
    # written here: same dict layout, GMM as arrays; reads back without the stand-in module
    mine = tmp_path / "mine.pkl"
    v.save(str(mine))
    monkeypatch.delitem(sys.modules, "mcmc.uncertainty.gmm")
    d = U.load_pickle(str(mine))
    assert set(d) == {"uncertainty_type", "unc_params"} and isinstance(d["unc_params"]["gm_model"], dict)
    w2 = U.Uncertainty.load(str(mine))
    w2.device = "cpu"
    assert torch.equal(w2({"embedding": X}, num_atoms=[4, 5]), got)
    # uncalibrated pickles load too
    e = tmp_path / "ens.pkl"
    U.EnsembleUncertainty("forces_std", "atomic", "std").save(str(e))
    assert isinstance(U.Uncertainty.load(str(e)), U.EnsembleUncertainty)

    # a pickle naming os.system is refused by name and never executed
    marker = tmp_path / "executed"

    class Evil:
        def __reduce__(self):
            return (os.system, (f"touch {marker}",))

    evil = tmp_path / "evil.pkl"
    evil.write_bytes(pickle.dumps({"uncertainty_type": "gmm", "unc_params": {"gm_model": Evil()}}))
    with pytest.raises(pickle.UnpicklingError, match="system"):
        U.Uncertainty.load(str(evil))
    with pytest.raises(pickle.UnpicklingError):
        U.GMMUncertainty(device="cpu", gmm_path=str(evil))
    assert not marker.exists()


# ---- library checks (no device is touched) ----------------------------------------------------------------------------------------
def _create(K, D, means=None, prec=None, w=None, log2pi=U.LOG2PI_F32):
    L = backend.load_library()
    means = np.zeros((max(K, 1), D)) if means is None else means
    prec = np.broadcast_to(np.eye(D), (max(K, 1), D, D)).copy() if prec is None else prec
    w = np.ones(max(K, 1)) if w is None else w
    cfg = backend.GmmConfig(C.sizeof(backend.GmmConfig), 0, K, D, backend._ptr(np.ascontiguousarray(means, np.float64), C.c_double),
                            backend._ptr(np.ascontiguousarray(prec, np.float64), C.c_double),
                            backend._ptr(np.ascontiguousarray(w, np.float64), C.c_double), log2pi)
    h = C.c_void_p()
    rc = L.vssr_gmm_create(C.byref(cfg), C.byref(h))
    assert not h, "a refused configuration must not return a handle"
    return rc, (L.vssr_last_error(None) or b"").decode()


def test_library_refuses_bad_mixtures_before_touching_a_device():
    rc, msg = _create(0, 4)
    assert rc == -1 and "n_components" in msg
    assert "1..256" in _create(257, 4)[1] and "1..256" in _create(2, 257)[1]
    bad = np.broadcast_to(np.eye(4), (2, 4, 4)).copy()
    bad[1, 2, 2] = 0.0
    rc, msg = _create(2, 4, prec=bad)
    assert rc == -1 and "diagonal entry 2" in msg and "component 1" in msg
    bad[1, 2, 2] = -1.0
    assert "not positive" in _create(2, 4, prec=bad)[1]
    nan = np.zeros((2, 4))
    nan[0, 1] = np.nan
    assert "non-finite mean" in _create(2, 4, means=nan)[1]
    inf = np.broadcast_to(np.eye(4), (2, 4, 4)).copy()
    inf[0, 0, 3] = np.inf
    assert "non-finite precision" in _create(2, 4, prec=inf)[1]
    assert "weight 1" in _create(2, 4, w=np.array([0.5, -0.1]))[1]
    assert "no positive weight" in _create(2, 4, w=np.zeros(2))[1]
    assert "log_2pi" in _create(2, 4, log2pi=float("nan"))[1]
    L = backend.load_library()
    assert L.vssr_gmm_score_rows(None, 1, None, None, None) == -1
    assert L.vssr_gmm_score_batch(None, None, 0, 0, 0, None, None) == -1


def test_full_expansion_of_every_covariance_type():
    K, D = 3, 5
    for cov in ("tied", "diag", "spherical"):
        means, prec, w = go.random_gmm(K, D, cov, seed=1)
        assert np.array_equal(U.full_precision_cholesky(prec, cov, K, D), go.expand(prec, cov, K, D))


def test_gmm_kernel_passes_the_isa_lint():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_mfma_loads.py"),
                        os.path.join(ROOT, "surface-sampling_amd", "csrc", "gmm.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 violations" in r.stdout and "dense MFMA pairs" in r.stdout


# ---- launcher ---------------------------------------------------------------------------------------------------------------------
def test_launcher_replaces_the_uncertainty_names_and_runs_without_them(tmp_path):
    pkg = tmp_path / "mcmc"
    (pkg / "calculators").mkdir(parents=True)
    (pkg / "uncertainty").mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "calculators" / "__init__.py").write_text("class EnsembleNFFSurface:\n    origin = 'reference'\n")
    (pkg / "uncertainty" / "uncertainty.py").write_text(textwrap.dedent("""
        class Uncertainty: pass
        class GMMUncertainty(Uncertainty): pass
        class EnsembleUncertainty(Uncertainty): pass
        class ConformalPrediction: pass
        def get_system_val(*a): return "reference"
    """))
    (pkg / "uncertainty" / "__init__.py").write_text("from .uncertainty import Uncertainty, EnsembleUncertainty, GMMUncertainty\n")
    script = tmp_path / "clustering.py"
    script.write_text(textwrap.dedent("""
        from mcmc.uncertainty import Uncertainty
        import mcmc.uncertainty.uncertainty as inner
        print("unc", Uncertainty.__module__, inner.GMMUncertainty.__module__, inner.get_system_val.__module__,
              inner.ConformalPrediction.__module__)
    """))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, str(tmp_path)]))
    r = subprocess.run([sys.executable, "-m", "surface_sampling_amd.launch", str(script)], env=env, capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "unc surface_sampling_amd.uncertainty surface_sampling_amd.uncertainty surface_sampling_amd.uncertainty " \
           "surface_sampling_amd.uncertainty" in r.stdout
    # without mcmc.uncertainty the launcher still runs the script
    import shutil

    shutil.rmtree(pkg / "uncertainty")
    script.write_text("print('ran')\n")
    r = subprocess.run([sys.executable, "-m", "surface_sampling_amd.launch", str(script)], env=env, capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and "ran" in r.stdout, r.stdout + r.stderr
    assert launch.install_uncertainty(package="no_such_package_here") == {}
