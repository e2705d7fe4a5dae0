"""Uncertainty of PaiNN predictions: the reference's ``mcmc.uncertainty`` (``mcmc/uncertainty/uncertainty.py``) with the
Gaussian-mixture scoring on the GPU.

Names and signatures follow the reference: ``Uncertainty`` (``load`` / ``save``), ``GMMUncertainty``, ``EnsembleUncertainty``,
``ConformalPrediction`` and ``get_system_val`` (``mcmc/uncertainty/prediction.py:181-223``).  Results are ``torch.float64`` CPU
tensors (``scripts/clustering.py`` calls ``.item()`` on them); inputs may be numpy arrays or torch tensors.

``GMMUncertainty(device="cpu")`` scores on the host in numpy fp64; ``device="cuda"`` / ``"cuda:n"`` on GPU n through
``backend.GMMEngine`` (``csrc/gmm.hip``), also fp64.  What the reference computes, and what is kept of it:

* the Gaussian normaliser uses ``LOG2PI_F32`` -- ``torch.log(torch.tensor([2 * torch.pi]))``, a float32 value -- as the reference's
  ``GMMUncertainty`` does (sklearn and ``gmm.py`` use the fp64 value ``LOG2PI_F64``; set ``log2pi`` on an instance to get theirs);
* the reference evaluates every covariance type with the ``full`` formula, which raises or is wrong for ``tied`` / ``diag`` /
  ``spherical``.  Here those are expanded to per-component full precision Cholesky factors (``full_precision_cholesky``) and scored
  with the correct formula of ``gmm.py::_estimate_log_gaussian_prob``;
* ``get_system_val`` pads the per-atom values of a ragged batch with zeros before ``max`` / ``min``, so a structure shorter than the
  longest one in the call gets ``max(., 0)`` / ``min(., 0)``; reproduced;
* the reference stores the squared distances in a float32 tensor (``torch.empty`` default dtype) and adds the constant in float32;
  here they stay fp64 (the values agree to float32 precision);
* ``Uncertainty.load`` of a pickle saved with ``calibrate=False`` raises ``AttributeError`` in the reference (it reads ``CP.qhat``,
  which only calibrated instances have); here it loads.

GMM pickles are read with a restricted unpickler (``load_pickle``): numpy arrays and the ``GaussianMixture`` classes of the reference
(``mcmc.uncertainty.gmm``) and of sklearn (``sklearn.mixture``), which map to ``GaussianMixtureParams`` (``means_``,
``precisions_cholesky_``, ``weights_``, ``covariance_type``); every other global is refused by name without being called.  Pickles
written here (``Uncertainty.save``, ``GMMUncertainty.fit_gmm`` with ``gmm_path``) keep the reference's dict layout but store the GMM
as a dict of numpy arrays: the reference cannot read them.
"""

from __future__ import annotations

import io
import os
import pickle
import warnings

import numpy as np

LOG2PI_F32 = 1.8378770351409912   # torch.log(torch.tensor([2 * torch.pi])).item(): what GMMUncertainty uses
LOG2PI_F64 = 1.8378770664093453   # np.log(2 * np.pi): sklearn / gmm.py

ORDERS = ("atomic", "system_sum", "system_mean", "system_max", "system_min", "system_mean_squared", "system_root_mean_squared")


def _torch():
    import torch

    return torch


def _to_numpy(x) -> np.ndarray:
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _tensor(x):
    """fp64 CPU torch tensor of a numpy value (0-dim values stay 0-dim)."""
    return _torch().from_numpy(np.array(x, dtype=np.float64, copy=True))


# ---- restricted unpickling -------------------------------------------------------------------------------------------------------
class GaussianMixtureParams:
    """Stand-in for a pickled ``GaussianMixture`` (the reference's ``mcmc.uncertainty.gmm`` or sklearn's): keeps the fitted
    parameters that scoring needs and nothing else."""

    KEEP = ("means_", "precisions_cholesky_", "weights_", "covariance_type")

    def __init__(self, means_=None, precisions_cholesky_=None, weights_=None, covariance_type="full"):
        self.means_, self.precisions_cholesky_, self.weights_ = means_, precisions_cholesky_, weights_
        self.covariance_type = covariance_type

    def __setstate__(self, state):
        if not isinstance(state, dict):
            raise pickle.UnpicklingError("unexpected GaussianMixture state")
        self.__init__(**{k: state[k] for k in self.KEEP if k in state})

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k in self.KEEP}


_NUMPY_GLOBALS = {
    ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
    ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
    ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
}
_GMM_MODULES = ("mcmc.uncertainty.gmm", "sklearn.mixture")


class _RestrictedUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if (module, name) in _NUMPY_GLOBALS:
            return getattr(__import__(module, fromlist=[name]), name)
        if name == "GaussianMixture" and any(module == m or module.startswith(m + ".") for m in _GMM_MODULES):
            return GaussianMixtureParams
        raise pickle.UnpicklingError(f"refused global {module}.{name} in a GMM pickle")


def load_pickle(path_or_bytes):
    """Unpickle a GMM / uncertainty pickle with the restricted unpickler (module docstring)."""
    if isinstance(path_or_bytes, (bytes, bytearray)):
        return _RestrictedUnpickler(io.BytesIO(path_or_bytes)).load()
    with open(path_or_bytes, "rb") as fh:
        return _RestrictedUnpickler(fh).load()


def _gmm_arrays(gm) -> dict:
    """means_, precisions_cholesky_, weights_, covariance_type of a GaussianMixture-like object or of a dict of them."""
    get = gm.get if isinstance(gm, dict) else (lambda k, d=None: getattr(gm, k, d))
    out = {k: get(k) for k in ("means_", "precisions_cholesky_", "weights_")}
    if any(v is None for v in out.values()):
        raise ValueError("the GMM has no fitted means_ / precisions_cholesky_ / weights_")
    out = {k: np.asarray(_to_numpy(v), dtype=np.float64) for k, v in out.items()}
    out["covariance_type"] = get("covariance_type", "full") or "full"
    return out


def full_precision_cholesky(prec_chol, covariance_type: str, n_components: int, n_features: int) -> np.ndarray:
    """Per-component full precision Cholesky factors [K, D, D] of any sklearn covariance type (``full``: as given; ``tied``: the
    one [D, D] factor for every component; ``diag``: diag(prec_chol[k]); ``spherical``: prec_chol[k] I)."""
    P = np.asarray(prec_chol, dtype=np.float64)
    K, D = n_components, n_features
    if covariance_type == "full":
        return np.ascontiguousarray(P.reshape(K, D, D))
    if covariance_type == "tied":
        return np.ascontiguousarray(np.broadcast_to(P.reshape(D, D), (K, D, D)))
    if covariance_type == "diag":
        d = P.reshape(K, D)
        out = np.zeros((K, D, D))
        out[:, np.arange(D), np.arange(D)] = d
        return out
    if covariance_type == "spherical":
        return np.ascontiguousarray(np.eye(D)[None] * P.reshape(K, 1, 1))
    raise ValueError(f"unknown covariance_type {covariance_type!r}")


# ---- per-structure reductions ----------------------------------------------------------------------------------------------------
def _system_from_rows(val: np.ndarray, num_atoms, order: str) -> np.ndarray:
    """The reference's ``get_system_val`` on per-row values (numpy fp64; the zero padding included)."""
    n = [int(a) for a in num_atoms]
    max_len = max(n)
    padded = np.zeros((len(n), max_len))
    mask = np.zeros((len(n), max_len), bool)
    o = 0
    for b, c in enumerate(n):
        padded[b, :c] = val[o:o + c]
        mask[b, :c] = True
        o += c
    cnt = mask.sum(axis=-1)
    if order == "system_sum":
        out = padded.sum(axis=-1)
    elif order == "system_max":
        out = padded.max(axis=-1)
    elif order == "system_min":
        out = padded.min(axis=-1)
    elif order == "system_mean":
        out = padded.sum(axis=-1) / cnt
    elif order == "system_mean_squared":
        out = (padded ** 2).sum(axis=-1) / cnt
    elif order == "system_root_mean_squared":
        out = ((padded ** 2).sum(axis=-1) / cnt) ** 0.5
    else:
        raise ValueError(f"{order} is not a system order")
    return out.squeeze()


def apply_padding_rule(system: np.ndarray, num_atoms, order: str) -> np.ndarray:
    """TRUE per-structure reductions (what the device returns) -> what ``get_system_val`` returns for the same batch: a structure
    shorter than the longest one sees the padding zeros in ``max`` / ``min``."""
    system = np.asarray(system, dtype=np.float64).copy()
    n = np.asarray([int(a) for a in num_atoms])
    short = n < n.max()
    if order == "system_max":
        system[short] = np.maximum(system[short], 0.0)
    elif order == "system_min":
        system[short] = np.minimum(system[short], 0.0)
    return system.squeeze()


def get_system_val(val, num_atoms, order: str):
    """Reference ``get_system_val`` (``mcmc/uncertainty/prediction.py:181-223``): per-atom values -> per-structure values in the
    ``order`` named; values already per structure (``len(val) == len(num_atoms)``) are returned unchanged."""
    if len(val) == len(num_atoms):
        return val
    return _tensor(_system_from_rows(np.asarray(_to_numpy(val), dtype=np.float64).reshape(-1), _to_numpy(num_atoms).reshape(-1),
                                     order))


# ---- conformal prediction, base class ----------------------------------------------------------------------------------------------
class ConformalPrediction:
    """Quantile of |residual / heuristic uncertainty| on calibration data (reference ``:139-166``)."""

    def __init__(self, alpha: float):
        self.alpha = alpha
        self.qhat = None

    def fit(self, residuals_calib, heuristic_uncertainty_calib) -> None:
        scores = np.abs(np.asarray(_to_numpy(residuals_calib), dtype=np.float64)
                        / np.asarray(_to_numpy(heuristic_uncertainty_calib), dtype=np.float64))
        n = len(scores)
        self.qhat = float(np.quantile(scores, np.ceil((n + 1) * (1 - self.alpha)) / n))   # (torch.quantile: linear, as numpy)

    def predict(self, heuristic_uncertainty_test):
        return heuristic_uncertainty_test * self.qhat, self.qhat


class Uncertainty:
    """Base class (reference ``:11-136``)."""

    def __init__(self, order: str, calibrate: bool, cp_alpha: float | None = 0.05, min_uncertainty: float | None = None,
                 *args, **kwargs):
        assert order in ORDERS, f"{order} not implemented"
        self.order = order
        self.calibrate = calibrate
        self.umin = min_uncertainty
        self.cp_alpha = cp_alpha
        if self.calibrate:
            assert cp_alpha is not None, "cp_alpha must be specified for calibration"
            self.CP = ConformalPrediction(alpha=cp_alpha)

    def __call__(self, *args, **kwargs):
        return self.get_uncertainty(*args, **kwargs)

    def set_min_uncertainty(self, uncertainty, force=False):
        if self.umin is None:
            self.umin = uncertainty
        elif force:
            warnings.warn(f"Uncertainty: min_uncertainty already set to {self.umin}. Overwriting.")
            self.umin = uncertainty
        else:
            raise Exception(f"Uncertainty: min_uncertainty already set to {self.umin}")

    def scale_to_min_uncertainty(self, uncertainty):
        if self.umin is not None:
            uncertainty = uncertainty - (self.umin ** 2 if self.order == "system_mean_squared" else self.umin)
        return uncertainty

    def fit_conformal_prediction(self, residuals_calib, heuristic_uncertainty_calib) -> None:
        self.CP.fit(residuals_calib, heuristic_uncertainty_calib)

    def calibrate_uncertainty(self, uncertainty, *args, **kwargs):
        if self.CP.qhat is None:
            raise Exception("Uncertainty: ConformalPrediction not fitted.")
        cp_uncertainty, _ = self.CP.predict(uncertainty)
        return cp_uncertainty

    def get_uncertainty(self, results, *args, **kwargs):
        return NotImplementedError

    def get_input_params(self):
        return NotImplementedError

    def save(self, path):
        unc_type, inputs = self.get_input_params()
        with open(path, "wb") as fh:
            pickle.dump({"uncertainty_type": unc_type, "unc_params": inputs}, fh)

    @classmethod
    def load(cls, path):
        info = load_pickle(path)
        if not isinstance(info, dict) or "uncertainty_type" not in info:
            raise ValueError(f"{path} is not an Uncertainty.save pickle")
        params = dict(info["unc_params"])
        qhat = params.pop("qhat", None)
        unc = UNC_DICT[info["uncertainty_type"]](**params)
        if params.get("calibrate"):
            unc.CP.qhat = qhat
        return unc


class EnsembleUncertainty(Uncertainty):
    """Variance or standard deviation of the ensemble's predictions (reference ``:169-260``), numpy fp64."""

    def __init__(self, quantity: str, order: str, std_or_var: str = "var", min_uncertainty: float | None = None, *args, **kwargs):
        super().__init__(order=order, min_uncertainty=min_uncertainty, calibrate=False, *args, **kwargs)
        assert std_or_var in ["std", "var"], f"{std_or_var} not implemented"
        self.q = quantity
        self.std_or_var = std_or_var

    def get_energy_uncertainty(self, results: dict):
        if self.std_or_var == "std":
            return np.asarray(_to_numpy(results["energy_std"]), dtype=np.float64)
        return np.asarray(_to_numpy(results["energy_var"]), dtype=np.float64) ** 2   # (the reference's key and square)

    def get_forces_uncertainty(self, results: dict, num_atoms: list):
        fs = np.asarray(_to_numpy(results["forces_std"]), dtype=np.float64)
        val = np.linalg.norm(fs if self.std_or_var == "std" else fs ** 2, axis=-1)
        if "system" in self.order:
            return np.asarray(_to_numpy(get_system_val(val, _to_numpy(num_atoms), self.order)), dtype=np.float64)
        return val

    def get_uncertainty(self, results: dict, num_atoms: list | None = None, *args, **kwargs):
        if self.q == "energy_std":
            val = self.get_energy_uncertainty(results=results)
        elif self.q in ["energy_grad_std", "forces_std"]:
            val = self.get_forces_uncertainty(results=results, num_atoms=num_atoms)
        else:
            raise TypeError(f"{self.q} not yet implemented")
        if self.umin is not None:
            val = self.scale_to_min_uncertainty(val)
        return _tensor(val)

    def get_input_params(self):
        return "ensemble", {"quantity": self.q, "order": self.order, "std_or_var": self.std_or_var, "min_uncertainty": self.umin}


def _device_index(device) -> int | None:
    """None for "cpu"; the ordinal of "cuda" / "cuda:n" / torch.device / int."""
    if isinstance(device, int):
        return device
    s = str(device)
    if s == "cpu":
        return None
    if s.startswith("cuda"):
        return int(s.split(":", 1)[1]) if ":" in s else 0
    raise ValueError(f"unknown device {device!r}")


class GMMUncertainty(Uncertainty):
    """Gaussian-mixture uncertainty of latent embeddings (reference ``:263-463``): the negative log-likelihood of each row."""

    log2pi = LOG2PI_F32

    def __init__(self, train_embed_key: str = "embedding", test_embed_key: str = "embedding", n_clusters: int = 5,
                 order: str = "atomic", covariance_type: str = "full", tol: float = 1e-3, max_iter: int = 100000,
                 n_init: int = 1, init_params: str = "kmeans", verbose: int = 0, device: str = "cuda", calibrate: bool = False,
                 cp_alpha: float | None = None, min_uncertainty: float | None = None, gmm_path: str | None = None,
                 gm_model=None, fit_device=None, *args, **kwargs):
        super().__init__(order=order, calibrate=calibrate, cp_alpha=cp_alpha, min_uncertainty=min_uncertainty, *args, **kwargs)
        self.train_key = train_embed_key
        self.test_key = test_embed_key
        self.n = n_clusters
        self.covar_type = covariance_type
        self.tol = tol
        self.max_iter = max_iter
        self.n_init = n_init
        self.init_params = init_params
        self.verbose = verbose
        self.device = device
        self.fit_device = fit_device   # None: fit_gmm runs scikit-learn on the host; "cuda" / "cuda:n": EM on that GPU (gmm_fit.hip)
        self._pending = None           # (GaussianMixture, GMMFitEngine) collecting resident rows (append_resident)
        self._engines = {}
        self.gm_model = None
        self.gmm_path = gmm_path
        if gmm_path is not None and os.path.exists(gmm_path):
            self.gm_model = load_pickle(gmm_path)
            self._set_gmm_params()
        elif gm_model is not None:
            self.gm_model = gm_model
            self._set_gmm_params()
        else:
            print(f"gm_model {gmm_path} does not exist")

    # -- fitting on the device (fit_device) --
    def _device_estimator(self):
        if self.fit_device is None or _device_index(self.fit_device) is None:
            raise ValueError("fitting on the device needs GMMUncertainty(fit_device='cuda' / 'cuda:n')")
        return GaussianMixture(n_components=self.n, covariance_type=self.covar_type, tol=self.tol, max_iter=self.max_iter,
                               n_init=self.n_init, init_params=self.init_params, verbose=self.verbose, device=self.fit_device,
                               random_state=getattr(self, "random_state", None))

    def _adopt_fit(self, gm) -> None:
        self.gm_model = gm
        if self.gmm_path is not None and not os.path.exists(self.gmm_path):
            gm.save(self.gmm_path)
            print(f"Saved fitted GMM model to {self.gmm_path}")
        self._set_gmm_params()

    def append_resident(self, painn_engine, model: int = 0, rows: str = "atoms") -> None:
        """Add the embedding resident on ``painn_engine``'s GPU after its last run to the rows of the next ``fit_appended``,
        device to device (vssr_gmm_fit_append_batch); call once per PaiNN batch."""
        if self._pending is None:
            gm = self._device_estimator()
            self._pending = (gm, gm.new_engine(painn_engine.embedding_dim()))
        self._pending[1].append_batch(painn_engine, model=model, rows=rows)

    def fit_appended(self) -> None:
        """Fit on everything ``append_resident`` collected; the rows never leave the device."""
        if self._pending is None:
            raise Exception("GMMUncertainty: no resident rows appended")
        gm, eng = self._pending
        self._pending = None
        self._adopt_fit(gm.fit_engine(eng))

    def fit_resident(self, painn_engine, model: int = 0, rows: str = "atoms") -> None:
        """``append_resident`` of one PaiNN batch and ``fit_appended``."""
        self._pending = None
        self.append_resident(painn_engine, model=model, rows=rows)
        self.fit_appended()

    # -- fitting (host, or the device with fit_device) --
    def fit_gmm(self, Xtrain) -> None:
        """Fit the mixture: with ``fit_device=None`` on the host with sklearn's ``GaussianMixture``; with ``fit_device="cuda"`` /
        ``"cuda:n"`` on that GPU (``uncertainty.GaussianMixture``)."""
        if self.fit_device is not None:
            self.Xtrain = Xtrain
            self._adopt_fit(self._device_estimator().fit(self._rows(Xtrain)))
            return
        try:
            from sklearn.mixture import GaussianMixture
        except ImportError as e:
            raise ImportError("GMMUncertainty.fit_gmm needs scikit-learn (sklearn.mixture.GaussianMixture), which is not "
                              "importable; load a fitted mixture instead (gmm_path= / gm_model= / Uncertainty.load)") from e
        self.Xtrain = Xtrain
        gm = GaussianMixture(n_components=self.n, covariance_type=self.covar_type, tol=self.tol, max_iter=self.max_iter,
                             n_init=self.n_init, init_params=self.init_params, verbose=self.verbose)
        gm.fit(self._rows(Xtrain))
        self.gm_model = gm
        if self.gmm_path is not None and not os.path.exists(self.gmm_path):
            with open(self.gmm_path, "wb") as fh:
                pickle.dump(_gmm_arrays(gm), fh)
            print(f"Saved fitted GMM model to {self.gmm_path}")
        self._set_gmm_params()

    def is_fitted(self) -> bool:
        return getattr(self, "gm_model", None) is not None

    def _set_gmm_params(self) -> None:
        if self.gm_model is None:
            raise Exception("GMMUncertainty: GMM does not exist/is not fitted")
        p = _gmm_arrays(self.gm_model)
        self.means = p["means_"].reshape(len(p["weights_"]), -1)
        self.precisions_cholesky = p["precisions_cholesky_"]
        self.weights = p["weights_"].reshape(-1)
        self.covariance_type = p["covariance_type"]
        K, D = self.means.shape
        self.prec_chol_full = full_precision_cholesky(self.precisions_cholesky, self.covariance_type, K, D)
        self._engines = {}

    @staticmethod
    def _rows(X) -> np.ndarray:
        """The reference's ``_check_tensor``: lists are concatenated, the input squeezed, fp64; one row becomes [1, D]."""
        if isinstance(X, list) and len(X) and hasattr(X[0], "__len__"):
            X = np.concatenate([np.asarray(_to_numpy(x)) for x in X])
        X = np.asarray(_to_numpy(X), dtype=np.float64).squeeze()
        return X.reshape(1, -1) if X.ndim == 1 else X

    def engine(self, device=None):
        """The ``backend.GMMEngine`` of this mixture on GPU ``device`` (default: this instance's device)."""
        idx = _device_index(self.device if device is None else device)
        if idx is None:
            raise ValueError("GMMUncertainty(device='cpu') scores on the host: no GPU engine")
        key = (idx, float(self.log2pi))
        if key not in self._engines:
            from . import backend

            gm = self.gm_model
            if isinstance(gm, GaussianMixture) and gm._fit_engine is not None and gm._fit_engine.device == idx:
                self._engines[key] = gm.scorer(float(self.log2pi))   # from the device arrays of the fit (vssr_gmm_fit_scorer)
                return self._engines[key]
            self._engines[key] = backend.GMMEngine(self.means, self.prec_chol_full, self.weights, device=idx,
                                                   log_2pi=float(self.log2pi))
        return self._engines[key]

    # -- scoring --
    def _log_prob_np(self, X: np.ndarray) -> np.ndarray:
        n, D = X.shape
        K = self.means.shape[0]
        P = self.prec_chol_full
        log_det = np.log(P[:, np.arange(D), np.arange(D)]).sum(axis=1)
        lp = np.empty((n, K))
        for k in range(K):
            y = X @ P[k] - self.means[k] @ P[k]
            lp[:, k] = np.sum(np.square(y), axis=1)
        return -0.5 * (D * self.log2pi + lp) + log_det

    def _scores(self, X, want_log_prob: bool):
        """(log_prob [n, K] or None, log_likelihood [n]) in numpy fp64 on this instance's device."""
        if not self.is_fitted():
            raise Exception("GMMUncertainty: GMM does not exist/is not fitted")
        X = self._rows(X)
        if _device_index(self.device) is None:
            lp = self._log_prob_np(X)
            wlp = lp + np.log(self.weights)
            m = wlp.max(axis=1)
            return lp, m + np.log(np.sum(np.exp(wlp - m.reshape(-1, 1)), axis=1))
        if want_log_prob:
            nll, lp = self.engine().score_rows(X, log_prob=True)
            return lp, -nll
        return None, -self.engine().score_rows(X)

    def estimate_log_prob(self, X):
        return _tensor(self._scores(X, True)[0])

    def estimate_weighted_log_prob(self, X):
        return _tensor(self._scores(X, True)[0] + np.log(self.weights))

    def log_likelihood(self, X):
        return _tensor(self._scores(X, False)[1])

    def probability(self, X):
        return _tensor(np.exp(self._scores(X, False)[1]))

    def negative_log_likelihood(self, X):
        return _tensor(-self._scores(X, False)[1])

    def _finish(self, u):
        if self.umin is not None:
            u = self.scale_to_min_uncertainty(u)
        if self.calibrate:
            u = self.calibrate_uncertainty(u)
        return u

    def get_uncertainty(self, results: dict, num_atoms: list | None = None, *args, **kwargs):
        """NLL of ``results[test_embed_key]``, reduced per structure for the ``system_*`` orders, shifted by ``min_uncertainty``
        and scaled by the conformal ``qhat`` when calibrated."""
        test = self._rows(results[self.test_key])
        if not self.is_fitted():
            self.fit_gmm(self._rows(results[self.train_key]))
        u = self.negative_log_likelihood(test)
        if "system" in self.order:
            u = get_system_val(u, num_atoms, self.order)
        return self._finish(u)

    def score_resident(self, painn_engine, model: int = 0, rows: str = "atoms"):
        """``get_uncertainty`` of the embedding resident on ``painn_engine``'s GPU after its last run, scored in place
        (vssr_gmm_score_batch) whatever this instance's ``device``.  ``rows="atoms"``: one row per atom, reduced per structure
        on the device for the ``system_*`` orders (the padding rule of ``get_system_val`` applied to the batch);
        ``rows="mean"``: one mean row per structure (already per structure, as in ``scripts/clustering.py``).  Returns
        ``(nll_rows, uncertainty)``: the raw NLL of every row, and the uncertainty (``min_uncertainty`` / calibration applied):
        per atom for ``order="atomic"`` with atom rows, else per structure [B]."""
        eng = self.engine(painn_engine.device_context()[0])
        if rows == "mean":
            nll, _ = eng.score_batch(painn_engine, model=model, rows="mean", order="atomic")
            return _tensor(nll), self._finish(_tensor(nll))
        if rows != "atoms":
            raise ValueError(f"rows must be 'atoms' or 'mean', got {rows!r}")
        if "system" not in self.order:
            nll, _ = eng.score_batch(painn_engine, model=model, rows="atoms", order="atomic")
            return _tensor(nll), self._finish(_tensor(nll))
        nll, sysv = eng.score_batch(painn_engine, model=model, rows="atoms", order=self.order)
        n_atoms = np.diff(np.asarray(painn_engine._cfg_start))
        sysv = nll if len(nll) == len(n_atoms) else apply_padding_rule(sysv, n_atoms, self.order)
        return _tensor(nll), self._finish(_tensor(sysv))

    def get_input_params(self):
        inputs = {"train_embed_key": self.train_key, "test_embed_key": self.test_key, "n_clusters": self.n, "order": self.order,
                  "covariance_type": self.covar_type, "tol": self.tol, "max_iter": self.max_iter, "n_init": self.n_init,
                  "verbose": self.verbose, "calibrate": self.calibrate, "cp_alpha": self.cp_alpha, "min_uncertainty": self.umin}
        if self.gm_model is not None:
            inputs["gm_model"] = _gmm_arrays(self.gm_model)
        else:
            inputs["gmm_path"] = self.gmm_path
        if self.calibrate:
            inputs["qhat"] = self.CP.qhat
        return "gmm", inputs


# ---- the estimator, fitted on the device ---------------------------------------------------------------------------------------------
class GaussianMixture:
    """Gaussian mixture fitted by expectation-maximisation on the GPU (``backend.GMMFitEngine``, ``csrc/gmm_fit.hip``): the
    reference's ``mcmc.uncertainty.gmm.GaussianMixture`` (a copy of sklearn's) with its constructor arguments and fitted
    attributes (``weights_``, ``means_``, ``covariances_``, ``precisions_cholesky_``, ``precisions_``, ``converged_``, ``n_iter_``,
    ``lower_bound_``, ``lower_bounds_``).

    What is and is not reproduced: the EM loop, the stopping rule, ``n_init`` and the precedence of ``weights_init`` /
    ``means_init`` / ``precisions_init`` are sklearn's; all arithmetic is fp64 with fixed summation orders (two fits of the same
    rows agree bit for bit).  The random draws of ``init_params="kmeans"`` (k-means++ seeding, then Lloyd iterations on the
    device) and ``"random_from_data"`` come from the project's counter-based generator (Philox4x32-10, ``mc.py``) keyed by
    ``random_state``: they cannot and need not reproduce numpy's or sklearn's streams, so a fit started that way matches sklearn
    in quality, not in numbers.  ``init_params="random"`` and ``"k-means++"`` are not built here (fit on the host with sklearn for
    those); ``warm_start`` is not supported.  ``fit(X, labels=...)`` starts from one-hot responsibilities of integer labels
    (what sklearn does with its k-means result) and is deterministic on both sides.  ``random_state=None`` draws a fresh seed.
    ``device``: "cuda" / "cuda:n" / int."""

    def __init__(self, n_components=1, *, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params="kmeans", weights_init=None, means_init=None, precisions_init=None, random_state=None,
                 warm_start=False, verbose=0, verbose_interval=10, device="cuda"):
        self.n_components, self.covariance_type, self.tol, self.reg_covar = n_components, covariance_type, tol, reg_covar
        self.max_iter, self.n_init, self.init_params = max_iter, n_init, init_params
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self.random_state, self.warm_start, self.verbose, self.verbose_interval = random_state, warm_start, verbose, verbose_interval
        self.device = device
        self._fit_engine = None
        self._scorers = {}

    # -- fitting --
    def _check_parameters(self):
        if self.covariance_type not in ("spherical", "tied", "diag", "full"):
            raise ValueError(f"Invalid value for 'covariance_type': {self.covariance_type} 'covariance_type' should be in "
                             "['spherical', 'tied', 'diag', 'full']")
        if self.warm_start:
            raise NotImplementedError("warm_start is not supported by the device fit")
        if self.init_params in ("random", "k-means++"):
            raise NotImplementedError(f"init_params={self.init_params!r} is not built on the device: use 'kmeans', "
                                      "'random_from_data' or labels=, or fit on the host (sklearn.mixture.GaussianMixture)")
        if self.init_params not in ("kmeans", "random_from_data"):
            raise ValueError(f"unknown init_params {self.init_params!r}")

    def new_engine(self, n_features: int, labels_given: bool = False):
        """A ``backend.GMMFitEngine`` configured from this estimator (rows still to be appended)."""
        from . import backend

        self._check_parameters()
        idx = _device_index(self.device)
        if idx is None:
            raise ValueError("GaussianMixture fits on a GPU: device must be 'cuda' / 'cuda:n'")
        seed = int.from_bytes(os.urandom(8), "little") if self.random_state is None else int(self.random_state)
        return backend.GMMFitEngine(self.n_components, n_features, covariance_type=self.covariance_type, tol=self.tol,
                                    reg_covar=self.reg_covar, max_iter=self.max_iter, n_init=self.n_init,
                                    init="given" if labels_given else self.init_params, seed=seed, device=idx)

    def fit_engine(self, eng, labels=None):
        """Fit on the rows resident in ``eng`` (``new_engine``; rows appended from the host or from PaiNN engines)."""
        eng.set_init(means=self.means_init, weights=self.weights_init, precisions=self.precisions_init, labels=labels)
        r = eng.fit()
        p = eng.params()
        self.weights_, self.means_ = p["weights_"], p["means_"]
        self.covariances_, self.precisions_cholesky_ = p["covariances_"], p["precisions_cholesky_"]
        self.converged_, self.n_iter_, self.lower_bound_ = r["converged"], r["n_iter"], r["lower_bound"]
        self.lower_bounds_ = list(r["lower_bounds"])
        if not self.converged_:
            warnings.warn("Best performing initialization did not converge. Try different init parameters, or increase "
                          "max_iter, tol, or check for degenerate data.")
        self._fit_engine, self._scorers = eng, {}
        return self

    def fit(self, X, y=None, labels=None):
        X = GMMUncertainty._rows(X)
        eng = self.new_engine(X.shape[1], labels_given=labels is not None)
        eng.append_rows(X)
        return self.fit_engine(eng, labels=labels)

    def fit_predict(self, X, y=None):
        return self.fit(X).predict(X)

    @property
    def precisions_(self):
        pc = np.asarray(self.precisions_cholesky_)
        if self.covariance_type == "full":
            return np.einsum("kij,klj->kil", pc, pc)
        if self.covariance_type == "tied":
            return pc @ pc.T
        return pc ** 2

    # -- scoring (fp64 log 2 pi, as sklearn) --
    def scorer(self, log_2pi: float = LOG2PI_F64):
        """The ``backend.GMMEngine`` of the fitted mixture: from the device arrays after a fit (vssr_gmm_fit_scorer)."""
        key = float(log_2pi)
        if key not in self._scorers:
            from . import backend

            if self._fit_engine is not None:
                self._scorers[key] = self._fit_engine.scorer(key)
            else:
                K, D = np.asarray(self.means_).shape
                self._scorers[key] = backend.GMMEngine(self.means_, full_precision_cholesky(self.precisions_cholesky_,
                                                       self.covariance_type, K, D), self.weights_,
                                                       device=_device_index(self.device), log_2pi=key)
        return self._scorers[key]

    def _estimate_log_prob(self, X):
        return self.scorer().score_rows(GMMUncertainty._rows(X), log_prob=True)[1]

    def score_samples(self, X):
        return -self.scorer().score_rows(GMMUncertainty._rows(X))

    def score(self, X, y=None):
        return float(np.mean(self.score_samples(X)))

    def predict_proba(self, X):
        nll, lp = self.scorer().score_rows(GMMUncertainty._rows(X), log_prob=True)
        return np.exp(lp + np.log(self.weights_) + nll[:, None])

    def predict(self, X):
        return (self._estimate_log_prob(X) + np.log(self.weights_)).argmax(axis=1)

    def _n_parameters(self) -> int:
        K, D = np.asarray(self.means_).shape
        cov = {"full": K * D * (D + 1) / 2.0, "diag": K * D, "tied": D * (D + 1) / 2.0, "spherical": K}[self.covariance_type]
        return int(cov + D * K + K - 1)

    def bic(self, X):
        n = GMMUncertainty._rows(X).shape[0]
        return -2 * self.score(X) * n + self._n_parameters() * np.log(n)

    def aic(self, X):
        return -2 * self.score(X) * GMMUncertainty._rows(X).shape[0] + 2 * self._n_parameters()

    # -- persistence: a dict of arrays, the form load_pickle reads --
    FITTED = ("weights_", "means_", "covariances_", "precisions_cholesky_", "converged_", "n_iter_", "lower_bound_", "lower_bounds_")

    def as_dict(self) -> dict:
        d = {"covariance_type": self.covariance_type, "n_components": self.n_components}
        for k in self.FITTED:
            if hasattr(self, k):
                v = getattr(self, k)
                d[k] = np.asarray(v) if k != "covariance_type" else v
        return d

    def save(self, filename):
        with open(filename, "wb") as fh:
            pickle.dump(self.as_dict(), fh)

    @classmethod
    def from_dict(cls, d, device="cuda"):
        gm = cls(n_components=int(d.get("n_components", len(d["weights_"]))), covariance_type=d.get("covariance_type", "full"),
                 device=device)
        for k in cls.FITTED:
            if k in d:
                setattr(gm, k, d[k])
        return gm


UNC_DICT = {"ensemble": EnsembleUncertainty, "gmm": GMMUncertainty}
