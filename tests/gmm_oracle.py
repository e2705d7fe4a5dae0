"""Independent numpy fp64 restatement of the Gaussian-mixture uncertainty (reference mcmc/uncertainty/uncertainty.py:238-463,
get_system_val of mcmc/uncertainty/prediction.py:181-223, EnsembleUncertainty :169-260) and test mixtures built at test time."""
import numpy as np

LOG2PI_F32 = float(np.float32(1.8378770351409912))
LOG2PI_F64 = float(np.log(2 * np.pi))
ORDERS = ("atomic", "system_sum", "system_mean", "system_max", "system_min", "system_mean_squared", "system_root_mean_squared")


def expand(prec, cov_type, K, D):
    """sklearn precisions_cholesky_ of any covariance type -> [K][D][D]."""
    prec = np.asarray(prec, dtype=np.float64)
    if cov_type == "full":
        return prec.reshape(K, D, D).copy()
    if cov_type == "tied":
        return np.stack([prec.reshape(D, D)] * K)
    if cov_type == "diag":
        return np.stack([np.diag(prec[k]) for k in range(K)])
    return np.stack([prec[k] * np.eye(D) for k in range(K)])


def log_prob(X, means, P, log2pi):
    """logp_k [n][K]: -0.5 (D log2pi + |x P_k - mu_k P_k|^2) + sum_d log P_k[d][d]."""
    X = np.asarray(X, dtype=np.float64)
    n, D = X.shape
    out = np.empty((n, len(means)))
    for k in range(len(means)):
        y = X @ P[k] - means[k] @ P[k]
        out[:, k] = -0.5 * (D * log2pi + np.einsum("ne,ne->n", y, y)) + np.sum(np.log(np.diagonal(P[k])))
    return out


def nll_of_log_prob(lp, weights):
    """NLL [n] from logp_k [n][K]: the logsumexp over the weighted components."""
    w = lp + np.log(np.asarray(weights, dtype=np.float64))
    m = np.max(w, axis=1, keepdims=True)
    return -(m[:, 0] + np.log(np.exp(w - m).sum(axis=1)))


def nll(X, means, P, weights, log2pi):
    return nll_of_log_prob(log_prob(X, means, P, log2pi), weights)


def system_val(val, num_atoms, order):
    """get_system_val: already per system when len(val) == len(num_atoms); else per-structure reductions of zero-padded rows
    (a structure shorter than the longest one sees the zeros in max / min)."""
    val = np.asarray(val, dtype=np.float64)
    num_atoms = [int(a) for a in num_atoms]
    if len(val) == len(num_atoms):
        return val
    L = max(num_atoms)
    out, o = [], 0
    for n in num_atoms:
        v = val[o:o + n]
        o += n
        pad = np.concatenate([v, np.zeros(L - n)])
        out.append({"system_sum": v.sum(), "system_mean": v.sum() / n, "system_max": pad.max(), "system_min": pad.min(),
                    "system_mean_squared": (v * v).sum() / n, "system_root_mean_squared": np.sqrt((v * v).sum() / n)}[order])
    return np.array(out).squeeze()


def uncertainty(X, gmm, order, num_atoms=None, umin=None, qhat=None, log2pi=LOG2PI_F32):
    means, P, weights = gmm
    u = nll(X, means, P, weights, log2pi)
    if order != "atomic":
        u = system_val(u, num_atoms, order)
    if umin is not None:
        u = u - (umin ** 2 if order == "system_mean_squared" else umin)
    if qhat is not None:
        u = u * qhat
    return u


def ensemble(results, quantity, order, std_or_var, num_atoms=None, umin=None):
    if quantity == "energy_std":
        val = np.asarray(results["energy_std"], np.float64) if std_or_var == "std" else np.asarray(results["energy_var"], np.float64) ** 2
    else:
        fs = np.asarray(results["forces_std"], np.float64)
        val = np.sqrt(((fs if std_or_var == "std" else fs ** 2) ** 2).sum(axis=-1))
        if order != "atomic":
            val = system_val(val, num_atoms, order)
    if umin is not None:
        val = val - (umin ** 2 if order == "system_mean_squared" else umin)
    return val


# ---- test mixtures ---------------------------------------------------------------------------------------------------------------
def random_gmm(K, D, cov_type="full", seed=0, scale=1.0):
    """Seeded random mixture in sklearn's parameter layout: (means [K][D], precisions_cholesky_, weights [K]); full factors are
    upper triangular, P = inv(chol(cov)).T as sklearn computes them."""
    rng = np.random.default_rng(seed)
    means = rng.normal(scale=scale, size=(K, D))
    weights = rng.uniform(0.2, 1.0, K)
    weights /= weights.sum()

    def chol_prec(cov):
        return np.linalg.inv(np.linalg.cholesky(cov)).T

    if cov_type == "full":
        prec = np.empty((K, D, D))
        for k in range(K):
            A = rng.normal(size=(D, D)) / np.sqrt(D)
            prec[k] = chol_prec(scale ** 2 * (A @ A.T + 0.5 * np.eye(D)))
    elif cov_type == "tied":
        A = rng.normal(size=(D, D)) / np.sqrt(D)
        prec = chol_prec(scale ** 2 * (A @ A.T + 0.5 * np.eye(D)))
    elif cov_type == "diag":
        prec = 1.0 / np.sqrt(scale ** 2 * rng.uniform(0.3, 2.0, size=(K, D)))
    else:
        prec = 1.0 / np.sqrt(scale ** 2 * rng.uniform(0.3, 2.0, size=K))
    return means, prec, weights


def species_gmm(emb, numbers):
    """One component per species of embedding rows (fp64): empirical mean and covariance + 1e-3 I, P = inv(chol(cov)).T."""
    emb = np.asarray(emb, dtype=np.float64)
    zs = sorted(set(int(z) for z in numbers))
    means, prec, w = [], [], []
    for z in zs:
        E = emb[np.asarray(numbers) == z]
        mu = E.mean(axis=0)
        cov = (E - mu).T @ (E - mu) / max(len(E) - 1, 1) + 1e-3 * np.eye(emb.shape[1])
        means.append(mu)
        prec.append(np.linalg.inv(np.linalg.cholesky(cov)).T)
        w.append(len(E))
    w = np.array(w, dtype=np.float64)
    return np.array(means), np.array(prec), w / w.sum()
