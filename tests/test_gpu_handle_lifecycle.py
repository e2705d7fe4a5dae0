"""Create / destroy routes of the eight handle kinds on the MI355X (csrc/api_handle.hip: one create path, owning buffers): every
kind is created, does one small piece of work, is closed, and is created again -- the second life gives the first one's bits.  A
create that fails after the device was opened leaves its message and a usable process; closing never-used and already-closed
handles works.  Nothing here faults the device: every failing call fails in host validation."""
import numpy as np
import pytest

import cell_cases as cc
import pair_oracle as po
import sw_oracle as so
from conftest import SI_T3, SI_T3_A0, diamond_cell
from surface_sampling_amd import backend

pytestmark = pytest.mark.gpu

ONES = np.ones(3, np.uint8)


def _two_chains(a):
    """Two chains on the 8-atom diamond cell: the lattice, and a copy with displaced atoms."""
    T, X, cell = diamond_cell(a)
    X2 = X + 0.05 * np.random.default_rng(3).normal(size=X.shape)
    return [(T, X, cell, ONES), (T, X2, cell, ONES)]


def _analytic(make, a):
    def life():
        eng = make()
        e, ea, f = eng.evaluate_f64(_two_chains(a))
        st, _ = eng.stress()
        eng.close()
        return [e, ea, f, st]
    return life


def _pair():
    """Born + coul/dsf on the 8-atom rocksalt cube (a 12 A cutoff over several images) and a copy with displaced atoms."""
    from surface_sampling_amd import pair

    T, X, cell = po.rocksalt(5.64)
    X2 = X + 0.05 * np.random.default_rng(3).normal(size=X.shape)
    eng = backend.PairEngine(pair.parse(po.ROCKSALT_COMMANDS, 2), device=0)
    e, ea, f = eng.evaluate_f64([(T, X, cell, ONES), (T, X2, cell, ONES)])
    st, _ = eng.stress()
    eng.close()
    return [e, ea, f, st]


def _painn(golden):
    s = golden.structure("GaN_3x3_pristine")      # the smallest golden structure; second chain: displaced atoms
    pbc = np.asarray(s.pbc)
    X2 = s.positions + 0.05 * np.random.default_rng(4).normal(size=s.positions.shape)
    chains = [(s.numbers, s.positions, np.asarray(s.cell), pbc), (s.numbers, X2, np.asarray(s.cell), pbc)]

    def life():
        eng = backend.PainnEngine(golden.blobs, device=0)
        r = eng.evaluate(chains)
        emb = eng.embedding(0)
        eng.close()
        return [r["energy_f64"], r["energy_std_f64"], r["forces"], r["forces_std"], emb]
    return life


def _rows(n, D, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(size=(n // 2, D)) - 2.0, rng.normal(size=(n - n // 2, D)) + 2.0])


def _gmm():
    K, D = 3, 16
    rng = np.random.default_rng(5)
    means, w = rng.normal(size=(K, D)), np.array([0.2, 0.3, 0.5])
    prec = np.stack([np.tril(0.1 * rng.normal(size=(D, D)), -1) + np.diag(rng.uniform(0.5, 2.0, D)) for _ in range(K)])
    eng = backend.GMMEngine(means, prec, w, device=0)
    nll, lp = eng.score_rows(_rows(16, D, 6), log_prob=True)
    eng.close()
    return [nll, lp]


def _gmm_fit():
    D = 8
    X = _rows(32, D, 7)
    eng = backend.GMMFitEngine(2, D, covariance_type="full", max_iter=3, tol=0.0, init="given", device=0)
    eng.append_rows(X)
    eng.set_init(labels=(np.arange(32) >= 16).astype(np.int32))
    res = eng.fit()
    p = eng.params()
    sc = eng.scorer()              # a scoring handle the library creates itself, on the same path
    nll = sc.score_rows(X)
    sc.close()
    eng.close()
    assert res["n_iter"] == 3
    return [res["lower_bounds"], p["weights_"], p["means_"], p["covariances_"], p["precisions_cholesky_"], nll]


def _cluster():
    D = 8
    eng = backend.ClusterEngine(D, n_components=4, whiten=True, cluster_dims=3, device=0)
    eng.append_rows(_rows(32, D, 8))
    eng.pca()
    p = eng.pca_params()
    xr = eng.projected()
    Z, _ = eng.linkage()
    eng.close()
    assert Z.shape == (31, 4)
    return [p["mean_"], p["components_"], p["explained_variance_"], xr, Z]


def _lives(golden):
    return {
        "painn": _painn(golden),
        "tersoff": _analytic(lambda: backend.TersoffEngine(SI_T3, device=0), SI_T3_A0),
        "eam": _analytic(lambda: backend.EAMEngine(cc.cu_funcfl(), device=0), 5.0),
        "sw": _analytic(lambda: backend.SWEngine(so.si_params(), device=0), 5.431),
        "pair": _pair,
        "gmm": _gmm,
        "gmm_fit": _gmm_fit,
        "cluster": _cluster,
    }


@pytest.mark.parametrize("kind", ["painn", "tersoff", "eam", "sw", "pair", "gmm", "gmm_fit", "cluster"])
def test_second_life_repeats_the_first_bit_for_bit(golden, kind):
    life = _lives(golden)[kind]
    first, second = life(), life()
    assert len(first) == len(second)
    for k, (a, b) in enumerate(zip(first, second)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.size > 0 and np.isfinite(a).all(), (kind, k)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (kind, k)


def test_create_failing_after_device_init_reports_and_recovers():
    lib = backend.load_library()
    bad = SI_T3.copy()
    bad[0, 0, 0, 0] = 2.0    # m must be 1 or 3: refused by vssr_tersoff_create after the stream exists
    with pytest.raises(backend.BackendError, match=r"\(-1\).*bad tersoff entry") as ei:
        backend.TersoffEngine(bad, device=0)
    assert "bad tersoff entry 0" in str(ei.value)
    msg = lib.vssr_last_error(None)
    assert msg and b"bad tersoff entry" in msg
    eng = backend.TersoffEngine(SI_T3, device=0)      # the process creates a good handle next
    e, _, f = eng.evaluate_f64(_two_chains(SI_T3_A0))
    eng.close()
    assert np.isfinite(e).all() and np.isfinite(f).all() and abs(e[0] / 8 + 4.63) < 1e-2


def test_closing_unused_and_closed_handles():
    fit = backend.GMMFitEngine(2, 16, device=0)       # neither ever received rows: no device behind them
    clu = backend.ClusterEngine(16, n_components=4, device=0)
    ters = backend.TersoffEngine(SI_T3, device=0)
    for eng in (fit, clu, ters):
        eng.close()
        assert not eng._h
        eng.close()                                   # a no-op
        assert not eng._h
