"""The Gaussian-mixture scoring and fit on the MI355X beyond their fixture shapes (csrc/gmm.hip, csrc/gmm_fit.hip through vssr_gmm_* and
vssr_gmm_fit_*), on the inputs of tests/gmm_cases.py (whose presumptions tests/test_gmm_cases_cpu.py asserts without a GPU):

A  caller rows: every instantiation of k_gmm_logp at its largest pad, the 64-row workgroup edges, K = 256, six different zero-block
   masks in one mixture, zero weights;
B  the resident embedding with chains of 1, 255, 256, 257 and 540 atoms (the strided trips of k_gmm_reduce and k_gmm_mean_rows);
C  one EM iteration at K = 256, D = 255 / 17 / 33 / 15 / 1 and every row-count residue of the slab kernels;
D  the start-up paths (partial explicit starts on top of labels, labels with -1, clear, a failed fit);
E  restarts: the parameters, trace and scorer of the reported restart are the ones restored, bit for bit;
F  the device k-means against its restatement, an empty cluster included.

Bounds.  Scoring (A, B): the project's max |got - want| / (1 + |want|) <= 1e-9 on nll and log_prob against tests/gmm_oracle.py.
Fit (C, D, F): ONE_ITER_REL = 1e-8 relative to each array's maximum against tests/gmm_fit_oracle.py (test_gpu_gmm_fit.py derives it for a
few thousand rows and cond(S_k) < 1e3; the rehearsal asserts the condition numbers of the new cases).  "Bit for bit" compares the
device with itself where the driver promises identical results."""
import numpy as np
import pytest

import gmm_cases as gc
import gmm_fit_oracle as fo
import gmm_oracle as go
from surface_sampling_amd import backend, uncertainty as U
from test_gpu_gmm_fit import ONE_ITER_REL, _engine_result
from test_gpu_uncertainty import _engine

pytestmark = pytest.mark.gpu
SCORE_BOUND = 1e-9


def _score_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not np.isnan(got).any()
    return float((np.abs(got - want) / (1.0 + np.abs(want))).max())


def _check_scores(eng, X, means, P, w, who):
    """nll and log_prob of caller rows against the restatement; returns the device arrays."""
    nll, lp = eng.score_rows(X, log_prob=True)
    want_lp = go.log_prob(X, means, P, go.LOG2PI_F32)
    with np.errstate(divide="ignore"):   # log(0) of a zero weight
        want = go.nll_of_log_prob(want_lp, w)                 # (go.nll of the same rows, without a second pass over the factors)
    e_nll, e_lp = _score_err(nll, want), _score_err(lp, want_lp)
    print(f"{who}: nll error {e_nll:.3e}  log_prob error {e_lp:.3e}  bound {SCORE_BOUND:.0e}  (max nll {want.max():.3e})")
    assert e_nll <= SCORE_BOUND and e_lp <= SCORE_BOUND, (who, e_nll, e_lp)
    return nll, lp, want


# ---- A. caller rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", gc.A_DIMS)
def test_every_instantiation_at_its_pad(D):
    for cov in gc.COVS:
        means, P, w, X = gc.scoring_case(3, D, cov)
        eng = backend.GMMEngine(means, P, w, device=0, log_2pi=go.LOG2PI_F32)
        _, _, want = _check_scores(eng, X, means, P, w, f"NB={gc.nb(D)} D={D} {cov}")
        eng.close()
        assert want.max() > 1e4


def test_row_count_edges_do_not_depend_on_neighbours():
    means, P, w, X = gc.scoring_case(3, 33, "full")
    X = X[-129:]                                              # ordinary rows and the three outliers
    eng = backend.GMMEngine(means, P, w, log_2pi=go.LOG2PI_F32)
    nll_all, lp_all, _ = _check_scores(eng, X, means, P, w, "D=33 n=129")
    for n in gc.A_ROW_COUNTS:
        for rows, sl in ((X[:n], slice(0, n)), (X[129 - n:], slice(129 - n, 129))):
            nll, lp = eng.score_rows(rows, log_prob=True)
            assert np.array_equal(nll, nll_all[sl]) and np.array_equal(lp, lp_all[sl]), n
    eng.close()


@pytest.mark.parametrize("cov", gc.COVS)
def test_256_components(cov):
    means, P, w, X = gc.scoring_case(256, 16, cov, 40)
    eng = backend.GMMEngine(means, P, w, log_2pi=go.LOG2PI_F32)
    _check_scores(eng, X, means, P, w, f"K=256 D=16 {cov}")
    eng.close()


def test_256_components_of_255_columns():
    means, P, w, X = gc.scoring_case(256, 255, "full", 107)
    X = X[list(range(20)) + list(range(256, 366))]            # 20 means, 107 ordinary rows, 3 outliers
    assert len(X) == 130
    eng = backend.GMMEngine(means, P, w, log_2pi=go.LOG2PI_F32)
    _check_scores(eng, X, means, P, w, "K=256 D=255 full")
    eng.close()


def test_components_with_different_masks():
    means, P, w, X = gc.mask_case()
    eng = backend.GMMEngine(means, P, w, log_2pi=go.LOG2PI_F32)
    _, lp, _ = _check_scores(eng, X, means, P, w, "six masks, D=80")
    want = go.log_prob(X, means, P, go.LOG2PI_F32)
    for k, kind in enumerate(gc.MASK_KINDS):
        print(f"  {kind}: log_prob error {_score_err(lp[:, k], want[:, k]):.3e}")
    eng.close()
    # the same mixture in reverse order: a mask belongs to its component, not to its position
    rev = backend.GMMEngine(means[::-1], P[::-1], w[::-1], log_2pi=go.LOG2PI_F32)
    _, lp_rev, _ = _check_scores(rev, X, means[::-1], P[::-1], w[::-1], "six masks reversed")
    assert np.array_equal(lp_rev[:, ::-1], lp)
    rev.close()


def test_zero_weights_drop_out():
    means, P, w, X = gc.zero_weight_case()
    keep = [0, 2, 4]
    eng = backend.GMMEngine(means, P, w, log_2pi=go.LOG2PI_F32)
    nll, lp, _ = _check_scores(eng, X, means, P, w, "w[1] = w[3] = 0")
    eng.close()
    assert np.isfinite(nll).all() and np.isfinite(lp).all()
    e3 = _score_err(nll, go.nll(X, means[keep], P[keep], w[keep], go.LOG2PI_F32))
    print(f"against the three-component mixture: {e3:.3e}  bound {SCORE_BOUND:.0e}")
    assert e3 <= SCORE_BOUND
    full = backend.GMMEngine(means, P, np.full(5, 0.2), log_2pi=go.LOG2PI_F32)
    assert np.array_equal(full.score_rows(X, log_prob=True)[1], lp)     # log_prob does not know the weights
    full.close()


# ---- B. the resident embedding -------------------------------------------------------------------------------------------------------
def _reduction(v, order):
    """The true reduction of one structure's row NLLs (gmm_oracle.system_val takes one row for a value that is reduced already)."""
    return {"system_sum": v.sum(), "system_mean": v.sum() / len(v), "system_max": v.max(), "system_min": v.min(),
            "system_mean_squared": (v * v).sum() / len(v), "system_root_mean_squared": np.sqrt((v * v).sum() / len(v))}[order]


def test_resident_chains_around_256_atoms(golden):
    eng = _engine(golden)
    structs = gc.long_chains(golden)
    n_atoms = [len(s[0]) for s in structs]
    assert tuple(n_atoms) == gc.B_CHAINS
    eng.evaluate(structs)
    emb = eng.embedding(1).astype(np.float64)
    starts = np.cumsum([0] + n_atoms[:-1])
    means, prec, w = go.species_gmm(emb, np.concatenate([s[0] for s in structs]))
    means2, prec2, w2 = go.random_gmm(4, 128, "full", seed=128, scale=float(np.abs(emb).mean()) + 0.1)
    worst = 0.0
    for gm in ((means, prec, w), (np.concatenate([means, means2]), np.concatenate([prec, prec2]), np.concatenate([w, w2]))):
        g = backend.GMMEngine(*gm)
        want_rows = go.nll(emb, *gm, go.LOG2PI_F32)
        for order in go.ORDERS:
            nll, sysv = g.score_batch(eng, model=1, rows="atoms", order=order)
            errs = [_score_err(nll, want_rows)]
            if order == "atomic":
                assert sysv is None
            else:
                true = np.array([_reduction(want_rows[o:o + n], order) for o, n in zip(starts, n_atoms)])
                errs += [_score_err(sysv, true),
                         _score_err(U.apply_padding_rule(sysv, n_atoms, order), go.system_val(want_rows, n_atoms, order))]
            print(f"K={len(gm[0])} {order}: errors {['%.3e' % e for e in errs]}  bound {SCORE_BOUND:.0e}")
            worst = max(worst, *errs)
            a = g.score_batch(eng, model=1, rows="atoms", order=order)
            assert np.array_equal(a[0], nll) and (sysv is None or np.array_equal(a[1], sysv)), order
        mrows = np.stack([emb[o:o + n].mean(axis=0) for o, n in zip(starts, n_atoms)])
        nll_m, sys_m = g.score_batch(eng, model=1, rows="mean", order="system_max")
        e_m = _score_err(nll_m, go.nll(mrows, *gm, go.LOG2PI_F32))
        print(f"K={len(gm[0])} mean rows: error {e_m:.3e}  bound {SCORE_BOUND:.0e}")
        worst = max(worst, e_m)
        b = g.score_batch(eng, model=1, rows="mean", order="system_max")
        assert np.array_equal(sys_m, nll_m) and np.array_equal(b[0], nll_m)
        g.close()
    eng.close()
    assert worst <= SCORE_BOUND, worst


# ---- fits ----------------------------------------------------------------------------------------------------------------------------
def _fit(X, K, cov="full", init="given", appends=1, start=None, **kw):
    """A fresh engine on rows X (in ``appends`` parts), started by set_init(**start): (result with sklearn's names, best_init)."""
    eng = backend.GMMFitEngine(K, X.shape[1], covariance_type=cov, init=init, **kw)
    for part in np.array_split(X, appends):
        eng.append_rows(part)
    if start:
        eng.set_init(**start)
    r, p = eng.fit(), eng.params()
    eng.close()
    return dict(p, n_iter_=r["n_iter"], converged_=r["converged"], lower_bound_=r["lower_bound"], lower_bounds_=r["lower_bounds"]), r["best_init"]


def _check_fit(got, want, who):
    worst = 0.0
    for key in fo.COMPARED:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and np.isfinite(g).all(), (who, key)
        err = float(np.max(np.abs(g - w))) / float(np.max(np.abs(w)))
        worst = max(worst, err)
        print(f"{who} {key}: relative error {err:.3e}  bound {ONE_ITER_REL:.0e}")
    assert worst <= ONE_ITER_REL, (who, worst)


def _same_bits(a, b, who=""):
    for key in fo.COMPARED:
        assert np.array_equal(a[key], b[key]), (who, key)
    assert a["n_iter_"] == b["n_iter_"] and a["converged_"] == b["converged_"]


# ---- C. one EM iteration -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.C_CASES, ids=lambda c: "-".join(map(str, c)))
def test_one_em_iteration_at_the_uncovered_shapes(case):
    cov, K, D, N = case
    c = gc.em_case(*case)
    got, _ = _fit(c["X"], K, cov, appends=2 if N > 2 else 1, tol=0.0, reg_covar=c["reg_covar"], max_iter=1,
                  start=dict(means=c["means"], weights=c["weights"], precisions=c["precisions"]))
    assert got["n_iter_"] == 1 and not got["converged_"]
    _check_fit(got, c["want"], f"{cov} K={K} D={D} N={N}")


# ---- D. start-up paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", gc.D_PARTIAL, ids="+".join)
@pytest.mark.parametrize("cov", gc.COVS)
@pytest.mark.parametrize("D", gc.D_DIMS)
def test_partial_explicit_start_on_top_of_labels(D, cov, names):
    c = gc.start_case(cov, D)
    start = {n: c["given"][n] for n in names}
    got, _ = _fit(c["X"], c["K"], cov, tol=0.0, max_iter=1, start=dict(start, labels=c["labels"]))
    _check_fit(got, gc.start_want(cov, D, names), f"{cov} D={D} labels + {'+'.join(names)}")


@pytest.mark.parametrize("cov", gc.COVS)
@pytest.mark.parametrize("D", gc.D_DIMS)
def test_labels_with_unassigned_rows(D, cov):
    c = gc.unlabelled_case(cov, D)
    got, _ = _fit(c["X"], c["K"], cov, appends=3, tol=0.0, max_iter=1, start=dict(labels=c["labels"]))
    _check_fit(got, c["want"], f"{cov} D={D} labels with -1")


def test_clear_drops_rows_and_labels():
    a, b = gc.start_case("full", 20), gc.start_case("full", 20, N=601)
    kw = dict(tol=0.0, max_iter=3)
    eng = backend.GMMFitEngine(3, 20, init="given", **kw)
    eng.append_rows(a["X"])
    eng.set_init(labels=a["labels"])
    first = _engine_result(eng)
    eng.clear()
    assert eng.n_rows == 0
    with pytest.raises(backend.BackendError, match="at least 2 rows"):
        eng.fit()
    eng.append_rows(b["X"])
    with pytest.raises(backend.BackendError, match="init = given needs labels"):     # the labels of A went with its rows
        eng.fit()
    with pytest.raises(backend.BackendError, match="no completed fit"):
        eng.params()
    eng.set_init(labels=b["labels"])
    second = _engine_result(eng)
    fresh, _ = _fit(b["X"], 3, start=dict(labels=b["labels"]), **kw)
    _same_bits(second, fresh, "after clear")
    assert not np.array_equal(first["means_"], second["means_"])
    # more rows without new labels: refused by the library; with labels for all rows the handle fits as a fresh one does
    eng.append_rows(a["X"][:100])
    with pytest.raises(backend.BackendError, match="601 labels for 701 resident rows"):
        eng.fit()
    both, labels = np.concatenate([b["X"], a["X"][:100]]), np.concatenate([b["labels"], a["labels"][:100]])
    eng.set_init(labels=labels)
    third = _engine_result(eng)
    eng.close()
    fresh, _ = _fit(both, 3, start=dict(labels=labels), **kw)
    _same_bits(third, fresh, "after the second append")


def test_a_failed_fit_leaves_no_parameters():
    fx = fo.load_fixture("full_d20_k3_collapsed")
    X, K = fx["X"], fx["K"]
    good = (np.arange(len(X)) % K).astype(np.int32)
    kw = dict(tol=fx["tol"], reg_covar=fx["reg_covar"], max_iter=5)
    eng = backend.GMMFitEngine(K, X.shape[1], init="given", **kw)
    eng.append_rows(X)
    eng.set_init(labels=good)
    before = _engine_result(eng)                      # a completed fit: its parameters must not outlive the failure below
    eng.set_init(labels=fx["labels"])
    with pytest.raises(ValueError, match=fo.ILL_DEFINED):
        eng.fit()
    with pytest.raises(backend.BackendError, match="vssr error -5: GMM fit: no completed fit"):
        eng.params()
    with pytest.raises(backend.BackendError, match="vssr error -5: GMM fit: no completed fit"):
        eng.scorer()
    eng.set_init(labels=good)
    after = _engine_result(eng)
    eng.close()
    fresh, _ = _fit(X, K, start=dict(labels=good), **kw)
    _same_bits(after, fresh, "after the failure")
    _same_bits(after, before, "before and after the failure")


# ---- E. restarts ---------------------------------------------------------------------------------------------------------------------
def _restart_run(X, cov, init, m, start=None):
    eng = backend.GMMFitEngine(4, X.shape[1], covariance_type=cov, tol=gc.E_TOL, max_iter=gc.E_MAX_ITER, init=init, seed=gc.E_SEED,
                               n_init=m)
    eng.append_rows(X)
    if start:
        eng.set_init(**start)
    r, p = eng.fit(), eng.params()
    res = dict(p, n_iter_=r["n_iter"], converged_=r["converged"], lower_bound_=r["lower_bound"], lower_bounds_=r["lower_bounds"])
    # the scorer built on the device from the restored buffers against an engine built from the downloaded parameters
    sc = eng.scorer(go.LOG2PI_F32)
    P = go.expand(p["precisions_cholesky_"], cov, 4, X.shape[1])
    host = backend.GMMEngine(p["means_"], P, p["weights_"], log_2pi=go.LOG2PI_F32)
    a, b = sc.score_rows(X[:50], log_prob=True), host.score_rows(X[:50], log_prob=True)
    for x in (sc, host, eng):
        x.close()
    return res, r["best_init"], (a, b)


@pytest.mark.parametrize("cov", gc.COVS)
@pytest.mark.parametrize("init", ["kmeans", "random_from_data"])
def test_restarts_restore_the_reported_restart(init, cov):
    X, _ = gc.separated()
    runs = {m: _restart_run(X, cov, init, m) for m in range(1, gc.E_M + 1)}
    bests = [runs[m][1] for m in runs]
    print(init, cov, "best_init", bests, "lower bounds", [runs[m][0]["lower_bound_"] for m in runs])
    for m, (res, best, (sc, host)) in runs.items():
        assert 0 <= best < m
        if m > 1:
            assert res["lower_bound_"] >= runs[m - 1][0]["lower_bound_"]
        _same_bits(res, runs[best + 1][0], f"n_init={m} against n_init={best + 1}")
        assert res["lower_bound_"] == res["lower_bounds_"][-1] == runs[best + 1][0]["lower_bound_"]
        print(f"n_init={m}: scorer against an engine of params(): max |d nll| {np.abs(sc[0] - host[0]).max():.3e}  "
              f"max |d log_prob| {np.abs(sc[1] - host[1]).max():.3e}  (must be 0)")
        assert np.array_equal(sc[0], host[0]) and np.array_equal(sc[1], host[1]), f"scorer of n_init={m}"
    if init == "random_from_data" and cov != "tied":
        # the restated restarts end further apart than any rounding: the device must report the same ones, and for n_init = 3, 4
        # the best is restart 1, restored over the later ones
        want = gc.restart_bounds(init, cov)
        assert bests == [gc.best_init(want, m) for m in runs] and 0 < bests[2] < 2 and 0 < bests[3] < 3
        print("best lower bound", runs[4][0]["lower_bound_"], "restated", want.max())   # (printed only: no multi-iteration bound here)


@pytest.mark.parametrize("cov", gc.COVS)
def test_given_start_restarts_are_identical(cov):
    X, labels = gc.separated()
    one, b1, _ = _restart_run(X, cov, "given", 1, start=dict(labels=labels))
    three, b3, (sc, host) = _restart_run(X, cov, "given", 3, start=dict(labels=labels))
    assert b1 == 0 and b3 == 0
    _same_bits(one, three, "given, n_init = 3")
    assert np.array_equal(sc[0], host[0]) and np.array_equal(sc[1], host[1])


# ---- F. k-means ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.F_CASES, ids=lambda c: "-".join(map(str, c)))
def test_kmeans_start_against_the_restatement(case):
    K, D, N, seed = case
    X = gc.kmeans_rows(K, D, N)
    wants = [gc.kmeans_case(K, D, N, seed, r)["want"] for r in range(gc.F_RESTARTS)]
    bounds = np.array([w["lower_bound_"] for w in wants])
    seen = set()
    for m in range(1, gc.F_RESTARTS + 1):
        got, best = _fit(X, K, init="kmeans", seed=seed, n_init=m, tol=0.0, max_iter=1)
        srt = np.sort(bounds[:m])
        if m == 1 or srt[-1] - srt[-2] > gc.F_GAP * abs(srt[-1]):  # (a gap rounding cannot close: the device must pick this restart)
            assert best == int(np.argmax(bounds[:m])), (m, best, bounds)
        assert 0 <= best < m
        seen.add(best)
        _check_fit(got, wants[best], f"kmeans K={K} D={D} N={N} n_init={m} (restart {best})")
    print("restarts compared:", sorted(seen), "restated bounds after one iteration:", bounds)
    if case == gc.F_EVERY_RESTART:
        assert seen == set(range(gc.F_RESTARTS))


@pytest.mark.parametrize("cov", gc.COVS)
def test_kmeans_empty_cluster(cov):
    c = gc.empty_cluster_case(cov)
    kw = dict(init="kmeans", seed=gc.EMPTY_SEED, tol=0.0, reg_covar=gc.EMPTY_REG, max_iter=1)
    got, _ = _fit(c["X"], 3, cov, **kw)
    again, _ = _fit(c["X"], 3, cov, **kw)
    for key in ("weights_", "means_", "covariances_", "precisions_cholesky_", "lower_bounds_"):
        assert np.isfinite(got[key]).all(), key
    _same_bits(got, again, "empty cluster")
    _check_fit(got, c["want"], f"empty cluster {cov}")
    empty = int(np.argmin(np.bincount(c["labels"], minlength=3)))
    print(f"empty cluster {cov}: component {empty} has weight {got['weights_'][empty]:.3e} and mean {got['means_'][empty]}")
    assert not got["means_"][empty].any() and 0.0 < got["weights_"][empty] < 1e-16
