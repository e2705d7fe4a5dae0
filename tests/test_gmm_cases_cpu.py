"""What tests/test_gpu_gmm_shapes.py presumes about its inputs (tests/gmm_cases.py), asserted against the numpy restatements without
a GPU: every instantiation of k_gmm_logp is reached, the six block masks differ, the one-iteration cases are as well conditioned as
ONE_ITER_REL assumes, a given start array changes the result, one restart in the middle is the best, the restated k-means is far from
every boundary where another summation order could pick differently, and the empty-cluster rows are exact."""
import numpy as np
import pytest

import gmm_cases as gc
import gmm_fit_oracle as fo
import gmm_oracle as go


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) / float(np.max(np.abs(b)))


def test_widths_reach_every_instantiation_at_its_largest_pad():
    assert {gc.nb(D) for D in gc.A_DIMS} == set(range(1, 17))
    assert {16 * n - 15 for n in range(1, 17)} <= set(gc.A_DIMS) and {15, 255} <= set(gc.A_DIMS)
    assert all(D % 16 for D in gc.A_DIMS)                      # every width has pad columns
    assert {1, 63, 64, 65, 128, 129} == set(gc.A_ROW_COUNTS)
    for D in gc.A_DIMS:                                        # the rows of the existing shape test: means, ordinary rows, outliers
        for cov in gc.COVS if D in (1, 15, 17) else ("full",):
            means, P, w, X = gc.scoring_case(3, D, cov)
            assert len(X) == 3 + 150 + 3 and np.array_equal(X[:3], means)
            assert 1e4 < go.nll(X, means, P, w, go.LOG2PI_F32).max() < 1e7, (D, cov)


def test_mask_components_differ_block_by_block():
    means, P, w, X = gc.mask_case()
    masks = [gc.block_mask(p) for p in P]
    assert len(masks) == 6 and all(m.shape == (5, 5) for m in masks)
    for i in range(6):
        for j in range(i):
            assert not np.array_equal(masks[i], masks[j]), (gc.MASK_KINDS[i], gc.MASK_KINDS[j])
    assert any(not np.array_equal(m, m.T) for m in masks)
    kind = dict(zip(gc.MASK_KINDS, masks))
    assert np.array_equal(kind["diagonal"], np.eye(5)) and kind["dense"].all()
    assert np.array_equal(kind["upper"], np.triu(np.ones((5, 5)))) and np.array_equal(kind["lower"], np.tril(np.ones((5, 5))))
    hole = np.triu(np.ones((5, 5)))
    hole[1, 3] = 0
    assert np.array_equal(kind["upper_with_hole"], hole)
    assert np.array_equal(kind["block_diagonal"], np.block([[np.ones((2, 2)), np.zeros((2, 3))], [np.zeros((3, 2)), np.ones((3, 3))]]))
    assert (np.diagonal(P, axis1=1, axis2=2) > 0).all() and np.isfinite(go.nll(X, means, P, w, go.LOG2PI_F32)).all()
    # a kernel that skipped by the transposed mask, or by another component's, would be wrong by far more than the scoring bound
    lp = go.log_prob(X, means, P, go.LOG2PI_F32)
    for k, name in enumerate(gc.MASK_KINDS):
        if np.array_equal(masks[k], masks[k].T):
            continue
        Pt = P.copy()
        Pt[k] *= np.kron(masks[k].T, np.ones((16, 16)))
        assert np.max(np.abs(go.log_prob(X, means, Pt, go.LOG2PI_F32)[:, k] - lp[:, k]) / (1 + np.abs(lp[:, k]))) > 1e-3, name


def test_zero_weights_drop_out_of_the_restatement():
    means, P, w, X = gc.zero_weight_case()
    assert w[1] == 0.0 and w[3] == 0.0 and abs(w.sum() - 1.0) < 1e-15
    keep = [0, 2, 4]
    with np.errstate(divide="ignore"):
        five = go.nll(X, means, P, w, go.LOG2PI_F32)
    three = go.nll(X, means[keep], P[keep], w[keep], go.LOG2PI_F32)
    assert np.isfinite(five).all() and np.max(np.abs(five - three) / (1 + np.abs(three))) <= 1e-12
    # rows at the means of the dropped components: their own component would dominate if it were counted
    lp = go.log_prob(X[[1, 3]], means, P, go.LOG2PI_F32)
    assert lp[0].argmax() == 1 and lp[1].argmax() == 3


@pytest.mark.parametrize("case", gc.C_CASES, ids=lambda c: "-".join(map(str, c)))
def test_one_iteration_cases_are_well_conditioned(case):
    cov, K, D, N = case
    c = gc.em_case(*case)
    cond = gc.covariance_condition(c["want"]["covariances_"], cov)
    print(case, "max cond", cond)
    assert cond <= 1e3
    assert c["X"].shape == (N, D) and np.isfinite(c["want"]["precisions_cholesky_"]).all()


def test_one_iteration_cases_cover_the_slab_edges():
    cases = set(gc.C_CASES)
    assert {c[3] % 4 for c in cases if c[:3] == ("full", 3, 17)} == {0, 1, 2, 3}
    assert {c[3] % 4 for c in cases if c[:3] == ("tied", 5, 33)} == {0, 1, 2, 3}
    assert ("full", 3, 17, 1025) in cases and ("diag", 2, 1, 2) in cases and ("full", 2, 255, 2300) in cases
    assert {c[0] for c in cases if c[1] == 256} == {"full", "diag", "tied"}    # S_m = 4096 / K = 16 moment slabs
    assert 4096 // 256 == 16 and 24576 // 256 >= 16


@pytest.mark.parametrize("cov", gc.COVS)
@pytest.mark.parametrize("D", gc.D_DIMS)
def test_every_given_start_array_changes_the_first_iteration(cov, D):
    base = gc.start_want(cov, D, ())
    for names in gc.D_PARTIAL:
        got = gc.start_want(cov, D, names)
        diffs = {k: _rel(got[k], base[k]) for k in fo.COMPARED}
        print(cov, D, names, {k: f"{v:.1e}" for k, v in diffs.items()})
        assert min(diffs.values()) > 1e-6, (names, diffs)
    u = gc.unlabelled_case(cov, D)
    lab = u["labels"]
    assert (lab[256:512] == -1).all() and (lab == -1).sum() == len(lab) // 4 and set(lab) == {-1, 0, 1, 2}
    assert min(_rel(u["want"][k], fo.fit(u["X"], 3, cov, tol=0.0, max_iter=1, labels=gc.start_case(cov, D, len(lab))["labels"])[k])
               for k in fo.COMPARED) > 1e-6


def test_philox_uniform_layout():
    """The draw restated in gmm_fit_oracle.uniform against a scalar transcription of Philox4x32-10 (Salmon et al., SC'11)."""
    def philox(c, k):
        c, k = list(c), list(k)
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        return c

    for seed, restart, draw in ((0, 0, 0), (5, 3, 17), (2 ** 40 + 9, 1, 2)):
        c = philox([draw, restart, 0x676D6D, 0], [seed & 0xFFFFFFFF, seed >> 32])
        assert fo.uniform(seed, restart, draw) == ((c[0] << 32 | c[1]) >> 11) * 2.0 ** -53
    assert 0.0 <= fo.uniform(1, 0, 0) < 1.0


def test_a_middle_restart_is_the_best():
    """Restart 1 of the "random_from_data" start on the separated rows reaches the optimum, restarts 0, 2 and 3 stop in worse
    maxima: for n_init = 3 and 4 the best restart is neither the first nor the last, by a gap no rounding can close."""
    for cov in ("full", "diag", "spherical"):
        b = gc.restart_bounds("random_from_data", cov)
        print(cov, b)
        srt = np.sort(b)
        assert srt[-1] - srt[-2] > gc.E_GAP
        for m in (3, 4):
            assert 0 < gc.best_init(b, m) < m - 1
    labels = [fo.random_from_data_labels(1600, 4, gc.E_SEED, r) for r in range(gc.E_M)]
    assert all((l >= 0).sum() == 4 and sorted(l[l >= 0]) == [0, 1, 2, 3] for l in labels)
    assert len({tuple(np.nonzero(l >= 0)[0]) for l in labels}) == gc.E_M        # the restarts draw different rows


@pytest.mark.parametrize("case", gc.F_CASES, ids=lambda c: "-".join(map(str, c)))
def test_restated_kmeans_is_far_from_every_boundary(case):
    K, D, N, seed = case
    for restart in range(gc.F_RESTARTS):
        c = gc.kmeans_case(K, D, N, seed, restart)
        m = c["margins"]
        print(case, "restart", restart, m, "members", np.bincount(c["labels"], minlength=K).tolist())
        assert m["walk"] >= gc.F_MARGIN and m["tie"] >= gc.F_MARGIN and m["exact_ties"] == 0
        assert np.bincount(c["labels"], minlength=K).min() > D            # every cluster can carry a full covariance
    if case == gc.F_EVERY_RESTART:       # n_init = 1, 2, 3 pick restarts 0, 1, 2: every restart index is compared on the device
        b = [gc.kmeans_case(K, D, N, seed, r)["want"]["lower_bound_"] for r in range(gc.F_RESTARTS)]
        assert b[1] - b[0] > gc.F_GAP * abs(b[1]) and b[2] - b[1] > gc.F_GAP * abs(b[2]), b
    # the restarts are different starts: the comparison through n_init is not three times the same one
    assert len({gc.kmeans_case(K, D, N, seed, r)["labels"].tobytes() for r in range(gc.F_RESTARTS)}) > 1


def test_restated_kmeans_finds_the_separated_clusters():
    X, truth = gc.separated()
    labels, centres, _ = fo.kmeans(X, 4, 3, 0)
    assert len({(a, b) for a, b in zip(labels, truth)}) == 4                  # a relabelling of the truth
    for k in range(4):
        assert np.allclose(centres[k], X[labels == k].mean(axis=0), rtol=0, atol=1e-12)


def test_empty_cluster_rows_are_exact():
    c = gc.empty_cluster_case()
    X, labels = c["X"], c["labels"]
    assert len(np.unique(X, axis=0)) == 2 and np.array_equal(X, np.round(X)) and np.abs(X).max() <= 5
    counts = np.bincount(labels, minlength=3)
    assert sorted(counts) == [0, 200, 200]
    empty = int(np.argmin(counts))
    assert not c["centres"][empty].any()                                       # the centre without members is the origin
    want = c["want"]
    assert all(np.isfinite(want[k]).all() for k in fo.COMPARED)
    assert not want["means_"][empty].any() and want["weights_"][empty] < 1e-16
    # the origin is so far from both rows (|x|^2 = 100 against a variance of reg_covar) that its responsibilities underflow to 0
    for cov in gc.COVS:
        w = gc.empty_cluster_case(cov)["want"]
        assert w["weights_"][empty] == 10 * np.finfo(np.float64).eps / 400 and np.isfinite(w["precisions_cholesky_"]).all()
