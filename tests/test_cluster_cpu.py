"""Latent-space clustering without a GPU: the numpy restatements (tests/cluster_oracle.py and the package's host path) against the
scikit-learn / SciPy fixtures of tools/make_cluster_golden.py, fcluster's numbering, select_data_and_save's rule, the ABI refusals
that need no device, and the launcher's rebinding of mcmc.utils.clustering; and the rehearsal of tests/cluster_cases.py: every case of the
device shape sweep is what it is listed as (spectral gaps, linkage margins, the closed-form tree) and the host path passes it."""
import ctypes as C
import os
import pickle
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import cluster_cases as cs
import cluster_oracle as co
from conftest import ROOT
from surface_sampling_amd import backend, clustering as cl


@pytest.mark.parametrize("name", ["ward_n1000_d3", "ward_n3000_d3"])
def test_restatements_reproduce_scipy_linkage(name):
    fx = co.load(name)
    for what, (Z, rounds) in (("oracle", co.ward_rnn(fx["points"])), ("host path", cl.ward_linkage_host(fx["points"]))):
        assert np.array_equal(Z[:, [0, 1, 3]], fx["Z"][:, [0, 1, 3]]), what
        err = float(np.max(np.abs(Z[:, 2] - fx["Z"][:, 2])) / fx["Z"][:, 2].max())
        print(f"{name} {what}: {rounds} rounds, height error {err:.2e}")
        assert err <= 1e-10 and rounds <= len(Z)
        for crit, t, labels in co.cuts(fx):
            assert co.same_partition(co.partition(Z, t, crit), labels), (what, crit, t)
            assert np.array_equal(cl.fcluster(Z, t, criterion=crit, depth=2), labels), (what, crit, t)


def test_fcluster_numbers_clusters_as_scipy_on_the_fixture_trees():
    for name in ("ward_n1000_d3", "ward_n3000_d3"):
        fx = co.load(name)
        cuts = co.cuts(fx)
        assert len(cuts) == 6
        for crit, t, labels in cuts:
            got = cl.fcluster(fx["Z"], t, criterion=crit)
            assert got.dtype == np.int32 and np.array_equal(got, labels), (name, crit, t)
    Z = co.load("ward_n1000_d3")["Z"]
    assert np.array_equal(cl.fcluster(Z, 5000, "maxclust"), np.arange(1, 1001))     # more clusters than rows: every row alone
    assert len(np.unique(cl.fcluster(Z, 1, "maxclust"))) == 1
    with pytest.raises(ValueError):
        cl.fcluster(Z, 1.0, "inconsistent")


def test_duplicated_points_same_partitions_and_termination():
    fx = co.load("ward_dups_n600")
    for Z, rounds in (co.ward_rnn(fx["points"]), cl.ward_linkage_host(fx["points"])):
        assert rounds <= 599 and np.sum(Z[:, 2] == 0.0) == 400
        for crit, t, labels in co.cuts(fx):
            assert co.same_partition(cl.fcluster(Z, t, criterion=crit), labels), (crit, t)


def test_pca_restatements_against_sklearn_fixture():
    fx = co.load("pca_d128_n1000")
    X = fx["X"].astype(np.float64)
    for what, (Xr, p) in (("oracle", co.pca_svd(X)), ("host path", cl.pca_host(X))):
        lam = fx["explained_variance_"]
        assert np.max(np.abs(p["explained_variance_"] - lam)) <= 1e-12 * lam[0], what
        assert np.max(np.abs(p["explained_variance_ratio_"] - fx["explained_variance_ratio_"])) <= 1e-12
        assert np.max(np.abs(p["mean_"] - fx["mean_"])) <= 1e-13
        d = float(np.max(np.abs(Xr[:, :3] - fx["X_r"][:, :3])))
        print(f"{what}: |X_r[:, :3] - fixture| = {d:.2e} (ref_spread {float(fx['ref_spread']):.2e})")
        assert d <= float(fx["ref_spread"]), what
        sv = np.linalg.svd(p["components_"] @ fx["components_"].T, compute_uv=False)
        assert np.max(np.abs(sv - 1.0)) <= 1e-9, what
    with pytest.raises(ValueError, match="n_components"):
        cl.pca_host(X[:20], 32)


def test_perform_clustering_on_the_host_equals_the_pipeline_fixture(tmp_path):
    fx = co.load("pipeline_n1000")
    rows = [r for r in fx["X"].astype(np.float64)]
    for crit in ("distance", "maxclust"):
        y = cl.perform_clustering(rows, float(fx[f"t_{crit}"]), cutoff_criterion=crit, save_folder=str(tmp_path), device=None)
        assert np.array_equal(y, fx[f"labels_{crit}"]), crit


def test_select_data_and_save_keeps_the_references_rule(tmp_path):
    fx = co.load("pipeline_n1000")
    y, mv = fx["labels_maxclust"], fx["metric_values"]
    items = [{"row": i} for i in range(len(y))]
    sel = cl.select_data_and_save(items, y, mv, "force_std", save_folder=str(tmp_path), save_prepend="t_")
    assert np.array_equal(sel, fx["selected"])
    tied = [c for c in np.unique(y) if np.sum(mv[y == c] == mv[y == c].max()) > 1]
    assert tied, "the fixture holds no tie"
    for c in tied:                       # the earliest row among the tied maxima
        rows = np.flatnonzero((y == c) & (mv == mv[y == c].max()))
        assert sel[c - 1] == rows[0]
    with open(tmp_path / "t_clustered.pkl", "rb") as fh:
        assert [d["row"] for d in pickle.load(fh)] == sel.tolist()
    rnd = cl.select_indices(y, mv, "random", rng=np.random.default_rng(0))
    assert np.array_equal(y[rnd], np.unique(y))


def test_get_cluster_centers_and_closest_points_on_the_host():
    P = co.load("ward_n1000_d3")["points"]
    centers, labels = cl.get_cluster_centers(P, 12, device=None)
    assert centers.shape == (12, 3) and np.array_equal(labels, co.load("ward_n1000_d3")["labels_maxclust_12"])
    idx = cl.find_closest_points_indices(P, centers, labels)
    assert np.array_equal(labels[idx], np.arange(1, 13))


# ---- the rehearsal of tests/cluster_cases.py -----------------------------------------------------------------------------------------
def test_pca_case_names_are_the_cases():
    assert tuple(c.name for c in cs.pca_cases()) == cs.PCA_NAMES
    for c in cs.pca_cases():
        N, D = c.X.shape
        assert 1 <= c.n_components <= min(N, D) and c.whiten in (0, 1) and np.all(np.isfinite(c.X)), c.name
    shapes = {c.X.shape[1]: c.X.shape[0] for c in cs.pca_cases() if c.name.startswith("shapes")}
    assert shapes == {1: 257, 2: 257, 3: 257, 15: 257, 16: 257, 17: 257, 100: 257, 255: 600, 256: 600}


@pytest.mark.parametrize("name", cs.PCA_NAMES)
def test_pca_cases_are_what_they_claim_and_the_host_path_passes_them(name):
    c = cs.pca_case(name)
    N, D = c.X.shape
    with np.errstate(all="ignore"):
        lam = co.pca_svd(c.X, min(N, D), False)[1]["explained_variance_"]      # the oracle's whole spectrum
    compared = [k for g in c.groups for k in g]
    assert compared == sorted(set(compared)) and all(list(g) == list(range(g[0], g[-1] + 1)) for g in c.groups)
    assert compared == [k for k in range(c.n_components) if lam[k] > cs.NULL_EV * lam[0]]     # exactly the non-zero components
    gaps = []
    for g in c.groups:
        lo, hi = g[0], g[-1]
        assert lam[lo] - lam[hi] <= cs.GROUP_EQ * lam[lo], (name, g)
        gaps += [(lam[lo - 1] - lam[lo]) / lam[lo - 1]] if lo > 0 else []
        gaps += [(lam[hi] - lam[hi + 1]) / lam[hi]] if hi + 1 < len(lam) else []
    print(f"{name}: {len(c.groups)} groups over {len(compared)} of {c.n_components} components, smallest relative gap "
          f"{min(gaps, default=np.inf):.2e}, l_min / l_0 {lam[compared[-1]] / lam[0]:.2e}")
    assert min(gaps, default=np.inf) >= cs.SINGLE_GAP
    if name.startswith("rank_deficient"):
        assert len(compared) == N - 1 < c.n_components
    if name == "constant_column":
        assert len(compared) == D - 2 and np.all(c.X[:, [4, 11]] == c.X[0, [4, 11]])
    if name == "degenerate":
        assert np.max(np.abs(lam - [4, 4, 4, 2, 1, 1, 0.5, 0.4, 0.3, 0.25, 0.2, 0.15, 0.1, 0.08, 0.06, 0.05])) <= 1e-13
        assert [len(g) for g in c.groups[:3]] == [3, 1, 2]
    if name == "diagonal":
        cov = np.cov(c.X.T)
        assert np.max(np.abs(cov - np.diag(np.diag(cov)))) <= 1e-14
    with np.errstate(all="ignore"):
        Xr, p = cl.pca_host(c.X, c.n_components, bool(c.whiten))
    cs.pca_check(c, cs.pca_figures(c, Xr, p), "host path, ")
    if name == "offset" or name in cs.SPREAD_XR:
        sp = cs.pca_spread(name)
        print(f"{name}: |pca_svd - pca_longdouble| " + ", ".join(f"{k} {sp[k]:.2e}" for k in ("mean", "ev", "ratio", "vec", "sub", "xr")))
        assert sp["sign_ok"] and sp["finite"]
        assert all(sp[k] <= 1e3 * b for k, b in cs.pca_bounds(c).items())      # the two oracles describe the same PCA


@pytest.mark.parametrize("name", cs.GENERAL_NAMES)
def test_general_linkage_cases_keep_their_margin_and_the_host_path_gives_the_oracles_tree(name):
    P = cs.general(name).points
    Zo, rounds_o, gap = cs.tree(name)
    Z, rounds = cl.ward_linkage_host(P)
    same, err, same_rounds = cs.tree_figures(Z, rounds, Zo, rounds_o)
    print(f"{name}: {rounds_o} rounds, margin {gap:.2e} (at least {cs.MARGIN:.0e}), host path height error {err:.2e}")
    assert gap >= cs.MARGIN
    assert same and same_rounds and err <= 1e-10
    assert co.ward_rnn(P)[1] == rounds_o                     # the default return is (Z, rounds)
    if P.shape[0] in (257, 513):
        assert 15 <= rounds_o <= 27


def test_pca_to_linkage_inputs_keep_their_margin():
    Xr0, _ = cs.pca_reference("shapes_d17_w1")
    for cd in (5, 9):
        Z, rounds, gap = co.ward_rnn(Xr0[:, :cd], margin=True)
        print(f"whitened coordinates of shapes_d17, {cd} columns: {rounds} rounds, margin {gap:.2e}")
        assert gap >= cs.MARGIN


@pytest.mark.parametrize("permuted", [False, True])
def test_hierarchy_gives_the_closed_form_tree_through_the_oracle(permuted):
    k = 8
    perm = np.random.default_rng(5).permutation(1 << k) if permuted else None
    P = cs.hierarchy(k, perm=perm)
    h, s = cs.hierarchy_heights(k)
    for what, (Z, rounds) in (("oracle", co.ward_rnn(P)), ("host path", cl.ward_linkage_host(P))):
        assert rounds == k, what
        cs.check_hierarchy_tree(Z, k, perm)
        assert np.array_equal(Z[:, 2], h) and np.array_equal(Z[:, 3], s), what       # exact heights and sizes
    _, _, gap = co.ward_rnn(P, margin=True)
    print(f"hierarchy({k}): margin {gap:.3f}")
    assert gap >= 0.75                                        # the sibling key is at most a quarter of any other key (x = 1 and 3)
    x = cs.hierarchy(17)[:, 0]                                # the size of the device test: exact integers, all distinct
    assert x[-1] == (3.0 ** 17 - 1) / 2 and len(np.unique(x)) == 1 << 17 and 9.0 ** 16 < 2.0 ** 53


def test_the_tree_checker_rejects_wrong_trees():
    k = 8
    Z, _ = co.ward_rnn(cs.hierarchy(k))
    cs.check_hierarchy_tree(Z, k)
    bad = Z.copy()                                            # one swapped pair: leaves 1 and 2 change partners
    r1, r2 = (int(np.flatnonzero((Z[:, 0] == a) & (Z[:, 1] == a + 1))[0]) for a in (0, 2))
    bad[r1, 1], bad[r2, 0] = 2, 1
    with pytest.raises(AssertionError, match="sibling"):
        cs.check_hierarchy_tree(bad, k)
    bad = Z.copy()                                            # a pair of the next level merged one level early
    top = int(np.flatnonzero(Z[:, 3] == 4)[0])
    bad[[0, top]] = bad[[top, 0]]
    with pytest.raises(AssertionError):
        cs.check_hierarchy_tree(bad, k)
    bad = Z.copy()                                            # a node used twice
    bad[-1, 0] = bad[-2, 0]
    with pytest.raises(AssertionError):
        cs.check_hierarchy_tree(bad, k)
    with pytest.raises(AssertionError):                       # the right tree of other points
        cs.check_hierarchy_tree(Z, k, np.random.default_rng(5).permutation(1 << k))


def _create(dim, n_components, cluster_dims, whiten=1, device=0):
    lib = backend.load_library()
    cfg = backend.ClusterConfig(C.sizeof(backend.ClusterConfig), device, dim, n_components, whiten, cluster_dims)
    h = C.c_void_p(None)
    rc = lib.vssr_cluster_create(C.byref(cfg), C.byref(h))
    return lib, rc, h


@pytest.mark.parametrize("dim,nc,cd", [(0, 1, 1), (257, 32, 3), (16, 17, 3), (16, 0, 3), (128, 32, 0), (128, 32, 33)])
def test_abi_refuses_bad_configurations_without_a_device(dim, nc, cd):
    lib, rc, h = _create(dim, nc, cd)
    assert rc == -1 and not h.value                        # VSSR_E_BADARG
    assert lib.vssr_last_error(None)
    with pytest.raises(backend.BackendError):
        backend.ClusterEngine(dim, n_components=nc, cluster_dims=cd)


def test_abi_refuses_bad_rows_and_states_without_a_device():
    eng = backend.ClusterEngine(4, n_components=2, cluster_dims=2)
    bad = np.ones((3, 4))
    bad[1, 2] = np.nan
    with pytest.raises(backend.BackendError, match="non-finite"):
        eng.append_rows(bad)
    pts = np.ones((3, 2))
    pts[2, 0] = np.inf
    with pytest.raises(backend.BackendError, match="non-finite"):
        eng.set_points(pts)
    with pytest.raises(backend.BackendError, match="at least 2 rows"):
        eng.pca()
    with pytest.raises(backend.BackendError, match="no points"):
        eng.linkage()
    with pytest.raises(backend.BackendError, match="no completed PCA"):
        eng.pca_params()
    lib = eng._lib
    assert lib.vssr_batch_run(eng._h, 1) == -1 and b"vssr_cluster_" in lib.vssr_last_error(eng._h)   # an evaluation entry point refuses kind 7
    assert lib.vssr_gmm_fit_clear(eng._h) == -1
    fit = backend.GMMFitEngine(2, 4)
    assert lib.vssr_cluster_clear(fit._h) == -1 and lib.vssr_cluster_linkage(fit._h, None, None) == -1
    fit.close()
    eng.close()
    assert C.sizeof(backend.ClusterConfig) == 24 and C.sizeof(backend.ClusterPcaResult) == 16


def test_install_clustering_rebinds_the_reference_namespace(tmp_path):
    pkg = tmp_path / "mcmc" / "utils"
    pkg.mkdir(parents=True)
    (tmp_path / "mcmc" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "clustering.py").write_text(textwrap.dedent("""
        def perform_clustering(*a, **k):
            return "reference"
        def select_data_and_save(*a, **k):
            return "reference"
        def untouched():
            return "reference"
    """))
    script = textwrap.dedent("""
        from surface_sampling_amd import launch
        done = launch.install_clustering()
        from mcmc.utils.clustering import perform_clustering, select_data_and_save, untouched
        print(sorted(done), perform_clustering.__module__, select_data_and_save.__module__, untouched())
        print(launch.install_clustering(package="no_such_package.utils"))
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, str(tmp_path)]))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert "perform_clustering" in lines[0] and "select_data_and_save" in lines[0]
    assert lines[0].endswith("surface_sampling_amd.clustering surface_sampling_amd.clustering reference")
    assert lines[1] == "{}"
