"""Latent-space clustering on the MI355X (csrc/cluster.hip through vssr_cluster_* and surface_sampling_amd.clustering) against the
scikit-learn / SciPy fixtures of tools/make_cluster_golden.py.  Bounds: explained variance 1e-12 x the largest eigenvalue (about
100 x D x 2^-53, the backward error of a symmetric eigen-solver with two orders of margin); the first three whitened coordinates
within the fixture's own ref_spread (how far sklearn's default randomized solver lies from its full solver on these rows);
trailing components as a subspace (singular values of V_dev^T V_ref within 1e-9 of 1); tree pairs and sizes identical, heights
within 1e-10 x the largest (N - 1 weighted-mean updates of 2^-53 each, one order of margin at 1e5 rows); labels identical.
The shape sweep (tests/cluster_cases.py, rehearsed in tests/test_cluster_cpu.py) holds the same bounds against co.pca_svd and
co.ward_rnn: single components 1 - |<v_dev, v_ref>| <= 1e-9, unwhitened coordinates 1e-9 sqrt(l_0), whitened coordinates 1e-6 for
l_c >= 1e-6 l_0 (a perturbation eps l_0 of the covariance turns such a vector by eps l_0 / gap, scaled up by 1 / sqrt(l_c)); the
offset case max(bound, 10 x |pca_svd - pca_longdouble|).  Above 65 536 points the reference is the closed-form tree of
cluster_cases.hierarchy.  Measured figures: profiles/r21/NOTES_cluster_shapes.md."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as cs
import cluster_oracle as co
from surface_sampling_amd import backend, clustering as cl
from test_gpu_uncertainty import _engine, _structs

pytestmark = pytest.mark.gpu


def test_pca_against_sklearn_fixture():
    fx = co.load("pca_d128_n1000")
    X = fx["X"].astype(np.float64)
    eng = backend.ClusterEngine(128, n_components=32, whiten=True, cluster_dims=3)
    eng.append_rows(X[:400])
    eng.append_rows(X[400:])
    info = eng.pca()
    p, Xr = eng.pca_params(), eng.projected()
    print("pca:", info)
    assert info["converged"] and info["n_rows"] == 1000
    lam = fx["explained_variance_"]
    e_ev = float(np.max(np.abs(p["explained_variance_"] - lam)) / lam[0])
    e_x3 = float(np.max(np.abs(Xr[:, :3] - fx["X_r"][:, :3])))
    sv = np.linalg.svd(p["components_"] @ fx["components_"].T, compute_uv=False)
    print(f"explained variance {e_ev:.2e} (bound 1e-12), X_r[:, :3] {e_x3:.2e} (ref_spread {float(fx['ref_spread']):.2e}), "
          f"subspace {float(np.max(np.abs(sv - 1))):.2e}")
    assert e_ev <= 1e-12
    assert np.max(np.abs(p["explained_variance_ratio_"] - fx["explained_variance_ratio_"])) <= 1e-12
    assert np.max(np.abs(p["mean_"] - fx["mean_"])) <= 1e-13
    assert e_x3 <= float(fx["ref_spread"])
    assert np.max(np.abs(sv - 1.0)) <= 1e-9
    for c in range(32):                                    # sklearn's sign rule: the largest-magnitude loading is positive
        assert p["components_"][c, np.argmax(np.abs(p["components_"][c]))] > 0
    assert np.array_equal(eng.projected(10, 5), Xr[10:15])
    eng.close()


@pytest.mark.parametrize("name", cs.PCA_NAMES)
def test_pca_shapes_against_the_svd(name):
    c = cs.pca_case(name)
    N, D = c.X.shape
    eng = backend.ClusterEngine(D, n_components=c.n_components, whiten=bool(c.whiten), cluster_dims=1)
    cut = max(1, N // 3)                                   # two unequal parts (equal only where N = 2)
    eng.append_rows(c.X[:cut])
    eng.append_rows(c.X[cut:])
    info = eng.pca()
    p, Xr = eng.pca_params(), eng.projected()
    first, n = N // 3, min(5, N - N // 3)
    window, rows = eng.projected(first, n), np.stack([eng.projected(r, 1)[0] for r in (0, N - 1)])
    eng.close()
    print(f"{name}: D = {D}, N = {N}, n_components = {c.n_components}, whiten = {c.whiten}, {info}")
    f = cs.pca_figures(c, Xr, p)
    cs.pca_check(c, f, "device, ")
    assert info["converged"] and info["n_rows"] == N and info["n_sweeps"] < 60
    assert Xr.shape == (N, c.n_components) and p["components_"].shape == (c.n_components, D)
    assert np.array_equal(window, Xr[first:first + n]) and np.array_equal(rows, Xr[[0, N - 1]])


def _linkage(P):
    eng = backend.ClusterEngine(P.shape[1], n_components=1, cluster_dims=P.shape[1])
    eng.set_points(P)
    Z, rounds = eng.linkage()
    eng.close()
    return Z, rounds


@pytest.mark.parametrize("name", cs.GENERAL_NAMES)
def test_linkage_trees_at_every_width_and_edge(name):
    P = cs.general(name).points
    Zo, rounds_o, gap = cs.tree(name)
    Z, rounds = _linkage(P)
    Z2, rounds2 = _linkage(P)
    same, err, same_rounds = cs.tree_figures(Z, rounds, Zo, rounds_o)
    print(f"{name}: {rounds} rounds (oracle {rounds_o}, margin {gap:.2e}), pairs and sizes identical {same}, "
          f"height error {err:.2e} (bound 1e-10)")
    assert Z.shape == (len(P) - 1, 4)
    assert same and same_rounds and err <= 1e-10
    assert Z.tobytes() == Z2.tobytes() and rounds == rounds2


@pytest.mark.parametrize("permuted", [False, True])
def test_linkage_above_65536_points_follows_the_closed_form(permuted):
    k = 17                                                 # 131 072 points: 512 workgroups, two entries per thread of k_ward_scan
    perm = np.random.default_rng(5).permutation(1 << k) if permuted else None
    Z, rounds = _linkage(cs.hierarchy(k, perm=perm))
    h, s = cs.hierarchy_heights(k)
    print(f"hierarchy({k}), permuted {permuted}: {rounds} rounds, heights exact {np.array_equal(Z[:, 2], h)}, "
          f"sizes exact {np.array_equal(Z[:, 3], s)}")
    assert rounds == k
    assert np.array_equal(Z[:, 2], h) and np.array_equal(Z[:, 3], s)
    cs.check_hierarchy_tree(Z, k, perm)


@pytest.mark.parametrize("cluster_dims", [5, 9])
def test_pca_feeds_the_linkage_at_padded_widths(cluster_dims):
    c = cs.pca_case("shapes_d17_w1")
    eng = backend.ClusterEngine(17, n_components=9, cluster_dims=cluster_dims)
    eng.append_rows(c.X)
    eng.pca()
    Xr = eng.projected()
    Z, rounds = eng.linkage()
    eng.close()
    Z2, rounds2 = _linkage(Xr[:, :cluster_dims])           # the same coordinates through set_points: the pad columns are zero
    Zo, rounds_o = co.ward_rnn(cs.pca_reference(c.name)[0][:, :cluster_dims])
    same, err, same_rounds = cs.tree_figures(Z, rounds, Zo, rounds_o)
    print(f"cluster_dims = {cluster_dims}: {rounds} rounds (oracle {rounds_o}), bit-identical to set_points "
          f"{Z.tobytes() == Z2.tobytes()}, pairs and sizes identical to the oracle {same}, height error {err:.2e}")
    assert Z.tobytes() == Z2.tobytes() and rounds == rounds2
    assert same and same_rounds and err <= 1e-10


@pytest.mark.parametrize("name", ["ward_n1000_d3", "ward_n3000_d3"])
def test_linkage_against_scipy_fixture(name):
    fx = co.load(name)
    eng = backend.ClusterEngine(3, n_components=1, cluster_dims=3)
    eng.set_points(fx["points"])
    Z, rounds = eng.linkage()
    eng.close()
    err = float(np.max(np.abs(Z[:, 2] - fx["Z"][:, 2])) / fx["Z"][:, 2].max())
    print(f"{name}: {rounds} rounds, height error {err:.2e}")
    assert np.array_equal(Z[:, [0, 1, 3]], fx["Z"][:, [0, 1, 3]])
    assert err <= 1e-10
    cuts = co.cuts(fx)
    assert len(cuts) == 6
    for crit, t, labels in cuts:
        assert np.array_equal(cl.fcluster(Z, t, criterion=crit, depth=2), labels), (crit, t)


def test_duplicated_points_terminate_with_the_same_partitions():
    fx = co.load("ward_dups_n600")
    eng = backend.ClusterEngine(3, n_components=1, cluster_dims=3)
    eng.set_points(fx["points"])
    Z, rounds = eng.linkage()
    eng.close()
    print(f"duplicates: {rounds} rounds")
    assert rounds <= 599 and np.sum(Z[:, 2] == 0.0) == 400
    cuts = co.cuts(fx)
    assert len(cuts) == 6
    for crit, t, labels in cuts:
        assert co.same_partition(cl.fcluster(Z, t, criterion=crit), labels), (crit, t)


@pytest.mark.parametrize("d", [1, 2, 5, 32])
def test_other_point_widths_against_the_restatement(d):
    rng = np.random.default_rng(d)
    P = rng.normal(size=(700, d)) + 3.0 * rng.integers(0, 4, size=(700, 1))
    centers, labels = cl.get_cluster_centers(P, 9)
    Zo, rounds_o = co.ward_rnn(P)
    assert np.array_equal(labels, cl.fcluster(Zo, 9, "maxclust"))
    assert centers.shape == (9, d)
    Z, rounds = _linkage(P)
    same, err, same_rounds = cs.tree_figures(Z, rounds, Zo, rounds_o)
    print(f"d = {d}: {rounds} rounds (oracle {rounds_o}), pairs and sizes identical {same}, height error {err:.2e} (bound 1e-10)")
    assert same and same_rounds and err <= 1e-10


def test_whole_pipeline_equals_the_fixture(tmp_path):
    fx = co.load("pipeline_n1000")
    rows = [r for r in fx["X"].astype(np.float64)]
    for crit in ("distance", "maxclust"):
        y = cl.perform_clustering(rows, float(fx[f"t_{crit}"]), cutoff_criterion=crit, save_folder=str(tmp_path))
        assert np.array_equal(y, fx[f"labels_{crit}"]), crit


def test_resident_flow_equals_host_pooled_rows(golden):
    eng = _engine(golden)
    structs = _structs(golden, n_synth=19)
    a, b = structs[:11], structs[11:]
    lc = cl.LatentClustering(128, n_components=8, cluster_dims=3, device=0)
    ref = cl.LatentClustering(128, n_components=8, cluster_dims=3, device=0)
    for part in (a, b):
        eng.evaluate(part)
        lc.append_resident(eng, model=0)
        emb = eng.embedding(0).astype(np.float64)
        off = np.cumsum([0] + [len(s[0]) for s in part])
        ref.append_rows(np.stack([emb[o:o + len(s[0])].sum(axis=0) / len(s[0]) for o, s in zip(off, part)]))
    assert lc.n_rows == ref.n_rows == len(structs)
    for k in (2, 5):
        assert np.array_equal(lc.fit(k, "maxclust"), ref.fit(k, "maxclust"))
    assert np.max(np.abs(lc.X_r_[:, :3] - ref.X_r_[:, :3])) <= 1e-9
    lc.clear()
    assert lc.n_rows == 0
    lc.close(); ref.close(); eng.close()


def test_two_runs_are_bit_identical():
    fx = co.load("pca_d128_n1000")
    X = fx["X"].astype(np.float64)
    out = []
    for _ in range(2):
        lc = cl.LatentClustering(128, device=0)
        lc.append_rows(X)
        lc.linkage()
        out.append((lc.Z_.tobytes(), lc.X_r_.tobytes()))
        lc.close()
    assert out[0] == out[1]


def test_kind_checks_without_a_device_fault(golden):
    eng = backend.ClusterEngine(3, n_components=1, cluster_dims=3)
    eng.set_points(np.random.default_rng(0).normal(size=(10, 3)))
    lib = eng._lib
    assert lib.vssr_batch_run(eng._h, 1) == -1
    assert lib.vssr_gmm_fit_clear(eng._h) == -1
    painn = _engine(golden)
    assert lib.vssr_cluster_clear(painn._h) == -1 and lib.vssr_cluster_pca(painn._h, None) == -1
    with pytest.raises(backend.BackendError, match="no completed PaiNN run"):
        backend.ClusterEngine(128).append_resident(painn)
    Z, _ = eng.linkage()                                   # both handles still work
    assert Z.shape == (9, 4)
    with pytest.raises(backend.BackendError, match="n_components"):
        e2 = backend.ClusterEngine(128, n_components=32)
        e2.append_rows(np.random.default_rng(1).normal(size=(20, 128)))
        e2.pca()
    painn.close(); eng.close()
