"""Gaussian-mixture uncertainty on the MI355X (csrc/gmm.hip through vssr_gmm_*): caller rows of every supported shape and
covariance type, the resident PaiNN embedding (atoms and structure means, every order) on the 128/20 fast path and the general-width
path, determinism, the state / argument errors, calculate_batch(uncertainty=...) and the clustering script's call pattern -- all
against the fp64 restatement tests/gmm_oracle.py."""
import numpy as np
import pytest
import torch

import gmm_oracle as go
from painn_shapes import reshape_ensemble
from surface_sampling_amd import backend, uncertainty as U

pytestmark = pytest.mark.gpu


def _close(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want) / (1.0 + np.abs(want))
    assert float(err.max()) <= 1e-9, f"{what}: max |d| / (1 + |NLL|) = {err.max():.3e}"


@pytest.mark.parametrize("D", [16, 48, 128, 256])
@pytest.mark.parametrize("K", [1, 5, 17])
def test_caller_rows_every_shape_and_covariance_type(K, D):
    rng = np.random.default_rng(K * 1000 + D)
    for cov in ("full", "tied", "diag", "spherical"):
        means, prec, w = go.random_gmm(K, D, cov, seed=K + D)
        P = go.expand(prec, cov, K, D)
        X = np.concatenate([
            means + 0.0,                                          # rows equal to a mean
            rng.normal(size=(150, D)),                            # ordinary rows (tail of a 64-row tile)
            means[:1] + 100.0 * rng.normal(size=(3, D)),          # outliers: NLL 1e4 .. 1e6, exp underflows for most components
        ])
        eng = backend.GMMEngine(means, P, w, device=0, log_2pi=go.LOG2PI_F32)
        nll, lp = eng.score_rows(X, log_prob=True)
        want = go.nll(X, means, P, w, go.LOG2PI_F32)
        _close(nll, want, f"K={K} D={D} {cov}")
        _close(lp, go.log_prob(X, means, P, go.LOG2PI_F32), f"log_prob K={K} D={D} {cov}")
        assert want.max() > 1e4
        # the same through GMMUncertainty(device="cuda")
        u = U.GMMUncertainty(device="cuda:0", covariance_type=cov, gm_model={"means_": means, "precisions_cholesky_": prec,
                                                                              "weights_": w, "covariance_type": cov})
        _close(u.negative_log_likelihood(X).numpy(), want, f"GMMUncertainty K={K} D={D} {cov}")
        eng.close()


def test_outliers_reach_1e5_and_one_row():
    D, K = 128, 5
    means, prec, w = go.random_gmm(K, D, "full", seed=11)
    X = means[2:3] + 60.0 * np.random.default_rng(0).normal(size=(1, D))
    eng = backend.GMMEngine(means, prec, w)
    want = go.nll(X, means, prec, w, go.LOG2PI_F32)
    assert want[0] > 1e5
    _close(eng.score_rows(X), want, "one outlier row")
    eng.close()


def _structs(golden, n_synth=6, seed=0):
    """Ragged batch: the committed SrTiO3 slabs, plus perturbed copies (synthetic chains of other sizes)."""
    names = ["SrTiO3_2x2_pristine", "O36Sr12Ti12", "O40Sr16Ti12", "O44Sr12Ti16", "SrTiO3_2x2x4_pristine"]
    out = [(golden.structure(n).numbers, golden.structure(n).positions, np.asarray(golden.structure(n).cell),
            np.asarray(golden.structure(n).pbc)) for n in names]
    rng = np.random.default_rng(seed)
    for i in range(n_synth):
        Z, pos, cell, pbc = out[i % len(names)]
        keep = np.sort(rng.choice(len(Z), size=len(Z) - 1 - 3 * i, replace=False))
        out.append((Z[keep], pos[keep] + rng.normal(scale=0.05, size=(len(keep), 3)), cell, pbc))
    return out


def _engine(golden, blobs=None, hp=None):
    table, const = golden.offset_table()
    return backend.PainnEngine(blobs or golden.blobs, device=0, offset_per_z=table, offset_const=const, hparams=hp)


def _check_resident(eng, structs, F, model):
    eng.evaluate(structs)
    emb = eng.embedding(model).astype(np.float64)                         # the download the oracle is applied to
    n_atoms = [len(s[0]) for s in structs]
    Zall = np.concatenate([s[0] for s in structs])
    means, prec, w = go.species_gmm(emb, Zall)
    means2, prec2, w2 = go.random_gmm(4, F, "full", seed=F, scale=float(np.abs(emb).mean()) + 0.1)
    for gm in ((means, prec, w), (np.concatenate([means, means2]), np.concatenate([prec, prec2]), np.concatenate([w, w2]))):
        g = backend.GMMEngine(*gm)
        want_rows = go.nll(emb, *gm, go.LOG2PI_F32)
        for order in go.ORDERS:
            nll, sysv = g.score_batch(eng, model=model, rows="atoms", order=order)
            _close(nll, want_rows, f"F={F} rows, {order}")
            if order == "atomic":
                assert sysv is None
                continue
            true = [go.system_val(want_rows[o:o + n], [n], order) for o, n in zip(np.cumsum([0] + n_atoms[:-1]), n_atoms)]
            _close(sysv, np.array(true, dtype=np.float64).reshape(-1), f"F={F} system {order}")
            _close(U.apply_padding_rule(sysv, n_atoms, order), go.system_val(want_rows, n_atoms, order), f"F={F} padded {order}")
        mrows = np.stack([emb[o:o + n].mean(axis=0) for o, n in zip(np.cumsum([0] + n_atoms[:-1]), n_atoms)])
        nll_m, sys_m = g.score_batch(eng, model=model, rows="mean", order="system_max")
        _close(nll_m, go.nll(mrows, *gm, go.LOG2PI_F32), f"F={F} mean rows")
        assert np.array_equal(sys_m, nll_m)
        # determinism: two identical calls, bit for bit
        a = g.score_batch(eng, model=model, rows="atoms", order="system_mean")
        b = g.score_batch(eng, model=model, rows="atoms", order="system_mean")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        g.close()


def test_resident_rows_fast_path(golden):
    eng = _engine(golden)
    _check_resident(eng, _structs(golden), 128, model=1)
    eng.close()


def test_resident_rows_general_width(golden):
    blobs, hp = reshape_ensemble(golden.blobs, 64, 16)
    eng = _engine(golden, blobs, hp)
    _check_resident(eng, _structs(golden, n_synth=3, seed=1), 64, model=0)
    eng.close()


def test_state_and_argument_errors(golden):
    eng = _engine(golden)
    means, prec, w = go.random_gmm(3, 128, seed=2)
    g = backend.GMMEngine(means, prec, w)
    Z, pos, cell, pbc = _structs(golden, n_synth=0)[0]
    rattled = pos + np.random.default_rng(5).normal(0, 0.15, pos.shape)
    s = [(Z, pos, cell, pbc), (Z, rattled, cell, pbc)]
    eng.upload(s)
    with pytest.raises(backend.BackendError, match="vssr error -5: no completed PaiNN run"):
        g.score_batch(eng)
    eng.run()
    g.score_batch(eng)
    f_a = np.linalg.norm(eng.download()["forces"][:len(Z)].astype(np.float64), axis=1).max()
    info = eng.relax("FIRE", max_steps=8, fmax=1.05 * f_a)   # chain 0 converged from the start: the graph is partial afterwards
    assert info["converged"][0] and not info["converged"][1]
    with pytest.raises(backend.BackendError, match="vssr error -5: .*last relaxation iteration"):
        g.score_batch(eng)
    eng.run()
    g.score_batch(eng)
    small = backend.GMMEngine(*go.random_gmm(2, 64, seed=3))
    with pytest.raises(backend.BackendError, match="vssr error -1: GMM dimension 64 differs from the PaiNN feat_dim 128"):
        small.score_batch(eng)
    # every other entry point refuses a GMM handle
    with pytest.raises(backend.BackendError, match="vssr error -1: vssr_batch_upload: a Gaussian-mixture handle"):
        backend.PainnEngine.upload(g, s)
    with pytest.raises(backend.BackendError, match="Gaussian-mixture handle"):
        backend.PainnEngine.run(g)
    with pytest.raises(backend.BackendError, match="Gaussian-mixture handle"):
        backend.PainnEngine.embedding(g)
    # ... and the vssr_gmm_* calls refuse every other handle
    with pytest.raises(backend.BackendError, match="not a GMM handle"):
        eng._check(eng._lib.vssr_gmm_score_batch(eng._h, eng._h, 0, 0, 0, None, None))
    with pytest.raises(backend.BackendError, match="not a PaiNN ensemble"):
        g._check(g._lib.vssr_gmm_score_batch(g._h, small._h, 0, 0, 0, None, None))
    for x in (small, g, eng):
        x.close()


def test_calculate_batch_uncertainty_equals_host_scoring(golden):
    from surface_sampling_amd import calculators as calcs
    from surface_sampling_amd.structures import Structure

    structs = _structs(golden, n_synth=2, seed=3)
    atoms = [Structure(Z, pos, cell, pbc) for Z, pos, cell, pbc in structs]
    calc = calcs.EnsembleNFFSurface(golden.blobs, device="cuda:0", properties=("energy", "forces", "embedding"))
    base = calc.calculate_batch(atoms)
    emb = np.concatenate([r["embedding"] for r in base]).astype(np.float64)
    means, prec, w = go.species_gmm(emb, np.concatenate([s[0] for s in structs]))
    gm = {"means_": means, "precisions_cholesky_": prec, "weights_": w, "covariance_type": "full"}
    n_atoms = [len(a) for a in atoms]
    for order, rows in (("atomic", "atoms"), ("system_max", "atoms"), ("system_mean_squared", "atoms"), ("system_mean", "mean")):
        u = U.GMMUncertainty(device="cpu", order=order, gm_model=gm, min_uncertainty=0.5)
        out = calc.calculate_batch(atoms, uncertainty=u, uncertainty_rows=rows)
        if rows == "mean":
            host = u({"embedding": np.stack([r["embedding"].astype(np.float64).mean(axis=0) for r in base])}, num_atoms=n_atoms)
        else:
            host = u({"embedding": emb}, num_atoms=n_atoms)
        host = host.numpy()
        got = np.concatenate([np.atleast_1d(r["uncertainty"]) for r in out])
        _close(got, host, f"calculate_batch {order} {rows}")
        assert out[0]["energy"] == base[0]["energy"]
    assert "uncertainty" not in base[0]


def test_clustering_call_pattern(golden, tmp_path):
    """scripts/clustering.py:204-255: Uncertainty.load(path), then unc(props, num_atoms=props["num_atoms"]) on one structure's
    flattened (mean) embedding, then .item()."""
    from surface_sampling_amd import calculators as calcs

    s = golden.structure("O40Sr16Ti12")
    single = calcs.EnsembleNFFSurface(golden.blobs[:1], device="cuda:0", properties=("energy", "forces", "embedding"))
    single.set(offset=True, offset_data=golden.offset_data, chem_pots={"Sr": -2, "Ti": 0, "O": 0})
    res = calcs.get_results_single(s, single)
    emb = calcs.get_embeddings_single(s, single, results_cache=res, flatten=True, flatten_axis=0)
    means, prec, w = go.species_gmm(res["embedding"].astype(np.float64), s.numbers)
    path = tmp_path / "gmm_unc.pkl"
    U.GMMUncertainty(order="system_mean", gm_model={"means_": means, "precisions_cholesky_": prec, "weights_": w},
                     calibrate=True, cp_alpha=0.05, min_uncertainty=0.1).save(str(path))
    d = U.load_pickle(str(path))
    d["unc_params"]["qhat"] = 1.3
    import pickle

    path.write_bytes(pickle.dumps(d))
    gmm_model = U.Uncertainty.load(str(path))
    props = {"embedding": emb, "num_atoms": torch.tensor([len(s)])}
    value = gmm_model(props, num_atoms=props["num_atoms"]).detach().cpu().numpy().item()
    want = go.uncertainty(emb.astype(np.float64).reshape(1, -1), (means, prec, w), "system_mean", [len(s)], 0.1, 1.3)
    _close(value, float(np.asarray(want).reshape(-1)[0]), "clustering pattern")
