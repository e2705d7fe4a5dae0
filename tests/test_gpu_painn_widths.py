"""GPU (-m gpu): PaiNN ensembles of other feature widths and radial-basis sizes, served by the general-width fp32 path
(painn_gen.hip), against the fp64 oracle, the committed vectors and the 128 / 20 path.

Test models: the shipped SrTiO3 weights cut / padded to the shape (tests/painn_shapes.py).  Contract of the suite: |dE| <= 1e-4 eV,
max|dF| <= 2e-4 eV/A, |d std| <= 2e-4.  Where a structure misses it (large chains: plain fp32 sums over ~1e3 atoms), the device
deviation must stay within twice the oracle's own fp32 deviation on the same structure (_check).

Measured on an MI355X (profiles/r08/test_gpu_painn_widths_deviations.log): every structure met the contract.  Largest device
deviations over F = 16..256 on the 60-76 atom slabs: 2.3e-5 eV, 1.3e-4 eV/A (F = 256, R = 32), std 1.6e-5; the oracle's own fp32
run on the same structures: up to 2.9e-5 eV, 1.8e-4 eV/A.  1 080-atom chain (F = 64): 3.8e-5 eV (oracle fp32 8.1e-5), 1.3e-6 eV/A.
"""
import os

import numpy as np
import pytest

from painn_config_cases import E_TOL, F_TOL, STD_TOL, check
from painn_shapes import checkpoint_bytes, reshape_ensemble

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8), (32, 12), (64, 16), (96, 20), (192, 24), (256, 32)]


def _arrays(s):
    return (s.numbers, s.positions, s.cell, s.pbc)


def _engine(golden, blobs, hp, general=False):
    from surface_sampling_amd import backend

    table, const = golden.offset_table()
    old = os.environ.get("VSSR_PAINN_PATH")
    if general:
        os.environ["VSSR_PAINN_PATH"] = "general"
    try:
        return backend.PainnEngine(blobs, device=0, offset_per_z=table, offset_const=const, hparams=hp)
    finally:
        if general:
            if old is None:
                os.environ.pop("VSSR_PAINN_PATH", None)
            else:
                os.environ["VSSR_PAINN_PATH"] = old


def _ohp(oracle_mod, hp):
    return oracle_mod.default_hparams(feat_dim=hp["feat_dim"], n_rbf=hp["n_rbf"], num_conv=hp["num_conv"],
                                      readout_hidden=hp["readout_hidden"])


def _check(golden, oracle_mod, blobs, hp, s, e, f, std, tag=""):
    """Device results of one structure against the fp64 oracle (the rule of painn_config_cases.check); returns (dE, dF, dstd)."""
    return check(golden, oracle_mod, blobs, _ohp(oracle_mod, hp), s, e, f, std, tag)


def test_forced_general_path_on_the_shipped_ensemble(golden, oracle_mod):
    """VSSR_PAINN_PATH=general at 128 / 20: the committed fp64 vectors, the KAT energies, and the fast path (energies, forces,
    stress, embeddings) within the contract."""
    from surface_sampling_amd import structures

    hp = {"feat_dim": 128, "n_rbf": 20}
    gen = _engine(golden, golden.blobs, hp, general=True)
    fast = _engine(golden, golden.blobs, hp)
    f = golden.fine
    for name in ("S240", "chain17"):
        r = gen.evaluate([(f[f"{name}.numbers"], f[f"{name}.positions"], f[f"{name}.cell"], f[f"{name}.pbc"])])
        assert abs(float(r["energy_f64"][0]) - float(f[f"{name}.energy"])) <= E_TOL, name
        assert np.abs(r["forces"] - f[f"{name}.forces"]).max() <= F_TOL, name
        assert abs(float(r["energy_std"][0]) - float(f[f"{name}.energy_std"])) <= STD_TOL, name
    tol = golden.kat["tolerance"]
    for case in golden.kat["painn_ensemble"]:
        r = gen.evaluate([_arrays(golden.structure(case["structure"]))])
        assert abs(float(r["energy"][0]) - case["energy"]) <= tol["energy_abs"], case["structure"]
    base = golden.structure("SrTiO3_2x2_pristine")
    batch = [_arrays(structures.synth_chain(base, c)) for c in (0, 7, 19)] + [_arrays(golden.structure("O44Sr12Ti16"))]
    a, b = gen.evaluate(batch), fast.evaluate(batch)
    assert np.abs(a["energy_f64"] - b["energy_f64"]).max() <= E_TOL
    assert np.abs(a["forces"] - b["forces"]).max() <= F_TOL
    assert np.abs(a["energy_std"] - b["energy_std"]).max() <= STD_TOL
    sa, sb = gen.stress()[0], fast.stress()[0]
    assert np.abs(sa - sb).max() <= 1e-6      # eV/A^3
    ea, eb = gen.embedding(), fast.embedding()
    assert ea.shape == eb.shape == (3, sum(len(x[0]) for x in batch), 128)
    # final scalar state: the general path against the fp64 oracle at the bound of test_embedding_is_the_final_scalar_state,
    # and the two paths against each other at 1e-5 relative (measured: 2.3e-4 absolute at |s| <= 192, i.e. 1.2e-6 relative)
    z, pos, cell, pbc = batch[3]
    a0 = sum(len(x[0]) for x in batch[:3])
    for m, blob in enumerate(golden.blobs):
        _, _, d = oracle_mod.painn(blob, z, pos, cell, pbc, 64, dump=True)
        ref = d["s_upd"][2]
        assert np.abs(ea[m, a0:] - ref).max() <= 1e-4 * max(1.0, float(np.abs(ref).max())), m
    scale = max(1.0, float(np.abs(eb).max()))
    print(f"embedding general vs fast at 128 / 20: max |d| {float(np.abs(ea - eb).max()):.2e} (scale {scale:.1f})")
    assert np.abs(ea - eb).max() <= 1e-5 * scale
    assert not gen.saturated().any()
    gen.close()
    fast.close()


@pytest.mark.parametrize("F,R", SHAPES)
def test_cut_and_padded_models_match_the_oracle(golden, oracle_mod, F, R):
    """Fails on the 128 / 20-only backend (PainnEngine raised BackendError for every other shape)."""
    from surface_sampling_amd import structures

    blobs, hp = reshape_ensemble(golden.blobs, F, R)
    eng = _engine(golden, blobs, hp)
    base = golden.structure("SrTiO3_2x2_pristine")
    slabs = [base, golden.structure("O40Sr16Ti12"), structures.synth_chain(base, 4), structures.synth_chain(base, 13)]
    res = eng.evaluate([_arrays(s) for s in slabs])
    cs = res["cfg_start"]
    for b, s in enumerate(slabs):
        _check(golden, oracle_mod, blobs, hp, s, float(res["energy_f64"][b]), res["forces"][cs[b]:cs[b + 1]],
               float(res["energy_std"][b]), (F, R, b))
    assert not eng.saturated().any()
    eng.close()


@pytest.mark.parametrize("L,H", [(1, 64), (2, 64), (4, 64), (3, 32)])
def test_f64_other_depths_and_readout_width(golden, oracle_mod, L, H):
    from surface_sampling_amd import structures

    blobs, hp = reshape_ensemble(golden.blobs, 64, 16, num_conv=L, readout_hidden=H)
    eng = _engine(golden, blobs, hp)
    base = golden.structure("SrTiO3_2x2_pristine")
    slabs = [base, structures.synth_chain(base, 9)]
    res = eng.evaluate([_arrays(s) for s in slabs])
    cs = res["cfg_start"]
    for b, s in enumerate(slabs):
        _check(golden, oracle_mod, blobs, hp, s, float(res["energy_f64"][b]), res["forces"][cs[b]:cs[b + 1]],
               float(res["energy_std"][b]), (L, H, b))
    eng.close()


def test_ragged_batch_lone_atom_small_large_and_periodic_images(golden, oracle_mod):
    """One engine: a lone atom (zero forces), chains of 3 and 5 atoms, ~260 atoms, > 1 000 atoms and a cell with nimg >= 2.
    Every chain gives bit for bit what it gives alone."""
    from cell_cases import battery

    from surface_sampling_amd import structures

    blobs, hp = reshape_ensemble(golden.blobs, 64, 16)
    eng = _engine(golden, blobs, hp)
    base = golden.structure("SrTiO3_2x2_pristine")
    big = base.repeat((3, 3, 2))
    big.positions = big.positions + np.random.default_rng(5).normal(0, 0.03, big.positions.shape)
    skew = [c for c in battery() if c.name == "sto_slab_skewed"][0]
    sk = structures.Structure(skew.numbers, skew.pos, skew.cell, skew.pbc.astype(np.uint8))
    lone = structures.Structure(np.array([8], np.int32), np.zeros((1, 3)), np.eye(3) * 30.0, np.zeros(3, np.uint8))
    tri = structures.Structure(np.array([8, 22, 8], np.int32), np.array([[0, 0, 0], [1.9, 0, 0], [3.8, 0.2, 0]], float),
                               np.eye(3) * 30.0, np.zeros(3, np.uint8))
    five = structures.Structure(np.array([38, 8, 8, 22, 8], np.int32),
                                np.array([[0, 0, 0], [2.0, 0, 0], [0, 2.1, 0], [2.0, 2.0, 0.3], [1.0, 1.0, 1.9]], float),
                                np.eye(3) * 30.0, np.zeros(3, np.uint8))
    chains = [lone, tri, structures.synth_chain(base, 21), big, five, sk]
    assert len(big) > 1000
    res = eng.evaluate([_arrays(s) for s in chains])
    cs = res["cfg_start"]
    assert np.abs(res["forces"][cs[0]:cs[1]]).max() == 0.0
    for b, s in enumerate(chains):
        alone = eng.evaluate([_arrays(s)])
        assert alone["energy_f64"][0] == res["energy_f64"][b], b
        assert np.array_equal(alone["forces"], res["forces"][cs[b]:cs[b + 1]]), b
        _check(golden, oracle_mod, blobs, hp, s, float(res["energy_f64"][b]), res["forces"][cs[b]:cs[b + 1]],
               float(res["energy_std"][b]), b)
    eng.close()


def test_energy_only_and_repeated_runs_are_bitwise_identical(golden):
    from surface_sampling_amd import backend, structures

    blobs, hp = reshape_ensemble(golden.blobs, 96, 20)
    eng = _engine(golden, blobs, hp)
    base = golden.structure("SrTiO3_2x2_pristine")
    chains = [_arrays(structures.synth_chain(base, c)) for c in range(5)]
    a, b = eng.evaluate(chains), eng.evaluate(chains)
    for k in ("energy", "energy_f64", "forces", "energy_std", "forces_std"):
        assert np.array_equal(a[k], b[k]), k
    e = eng.evaluate(chains, want=backend.WANT_ENERGY)
    assert np.array_equal(e["energy"], a["energy"]) and np.array_equal(e["energy_f64"], a["energy_f64"])
    eng.close()


def test_forces_are_minus_the_energy_gradient(golden):
    """Central differences of the device energy (fp64 output word) on a few atoms, h = 5e-3 A."""
    blobs, hp = reshape_ensemble(golden.blobs, 32, 12)
    eng = _engine(golden, blobs, hp)
    s = golden.structure("SrTiO3_2x2_pristine")
    f0 = eng.evaluate([_arrays(s)])["forces"]
    h = 5e-3
    for atom in (3, 22, 41):
        for x in range(3):
            e = []
            for sign in (1, -1):
                p = s.positions.copy()
                p[atom, x] += sign * h
                e.append(float(eng.evaluate([(s.numbers, p, s.cell, s.pbc)])["energy_f64"][0]))
            fd = -(e[0] - e[1]) / (2 * h)
            assert abs(fd - float(f0[atom, x])) <= 3e-3, (atom, x, fd, float(f0[atom, x]))
    eng.close()


def test_embedding_is_the_final_scalar_state(golden, oracle_mod):
    blobs, hp = reshape_ensemble(golden.blobs, 64, 16)
    eng = _engine(golden, blobs, hp)
    s = golden.structure("O36Sr12Ti12")
    eng.evaluate([_arrays(s)])
    emb = eng.embedding()
    assert emb.shape == (3, len(s), 64)
    assert np.array_equal(eng.embedding(model=1), emb[1])
    for m, blob in enumerate(blobs):
        _, _, d = oracle_mod.painn(blob, s.numbers, s.positions, s.cell, s.pbc, 64, dump=True, hp=_ohp(oracle_mod, hp))
        ref = d["s_upd"][hp["num_conv"] - 1]
        assert np.abs(emb[m] - ref).max() <= 1e-4 * max(1.0, float(np.abs(ref).max())), m
    eng.close()


def test_lockstep_relaxations_with_a_64_feature_ensemble(golden, oracle_mod):
    from conftest import top_layer

    from surface_sampling_amd.calculators import EnsembleNFFSurface

    blobs, hp = reshape_ensemble(golden.blobs, 64, 16)
    table, const = golden.offset_table()
    slabs = [golden.structure("SrTiO3_2x2_pristine"), golden.structure("O36Sr12Ti12")]
    mask = np.concatenate([np.isin(np.arange(len(s)), top_layer(s), invert=True) for s in slabs]).astype(np.uint8)
    for method in ("bfgs", "fire"):
        eng = _engine(golden, blobs, hp)
        eng.upload([_arrays(s) for s in slabs])
        info = getattr(eng, f"relax_{method}")(fixed=mask, max_steps=300, fmax=0.05)
        res = eng.download()
        cs = res["cfg_start"]
        assert info["converged"].all(), (method, info["n_steps"])
        for b, s in enumerate(slabs):
            p = info["positions"][cs[b]:cs[b + 1]]
            ref = oracle_mod.ensemble(blobs, s.numbers, p, s.cell, s.pbc, 64, table, const, hp=_ohp(oracle_mod, hp))
            assert abs(float(res["energy_f64"][b]) - ref["energy"]) <= E_TOL, (method, b)
            assert np.linalg.norm(ref["forces"][top_layer(s)], axis=1).max() <= 0.05 + 1e-3
        eng.close()
    calc = EnsembleNFFSurface(blobs, device="cuda:0", hparams=hp)
    calc.set(offset=True, offset_data=golden.offset_data)
    s = slabs[0]
    fixed = np.setdiff1d(np.arange(len(s)), top_layer(s))
    out = calc.relax_batch([s, s.copy()], fixed_indices=[fixed, fixed], relax_steps=300, fmax=0.05)
    (slab, _, energy, _, r), (_, _, energy2, _, _) = out
    assert energy == energy2 and r["n_steps"] < 300
    ref = oracle_mod.ensemble(blobs, slab.numbers, slab.positions, slab.cell, slab.pbc, 64, table, const, hp=_ohp(oracle_mod, hp))
    assert abs(energy - ref["energy"]) <= E_TOL


@pytest.mark.parametrize("bad", [{"feat_dim": 100}, {"n_rbf": 40}])
def test_unsupported_shapes_raise_naming_the_accepted_set(golden, bad):
    from surface_sampling_amd import backend

    with pytest.raises(backend.BackendError, match=r"multiple of 16 in 16\.\.256 and n_rbf in 1\.\.32"):
        _engine(golden, golden.blobs, bad)


def test_auto_hparams_from_a_64_feature_checkpoint(golden, oracle_mod, tmp_path):
    from surface_sampling_amd.calculators import EnsembleNFFSurface

    blobs, hp = reshape_ensemble(golden.blobs, 64, 16)
    paths = []
    for m, b in enumerate(blobs):
        d = tmp_path / f"model0{m + 1}"
        d.mkdir()
        (d / "best_model").write_bytes(checkpoint_bytes(b, hp))
        (d / "params.json").write_text('{"feat_dim": 64, "n_rbf": 16, "num_conv": 3, "cutoff": 5.0}')
        paths.append(str(d / "best_model"))
    calc = EnsembleNFFSurface(paths, device="cuda:0", hparams="auto")
    assert calc.hparams["feat_dim"] == 64 and calc.hparams["n_rbf"] == 16
    calc.set(offset=True, offset_data=golden.offset_data)
    s = golden.structure("SrTiO3_2x2_pristine")
    calc.calculate(s, properties=("energy", "forces"))
    table, const = golden.offset_table()
    ref = oracle_mod.ensemble(blobs, s.numbers, s.positions, s.cell, s.pbc, 64, table, const, hp=_ohp(oracle_mod, hp))
    assert abs(float(np.ravel(calc.results["energy"])[0]) - ref["energy"]) <= E_TOL
    assert np.abs(np.asarray(calc.results["forces"]) - ref["forces"]).max() <= F_TOL
