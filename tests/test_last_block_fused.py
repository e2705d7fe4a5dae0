"""GPU (-m gpu): the last update block's forward pass inside its reverse kernel (k_update_bwd_mfma, mode 3).

With forces wanted, update_fwd(L - 1) is not launched: the reverse kernel of the last layer runs the block's forward pass itself,
writes the final scalar features, evaluates the readout and goes on with the adjoints.  Energy-only evaluations keep update_fwd<2> +
k_readout_mfma, so the two kinds of evaluation are two implementations of the same forward pass and must agree bit for bit.
"""
import numpy as np
import pytest

from painn_shapes import reshape_blob

pytestmark = pytest.mark.gpu

E_TOL, F_TOL = 1e-4, 2e-4   # eV, eV/A: GPU fp32 vs the fp64 oracle (tests/test_gpu_parity.py)


def _arrays(s):
    return (s.numbers, s.positions, s.cell, s.pbc)


def _engine(golden, blobs=None, **kw):
    from surface_sampling_amd import backend

    table, const = golden.offset_table()
    return backend.PainnEngine(golden.blobs if blobs is None else blobs, device=0, offset_per_z=table, offset_const=const, **kw)


@pytest.fixture(scope="module")
def engine(golden):
    eng = _engine(golden)
    yield eng
    eng.close()


def _ragged(golden):
    """The four chains of test_batched_ragged_chains_vs_oracle_and_vs_single: 3 x 240 + 68 atoms, no multiple of 32, chain
    boundaries inside atom tiles."""
    from surface_sampling_amd import structures

    big = golden.structure("SrTiO3_2x2_pristine").repeat((2, 2, 1))
    return [structures.synth_chain(big, c) for c in (0, 7, 24)] + [golden.structure("O40Sr16Ti12")]


@pytest.mark.parametrize("case", ["slab60", "ragged"])
def test_forces_run_and_energy_only_run_agree_bit_for_bit(golden, engine, case):
    """slab60: two atom tiles, the second with 28 real rows.  ragged: see _ragged."""
    from surface_sampling_amd import backend

    chains = [golden.structure("SrTiO3_2x2_pristine")] if case == "slab60" else _ragged(golden)
    assert case != "ragged" or sum(len(s) for s in chains) % 32 != 0
    batch = [_arrays(s) for s in chains]
    full = engine.evaluate(batch)
    emb_full = engine.embedding()
    s_upd_full = engine.debug_read("s_upd2", 1)
    e_only = engine.evaluate(batch, want=backend.WANT_ENERGY | backend.WANT_STD | backend.WANT_PER_MODEL)
    emb_e = engine.embedding()
    s_upd_e = engine.debug_read("s_upd2", 1)
    assert np.isfinite(full["forces"]).all() and np.abs(full["forces"]).max() > 0
    for k in ("energy", "energy_std", "energy_models", "energy_f64", "energy_std_f64", "energy_models_f64"):
        assert np.array_equal(full[k], e_only[k]), k
    assert emb_full.shape == (3, sum(len(s) for s in chains), 128)
    assert np.array_equal(emb_full, emb_e)
    assert np.array_equal(s_upd_full, s_upd_e) and np.array_equal(s_upd_full, emb_full[1].reshape(-1))


@pytest.mark.parametrize("num_conv", [1, 2, 3])
def test_model_depths_against_the_oracle(golden, oracle_mod, num_conv):
    """The fused kernel serves whatever layer is the last one: the factorised layer 0 (num_conv = 1) as well as layers >= 1."""
    from surface_sampling_amd import structures

    cut = [reshape_blob(b, 128, 20, num_conv=num_conv, seed=m) for m, b in enumerate(golden.blobs)]
    blobs, hp = [c[0] for c in cut], cut[0][1]
    assert hp["num_conv"] == num_conv
    eng = _engine(golden, blobs, hparams=hp)
    ohp = oracle_mod.default_hparams(feat_dim=128, n_rbf=20, num_conv=num_conv, readout_hidden=64)
    table, const = golden.offset_table()
    base = golden.structure("SrTiO3_2x2_pristine")
    chains = [base, structures.synth_chain(base, 5)]
    res = eng.evaluate([_arrays(s) for s in chains])
    cs = res["cfg_start"]
    for b, s in enumerate(chains):
        ref = oracle_mod.ensemble(blobs, s.numbers, s.positions, s.cell, s.pbc, 64, table, const, hp=ohp)
        f = res["forces"][cs[b]:cs[b + 1]]
        de, df = abs(float(res["energy_f64"][b]) - ref["energy"]), float(np.abs(f - ref["forces"]).max())
        print(f"num_conv={num_conv} chain {b}: dE {de:.2e} dF {df:.2e}")
        assert de <= E_TOL and df <= F_TOL, (num_conv, b, de, df)
        single = eng.evaluate([_arrays(s)])
        assert float(single["energy"][0]) == float(res["energy"][b])
        assert np.array_equal(single["forces"], f)
    assert not eng.saturated().any()
    eng.close()


def test_default_engine_vs_stored_intermediates_engine(golden, engine, monkeypatch):
    """VSSR_UPD_SAVE=1 keeps update_fwd(L - 1) and the reverse kernel that loads its intermediates.  Both engines differentiate
    the forward kernel's values now; what is left between them is the summation order of the adjoints' producers (fp32
    rounding): the bound of test_stored_forward_intermediates_give_identical_results."""
    monkeypatch.setenv("VSSR_UPD_SAVE", "1")
    saved = _engine(golden)
    monkeypatch.delenv("VSSR_UPD_SAVE")
    batch = [_arrays(s) for s in _ragged(golden)]
    r1, r0 = saved.evaluate(batch), engine.evaluate(batch)
    saved.close()
    for k in ("energy", "energy_std", "energy_models", "energy_f64"):
        assert np.array_equal(r1[k], r0[k]), k
    df, ds = np.abs(r1["forces"] - r0["forces"]).max(), np.abs(r1["forces_std"] - r0["forces_std"]).max()
    print(f"default vs VSSR_UPD_SAVE=1: max|dF| {df:.2e} max|dF_std| {ds:.2e}")
    assert df <= 2e-5 and ds <= 2e-5


def test_masked_chain_in_lock_step_fire(golden, engine):
    """The fire_masked recipe of tools/dump_painn.py: two chains in lock-step FIRE, the first held fixed entirely, so the last
    evaluations run under an active mask that switches its atom tiles off.  The moving chain must not notice its neighbour, and the
    frozen chain keeps the results of its (unrelaxed) positions."""
    from surface_sampling_amd import structures

    base = golden.structure("SrTiO3_2x2_pristine")
    frozen, moving = structures.synth_chain(base, 2, grid=(4, 4)), golden.structure("O44Sr12Ti16")
    n0, n1 = len(frozen), len(moving)
    fixed1 = (np.arange(n1) % 4 == 0).astype(np.uint8)
    engine.upload([_arrays(frozen), _arrays(moving)])
    out = engine.relax("FIRE", fixed=np.concatenate([np.ones(n0, np.uint8), fixed1]), max_steps=6, fmax=0.01)
    both = engine.download()
    engine.upload([_arrays(moving)])
    out1 = engine.relax("FIRE", fixed=fixed1, max_steps=6, fmax=0.01)
    alone = engine.download()
    assert np.array_equal(np.asarray(out["positions"])[n0:], np.asarray(out1["positions"]))
    assert not np.array_equal(np.asarray(out1["positions"]), moving.positions)   # it did move
    for k in ("energy", "energy_std", "energy_f64"):
        assert both[k][1] == alone[k][0], k
    assert np.array_equal(both["energy_models"][1], alone["energy_models"][0])
    assert np.array_equal(both["forces"][n0:], alone["forces"]) and np.array_equal(both["forces_std"][n0:], alone["forces_std"])
    still = engine.evaluate([_arrays(frozen)])
    assert np.array_equal(np.asarray(out["positions"])[:n0], frozen.positions)
    for k in ("energy", "energy_std", "energy_f64"):
        assert both[k][0] == still[k][0], k
    assert np.array_equal(both["forces"][:n0], still["forces"])


@pytest.mark.parametrize("what", ["embed", "last_V"])
def test_saturation_is_reported_by_a_forces_evaluation(golden, what):
    """embed: the embedding table doubled, the input of test_precision_envelope_of_the_fp16_split that leaves the fp16-split
    range.  last_V: only the last block's V matrix scaled by 1e6, so that the first value beyond +-65504 is that block's |V v|
    (shipped activations peak at ~160): a forward intermediate no kernel but the fused one splits in a forces evaluation."""
    from surface_sampling_amd import backend, checkpoint, structures

    s = structures.synth_chain(golden.structure("SrTiO3_2x2_pristine"), 3, grid=(4, 4))
    blobs = []
    for b in golden.blobs:
        b = b.copy()
        f = checkpoint.blob_to_fields(b)
        if what == "embed":
            f["embed"] *= 2.0
        else:
            f["upd2.V"] *= 1e6
        blobs.append(b)
    eng = backend.PainnEngine(blobs, device=0, model_units_per_ev=1.0)
    r = eng.evaluate([_arrays(s)])
    e = eng.evaluate([_arrays(s)], want=backend.WANT_ENERGY)
    eng.close()
    assert r["saturated"].all(), "a forces evaluation clamped values beyond +-65504 without raising the saturation flag"
    assert e["saturated"].all()
