"""GPU (-m gpu): the PaiNN paths at every depth, ensemble size, cutoff, repulsion, embedding-table length and readout width that
vssr_create accepts, against the fp64 oracle (case table, models and acceptance rule: tests/painn_config_cases.py; the table is
pinned on the CPU by tests/test_painn_config_cpu.py).

Accepted: inside the contract of tests/test_gpu_parity.py (|dE| <= 1e-4 eV, max |dF| <= 2e-4 eV/A, |d std| <= 2e-4, forces_std at
2e-4), or -- only for the cases of BEYOND_CONTRACT (cutoff 6.0 A) -- within twice the oracle's own fp32 deviation on the same
structure.  Every case is evaluated twice on its engine and must give the same bits.  Measured deviations:
profiles/r39/NOTES_painn_config.md.
"""
import numpy as np
import pytest

import painn_config_cases as pc

pytestmark = pytest.mark.gpu

KEYS = ("energy", "energy_f64", "forces", "energy_std", "forces_std", "energy_models")
KNOBS = {"8-feature": {"VSSR_EDGE_FS16_MAX": "0"}, "4-feature": {"VSSR_EDGE_FS16_MAX": "0", "VSSR_EDGE_FS8_MAX": "0"},
         "per-edge-layer-0": {"VSSR_L0_FACTORISE": "0"}, "gather": {"VSSR_EDGE_IMPL": "gather"}}
# the 72-atom chain leaves the 16-feature class, the 60-atom slab stays: two slice classes in one batch
MIXED_KNOBS = {"16+8-feature": {"VSSR_EDGE_FS16_MAX": "64"}, "16+4-feature": {"VSSR_EDGE_FS16_MAX": "64", "VSSR_EDGE_FS8_MAX": "64"}}


def _engine(golden, case, monkeypatch=None, env=None, cutoff=None, hparams=None, blobs=None):
    """A PainnEngine of the case; ``env``: knobs set while the engine is created (the library reads them at create)."""
    from surface_sampling_amd import backend

    table, const = case.offset(golden)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        return backend.PainnEngine(case.blobs(golden) if blobs is None else blobs, device=0, cutoff=case.cutoff if cutoff is None else cutoff,
                                   offset_per_z=table, offset_const=const, hparams={**case.engine_hp(), **(hparams or {})})
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k)


def _run(golden, oracle_mod, case, eng, tag=""):
    """Evaluate the case's structures in one batch, twice (same bits), and judge every structure against the fp64 oracle."""
    ss = [pc.structure(golden, n) for n in case.structs]
    res = eng.evaluate([pc.arrays(s) for s in ss])
    again = eng.evaluate([pc.arrays(s) for s in ss])
    for k in KEYS:
        assert np.array_equal(res[k], again[k]), (case.id, tag, k)
    assert np.isfinite(res["energy"]).all() and np.isfinite(res["forces"]).all() and not res["saturated"].any()
    cs = res["cfg_start"]
    for b, (n, s) in enumerate(zip(case.structs, ss)):
        refs = [pc.reference(golden, oracle_mod, case, n, bits) for bits in (64, 32)]
        pc.check(golden, oracle_mod, None, None, s, float(res["energy_f64"][b]), res["forces"][cs[b]:cs[b + 1]], float(res["energy_std"][b]),
                 f"{case.id} {tag} {n}".replace("  ", " "), fstd=res["forces_std"][cs[b]:cs[b + 1]], beyond=case.id in pc.BEYOND_CONTRACT,
                 refs=refs)
    return res


def _good_engine_still_evaluates(golden):
    """After a refusal: the shipped configuration on a fresh engine gives the committed energy of the pristine slab."""
    eng = _engine(golden, pc.Case("shipped", "depth", ("base",)))
    ok = eng.evaluate([pc.arrays(pc.structure(golden, "base"))])
    eng.close()
    assert abs(float(ok["energy"][0]) - (-467.5219)) < 1e-3


# ---- 1: every row of the table on the default path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_every_case_matches_the_oracle_and_energy_only_gives_the_same_energies(golden, oracle_mod, case):
    """The energy-only evaluation runs other kernels than the energy-and-forces one at depth 1 (stand-alone update + readout instead
    of the fused forward + readout + reverse kernel) and at H != 64: the energies must be the same bits."""
    from surface_sampling_amd import backend

    eng = _engine(golden, case)
    res = _run(golden, oracle_mod, case, eng)
    e_only = eng.evaluate([pc.arrays(pc.structure(golden, n)) for n in case.structs], want=backend.WANT_ENERGY)
    assert np.array_equal(e_only["energy"], res["energy"]) and np.array_equal(e_only["energy_f64"], res["energy_f64"])
    assert res["energy_models"].shape == (len(case.structs), case.M)
    eng.close()


# ---- 2: depth x slice class ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
@pytest.mark.parametrize("case", pc.DEPTH_CASES, ids=lambda c: c.id)
def test_depths_on_every_slice_class_and_fallback_path(golden, oracle_mod, monkeypatch, case, knobs):
    """Depths 1, 2 and 4 on the 8- and 4-feature slices, with the per-edge layer 0 (at depth 1 the layer-0 gather kernel is the
    last layer: its only way to run with accumulate = 0) and on the gather kernels; the default classes are check 1."""
    eng = _engine(golden, case, monkeypatch, KNOBS[knobs])
    _run(golden, oracle_mod, case, eng, knobs)
    eng.close()


def _knob_pairs():
    """Ensemble sizes and cutoffs on every slice class (the model count is a grid dimension, the cutoff sets the row lengths and the
    fp16-split radial tables); those, the repulsion cases and the 39-row embedding table on the per-edge layer 0 and the gather
    kernels, which evaluate the envelope and (sigma / d)^p on their own (powf) and index the embedding table by Z."""
    out = []
    for c in pc.BOTH_PATH_CASES + [pc.BY_ID["embed-39"]]:
        for k in KNOBS:
            if k in ("per-edge-layer-0", "gather") or c.axis in ("models", "cutoff"):
                out.append(pytest.param(c, k, id=f"{c.id}-{k}"))
    return out


@pytest.mark.parametrize("case,knobs", _knob_pairs())
def test_ensemble_cutoff_repulsion_and_embedding_cases_off_the_default_kernels(golden, oracle_mod, monkeypatch, case, knobs):
    eng = _engine(golden, case, monkeypatch, KNOBS[knobs])
    _run(golden, oracle_mod, case, eng, knobs)
    eng.close()


@pytest.mark.parametrize("knobs", list(MIXED_KNOBS), ids=list(MIXED_KNOBS))
@pytest.mark.parametrize("case", pc.MIXED_CASES, ids=lambda c: c.id)
def test_batches_that_mix_slice_classes_reduce_every_layer_set(golden, oracle_mod, monkeypatch, case, knobs):
    """A 60-atom slab on 16-feature slices next to a 72-atom chain on 8- or 4-feature slices: the partial edge gradients are reduced
    chain by chain (uni = 0) over one (depth 2) and three (depth 4) layer sets.  Every chain gives what it gives alone."""
    eng = _engine(golden, case, monkeypatch, MIXED_KNOBS[knobs])
    res = _run(golden, oracle_mod, case, eng, knobs)
    cs = res["cfg_start"]
    for b, n in enumerate(case.structs):
        alone = eng.evaluate([pc.arrays(pc.structure(golden, n))])
        assert alone["energy_f64"][0] == res["energy_f64"][b], n
        assert np.array_equal(alone["forces"], res["forces"][cs[b]:cs[b + 1]]), n
    eng.close()


# ---- 3: depth x readout: rows of the table (readout-32-depth1 / -depth2 / -depth4, check 1): reverse update kernel in mode 0 and the
# stand-alone reverse message MLP at depths 1, 2 and 4


@pytest.mark.parametrize("order", [(2,), (0, 2), (0, 1, 1, 2)], ids=["depth1", "depth2", "depth4"])
def test_launch_counts_show_the_kernels_each_depth_and_readout_width_takes(golden, monkeypatch, order):
    """The per-class profiler counts one launch group per layer and kernel class: the control flow of painn_run the cases above rely
    on (last block fused into its reverse kernel only with forces and H = 64, stand-alone readout and reverse message MLP at
    H = 32, per-edge layer 0 on request) is the one that ran."""
    from surface_sampling_amd import backend

    L = len(order)
    s = pc.arrays(pc.structure(golden, "base"))
    zero = ("embed", "message_mlp", "readout", "message_mlp_bwd")

    def counts(eng, want):
        eng.upload([s])
        eng.profile_enable(True)
        eng.profile_reset()
        eng.run(want)
        eng.synchronize()
        return {k: v["launches"] for k, v in eng.profile_read().items()}

    def expect(got, **want):
        for k, v in want.items():
            assert got.get(k, 0) == v, (L, k, got)

    fused = _engine(golden, pc.Case("fused", "depth", ("base",), order=order))
    expect(counts(fused, backend.WANT_ALL), layer0_factorised_fwd=1, edge_message_fwd=L - 1, update_fwd=L - 1, update_bwd=L,
           edge_message_bwd=L - 1, layer0_factorised_bwd=1, finalize=1, **dict.fromkeys(zero, 0))
    expect(counts(fused, backend.WANT_ENERGY), layer0_factorised_fwd=1, edge_message_fwd=L - 1, update_fwd=L, readout=1, update_bwd=0,
           edge_message_bwd=0, layer0_factorised_bwd=0)
    fused.close()
    h32 = _engine(golden, pc.Case("unfused", "readout", ("base",), order=order, H=32))
    expect(counts(h32, backend.WANT_ALL), update_fwd=L, readout=1, update_bwd=L, message_mlp_bwd=L - 1, edge_message_bwd=L - 1,
           layer0_factorised_bwd=1)
    h32.close()
    edge0 = _engine(golden, pc.Case("per-edge", "depth", ("base",), order=order), monkeypatch, {"VSSR_L0_FACTORISE": "0"})
    expect(counts(edge0, backend.WANT_ALL), embed=1, message_mlp=1, edge_message_fwd=L, update_fwd=L - 1, edge_message_bwd=L,
           layer0_factorised_fwd=0, layer0_factorised_bwd=0)
    edge0.close()


# ---- 4: intermediates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,env", [((2,), {}), ((0, 2), {}), ((0, 1, 1, 2), {}), ((2,), {"VSSR_L0_FACTORISE": "0"}),
                                       ((0, 1, 1, 2), {"VSSR_L0_FACTORISE": "0"})],
                         ids=["depth1", "depth2", "depth4", "depth1-per-edge-layer-0", "depth4-per-edge-layer-0"])
def test_per_layer_intermediates_at_other_depths(golden, oracle_mod, monkeypatch, order, env):
    """Every activation vssr_debug_read serves for layers 0 .. L - 1, e_atom and the adjoints of layer 0's message output against the
    oracle's dump (model 1) at 2e-5 relative.  Not materialised, as at depth 3: phi0 under the species factorisation and the last
    block's vector output -- nothing else may be refused.  embedding() is s_upd{L - 1}."""
    from surface_sampling_amd import backend

    L, m = len(order), 1
    case = pc.Case("intermediates", "depth", ("O40",), order=order)
    eng = _engine(golden, case, monkeypatch, env)
    s = pc.structure(golden, "O40")
    eng.evaluate([pc.arrays(s)])
    _, _, d = oracle_mod.painn(case.blobs(golden)[m], s.numbers, s.positions, s.cell, s.pbc, 64, dump=True, hp=case.oracle_hp(oracle_mod))
    n = len(s)
    report, refused = [], []
    for l in range(L):
        for name, shape in (("phi", (n, 384)), ("s_msg", (n, 128)), ("v_msg", (n, 3, 128)), ("s_upd", (n, 128)), ("v_upd", (n, 3, 128))):
            try:
                got = eng.debug_read(f"{name}{l}", m).reshape(shape).astype(np.float64)
            except backend.BackendError as exc:
                assert "not materialised" in str(exc), (name, l, str(exc))
                refused.append(f"{name}{l}")
                continue
            want = d[name][l]
            report.append((f"{name}{l}", np.abs(got - want).max() / max(1.0, np.abs(want).max())))
    assert refused == (["phi0"] if not env else []) + [f"v_upd{L - 1}"], refused
    with pytest.raises(backend.BackendError):
        eng.debug_read(f"s_upd{L}", m)                       # no such layer
    got = eng.debug_read("e_atom", m).astype(np.float64)
    report.append(("e_atom", np.abs(got - d["e_atom"]).max() / max(1.0, np.abs(d["e_atom"]).max())))
    for name, shape in (("sbar_msg", (n, 128)), ("vbar_msg", (n, 3, 128))):
        got = eng.debug_read(f"{name}0", m).reshape(shape).astype(np.float64)
        want = d[name][0]
        report.append((f"{name}0", np.abs(got - want).max() / max(1.0, np.abs(want).max())))
    emb = eng.embedding()
    assert emb.shape == (3, n, 128) and np.array_equal(emb[m], eng.embedding(m))
    assert np.array_equal(emb[m].reshape(-1), eng.debug_read(f"s_upd{L - 1}", m))
    want = d["s_upd"][L - 1]
    report.append(("embedding", np.abs(emb[m].astype(np.float64) - want).max() / max(1.0, np.abs(want).max())))
    print(f"intermediates depth {L} {env}: " + " ".join(f"{k} {v:.1e}" for k, v in report))
    bad = [(k, v) for k, v in report if not v < 2e-5]
    assert not bad, f"intermediates off: {bad}; all: {report}"
    assert len(report) == 5 * L - len(refused) + 4
    eng.close()


# ---- 5: both paths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.BOTH_PATH_CASES, ids=lambda c: c.id)
def test_general_path_on_the_ensemble_cutoff_and_repulsion_cases(golden, oracle_mod, monkeypatch, case):
    """VSSR_PAINN_PATH=general (powf and plain fp32 sums, painn_gen.hip) against the same oracle values by the same rule, and against
    the 128 / 20 path at the contract; stress of the two paths within 1e-6 eV/A^3."""
    gen = _engine(golden, case, monkeypatch, {"VSSR_PAINN_PATH": "general"})
    fast = _engine(golden, case)
    a = _run(golden, oracle_mod, case, gen, "general")
    sa, sda = gen.stress()
    b = fast.evaluate([pc.arrays(pc.structure(golden, n)) for n in case.structs])
    sb, sdb = fast.stress()
    de, df = float(np.abs(a["energy_f64"] - b["energy_f64"]).max()), float(np.abs(a["forces"] - b["forces"]).max())
    ds, dfs = float(np.abs(a["energy_std"] - b["energy_std"]).max()), float(np.abs(a["forces_std"] - b["forces_std"]).max())
    print(f"general against 128 / 20 {case.id}: dE {de:.2e} dF {df:.2e} dstd {ds:.2e} dFstd {dfs:.2e} stress {np.abs(sa - sb).max():.2e} "
          f"stress std {np.abs(sda - sdb).max():.2e}")
    assert de <= pc.E_TOL and df <= pc.F_TOL and ds <= pc.STD_TOL and dfs <= pc.F_TOL
    assert np.isfinite(sa).all() and np.abs(sa - sb).max() <= 1e-6 and np.abs(sda - sdb).max() <= 1e-6      # eV/A^3
    gen.close()
    fast.close()


# ---- 6: ensemble statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["128-20", "general"])
def test_one_model_has_no_spread(golden, oracle_mod, monkeypatch, general):
    case = pc.BY_ID["models-1"]
    eng = _engine(golden, case, monkeypatch, {"VSSR_PAINN_PATH": "general"} if general else {})
    res = _run(golden, oracle_mod, case, eng, "general" if general else "")        # (forces against the oracle: there)
    assert res["energy_std"][0] == 0.0 and res["energy_std_f64"][0] == 0.0
    assert np.abs(res["forces_std"]).max() == 0.0 and np.abs(res["forces"]).max() > 1.0
    st, sd = eng.stress()
    assert np.abs(st).max() > 0.0 and np.abs(sd).max() == 0.0
    assert res["energy_models"].shape == (1, 1) and res["energy_models_f64"][0, 0] == res["energy_f64"][0]
    eng.close()


def test_eight_models_have_eight_energies(golden, oracle_mod):
    case = pc.BY_ID["models-8"]
    eng = _engine(golden, case)
    res = eng.evaluate([pc.arrays(pc.structure(golden, "syn4"))])
    ref = pc.reference(golden, oracle_mod, case, "syn4")
    assert res["energy_models"].shape == (1, 8) and ref["energy_models"].shape == (8,)
    d = np.abs(res["energy_models_f64"][0] - ref["energy_models"])
    print("models-8: |d energy_models| " + " ".join(f"{x:.1e}" for x in d) + f"; spread of the models {np.ptp(ref['energy_models']):.2e} eV")
    assert d.max() <= pc.E_TOL
    assert np.ptp(ref["energy_models"]) > 100 * pc.E_TOL            # eight different numbers, not one repeated
    assert np.array_equal(res["energy_models"][0], res["energy_models_f64"][0].astype(np.float32))   # the float32 words: the same values, narrowed
    eng.close()


def test_nine_models_are_refused(golden):
    from surface_sampling_amd import backend

    case = pc.BY_ID["models-8"]
    with pytest.raises(backend.BackendError):
        _engine(golden, case, blobs=pc.perturbed_ensemble(golden.blobs, 9))
    _good_engine_still_evaluates(golden)


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [{"num_conv": 0}, {"num_conv": 5}, {"readout_hidden": 129}, {"V_ex_power": 65}],
                         ids=["num_conv-0", "num_conv-5", "readout-129", "power-65"])
def test_configurations_outside_the_family_are_refused(golden, bad):
    """(The blob is not looked at before the shape is refused; excl_power 65 with the repulsion ON: off, any power is accepted.)"""
    from surface_sampling_amd import backend

    with pytest.raises(backend.BackendError):
        _engine(golden, pc.Case("shipped", "depth", ("base",)), hparams=bad)
    _good_engine_still_evaluates(golden)


def test_species_beyond_the_embedding_table_is_refused(golden, oracle_mod):
    """Z = 39 against n_embed = 39 (the first row that is not there); the same engine then evaluates the slab (Z <= 38)."""
    from surface_sampling_amd import backend

    case = pc.BY_ID["embed-39"]
    eng = _engine(golden, case)
    s = pc.structure(golden, "base")
    z = s.numbers.copy()
    z[z == 38] = 39
    with pytest.raises(backend.BackendError, match=r"species index 39 outside \[0,39\)"):
        eng.evaluate([(z, s.positions, s.cell, s.pbc)])
    _run(golden, oracle_mod, case, eng, "after the refusal")
    eng.close()
    _good_engine_still_evaluates(golden)
