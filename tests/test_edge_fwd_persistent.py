"""GPU (-m gpu): the persistent 16-wave forward neighbor-sum kernel (painn_edge_mfma.hip, k_edge_fwd_mfma<4, true, 16, false, true>)
with several items per workgroup against one item per workgroup (VSSR_EDGE_FWD_GRID=0: the grid of the one-item launch it replaced, a
single trip through the kernel).

A persistent workgroup walks the items w, w + G, w + 2 G, ... and stages the next item's slice while its slower waves still walk
the current one.  Addresses, LDS placement and every centre's summation order do not depend on the grid, so every result must
be the same bits; one engine of every case is also held against the fp64 oracle at the tolerances of test_gpu_parity.py.  On a
256-CU device a test batch has fewer items than CUs, so the cases cap the grid (VSSR_EDGE_FWD_GRID=8 / 16) and force the 16-wave
class with a chain of more than 176 atoms (two slices of a smaller chain fit the LDS and take the 8-wave form)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_TOL = 1e-4      # eV, GPU fp32 vs fp64 oracle        (tests/test_gpu_parity.py)
F_TOL = 2e-4      # eV/A
STD_TOL = 2e-4
KEYS = ("energy", "energy_f64", "energy_std", "energy_models", "forces", "forces_std")
LAYER_OUT = ("s_msg1", "v_msg1", "s_msg2", "v_msg2")   # what the kernel under test writes (layers 1 and 2), per model


def _arrays(s):
    return (s.numbers, s.positions, s.cell, s.pbc)


def _engine(golden, monkeypatch, grid):
    """A PaiNN engine created under VSSR_EDGE_FWD_GRID=grid (None: the default, one workgroup per CU); read at create only."""
    from surface_sampling_amd import backend

    table, const = golden.offset_table()
    if grid is not None:
        monkeypatch.setenv("VSSR_EDGE_FWD_GRID", str(grid))
    try:
        return backend.PainnEngine(golden.blobs, device=0, offset_per_z=table, offset_const=const)
    finally:
        if grid is not None:
            monkeypatch.delenv("VSSR_EDGE_FWD_GRID")


def _layer_outputs(eng):
    out = {}
    for name in LAYER_OUT:
        for m in range(3):
            try:
                out[name, m] = eng.debug_read(name, m).copy()
            except Exception as exc:
                assert "not materialised" in str(exc), (name, m, exc)
    return out


def _same_bits(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


def _against_oracle(golden, oracle_mod, res, chains, refs):
    for b, s in enumerate(chains):
        a0, a1 = res["cfg_start"][b], res["cfg_start"][b + 1]
        ref = refs[b]
        de, df = abs(float(res["energy"][b]) - ref["energy"]), np.abs(res["forces"][a0:a1] - ref["forces"]).max()
        print(f"chain {b} ({len(s)} atoms): |dE| {de:.2e} eV  max|dF| {df:.2e} eV/A")
        assert de <= E_TOL and df <= F_TOL, (b, len(s), de, df)
        assert abs(float(res["energy_std"][b]) - ref["energy_std"]) <= STD_TOL
        assert np.abs(res["forces_std"][a0:a1] - ref["forces_std"]).max() <= STD_TOL


@pytest.fixture(scope="module")
def slab(golden):
    return golden.structure("SrTiO3_2x2_pristine")


@pytest.fixture(scope="module")
def ragged(golden, slab):
    """272, 248, 60 and 12 atoms in one launch of the 16-feature class: the largest chain sizes the LDS tile, so all four take the
    16-wave form.  A larger slice follows a smaller one and the other way round; 60 atoms are 15 bundles for 16 waves, 12 atoms 3
    bundles (13 waves without one); 4 chains are padded to 8, so padding ids sit in the middle of a workgroup's sequence (192 items,
    half of them padding)."""
    from surface_sampling_amd import structures

    big = slab.repeat((2, 2, 1))
    keep = np.sort(np.random.default_rng(11).choice(len(slab), size=12, replace=False))
    chains = [structures.synth_chain(big, 24), structures.synth_chain(big, 25), slab,
              structures.Structure(slab.numbers[keep], slab.positions[keep], slab.cell, slab.pbc)]
    assert [len(c) for c in chains] == [272, 248, 60, 12]
    return chains


@pytest.fixture(scope="module")
def ragged_refs(golden, oracle_mod, ragged):
    table, const = golden.offset_table()
    return [oracle_mod.ensemble(golden.blobs, s.numbers, s.positions, s.cell, s.pbc, 64, table, const) for s in ragged]


def test_one_chain_three_items_per_workgroup(golden, oracle_mod, slab, monkeypatch):
    """One 240-atom chain, grid 8: 24 items on 8 workgroups, 3 each; slice and model change between a workgroup's items, the chain
    does not."""
    s = slab.repeat((2, 2, 1))
    s.positions = s.positions + np.random.default_rng(5).normal(0.0, 0.05, s.positions.shape)
    assert len(s) == 240
    runs = []
    for grid in (8, 0):
        eng = _engine(golden, monkeypatch, grid)
        runs.append((eng.evaluate([_arrays(s)]), _layer_outputs(eng)))
        eng.close()
    (res, lay), (res0, lay0) = runs
    _same_bits(res, res0, "240 atoms")
    assert lay.keys() == lay0.keys()
    for k in lay:
        assert np.array_equal(lay[k], lay0[k]), k
    print(f"layer outputs compared: {sorted(set(n for n, _ in lay))}")
    table, const = golden.offset_table()
    ref = oracle_mod.ensemble(golden.blobs, s.numbers, s.positions, s.cell, s.pbc, 64, table, const)
    _against_oracle(golden, oracle_mod, res, [s], [ref])


@pytest.mark.parametrize("grid", [8, 16, 40, None])
def test_ragged_batch(golden, oracle_mod, ragged, ragged_refs, monkeypatch, grid):
    """The ragged batch under a grid of 8 (24 items per workgroup), of 16 (12), of 40 (192 items are no multiple of it: 5 items for
    workgroups 0 .. 31, 4 for the rest) and the default (one workgroup per CU: one item per workgroup when the device has more CUs than the
    batch has items)."""
    packs = [_arrays(s) for s in ragged]
    runs = []
    for g in (grid, 0):
        eng = _engine(golden, monkeypatch, g)
        runs.append((eng.evaluate(packs), _layer_outputs(eng)))
        eng.close()
    (res, lay), (res0, lay0) = runs
    _same_bits(res, res0, f"ragged, grid {grid}")
    assert lay.keys() == lay0.keys()
    for k in lay:
        assert np.array_equal(lay[k], lay0[k]), k
    _against_oracle(golden, oracle_mod, res, ragged, ragged_refs)


def test_active_mask_with_a_converged_chain_between_live_ones(golden, oracle_mod, slab, monkeypatch):
    """Lock-step FIRE on three chains, the middle one held fixed entirely: after the driver's first poll the evaluations run under the
    activity mask, and the items of the middle chain -- in the middle of every workgroup's sequence -- are skipped."""
    from surface_sampling_amd import structures

    big = slab.repeat((2, 2, 1))
    chains = [structures.synth_chain(big, 5), structures.synth_chain(big, 9), structures.synth_chain(big, 13)]
    packs = [_arrays(c) for c in chains]
    fixed = np.concatenate([(c.positions[:, 2] < c.positions[:240, 2].max() - 4.0).astype(np.uint8) for c in chains])
    fixed[len(chains[0]):len(chains[0]) + len(chains[1])] = 1
    runs = []
    for grid in (8, 0):
        eng = _engine(golden, monkeypatch, grid)
        eng.upload(packs)
        info = eng.relax("FIRE", fixed=fixed, max_steps=6, fmax=0.01)
        res = eng.download()
        runs.append((info, res))
        eng.close()
    (info, res), (info0, res0) = runs
    assert info["converged"][1] and info["n_steps"][0] == 6 and info["n_steps"][2] == 6
    for k in ("positions", "n_steps", "converged"):
        assert np.array_equal(info[k], info0[k]), k
    _same_bits(res, res0, "masked FIRE")
    # the last evaluation (masked) against the oracle at the relaxed geometry of a live chain
    a0, a1 = res["cfg_start"][2], res["cfg_start"][3]
    s = structures.Structure(chains[2].numbers, info["positions"][a0:a1], chains[2].cell, chains[2].pbc)
    table, const = golden.offset_table()
    ref = oracle_mod.ensemble(golden.blobs, s.numbers, s.positions, s.cell, s.pbc, 64, table, const)
    de, df = abs(float(res["energy"][2]) - ref["energy"]), np.abs(res["forces"][a0:a1] - ref["forces"]).max()
    print(f"live chain after 6 FIRE steps: |dE| {de:.2e} eV  max|dF| {df:.2e} eV/A")
    assert de <= E_TOL and df <= F_TOL


def test_capacity_overflow_returns_and_the_rerun_is_right(golden, oracle_mod, ragged, ragged_refs, monkeypatch):
    """A slot capacity too small for the first evaluation: every workgroup of the persistent launch returns on the overflow flag, the
    host regrows the buffers and the rerun under a capped grid gives the bits of a roomy one-item-per-workgroup engine."""
    packs = [_arrays(s) for s in ragged]
    eng = _engine(golden, monkeypatch, 8)
    eng.debug_capacity(slots_per_atom=16, tight=1)
    res = eng.evaluate(packs)
    eng.close()
    eng0 = _engine(golden, monkeypatch, 0)
    res0 = eng0.evaluate(packs)
    eng0.close()
    _same_bits(res, res0, "after a regrow")
    _against_oracle(golden, oracle_mod, res, ragged, ragged_refs)
