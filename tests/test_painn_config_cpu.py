"""CPU: pins the case table of tests/painn_config_cases.py with the fp64 / fp32 oracle alone -- the builders give blobs of the layout's
length, the reference itself stays inside the contract on every case but the ones named in BEYOND_CONTRACT, and every case moves the
result far enough from the shipped configuration that a device ignoring the parameter would be caught."""
import numpy as np
import pytest

import painn_config_cases as pc
from painn_shapes import reshape_blob


def _length(hp):
    from surface_sampling_amd import checkpoint

    return sum(int(np.prod(s)) for s in checkpoint.painn_blob_shapes({**pc.SRC, **hp}).values())


def test_builders_give_blobs_of_the_layouts_length(golden):
    b = golden.blobs[0]
    assert np.array_equal(pc.relayer(b, [0, 1, 2]), b) and pc.relayer(b, [0, 1, 2]).tobytes() == b.tobytes()
    for order in ([2], [0], [0, 2], [1, 2], [0, 1, 1, 2]):
        assert pc.relayer(b, order).size == _length({"num_conv": len(order)}), order
    assert pc.cut_embed(b, 39).size == _length({"n_embed": 39})
    for H in (1, 32, 40, 128):
        bh, hp = reshape_blob(b, 128, 20, readout_hidden=H)
        assert bh.size == _length({"readout_hidden": H}) and hp["readout_hidden"] == H
        assert pc.relayer(bh, [2], readout_hidden=H).size == _length({"num_conv": 1, "readout_hidden": H})
    for M in (5, 8):
        ens = pc.perturbed_ensemble(golden.blobs, M)
        assert len(ens) == M and all(x.size == b.size and x.dtype == np.float32 for x in ens)
        assert len({x.tobytes() for x in ens}) == M                      # distinct models
    for c in pc.CASES:                                                   # and every case's own models
        want = _length({"num_conv": c.L, "readout_hidden": c.H, "n_embed": c.n_embed})
        blobs = c.blobs(golden)
        assert len(blobs) == c.M and all(x.size == want for x in blobs), c.id


def test_relayer_moves_whole_blocks(golden):
    from surface_sampling_amd import checkpoint

    src = checkpoint.blob_to_fields(golden.blobs[1])
    got = checkpoint.blob_to_fields(pc.relayer(golden.blobs[1], [0, 1, 1, 2]), {"num_conv": 4})
    for l, o in enumerate([0, 1, 1, 2]):
        for part in ("msg{}.W1", "msg{}.b2", "msg{}.Wd", "upd{}.U", "upd{}.W3", "upd{}.b4"):
            assert np.array_equal(got[part.format(l)], src[part.format(o)]), (l, part)
    assert np.array_equal(got["embed"], src["embed"]) and np.array_equal(got["readout.W5"], src["readout.W5"])


def test_cut_embedding_table_gives_the_same_bits(golden, oracle_mod):
    """39 rows (Sr, Z = 38, is the last one) against 100 rows: the oracle's energies and forces are equal to the last bit."""
    case = pc.BY_ID["embed-39"]
    for name in case.structs:
        a, b = pc.reference(golden, oracle_mod, case, name), pc.reference(golden, oracle_mod, case.shipped(), name)
        assert a["energy"] == b["energy"] and a["energy_std"] == b["energy_std"], name
        assert np.array_equal(a["forces"], b["forces"]) and np.array_equal(a["forces_std"], b["forces_std"]), name
        assert np.array_equal(a["energy_models"], b["energy_models"]), name


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_reference_alone_stays_inside_the_contract(golden, oracle_mod, case):
    """The oracle at 32 bits against the oracle at 64 bits: inside the contract for every case outside BEYOND_CONTRACT, outside it
    for every case in the list (a listed case that meets the contract does not belong there)."""
    inside = True
    for name in case.structs:
        de, df, ds, dfs = pc.deviation(pc.reference(golden, oracle_mod, case, name, 32), pc.reference(golden, oracle_mod, case, name, 64))
        print(f"{case.id} {name}: oracle fp32 against fp64 dE {de:.2e} dF {df:.2e} dstd {ds:.2e} dFstd {dfs:.2e}")
        inside = inside and de <= pc.E_TOL and df <= pc.F_TOL and ds <= pc.STD_TOL and dfs <= pc.F_TOL
    assert inside == (case.id not in pc.BEYOND_CONTRACT), case.id


def test_beyond_contract_names_the_six_angstrom_cases_only():
    assert pc.BEYOND_CONTRACT == [c.id for c in pc.CASES if c.cutoff == 6.0] and len(pc.BEYOND_CONTRACT) == 1


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.axis != "embed"], ids=lambda c: c.id)
def test_every_case_is_sensitive_to_its_parameter(golden, oracle_mod, case):
    """The fp64 oracle with the case's value against the fp64 oracle with the shipped value (3 models, 3 blocks, 5.0 A, on / 12 / 1.5,
    H = 64) on the same structure: at least ten times the tolerance apart in energy or in the largest force difference, on every
    structure of the case.  (The embedding-row case changes nothing by construction: test_cut_embedding_table_gives_the_same_bits;
    the device is caught there by the refusal of Z = 39.)"""
    for name in case.structs:
        de, df, _, _ = pc.deviation(pc.reference(golden, oracle_mod, case, name), pc.reference(golden, oracle_mod, case.shipped(), name))
        print(f"{case.id} {name}: against the shipped value dE {de:.2e} dF {df:.2e}")
        assert de >= 10 * pc.E_TOL or df >= 10 * pc.F_TOL, (case.id, name, de, df)


def test_the_table_covers_what_it_claims():
    ids = set(pc.BY_ID)
    assert {c.order for c in pc.DEPTH_CASES} == {(2,), (0,), (0, 2), (1, 2), (0, 1, 1, 2)}
    assert {c.M for c in pc.CASES if c.axis == "models"} == {1, 2, 5, 8}
    assert {c.cutoff for c in pc.CASES if c.axis == "cutoff"} == {4.0, 4.5, 5.5, 6.0}
    assert {(c.p, c.sigma) for c in pc.CASES if c.axis == "repulsion" and c.excl_vol} == {(1, 1.5), (2, 1.0), (7, 1.5), (13, 1.2), (6, 2.5),
                                                                                         (33, 1.6), (64, 1.5)}
    assert {c.p for c in pc.CASES if not c.excl_vol} == {12, 0}
    assert any(not c.excl_vol and c.H == 32 for c in pc.CASES)
    assert {(c.H, c.L) for c in pc.CASES if c.axis == "readout"} == {(1, 3), (40, 3), (128, 3), (1, 1), (32, 1), (40, 1), (128, 1),
                                                                      (32, 2), (32, 4)}
    assert {c.L for c in pc.MIXED_CASES} == {2, 4} and all(c.structs == ("base", "syn4") for c in pc.MIXED_CASES)
    assert "embed-39" in ids and len(pc.CASES) == 35


def test_structures_are_small(golden):
    sizes = {n: len(pc.structure(golden, n)) for n in ("base", "O40", "syn4", "syn2")}
    assert all(60 <= v <= 76 for v in sizes.values()), sizes
    s = pc.structure(golden, "base")
    assert int(s.numbers.max()) == 38      # Sr is the last row of a 39-row embedding table
