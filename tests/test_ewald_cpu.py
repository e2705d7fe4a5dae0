"""The Ewald sum without a GPU: the numpy restatement tests/ewald_oracle.py against Madelung constants, its own forces against central
differences, its independence of the damping parameter; what pair.parse reads and refuses; the ABI's new name; and the rehearsal of
what tests/test_ewald_gpu.py presumes about its inputs.  Every figure is printed before it is asserted."""
import math
import os
import re

import numpy as np
import pytest

import ewald_cases as ec
import ewald_oracle as eo
import pair_oracle as po
from surface_sampling_amd import backend, pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ewald(lines, struct, n_types=3):
    m = pair.parse(lines, n_types)
    T, X, C, _ = struct
    return m, eo.ewald(*eo.model_of(m), T, X, C)


# -- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, struct, pairs, r0, madelung", [
    ("rocksalt", ec.cube(), 4, 5.64 / 2, 1.7475645946),
    ("CsCl", ec.cscl(4.12), 1, 4.12 * math.sqrt(3.0) / 2, 1.7626747731),
])
def test_madelung_energy_from_the_ewald_sum(name, struct, pairs, r0, madelung):
    """A = 1e-12, rc = 10 A: the energy per ion pair in units of qqrd2e / r0 is the Madelung constant to 1e-10 relative; the forces
    on the perfect crystal vanish and the atoms sum to E."""
    m, (E, ea, F) = _ewald(ec.coul(10.0, 1e-12), struct)
    M = -E / pairs * r0 / po.QQRD2E
    print(f"{name}: Madelung {M:.13f} (reference {madelung})  relative error {abs(M / madelung - 1):.2e}  k vectors "
          f"{len(eo.k_indices(struct[2], m.kspace.k_cut)[0])}  max|F| {np.abs(F).max():.2e}")
    assert abs(M / madelung - 1) <= 1e-10
    assert np.abs(F).max() < 1e-12
    assert abs(ea.sum() - E) <= 1e-14 * abs(E)


def test_forces_and_per_atom_energies_on_the_skewed_charged_cell():
    T, X, C, _ = s = ec.skewed()
    m, (E, ea, F) = _ewald(ec.coul(9.0, 1e-12), s)
    assert abs(float(np.asarray(m.charges)[T].sum()) - 1.0) < 1e-15          # non-neutral: the background term is in play
    h, worst = 1e-5, 0.0
    for i in range(len(T)):
        for x in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[i, x] += h
            Xm[i, x] -= h
            fd = -(eo.ewald(*eo.model_of(m), T, Xp, C)[0] - eo.ewald(*eo.model_of(m), T, Xm, C)[0]) / (2 * h)
            worst = max(worst, abs(fd - F[i, x]))
    print(f"skewed cell: E {E:.12f} eV  max|F - central difference| {worst:.2e}  |sum(ea) - E| / |E| {abs(ea.sum() - E) / abs(E):.2e}")
    assert worst <= 1e-7
    assert abs(ea.sum() - E) <= 1e-14 * abs(E)


def test_the_sum_does_not_depend_on_the_damping_parameter():
    s = ec.skewed()
    (_, (E1, _, F1)), (_, (E2, _, F2)) = _ewald(ec.coul(9.0, 1e-12), s), _ewald(ec.coul(6.5, 1e-12), s)
    print(f"g-independence: E {E1:.12f} / {E2:.12f}  |dE| {abs(E1 - E2):.2e}  max|dF| {np.abs(F1 - F2).max():.2e}")
    assert abs(E1 - E2) <= 1e-10 * max(1.0, abs(E1))
    assert np.abs(F1 - F2).max() <= 1e-8


# -- the parser ---------------------------------------------------------------------------------------------------------------------
def test_composite_styles_expand_to_their_terms():
    m = pair.parse(["pair_style buck/coul/long 8.0 10.0", "pair_coeff 1 1 0 1 0", "pair_coeff 1 2 1000 0.3 0 7.0",
                    "pair_coeff 2 2 2000 0.2 30", "kspace_style ewald 1e-8", "set type 1 charge 1", "set type 2 charge -1"], 2)
    S = pair.STYLES
    assert [(t.type_a, t.type_b, t.style, t.rc) for t in m.terms] == [
        (0, 0, S["buck"], 8.0), (0, 0, S["coul/long"], 10.0), (0, 1, S["buck"], 7.0), (0, 1, S["coul/long"], 10.0),
        (1, 1, S["buck"], 8.0), (1, 1, S["coul/long"], 10.0)]                  # the optional pair cutoff is the short-range one
    assert m.terms[2].c == (1000.0, 0.3, 0.0, 0.0, 0.0) and m.cutoff == 10.0 and list(m.charges) == [1.0, -1.0]
    L = math.sqrt(-math.log(1e-8))
    assert m.kspace == pair.KSpace(1e-8, L / 10.0, 2.0 * (L / 10.0) * L)       # g = L / rc, k_cut = 2 g L
    m = pair.parse(ec.born(8.0, 1e-5), 3)
    assert sorted({t.style for t in m.terms}) == [S["born"], S["coul/long"]] and len(m.terms) == 12
    assert m.kspace.g_ewald == math.sqrt(-math.log(1e-5)) / 8.0               # one cutoff: also the Coulomb one
    m = pair.parse(["pair_style lj/cut/coul/long 9.0", "pair_coeff 1 1 0.01 3.0", "pair_coeff 2 2 0.04 2.0", "kspace_style ewald 1e-6",
                    "set type * charge 0.5"], 2)
    mixed = [t for t in m.terms if (t.type_a, t.type_b, t.style) == (0, 1, S["lj/cut"])]
    assert len(mixed) == 1 and mixed[0].c[:2] == (0.02, math.sqrt(6.0))       # geometric mixing, as for lj/cut
    m = pair.parse(ec.coul(9.0, 1e-6), 3)
    assert [(t.type_a, t.type_b) for t in m.terms] == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert all(t.style == S["coul/long"] and t.rc == 9.0 and t.shift == 0 for t in m.terms)


def test_hybrid_overlay_forms_and_gewald():
    S = pair.STYLES
    m = pair.parse(["pair_style hybrid/overlay born/coul/long 9 10 morse 4", "pair_coeff * * born/coul/long 1 1 1 0 0",
                    "pair_coeff 1 2 morse 1 1 1", "kspace_style ewald 1e-5", "kspace_modify gewald 0.3", "set type * charge 1"], 2)
    assert [(t.type_a, t.type_b, t.style, t.rc) for t in m.terms] == [
        (0, 0, S["born"], 9.0), (0, 0, S["coul/long"], 10.0), (0, 1, S["born"], 9.0), (0, 1, S["morse"], 4.0),
        (0, 1, S["coul/long"], 10.0), (1, 1, S["born"], 9.0), (1, 1, S["coul/long"], 10.0)]
    assert m.kspace.g_ewald == 0.3 and m.kspace.k_cut == 2.0 * 0.3 * math.sqrt(-math.log(1e-5))   # gewald overrides g only
    m = pair.parse(["pair_style hybrid/overlay coul/long 9 lj/cut 5", "pair_coeff * * coul/long", "pair_coeff 1 1 lj/cut 1 1",
                    "pair_coeff 2 2 lj/cut 1 1", "kspace_style ewald 1e-5", "set type * charge 1"], 2)
    assert [(t.type_a, t.type_b, t.style) for t in m.terms] == [(0, 0, 1), (0, 0, 6), (0, 1, 6), (1, 1, 1), (1, 1, 6)]
    # a 'none' pair of a composite hybrid still carries the Coulomb term: the reciprocal sum runs over every pair
    m = pair.parse(["pair_style hybrid buck/coul/long 8", "pair_coeff 1 1 buck/coul/long 100 0.3 1", "pair_coeff 1 2 none",
                    "pair_coeff 2 2 buck/coul/long 100 0.3 1", "kspace_style ewald 1e-5", "set type * charge 1"], 2)
    assert [(t.type_a, t.type_b, t.style) for t in m.terms] == [(0, 0, 3), (0, 0, 6), (0, 1, 6), (1, 1, 3), (1, 1, 6)]


@pytest.mark.parametrize("lines, match", [
    (["pair_style coul/long 9", "pair_coeff * *", "kspace_style pppm 1e-4", "set type * charge 1"], r"kspace_style pppm 1e-4"),
    (["pair_style coul/long 9", "pair_coeff * *", "kspace_style ewald/disp 1e-4", "set type * charge 1"], r"kspace_style ewald/disp"),
    (["pair_style coul/long 9", "pair_coeff * *", "kspace_style ewald", "set type * charge 1"], r"'kspace_style ewald'"),
    (["pair_style coul/long 9", "pair_coeff * *", "kspace_style ewald 1e-4", "kspace_modify slab 3.0", "set type * charge 1"],
     r"kspace_modify slab 3.0"),
    (["pair_style coul/long 9", "pair_coeff * *", "kspace_style ewald 1e-4", "kspace_modify mesh 8 8 8", "set type * charge 1"],
     r"kspace_modify mesh"),
    (["pair_style buck/coul/long 9", "pair_coeff * * 100 0.3 1", "set type * charge 1"], r"pair_style buck/coul/long 9.*KSpace"),
    (["pair_style lj/cut 9", "pair_coeff * * 1 1", "kspace_style ewald 1e-4"], r"without a \*/coul/long"),
    (["pair_style coul/long 9", "pair_coeff * *", "kspace_style ewald 1e-4"], r"needs charges"),
    (["pair_style hybrid/overlay coul/long 9 coul/dsf 0.2 9", "pair_coeff * * coul/long", "pair_coeff * * coul/dsf",
      "kspace_style ewald 1e-4", "set type * charge 1"], r"one Coulomb sum"),
    (["pair_style hybrid/overlay coul/long 9 lj/cut 5", "pair_coeff 1 1 coul/long", "pair_coeff * * lj/cut 1 1",
      "kspace_style ewald 1e-4", "set type * charge 1"], r"every type pair"),
    (["pair_style hybrid/overlay buck/coul/long 8 9 born/coul/long 8 10", "pair_coeff 1 1 buck/coul/long 1 1 1",
      "pair_coeff 1 2 born/coul/long 1 1 1 1 1", "pair_coeff 2 2 buck/coul/long 1 1 1", "kspace_style ewald 1e-4", "set type * charge 1"],
     r"differ in their Coulomb cutoff"),
])
def test_refusals_of_the_parser(lines, match):
    with pytest.raises(ValueError, match=match):
        pair.parse(lines, 2)


def test_a_dsf_model_parses_to_what_it_did():
    m = pair.parse(po.ROCKSALT_COMMANDS, 2)
    assert m.kspace is None and len(m) == 5
    old = pair.PairModel(m.n_types, m.terms, m.charges, m.cutoff)             # the four-field construction still holds
    assert old.kspace is None and old[:4] == m[:4]
    S = pair.STYLES
    assert [(t.type_a, t.type_b, t.style, t.rc, t.shift) for t in m.terms] == [
        (0, 0, S["born"], 8.0, 0), (0, 0, S["coul/dsf"], 12.0, 0), (0, 1, S["born"], 8.0, 0), (0, 1, S["coul/dsf"], 12.0, 0),
        (1, 1, S["born"], 8.0, 0), (1, 1, S["coul/dsf"], 12.0, 0)]
    assert m.terms[1].c == (0.2, 0.0, 0.0, 0.0, 0.0) and m.terms[0].c == (0.2637, 0.317, 2.340, 1.0486, -0.4993)


def test_calculator_keywords_override_the_k_space_parameters(monkeypatch):
    from surface_sampling_amd import calculators

    monkeypatch.setattr(calculators.PairSurfCalc, "_init_common", lambda self, *a, **k: None)
    monkeypatch.setattr(calculators._AnalyticSurfCalc, "__init__", lambda self, **k: None)
    L = math.sqrt(-math.log(1e-6))
    c = calculators.PairSurfCalc(commands=ec.coul(9.0, 1e-6), species=["Na", "Cl", "Mg"], k_cut=3.5)
    assert c.pair_model.kspace == pair.KSpace(1e-6, L / 9.0, 3.5)
    c = calculators.PairSurfCalc(commands=ec.coul(9.0, 1e-6), species=["Na", "Cl", "Mg"], g_ewald=0.4)
    assert c.pair_model.kspace == pair.KSpace(1e-6, 0.4, 2.0 * 0.4 * L)
    with pytest.raises(ValueError, match="need a"):
        calculators.PairSurfCalc(commands=po.ROCKSALT_COMMANDS, species=["Na", "Cl"], k_cut=3.0)


def test_lammps_surf_calc_refuses_an_open_boundary_for_an_ewald_template(tmp_path):
    import json

    from surface_sampling_amd.calculators import LAMMPSSurfCalc

    (tmp_path / "lammps_config.json").write_text(json.dumps({"atoms": ["Na", "Cl", "Mg"], "bulk_index": 0}))
    body = "units metal\nboundary p p f\nread_data {}\n" + "\n".join(ec.born(8.0, 1e-8)) + "\nrun 0\n"
    (tmp_path / "lammps_energy_template.txt").write_text(body)
    calc = LAMMPSSurfCalc(device="cuda:0")
    calc.set(run_dir=str(tmp_path))
    with pytest.raises(backend.BackendError, match=r"boundary 'p p f'.*boundary p p p"):
        calc._configure()                                                     # (what the first evaluation does before it packs)


# -- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_new_creator_is_declared_exported_and_built():
    assert "vssr_pair_create_kspace" in backend.EXPORTS
    header = open(os.path.join(ROOT, "include", "vssr_eval.h")).read()
    assert re.search(r"\bint vssr_pair_create_kspace\s*\(", header) and "VSSR_PAIR_COUL_LONG = 6" in header
    assert getattr(backend.load_library(), "vssr_pair_create_kspace") is not None
    import ctypes

    assert ctypes.sizeof(backend.KSpace) == 16


# -- rehearsal of the device inputs -------------------------------------------------------------------------------------------------
def test_ragged_inputs_have_the_k_boxes_the_device_test_presumes():
    """Per-axis bounds and half-box sizes of every chain of the ragged batch, the shapes the batch is there for (a box that is no
    multiple of the kernel's k block, one below a block, a long thin one, a chain longer than one atom tile and than one wave of the
    atom kernel), and no lattice vector within 1e-9 (relative, in k^2) of the sphere: a vector that close could fall on either side
    in two correct implementations, and it would carry exp(-k_cut^2 / 4 g^2) = 1e-8 of the sum."""
    m = pair.parse(ec.RAGGED_MODEL, 3)
    assert abs(m.kspace.k_cut - 4.605170185988092) < 1e-12
    shapes = {}
    for name, make, bound, cells in ec.RAGGED:
        T, X, C, pbc = make()
        b = tuple(eo.bounds(C, m.kspace.k_cut))
        hkl, _ = eo.k_indices(C, m.kspace.k_cut)
        margin = eo.sphere_margin(C, m.kspace.k_cut)
        print(f"{name}: {len(T)} atoms  bounds {b}  half box {ec.half_box(b)}  k vectors {len(hkl)}  atom tile {ec.atom_tile(b)}  "
              f"sphere margin {margin:.2e}  total charge {float(np.asarray(m.charges)[T].sum()):+.1f}")
        assert b == bound and ec.half_box(b) == cells
        assert (np.abs(hkl).max(axis=0) <= np.array(b)).all() and len(hkl) % 2 == 0 and len(hkl) // 2 <= cells
        assert margin > 1e-9
        assert all(pbc)
        shapes[name] = (len(T), ec.half_box(b), ec.atom_tile(b))
    assert shapes["cube"][1] > ec.KBLOCK and shapes["cube"][1] % ec.KBLOCK != 0
    assert shapes["small"][1] < ec.KBLOCK
    assert shapes["slab70"][0] == 70 > ec.TILE_MAX >= shapes["slab70"][2] and shapes["slab70"][1] % ec.KBLOCK != 0
    assert shapes["thin"][1] // 5 // 9 == 49                                   # 2 m_z + 1 = 49 indices along z, 4 along x and y
    T, X, C, _ = ec.slab70()
    assert float(np.asarray(m.charges)[T].sum()) == 2.0 and float(np.asarray(m.charges)[ec.skewed()[0]].sum()) == 1.0


def test_capacity_case_of_the_device_test():
    """12 x 12 x 40 A at A = 1e-8, rc = 10 fits the kernels' caps with room to spare (index 63 per axis, 65 536 cells); the cell the
    device test expects to be refused does not."""
    m = pair.parse(ec.coul(10.0, 1e-8), 3)
    b = eo.bounds(np.diag([12.0, 12.0, 40.0]), m.kspace.k_cut)
    print(f"12 x 12 x 40: bounds {b}, half box {ec.half_box(b)}")
    assert max(b) <= 31 and ec.half_box(b) * 8 <= 65536
    m = pair.parse(ec.RAGGED_MODEL, 3)
    assert eo.bounds(np.diag([5.64, 5.64, 90.0]), m.kspace.k_cut)[2] > 63     # per-axis cap
    b = eo.bounds(np.diag([40.0, 40.0, 40.0]), m.kspace.k_cut)
    assert max(b) <= 63 and ec.half_box(b) > 65536                             # cell cap
