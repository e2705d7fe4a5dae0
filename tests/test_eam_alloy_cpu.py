"""Several-element EAM on the host: setfl / eam/fs / mixed-funcfl readers and writer, their refusals, the numpy restatement
(tests/eam_alloy_oracle.py) against central differences, the reference's one-element numbers through one-element setfl files,
element-order invariance, the fs orientation, and the calculators' configuration (no device needed)."""
import itertools
import json
import os

import numpy as np
import pytest

import eam_alloy_oracle as ao
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fl():
    from surface_sampling_amd import eam

    return eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(GOLDEN, "eam_kat.json")) as fh:
        return json.load(fh)


def _cu100(adatoms):
    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    return np.vstack([d["positions"], d["ads_coords"][list(adatoms)]]), d["cell"], d["pbc"], len(d["ads_coords"])


def _cluster(seed=0, n=14):
    """A small open Cu/Au cluster with every pair inside the cutoff range that matters."""
    rng = np.random.default_rng(seed)
    g = np.array(list(itertools.product(range(3), range(3), range(2))), float)[:n] * 2.5
    return g + rng.normal(0, 0.12, g.shape), np.eye(3) * 30.0, np.zeros(3, np.uint8), rng.integers(0, 2, n)


def test_setfl_round_trip(fl):
    from surface_sampling_amd import eam

    for fs in (None, (0.7, 1.3)):
        s = ao.cuau_setfl(*fl, fs_scale=fs)
        text = eam.write_setfl(s)
        back = eam.parse_setfl(text, fs=fs is not None)
        assert back.elements == ["Cu", "Au"] and back.atomic_numbers == [29, 79] and back.fs == (fs is not None)
        assert (back.nrho, back.nr, back.drho, back.dr, back.cutoff) == (s.nrho, s.nr, s.drho, s.dr, s.cutoff)
        for x, y in ((back.frho, s.frho), (back.rhor, s.rhor), (back.z2r, s.z2r)):
            assert x.shape == y.shape and np.array_equal(x, y)
        assert eam.write_setfl(back) == text


def test_setfl_refusals(fl):
    from surface_sampling_amd import calculators, eam

    text = eam.write_setfl(ao.cuau_setfl(*fl))
    lines = text.splitlines()
    with pytest.raises(ValueError, match="ends early"):
        eam.parse_setfl("\n".join(lines[:len(lines) // 2]))                 # truncated
    with pytest.raises(ValueError, match="announces"):
        eam.parse_setfl("\n".join(lines[:3] + ["3 Cu Au"] + lines[4:]))     # wrong N
    with pytest.raises(ValueError, match="ends early|bad number"):
        eam.parse_setfl(text, fs=True)                                       # an alloy file read as fs
    bad = lines[:]
    bad[7] = bad[7].replace(bad[7].split()[1], "nan", 1)
    with pytest.raises(ValueError, match="non-finite"):
        eam.parse_setfl("\n".join(bad))
    with pytest.raises(ValueError, match="bad number"):
        eam.parse_setfl("\n".join(lines[:7] + ["1.0 x 2.0"] + lines[8:]))
    with pytest.raises(ValueError, match="bad grid"):
        eam.parse_setfl("\n".join(lines[:4] + ["3 0.1 500 0.01 5.0"] + lines[5:]))
    s = eam.parse_setfl(text)
    with pytest.raises(ValueError, match="NULL"):
        eam.tables_from_setfl(s, ["Cu", "NULL"])
    with pytest.raises(ValueError, match="not in the potential"):
        eam.tables_from_setfl(s, ["Cu", "Ag"])
    with pytest.raises(ValueError, match="at most 8"):
        eam.tables_from_setfl(s, ["Cu"] * 9)
    resolve = lambda name: text   # noqa: E731
    with pytest.raises(ValueError, match="NULL"):
        calculators.eam_tables("eam/alloy", ["* * x.eam.alloy Cu NULL"], resolve)
    with pytest.raises(ValueError, match="evaluates"):
        calculators.eam_tables("eam/cd", ["* * x Cu Au"], resolve)
    with pytest.raises(ValueError, match="several types"):
        calculators.eam_tables("eam/alloy", ["* * x Cu Cu"], resolve)


def test_oracle_forces_are_minus_the_energy_gradient(fl):
    from surface_sampling_amd import eam

    pos, cell, pbc, types = _cluster()
    for fs in (None, (0.7, 1.3)):
        t = eam.tables_from_setfl(ao.cuau_setfl(*fl, fs_scale=fs), ["Cu", "Au"])
        E, ea, F = ao.eam_typed(t, types, pos, cell, pbc)
        assert abs(ea.sum() - E) < 1e-10
        h = 1e-5
        for i in (0, 3, 7, 13):
            for x in range(3):
                p, m = pos.copy(), pos.copy()
                p[i, x] += h
                m[i, x] -= h
                g = (ao.eam_typed(t, types, p, cell, pbc)[0] - ao.eam_typed(t, types, m, cell, pbc)[0]) / (2 * h)
                assert abs(F[i, x] + g) < 1e-6, (fs, i, x, F[i, x], -g)


def test_one_element_setfl_reproduces_the_reference_numbers(fl, kat):
    """Cu_u3 / Au_u3 converted to one-element setfl files (written and read back): the reference's -25.2893 (one Cu adatom, bridge
    site) and -79.03490823689619 (6 Au adatoms on Au(110))."""
    from surface_sampling_amd import eam

    cu, au = fl
    t = eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(eam.funcfl_to_setfl(cu))), ["Cu"])
    _, cell, pbc, _ = _cu100([])
    bridge = int(np.flatnonzero(np.load(os.path.join(GOLDEN, "cu100.npz"))["site_kind"] == 1)[0])
    e = ao.eam_typed(t, np.zeros(9, int), _cu100([bridge])[0], cell, pbc)[0]
    assert np.allclose(e, kat["min_energy_one_bridge_adatom"]["value"])
    d = np.load(os.path.join(GOLDEN, "au110.npz"))
    ta = eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(eam.funcfl_to_setfl(au))), ["Au"])
    k = kat["au110"]["num_ads_atoms"]
    n = len(d["positions"]) + k
    e = sorted(ao.eam_typed(ta, np.zeros(n, int), np.vstack([d["positions"], d["ads_coords"][list(sub)]]), d["cell"], d["pbc"])[0]
               for sub in itertools.combinations(range(len(d["ads_coords"])), k))
    target = kat["au110"]["min_energy"]["value"]
    assert np.allclose(e[0], target) and min(abs(x - target) for x in e[:2]) < 1e-11


def test_element_order_changes_no_energy(fl):
    """Cu/Au listed as (Cu, Au) or (Au, Cu) in the file, and in either pair_coeff order: the same energies."""
    from surface_sampling_amd import eam

    pos, cell, pbc = ao.cu100_slab(3, 3, 4)
    types = ao.random_alloy(pos, 0.35, 4)
    sym = np.array(["Cu", "Au"])[types]
    for fs in (None, (0.7, 1.3)):
        base = ao.cuau_setfl(*fl, fs_scale=fs)
        ref = None
        for order in ((0, 1), (1, 0)):
            s = eam.parse_setfl(eam.write_setfl(ao.permuted(base, order)), fs=fs is not None)
            for names in (["Cu", "Au"], ["Au", "Cu"]):
                t = eam.tables_from_setfl(s, names)
                E = ao.eam_typed(t, np.array([names.index(x) for x in sym]), pos, cell, pbc)[0]
                ref = E if ref is None else ref
                assert abs(E - ref) <= 1e-12 * abs(ref), (fs, order, names, E, ref)


def test_fs_orientation_and_the_alloy_reduction(fl):
    """An fs file with rho_{I->J} = rho_I is the alloy potential; the asymmetric file is read with block I, entry J = the
    density I contributes at J (a Cu-Au dimer by hand: rho at Cu = 1.3 rho_Au, at Au = 0.7 rho_Cu)."""
    import eam_oracle
    from surface_sampling_amd import eam

    cu, au = fl
    pos, cell, pbc = ao.cu100_slab(3, 3, 4)
    types = ao.random_alloy(pos, 0.4, 2)
    alloy = eam.tables_from_setfl(ao.cuau_setfl(cu, au), ["Cu", "Au"])
    fs1 = eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (1.0, 1.0))), fs=True), ["Cu", "Au"])
    a, b = ao.eam_typed(alloy, types, pos, cell, pbc), ao.eam_typed(fs1, types, pos, cell, pbc)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0]) and np.abs(a[2] - b[2]).max() < 1e-12
    s = eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (0.7, 1.3))), fs=True)
    t = eam.tables_from_setfl(s, ["Cu", "Au"])
    r = 2.6
    E = ao.eam_typed(t, [0, 1], np.array([[0, 0, 0], [r, 0, 0.0]]), np.eye(3) * 30, np.zeros(3))[0]
    spl = lambda f, d: eam_oracle.spline_eval(eam_oracle.build_spline(f, d), np.array([r]), d, len(f))[0][0]   # noqa: E731
    splF = lambda f, x: eam_oracle.spline_eval(eam_oracle.build_spline(f, s.drho), np.array([x]), s.drho, s.nrho, True)[0][0]   # noqa: E731
    rho_cu, rho_au = spl(s.rhor[0][0], s.dr), spl(s.rhor[1][1], s.dr)
    want = splF(s.frho[0], 1.3 * rho_au) + splF(s.frho[1], 0.7 * rho_cu) + spl(s.z2r[1], s.dr) / r
    assert abs(E - want) < 1e-12 * abs(want)
    wrong = splF(s.frho[0], 0.7 * rho_au) + splF(s.frho[1], 1.3 * rho_cu) + spl(s.z2r[1], s.dr) / r
    assert abs(want - wrong) > 1e-3                                    # a transposed reading would be seen


def test_mixed_funcfl_with_one_file_is_the_one_element_potential(fl):
    import eam_oracle
    from surface_sampling_amd import eam

    cu, au = fl
    t = eam.tables_from_funcfl([cu, cu])
    assert (t.nr, t.nrho, t.cutoff) == (cu.nr - 1, cu.nrho - 1, cu.cutoff)
    _, cell, pbc, n_sites = _cu100([])
    for sub in ((), (5,), (2, 9), (0, 4, 11)):
        pos = _cu100(sub)[0]
        E0, ea0, F0 = eam_oracle.eam(cu, pos, cell, pbc)
        E1, ea1, F1 = ao.eam_typed(t, np.arange(len(pos)) % 2, pos, cell, pbc)
        assert abs(E1 - E0) <= 1e-9 and np.abs(ea1 - ea0).max() <= 1e-9 and np.abs(F1 - F0).max() <= 1e-9
    m = eam.tables_from_funcfl([cu, au])
    assert (m.dr, m.cutoff, m.elements) == (max(cu.dr, au.dr), au.cutoff, ["Cu", "Au"])
    # the grid points of the finer file are reproduced where the resampling lands on them (here r = 0)
    assert m.rhor[0][0] == cu.rhor[0] and m.frho[1][5] == pytest.approx(au.frho[5], rel=1e-12)


def _run_dir(tmp_path, style, pot, atoms):
    rd = tmp_path / "run"
    rd.mkdir()
    (rd / "lammps_config.json").write_text(json.dumps({"potential_file": pot, "atoms": atoms, "bulk_index": 8}))
    for name in ("lammps_energy_template.txt", "lammps_opt_template.txt"):
        (rd / name).write_text(f"units metal\nboundary p p p\npair_style {style}\npair_coeff * * {{}} {{}}\n")
    return rd


def test_calculators_configure_several_elements(fl, tmp_path):
    from surface_sampling_amd import backend, eam
    from surface_sampling_amd.calculators import EAMSurfCalc, LAMMPSRunSurfCalc, LAMMPSSurfCalc

    cu, au = fl
    path = str(tmp_path / "CuAu.eam.alloy")
    eam.write_setfl(ao.cuau_setfl(cu, au), path)
    calc = LAMMPSRunSurfCalc(files=[path])
    calc.set(pair_style="eam/alloy", pair_coeff=["* * CuAu.eam.alloy Au Cu"])
    assert calc.species == ["Au", "Cu"] and calc.tables is not None and calc.funcfl is None
    assert calc._types_of([29, 79, 29]).tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="not covered"):
        calc._types_of([29, 47])
    calc.set(specorder=["Cu", "Au"], pair_coeff=["* * CuAu.eam.alloy Cu Au"])
    assert calc.species == ["Cu", "Au"]
    mixed = EAMSurfCalc(files=[os.path.join(GOLDEN, "Cu_u3.eam"), os.path.join(GOLDEN, "Au_u3.eam")])
    mixed.set(pair_style="eam", pair_coeff=["1 1 Cu_u3.eam", "2 2 Au_u3.eam"])
    assert mixed.species == ["Cu", "Au"] and mixed.tables.nr == 499
    with pytest.raises(ValueError, match="i i"):
        mixed.set(pair_coeff=["1 2 Cu_u3.eam"])
    with pytest.raises(ValueError, match="evaluates"):
        mixed.set(pair_style="eam/cd")
    rd = _run_dir(tmp_path, "eam/alloy", path, ["Cu", "Au"])
    lc = LAMMPSSurfCalc()
    lc.set(run_dir=str(rd))
    lc._configure()
    assert lc.pair_style == "eam/alloy" and lc.species == ["Cu", "Au"] and lc.tables.elements == ["Cu", "Au"]
    rd2 = tmp_path / "mixed"
    rd2.mkdir()
    (rd2 / "lammps_config.json").write_text(json.dumps({"potential_file": [os.path.join(GOLDEN, "Cu_u3.eam"),
                                                                           os.path.join(GOLDEN, "Au_u3.eam")],
                                                        "atoms": ["Cu", "Au"]}))
    (rd2 / "lammps_energy_template.txt").write_text("pair_style eam\n")
    lc2 = LAMMPSSurfCalc()
    lc2.set(run_dir=str(rd2))
    lc2._configure()
    assert lc2.tables.elements == ["Cu", "Au"]
    rd3 = _run_dir(tmp_path / "x", "eam/cd", path, ["Cu", "Au"]) if (tmp_path / "x").mkdir() is None else None
    lc3 = LAMMPSSurfCalc()
    lc3.set(run_dir=str(rd3))
    with pytest.raises(backend.BackendError, match="eam/cd"):
        lc3._configure()
