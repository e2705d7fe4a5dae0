"""The slab Ewald sum without a GPU: the numpy restatement tests/ewald_slab_oracle.py against an exact two-dimensional Ewald sum, its
own forces, invariances, limits and virial; what pair.parse and LAMMPSSurfCalc read and refuse; the ABI's new name; and the rehearsal
of what tests/test_ewald_slab_gpu.py presumes about its inputs.  Every figure is printed before it is asserted."""
import json
import math
import os
import re

import numpy as np
import pytest

import cell_cases as cc
import ewald_cases as ec
import ewald_oracle as eo
import ewald_slab_cases as sc
import ewald_slab_oracle as so
import strain_fd as sf
from surface_sampling_amd import backend, pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test 1: |(a) - (b)| measured with this file at F = 3, 5, 8 (e^2 / A); the bounds are 100 x these (rounding of ~1e3 terms)
MEASURED_2D = {3: 9.5e-15, 5: 1.6e-15, 8: 3.6e-15}


# -- 1: the slab-corrected 3-D sum against the exact 2-D sum ------------------------------------------------------------------------
def dipolar_random8():
    """Eight random charges made neutral in an orthogonal 6 x 7 x 12 A cell, z in [3, 9]; the charges are dealt in ascending order to
    the ions in ascending z, so the cell carries a dipole whatever the draw."""
    rng = np.random.default_rng(45)
    q = rng.uniform(-1.0, 1.0, 8)
    q = np.sort(q - q.mean())
    X = np.c_[rng.uniform(0, 6, 8), rng.uniform(0, 7, 8), np.sort(rng.uniform(3, 9, 8))]
    return q, X, np.diag([6.0, 7.0, 12.0])


def test_corrected_sum_is_the_two_dimensional_sum():
    """This test validates the restatement tests/ewald_slab_oracle.py, the contract of the device tests, and runs none of the shipped
    code: form (a), the slab-corrected 3-D sum, against form (b), an exact two-dimensional sum that shares only the real-space pair
    list with it.  g = 0.6, rc = 14, k_cut = 7 (erfc(g rc) and exp(-k_cut^2 / 4 g^2) are below 1e-14).  Measured here (e^2 / A): |(a) - (b)| =
    4.2e-10, 9.5e-15, 1.6e-15, 3.6e-15 at F = 2, 3, 5, 8; the sum without the correction is off by 4.2e-2, 2.8e-2, 1.7e-2, 1.1e-2."""
    q, X, C = dipolar_random8()
    g, rc, k_cut = 0.6, 14.0, 7.0
    exact = so.ewald_2d(q, g, rc, k_cut, X, C)
    plain3 = None
    for F in (2, 3, 5, 8):
        a = so.coulomb(q, g, rc, k_cut, F, np.arange(8), X, C)[0] / so.QQRD2E
        plain = so.coulomb(q, g, rc, k_cut, F, np.arange(8), X, C, correct=False)[0] / so.QQRD2E
        print(f"F = {F}: 2-D sum {exact:+.15f}  corrected {a:+.15f}  |(a) - (b)| {abs(a - exact):.2e}  uncorrected off by {abs(plain - exact):.2e} e^2/A")
        if F >= 3:
            assert abs(a - exact) <= min(100 * MEASURED_2D[F], 1e-9 / so.QQRD2E), F
        if F == 3:
            plain3 = abs(plain - exact)
    assert plain3 > 1e-2                                                       # the test cannot pass with the correction missing


# -- 2: the restatement against itself ----------------------------------------------------------------------------------------------
def _model(lines=None):
    return pair.parse(sc.MODEL if lines is None else lines, 3)


def _E(m, T, X, C):
    return so.ewald(*eo.model_of(m), T, X, C)


@pytest.mark.parametrize("make", [sc.dipolar8, sc.charged8, sc.skewed8], ids=["neutral", "charged", "skewed-charged"])
def test_forces_sum_and_invariances_of_the_restatement(make):
    T, X, C, _ = make()
    m = _model()
    E, ea, Fo = _E(m, T, X, C)
    Q = float(np.asarray(m.charges)[T].sum())
    h, worst = 1e-5, 0.0
    for i in range(len(T)):
        for x in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[i, x] += h
            Xm[i, x] -= h
            worst = max(worst, abs(-(_E(m, T, Xp, C)[0] - _E(m, T, Xm, C)[0]) / (2 * h) - Fo[i, x]))
    dz = abs(_E(m, T, X + [0, 0, sc.SHIFT_Z], C)[0] - E)
    dxy = abs(_E(m, T, X + sc.in_plane_shift(C), C)[0] - E)
    print(f"Q {Q:+.0f}: E {E:.12f}  max|F - central difference| {worst:.2e}  |sum e_i - E| {abs(ea.sum() - E):.2e}  "
          f"|dE| z shift {dz:.2e}  in-plane shift {dxy:.2e}  |sum F_z| {abs(Fo[:, 2].sum()):.2e}")
    assert worst <= 1e-7
    assert abs(ea.sum() - E) <= 1e-13 * max(1.0, abs(E))
    assert dz <= 1e-12 * max(1.0, abs(E)) and dxy <= 1e-12 * max(1.0, abs(E))
    assert abs(Fo[:, 2].sum()) <= 1e-11 and np.abs(Fo.sum(axis=0)).max() <= 1e-11


def test_single_ion_closed_form_and_the_slab_virial():
    """One ion: E_slab = -qqrd2e 2 pi q^2 L'^2 / (12 V'), no force.  The strain derivative of the dipole term alone on the in-plane
    skewed charged cell is E_slab (-1, -1, +1, 0, 0, 0)."""
    T, X, C, _ = sc.single()
    E, e, f = so.slab_term([1.0], X, C, sc.F)
    closed = -so.QQRD2E * 2 * math.pi * (sc.F * 12.0) ** 2 / (12.0 * sc.F * 6 * 7 * 12)
    print(f"single ion: E_slab {E:.15f}  closed form {closed:.15f}")
    assert abs(E - closed) <= 1e-14 * abs(closed) and abs(e[0] - E) <= 1e-14 * abs(E) and np.abs(f).max() == 0.0
    T, X, C, _ = sc.skewed8()
    q = np.asarray(_model().charges)[T]
    Es = so.slab_term(q, X, C, sc.F)[0]
    chk = sf.fd_stress(lambda x, c: so.slab_term(q, x, c, sc.F)[0], X, C)
    want = Es * np.array([-1.0, -1.0, 1.0, 0.0, 0.0, 0.0])
    print(f"slab virial: E_slab {Es:.9f}  finite difference {chk.virial}  unc {chk.unc}")
    assert (np.abs(chk.virial - want) <= 10 * chk.unc).all()


# -- 3: the parser ------------------------------------------------------------------------------------------------------------------
COUL = ["pair_style coul/long 9", "pair_coeff * *", "kspace_style ewald 1e-4", "set type * charge 1"]


def test_parser_reads_the_slab_factor():
    m = pair.parse(["boundary p p f", *COUL, "kspace_modify slab 3.0"], 1)
    assert m.kspace.slab == 3.0
    m2 = pair.parse("units metal\nboundary p p f   # open along z\nkspace_modify slab 2.5\n" + "\n".join(COUL), 1)
    assert m2.kspace.slab == 2.5 and m2.kspace[:3] == m.kspace[:3]
    plain = pair.parse(COUL, 1)
    assert plain.kspace.slab == 0.0 and plain.kspace == pair.KSpace(plain.kspace.accuracy, plain.kspace.g_ewald, plain.kspace.k_cut)
    assert pair.parse(["boundary p p p", *COUL], 1).kspace == plain.kspace
    assert pair.KSpace(1e-4, 0.3, 2.0) == (1e-4, 0.3, 2.0, 0.0) and pair.KSpace(1e-4, 0.3, 2.0).slab == 0.0
    assert pair.ewald_defaults(1e-4, 9.0, slab=3.0).slab == 3.0 and pair.ewald_defaults(1e-4, 9.0) == plain.kspace
    for t3, t in zip(pair.parse(ec.coul(8.0, 1e-8), 3).terms, pair.parse(sc.slab_lines(ec.coul(8.0, 1e-8)), 3).terms):
        assert t3 == t


@pytest.mark.parametrize("lines, match", [
    ([*COUL, "kspace_modify slab 3.0"], r"'kspace_modify slab 3.0'.*boundary p p f"),
    (["boundary p p p", *COUL, "kspace_modify slab 3.0"], r"'kspace_modify slab 3.0'.*incorrect boundaries with slab Ewald"),
    (["boundary p f p", *COUL, "kspace_modify slab 3.0"], r"'kspace_modify slab 3.0'.*boundary p p f"),
    ([*COUL, "kspace_modify slab 3.0", "boundary p p f"], r"'kspace_modify slab 3.0'"),
    (["boundary p p f", *COUL, "kspace_modify slab 3.0", "boundary p p p"], r"'boundary p p p'.*incorrect boundaries with slab Ewald"),
    (["boundary p p f", *COUL, "kspace_modify slab nozforce"], r"'kspace_modify slab nozforce'.*nozforce"),
    (["boundary p p f", *COUL, "kspace_modify slab ew2d"], r"'kspace_modify slab ew2d'.*ew2d"),
    (["boundary p p f", *COUL, "kspace_modify slab 1.0"], r"'kspace_modify slab 1.0'.*bad slab parameter"),
    (["boundary p p f", *COUL, "kspace_modify slab 0.5"], r"'kspace_modify slab 0.5'.*bad slab parameter"),
    (["boundary p p f", *COUL, "kspace_modify slab"], r"'kspace_modify slab'"),
    (["boundary p p f", *COUL, "kspace_modify slab three"], r"'three' is not a number"),
    (["boundary p p f", "pair_style lj/cut 9", "pair_coeff * * 1 1", "kspace_modify slab 3.0"], r"slab without a \*/coul/long"),
])
def test_parser_refusals(lines, match):
    with pytest.raises(ValueError, match=match):
        pair.parse(lines, 1)
    with pytest.raises(ValueError, match="slab factor"):
        pair.ewald_defaults(1e-4, 9.0, slab=1.0)


# -- 4: a LAMMPS run directory ------------------------------------------------------------------------------------------------------
def _run_dir(path, boundary, extra):
    (path / "lammps_config.json").write_text(json.dumps({"atoms": ["Na", "Cl", "Mg"], "bulk_index": 0}))
    lines = ec.born(8.0, 1e-8)
    body = f"units metal\nboundary {boundary}\nread_data {{}}\n" + "\n".join(lines[:-3] + extra + lines[-3:]) + "\nrun 0\n"
    (path / "lammps_energy_template.txt").write_text(body)
    from surface_sampling_amd.calculators import LAMMPSSurfCalc

    calc = LAMMPSSurfCalc(device="cuda:0")
    calc.set(run_dir=str(path))
    return calc


def test_lammps_surf_calc_serves_a_slab_template(tmp_path):
    from surface_sampling_amd.structures import Structure

    calc = _run_dir(tmp_path, "p p f", ["kspace_modify slab 3.0"])
    calc._configure()
    assert calc.pair_model.kspace.slab == 3.0 and list(calc._fixed_pbc()) == [1, 1, 0]
    T, X, C, _ = sc.dipolar8()
    types, _, _, pbc = calc._pack(Structure(np.where(T == 0, 11, 17), X, C, [1, 1, 1]))
    assert list(pbc) == [1, 1, 0] and list(types) == list(T)


def test_lammps_surf_calc_refuses_a_slab_factor_under_full_periodicity(tmp_path):
    calc = _run_dir(tmp_path, "p p p", ["kspace_modify slab 3.0"])
    with pytest.raises(backend.BackendError, match=r"kspace_modify slab 3.0.*incorrect boundaries with slab Ewald"):
        calc._configure()


def test_pair_surf_calc_takes_the_slab_keyword_and_imposes_the_boundary():
    from surface_sampling_amd.calculators import PairSurfCalc
    from surface_sampling_amd.structures import Structure

    calc = PairSurfCalc(commands=ec.born(8.0, 1e-8), species=["Na", "Cl", "Mg"], slab=3.0)
    parsed = PairSurfCalc(commands=sc.slab_lines(ec.born(8.0, 1e-8)), species=["Na", "Cl", "Mg"])
    assert calc.pair_model.kspace == parsed.pair_model.kspace and calc.pair_model.kspace.slab == 3.0
    T, X, C, _ = sc.dipolar8()
    assert list(calc._pack(Structure(np.where(T == 0, 11, 17), X, C, [1, 1, 1]))[3]) == [1, 1, 0]
    plain = PairSurfCalc(commands=ec.born(8.0, 1e-8), species=["Na", "Cl", "Mg"])
    assert plain.pair_model.kspace.slab == 0.0 and plain._fixed_pbc() is None
    assert PairSurfCalc(commands=sc.slab_lines(ec.born(8.0, 1e-8)), species=["Na", "Cl", "Mg"], slab=0.0).pair_model.kspace.slab == 0.0
    with pytest.raises(ValueError, match="slab factor"):
        PairSurfCalc(commands=ec.born(8.0, 1e-8), species=["Na", "Cl", "Mg"], slab=1.0)


# -- 5: the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_slab_creator_is_declared_exported_and_built():
    assert "vssr_pair_create_kspace_slab" in backend.EXPORTS
    header = open(os.path.join(ROOT, "include", "vssr_eval.h")).read()
    assert re.search(r"\bint vssr_pair_create_kspace_slab\s*\([^)]*const vssr_kspace \*ks, double slab_factor, vssr_handle \*\*out\)", header)
    assert getattr(backend.load_library(), "vssr_pair_create_kspace_slab") is not None
    import ctypes

    assert ctypes.sizeof(backend.KSpace) == 16                                # vssr_kspace keeps its layout


# -- 6: rehearsal of the device inputs ----------------------------------------------------------------------------------------------
def test_device_cases_have_the_shapes_the_device_test_presumes():
    """Extended k box, atom tile and cell count of every chain of the ragged batch; none trips a refusal of vssr_batch_upload (caps,
    cell shape, z span); no lattice vector of an extended cell within 1e-9 (relative, in k^2) of the sphere."""
    m = _model()
    assert m.kspace.slab == sc.F and abs(m.kspace.k_cut - 3.6841361487904734) < 1e-12
    shapes = {}
    for name, make in sc.RAGGED:
        T, X, C, pbc = make()
        b = sc.ext_bounds(C, m.kspace.k_cut)
        assert b == tuple(eo.bounds(so.extended(C, sc.F), m.kspace.k_cut))
        margin = eo.sphere_margin(so.extended(C, sc.F), m.kspace.k_cut)
        span = np.ptp(X[:, 2])
        print(f"{name}: {len(T)} atoms  extended k box {b}  half box {ec.half_box(b)}  atom tile {ec.atom_tile(b)}  sphere margin {margin:.2e}  "
              f"z in [{X[:, 2].min():.2f}, {X[:, 2].max():.2f}] of {C[2, 2]}  total charge {float(np.asarray(m.charges)[T].sum()):+.1f}")
        assert max(b) <= 63 and ec.half_box(b) <= 65536 and margin > 1e-9
        assert list(pbc) == [1, 1, 0] and C[0, 2] == C[1, 2] == C[2, 0] == C[2, 1] == 0.0 and span <= C[2, 2]
        shapes[name] = (len(T), b, ec.half_box(b), ec.atom_tile(b))
    tile = shapes["big70"][3]
    assert shapes["big63"][1] == shapes["big70"][1] and tile < 63                         # the moments of these chains cross tiles ...
    assert len({shapes[f"big{n}"][0] % tile for n in (63, 64, 65, 70)}) == 4               # ... and end in tiles filled differently
    assert shapes["big64"][0] == ec.TILE_MAX and shapes["big65"][0] == ec.TILE_MAX + 1     # one wave of the atom kernel, and one atom more
    assert shapes["dipolar8"][0] <= shapes["dipolar8"][3]                                  # one tile
    n, b, cells, tile = shapes["thin32"]
    assert 50 <= b[2] <= 63 and tile <= 10 and n > 3 * tile and cells % ec.KBLOCK != 0     # many l rows, moments over four tiles
    assert shapes["single"][0] == 1
    assert shapes["skewed8"][1] != shapes["dipolar8"][1]
    T, X, C, _ = sc.lefthanded8()
    assert np.linalg.det(C) < 0 and np.array_equal(X, sc.charged8()[1])                    # a left-handed cell, the same ions
    T, X, C, _ = sc.below_and_outside()
    frac = X @ np.linalg.inv(C)
    assert X[:, 2].max() < 0 and (frac[:, 0] > 1).all() and (frac[:, 1] < 0).all()
    q = np.asarray(m.charges)
    assert q[sc.dipolar8()[0]].sum() == 0 and q[sc.charged8()[0]].sum() == 1 and q[sc.big(70)[0]].sum() == 2 and q[sc.big(63)[0]].sum() != 0
    z = sc.dipolar8()[1][:, 2]
    assert abs((q[sc.dipolar8()[0]] * z).sum()) > 1.0                                      # a dipole: the correction is no rounding matter


def test_stress_relaxation_and_refusal_cases_of_the_device_test():
    for name, make, rc in sc.STRESS:
        s = make()
        _, _, _, rv = cc.brute_neighbors(s[1], s[2], s[3], rc + 1.0)
        margin = np.abs(np.linalg.norm(rv, axis=1) - rc).min()
        m = _model(sc.slab_lines(ec.born(rc, 1e-12)))
        b = sc.ext_bounds(s[2], m.kspace.k_cut)
        print(f"stress {name}: rc {rc}  nearest pair to the cutoff {margin:.4f} A  extended k box {b}  half box {ec.half_box(b)}")
        assert margin > 0.01 and max(b) <= 63 and ec.half_box(b) <= 65536
    (T, X, C, pbc), fixed = sc.relax16()
    m = _model(sc.slab_lines(ec.born(8.0, 1e-8)))
    b = sc.ext_bounds(C, m.kspace.k_cut)
    assert len(T) == 16 and fixed.sum() == 8 and X[fixed, 2].max() < X[~fixed, 2].min() and max(b) <= 63
    assert np.asarray(m.charges)[T].sum() == 0 and np.asarray(m.charges)[T[fixed]].sum() == 0
    # the refusals: 5.64 x 5.64 x 12 at F = 6 needs index 42 along z (served), the capacity case 5.64 x 5.64 x 40 at F = 3 needs 70
    k_cut = _model().kspace.k_cut
    assert sc.ext_bounds(np.diag([5.64, 5.64, 40.0]), k_cut)[2] > 63 >= eo.bounds(np.diag([5.64, 5.64, 40.0]), k_cut)[2]
