"""Virial stress of the fp64 analytic potentials on the MI355X (vssr_batch_stress on Tersoff, Stillinger-Weber and EAM handles):
parity with the strain derivative of the matching CPU restatement (tests/strain_fd.py; no executed LAMMPS is compared), the
published SW silicon answers through the device, rotation covariance, repeatability, the state rules of the entry point and the
calculator surface.

Tolerance of every parity comparison, per component, on the virial V sigma in eV: ten times the checker's own uncertainty
(strain_fd.fd_stress), no fixed constant.  Every component is printed before anything is asserted; the line ``max ratio`` of each
potential is what profiles/r13/NOTES_analytic_stress.md records."""
import ctypes as C
import os

import numpy as np
import pytest

import cell_cases as cc
import eam_alloy_oracle as ao
import strain_fd as sf
import sw_oracle as so
from conftest import GOLDEN, SI_T3, SI_T3_A0, diamond_cell, synthetic_tersoff
from test_sw_cpu import _si_run_dir

pytestmark = pytest.mark.gpu

FACTOR = 10.0
ONES = np.ones(3, np.uint8)


def _rattled(X, sigma, seed):
    return X + np.random.default_rng(seed).normal(0.0, sigma, np.shape(X))


def _parity(tag, eng, structs, energy_of):
    """One evaluation + one stress call of ``structs`` = [(types, positions, cell, pbc)] against fd_stress of
    ``energy_of(types, positions, cell, pbc)``; returns the largest |device - checker| / uncertainty."""
    eng.evaluate_f64(structs)
    st, sd = eng.stress()
    assert st.shape == (len(structs), 6) and np.isfinite(st).all()
    assert not sd.any()                                           # one model: the spread is zero by definition
    worst, bad = 0.0, []
    for b, (T, X, Cl, pbc) in enumerate(structs):
        chk = sf.fd_stress(lambda x, c: energy_of(T, x, c, pbc), X, Cl)
        for k in range(6):
            dev = st[b, k] * chk.volume
            ratio = abs(dev - chk.virial[k]) / chk.unc[k]
            print(f"{tag} chain {b} ({len(T)} atoms) voigt {k}: device {dev:+.12e}  checker {chk.virial[k]:+.12e}  "
                  f"unc {chk.unc[k]:.3e} eV  ratio {ratio:.3f}")
            worst = max(worst, ratio)
            if not abs(dev - chk.virial[k]) <= FACTOR * chk.unc[k]:
                bad.append((b, k, dev, chk.virial[k], chk.unc[k]))
    print(f"{tag}: max ratio |device - checker| / uncertainty = {worst:.3f}")
    assert not bad, (tag, bad)
    return worst


def _padded_rows(X, Cl, pbc, rc):
    i, _, _, _ = cc.brute_neighbors(X, Cl, pbc, rc)
    return 4 * np.ceil(np.bincount(i, minlength=len(X)) / 4)


def _cu():
    from surface_sampling_amd import eam

    return eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam"))


def _fcc_block(a=3.615, reps=3):
    basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    shifts = np.array([[x, y, z] for x in range(reps) for y in range(reps) for z in range(reps)], float)
    return (basis[None] + shifts[:, None]).reshape(-1, 3) * a, np.eye(3) * a * reps


# -- parity with the strain derivative of the restatements ---------------------------------------------------------------------------
def test_tersoff_stress_is_the_strain_derivative_of_the_oracle_energy(golden, oracle_mod):
    """GaN.tersoff on the rattled slab cell (periodic in all three directions, as the GaN templates say), its 72-atom supercell, the
    skewed slab and the thin wurtzite cell of tests/cell_cases.py; Si(C) on diamond silicon, the skewed 2-atom primitive cell and
    the simple-cubic cell whose neighbors are all self images; synthetic three-species entries (m = 3, lam3 != 0, n != 1) on dense
    boxes with rows on both sides of the 16-slot tile, and five species (more than the LDS kernel holds: every row takes the
    one-thread-per-centre form)."""
    from surface_sampling_amd import backend

    nm = cc.by_name(cc.battery())
    g = golden.structure("GaN_3x3_pristine")
    tg = np.array([0 if z == 31 else 1 for z in g.numbers], np.int32)
    slab = cc.Case("gan_rattled", "gan", g.numbers, _rattled(g.positions, 0.05, 4), g.cell, [1, 1, 1], None, None, tg)
    gan = [slab.typed(), cc.supercell(slab.with_(pos=_rattled(g.positions, 0.08, 6))).typed(),
           nm["gan_slab_skewed"].with_(pos=_rattled(nm["gan_slab_skewed"].pos, 0.04, 2)).typed(), nm["gan_wurtzite_rattled"].typed()]
    assert sorted(len(s[0]) for s in gan) == [4, 36, 36, 72]
    assert max(cc.face_nimg(gan[3][2], gan[3][3], cc.tersoff_cutoff(cc.gan_params()))) >= 2
    P = golden.tersoff_params
    eng = backend.TersoffEngine(P, device=0)
    _parity("tersoff GaN", eng, gan, lambda T, x, c, pbc: oracle_mod.tersoff(P, T, x, c, pbc)[0])
    eng.close()

    T8, X8, C8 = diamond_cell(SI_T3_A0)
    si = [(T8, X8, C8, ONES), (T8, _rattled(X8, 0.06, 1), C8, ONES), nm["si_simple_cubic"].typed(),
          nm["si_diamond_primitive"].with_(pos=_rattled(nm["si_diamond_primitive"].pos, 0.05, 3)).typed()]
    eng = backend.TersoffEngine(SI_T3, device=0)
    _parity("tersoff Si(C)", eng, si, lambda T, x, c, pbc: oracle_mod.tersoff(SI_T3, T, x, c, pbc)[0])
    eng.close()

    for nt, seed in ((3, 1), (5, 2)):
        Ps = synthetic_tersoff(nt, seed)
        boxes = [so.dense_box(n=100, box=9.5, min_dist=1.7, seed=3, nt=nt), so.dense_box(n=30, box=8.0, min_dist=1.9, seed=5, nt=nt)]
        rows = _padded_rows(*boxes[0][1:], cc.tersoff_cutoff(Ps))
        assert (rows > 16).any() and (rows <= 16).any()
        eng = backend.TersoffEngine(Ps, device=0)
        _parity(f"tersoff synthetic nt={nt}", eng, boxes, lambda T, x, c, pbc, Ps=Ps: oracle_mod.tersoff(Ps, T, x, c, pbc)[0])
        eng.close()


def test_sw_stress_is_the_strain_derivative_of_the_restatement():
    """1985 silicon on the dense box (rows of 10 .. 30 neighbors: both forms of the site kernel in one launch), the Si(111) 5x5 slab
    with its vacuum axis (V = |det cell| all the same) and a rattled copy, the skewed primitive cell and the self-image cell of
    tests/cell_cases.py; the three-species set on dense and sparse boxes."""
    from surface_sampling_amd import backend

    nm = cc.by_name(cc.battery())
    P = so.si_params()
    Z, X, Cl, pbc, _ = so.si_slab()
    T = np.zeros(len(Z), np.int32)
    pbc = pbc.astype(np.uint8)
    assert not pbc[2]
    dense = so.dense_box()
    rows = _padded_rows(*dense[1:], so.cutoff(P))
    assert (rows > 16).any() and (rows <= 16).any()
    prim = nm["si_diamond_primitive"]
    thin = nm["si_simple_cubic"]
    assert max(cc.face_nimg(thin.cell, thin.pbc, so.cutoff(P))) >= 2
    structs = [dense, (T, X, Cl, pbc), (T, _rattled(X, 0.08, 11), Cl, pbc), cc.skew_basis(prim.with_(pos=_rattled(prim.pos, 0.05, 4))).typed(),
               thin.typed()]
    eng = backend.SWEngine(P, device=0)
    _parity("sw Si", eng, structs, lambda T, x, c, pbc: so.sw(P, T, x, c, pbc)[0])
    eng.close()
    sp, P3, _ = so.three_species()
    structs = [so.dense_box(nt=3, seed=3), so.dense_box(n=30, box=9.0, min_dist=2.1, seed=9, nt=3)]
    eng = backend.SWEngine(P3, device=0)
    _parity("sw three species", eng, structs, lambda T, x, c, pbc: so.sw(P3, T, x, c, pbc)[0])
    eng.close()


def test_eam_funcfl_stress_is_the_strain_derivative_of_the_oracle_energy():
    """Cu_u3.eam on a rattled 108-atom fcc block, the 192-atom Cu(100) slab (vacuum axis), and from tests/cell_cases.py the skewed
    Cu(100) cell, the thin rattled two-atom cell and the one-atom primitive cell (343 images)."""
    import eam_oracle
    from surface_sampling_amd import backend

    nm = cc.by_name(cc.battery())
    fl = _cu()
    Xb, Cb = _fcc_block()
    Xs, Cs, ps = ao.cu100_slab()
    z = lambda n: np.zeros(n, np.int32)                                                  # noqa: E731
    structs = [(z(len(Xb)), _rattled(Xb, 0.06, 2), Cb, ONES), (z(len(Xs)), _rattled(Xs, 0.03, 3), Cs, ps)]
    structs += [nm[k].typed() for k in ("cu100_skewed", "cu_fcc_primitive_rattled2", "cu_fcc_primitive")]
    assert max(nm["cu_fcc_primitive_rattled2"].nimg) >= 2
    eng = backend.EAMEngine(fl, device=0)
    _parity("eam funcfl", eng, structs, lambda T, x, c, pbc: eam_oracle.eam(fl, x, c, pbc)[0])
    eng.close()


def test_eam_typed_stress_is_the_strain_derivative_of_the_restatement():
    """Cu/Au eam/alloy and an asymmetric eam/fs set (the two density derivatives of a mixed pair differ) on random alloys: a Cu(100)
    slab, a rattled periodic fcc block and the thin two-atom cell of tests/cell_cases.py as a Cu-Au pair."""
    from surface_sampling_amd import backend, eam

    cu, au = _cu(), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))
    forms = {"alloy": eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au))), ["Cu", "Au"]),
             "fs": eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (0.7, 1.3))), fs=True), ["Cu", "Au"])}
    Xs, Cs, ps = ao.cu100_slab(3, 3, 4)
    Xs = _rattled(Xs, 0.05, 1)
    Xb, Cb = _fcc_block(3.8, 2)
    Xb = _rattled(Xb, 0.07, 5)
    thin = cc.by_name(cc.battery())["cu_fcc_primitive_rattled2"]
    structs = [(ao.random_alloy(Xs, 0.3, 2), Xs, Cs, ps), (ao.random_alloy(Xb, 0.5, 3), Xb, Cb, ONES),
               (np.array([0, 1], np.int32), thin.pos, thin.cell, thin.pbc.astype(np.uint8))]
    assert all(0 < s[0].sum() < len(s[0]) for s in structs)       # both species in every chain
    res = {}
    for form, tab in forms.items():
        eng = backend.EAMEngine(tab, device=0)
        _parity(f"eam {form}", eng, structs, lambda T, x, c, pbc, tab=tab: ao.eam_typed(tab, T, x, c, pbc)[0])
        res[form] = eng.stress()[0]
        eng.close()
    assert np.abs(res["fs"] - res["alloy"]).max() > 1e-4          # the asymmetric densities matter on these states


# -- known answers through the device ---------------------------------------------------------------------------------------------
def test_sw_silicon_known_answers_through_the_device():
    """|sigma| < 1e-6 eV / A^3 at a0 = 5.430950 A; C11 and C12 from the device stresses at xx strains of +-1e-3: 151.4 and 76.4 GPa
    to the printed digit."""
    from surface_sampling_amd import backend

    T, X, Cl = so.diamond_si(so.SI_A0)
    d = 1e-3
    structs = [(T, X, Cl, ONES)] + [(T, *sf.strained((X, Cl), sf.voigt_strain(0, e)), ONES) for e in (d, -d)]
    eng = backend.SWEngine(so.si_params(), device=0)
    eng.evaluate_f64(structs)
    st, _ = eng.stress()
    eng.close()
    print("sigma(a0) =", st[0], "eV/A^3")
    assert np.abs(st[0]).max() < 1e-6
    Cij = (st[1] - st[2]) / (2 * d) * so.EV_A3_GPA
    print(f"C11 = {Cij[0]:.3f} GPa, C12 = {Cij[1]:.3f} / {Cij[2]:.3f} GPa")
    assert f"{Cij[0]:.1f}" == "151.4" and f"{Cij[1]:.1f}" == "76.4" and f"{Cij[2]:.1f}" == "76.4"


# -- consistency --------------------------------------------------------------------------------------------------------------------
def _engines():
    """(tag, engine factory, one stressed structure) for the three kinds."""
    from surface_sampling_amd import backend, eam

    cu, au = _cu(), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))
    fs = eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (0.7, 1.3))), fs=True), ["Cu", "Au"])
    Xb, Cb = _fcc_block(3.8, 2)
    Xb = _rattled(Xb, 0.07, 5)
    return [("tersoff", lambda: backend.TersoffEngine(synthetic_tersoff(3, 1), device=0), so.dense_box(n=60, box=8.5, seed=2, nt=3)),
            ("sw", lambda: backend.SWEngine(so.si_params(), device=0), so.dense_box()),
            ("eam/fs", lambda: backend.EAMEngine(fs, device=0), (ao.random_alloy(Xb, 0.5, 3), Xb, Cb, ONES))]


def test_rotation_covariance_repeatability_and_the_raw_entry_point():
    """The device stress of a rotated copy is R sigma R^T; two calls return identical bits; stress_std is all zeros; the C entry
    point accepts NULL for either output.  Rotation bound on the virial: 1e-9 x max(1, |V sigma|) eV -- the rotated coordinates
    differ from exact ones by 1e-16 relative, the second derivative that carries this into the virial is ~1e3 times the virial
    itself, the sums run over < 1e4 slots; two decades of margin on top."""
    R = cc.rotation(7)
    dp = C.POINTER(C.c_double)
    for tag, make, (T, X, Cl, pbc) in _engines():
        eng = make()
        small = (T[:20], X[:20] * 1.0, Cl * 1.5, pbc)             # chains of different sizes in one batch
        eng.evaluate_f64([(T, X, Cl, pbc), small, (T, X @ R.T, Cl @ R.T, pbc)])
        st, sd = eng.stress()
        st2, sd2 = eng.stress()
        assert np.array_equal(st, st2) and not sd.any() and not sd2.any()
        vol = abs(np.linalg.det(Cl))
        want = sf.rotated_voigt(st[0], R)
        diff = np.abs(st[2] - want).max() * vol
        print(f"{tag}: |R sigma R^T - sigma(rotated)| = {diff:.3e} eV on a virial of {np.abs(st[0]).max() * vol:.3e} eV")
        assert np.abs(st[0]).max() * vol > 1.0 and diff <= 1e-9 * max(1.0, np.abs(st[0]).max() * vol)
        a, b = np.zeros((3, 6)), np.full((3, 6), 7.0)
        lib, h = eng._lib, eng._h
        assert lib.vssr_batch_stress(h, a.ctypes.data_as(dp), None) == 0 and np.array_equal(a, st)
        assert lib.vssr_batch_stress(h, None, b.ctypes.data_as(dp)) == 0 and not b.any()
        assert lib.vssr_batch_stress(h, None, None) == 0
        # a chain's stress does not depend on what else is in the batch
        eng.evaluate_f64([small])
        assert np.array_equal(eng.stress()[0][0], st[1])
        eng.close()


# -- state rules ----------------------------------------------------------------------------------------------------------------------
def test_stress_needs_a_completed_run_that_produced_forces():
    from surface_sampling_amd import backend

    for tag, make, s in _engines():
        eng = make()
        eng.upload([s])
        with pytest.raises(backend.BackendError):                 # before any run
            eng.stress()
        eng.run(backend.WANT_ENERGY)
        with pytest.raises(backend.BackendError, match="energies only"):
            eng.stress()
        eng.run(backend.WANT_ENERGY | backend.WANT_FORCES)
        assert np.isfinite(eng.stress()[0]).all()
        eng.close()


def test_stress_after_the_chain_resident_cg_needs_one_plain_run(golden):
    """vssr_batch_relax_cg on Tersoff chains of <= 256 atoms runs the chain-resident minimiser, which leaves no batch-wide per-slot
    gradients: the call refuses; after one plain run it returns the stress of the relaxed positions, the bits a fresh engine gives."""
    from surface_sampling_amd import backend

    g = golden.structure("GaN_3x3_pristine")
    tg = np.array([0 if z == 31 else 1 for z in g.numbers], np.int32)
    structs = [(tg, _rattled(g.positions, s, seed), g.cell, ONES) for s, seed in ((0.05, 4), (0.02, 9), (0.1, 5))]
    eng = backend.TersoffEngine(golden.tersoff_params, device=0)
    eng.upload(structs)
    N = sum(len(s[0]) for s in structs)
    p = backend.CgParams.default(100, 10000, 1e-5, 1e-5)
    pos = np.zeros((N, 3))
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    eng._check(eng._lib.vssr_batch_relax_cg(eng._h, C.byref(p), None, want, pos.ctypes.data_as(C.POINTER(C.c_double)), None, None, None))
    assert np.abs(pos - np.concatenate([s[1] for s in structs])).max() > 1e-3
    with pytest.raises(backend.BackendError, match="run the batch once"):
        eng.stress()
    eng.run(want)
    st, _ = eng.stress()
    fresh = backend.TersoffEngine(golden.tersoff_params, device=0)
    o, relaxed = 0, []
    for T, _, Cl, pbc in structs:
        relaxed.append((T, pos[o:o + len(T)], Cl, pbc))
        o += len(T)
    fresh.evaluate_f64(relaxed)
    assert np.array_equal(st, fresh.stress()[0])
    eng.close(); fresh.close()


def test_stress_after_a_lock_step_fire_is_that_of_the_final_geometry():
    """FIRE on SW and EAM batches (a force tolerance no chain reaches in the given steps: the relaxation ends with its batch-wide
    evaluation of the final positions): the stress call succeeds directly and equals a fresh evaluation of those positions."""
    from surface_sampling_amd import backend

    for tag, make, (T, X, Cl, pbc) in _engines()[1:]:
        structs = [(T, X, Cl, pbc), (T, _rattled(X, 0.02, 8), Cl, pbc)]
        eng = make()
        eng.upload(structs)
        info = eng.relax_fire(max_steps=6, fmax=1e-9, want=backend.WANT_ENERGY | backend.WANT_FORCES)
        assert not info["converged"].any() and np.abs(info["positions"] - np.concatenate([s[1] for s in structs])).max() > 1e-4
        st, _ = eng.stress()
        n = len(T)
        fresh = make()
        fresh.evaluate_f64([(T, info["positions"][:n], Cl, pbc), (T, info["positions"][n:], Cl, pbc)])
        assert np.array_equal(st, fresh.stress()[0]), tag
        eng.close(); fresh.close()


# -- calculator surface -----------------------------------------------------------------------------------------------------------
def _calculators(golden, tmp_path):
    """(calculator, two structures) for the four analytic calculators."""
    from surface_sampling_amd import calculators as calcs
    from surface_sampling_amd.structures import Structure

    g = golden.structure("GaN_3x3_pristine")
    gan = [Structure(g.numbers, _rattled(g.positions, s, seed), g.cell, g.pbc) for s, seed in ((0.05, 4), (0.03, 7))]
    Z, X, Cl, pbc, _ = so.si_slab()
    si = [Structure(Z, _rattled(X, s, seed), Cl, pbc) for s, seed in ((0.04, 1), (0.08, 2))]
    Xs, Cs, ps = ao.cu100_slab(3, 3, 4)
    cu = [Structure(np.full(len(Xs), 29), _rattled(Xs, s, seed), Cs, ps.astype(bool)) for s, seed in ((0.05, 3), (0.02, 4))]
    lmp = calcs.LAMMPSSurfCalc()
    lmp.set(run_dir=_si_run_dir(tmp_path / "si", opt_model=so.SI_1985), relax_steps=4)
    return [(calcs.TersoffSurfCalc(golden.tersoff_params, ["Ga", "N"], device="cuda:0", relax_steps=4), gan),
            (calcs.SWSurfCalc(so.SI_1985, device="cuda:0", relax_steps=4), si),
            (calcs.EAMSurfCalc(files=[os.path.join(GOLDEN, "Cu_u3.eam")], device="cuda:0", relax_steps=4), cu),
            (lmp, si)]


def test_the_calculators_serve_stress_on_request_only(golden, tmp_path):
    for calc, (a, b) in _calculators(golden, tmp_path):
        name = type(calc).__name__
        packs = [calc._pack(a), calc._pack(b)]                   # (configures a LAMMPSSurfCalc from its run directory)
        fresh = calc._make_engine()
        fresh.evaluate_f64(packs)
        want = fresh.stress()[0]
        # a default calculate() does the work it did and leaves no stress; a later get_stress-style request computes it
        calc.calculate(a)
        assert "stress" not in calc.results and "energy" in calc.results, name
        got = calc.get_property("stress", a)
        assert got.shape == (6,) and got.dtype == np.float64 and np.array_equal(got, want[0]), name
        calc.calculate(b, properties=("energy", "stress"))
        assert np.array_equal(calc.results["stress"], want[1]), name
        calc.calculate(a, properties=("energy",))                # the entry of b must not survive a calculation of a
        assert "stress" not in calc.results, name
        out = calc.calculate_batch([a, b], want_stress=True)
        assert np.array_equal(out[0]["stress"], want[0]) and np.array_equal(out[1]["stress"], want[1]), name
        assert all("stress" not in r for r in calc.calculate_batch([a, b])), name
        for optimizer in ("LAMMPS", "FIRE"):
            rel = calc.relax_batch([a, b], relax_steps=4, optimizer=optimizer, want_stress=True)
            fresh.evaluate_f64([calc._pack(r[0]) for r in rel])
            st = fresh.stress()[0]
            assert np.array_equal(rel[0][4]["stress"], st[0]) and np.array_equal(rel[1][4]["stress"], st[1]), (name, optimizer)
            assert np.abs(rel[0][0].positions - a.positions).max() > 1e-6, (name, optimizer)
        assert all("stress" not in r[4] for r in calc.relax_batch([a, b], relax_steps=2)), name
        if "free_energy" in calc.implemented_properties:
            calc.calculate(a, properties=("energy", "free_energy", "energies"))
            assert calc.results["free_energy"] == calc.results["energy"], name
            assert np.array_equal(calc.results["energies"], calc.results["per_atom_energies"]), name
        fresh.close()


def test_a_painn_engine_returns_the_stress_it_returned(golden, oracle_mod):
    """The PaiNN path of the same entry point, one chain against the contract of tests/test_gpu_wrappers.py: central differences of
    the fp64 oracle energy at 2e-4, 3e-3 eV + 2e-4 relative on the virial; the ensemble spread is not zero there."""
    from surface_sampling_amd import backend

    table, const = golden.offset_table()
    s = golden.structure("O44Sr12Ti16")
    eng = backend.PainnEngine(golden.blobs, device=0, offset_per_z=table, offset_const=const)
    eng.evaluate([(s.numbers, s.positions, s.cell, s.pbc)])
    st, sd = eng.stress()
    eng.close()
    assert st.shape == (1, 6) and sd.shape == (1, 6) and (sd > 0).any()
    vol = abs(np.linalg.det(s.cell))
    delta = 2e-4
    for k in range(6):
        e = []
        for sign in (1.0, -1.0):
            X, Cl = sf.strained((s.positions, s.cell), sf.voigt_strain(k, sign * delta))
            e.append(oracle_mod.ensemble(golden.blobs, s.numbers, X, Cl, s.pbc, 64, table, const)["energy"])
        want = (e[0] - e[1]) / (2 * delta) / vol
        print(f"painn voigt {k}: device {st[0, k]:+.6e}  oracle FD {want:+.6e} eV/A^3")
        assert abs(st[0, k] - want) * vol <= 3e-3 + 2e-4 * abs(want) * vol
