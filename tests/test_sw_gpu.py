"""Stillinger-Weber on the MI355X: the published diamond-Si values, parity with the numpy restatement (tests/sw_oracle.py) on the
Si(111) 5x5 slab, a three-species set, dense rows beyond the LDS tile and transformed / partly periodic / self-image cells,
batch independence, FIRE / BFGS / CG relaxations and the batched MC through LAMMPSSurfCalc and SWSurfCalc."""
import numpy as np
import pytest

import cell_cases as cc
import sw_oracle as so
from test_sw_cpu import SRS, _si_run_dir

pytestmark = pytest.mark.gpu


def _engine(params):
    from surface_sampling_amd import backend

    return backend.SWEngine(params, device=0)


def _check(eng, P, structs, tag=""):
    """One batch on the device against the restatement of every structure: E 1e-10 relative, pe/atom 1e-9 eV, F 1e-8 eV/A."""
    e, ea, f = eng.evaluate_f64(structs)
    o = 0
    for b, (T, X, Cl, pbc) in enumerate(structs):
        n = len(T)
        E, EA, F = so.sw(P, T, X, Cl, pbc)
        assert abs(e[b] - E) <= 1e-10 * max(1.0, abs(E)), (tag, b, e[b], E)
        assert np.abs(ea[o:o + n] - EA).max() <= 1e-9, (tag, b)
        assert np.abs(f[o:o + n] - F).max() <= 1e-8, (tag, b, np.abs(f[o:o + n] - F).max())
        o += n
    return e, ea, f


def _slab_typed():
    Z, X, Cl, pbc, fixed = so.si_slab()
    return np.zeros(len(Z), np.int32), X, Cl, pbc.astype(np.uint8), fixed


def test_device_reproduces_the_published_diamond_values():
    P = so.si_params()
    eng = _engine(P)
    strains = (-0.01, -0.002, 0.0, 0.002, 0.01)
    structs = []
    for s in strains:
        T, X, Cl = so.diamond_si(so.SI_A0 * (1 + s))
        structs.append((T, X, Cl, np.ones(3, np.uint8)))
    T, X, Cl = so.diamond_si(so.SI_A0, reps=2)
    structs.append((T, X, Cl, np.ones(3, np.uint8)))
    e, ea, f = eng.evaluate_f64(structs)
    assert int(np.argmin(e[:5])) == 2
    assert e[2] / 8 == pytest.approx(-4.3366, abs=1e-9) and e[5] / 64 == pytest.approx(-4.3366, abs=1e-9)
    n0 = 8 * 2
    assert np.abs(f[n0:n0 + 8]).max() < 1e-10 and np.abs(f[40:]).max() < 1e-10
    assert np.allclose(ea[n0:n0 + 8], -4.3366, atol=1e-9)
    eng.close()


def test_parity_on_the_si111_slab_and_rattled_copies():
    P = so.si_params()
    T, X, Cl, pbc, _ = _slab_typed()
    rng = np.random.default_rng(11)
    structs = [(T, X, Cl, pbc)] + [(T, X + rng.normal(0, s, X.shape), Cl, pbc) for s in (0.03, 0.1, 0.2)]
    eng = _engine(P)
    _check(eng, P, structs, "slab")
    eng.close()


def test_parity_on_three_species_dense_rows_and_both_kernel_forms():
    """A three-species set parsed by the library (text) and given as an array: the same bits; dense boxes whose padded rows lie on
    both sides of the 16-slot LDS tile run both forms of the site kernel in one launch."""
    from surface_sampling_amd import backend

    sp, P, text = so.three_species()
    dense = [so.dense_box(nt=3, seed=s) for s in (3, 4)]
    for T, X, Cl, pbc in dense:
        i, _, _, _ = cc.brute_neighbors(X, Cl, pbc, so.cutoff(P))
        rows = 4 * np.ceil(np.bincount(i, minlength=len(X)) / 4)
        assert (rows > 16).any() and (rows <= 16).any()
    T, X, Cl, pbc, _ = _slab_typed()
    mixed = np.random.default_rng(2).integers(0, 3, len(T)).astype(np.int32)
    sparse = so.dense_box(n=30, box=9.0, min_dist=2.1, seed=9, nt=3)
    structs = dense + [(mixed, X + np.random.default_rng(3).normal(0, 0.05, X.shape), Cl, pbc), sparse]
    a = _engine(P)
    b = backend.SWEngine(text, device=0, species=sp)
    ra = _check(a, P, structs, "three-species")
    rb = b.evaluate_f64(structs)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    a.close(); b.close()


def _diamond_primitive():
    a0 = so.SI_A0
    cell = cc.fcc_primitive(a0)
    pos = np.array([[0.0, 0.0, 0.0], [a0 / 4, a0 / 4, a0 / 4]])
    return cc.Case("si_sw_primitive", "si", [14, 14], pos, cell, [1, 1, 1], None, None)


def test_parity_on_transformed_partly_periodic_and_self_image_cells():
    """Diamond Si in its 2-atom primitive cell (nimg >= 2 at the 3.77 A cutoff), periodic in 3, 2 and 1 directions, under every
    transform of tests/cell_cases.py; a simple-cubic cell with a 2.4 A edge (below the cutoff: an atom bonds to its own images)."""
    P = so.si_params()
    base = _diamond_primitive()
    rng = np.random.default_rng(4)
    cases = []
    for pbc in ([1, 1, 1], [1, 1, 0], [1, 0, 0]):
        c = base.with_(base.name + "".join(map(str, pbc)), pos=base.pos + rng.normal(0, 0.05, base.pos.shape), pbc=pbc)
        cases += [c] + cc.variants(c)
    assert any(v.pbc.sum() < 3 for v in cases)
    assert any(max(cc.face_nimg(c.cell, c.pbc, so.cutoff(P))) >= 2 for c in cases)
    sc = cc.Case("sc_2.4", "si", [14], np.zeros((1, 3)), np.eye(3) * 2.4, [1, 1, 1], None, None)
    sc2 = sc.with_("sc_2.4_open", pos=np.array([[0.1, 0.2, 0.3]]), pbc=[1, 1, 0])
    cases += [sc, sc2, cc.skew_basis(sc)]
    eng = _engine(P)
    _check(eng, P, [c.typed() for c in cases], "cells")
    eng.close()


def test_a_chain_is_bit_identical_alone_and_in_a_mixed_batch():
    sp, P, _ = so.three_species()
    T, X, Cl, pbc, _ = _slab_typed()
    slab = (T, X + np.random.default_rng(5).normal(0, 0.05, X.shape), Cl, pbc)
    others = [so.dense_box(nt=3, seed=7), so.dense_box(n=30, box=9.0, min_dist=2.1, seed=8, nt=3)]
    eng = _engine(P)
    e1, ea1, f1 = eng.evaluate_f64([slab])
    e2, ea2, f2 = eng.evaluate_f64([others[0], slab, others[1]])
    o = len(others[0][0])
    n = len(T)
    assert e2[1] == e1[0] and np.array_equal(ea2[o:o + n], ea1) and np.array_equal(f2[o:o + n], f1)
    eng.close()


@pytest.mark.parametrize("optimizer", ["FIRE", "BFGS", "LAMMPS"])
def test_relaxations_of_the_slab_hold_the_bulk_and_store_restated_energies(optimizer):
    from surface_sampling_amd.calculators import SWSurfCalc
    from surface_sampling_amd.structures import Structure

    Z, X, Cl, pbc, fixed = so.si_slab()
    rng = np.random.default_rng(6)
    slabs = [Structure(Z, X + np.where(fixed[:, None], 0.0, rng.normal(0, s, X.shape)), Cl, pbc) for s in (0.05, 0.1, 0.15)]
    held = np.flatnonzero(fixed)
    calc = SWSurfCalc(so.SI_1985, device="cuda:0")
    start = calc.calculate_batch(slabs)
    out = calc.relax_batch(slabs, fixed_indices=[held] * 3, relax_steps=40, fmax=0.05, optimizer=optimizer)
    P = so.si_params()
    for b, (relaxed, _, energy, oob, r) in enumerate(out):
        assert not oob and energy < start[b]["energy"] - 1e-3
        assert np.array_equal(relaxed.positions[held], slabs[b].positions[held])
        E, EA, F = so.sw(P, np.zeros(len(Z)), relaxed.positions, Cl, pbc)
        assert abs(E - energy) <= 1e-10 * abs(E)
        assert np.abs(r["per_atom_energies"] - EA).max() <= 1e-9
    if optimizer == "LAMMPS":
        assert calc._get_engine().last_relax_counts[0] > 1


def test_cg_compaction_and_trajectory_recording():
    """Live-chain compaction (forced on the small batch) gives the same relaxed slabs bit for bit; FIRE with trajectory records
    stores restated energies of the recorded geometries."""
    import os

    T, X, Cl, pbc, fixed = _slab_typed()
    rng = np.random.default_rng(8)
    structs = [(T, X + np.where(fixed[:, None], 0.0, rng.normal(0, s, X.shape)), Cl, pbc) for s in (0.02, 0.08, 0.12, 0.2)]
    mask = np.tile(fixed, 4).astype(np.uint8)
    P = so.si_params()
    eng = _engine(P)
    runs = []
    for env in ("0", "2"):
        os.environ["VSSR_RELAX_COMPACT"] = env
        try:
            runs.append(eng.relax_cg_f64(structs, fixed=mask, max_iter=60))
        finally:
            del os.environ["VSSR_RELAX_COMPACT"]
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(x, y)
    from surface_sampling_amd import backend

    eng.upload(structs)
    info = eng.relax_fire(fixed=mask, max_steps=12, fmax=0.01, want=backend.WANT_ENERGY | backend.WANT_FORCES, record_interval=4)
    tr = info["traj"]
    assert (tr["n_records"] >= 2).all()
    n = len(T)
    for b in range(4):
        for r in range(int(tr["n_records"][b])):
            E, _, _ = so.sw(P, T, tr["positions"][r, b * n:(b + 1) * n], Cl, pbc)
            assert abs(E - tr["energies"][r, b]) <= 1e-10 * abs(E)
    eng.close()


def _adatom_sites(X, Cl):
    ztop = X[:, 2].max()
    a, b = Cl[0], Cl[1]
    sites = np.array([(i + 0.3) / 4 * a + (j + 0.6) / 4 * b for i in range(4) for j in range(4)], float)
    sites[:, 2] = ztop + 1.6
    return sites


def test_batched_mc_on_si_adatom_sites_single_point_and_cg(tmp_path):
    """Semigrand MC with Si adatoms: single points through LAMMPSSurfCalc on a Si run directory (its relaxation is refused: the
    opt template names the SRS model), CG-relaxed through SWSurfCalc.  Stored energies = the restatement's, two runs agree."""
    from surface_sampling_amd import backend, mc
    from surface_sampling_amd.calculators import LAMMPSSurfCalc, SWSurfCalc
    from surface_sampling_amd.structures import Structure

    Z, X, Cl, pbc, fixed = so.si_slab()
    g = Structure(Z, X, Cl, pbc)
    held = np.flatnonzero(fixed)
    sites = _adatom_sites(X, Cl)
    P = so.si_params()
    rd = _si_run_dir(tmp_path / "si")
    for relax in (False, True):
        runs = []
        for _ in range(2):
            if relax:
                calc = SWSurfCalc(so.SI_1985, device="cuda:0")
                calc.set(relax_steps=25)
            else:
                calc = LAMMPSSurfCalc(device="cuda:0")
                calc.set(run_dir=rd, relax_steps=25)
                with pytest.raises(backend.BackendError, match=SRS):
                    calc.relax_batch([g])
            ens = mc.ChainEnsemble(g, sites, ("Si",), 6, calc, seed=3, relax=relax, relax_steps=25, fixed_indices=held,
                                   temperature=0.5, optimizer="LAMMPS")
            ens.initialize()
            for _ in range(4):
                ens.step_semigrand()
            assert (ens.num_adsorbates() > 0).any()
            for b in range(6):
                r = ens.relaxed[b]
                E, _, _ = so.sw(P, np.zeros(len(r.numbers), np.int32), r.positions, r.cell, [1, 1, 0])
                assert abs(E - ens.state.energy[b]) <= 1e-9 * max(1.0, abs(E)), (relax, b)
                if relax:
                    assert np.array_equal(r.positions[held], g.positions[held])
            runs.append((ens.state.species.copy(), ens.state.energy.copy()))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
