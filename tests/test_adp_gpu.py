"""Angular-dependent potential on the MI355X (vssr_eam_create_adp, csrc/adp.hip) against the numpy restatement tests/adp_oracle.py:
parity on two- and three-element slabs, a skewed cell thinner than the cutoff, partly periodic cells, a lone atom and a dimer;
the reductions to eam/alloy; batch independence; stress; FIRE / BFGS / CG against their restatements, live-chain compaction and
trajectory records; the calculators and a semigrand MC; refusals.

Tolerances are those tests/test_eam_alloy_gpu.py applies to the same fp64 quantities: E 1e-9 relative (floor 1 eV), pe/atom 1e-9 eV,
F 1e-8 eV/A; stress: ten times the uncertainty of the strain derivative of the restatement (tests/strain_fd.py), as
tests/test_pair_gpu.py.  Every figure is printed before it is asserted.  No executed LAMMPS is compared."""
import json
import os

import numpy as np
import pytest

import adp_oracle as adp
import eam_alloy_oracle as ao
import strain_fd as sf
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

E_REL, EA_ABS, F_ABS, STRESS_FACTOR = 1e-9, 1e-9, 1e-8, 10.0


@pytest.fixture(scope="module")
def fl():
    from surface_sampling_amd import eam

    return eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))


@pytest.fixture(scope="module")
def tab2(fl):
    """(Cu, Au) through the file writer and reader, as a user would load it."""
    from surface_sampling_amd import eam

    return eam.tables_from_adp(eam.parse_adp(eam.write_adp(adp.cuau_adp(*fl))), ["Cu", "Au"])


@pytest.fixture(scope="module")
def tab3(fl):
    from surface_sampling_amd import eam

    return eam.tables_from_adp(eam.parse_adp(eam.write_adp(adp.cuauag_adp(*fl))), ["Cu", "Au", "Ag"])


def _lone():
    return np.array([1], np.int32), np.array([[1.0, 2.0, 3.0]]), np.diag([9.0, 10.0, 11.0]), np.array([1, 1, 0], np.uint8)


def _dimer():
    return (np.array([2, 0], np.int32), np.array([[0.3, -0.2, 0.1], [0.3 + 0.6 * 2.7, -0.2, 0.1 + 0.8 * 2.7]]), np.eye(3) * 30.0,
            np.zeros(3, np.uint8))


def _check(eng, tab, structs, tag, stress=()):
    """Device against the restatement; ``stress``: indices of the chains whose virial is checked as well."""
    e, ea, f = eng.evaluate_f64(structs)
    st = eng.stress()[0] if len(stress) else None
    o = 0
    for b, (T, X, Cl, pbc) in enumerate(structs):
        n = len(T)
        E, EA, F = adp.adp(tab, T, X, Cl, pbc)
        de, dea, df = abs(e[b] - E), np.abs(ea[o:o + n] - EA).max(), np.abs(f[o:o + n] - F).max()
        print(f"{tag} chain {b} ({n} atoms): E {E:+.12e}  |dE| {de:.2e}  max|d pe/atom| {dea:.2e}  max|dF| {df:.2e}  max|F| {np.abs(F).max():.3e}")
        assert de <= E_REL * max(1.0, abs(E)), (tag, b, e[b], E)
        assert dea <= EA_ABS, (tag, b, dea)
        assert df <= F_ABS, (tag, b, df)
        if b in stress:
            chk = sf.fd_stress(lambda x, c: adp.adp(tab, T, x, c, pbc)[0], X, Cl)
            dev = st[b] * chk.volume
            ratio = np.abs(dev - chk.virial) / chk.unc
            print(f"{tag} chain {b} virial: device {dev}  checker {chk.virial}  unc {chk.unc}  max ratio {ratio.max():.3f}")
            assert (np.abs(dev - chk.virial) <= STRESS_FACTOR * chk.unc).all(), (tag, b, dev, chk.virial, chk.unc)
            W0 = adp.adp(tab, T, X, Cl, pbc, angular=False, virial=True)[3]
            assert np.abs(chk.virial - W0).max() > 100 * chk.unc.max(), (tag, b)     # the angular virial is resolved
        o += n
    return e, ea, f


# ---- parity ----------------------------------------------------------------------------------------------------------------------
def test_two_element_states_match_the_restatement(tab2):
    from surface_sampling_amd import backend

    structs = adp.cu100_states()
    assert max(len(s[0]) for s in structs) == 192
    eng = backend.EAMEngine(tab2, device=0)
    e = _check(eng, tab2, structs, "Cu/Au")[0]
    e0 = np.array([adp.adp(tab2, *s, angular=False)[0] for s in structs])
    assert np.abs(e - e0).min() > 1e-2                                 # the angular terms matter on every one of these states
    eng.close()


def test_three_elements_thin_skewed_and_partly_periodic_cells_with_stress(tab3):
    """One ragged batch: the three-element 4 x 4 x 3 slab under pbc TTF and TFF, the skewed cell whose atoms see their own images,
    a lone atom (empty row) and a dimer; stress on the slab and on the skewed cell."""
    from surface_sampling_amd import backend

    structs = [adp.three_element_slab((1, 1, 0)), adp.three_element_slab((1, 0, 0)), adp.skewed_thin_cell(), _lone(), _dimer()]
    assert sorted(set(structs[0][0].tolist())) == [0, 1, 2]
    ii, jj, _ = ao.neighbor_pairs(*structs[2][1:], tab3.cutoff)
    assert (ii == jj).sum() >= 6                                       # self images
    eng = backend.EAMEngine(tab3, device=0)
    e, ea, f = _check(eng, tab3, structs, "three elements", stress=(0, 2))
    assert np.abs(f[-3]).max() == 0.0 and ea[-3] == e[3]              # the lone atom: F(0) and no force
    # the skewed cell: the images of an atom cancel in mu and not in lambda
    T, X, Cl, pbc = structs[2]
    assert abs(e[2] - adp.adp(tab3, T, X, Cl, pbc, angular=False)[0]) > 1e-2
    eng.close()


# ---- reductions ------------------------------------------------------------------------------------------------------------------
def test_zero_angular_tables_and_cubic_sites_give_the_alloy_handle(fl, tab3):
    from surface_sampling_amd import backend, eam

    zero = eam.tables_from_adp(adp.cuauag_adp(*fl, scale=0.0), ["Cu", "Au", "Ag"])
    assert not zero.u.any() and not zero.w.any()
    alloy = eam.tables_from_setfl(adp.cuauag_adp(*fl), ["Cu", "Au", "Ag"])
    assert alloy.u is None
    structs = [adp.three_element_slab(), adp.skewed_thin_cell(), adp.cu100_states()[2], _dimer()]
    a, z, full = backend.EAMEngine(alloy, device=0), backend.EAMEngine(zero, device=0), backend.EAMEngine(tab3, device=0)
    ea_, eaa, fa = a.evaluate_f64(structs)
    ez, eaz, fz = z.evaluate_f64(structs)
    print("u = w = 0 against eam/alloy: |dE|", np.abs(ez - ea_).max(), " |d pe/atom|", np.abs(eaz - eaa).max(), " |dF|", np.abs(fz - fa).max())
    assert (np.abs(ez - ea_) <= E_REL * np.maximum(1.0, np.abs(ea_))).all()
    assert np.abs(eaz - eaa).max() <= EA_ABS and np.abs(fz - fa).max() <= F_ABS
    assert np.abs(full.evaluate_f64(structs)[0] - ea_).min() > 1e-3    # the full tables are another potential
    # perfect fcc, one atom per cell, each element: cubic site symmetry, the angular energy vanishes although u, w do not
    T, X, Cl, pbc = adp.fcc_bulk()
    bulk = [(T + t, X, Cl, pbc) for t in (0, 1, 2)]
    eb, eab, fb = full.evaluate_f64(bulk)
    e0 = a.evaluate_f64(bulk)[0]
    print("fcc: ADP", eb, " eam/alloy", e0)
    assert (np.abs(eb - e0) <= E_REL * np.maximum(1.0, np.abs(e0))).all() and np.abs(fb).max() <= F_ABS
    for eng in (a, z, full):
        eng.close()


def test_swapping_type_labels_with_their_tables_changes_no_energy(fl, tab3):
    from surface_sampling_amd import backend, eam

    base = adp.cuauag_adp(*fl)
    T, X, Cl, pbc = adp.three_element_slab()
    sym = np.array(base.elements)[T]
    ref = backend.EAMEngine(tab3, device=0)
    e0 = ref.evaluate_f64([(T, X, Cl, pbc)])[0][0]
    ref.close()
    for order, names in (((2, 0, 1), ["Ag", "Cu", "Au"]), ((1, 0, 2), ["Cu", "Ag", "Au"])):
        t = eam.tables_from_adp(eam.parse_adp(eam.write_adp(adp.permuted(base, order))), names)
        Tp = np.array([names.index(x) for x in sym], np.int32)
        assert (Tp != T).any()
        eng = backend.EAMEngine(t, device=0)
        e1 = eng.evaluate_f64([(Tp, X, Cl, pbc)])[0][0]
        eng.close()
        print(f"labels {names}: E {e1:+.12e}  against {e0:+.12e}")
        assert abs(e1 - e0) <= E_REL * max(1.0, abs(e0))


# ---- batch independence ----------------------------------------------------------------------------------------------------------
def test_a_chain_is_bit_identical_alone_and_in_a_ragged_batch(tab3):
    from surface_sampling_amd import backend

    structs = [_lone(), adp.cu100_states()[4], _dimer(), adp.three_element_slab(), adp.skewed_thin_cell(), adp.relax_case()[0],
               adp.cu100_states()[1]]
    assert sorted(len(s[0]) for s in structs) == [1, 2, 3, 10, 32, 96, 192]
    eng = backend.EAMEngine(tab3, device=0)
    e, ea, f = eng.evaluate_f64(structs)
    o = 0
    for b, s in enumerate(structs):
        n = len(s[0])
        e1, ea1, f1 = eng.evaluate_f64([s])
        assert e1[0] == e[b] and np.array_equal(ea1, ea[o:o + n]) and np.array_equal(f1, f[o:o + n]), b
        o += n
    eng.close()


# ---- relaxation ------------------------------------------------------------------------------------------------------------------
def _fn(tab, T, Cl, pbc):
    def fn(p):
        E, _, F = adp.adp(tab, T, p, Cl, pbc)
        return E, F
    return fn


def test_cg_follows_the_restatement_and_the_resident_request_runs_in_lock_step(tab2):
    from cg_oracle import cg_minimize
    from surface_sampling_amd import backend

    (T, X, Cl, pbc), mask = adp.relax_case()
    assert len(T) == 32 and mask.sum() == 8 and set(T.tolist()) == {0, 1}
    eng = backend.EAMEngine(tab2, device=0)
    res = eng.relax_cg_f64([(T, X, Cl, pbc)], fixed=mask, max_iter=60)
    e, ea, f, pos, it, ev, why = res
    assert eng.last_cg_driver == "lockstep"
    pref, eref, niter, neval, reason, _ = cg_minimize(_fn(tab2, T, Cl, pbc), X, fixed=np.flatnonzero(mask), max_iter=60)
    print(f"CG: device {it[0]} iterations {ev[0]} evaluations stop {why[0]}; restatement {niter} {neval} {reason}; "
          f"|dE| {abs(e[0] - eref):.2e}  max|dx| {np.abs(pos - pref).max():.2e}")
    assert (it[0], ev[0], why[0]) == (niter, neval, reason)
    assert abs(e[0] - eref) < 1e-9 and np.abs(pos - pref).max() < 1e-9
    assert eref < adp.adp(tab2, T, X, Cl, pbc)[0] - 0.1
    assert np.array_equal(pos[:8], X[:8])                              # the bottom layer stayed
    again = eng.relax_cg_f64([(T, X, Cl, pbc)], fixed=mask, max_iter=60, driver="resident")
    assert eng.last_cg_driver == "lockstep"                            # no chain-resident minimiser for an ADP handle
    for x, y in zip(res, again):
        assert np.array_equal(x, y)
    eng.close()


@pytest.mark.parametrize("optimizer", ["FIRE", "BFGS"])
def test_fire_and_bfgs_follow_the_restatements(tab2, optimizer):
    from bfgs_oracle import bfgs_relax
    from fire_oracle import fire_relax
    from surface_sampling_amd import backend

    (T, X, Cl, pbc), mask = adp.relax_case()
    eng = backend.EAMEngine(tab2, device=0)
    e, ea, f, pos, nst, conv = eng.relax_f64([(T, X, Cl, pbc)], fixed=mask, max_steps=12, fmax=0.01, optimizer=optimizer)
    relax = fire_relax if optimizer == "FIRE" else bfgs_relax
    pref, _, steps, _ = relax(_fn(tab2, T, Cl, pbc), X, fixed=np.flatnonzero(mask), max_steps=12, fmax=0.01)
    eref = adp.adp(tab2, T, pref, Cl, pbc)[0]
    print(f"{optimizer}: device {nst[0]} steps, restatement {steps}; max|dx| {np.abs(pos - pref).max():.2e}  |dE| {abs(e[0] - eref):.2e}")
    assert nst[0] == steps
    assert np.abs(pos - pref).max() < 1e-7
    assert abs(e[0] - eref) < 1e-7
    assert np.abs(pos - X).max() > 1e-3 and np.array_equal(pos[:8], X[:8])
    eng.close()


def test_compaction_and_trajectory_records_change_nothing(tab2, monkeypatch):
    """Four copies of the 32-atom slab with different rattles stop at different times: with VSSR_RELAX_COMPACT=2 the resident batch
    is compacted while the CG runs, with the same bits; the energies FIRE records on the way are the restatement's."""
    from surface_sampling_amd import backend

    (T, X, Cl, pbc), mask = adp.relax_case()
    structs = [(T, X + np.random.default_rng(20 + k).normal(0, s, X.shape) * (1 - mask[:, None]), Cl, pbc)
               for k, s in enumerate((0.0, 0.02, 0.05, 0.002))]
    masks = np.tile(mask, len(structs))
    eng = backend.EAMEngine(tab2, device=0)
    runs = []
    for flag in ("0", "2"):
        monkeypatch.setenv("VSSR_RELAX_COMPACT", flag)
        runs.append(eng.relax_cg_f64(structs, fixed=masks, max_iter=60))
        assert eng.last_cg_driver == "lockstep"
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    print("CG evaluations per chain:", runs[0][5])
    assert runs[0][5].min() < runs[0][5].max()                       # the chains stop at different times
    eng.upload(structs)
    info = eng.relax_fire(fixed=masks, max_steps=12, fmax=0.01, want=backend.WANT_ENERGY | backend.WANT_FORCES, record_interval=4)
    tr = info["traj"]
    assert (tr["n_records"] >= 2).all()
    for b in range(len(structs)):
        for r in range(int(tr["n_records"][b])):
            E = adp.adp(tab2, T, tr["positions"][r, 32 * b:32 * b + 32], Cl, pbc)[0]
            assert abs(E - tr["energies"][r, b]) <= E_REL * max(1.0, abs(E)), (b, r, E, tr["energies"][r, b])
    eng.close()


# ---- front end -------------------------------------------------------------------------------------------------------------------
def test_lammps_run_surf_calc_reads_an_adp_file(fl, tab3, tmp_path):
    from surface_sampling_amd import eam
    from surface_sampling_amd.calculators import LAMMPSRunSurfCalc
    from surface_sampling_amd.structures import Structure

    path = str(tmp_path / "CuAuAg.adp")
    eam.write_adp(adp.cuauag_adp(*fl), path)
    T, X, Cl, pbc = adp.three_element_slab()
    numbers = np.array([29, 79, 47])[T]
    calc = LAMMPSRunSurfCalc(files=[path], device="cuda:0")
    calc.set(pair_style="adp", pair_coeff=["* * CuAuAg.adp Cu Au Ag"])
    calc.calculate(Structure(numbers, X, Cl, pbc.astype(bool)), properties=("energy", "forces", "stress", "energies"))
    E, EA, F = adp.adp(tab3, T, X, Cl, pbc)
    chk = sf.fd_stress(lambda x, c: adp.adp(tab3, T, x, c, pbc)[0], X, Cl)
    r = calc.results
    dev = np.asarray(r["stress"]) * chk.volume
    print(f"calculator: |dE| {abs(r['energy'] - E):.2e}  max|dF| {np.abs(r['forces'] - F).max():.2e}  virial ratio {(np.abs(dev - chk.virial) / chk.unc).max():.3f}")
    assert abs(r["energy"] - E) <= E_REL * max(1.0, abs(E))
    assert np.abs(r["energies"] - EA).max() <= EA_ABS and np.abs(r["forces"] - F).max() <= F_ABS
    assert (np.abs(dev - chk.virial) <= STRESS_FACTOR * chk.unc).all()
    calc.calculate(Structure(numbers, X, Cl, pbc.astype(bool)))
    assert "stress" not in calc.results                               # on request only, as for the other EAM forms


def test_semigrand_mc_of_8_chains_through_a_run_directory(fl, tmp_path):
    from surface_sampling_amd import eam, mc
    from surface_sampling_amd.calculators import LAMMPSSurfCalc
    from surface_sampling_amd.structures import Structure

    path = str(tmp_path / "CuAu.adp")
    eam.write_adp(adp.cuau_adp(*fl), path)
    rd = tmp_path / "run"
    rd.mkdir()
    (rd / "lammps_config.json").write_text(json.dumps({"potential_file": path, "atoms": ["Cu", "Au"], "bulk_index": 4}))
    for name in ("lammps_energy_template.txt", "lammps_opt_template.txt"):
        (rd / name).write_text("units metal\nboundary p p p\npair_style adp\npair_coeff * * {} {}\n")
    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    g = Structure(d["numbers"], d["positions"], d["cell"], d["pbc"])
    tab = eam.tables_from_adp(eam.read_adp(path), ["Cu", "Au"])
    for relax in (False, True):
        calc = LAMMPSSurfCalc(device="cuda:0")
        calc.set(run_dir=str(rd), relax_steps=20)
        ens = mc.ChainEnsemble(g, d["ads_coords"], ("Cu", "Au"), 8, calc, seed=11, relax=relax, relax_steps=20,
                               fixed_indices=np.arange(4), temperature=0.5, optimizer="LAMMPS")
        ens.initialize()
        for _ in range(10):
            ens.step_semigrand()
        nums = np.concatenate([ens.relaxed[b].numbers for b in range(8)])
        assert (nums == 79).any() and (nums == 29).sum() > 8 * len(g.numbers)     # both species were placed
        for b in range(8):
            r = ens.relaxed[b]
            T = np.where(np.asarray(r.numbers) == 79, 1, 0)
            E = adp.adp(tab, T, r.positions, r.cell, [1, 1, 1])[0]
            E0 = adp.adp(tab, T, r.positions, r.cell, [1, 1, 1], angular=False)[0]
            print(f"relax {relax} chain {b}: {len(T)} atoms  E {E:+.10f}  device {ens.state.energy[b]:+.10f}  angular part {E - E0:+.3e}")
            assert abs(E - ens.state.energy[b]) <= E_REL * max(1.0, abs(E)), (relax, b, E, ens.state.energy[b])
            assert abs(E - E0) > 1e-2


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_bad_tables_and_types_are_refused_and_the_handle_goes_on(tab3):
    from surface_sampling_amd import backend, eam

    def copy(**kw):
        f = dict(elements=tab3.elements, fs=False, nrho=tab3.nrho, drho=tab3.drho, nr=tab3.nr, dr=tab3.dr, cutoff=tab3.cutoff,
                 frho=tab3.frho, rhor=tab3.rhor, z2r=tab3.z2r, u=tab3.u, w=tab3.w)
        f.update(kw)
        return eam.EamTables(**f)

    eng = backend.EAMEngine(tab3, device=0)
    batch = [adp.three_element_slab(), adp.skewed_thin_cell()]
    first = eng.evaluate_f64(batch)
    w = tab3.w.copy()
    w[4, 17] = np.nan
    u = tab3.u.copy()
    u[0, 3] = np.inf
    frho = tab3.frho.copy()
    frho[2, 7] = np.nan
    for bad in (copy(w=w), copy(u=u), copy(u=None), copy(w=None), copy(frho=frho)):
        with pytest.raises(backend.BackendError, match=r"vssr_eam_create_adp failed \(-1\)"):
            backend.EAMEngine(bad, device=0)
    T, X, Cl, pbc = batch[0]
    for bad in (3, -1):
        t = T.copy()
        t[5] = bad
        with pytest.raises(backend.BackendError, match="vssr error -1"):
            eng.evaluate_f64([(t, X, Cl, pbc)])
    for x, y in zip(first, eng.evaluate_f64(batch)):                   # the handle serves the next batch with identical bits
        assert np.array_equal(x, y)
    eng.close()
