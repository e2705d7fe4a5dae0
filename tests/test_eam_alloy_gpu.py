"""Several-element EAM on the MI355X (vssr_eam_create_alloy): parity with the numpy restatement (tests/eam_alloy_oracle.py) for
eam/alloy, an asymmetric eam/fs set and mixed funcfl files on Cu/Au states; the one-element reductions against the funcfl handle
and the reference's numbers; batch independence; type refusals; CG / FIRE / BFGS relaxations against their restatements, with
and without live-chain compaction; semigrand Au/Cu MC over 64 chains through LAMMPSSurfCalc."""
import itertools
import json
import os

import numpy as np
import pytest

import eam_alloy_oracle as ao
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fl():
    from surface_sampling_amd import eam

    return eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))


def _forms(fl):
    """{form: EamTables with types (Cu, Au)} -- through the file readers, as a user would load them."""
    from surface_sampling_amd import eam

    cu, au = fl
    return {
        "alloy": eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au))), ["Cu", "Au"]),
        "fs": eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (0.7, 1.3))), fs=True), ["Cu", "Au"]),
        "funcfl": eam.tables_from_funcfl([cu, au]),
    }


def _states():
    """Cu(100) with Au / Cu adatoms, Au(110) with Cu adatoms, and generated Cu(100) slabs with random Au substitution."""
    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    out = []
    for k, sub in enumerate(((3,), (2, 9), (0, 5, 11), (1, 4, 7, 12))):
        pos = np.vstack([d["positions"], d["ads_coords"][list(sub)]])
        t = np.concatenate([np.zeros(len(d["positions"]), np.int32), (np.arange(len(sub)) + k) % 2])
        out.append((t.astype(np.int32), pos, d["cell"], d["pbc"].astype(np.uint8)))
    a = np.load(os.path.join(GOLDEN, "au110.npz"))
    pos = np.vstack([a["positions"], a["ads_coords"][[0, 3, 5]]])
    out.append((np.concatenate([np.ones(len(a["positions"]), np.int32), np.zeros(3, np.int32)]), pos, a["cell"],
                a["pbc"].astype(np.uint8)))
    for seed, frac in ((1, 0.1), (2, 0.3), (3, 0.5)):
        pos, cell, pbc = ao.cu100_slab(4, 4, 6)
        pos = pos + np.random.default_rng(seed).normal(0, 0.05, pos.shape)
        out.append((ao.random_alloy(pos, frac, seed), pos, cell, pbc))
    return out


def _check(eng, tab, structs, tag):
    e, ea, f = eng.evaluate_f64(structs)
    o = 0
    for b, (T, X, Cl, pbc) in enumerate(structs):
        n = len(T)
        E, EA, F = ao.eam_typed(tab, T, X, Cl, pbc)
        assert abs(e[b] - E) <= 1e-9 * max(1.0, abs(E)), (tag, b, e[b], E)
        assert np.abs(ea[o:o + n] - EA).max() <= 1e-9, (tag, b)
        assert np.abs(f[o:o + n] - F).max() <= 1e-8, (tag, b, np.abs(f[o:o + n] - F).max())
        o += n
    return e, ea, f


def test_device_matches_the_restatement_for_all_three_forms(fl):
    from surface_sampling_amd import backend

    structs = _states()
    assert max(len(s[0]) for s in structs) == 192
    res = {}
    for form, tab in _forms(fl).items():
        eng = backend.EAMEngine(tab, device=0)
        res[form] = _check(eng, tab, structs, form)
        eng.close()
    assert np.abs(res["fs"][0] - res["alloy"][0]).max() > 1e-2        # the asymmetric densities matter on these states


def test_one_element_setfl_equals_the_funcfl_handle_and_the_reference_numbers(fl):
    from surface_sampling_amd import backend, eam

    with open(os.path.join(GOLDEN, "eam_kat.json")) as fh:
        kat = json.load(fh)
    for f, case in zip(fl, ("cu", "au")):
        tab = eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(eam.funcfl_to_setfl(f))), [eam.funcfl_to_setfl(f).elements[0]])
        if case == "cu":
            d = np.load(os.path.join(GOLDEN, "cu100.npz"))
            bridge = int(np.flatnonzero(d["site_kind"] == 1)[0])
            subs = [(bridge,), (2, 9), ()]
            target = kat["min_energy_one_bridge_adatom"]["value"]
            k = None
        else:
            d = np.load(os.path.join(GOLDEN, "au110.npz"))
            k = kat["au110"]["num_ads_atoms"]
            subs = list(itertools.combinations(range(len(d["ads_coords"])), k))
            target = kat["au110"]["min_energy"]["value"]
        structs = [(np.zeros(len(d["positions"]) + len(s), np.int32), np.vstack([d["positions"], d["ads_coords"][list(s)]]),
                    d["cell"], d["pbc"].astype(np.uint8)) for s in subs]
        typed, plain = backend.EAMEngine(tab, device=0), backend.EAMEngine(f, device=0)
        e1, ea1, f1 = typed.evaluate_f64(structs)
        e0, ea0, f0 = plain.evaluate_f64(structs)
        assert (np.abs(e1 - e0) <= 1e-12 * np.abs(e0)).all()
        assert np.abs(ea1 - ea0).max() <= 1e-12 * np.abs(ea0).max() and np.abs(f1 - f0).max() <= 1e-12 * max(1.0, np.abs(f0).max())
        if case == "cu":
            assert np.allclose(e1[0], target)
        else:
            e = np.sort(e1)
            assert np.allclose(e[0], target) and min(abs(x - target) for x in e[:2]) < 1e-11
        typed.close()
        plain.close()


def test_fs_with_symmetric_densities_is_the_alloy_bit_for_bit(fl):
    from surface_sampling_amd import backend, eam

    cu, au = fl
    alloy = eam.tables_from_setfl(ao.cuau_setfl(cu, au), ["Cu", "Au"])
    fs1 = eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (1.0, 1.0))), fs=True), ["Cu", "Au"])
    structs = _states()
    a, b = backend.EAMEngine(alloy, device=0), backend.EAMEngine(fs1, device=0)
    for x, y in zip(a.evaluate_f64(structs), b.evaluate_f64(structs)):
        assert np.array_equal(x, y)
    a.close()
    b.close()


def test_a_chain_is_bit_identical_alone_and_in_a_batch(fl):
    from surface_sampling_amd import backend

    structs = _states()
    eng = backend.EAMEngine(_forms(fl)["fs"], device=0)
    e, ea, f = eng.evaluate_f64(structs)
    o = 0
    for b, s in enumerate(structs):
        n = len(s[0])
        e1, ea1, f1 = eng.evaluate_f64([s])
        assert e1[0] == e[b] and np.array_equal(ea1, ea[o:o + n]) and np.array_equal(f1, f[o:o + n]), b
        o += n
    eng.close()


def test_types_outside_the_table_and_bad_tables_are_refused(fl):
    from surface_sampling_amd import backend, eam

    tab = _forms(fl)["alloy"]
    eng = backend.EAMEngine(tab, device=0)
    T, X, Cl, pbc = _states()[0]
    for bad in (2, -1):
        t = T.copy()
        t[3] = bad
        with pytest.raises(backend.BackendError, match="vssr error -1"):
            eng.evaluate_f64([(t, X, Cl, pbc)])
    eng.evaluate_f64([(T, X, Cl, pbc)])                                # the handle still works
    eng.close()
    nan = eam.EamTables(tab.elements, False, tab.nrho, tab.drho, tab.nr, tab.dr, tab.cutoff, tab.frho.copy(), tab.rhor, tab.z2r)
    nan.frho[1, 7] = np.nan
    with pytest.raises(backend.BackendError, match=r"failed \(-1\)"):
        backend.EAMEngine(nan, device=0)
    nine = eam.EamTables(["Cu"] * 9, False, tab.nrho, tab.drho, tab.nr, tab.dr, tab.cutoff, np.tile(tab.frho[:1], (9, 1)),
                         np.tile(tab.rhor[:1], (9, 1)), np.tile(tab.z2r[:1], (45, 1)))
    with pytest.raises(backend.BackendError, match=r"failed \(-1\)"):
        backend.EAMEngine(nine, device=0)


def _relax_case(n_chains=3):
    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    out = []
    for k in range(n_chains):
        sub = [(2 + 3 * k) % len(d["ads_coords"]), (9 + 5 * k) % len(d["ads_coords"])]
        pos = np.vstack([d["positions"], d["ads_coords"][sub]]) + np.random.default_rng(k).normal(0, 0.03, (10, 3))
        t = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1, k % 2], np.int32)
        out.append((t, pos, d["cell"], d["pbc"].astype(np.uint8)))
    return out, np.tile(np.array([1] * 4 + [0] * 6, np.uint8), n_chains)


def test_cg_follows_the_restatement(fl):
    from cg_oracle import cg_minimize
    from surface_sampling_amd import backend

    tab = _forms(fl)["fs"]
    structs, mask = _relax_case()
    eng = backend.EAMEngine(tab, device=0)
    e, ea, f, pos, it, ev, why = eng.relax_cg_f64(structs, fixed=mask, max_iter=60)
    for b, (T, X, Cl, pbc) in enumerate(structs):
        def fn(p, T=T, Cl=Cl, pbc=pbc):
            E, _, F = ao.eam_typed(tab, T, p, Cl, pbc)
            return E, F

        pref, eref, niter, neval, reason, _ = cg_minimize(fn, X, fixed=np.arange(4), max_iter=60)
        assert (it[b], ev[b], why[b]) == (niter, neval, reason), (b, it[b], ev[b], why[b], niter, neval, reason)
        assert abs(e[b] - eref) < 1e-9 and np.abs(pos[10 * b:10 * b + 10] - pref).max() < 1e-9
        assert eref < ao.eam_typed(tab, T, X, Cl, pbc)[0] - 0.1
    eng.close()


@pytest.mark.parametrize("optimizer", ["FIRE", "BFGS"])
def test_fire_and_bfgs_follow_the_restatements(fl, optimizer):
    from bfgs_oracle import bfgs_relax
    from fire_oracle import fire_relax
    from surface_sampling_amd import backend

    tab = _forms(fl)["alloy"]
    structs, mask = _relax_case()
    eng = backend.EAMEngine(tab, device=0)
    e, ea, f, pos, nst, conv = eng.relax_f64(structs, fixed=mask, max_steps=12, fmax=0.01, optimizer=optimizer)
    for b, (T, X, Cl, pbc) in enumerate(structs):
        def fn(p, T=T, Cl=Cl, pbc=pbc):
            E, _, F = ao.eam_typed(tab, T, p, Cl, pbc)
            return E, F

        relax = fire_relax if optimizer == "FIRE" else bfgs_relax
        pref, _, steps, _ = relax(fn, X, fixed=np.arange(4), max_steps=12, fmax=0.01)
        assert nst[b] == steps
        assert np.abs(pos[10 * b:10 * b + 10] - pref).max() < 1e-7, (b, np.abs(pos[10 * b:10 * b + 10] - pref).max())
        assert abs(e[b] - ao.eam_typed(tab, T, pref, Cl, pbc)[0]) < 1e-7
    eng.close()


def test_compaction_and_trajectory_records_change_nothing(fl, monkeypatch):
    from surface_sampling_amd import backend

    tab = _forms(fl)["funcfl"]
    structs, mask = _relax_case(8)
    eng = backend.EAMEngine(tab, device=0)
    runs = []
    for flag in ("0", "2"):
        monkeypatch.setenv("VSSR_RELAX_COMPACT", flag)
        runs.append(eng.relax_cg_f64(structs, fixed=mask, max_iter=60))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    assert runs[0][5].min() < runs[0][5].max()                       # the chains stop at different times
    eng.upload(structs)
    info = eng.relax_fire(fixed=mask, max_steps=12, fmax=0.01, want=backend.WANT_ENERGY | backend.WANT_FORCES, record_interval=4)
    tr = info["traj"]
    assert (tr["n_records"] >= 2).all()
    for b, (T, _, Cl, pbc) in enumerate(structs):
        for r in range(int(tr["n_records"][b])):
            E = ao.eam_typed(tab, T, tr["positions"][r, 10 * b:10 * b + 10], Cl, pbc)[0]
            assert abs(E - tr["energies"][r, b]) <= 1e-9 * abs(E)
    eng.close()


def test_semigrand_au_cu_mc_over_64_chains_through_lammps_surf_calc(fl, tmp_path):
    from surface_sampling_amd import eam, mc
    from surface_sampling_amd.calculators import LAMMPSSurfCalc
    from surface_sampling_amd.structures import Structure

    cu, au = fl
    path = str(tmp_path / "CuAu.eam.alloy")
    eam.write_setfl(ao.cuau_setfl(cu, au), path)
    rd = tmp_path / "run"
    rd.mkdir()
    (rd / "lammps_config.json").write_text(json.dumps({"potential_file": path, "atoms": ["Cu", "Au"], "bulk_index": 4}))
    for name in ("lammps_energy_template.txt", "lammps_opt_template.txt"):
        (rd / name).write_text("units metal\nboundary p p p\npair_style eam/alloy\npair_coeff * * {} {}\n")
    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    g = Structure(d["numbers"], d["positions"], d["cell"], d["pbc"])
    tab = eam.tables_from_setfl(eam.read_setfl(path), ["Cu", "Au"])
    for relax in (False, True):
        calc = LAMMPSSurfCalc(device="cuda:0")
        calc.set(run_dir=str(rd), relax_steps=20)
        ens = mc.ChainEnsemble(g, d["ads_coords"], ("Cu", "Au"), 64, calc, seed=11, relax=relax, relax_steps=20,
                               fixed_indices=np.arange(4), temperature=0.5, optimizer="LAMMPS")
        ens.initialize()
        for _ in range(5):
            ens.step_semigrand()
        nums = np.concatenate([ens.relaxed[b].numbers for b in range(64)])
        assert (nums == 79).any() and (nums == 29).sum() > 64 * len(g.numbers)   # both species were placed
        for b in range(64):
            r = ens.relaxed[b]
            T = np.where(np.asarray(r.numbers) == 79, 1, 0)
            E = ao.eam_typed(tab, T, r.positions, r.cell, [1, 1, 1])[0]
            assert abs(E - ens.state.energy[b]) <= 1e-9 * max(1.0, abs(E)), (relax, b, E, ens.state.energy[b])
