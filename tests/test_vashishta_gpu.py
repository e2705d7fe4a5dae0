"""Vashishta on the MI355X (vssr_vashishta_create, csrc/vashishta.hip) against the numpy restatement tests/vashishta_oracle.py: the
published SiC values through the device, parity on a three-species set with short rows on both sides of the 16-entry LDS row, on
sparse, ragged and empty rows, on transformed / partly periodic / self-image cells, batch independence, stress, FIRE / BFGS / CG
against their restatements, live-chain compaction and trajectory records, a semigrand MC through a run directory, refusals.

Parity bounds are those of tests/test_sw_gpu.py: E 1e-10 relative (floor 1 eV), pe/atom 1e-9 eV, F 1e-8 eV/A; the virial at the bound
of the analytic-stress tests, 1e-9 x max(1, |V sigma|) eV; the relaxations at the tolerances tests/test_adp_gpu.py applies to the same
drivers.  Every figure is printed before it is asserted.  No executed LAMMPS is compared."""
import numpy as np
import pytest

import cell_cases as cc
import strain_fd as sf
import sw_oracle as so
import vashishta_oracle as vo
from test_vashishta_cpu import _run_dir

pytestmark = pytest.mark.gpu

ONES = np.ones(3, np.uint8)


def _engine(params):
    from surface_sampling_amd import backend

    return backend.VashishtaEngine(params, device=0)


def _check(eng, P, structs, tag="", stress=()):
    """One batch on the device against the restatement of every structure; ``stress``: the chains whose virial is compared too."""
    e, ea, f = eng.evaluate_f64(structs)
    st = eng.stress()[0] if len(stress) else None
    o = 0
    for b, (T, X, Cl, pbc) in enumerate(structs):
        n = len(T)
        E, EA, F, W = vo.vashishta(P, T, X, Cl, pbc, virial=True)
        de, dea, df = abs(e[b] - E), np.abs(ea[o:o + n] - EA).max(), np.abs(f[o:o + n] - F).max()
        print(f"{tag} chain {b} ({n} atoms): E {E:+.12e}  |dE| {de:.2e}  max|d pe/atom| {dea:.2e}  max|dF| {df:.2e}  max|F| {np.abs(F).max():.3e}")
        assert de <= 1e-10 * max(1.0, abs(E)), (tag, b, e[b], E)
        assert dea <= 1e-9, (tag, b, dea)
        assert df <= 1e-8, (tag, b, df)
        if b in stress:
            dev = st[b] * abs(np.linalg.det(Cl))
            print(f"{tag} chain {b} virial: device {dev}  restatement {W}  max|d| {np.abs(dev - W).max():.2e}")
            assert np.abs(dev - W).max() <= 1e-9 * max(1.0, np.abs(W).max()), (tag, b, dev, W)
        o += n
    return e, ea, f


def _short_counts(P, T, X, Cl, pbc):
    i, _, _, _ = cc.brute_neighbors(X, Cl, pbc, vo.r0max(P))
    return np.bincount(i, minlength=len(X))


def _lone():
    return np.array([1], np.int32), np.array([[1.0, 2.0, 3.0]]), np.diag([19.0, 20.0, 21.0]), np.array([1, 1, 0], np.uint8)


# ---- SiC known answers through the device ---------------------------------------------------------------------------------------------
def test_device_reproduces_the_published_sic_values():
    """E/atom of the restatement (and with it the 6.3410 eV cohesive energy at a = 4.3581 A) at the five lattice constants and in a
    2 x 2 x 2 block, zero forces, C11 / C12 from device stresses at +-1e-3 xx strain."""
    _, P = vo.sic_params()
    grid = (4.30, 4.34, 4.3581, 4.38, 4.42)
    structs = [vo.zincblende(a) + (ONES,) for a in grid] + [vo.zincblende(vo.SIC_A0, reps=2) + (ONES,)]
    eng = _engine(P)
    e, ea, f = eng.evaluate_f64(structs)
    for b, (T, X, Cl, pbc) in enumerate(structs):
        E = vo.energy(P, T, X, Cl, pbc)
        print(f"a {Cl[0, 0]:.4f}: device {e[b] / len(T):+.12f}  restatement {E / len(T):+.12f} eV/atom")
        assert abs(e[b] - E) / len(T) <= 1e-9
    assert int(np.argmin(e[:5])) == 2 and abs(e[2] / 8 + 6.3410) <= 2e-3
    assert np.abs(f).max() < 1e-9
    ref = vo.elastic(lambda t, x, c: vo.vashishta(P, t, x, c, ONES, virial=True)[3])

    def device_virial(t, x, c):
        eng.evaluate_f64([(t, x, c, ONES)])
        return eng.stress()[0][0] * abs(np.linalg.det(c))

    C11, C12 = vo.elastic(device_virial)
    print(f"device C11 {C11:.4f}  C12 {C12:.4f} GPa; restatement {ref[0]:.4f} {ref[1]:.4f}; published 390.0 142.6")
    assert abs(C11 - ref[0]) <= 1e-6 * ref[0] and abs(C12 - ref[1]) <= 1e-6 * ref[1]
    assert abs(C11 - 390.0) <= 0.4 and abs(C12 - 142.6) <= 0.2
    eng.close()


# ---- parity on the three-species set ------------------------------------------------------------------------------------------------
def test_parity_on_three_species_short_rows_on_both_sides_of_the_tile():
    """Two dense 80-atom boxes whose short rows (r < r0max = 3.8 A) hold up to 22 slots: centres of both forms of the site kernel in
    one launch; a sparse box with centres that have no and one short neighbor; a 65-atom chain in front, so that the edges of the
    64-centre tiles fall inside chains; a lone atom with an empty row.  The text and the array construction give the same bits."""
    from surface_sampling_amd import backend

    sp, P, text = vo.three_species()
    dense = [so.dense_box(nt=3, seed=s) for s in (3, 4)]
    for s in dense:
        c = _short_counts(P, *s)
        assert (c > 16).any() and (c <= 16).any(), c
    sparse = so.dense_box(n=30, box=14.0, min_dist=2.1, seed=9, nt=3)
    c = _short_counts(P, *sparse)
    assert (c == 0).any() and (c == 1).any(), c
    odd = so.dense_box(n=65, box=9.8, min_dist=1.75, seed=6, nt=3)
    structs = [odd] + dense + [_lone(), sparse]
    a = _engine(P)
    b = backend.VashishtaEngine(text, device=0, species=sp)
    ra = _check(a, P, structs, "three-species", stress=(0, 1, 4))
    rb = b.evaluate_f64(structs)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    o = 65 + 160
    assert ra[0][3] == 0.0 and ra[1][o] == 0.0 and not ra[2][o].any()          # the lone atom
    a.close(); b.close()


def test_parity_with_a_centre_that_has_no_three_body_term():
    """r0 = 0 on every entry of centre 0: its short row is filled (r0max comes from centre 1) and contributes nothing."""
    _, P = vo.two_species_r0_zero()
    structs = [so.dense_box(n=40, box=8.2, min_dist=1.9, seed=6, nt=2), so.dense_box(n=20, box=6.8, min_dist=1.9, seed=6, nt=2)]
    eng = _engine(P)
    _check(eng, P, structs, "r0 = 0", stress=(1,))
    eng.close()


# ---- cells -------------------------------------------------------------------------------------------------------------------------
def test_parity_on_transformed_partly_periodic_and_self_image_cells():
    """Zincblende SiC in its 2-atom primitive cell (nimg >= 2 at the 7.35 A cutoff), periodic in 3, 2 and 1 directions, under every
    transform of tests/cell_cases.py; a one-atom simple-cubic cell with a 3.0 A edge (below r0max of the three-species set: an atom
    is its own short neighbor)."""
    _, P = vo.sic_params()
    a0 = vo.SIC_A0
    base = cc.Case("sic_primitive", "si", [6, 14], np.array([[0.0, 0.0, 0.0], [a0 / 4, a0 / 4, a0 / 4]]), cc.fcc_primitive(a0), [1, 1, 1],
                   None, None, types=np.array([0, 1], np.int32))
    rng = np.random.default_rng(4)
    cases = []
    for pbc in ([1, 1, 1], [1, 1, 0], [1, 0, 0]):
        c = base.with_(base.name + "".join(map(str, pbc)), pos=base.pos + rng.normal(0, 0.05, base.pos.shape), pbc=pbc)
        cases += [c] + cc.variants(c)
    assert any(v.pbc.sum() < 3 for v in cases)
    assert any(max(cc.face_nimg(c.cell, c.pbc, vo.cutoff(P))) >= 2 for c in cases)
    eng = _engine(P)
    _check(eng, P, [c.typed() for c in cases], "SiC cells")
    eng.close()
    _, P3, _ = vo.three_species()
    sc = cc.Case("sc_3.0", "si", [14], np.zeros((1, 3)), np.eye(3) * 3.0, [1, 1, 1], None, None, types=np.array([1], np.int32))
    sc2 = sc.with_("sc_3.0_open", pos=np.array([[0.1, 0.2, 0.3]]), pbc=[1, 1, 0])
    T, X, Cl, pbc = sc.typed()
    i, j, _, _ = cc.brute_neighbors(X, Cl, pbc, vo.r0max(P3))
    assert len(i) == 6 and (i == j).all()                                       # self images inside the short row
    eng = _engine(P3)
    _check(eng, P3, [c.typed() for c in (sc, sc2, cc.skew_basis(sc))], "self images", stress=(0, 2))
    eng.close()


# ---- batch independence -------------------------------------------------------------------------------------------------------------
def test_a_chain_is_bit_identical_alone_and_in_a_ragged_batch():
    sp, P, _ = vo.three_species()
    chain = so.dense_box(n=65, box=9.8, min_dist=1.75, seed=6, nt=3)
    others = [so.dense_box(n=30, box=14.0, min_dist=2.1, seed=9, nt=3), so.dense_box(nt=3, seed=7)]
    eng = _engine(P)
    e1, ea1, f1 = eng.evaluate_f64([chain])
    s1 = eng.stress()[0]
    e2, ea2, f2 = eng.evaluate_f64([others[0], chain, others[1]])
    s2 = eng.stress()[0]
    o, n = len(others[0][0]), len(chain[0])
    assert e2[1] == e1[0] and np.array_equal(ea2[o:o + n], ea1) and np.array_equal(f2[o:o + n], f1) and np.array_equal(s2[1], s1[0])
    eng.close()


# ---- stress -------------------------------------------------------------------------------------------------------------------------
def test_stress_rotation_covariance_repeatability_and_state_rules():
    from surface_sampling_amd import backend

    _, P = vo.sic_params()
    T, X, Cl, pbc = vo.rattled_sic(seed=3, sigma=0.1, reps=(2, 1, 1))
    R = cc.rotation(7)
    eng = _engine(P)
    eng.upload([(T, X, Cl, pbc)])
    with pytest.raises(backend.BackendError, match=r"vssr error -5"):           # VSSR_E_STATE before any run
        eng.stress()
    eng.run(backend.WANT_ENERGY)
    with pytest.raises(backend.BackendError, match="energies only"):
        eng.stress()
    _check(eng, P, [(T, X, Cl, pbc), (T, X @ R.T, Cl @ R.T, pbc)], "rattled SiC", stress=(0, 1))
    st = eng.stress()[0]
    assert np.array_equal(st, eng.stress()[0])
    vol = abs(np.linalg.det(Cl))
    diff = np.abs(st[1] - sf.rotated_voigt(st[0], R)).max() * vol
    print(f"|R sigma R^T - sigma(rotated)| = {diff:.3e} eV on a virial of {np.abs(st[0]).max() * vol:.3e} eV")
    assert np.abs(st[0]).max() * vol > 1.0 and diff <= 1e-9 * max(1.0, np.abs(st[0]).max() * vol)
    # against the strain derivative of the restated energy as well (ten times the checker's own uncertainty)
    chk = sf.fd_stress(lambda x, c: vo.energy(P, T, x, c, pbc), X, Cl)
    print(f"virial: device {st[0] * vol}  checker {chk.virial}  unc {chk.unc}")
    assert (np.abs(st[0] * vol - chk.virial) <= 10.0 * chk.unc).all()
    # an evaluation after a stress call is not disturbed by the gradients the stress call left in the scratch
    again = eng.evaluate_f64([(T, X, Cl, pbc)])
    fresh = _engine(P)
    for x, y in zip(again, fresh.evaluate_f64([(T, X, Cl, pbc)])):
        assert np.array_equal(x, y)
    eng.close(); fresh.close()


# ---- relaxation ---------------------------------------------------------------------------------------------------------------------
def _relax_case():
    """24 atoms of rattled zincblende SiC (3 x 1 x 1 cells), the first 12 held."""
    T, X, Cl, pbc = vo.rattled_sic(seed=2, sigma=0.08, reps=(3, 1, 1), n_fixed=12)
    mask = np.zeros(len(T), np.uint8)
    mask[:12] = 1
    return (T, X, Cl, pbc), mask


def _fn(P, T, Cl, pbc):
    def fn(p):
        E, _, F = vo.vashishta(P, T, p, Cl, pbc)
        return E, F
    return fn


def test_cg_follows_the_restatement_and_the_resident_request_runs_in_lock_step():
    from cg_oracle import cg_minimize

    _, P = vo.sic_params()
    (T, X, Cl, pbc), mask = _relax_case()
    assert len(T) == 24 and mask.sum() == 12
    eng = _engine(P)
    res = eng.relax_cg_f64([(T, X, Cl, pbc)], fixed=mask, max_iter=10)
    e, ea, f, pos, it, ev, why = res
    assert eng.last_cg_driver == "lockstep"
    pref, eref, niter, neval, reason, _ = cg_minimize(_fn(P, T, Cl, pbc), X, fixed=np.flatnonzero(mask), max_iter=10)
    print(f"CG: device {it[0]} iterations {ev[0]} evaluations stop {why[0]}; restatement {niter} {neval} {reason}; "
          f"|dE| {abs(e[0] - eref):.2e}  max|dx| {np.abs(pos - pref).max():.2e}")
    assert (it[0], ev[0], why[0]) == (niter, neval, reason)
    assert abs(e[0] - eref) < 1e-9 and np.abs(pos - pref).max() < 1e-9
    assert eref < vo.energy(P, T, X, Cl, pbc) - 0.1
    assert np.array_equal(pos[:12], X[:12])                            # the held half stayed
    again = eng.relax_cg_f64([(T, X, Cl, pbc)], fixed=mask, max_iter=10, driver="resident")
    assert eng.last_cg_driver == "lockstep"                            # no chain-resident minimiser for a Vashishta handle
    for x, y in zip(res, again):
        assert np.array_equal(x, y)
    eng.close()


@pytest.mark.parametrize("optimizer", ["FIRE", "BFGS"])
def test_fire_and_bfgs_follow_the_restatements(optimizer):
    from bfgs_oracle import bfgs_relax
    from fire_oracle import fire_relax

    _, P = vo.sic_params()
    (T, X, Cl, pbc), mask = _relax_case()
    eng = _engine(P)
    e, ea, f, pos, nst, conv = eng.relax_f64([(T, X, Cl, pbc)], fixed=mask, max_steps=10, fmax=0.01, optimizer=optimizer)
    relax = fire_relax if optimizer == "FIRE" else bfgs_relax
    pref, _, steps, _ = relax(_fn(P, T, Cl, pbc), X, fixed=np.flatnonzero(mask), max_steps=10, fmax=0.01)
    eref = vo.energy(P, T, pref, Cl, pbc)
    print(f"{optimizer}: device {nst[0]} steps, restatement {steps}; max|dx| {np.abs(pos - pref).max():.2e}  |dE| {abs(e[0] - eref):.2e}")
    assert nst[0] == steps
    assert np.abs(pos - pref).max() < 1e-7
    assert abs(e[0] - eref) < 1e-7
    assert np.abs(pos - X).max() > 1e-3 and np.array_equal(pos[:12], X[:12])
    eng.close()


def test_compaction_and_trajectory_records_change_nothing(monkeypatch):
    """Four copies of the 24-atom cell with different rattles stop at different times: with VSSR_RELAX_COMPACT=2 the resident batch
    is compacted while the CG runs, with the same bits; the energies FIRE records on the way are the restatement's; the fp64
    results of the batch are those of a plain evaluation."""
    from surface_sampling_amd import backend

    _, P = vo.sic_params()
    (T, X, Cl, pbc), mask = _relax_case()
    X0 = vo.zincblende(vo.SIC_A0)
    ideal = np.concatenate([X0[1] + np.array([k, 0, 0]) * vo.SIC_A0 for k in range(3)])
    structs = [(T, ideal + (X - ideal) * s, Cl, pbc) for s in (1.0, 0.25, 0.6, 0.02)]
    masks = np.tile(mask, len(structs))
    eng = _engine(P)
    runs = []
    for flag in ("0", "2"):
        monkeypatch.setenv("VSSR_RELAX_COMPACT", flag)
        runs.append(eng.relax_cg_f64(structs, fixed=masks, max_iter=40))
        assert eng.last_cg_driver == "lockstep"
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    print("CG evaluations per chain:", runs[0][5])
    assert runs[0][5].min() < runs[0][5].max()                       # the chains stop at different times
    e, ea, f = eng.evaluate_f64(structs)
    r = eng.results_f64()
    assert np.array_equal(r[0], e) and np.array_equal(r[1], ea) and np.array_equal(r[2], f)
    eng.upload(structs)
    info = eng.relax_fire(fixed=masks, max_steps=12, fmax=0.01, want=backend.WANT_ENERGY | backend.WANT_FORCES, record_interval=4)
    tr = info["traj"]
    assert (tr["n_records"] >= 2).all()
    for b in range(len(structs)):
        for k in range(int(tr["n_records"][b])):
            E = vo.energy(P, T, tr["positions"][k, 24 * b:24 * b + 24], Cl, pbc)
            assert abs(E - tr["energies"][k, b]) <= 1e-10 * max(1.0, abs(E)), (b, k, E, tr["energies"][k, b])
    eng.close()


def test_bfgs_linesearch_runs_through_the_table():
    """The device BFGSLineSearch has no kind-specific branch either: it lowers the energy of the rattled cell and holds the mask."""
    _, P = vo.sic_params()
    (T, X, Cl, pbc), mask = _relax_case()
    eng = _engine(P)
    eng.upload([(T, X, Cl, pbc)])
    info = eng.relax_bfgs_linesearch(fixed=mask, max_steps=6, fmax=0.01)
    pos = info["positions"]
    E0, E1 = vo.energy(P, T, X, Cl, pbc), vo.energy(P, T, pos, Cl, pbc)
    print(f"BFGSLineSearch: {info['n_steps']} steps, E {E0:.6f} -> {E1:.6f}")
    assert E1 < E0 - 0.1 and np.array_equal(pos[:12], X[:12])
    assert abs(eng.results_f64()[0][0] - E1) <= 1e-10 * abs(E1)
    eng.close()


# ---- semigrand MC through a run directory ----------------------------------------------------------------------------------------------
def test_semigrand_mc_of_8_chains_through_a_run_directory(tmp_path):
    """A SiC(001) slab (64 atoms, periodic in x and y by the template's ``boundary p p f``) with the C sites of the next layer:
    single points and CG-relaxed.  State energies are the restatement's, and a run is reproducible from its seed."""
    from surface_sampling_amd import mc, vashishta as va
    from surface_sampling_amd.calculators import LAMMPSSurfCalc
    from surface_sampling_amd.structures import Structure

    _, P = vo.sic_params()
    Z, X, Cl, pbc, sites = vo.sic001_slab()
    g = Structure(Z, X, Cl, pbc)
    rd = _run_dir(tmp_path / "sic", va.builtin_text(vo.SIC))
    for relax in (False, True):
        runs = []
        for _ in range(2):
            calc = LAMMPSSurfCalc(device="cuda:0")
            calc.set(run_dir=rd, relax_steps=10)
            ens = mc.ChainEnsemble(g, sites, ("C",), 8, calc, seed=5, relax=relax, relax_steps=10, temperature=0.5, optimizer="LAMMPS")
            ens.initialize()
            for _ in range(4):
                ens.step_semigrand()
            assert (ens.num_adsorbates() > 0).any()
            for b in range(8):
                r = ens.relaxed[b]
                T = np.where(np.asarray(r.numbers) == 6, 0, 1)
                E = vo.energy(P, T, r.positions, r.cell, [1, 1, 0])
                print(f"relax {relax} chain {b}: {len(T)} atoms  E {E:+.10f}  device {ens.state.energy[b]:+.10f}")
                assert abs(E - ens.state.energy[b]) <= 1e-10 * max(1.0, abs(E)), (relax, b)
                assert np.array_equal(r.positions[:16], X[:16])                 # the template's bulk group (bulk_index 16) stayed
            runs.append((ens.state.species.copy(), ens.state.energy.copy()))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_vashishta_surf_calc_serves_the_sw_property_set():
    from surface_sampling_amd.calculators import VashishtaSurfCalc
    from surface_sampling_amd.structures import Structure

    _, P = vo.sic_params()
    Z, X, Cl, pbc, _ = vo.sic001_slab()
    X = X + np.random.default_rng(12).normal(0, 0.05, X.shape)
    T = np.where(Z == 6, 0, 1)
    calc = VashishtaSurfCalc(vo.SIC, device="cuda:0")
    calc.calculate(Structure(Z, X, Cl, pbc.astype(bool)), properties=("energy", "forces", "stress", "per_atom_energies"))
    E, EA, F, W = vo.vashishta(P, T, X, Cl, pbc, virial=True)
    r = calc.results
    vol = abs(np.linalg.det(Cl))
    print(f"calculator: |dE| {abs(r['energy'] - E):.2e}  max|dF| {np.abs(r['forces'] - F).max():.2e}  "
          f"max|d virial| {np.abs(np.asarray(r['stress']) * vol - W).max():.2e}")
    assert abs(r["energy"] - E) <= 1e-10 * abs(E) and np.abs(r["forces"] - F).max() <= 1e-8
    assert np.abs(r["per_atom_energies"] - EA).max() <= 1e-9
    assert np.abs(np.asarray(r["stress"]) * vol - W).max() <= 1e-9 * max(1.0, np.abs(W).max())


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_tables_and_types_are_refused_and_the_handle_goes_on():
    from surface_sampling_amd import backend

    sp, P, text = vo.three_species()
    eng = _engine(P)
    batch = [so.dense_box(n=30, box=14.0, min_dist=2.1, seed=9, nt=3), _lone()]
    first = eng.evaluate_f64(batch)
    for entry, field, value in (((0, 1, 1), 8, 0.0), ((1, 1, 1), 0, np.nan), ((0, 1, 1), 11, 6.5), ((2, 0, 0), 7, 1.0), ((1, 0, 2), 13, 0.5)):
        Q = P.copy()
        Q[entry + (field,)] = value
        with pytest.raises(backend.BackendError, match=r"vssr_vashishta_create failed \(-1\)"):
            backend.VashishtaEngine(Q, device=0)
    with pytest.raises(backend.BackendError, match=r"vssr_vashishta_create_from_text failed \(-1\).*lacks the entry"):
        backend.VashishtaEngine(text, device=0, species=["Si", "O", "Ga"])
    with pytest.raises(backend.BackendError, match=r"failed \(-1\)"):
        backend.VashishtaEngine(np.zeros((9, 9, 9, 14)), device=0)
    T, X, Cl, pbc = batch[0]
    for bad in (3, -1):
        t = T.copy()
        t[5] = bad
        with pytest.raises(backend.BackendError, match="vssr error -1"):
            eng.evaluate_f64([(t, X, Cl, pbc)])
    for x, y in zip(first, eng.evaluate_f64(batch)):                   # the handle serves the next batch with identical bits
        assert np.array_equal(x, y)
    eng.close()
