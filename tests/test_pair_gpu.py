"""Pair potentials with damped-shifted Coulomb on the MI355X (vssr_pair_*, PairSurfCalc, LAMMPSSurfCalc) against the numpy
restatement tests/pair_oracle.py: dimers of every style, the rocksalt cube whose 12 A cutoff spans several images, a skewed
three-type slab under pair_style hybrid, batch independence, the lock-step relaxations, the batched MC and the refusals.

Tolerances are those tests/test_sw_gpu.py applies to the same fp64 quantities: E 1e-10 relative (floor 1 eV), pe/atom 1e-9 eV,
F 1e-8 eV/A; stress: ten times the uncertainty of the strain derivative of the restatement (tests/strain_fd.py), as
tests/test_gpu_analytic_stress.py.  Every figure is printed before it is asserted.  No executed LAMMPS is compared."""
import json

import numpy as np
import pytest

import pair_oracle as po
from pair_cases import OVERLAY5, grid_chain as _grid_chain
import strain_fd as sf

pytestmark = pytest.mark.gpu

E_REL, EA_ABS, F_ABS, STRESS_FACTOR = 1e-10, 1e-9, 1e-8, 10.0
NACL = ["Na", "Cl"]


def _model(lines, n_types):
    from surface_sampling_amd import pair

    return pair.parse(lines, n_types)


def _engine(model):
    from surface_sampling_amd import backend

    return backend.PairEngine(model, device=0)


def _check(eng, model, structs, tag, stress=False):
    terms, q = po.model_of(model)
    e, ea, f = eng.evaluate_f64(structs)
    st = eng.stress()[0] if stress else None
    o = 0
    for b, (T, X, Cl, pbc) in enumerate(structs):
        n = len(T)
        E, EA, F = po.pair(terms, q, T, X, Cl, pbc)
        de, dea, df = abs(e[b] - E), np.abs(ea[o:o + n] - EA).max(), np.abs(f[o:o + n] - F).max()
        print(f"{tag} chain {b} ({n} atoms): E {E:+.12e}  |dE| {de:.2e}  max|d pe/atom| {dea:.2e}  max|dF| {df:.2e}  max|F| {np.abs(F).max():.3e}")
        assert de <= E_REL * max(1.0, abs(E)), (tag, b, e[b], E)
        assert dea <= EA_ABS, (tag, b, dea)
        assert df <= F_ABS, (tag, b, df)
        if stress:
            chk = sf.fd_stress(lambda x, c: po.pair(terms, q, T, x, c, pbc)[0], X, Cl)
            dev = st[b] * chk.volume
            ratio = np.abs(dev - chk.virial) / chk.unc
            print(f"{tag} chain {b} virial: device {dev}  checker {chk.virial}  unc {chk.unc}  max ratio {ratio.max():.3f}")
            assert (np.abs(dev - chk.virial) <= STRESS_FACTOR * chk.unc).all(), (tag, b, dev, chk.virial, chk.unc)
        o += n
    return e, ea, f


HYBRID = ["pair_style hybrid lj/cut 6.0 morse 5.0 buck 7.0",
          "pair_coeff 1 1 lj/cut 0.02 2.6", "pair_coeff 2 2 lj/cut 0.03 2.5 5.5", "pair_coeff 1 2 morse 0.2 1.4 2.6",
          "pair_coeff 1 3 buck 900.0 0.29 25.0", "pair_coeff 3 3 morse 0.15 1.2 2.9", "pair_coeff 2 3 none"]


# 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lines, q", [
    (["pair_style lj/cut 8.0", "pair_coeff 1 1 0.0104 3.4", "pair_coeff 2 2 0.02 3.0", "pair_coeff 1 2 0.015 3.1 7.0"], None),
    (["pair_style morse 7.0", "pair_coeff 1 1 0.3 1.5 2.4", "pair_coeff 2 2 0.2 1.1 2.9", "pair_coeff 1 2 0.35 1.6 2.3"], None),
    (["pair_style buck 8.0", "pair_coeff 1 1 800 0.31 12", "pair_coeff 2 2 1200 0.27 40", "pair_coeff 1 2 1000.0 0.3 30.0"], None),
    (["pair_style born 8.0", "pair_coeff 1 1 0.3 0.31 2.3 1.0 -0.5", "pair_coeff 2 2 0.2 0.3 3.1 70 -140", "pair_coeff 1 2 0.5 0.3 2.8 30.0 50.0"], None),
    (["pair_style coul/dsf 0.2 12.0", "pair_coeff * *", "set type 1 charge 1.0", "set type 2 charge -0.7"], (1.0, -0.7)),
], ids=["lj_cut", "morse", "buck", "born", "coul_dsf"])
def test_dimer_of_every_style(lines, q):
    """Two atoms of types 1 and 2 in a 20 A open box at three separations (and the like pairs once each): a coefficient read in the
    wrong order, or the wrong pair's entry, shows here."""
    m = _model(lines, 2)
    box, open_ = np.eye(3) * 20.0, np.zeros(3, np.uint8)
    d = np.array([0.6, 0.5, 0.4]); d /= np.linalg.norm(d)
    structs = [(np.array(t, np.int32), np.array([[5.0, 6.0, 7.0], [5.0, 6.0, 7.0] + r * d]), box, open_)
               for t, r in (((0, 1), 2.2), ((0, 1), 3.1), ((1, 0), 5.9), ((0, 0), 2.9), ((1, 1), 3.3))]
    eng = _engine(m)
    _check(eng, m, structs, "dimer " + lines[0])
    eng.close()


# 2 --------------------------------------------------------------------------------------------------------------------------------
def test_rocksalt_cube_with_a_cutoff_of_several_images():
    """8-atom rocksalt cube, pbc TTT, born 8.0 + coul/dsf 0.2 12.0: the cutoff is more than twice the cell, so every atom sees itself
    and its neighbors through several images, in rows of several hundred slots.  The perfect crystal (forces vanish, pe/atom carries
    the self term) and a rattled copy (no pair within 0.02 A of the unshifted Born cutoff, so the strain derivative of the checker
    crosses no discontinuity)."""
    import cell_cases as cc

    m = _model(po.ROCKSALT_COMMANDS, 2)
    T, X, C = po.rocksalt(5.64)
    pbc = np.ones(3, np.uint8)
    Xr = X + np.random.default_rng(21).normal(0, 0.05, X.shape)
    i, _, _, rv = cc.brute_neighbors(Xr, C, pbc, 12.0)
    d = np.linalg.norm(rv, axis=1)
    assert np.abs(d - 8.0).min() > 0.02
    rows = np.bincount(i, minlength=8)
    assert rows.min() > 300 and max(cc.face_nimg(C, pbc, 12.0)) >= 3
    eng = _engine(m)
    e, ea, f = _check(eng, m, [(T, X, C, pbc), (T, Xr, C, pbc)], "rocksalt", stress=True)
    assert np.abs(f[:8]).max() < 1e-10
    stats = eng.stats()
    print("rocksalt batch:", stats)
    eng.close()


# 3 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", ["no", "yes"])
def test_skewed_three_type_slab_under_hybrid(shift):
    """40 atoms of three types on a jittered grid, skewed cell, pbc TTF; lj/cut, morse and buck each on their own type pairs, the pair
    2 3 switched off (none).  With and without pair_modify shift yes."""
    m = _model(HYBRID + [f"pair_modify shift {shift}"], 3)
    assert sorted({t.style for t in m.terms}) == [1, 2, 3] and all(t.shift == (shift == "yes") for t in m.terms)
    import cell_cases as cc

    s = _grid_chain(40, 38, [1, 1, 0])
    # the checker strains the cell by up to 4e-4: no pair may cross its term's cutoff on the way (the unshifted energy jumps there)
    i, j, _, rv = cc.brute_neighbors(s[1], s[2], s[3], 7.5)
    d, ti, tj = np.linalg.norm(rv, axis=1), s[0][i], s[0][j]
    for t in m.terms:
        on = ((ti == t.type_a) & (tj == t.type_b)) | ((ti == t.type_b) & (tj == t.type_a))
        assert np.abs(d[on] - t.rc).min() > 0.005
    eng = _engine(m)
    _check(eng, m, [s], f"hybrid slab shift {shift}", stress=True)
    eng.close()


# 4 --------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_is_bit_identical_chain_by_chain_and_run_to_run():
    m = _model(OVERLAY5, 3)
    chains = [_grid_chain(n, 40 + k, pbc) for k, (n, pbc) in enumerate(((7, [1, 1, 1]), (16, [1, 1, 0]), (23, [1, 0, 0]), (40, [1, 1, 1]),
                                                                         (40, [0, 0, 0])))]
    eng = _engine(m)
    e1, ea1, f1 = _check(eng, m, chains, "ragged")
    e2, ea2, f2 = eng.evaluate_f64(chains)
    assert np.array_equal(e1, e2) and np.array_equal(ea1, ea2) and np.array_equal(f1, f2)
    o = 0
    for b, c in enumerate(chains):
        n = len(c[0])
        e, ea, f = eng.evaluate_f64([c])
        assert e[0] == e1[b] and np.array_equal(ea, ea1[o:o + n]) and np.array_equal(f, f1[o:o + n]), b
        o += n
    eng.close()


# 5 --------------------------------------------------------------------------------------------------------------------------------
LJ_AR = ["pair_style lj/cut 6.0", "pair_coeff 1 1 0.0104 3.4"]


def _fcc_rattled():
    a = 2.0 ** (1 / 6) * 3.4 * np.sqrt(2.0)             # nearest neighbors at the pair minimum
    basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    shifts = np.array([[x, y, z] for x in range(2) for y in range(2) for z in range(2)], float)
    X = (basis[None] + shifts[:, None]).reshape(-1, 3) * a
    rng = np.random.default_rng(5)
    fixed = np.zeros(32, np.uint8)
    fixed[:8] = 1
    X = X + np.where(fixed[:, None] == 1, 0.0, rng.uniform(-0.1, 0.1, X.shape) * a / np.sqrt(2.0))   # 10 % of the bond length
    return np.zeros(32, np.int32), X, np.eye(3) * 2 * a, np.ones(3, np.uint8), fixed


@pytest.mark.parametrize("optimizer", ["CG", "FIRE"])
def test_lockstep_relaxations_of_a_rattled_lj_crystal(optimizer):
    """32-atom fcc cell, free atoms displaced by up to 10 % of the bond length, 8 atoms held.  The relaxed energy is below the
    starting energy (FIRE's potential energy is not monotone step by step by construction, so start against end is what holds for
    both drivers), the largest force on a free atom is below the requested tolerance, held atoms have not moved, and the stored
    energy is the restatement's at the relaxed positions.  CG: ftol bounds the 2-norm of the force vector, hence the largest
    component."""
    tol = 1e-3
    m = _model(LJ_AR, 1)
    T, X, C, pbc, fixed = _fcc_rattled()
    eng = _engine(m)
    e0, _, f0 = eng.evaluate_f64([(T, X, C, pbc)])
    assert np.abs(f0[fixed == 0]).max() > 20 * tol
    if optimizer == "CG":
        e, ea, f, pos, it, ev, why = eng.relax_cg_f64([(T, X, C, pbc)], fixed=fixed, max_iter=500, etol=0.0, ftol=tol)
        print(f"CG: {it[0]} iterations, {ev[0]} evaluations, stop {why[0]}; lock-step evaluations {eng.last_relax_counts}")
        assert eng.last_relax_counts[0] > 1                          # the lock-step driver ran (never the chain-resident one)
    else:
        e, ea, f, pos, steps, conv = eng.relax_f64([(T, X, C, pbc)], fixed=fixed, max_steps=800, fmax=tol, optimizer="FIRE")
        print(f"FIRE: {steps[0]} steps, converged {conv[0]}")
        assert conv[0]
    fmax = np.linalg.norm(f[fixed == 0], axis=1).max()
    print(f"{optimizer}: E {e0[0]:.9f} -> {e[0]:.9f} eV, fmax(free) {fmax:.3e}")
    assert e[0] < e0[0] and fmax <= tol
    assert np.array_equal(pos[fixed == 1], X[fixed == 1])
    E, _, _ = po.pair(*po.model_of(m), T, pos, C, pbc)
    assert abs(E - e[0]) <= E_REL * max(1.0, abs(E))
    eng.close()


def _run_dir(path, body, atoms, bulk_index=0, boundary="p p p"):
    path.mkdir()
    (path / "lammps_config.json").write_text(json.dumps({"atoms": list(atoms), "bulk_index": bulk_index}))
    head = f"units metal\nboundary {boundary}\nread_data {{}}\ngroup bulk id <= {{}}\n" + "\n".join(body) + "\n"
    (path / "lammps_energy_template.txt").write_text(head + "run 0\n")
    (path / "lammps_opt_template.txt").write_text(head + "fix 2 bulk setforce 0.0 0.0 0.0\nmin_style cg\nminimize 1e-5 1e-5 {} 10000\n")
    return path


def test_lammps_surf_calc_relaxes_from_a_run_directory(tmp_path):
    from surface_sampling_amd.calculators import LAMMPSSurfCalc
    from surface_sampling_amd.structures import Structure

    T, X, C, pbc, fixed = _fcc_rattled()
    slab = Structure(np.full(32, 18), X, C, pbc)
    calc = LAMMPSSurfCalc(device="cuda:0")
    calc.set(run_dir=_run_dir(tmp_path / "ar", LJ_AR, ["Ar"], bulk_index=8), relax_steps=500)
    _, e0, _ = calc.run_lammps_energy(slab)
    relaxed, e, ea = calc.run_lammps_opt(slab, etol=0.0, ftol=1e-3)                 # CG; the template's bulk group is held
    print(f"run_lammps_opt: E {e0:.9f} -> {e:.9f} eV, {calc.last_opt}")
    assert e < e0 and np.array_equal(relaxed.positions[:8], X[:8]) and not np.array_equal(relaxed.positions[8:], X[8:])
    f = calc.calculate_batch([relaxed])[0]["forces"]
    assert np.linalg.norm(f[8:], axis=1).max() <= 1e-3
    E, EA, _ = po.pair(*po.model_of(_model(LJ_AR, 1)), T, relaxed.positions, C, pbc)
    assert abs(E - e) <= E_REL * max(1.0, abs(E)) and np.abs(EA - ea).max() <= EA_ABS


def test_lammps_surf_calc_serves_overlay_born_dsf_from_a_run_directory(tmp_path):
    from surface_sampling_amd.calculators import LAMMPSSurfCalc
    from surface_sampling_amd.structures import Structure

    T, X, C = po.rocksalt(5.64)
    X = X + np.random.default_rng(22).normal(0, 0.05, X.shape)
    Cz = C.copy(); Cz[2, 2] = 25.0
    slab = Structure(np.where(T == 0, 11, 17), X, Cz, [1, 1, 1])                    # the template's boundary p p f decides
    calc = LAMMPSSurfCalc(device="cuda:0")
    calc.set(run_dir=_run_dir(tmp_path / "nacl", po.ROCKSALT_COMMANDS, NACL, boundary="p p f"))
    _, e, ea = calc.run_lammps_energy(slab)
    E, EA, F = po.pair(*po.model_of(_model(po.ROCKSALT_COMMANDS, 2)), T, X, Cz, [1, 1, 0])
    print(f"LAMMPSSurfCalc born + coul/dsf: E {e:.12f}  oracle {E:.12f}")
    assert abs(E - e) <= E_REL * max(1.0, abs(E)) and np.abs(EA - ea).max() <= EA_ABS
    calc.calculate(slab, properties=("energy", "forces", "stress"))
    assert np.abs(calc.results["forces"] - F).max() <= F_ABS and np.isfinite(calc.results["stress"]).all()


# 6 --------------------------------------------------------------------------------------------------------------------------------
def test_batched_mc_on_the_rocksalt_slab():
    """mc.ChainEnsemble with PairSurfCalc, 4 chains, 3 semigrand steps of Na / Cl adatoms over the 8-atom rocksalt slab (single
    points): the stored energies of the accepted states are the restatement's; two runs agree."""
    from surface_sampling_amd import mc
    from surface_sampling_amd.calculators import PairSurfCalc
    from surface_sampling_amd.structures import Structure

    T, X, C = po.rocksalt(5.64)
    Cz = C.copy(); Cz[2, 2] = 25.0
    base = Structure(np.where(T == 0, 11, 17), X, Cz, [1, 1, 0])
    sites = np.array([[(i + 0.5) * 2.82, (j + 0.5) * 2.82, X[:, 2].max() + 2.6] for i in range(2) for j in range(2)])
    model = _model(po.ROCKSALT_COMMANDS, 2)
    runs = []
    for _ in range(2):
        calc = PairSurfCalc(commands=po.ROCKSALT_COMMANDS, species=NACL, device="cuda:0")
        ens = mc.ChainEnsemble(base, sites, ("Na", "Cl"), 4, calc, seed=7, relax=False, temperature=1.0)
        ens.initialize()
        for _ in range(3):
            ens.step_semigrand()
        assert (ens.num_adsorbates() > 0).any()
        for b in range(4):
            r = ens.relaxed[b]
            E, _, _ = po.pair(*po.model_of(model), np.where(r.numbers == 11, 0, 1), r.positions, r.cell, [1, 1, 0])
            print(f"MC chain {b}: {len(r.numbers)} atoms, E {ens.state.energy[b]:.12f}  oracle {E:.12f}")
            assert abs(E - ens.state.energy[b]) <= 1e-9 * max(1.0, abs(E)), b
        runs.append((ens.state.species.copy(), ens.state.energy.copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


# 7 --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from surface_sampling_amd import backend

    m = _model(po.ROCKSALT_COMMANDS, 2)
    T, X, C = po.rocksalt(5.64)
    pbc = np.ones(3, np.uint8)
    eng = _engine(m)
    good = eng.evaluate_f64([(T, X, C, pbc)])
    thin = C.copy(); thin[2, 2] = 0.11                     # 12 A / 0.11 A: 110 images along z, the search scans 100 at the most
    with pytest.raises(backend.BackendError, match=r"vssr error -3: .*periodic images along axis 2"):
        eng.evaluate_f64([(T, X, thin, pbc)])
    again = eng.evaluate_f64([(T, X, C, pbc)])             # the handle serves the next batch
    assert all(np.array_equal(a, b) for a, b in zip(good, again))
    lj = (0, 0, "lj/cut", (0.01, 3.0), 6.0, 0)
    with pytest.raises(backend.BackendError, match=r"\(-1\): .*more than 3 terms on the type pair 0 0"):
        backend.PairEngine([lj, (0, 0, "morse", (0.1, 1.0, 2.0), 5.0, 0), (0, 0, "buck", (100.0, 0.3, 1.0), 5.0, 0),
                            (0, 0, "born", (1.0, 0.3, 2.0, 1.0, 1.0), 5.0, 0)], n_types=1, device=0)
    with pytest.raises(backend.BackendError, match=r"\(-1\): .*coul/dsf needs per-type charges"):
        backend.PairEngine([(0, 0, "coul/dsf", (0.2,), 9.0, 0)], charges=None, n_types=1, device=0)
    with pytest.raises(backend.BackendError, match=r"\(-1\): .*bad rho"):
        backend.PairEngine([(0, 0, "buck", (100.0, 0.0, 1.0), 5.0, 0)], n_types=1, device=0)
    with pytest.raises(backend.BackendError, match=r"\(-1\): .*bad cutoff"):
        backend.PairEngine([(0, 0, "lj/cut", (0.01, 3.0), float("nan"), 0)], n_types=1, device=0)
    last = eng.evaluate_f64([(T, X, C, pbc)])
    assert all(np.array_equal(a, b) for a, b in zip(good, last))
    eng.close()
