"""Ewald sums on the MI355X (vssr_pair_create_kspace, ewald.hip: pair_style */coul/long + kspace_style ewald) against the numpy
restatement tests/ewald_oracle.py: parity on a cube and a skewed charged cell, a ragged batch with every k-box shape the kernels
tile differently, batch independence, stress, the lock-step relaxations, the batched MC, a LAMMPS run directory and the refusals.

Tolerances are those of tests/test_pair_gpu.py for the same fp64 quantities: E 1e-10 relative (floor 1 eV), pe/atom 1e-9 eV,
F 1e-8 eV/A; stress: ten times the uncertainty of the strain derivative of the restatement (tests/strain_fd.py).  Every figure is
printed before it is asserted.  No executed LAMMPS is compared."""
import json

import numpy as np
import pytest

import ewald_cases as ec
import ewald_oracle as eo
import strain_fd as sf

pytestmark = pytest.mark.gpu

E_REL, EA_ABS, F_ABS, STRESS_FACTOR = 1e-10, 1e-9, 1e-8, 10.0
NACL = ["Na", "Cl"]


def _model(lines, n_types=3):
    from surface_sampling_amd import pair

    return pair.parse(lines, n_types)


def _engine(model):
    from surface_sampling_amd import backend

    return backend.PairEngine(model, device=0)


def _check(eng, model, structs, tag, stress=False):
    terms, q, ks = eo.model_of(model)
    e, ea, f = eng.evaluate_f64(structs)
    st = eng.stress()[0] if stress else None
    o = 0
    for b, (T, X, Cl, _) in enumerate(structs):
        n = len(T)
        E, EA, F = eo.ewald(terms, q, ks, T, X, Cl)
        de, dea, df = abs(e[b] - E), np.abs(ea[o:o + n] - EA).max(), np.abs(f[o:o + n] - F).max()
        print(f"{tag} chain {b} ({n} atoms): E {E:+.12e}  |dE| {de:.2e}  max|d pe/atom| {dea:.2e}  max|dF| {df:.2e}  max|F| {np.abs(F).max():.3e}")
        assert de <= E_REL * max(1.0, abs(E)), (tag, b, e[b], E)
        assert dea <= EA_ABS, (tag, b, dea)
        assert df <= F_ABS, (tag, b, df)
        if stress:
            # the strain derivative at the k set of the unstrained cell: the virial does not see vectors entering or leaving the sphere
            hkl = eo.k_indices(Cl, ks.k_cut)[0]
            chk = sf.fd_stress(lambda x, c: eo.ewald(terms, q, ks, T, x, c, hkl=hkl)[0], X, Cl)
            dev = st[b] * chk.volume
            ratio = np.abs(dev - chk.virial) / chk.unc
            print(f"{tag} chain {b} virial: device {dev}  checker {chk.virial}  unc {chk.unc}  max ratio {ratio.max():.3f}")
            assert (np.abs(dev - chk.virial) <= STRESS_FACTOR * chk.unc).all(), (tag, b, dev, chk.virial, chk.unc)
        o += n
    return e, ea, f


def _pair_margin(struct, rc):
    import cell_cases as cc

    _, _, _, rv = cc.brute_neighbors(struct[1], struct[2], struct[3], rc + 1.0)
    return np.abs(np.linalg.norm(rv, axis=1) - rc).min()


# 1 --------------------------------------------------------------------------------------------------------------------------------
def test_parity_on_the_rocksalt_cube_and_the_skewed_charged_cell():
    """Bare Coulomb at A = 1e-8, rc = 8: the perfect cube (forces vanish, the energy is the Madelung energy to the accuracy asked
    for), and the skewed cell with total charge +1 (the background term, reciprocal vectors of a triclinic cell)."""
    m = _model(ec.RAGGED_MODEL)
    eng = _engine(m)
    e, ea, f = _check(eng, m, [ec.cube(), ec.skewed()], "parity")
    M = -e[0] / 4 * 2.82 / eo.QQRD2E
    print(f"cube: Madelung {M:.12f}, relative error {abs(M / 1.7475645946 - 1):.2e} at A = 1e-8")
    assert abs(M / 1.7475645946 - 1) < 1e-8 and np.abs(f[:8]).max() < 1e-10
    eng.close()


# 2 --------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_against_the_restatement_and_bit_for_bit():
    """The five chains of ewald_cases.RAGGED in one batch (their k boxes are rehearsed in tests/test_ewald_cpu.py): against the
    restatement chain by chain, bit-identical run to run, and every chain bit-identical to its single-chain evaluation."""
    m = _model(ec.RAGGED_MODEL)
    chains = [make() for _, make, _, _ in ec.RAGGED]
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
    e3, ea3, f3 = eng.evaluate_f64(chains[::-1])                   # another order: other offsets into S(k), other neighbors in the batch
    assert np.array_equal(e3[::-1], e1)
    start = np.concatenate([[0], np.cumsum([len(c[0]) for c in chains])])
    o = 0
    for b in reversed(range(len(chains))):
        n = len(chains[b][0])
        assert np.array_equal(ea3[o:o + n], ea1[start[b]:start[b + 1]]) and np.array_equal(f3[o:o + n], f1[start[b]:start[b + 1]]), b
        o += n
    eng.close()


# 3 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, make, rc", [("neutral", ec.rattled_cube, 8.14), ("charged", ec.skewed, 8.42)])
def test_stress_is_the_strain_derivative(name, make, rc):
    """born/coul/long at A = 1e-12: the rattled cube and the skewed cell with total charge +1.  The cutoff is chosen so that no pair
    comes within 0.01 A of it (the checker strains by up to 4e-4 and the unshifted real-space terms jump there)."""
    s = make()
    assert _pair_margin(s, rc) > 0.01
    m = _model(ec.born(rc, 1e-12))
    eng = _engine(m)
    _check(eng, m, [s], f"stress {name}", stress=True)
    eng.close()


# 4 --------------------------------------------------------------------------------------------------------------------------------
RELAX_MODEL = ec.born(8.0, 1e-8)


@pytest.mark.parametrize("optimizer", ["FIRE", "BFGS", "CG"])
def test_relaxations_of_a_rattled_64_ion_cell(optimizer):
    """To fmax 1e-3: the energy the minimiser leaves on the device is that of a fresh single point of the returned positions, which
    is the restatement's; CG asked for the chain-resident driver runs in lock step, with the same bits."""
    from surface_sampling_amd import backend

    tol = 1e-3
    m = _model(RELAX_MODEL)
    c = T, X, C, pbc = ec.rattled64()
    eng = _engine(m)
    e0, _, f0 = eng.evaluate_f64([c])
    assert np.abs(f0).max() > 50 * tol
    if optimizer == "CG":
        e, ea, f, pos, it, ev, why = eng.relax_cg_f64([c], max_iter=500, etol=0.0, ftol=tol, rerun=False)
        print(f"CG: {it[0]} iterations, {ev[0]} evaluations, stop {why[0]}, driver {eng.last_cg_driver}, counts {eng.last_relax_counts}")
        assert eng.last_cg_driver == "lockstep"
        res = eng.relax_cg_f64([c], max_iter=500, etol=0.0, ftol=tol, rerun=False, driver="resident")
        assert eng.last_cg_driver == "lockstep"                   # no chain-resident minimiser for a handle with k-space
        for x, y in zip((e, ea, f, pos, it, ev, why), res):
            assert np.array_equal(x, y)
    else:
        eng.upload([c])
        info = eng.relax(optimizer, max_steps=600, fmax=tol, want=backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM)
        print(f"{optimizer}: {info['n_steps'][0]} steps, converged {info['converged'][0]}")
        assert info["converged"][0]
        pos = info["positions"]
        e, ea, f = eng.results_f64()
    fresh, _, ffresh = eng.evaluate_f64([(T, pos, C, pbc)])
    E, _, _ = eo.ewald(*eo.model_of(m), T, pos, C)
    fmax = np.linalg.norm(ffresh, axis=1).max()
    print(f"{optimizer}: E {e0[0]:.9f} -> {e[0]:.9f} eV  fresh {fresh[0]:.9f}  restatement {E:.9f}  fmax {fmax:.3e}")
    assert abs(e[0] - fresh[0]) <= 1e-9 * max(1.0, abs(fresh[0]))
    assert abs(E - fresh[0]) <= E_REL * max(1.0, abs(E))
    assert e[0] < e0[0] and fmax <= float(np.float32(tol))        # (the ABI carries fmax as a C float)
    eng.close()


def test_cg_with_live_chain_compaction(monkeypatch):
    """Two cubes that meet the force tolerance at the start, a strongly rattled cube and the rattled 64-ion cell: the chains stop
    at different polls (asserted), so with VSSR_RELAX_COMPACT=2 the resident batch is compacted while the relaxation runs (asserted:
    fewer chain evaluations than lock-step evaluations x chains).  Results equal those without compaction bit for bit, and the
    energies left on the device are those of fresh single points."""
    m = _model(RELAX_MODEL)
    T, X, C, pbc = ec.cube()
    chains = [(T, X + np.random.default_rng(50 + k).normal(0, s, X.shape), C, pbc) for k, s in enumerate((1e-5, 0.15, 2e-5))]
    chains.insert(1, ec.rattled64())
    eng = _engine(m)
    runs, counts = [], []
    for flag in ("0", "2"):
        monkeypatch.setenv("VSSR_RELAX_COMPACT", flag)
        runs.append(eng.relax_cg_f64(chains, max_iter=300, etol=0.0, ftol=1e-3, rerun=False))
        counts.append(eng.last_relax_counts)
    monkeypatch.delenv("VSSR_RELAX_COMPACT")
    ev = runs[0][5]
    print(f"compaction: evaluations per chain {ev.tolist()}, stop {runs[0][6].tolist()}, (lock-step, chain) evaluations {counts}")
    assert ev.min() < 8 and ev.max() > 16                         # the driver polls every 8 evaluations
    assert counts[0][1] == counts[0][0] * 4 and counts[1][1] < counts[1][0] * 4
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    pos, o, moved = runs[1][3], 0, []
    for c in chains:
        moved.append((c[0], pos[o:o + len(c[0])], c[2], c[3]))
        o += len(c[0])
    fresh, _, _ = eng.evaluate_f64(moved)
    print(f"compaction: energies {runs[1][0].tolist()}  fresh {fresh.tolist()}")
    assert (np.abs(fresh - runs[1][0]) <= 1e-9 * np.maximum(1.0, np.abs(fresh))).all()
    eng.close()


# 5 --------------------------------------------------------------------------------------------------------------------------------
def test_batched_mc_on_a_rocksalt_slab_with_vacuum():
    """mc.ChainEnsemble with PairSurfCalc, 4 chains, 30 semigrand steps of Na / Cl adatoms over the 8-atom rocksalt slab under
    vacuum, periodic in z: the stored energy of every chain is that of a fresh evaluation and the restatement's, charged states
    included (asserted to occur)."""
    import pair_oracle as po
    from surface_sampling_amd import mc
    from surface_sampling_amd.calculators import PairSurfCalc
    from surface_sampling_amd.structures import Structure

    T, X, C = po.rocksalt(5.64)
    Cz = C.copy(); Cz[2, 2] = 25.0
    base = Structure(np.where(T == 0, 11, 17), X, Cz, [1, 1, 1])
    sites = np.array([[(i + 0.5) * 2.82, (j + 0.5) * 2.82, X[:, 2].max() + 2.6] for i in range(2) for j in range(2)])
    lines = [ln for ln in ec.born(8.0, 1e-8) if " 3 " not in ln and "type 3" not in ln]
    model = _model(lines, 2)
    calc = PairSurfCalc(commands=lines, species=NACL, device="cuda:0")
    ens = mc.ChainEnsemble(base, sites, ("Na", "Cl"), 4, calc, seed=7, relax=False, temperature=1.0)
    ens.initialize()
    charged = 0
    for _ in range(30):
        ens.step_semigrand()
    eng = _engine(model)
    for b in range(4):
        r = ens.relaxed[b]
        Tb = np.where(r.numbers == 11, 0, 1).astype(np.int32)
        Q = float(np.asarray(model.charges)[Tb].sum())
        charged += Q != 0.0
        fresh = eng.evaluate_f64([(Tb, r.positions, r.cell, ec.PBC)])[0][0]
        E, _, _ = eo.ewald(*eo.model_of(model), Tb, r.positions, r.cell)
        print(f"MC chain {b}: {len(r.numbers)} atoms, charge {Q:+.0f}, E {ens.state.energy[b]:.12f}  fresh {fresh:.12f}  restatement {E:.12f}")
        assert abs(fresh - ens.state.energy[b]) <= 1e-9 * max(1.0, abs(fresh)), b
        assert abs(E - ens.state.energy[b]) <= 1e-9 * max(1.0, abs(E)), b
    assert charged > 0 and (ens.num_adsorbates() > 0).any()
    eng.close()


# 6 --------------------------------------------------------------------------------------------------------------------------------
BUCK = ["pair_style buck/coul/long 8.0", "pair_coeff 1 1 500.0 0.30 1.0", "pair_coeff 1 2 1200.0 0.30 5.0", "pair_coeff 2 2 3000.0 0.30 50.0",
        "kspace_style ewald 1e-8", "set type 1 charge 1.0", "set type 2 charge -1.0"]


def test_lammps_surf_calc_serves_buck_coul_long_from_a_run_directory(tmp_path):
    from surface_sampling_amd.calculators import LAMMPSSurfCalc
    from surface_sampling_amd.structures import Structure

    T, X, C, pbc = ec.rattled_cube()
    path = tmp_path / "nacl"
    path.mkdir()
    (path / "lammps_config.json").write_text(json.dumps({"atoms": NACL, "bulk_index": 0}))
    head = "units metal\nboundary p p p\nread_data {}\ngroup bulk id <= {}\n" + "\n".join(BUCK) + "\n"
    (path / "lammps_energy_template.txt").write_text(head + "run 0\n")
    slab = Structure(np.where(T == 0, 11, 17), X, C, [1, 1, 1])
    calc = LAMMPSSurfCalc(device="cuda:0")
    calc.set(run_dir=path)
    _, e, ea = calc.run_lammps_energy(slab)
    m = _model(BUCK, 2)
    E, EA, F = eo.ewald(*eo.model_of(m), T, X, C)
    print(f"LAMMPSSurfCalc buck/coul/long: E {e:.12f}  restatement {E:.12f}")
    assert abs(E - e) <= E_REL * max(1.0, abs(E)) and np.abs(EA - ea).max() <= EA_ABS
    calc.calculate(slab, properties=("energy", "forces", "stress"))
    assert np.abs(calc.results["forces"] - F).max() <= F_ABS and np.isfinite(calc.results["stress"]).all()


# 7 --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from surface_sampling_amd import backend

    m = _model(ec.RAGGED_MODEL)
    c = T, X, C, pbc = ec.rattled_cube()
    eng = _engine(m)
    good = eng.evaluate_f64([c])
    with pytest.raises(backend.BackendError, match=r"vssr error -1: .*three periodic axes"):
        eng.evaluate_f64([(T, X, C, np.array([1, 1, 0], np.uint8))])
    with pytest.raises(backend.BackendError, match=r"vssr error -3: .*reciprocal index 65 along axis 2.*nothing is truncated"):
        eng.evaluate_f64([(T, X, np.diag([5.64, 5.64, 90.0]), pbc)])
    with pytest.raises(backend.BackendError, match=r"vssr error -3: .*reciprocal vectors.*nothing is truncated"):
        eng.evaluate_f64([(T, X, np.diag([40.0, 40.0, 40.0]), pbc)])
    again = eng.evaluate_f64([c])                                  # the handle serves the next batch
    assert all(np.array_equal(a, b) for a, b in zip(good, again))
    long_ = (0, 0, "coul/long", (), 9.0, 0)
    with pytest.raises(backend.BackendError, match=r"vssr_pair_create failed \(-1\): .*vssr_pair_create_kspace"):
        backend.PairEngine([long_], charges=[1.0], n_types=1, device=0)
    with pytest.raises(backend.BackendError, match=r"vssr_pair_create_kspace failed \(-1\): .*needs per-type charges"):
        backend.PairEngine([long_], charges=None, n_types=1, device=0, kspace=(0.3, 2.0))
    for ks in ((0.0, 2.0), (0.3, float("inf")), (float("nan"), 2.0), (0.3, -1.0)):
        with pytest.raises(backend.BackendError, match=r"\(-1\): .*bad k-space parameters"):
            backend.PairEngine([long_], charges=[1.0], n_types=1, device=0, kspace=ks)
    with pytest.raises(backend.BackendError, match=r"\(-1\): .*do not cover the type pair 0 1"):
        backend.PairEngine([long_, (1, 1, "coul/long", (), 9.0, 0)], charges=[1.0, -1.0], n_types=2, device=0, kspace=(0.3, 2.0))
    with pytest.raises(backend.BackendError, match=r"\(-1\): .*differ in rc"):
        backend.PairEngine([long_, (0, 1, "coul/long", (), 8.0, 0), (1, 1, "coul/long", (), 9.0, 0)], charges=[1.0, -1.0], n_types=2,
                           device=0, kspace=(0.3, 2.0))
    with pytest.raises(backend.BackendError, match=r"\(-1\): .*coul/long and coul/dsf"):
        backend.PairEngine([long_, (0, 0, "coul/dsf", (0.2,), 9.0, 0)], charges=[1.0], n_types=1, device=0, kspace=(0.3, 2.0))
    last = eng.evaluate_f64([c])
    assert all(np.array_equal(a, b) for a, b in zip(good, last))
    eng.close()
