"""Slab Ewald sums on the MI355X (vssr_pair_create_kspace_slab, ewald.hip: kspace_style ewald + kspace_modify slab F under boundary
p p f) against the numpy restatement tests/ewald_slab_oracle.py, whose agreement with an exact two-dimensional Ewald sum
tests/test_ewald_slab_cpu.py measures: parity, invariances, batch independence, stress, a relaxation, the batched MC and the refusals.
The inputs are rehearsed on the CPU in tests/test_ewald_slab_cpu.py.

Tolerances are those of tests/test_ewald_gpu.py for the same fp64 quantities: E 1e-10 relative (floor 1 eV), pe/atom 1e-9 eV,
F 1e-8 eV/A; stress: ten times the uncertainty of the strain derivative of the restatement (tests/strain_fd.py).  Every figure is
printed before it is asserted.  No executed LAMMPS is compared.

Measured on an MI355X (worst over the ragged batch): |dE| 1.7e-13 eV, pe/atom 4.1e-14 eV, F 1.1e-14 eV/A; stress: at most 0.42 of the
checker's uncertainty (profiles/r34/NOTES_ewald_slab.md)."""
import math

import numpy as np
import pytest

import cell_cases as cc
import ewald_cases as ec
import ewald_oracle as eo
import ewald_slab_cases as sc
import ewald_slab_oracle as so
import strain_fd as sf

pytestmark = pytest.mark.gpu

E_REL, EA_ABS, F_ABS, STRESS_FACTOR = 1e-10, 1e-9, 1e-8, 10.0
NACL = ["Na", "Cl"]


def _model(lines=None, n_types=3):
    from surface_sampling_amd import pair

    return pair.parse(sc.MODEL if lines is None else lines, n_types)


def _engine(model):
    from surface_sampling_amd import backend

    return backend.PairEngine(model, device=0)


@pytest.fixture(scope="module")
def ragged():
    """The chains of the ragged batch and the restatement's (E, e_atom, F) of each, computed once."""
    m = _model()
    chains = [make() for _, make in sc.RAGGED]
    return m, chains, [so.ewald(*eo.model_of(m), T, X, C) for T, X, C, _ in chains]


def _compare(tag, got, want):
    (e, ea, f), (E, EA, F) = got, want
    de, dea, df = abs(e - E), np.abs(ea - EA).max(), np.abs(f - F).max()
    print(f"{tag} ({len(EA)} atoms): E {E:+.12e}  |dE| {de:.2e}  max|d pe/atom| {dea:.2e}  max|dF| {df:.2e}  max|F| {np.abs(F).max():.3e}")
    assert de <= E_REL * max(1.0, abs(E)), (tag, e, E)
    assert dea <= EA_ABS, (tag, dea)
    assert df <= F_ABS, (tag, df)


# 7, 9 -----------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_against_the_restatement_and_bit_for_bit(ragged):
    """Neutral and charged 8-ion slabs, the in-plane skewed cell, one ion, 63 / 64 / 65 / 70 ions, the thin tall cell, a slab at
    negative z outside the cell in the plane, the charged slab in a left-handed cell: in one batch against the restatement, bit-identical run to run, chain by chain as a
    batch of one, and in reversed order."""
    m, chains, want = ragged
    eng = _engine(m)
    e1, ea1, f1 = eng.evaluate_f64(chains)
    start = np.concatenate([[0], np.cumsum([len(c[0]) for c in chains])])
    for b, (name, _) in enumerate(sc.RAGGED):
        _compare(name, (e1[b], ea1[start[b]:start[b + 1]], f1[start[b]:start[b + 1]]), want[b])
    # one ion: what the dipole term adds is its closed form -qqrd2e 2 pi q^2 L'^2 / (12 V')
    b = [n for n, _ in sc.RAGGED].index("single")
    T, X, C, _ = chains[b]
    ks = m.kspace
    plain = so.coulomb(m.charges, ks.g_ewald, 10.0, ks.k_cut, sc.F, T, X, C, correct=False)[0]
    closed = -so.QQRD2E * 2 * math.pi * (sc.F * C[2, 2]) ** 2 / (12.0 * sc.F * abs(np.linalg.det(C)))
    print(f"single ion: device E - uncorrected restatement {e1[b] - plain:.12f}  closed form {closed:.12f}")
    assert abs(e1[b] - plain - closed) <= E_REL * max(1.0, abs(e1[b]))
    # rows a and b exchanged (det < 0, the kernels' normal along -z): the same lattice, the same energy
    names = [n for n, _ in sc.RAGGED]
    dl = abs(e1[names.index("lefthanded8")] - e1[names.index("charged8")])
    print(f"left-handed cell: |E - E(charged8)| {dl:.2e}")
    assert dl <= E_REL * max(1.0, abs(e1[names.index("charged8")]))
    e2, ea2, f2 = eng.evaluate_f64(chains)
    assert np.array_equal(e1, e2) and np.array_equal(ea1, ea2) and np.array_equal(f1, f2)
    for b, c in enumerate(chains):
        e, ea, f = eng.evaluate_f64([c])
        assert e[0] == e1[b] and np.array_equal(ea, ea1[start[b]:start[b + 1]]) and np.array_equal(f, f1[start[b]:start[b + 1]]), b
    e3, ea3, f3 = eng.evaluate_f64(chains[::-1])
    assert np.array_equal(e3[::-1], e1)
    o = 0
    for b in reversed(range(len(chains))):
        n = len(chains[b][0])
        assert np.array_equal(ea3[o:o + n], ea1[start[b]:start[b + 1]]) and np.array_equal(f3[o:o + n], f1[start[b]:start[b + 1]]), b
        o += n
    eng.close()


# 8 --------------------------------------------------------------------------------------------------------------------------------
def test_shifts_leave_the_energy_of_a_charged_slab_unchanged(ragged):
    m, chains, want = ragged
    b = [n for n, _ in sc.RAGGED].index("charged8")
    T, X, C, pbc = chains[b]
    eng = _engine(m)
    e = eng.evaluate_f64([(T, X, C, pbc), (T, X + [0, 0, sc.SHIFT_Z], C, pbc), (T, X + sc.in_plane_shift(C), C, pbc)])[0]
    print(f"charged slab: E {e[0]:.12f}  |dE| after +{sc.SHIFT_Z} A along z {abs(e[1] - e[0]):.2e}  after 2.3 a - 1.7 b {abs(e[2] - e[0]):.2e}")
    assert abs(e[1] - e[0]) <= E_REL * max(1.0, abs(e[0])) and abs(e[2] - e[0]) <= E_REL * max(1.0, abs(e[0]))
    eng.close()


# 10 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, make, rc", sc.STRESS, ids=[s[0] for s in sc.STRESS])
def test_stress_is_the_strain_derivative_per_real_volume(name, make, rc):
    """born/coul/long at A = 1e-12 against the strain derivative of the restatement at the k set of the unstrained extended cell.
    The comparison is of stress x |det cell|: a division by the extended volume would leave every component a factor F short."""
    T, X, C, pbc = s = make()
    _, _, _, rv = cc.brute_neighbors(X, C, pbc, rc + 1.0)
    assert np.abs(np.linalg.norm(rv, axis=1) - rc).min() > 0.01
    m = _model(sc.slab_lines(ec.born(rc, 1e-12)))
    terms, q, ks = eo.model_of(m)
    eng = _engine(m)
    e, ea, f = eng.evaluate_f64([s])
    st = eng.stress()[0][0]
    _compare(f"stress {name}", (e[0], ea, f), so.ewald(terms, q, ks, T, X, C))
    hkl = so.k_indices(C, ks.k_cut, ks.slab)[0]
    chk = sf.fd_stress(lambda x, c: so.ewald(terms, q, ks, T, x, c, hkl=hkl)[0], X, C)
    assert chk.volume == abs(np.linalg.det(C))
    dev = st * chk.volume
    ratio = np.abs(dev - chk.virial) / chk.unc
    print(f"stress {name} virial: device {dev}  checker {chk.virial}  unc {chk.unc}  max ratio {ratio.max():.3f}")
    assert (np.abs(dev - chk.virial) <= STRESS_FACTOR * chk.unc).all(), (dev, chk.virial, chk.unc)
    assert np.abs(chk.virial[:3]).max() > 1e3 * chk.unc.max()                  # (a factor F would not hide in the uncertainty)
    eng.close()


# 11 -------------------------------------------------------------------------------------------------------------------------------
def test_fire_relaxation_of_a_two_layer_slab():
    from surface_sampling_amd import backend

    tol = 1e-3
    m = _model(sc.slab_lines(ec.born(8.0, 1e-8)))
    (T, X, C, pbc), fixed = sc.relax16()
    eng = _engine(m)
    e0, _, f0 = eng.evaluate_f64([(T, X, C, pbc)])
    assert np.abs(f0[~fixed]).max() > 50 * tol
    eng.upload([(T, X, C, pbc)])
    info = eng.relax("FIRE", fixed=fixed, max_steps=600, fmax=tol, want=backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM)
    print(f"FIRE: {info['n_steps'][0]} steps, converged {info['converged'][0]}")
    assert info["converged"][0]
    pos = info["positions"]
    e, ea, f = eng.results_f64()
    assert np.array_equal(pos[fixed], X[fixed])
    fresh, _, ffresh = eng.evaluate_f64([(T, pos, C, pbc)])
    E = so.ewald(*eo.model_of(m), T, pos, C)[0]
    fmax = np.linalg.norm(ffresh[~fixed], axis=1).max()
    print(f"FIRE: E {e0[0]:.9f} -> {e[0]:.9f} eV  fresh {fresh[0]:.9f}  restatement {E:.9f}  fmax {fmax:.3e}")
    assert abs(e[0] - fresh[0]) <= 1e-9 * max(1.0, abs(fresh[0]))
    assert abs(E - fresh[0]) <= E_REL * max(1.0, abs(E))
    assert e[0] < e0[0] and fmax <= float(np.float32(tol))
    eng.close()


# 12 -------------------------------------------------------------------------------------------------------------------------------
def test_batched_mc_on_a_rocksalt_slab():
    """mc.ChainEnsemble with PairSurfCalc(slab=3.0), 4 chains, 30 semigrand steps of Na / Cl adatoms over the 8-atom rocksalt slab:
    after every step the stored energy of every chain is that of a fresh evaluation and the restatement's -- every accepted state of
    the trajectory, charged, partially filled and neutral ones included (counted and asserted)."""
    import pair_oracle as po
    from surface_sampling_amd import mc
    from surface_sampling_amd.calculators import PairSurfCalc
    from surface_sampling_amd.structures import Structure

    T, X, C = po.rocksalt(5.64)
    Cz = C.copy(); Cz[2, 2] = 25.0
    X = X + [0.0, 0.0, 2.0]
    base = Structure(np.where(T == 0, 11, 17), X, Cz, [1, 1, 1])          # (the calculator imposes pbc 1 1 0)
    sites = np.array([[(i + 0.5) * 2.82, (j + 0.5) * 2.82, X[:, 2].max() + 2.6] for i in range(2) for j in range(2)])
    lines = [ln for ln in ec.born(8.0, 1e-8) if " 3 " not in ln and "type 3" not in ln]
    calc = PairSurfCalc(commands=lines, species=NACL, device="cuda:0", slab=3.0)
    model = calc.pair_model
    assert model.kspace.slab == 3.0
    ens = mc.ChainEnsemble(base, sites, ("Na", "Cl"), 4, calc, seed=7, relax=False, temperature=1.0)
    ens.initialize()
    eng = _engine(model)
    seen, worst = {}, 0.0                                                   # (total charge, adatoms) -> states met over the trajectory
    for step in range(31):                                                  # the initial states, then the states after every step
        if step:
            ens.step_semigrand()
        for b in range(4):
            r = ens.relaxed[b]
            Tb = np.where(r.numbers == 11, 0, 1).astype(np.int32)
            Q = float(np.asarray(model.charges)[Tb].sum())
            seen[(Q, len(Tb) - 8)] = seen.get((Q, len(Tb) - 8), 0) + 1
            fresh = eng.evaluate_f64([(Tb, r.positions, r.cell, sc.PBC)])[0][0]
            E = so.ewald(*eo.model_of(model), Tb, r.positions, r.cell)[0]
            worst = max(worst, abs(fresh - ens.state.energy[b]), abs(E - ens.state.energy[b]))
            if step in (0, 30) or step % 10 == 0:
                print(f"MC step {step} chain {b}: {len(Tb)} atoms, charge {Q:+.0f}, E {ens.state.energy[b]:.12f}  fresh {fresh:.12f}  restatement {E:.12f}")
            assert abs(fresh - ens.state.energy[b]) <= 1e-9 * max(1.0, abs(fresh)), (step, b)
            assert abs(E - ens.state.energy[b]) <= 1e-9 * max(1.0, abs(E)), (step, b)
    charged = sum(n for (Q, _), n in seen.items() if Q != 0.0)
    print(f"MC: (charge, adatoms) -> states met {dict(sorted(seen.items()))}  charged states {charged} of 124  worst |dE| {worst:.2e} eV")
    assert charged > 0 and (ens.num_adsorbates() > 0).any()
    # (not only the saturated end states: partially filled charged states, and neutral states with adatoms or none)
    assert any(Q != 0.0 and 0 < n < 4 for Q, n in seen) and any(Q == 0.0 for Q, _ in seen)
    eng.close()


# 13 -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(ragged):
    from surface_sampling_amd import backend

    m, chains, _ = ragged
    T, X, C, pbc = chains[0]
    eng = _engine(m)
    good = eng.evaluate_f64(chains[:3])
    for bad in ([1, 1, 1], [1, 0, 1]):
        with pytest.raises(backend.BackendError, match=rf"vssr error -1: .*slab Ewald sum needs pbc 1 1 0 \(pbc {bad[0]} {bad[1]} {bad[2]}\)"):
            eng.evaluate_f64([(T, X, C, np.array(bad, np.uint8))])
    tilted = C.copy(); tilted[2, 0] = 0.5
    with pytest.raises(backend.BackendError, match=r"vssr error -1: .*c along z"):
        eng.evaluate_f64([(T, X, tilted, pbc)])
    tilted = C.copy(); tilted[1, 2] = 1e-6
    with pytest.raises(backend.BackendError, match=r"vssr error -1: .*a and b in the xy plane"):
        eng.evaluate_f64([(T, X, tilted, pbc)])
    far = X.copy(); far[3, 2] += 13.0
    with pytest.raises(backend.BackendError, match=r"vssr error -1: .*atoms span .* A along z, more than \|c\| = 12 A"):
        eng.evaluate_f64([(T, far, C, pbc)])
    with pytest.raises(backend.BackendError, match=r"vssr error -3: .*reciprocal index 70 along axis 2 of the cell extended to 120 A.*nothing is truncated"):
        eng.evaluate_f64([(T, X, np.diag([5.64, 5.64, 40.0]), pbc)])
    with pytest.raises(backend.BackendError, match=r"vssr error -3: .*reciprocal vectors of the cell extended to 90 A.*nothing is truncated"):
        eng.evaluate_f64([(T, X, np.diag([40.0, 40.0, 30.0]), pbc)])
    again = eng.evaluate_f64(chains[:3])
    assert all(np.array_equal(a, b) for a, b in zip(good, again))
    terms = [tuple(t) for t in m.terms]
    ks = m.kspace
    for bad in (1.0, float("nan"), float("inf"), 0.5, -3.0):
        with pytest.raises(backend.BackendError, match=r"vssr_pair_create_kspace_slab failed \(-1\): .*bad slab parameter"):
            backend.PairEngine(terms, charges=m.charges, n_types=3, device=0, kspace=(ks.g_ewald, ks.k_cut, bad))
    with pytest.raises(backend.BackendError, match=r"vssr_pair_create_kspace_slab failed \(-1\): .*bad k-space parameters"):
        backend.PairEngine(terms, charges=m.charges, n_types=3, device=0, kspace=(0.0, ks.k_cut, 3.0))
    same = backend.PairEngine(terms, charges=m.charges, n_types=3, device=0, kspace=(ks.g_ewald, ks.k_cut, 3.0))
    assert all(np.array_equal(a, b) for a, b in zip(good, same.evaluate_f64(chains[:3])))
    same.close()
    last = eng.evaluate_f64(chains[:3])
    assert all(np.array_equal(a, b) for a, b in zip(good, last))
    eng.close()


# 14 -------------------------------------------------------------------------------------------------------------------------------
def test_a_handle_without_the_slab_factor_still_refuses_an_open_axis():
    from surface_sampling_amd import backend

    m = _model(ec.coul(10.0, 1e-8))
    assert m.kspace.slab == 0.0
    T, X, C, pbc = sc.dipolar8()
    eng = _engine(m)
    with pytest.raises(backend.BackendError, match=r"vssr error -1: configuration 0: an Ewald sum needs three periodic axes \(pbc 1 1 0; no slab correction\)"):
        eng.evaluate_f64([(T, X, C, pbc)])
    e = eng.evaluate_f64([(T, X, C, ec.PBC)])[0]
    assert np.isfinite(e).all()
    eng.close()
