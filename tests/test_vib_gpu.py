"""Device harmonic vibrations (vssr_batch_vibrations: csrc/vib.hip, csrc/jacobi_dev.h) against the numpy restatement
tests/vib_oracle.py driven by the device's own single-point forces, against LAPACK, and against themselves across replica counts."""
import os

import numpy as np
import pytest

import vib_cases as vc
import vib_oracle as vo
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KEYS = ("energies", "hessian", "modes", "energy", "zpe", "f_vib", "m", "n_imag", "n_left_out", "stop_reason")


def _vib(eng, structs, idx, n_rep=None, **kw):
    """Upload (every structure n_rep times), one vibrations call; the engine's dict plus the counters."""
    S, I = (structs, idx) if n_rep is None else vc.repeat(structs, idx, n_rep)
    eng.upload(S)
    out = eng.vibrations(vc.masses(S), vib=vc.mask_of(S, I), n_rep=n_rep, want=vc.WANT, return_hessian=True, return_modes=True, **kw)
    out["counts"], out["regrows"] = eng.last_relax_counts, eng.debug_capacity()
    return out


def _same(a, b, ga, gb, tag):
    """Group ga of a equals group gb of b bit for bit."""
    for k in KEYS:
        assert np.array_equal(a[k][ga], b[k][gb], equal_nan=True), (tag, k)


def _positions(eng, mass):
    """The resident positions: what a molecular-dynamics call of no steps hands back."""
    eng.set_velocities(None)
    return eng.md(mass, 0, 1.0, want=vc.WANT, driver="lockstep")["positions"]


def _chain_forces(eng, struct):
    """The device's own single-point forces of one chain as the oracle's force function: the potential's tolerance does not enter."""
    from surface_sampling_amd import backend

    n_atoms, T, _, cell, pbc = backend.pack_batch([struct])
    return lambda p: eng.evaluate_arrays_f64(n_atoms, T, p, cell, pbc)[2]


# A ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfree,method", [(2, "standard"), (4, "frederiksen")])
@pytest.mark.parametrize("kind", vc.ASSEMBLY_KINDS)
def test_assembly_against_the_oracle_on_the_devices_own_forces(kind, nfree, method, golden):
    eng = vc.engine(kind, golden)
    structs, idx = vc.assembly_batch(kind)
    ms = [3 * len(i) for i in idx]
    out = _vib(eng, structs, idx, delta=0.01, nfree=nfree, method=method)
    assert list(out["m"]) == ms == [3, 6, 9, 15, 0] and list(out["stop_reason"]) == [1] * 5
    assert out["counts"][0] == vc.evaluations(ms, [1] * 5, nfree) == nfree * 15 + 1
    assert out["hessian"][4].shape == (0, 0) and out["energies"][4].shape == (0,) and out["zpe"][4] == 0.0
    after = eng.results_f64()
    pos = _positions(eng, vc.masses(structs))
    assert np.array_equal(pos, np.concatenate([s[1] for s in structs]))
    fresh = eng.evaluate_f64(structs)
    for a, b in zip(after, fresh):
        assert np.array_equal(a, b)
    assert np.array_equal(out["energy"], fresh[0])
    for g, (s, ix) in enumerate(zip(structs, idx)):
        H = vo.hessian(_chain_forces(eng, s), s[1], ix, 0.01, nfree, method)
        err = float(np.abs(out["hessian"][g] - H).max()) if len(ix) else 0.0
        print(f"{kind} nfree {nfree} {method} chain {g}: max |H| {np.abs(H).max() if len(ix) else 0.0:.3e}, max |device - oracle| {err:.3e}")
        assert np.isfinite(H).all() and err <= 1e-12 * (np.abs(H).max() if len(ix) else 0.0)
        if len(ix):
            mv = vc.TYPE_MASS[np.asarray(s[0])[ix] % 3]
            A = vo.mass_weighted(out["hessian"][g], mv)          # (compared as eigenvalues: a square root magnifies the noise of a zero mode)
            w2 = np.sign(out["energies"][g]) * (out["energies"][g] / vo.S_UNIT) ** 2
            assert np.abs(w2 - np.linalg.eigvalsh(A)).max() <= 64 * len(w2) * EPS * np.linalg.norm(A)
            zpe, f, n_imag, n_out = vo.thermo(out["energies"][g])
            assert np.isclose(out["zpe"][g], zpe, rtol=1e-14, atol=0) and out["f_vib"][g] == out["zpe"][g]
            assert (out["n_imag"][g], out["n_left_out"][g]) == (n_imag, n_out)
    eng.close()


@pytest.mark.parametrize("kind", ["ewald", "vashishta"])
def test_assembly_on_the_other_fp64_kinds(kind):
    """Pair handles with k-space and Vashishta handles: periodic cells, two structures, the first two atoms of each vibrate, one
    structure as two replicas.  The oracle's forces come from evaluations of the whole batch with one chain displaced."""
    from surface_sampling_amd import backend, pair

    if kind == "ewald":
        import ewald_cases as ec

        structs = [ec.rattled_cube(), ec.cube()]
        eng = backend.PairEngine(pair.parse(ec.RAGGED_MODEL, 3), device=0)
    else:
        import vashishta_oracle as vh

        structs = [vh.rattled_sic(seed=2, sigma=0.08, reps=(2, 1, 1)), vh.rattled_sic(seed=3, sigma=0.05)]
        eng = backend.VashishtaEngine(vh.sic_params()[1], device=0)
    idx = [[0, 1], [0, 1]]
    out = _vib(eng, structs, idx, n_rep=[2, 1], delta=0.01, nfree=2, method="frederiksen")
    assert list(out["m"]) == [6, 6] and list(out["stop_reason"]) == [1, 1]
    need = vc.evaluations([6, 6], [2, 1], 2)
    # (rows under the 8 A cutoff of the k-space model outgrow the default capacity: the regrow repeats the evaluations of its poll window)
    assert need == 13 and (out["counts"][0] == need if out["regrows"] == 0 else out["counts"][0] > need)
    after = eng.results_f64()
    S, _ = vc.repeat(structs, idx, [2, 1])
    n_atoms, T, pos0, cell, pbc = backend.pack_batch(S)
    fresh = eng.evaluate_arrays_f64(n_atoms, T, pos0, cell, pbc)
    for a, b in zip(after, fresh):
        assert np.array_equal(a, b)
    start = vc.start(S)
    for g, b in ((0, 0), (1, 2)):
        a0, a1 = start[b], start[b + 1]

        def fn(p):
            q = pos0.copy()
            q[a0:a1] = p
            return eng.evaluate_arrays_f64(n_atoms, T, q, cell, pbc)[2][a0:a1]

        H = vo.hessian(fn, S[b][1], idx[g], 0.01, 2, "frederiksen")
        err = float(np.abs(out["hessian"][g] - H).max())
        print(f"{kind} group {g}: max |H| {np.abs(H).max():.3e}, max |device - oracle| {err:.3e}")
        assert np.isfinite(H).all() and np.abs(H).max() > 1e-3 and err <= 1e-12 * np.abs(H).max()
    eng.close()


# B ---------------------------------------------------------------------------------------------------------------------------------
def test_replicas_share_a_structure_without_changing_a_bit():
    from surface_sampling_amd import backend

    eng = vc.engine("pair_lj")
    structs, idx = vc.replica_structs()
    kw = dict(delta=0.01, nfree=2, temperature=300.0, e_min=1e-4)
    alone = [_vib(eng, [s], [ix], **kw) for s, ix in zip(structs, idx)]
    assert alone[0]["m"][0] == 12 and alone[0]["stop_reason"][0] == 1 and np.isfinite(alone[0]["hessian"][0]).all()
    assert alone[0]["f_vib"][0] < alone[0]["zpe"][0]
    for n in vc.REPLICA_COUNTS:
        r = _vib(eng, structs[:1], idx[:1], n_rep=[n], **kw)
        assert r["counts"][0] == vc.evaluations([12], [n], 2) and len(r["m"]) == 1
        _same(r, alone[0], 0, 0, f"n_rep {n}")
    both = _vib(eng, structs, idx, n_rep=[3, 2], **kw)
    assert both["counts"][0] == vc.evaluations([12, 6], [3, 2], 2) == 9
    _same(both, alone[0], 0, 0, "(3, 2) group 0")
    _same(both, alone[1], 1, 0, "(3, 2) group 1")
    again = _vib(eng, structs, idx, n_rep=[3, 2], **kw)          # F (iii): the same call twice
    for g in (0, 1):
        _same(again, both, g, g, "repeat")
    # a replica whose position differs in one bit
    S, I = vc.repeat(structs[:1], idx[:1], [5])
    T, pos, cell, pbc = S[3]
    off = pos.copy()
    off[20, 1] = np.nextafter(off[20, 1], np.inf)
    S[3] = (T, off, cell, pbc)
    eng.upload(S)
    with pytest.raises(backend.BackendError, match="vssr error -1.*replicas"):
        eng.vibrations(vc.masses(S), vib=vc.mask_of(S, I), n_rep=[5], want=vc.WANT)
    for bad in ([4], [5, 1], [0, 5]):
        with pytest.raises(backend.BackendError, match="vssr error -1"):
            eng.vibrations(vc.masses(S), vib=vc.mask_of(S, I), n_rep=bad, want=vc.WANT)
    m5 = vc.masses(S)
    m5[27 + 3] *= 1.0 + 2 * EPS
    with pytest.raises(backend.BackendError, match="vssr error -1.*masses"):
        eng.vibrations(m5, vib=vc.mask_of(S, I), n_rep=[5], want=vc.WANT)
    for kw_bad in (dict(nfree=3), dict(delta=0.0), dict(delta=np.nan), dict(temperature=-1.0), dict(e_min=-1.0)):
        with pytest.raises(backend.BackendError, match="vssr error -1"):
            eng.vibrations(vc.masses(S), vib=vc.mask_of(S, I), **kw_bad)
    ok = _vib(eng, structs[:1], idx[:1], n_rep=[5], **kw)        # the handle is still usable
    _same(ok, alone[0], 0, 0, "after the refusals")
    fresh = backend.PairEngine(vc.cc.LJ_TERMS, n_types=vc.cc.LJ_NTYPES, device=0)
    with pytest.raises(backend.BackendError, match="vssr error -5"):
        fresh.vibrations(np.zeros(0), want=vc.WANT)             # before an upload
    fresh.close()
    eng.close()


# C ---------------------------------------------------------------------------------------------------------------------------------
def test_jacobi_against_lapack():
    from surface_sampling_amd import backend

    eng = vc.engine("pair_lj")
    structs, idx = vc.eigen_batch()
    out = _vib(eng, structs, idx, delta=0.01, nfree=2)
    assert list(out["m"]) == [3, 6, 9, 96, 255] and out["counts"][0] == 511
    assert list(out["stop_reason"]) == [1] * 5                   # every solve ended below the sweep limit
    for g, s in enumerate(structs):
        m = int(out["m"][g])
        A = vo.mass_weighted(out["hessian"][g], vc.TYPE_MASS[np.asarray(s[0]) % 3])
        bound = 64 * m * EPS * np.linalg.norm(A)
        e, V = out["energies"][g], out["modes"][g]
        w2 = np.sign(e) * (e / vo.S_UNIT) ** 2
        lam = np.linalg.eigvalsh(A)
        err = float(np.abs(w2 - lam).max())
        ortho = float(np.abs(V @ V.T - np.eye(m)).max())
        resid = float(np.linalg.norm(V @ A - w2[:, None] * V, axis=1).max())
        print(f"m = {m}: |A|_F {np.linalg.norm(A):.3e}, eigenvalues {err:.2e}, residual {resid:.2e} (bound {bound:.2e}); "
              f"orthonormality {ortho:.2e} (bound {64 * m * EPS:.2e})")
        assert (np.diff(w2) >= 0).all()
        if g == 0:                                               # one atom alone: the zero matrix
            assert not A.any() and not e.any() and np.array_equal(np.abs(V), np.eye(3))
            continue
        assert err <= bound and resid <= bound and ortho <= 64 * m * EPS
        for v in V:                                              # the largest-magnitude entry is positive, the first one on ties
            assert v[int(np.argmax(np.abs(v)))] > 0
    T, pos, cell, pbc = vc.too_many()
    eng.upload([(T, pos, cell, pbc)])
    with pytest.raises(backend.BackendError, match="vssr error -1.*degrees of freedom"):
        eng.vibrations(vc.masses([(T, pos, cell, pbc)]), want=vc.WANT)
    eng.close()


# D ---------------------------------------------------------------------------------------------------------------------------------
def test_morse_dimer_through_the_calculator():
    from surface_sampling_amd.calculators import PairSurfCalc
    from surface_sampling_amd.structures import Structure

    _, pos, cell, _ = vc.morse_dimer()
    s = Structure([8, 1], pos, cell, [False] * 3)
    calc = PairSurfCalc(commands=vc.MORSE_COMMANDS, species=["O", "H"], device="cuda:0")
    exact = vc.morse_top_mode()
    r2 = calc.vibrations_batch([s], nfree=2, e_min=1e-3)[0]
    r4 = calc.vibrations_batch([s], nfree=4, e_min=1e-3)[0]
    print(f"Morse dimer: top mode {r2['energies'][-1]:.10f} eV (nfree 2), {r4['energies'][-1]:.10f} eV (nfree 4), closed form {exact:.10f} eV")
    assert abs(r2["energies"][-1] / exact - 1.0) < 2e-4
    assert abs(r4["energies"][-1] / exact - 1.0) < 1e-6
    for r in (r2, r4):
        assert r["zpe"] == 0.5 * r["energies"][-1] == r["helmholtz_vib"] and r["n_left_out"] == 5 and r["stop_reason"] == 1
        assert np.array_equal(r["frequencies"], r["energies"] / 1.239841984e-4) and r["replicas"] == 6


# E ---------------------------------------------------------------------------------------------------------------------------------
def test_painn_hessian_against_the_fp64_oracle(golden, oracle_mod):
    from surface_sampling_amd import backend, structures
    from surface_sampling_amd.calculators import EnsembleNFFSurface

    st = golden.structure("SrTiO3_2x2_pristine")
    Z, pos, cell, pbc = structures.as_arrays(st)
    assert len(Z) == 60
    order = np.argsort(-pos[:, 2], kind="stable")
    ix = sorted(int(i) for i in order[:2])                       # the two topmost atoms
    mass = structures.masses_of(st)
    H = {bits: vo.hessian(lambda p: oracle_mod.ensemble(golden.blobs, Z, p, cell, pbc, bits)["forces"], pos, ix, 0.01, 2) for bits in (64, 32)}
    bound = 2.0 * float(np.abs(H[32] - H[64]).max())
    eng = backend.PainnEngine(golden.blobs, device=0)
    eng.upload([(Z, pos, cell, pbc)])
    vib = np.zeros(60, np.uint8)
    vib[ix] = 1
    out = eng.vibrations(mass, vib=vib, delta=0.01, nfree=2, return_hessian=True, return_modes=True)
    dev = float(np.abs(out["hessian"][0] - H[64]).max())
    print(f"PaiNN Hessian, 2 vib atoms of the 60-atom SrTiO3 slab: max |H| {np.abs(H[64]).max():.4e} eV/A^2; oracle fp32 mode against fp64 mode "
          f"{bound / 2:.3e}; device against fp64 mode {dev:.3e} (bound {bound:.3e})")
    assert out["stop_reason"][0] == 1 and out["m"][0] == 6
    assert dev <= bound
    e = out["energies"][0]
    w2 = np.sign(e) * (e / vo.S_UNIT) ** 2
    lam = np.linalg.eigvalsh(vo.mass_weighted(H[64], mass[ix]))
    eb = bound * float((1.0 / mass[ix]).max())
    print(f"PaiNN eigenvalues of D H D: max |device - fp64 oracle| {np.abs(w2 - lam).max():.3e} (bound {eb:.3e})")
    assert np.abs(w2 - lam).max() <= eb
    eng.close()
    # the calculator hands out what the engine computed
    calc = EnsembleNFFSurface(golden.blobs, device="cuda:0", model_units="kcal/mol", prediction_units="eV", offset_units="atomic")
    r = calc.vibrations_batch([st], indices=ix, replicas=1, return_hessian=True)[0]
    assert np.array_equal(r["hessian"], out["hessian"][0]) and np.array_equal(r["energies"], e) and r["replicas"] == 1


# F ---------------------------------------------------------------------------------------------------------------------------------
def test_a_capacity_overflow_repeats_evaluations_without_changing_a_bit():
    s = vc.tight_cluster()
    idx = [list(range(27))]
    kw = dict(n_rep=[9], delta=vc.TIGHT_DELTA, nfree=2, method="frederiksen", temperature=200.0)
    roomy_eng = vc.engine("pair_lj")
    roomy = _vib(roomy_eng, [s], idx, **kw)
    roomy_eng.close()
    tight_eng = vc.engine("pair_lj")
    tight_eng.debug_capacity(slots_per_atom=vc.TIGHT_SLOTS_PER_ATOM, tight=1)
    tight = _vib(tight_eng, [s], idx, **kw)
    print(f"roomy counts {roomy['counts']} regrows {roomy['regrows']}; tight counts {tight['counts']} regrows {tight['regrows']}")
    assert roomy["regrows"] == 0 and roomy["counts"][0] == vc.evaluations([81], [9], 2) == 19
    assert tight["regrows"] >= 1 and tight["counts"][0] > 19
    _same(tight, roomy, 0, 0, "tight against roomy")
    assert roomy["stop_reason"][0] == 1 and np.isfinite(roomy["hessian"][0]).all()
    # (iv) stress and stats are served at once
    stress, _ = tight_eng.stress()
    assert stress.shape == (9, 6) and np.isfinite(stress).all() and np.array_equal(stress[0], stress[8])
    assert tight_eng.stats()["atoms"] == 9 * 27 and tight_eng.stats()["edges"] == 9 * vc.slots(s[1])[1]
    tight_eng.close()


def test_a_collision_voids_its_group_only():
    eng = vc.engine("pair_lj")
    structs, idx = vc.collide_batch()
    kw = dict(delta=vc.COLLIDE_DELTA, nfree=2)
    out = _vib(eng, structs, idx, **kw)
    after = eng.results_f64()
    assert list(out["stop_reason"]) == [1, 2, 1] and list(out["m"]) == [6, 6, 9]
    for k in ("energies", "hessian", "modes"):
        assert np.isnan(out[k][1]).all() and out[k][1].shape[0] == 6
    assert np.isnan(out["zpe"][1]) and np.isnan(out["f_vib"][1]) and np.isfinite(out["energy"]).all()
    pos = _positions(eng, vc.masses(structs))
    assert np.array_equal(pos, np.concatenate([s[1] for s in structs]))
    fresh = eng.evaluate_f64(structs)
    for a, b in zip(after, fresh):                               # the final evaluation is complete, the dimer's chain included
        assert np.array_equal(a, b)
    assert np.array_equal(out["energy"], fresh[0])
    for g in (0, 2):
        alone = _vib(eng, [structs[g]], [idx[g]], **kw)
        _same(out, alone, g, 0, f"group {g} alone")
    eng.close()


# G ---------------------------------------------------------------------------------------------------------------------------------
def test_vibrations_batch_end_to_end_on_the_cu_au_slab():
    from surface_sampling_amd import structures
    from surface_sampling_amd.calculators import EAMSurfCalc
    from surface_sampling_amd.structures import Structure

    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    hollow = d["ads_coords"][int(np.argmin(d["ads_coords"][:, 2]))]
    s = Structure(np.append(d["numbers"], 79), np.vstack([d["positions"], hollow]), d["cell"], d["pbc"])
    calc = EAMSurfCalc(files=[os.path.join(GOLDEN, "Cu_u3.eam"), os.path.join(GOLDEN, "Au_u3.eam")], device="cuda:0")
    calc.set(pair_style="eam", pair_coeff=["1 1 Cu_u3.eam", "2 2 Au_u3.eam"])
    r = calc.vibrations_batch([s], indices=[8], replicas="auto", temperature=300.0, return_hessian=True, return_modes=True)[0]
    for k in ("energies", "frequencies", "zpe", "helmholtz_vib", "n_imag", "n_left_out", "energy", "hessian", "modes"):
        assert k in r, k
    print(f"Au on Cu(100): energies {r['energies']} eV, zpe {r['zpe']:.5f} eV, f_vib(300 K) {r['helmholtz_vib']:.5f} eV, n_imag {r['n_imag']}")
    assert r["energies"].shape == (3,) and r["hessian"].shape == (3, 3) and r["replicas"] == 3 and r["stop_reason"] == 1
    assert np.array_equal(r["frequencies"], r["energies"] / 1.239841984e-4)
    assert r["energies"][-1] > 0 and r["helmholtz_vib"] < r["zpe"]
    assert r["energy"] == calc.calculate_batch([s])[0]["energy"]
    eng = calc._get_engine()
    pk = calc._pack(s)
    eng.upload([pk] * 3)
    vib = np.zeros(27, np.uint8)
    vib[[8, 17, 26]] = 1
    ref = eng.vibrations(np.tile(structures.masses_of(s), 3), vib=vib, n_rep=[3], temperature=300.0, want=vc.WANT, return_hessian=True,
                         return_modes=True)
    assert np.array_equal(ref["energies"][0], r["energies"]) and np.array_equal(ref["hessian"][0], r["hessian"])
    assert np.array_equal(ref["modes"][0], r["modes"]) and ref["zpe"][0] == r["zpe"] and ref["f_vib"][0] == r["helmholtz_vib"]
    one = calc.vibrations_batch([s], indices=[8], replicas=1, temperature=300.0, return_hessian=True)[0]
    assert np.array_equal(one["hessian"], r["hessian"]) and one["helmholtz_vib"] == r["helmholtz_vib"]
