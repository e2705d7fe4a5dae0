"""The harmonic-vibrations restatement (tests/vib_oracle.py) checked on its own, the front end / ABI of ``vssr_batch_vibrations`` as far
as they can be checked without a GPU, and rehearsals of what tests/test_vib_gpu.py presumes of its cases."""
import ctypes
import os
import re

import numpy as np
import pytest

import cg_cases as cc
import vib_cases as vc
import vib_oracle as vo
from surface_sampling_amd import backend, calculators, structures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_library_exports_it():
    header = open(os.path.join(ROOT, "include", "vssr_eval.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"enum\s*\{\s*VSSR_VIB_STANDARD\s*=\s*0,\s*VSSR_VIB_FREDERIKSEN\s*=\s*1\s*\}\s*;", flat)
    assert re.search(r"typedef\s+struct\s*\{\s*int32_t\s+nfree;\s*int32_t\s+method;\s*double\s+delta;\s*double\s+temperature;\s*double\s+e_min;\s*\}"
                     r"\s*vssr_vib_params;", flat)
    assert re.search(r"int\s+vssr_batch_vibrations\s*\(\s*vssr_handle\s*\*h,\s*const\s+vssr_vib_params\s*\*p,\s*const\s+double\s*\*mass\s*,\s*"
                     r"const\s+uint8_t\s*\*vib\s*,\s*const\s+int32_t\s*\*n_rep\s*,\s*int32_t\s+n_groups,\s*int32_t\s+ld,\s*uint32_t\s+want,\s*"
                     r"double\s*\*energies\s*,\s*double\s*\*hessian\s*,\s*double\s*\*modes\s*,\s*double\s*\*thermo\s*,\s*int32_t\s*\*info\s*\)\s*;", flat)
    assert re.search(r"#define\s+VSSR_ABI_VERSION\s+1\b", header)
    assert "vssr_batch_vibrations" in backend.EXPORTS
    fn = backend.load_library().vssr_batch_vibrations
    assert fn.argtypes is not None and len(fn.argtypes) == 13
    assert fn(None, None, None, None, None, 0, 0, 0, None, None, None, None, None) == -1     # a null handle: the usual kind check
    assert [n for n, _ in backend.VibParams._fields_] == ["nfree", "method", "delta", "temperature", "e_min"]
    assert ctypes.sizeof(backend.VibParams) == 32
    assert backend.VIB_METHODS == {"standard": 0, "frederiksen": 1}
    assert backend.VIB_ENERGY_UNIT == vo.S_UNIT and abs(vo.S_UNIT - 0.0646541513) < 1e-10 and backend.EV_PER_INV_CM == vo.EV_PER_INV_CM
    for name in dir(backend):
        eng = getattr(backend, name)
        if isinstance(eng, type) and hasattr(eng, "md"):
            assert hasattr(eng, "vibrations"), name
    for name in ("PainnEngine", "TersoffEngine", "SWEngine", "EAMEngine", "PairEngine", "VashishtaEngine"):
        assert hasattr(getattr(backend, name), "vibrations"), name
    for calc in (calculators.EnsembleNFFSurface, calculators.NFFPourbaix, calculators.TersoffSurfCalc, calculators.PairSurfCalc,
                 calculators.EAMSurfCalc):
        assert hasattr(calc, "vibrations_batch"), calc.__name__


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _morse_top(delta, nfree, method="standard"):
    s = vc.morse_dimer()
    H = vo.hessian(vc.pair_force_fn(vc.MORSE_TERMS, s), s[1], [0, 1], delta, nfree, method)
    e, _ = vo.modes(H, vc.MORSE_MASS)
    return H, e


def test_morse_dimer_against_the_closed_form():
    exact = vc.morse_top_mode()
    assert abs(exact - 0.11951050758) < 1e-10
    H, e = _morse_top(0.01, 2)
    err2 = e[-1] / exact - 1.0
    err2h = _morse_top(0.005, 2)[1][-1] / exact - 1.0
    err4 = _morse_top(0.01, 4)[1][-1] / exact - 1.0
    sum_rule = np.abs(H.sum(axis=0)).max() / np.abs(H).max()
    print(f"top mode: relative error {err2:.4e} (nfree 2, delta 0.01), {err2h:.4e} (delta 0.005), {err4:.3e} (nfree 4); "
          f"column sums / max |H| = {sum_rule:.1e}")
    assert abs(err2 - 1.63e-4) <= 0.05e-4
    assert abs(err2 / err2h - 4.0) < 0.05          # second order in delta
    assert abs(err4) < 1e-7
    assert sum_rule < 1e-13
    assert np.array_equal(H, H.T) and (np.abs(e[:5]) < 1e-3).all()      # five rigid motions of a dimer carry no energy


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_thermo():
    e = np.array([-0.02, 0.0, 5e-4, 0.05, 0.12, 0.2])
    zpe, f, n_imag, n_out = vo.thermo(e, 0.0, 1e-3)
    assert zpe == 0.5 * (0.05 + 0.12 + 0.2) and f == zpe and (n_imag, n_out) == (1, 3)
    assert vo.thermo(e, 0.0, 0.0)[3] == 2 and vo.thermo(e, 0.0, 0.0)[0] == 0.5 * (5e-4 + 0.05 + 0.12 + 0.2)
    cold = vo.thermo(e, 1.0, 1e-3)[1]                # kT = 8.6e-5 eV: exp(-0.05 / kT) underflows to 0
    assert cold == zpe
    kT = vo.KB * 300.0
    one = vo.thermo([0.1], 300.0)[1]
    assert np.isclose(one, 0.05 + kT * np.log(1.0 - np.exp(-0.1 / kT)), rtol=1e-14, atol=0) and one < 0.05
    assert vo.thermo([], 300.0) == (0.0, 0.0, 0, 0)
    seq = [vo.thermo(e, T, 1e-3)[1] for T in (300.0, 100.0, 30.0, 10.0)]
    assert all(a < b for a, b in zip(seq, seq[1:])) and abs(seq[-1] - zpe) < 1e-12


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_frederiksen_touches_the_diagonal_blocks_only_and_restores_the_sum_rule():
    s = vc.lj_cluster(8, 31)
    f = vc.lj_force_fn(s)
    idx = [0, 3, 6]                                   # a subset: the rows of the standard Hessian do not sum to zero
    Ks, Kf = (vo.rows(f, s[1], idx, 0.01, 2, m) for m in ("standard", "frederiksen"))
    diag = np.kron(np.eye(3), np.ones((3, 3))).astype(bool)
    assert np.array_equal(Ks[~diag], Kf[~diag]) and not np.array_equal(Ks[diag], Kf[diag])
    Hs, Hf = Ks + Ks.T, Kf + Kf.T
    assert np.abs(Hs.sum(axis=0)).max() > 1e-3 * np.abs(Hs).max()
    full = vo.rows(f, s[1], list(range(8)), 0.01, 2, "frederiksen")
    Hfull = full + full.T
    assert np.abs(Hfull.sum(axis=0)).max() < 1e-12 * np.abs(Hfull).max()
    # with a subset the correction makes every row of the FULL force-constant matrix sum to zero: the diagonal block of a vib atom
    # equals minus the sum of its couplings to all other atoms, vib or not
    every = vo.rows(f, s[1], list(range(8)), 0.01, 2, "standard")
    for k, a in enumerate(idx):
        others = [b for b in range(8) if b != a]
        coupling = sum(every[3 * a:3 * a + 3, 3 * b:3 * b + 3] for b in others)
        assert np.abs(Kf[3 * k:3 * k + 3, 3 * k:3 * k + 3] + coupling).max() < 1e-11 * np.abs(every).max()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_python_side_argument_checks_come_before_any_device_call():
    for bad in ("bogus", "Standard", "", None, 1):
        with pytest.raises(ValueError, match="method"):
            backend.vib_method_code(bad)
    s = structures.Structure([31, 7], np.array([[0, 0, 0], [0, 0, 1.9]], float), np.eye(3) * 10)

    def no_engine():
        raise AssertionError("the engine was asked for before the arguments were checked")

    for calc in (calculators.TersoffSurfCalc.__new__(calculators.TersoffSurfCalc), calculators.EnsembleNFFSurface.__new__(calculators.EnsembleNFFSurface)):
        calc.parameters, calc.results, calc.atoms = {}, {}, None
        calc.species, calc.all_periodic = ["Ga", "N"], True
        calc._get_engine = no_engine
        for kw, match in ((dict(nfree=3), "nfree"), (dict(method="forward"), "method"), (dict(delta=0.0), "delta"), (dict(delta=-0.01), "delta"),
                          (dict(temperature=-1.0), "temperature"), (dict(e_min=-1e-3), "e_min"), (dict(masses=[[1.0, 2.0, 3.0]]), "masses"),
                          (dict(masses=[[1.0, 2.0], [1.0]]), "mass arrays"), (dict(indices=[0, 2]), "out of range"),
                          (dict(indices=[[0], [1]]), "index lists"), (dict(replicas=0), "replicas"), (dict(replicas="many"), "replicas"),
                          (dict(replicas=1.5), "replicas")):
            with pytest.raises(ValueError, match=match):
                calc.vibrations_batch([s], **kw)
    assert [i.tolist() for i in calculators._vib_indices([3, 2], [1, 0])] == [[0, 1], [0, 1]]
    assert [i.tolist() for i in calculators._vib_indices([3, 2], [[2], []])] == [[2], []]
    assert [i.tolist() for i in calculators._vib_indices([3, 2], None)] == [[0, 1, 2], [0, 1]]


# 6: rehearsals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", vc.ASSEMBLY_KINDS)
def test_rehearsal_of_the_assembly_batch(kind, golden, oracle_mod):
    structs, idx = vc.assembly_batch(kind)
    assert tuple(len(s[0]) for s in structs) == vc.ASSEMBLY_SIZES and [3 * len(i) for i in idx] == [3, 6, 9, 15, 0]
    assert [tuple(int(x) for x in s[3]) for s in structs] == [(0, 0, 0)] * 3 + [(1, 1, 0), (0, 0, 0)]
    for s, ix in zip(structs, idx):
        fn = vc.restatement_force_fn(kind, s, golden, oracle_mod)
        for nfree, method in ((2, "standard"), (4, "frederiksen")):
            H = vo.hessian(fn, s[1], ix, 0.01, nfree, method)
            assert H.shape == (3 * len(ix),) * 2 and np.isfinite(H).all()
            if len(s[0]) > 1 and len(ix):
                assert np.abs(H).max() > 1e-3                              # the atoms feel each other
    fn = vc.restatement_force_fn(kind, structs[0], golden, oracle_mod)
    assert not vo.hessian(fn, structs[0][1], [0]).any()                    # one atom alone in an open box feels nothing


def test_rehearsal_of_the_replica_cases():
    structs, idx = vc.replica_structs()
    m = 3 * len(idx[0])
    assert m == 12 and [vc.idle_replicas(m, n) for n in vc.REPLICA_COUNTS] == [[], [], [], [12, 13, 14, 15]]
    assert [vc.evaluations([m], [n], 2) for n in vc.REPLICA_COUNTS] == [25, 7, 3, 3]
    assert vc.evaluations([12, 6], [3, 2], 4) == 17
    for s, ix in zip(structs, idx):
        H = vo.hessian(vc.lj_force_fn(s), s[1], ix)
        e, V = vo.modes(H, vc.TYPE_MASS[s[0][ix] % 3])
        assert np.isfinite(H).all() and np.isfinite(e).all() and np.abs(V @ V.T - np.eye(len(e))).max() < 1e-12
    S, I = vc.repeat(structs, idx, (3, 2))
    assert len(S) == 5 and S[0] is S[2] and S[3] is S[4] and vc.mask_of(S, I).sum() == 3 * 4 + 2 * 2


def test_rehearsal_of_the_eigen_batch():
    structs, idx = vc.eigen_batch()
    assert [3 * len(i) for i in idx] == [3, 6, 9, 96, 255] and 3 * len(vc.too_many()[0]) == 258 > backend.VIB_MAX_DOF
    assert vc.evaluations([3 * len(i) for i in idx], [1] * 5, 2) == 511
    s = structs[3]
    H = vo.hessian(vc.lj_force_fn(s), s[1], idx[3])
    e, V = vo.modes(H, vc.TYPE_MASS[s[0] % 3])
    assert np.isfinite(e).all() and (np.abs(V).max(axis=1) == V.max(axis=1)).all()       # the sign convention
    assert e[-1] > 0.01 and np.abs(V @ V.T - np.eye(96)).max() < 1e-12


def test_rehearsal_of_the_tight_cluster_and_the_collision():
    T, pos, _, _ = vc.tight_cluster()
    need0 = vc.slots(pos)[0]
    assert need0 > 27 * vc.TIGHT_SLOTS_PER_ATOM                       # the start capacity holds not even the undisplaced rows
    edges = {vc.slots(vo.displaced(pos, a, c, k, vc.TIGHT_DELTA))[1] for a in range(27) for c in range(3) for k in (-1, 1)}
    assert max(edges) > vc.slots(pos)[1]                              # and displaced geometries gain neighbors
    structs, idx = vc.collide_batch()
    for g, (s, ix) in enumerate(zip(structs, idx)):
        with np.errstate(all="ignore"):
            H = vo.hessian(vc.lj_force_fn(s), s[1], ix, vc.COLLIDE_DELTA, 2)
        assert np.isfinite(H).all() == (g != 1), g                    # the dimer is the group that blows up, and the only one
    s = structs[1]
    with np.errstate(all="ignore"):
        f0 = vc.lj_force_fn(s)(s[1])
        bad = [(a, c, k) for a in range(2) for c in range(3) for k in (-1, 1)
               if not np.isfinite(vc.lj_force_fn(s)(vo.displaced(s[1], a, c, k, vc.COLLIDE_DELTA))).all()]
    assert np.isfinite(f0).all() and bad == [(0, 0, 1), (1, 0, -1)]


def test_rehearsal_of_the_physics_anchor():
    H, e = _morse_top(0.01, 2)
    zpe, _, n_imag, n_out = vo.thermo(e, 0.0, 1e-3)
    assert n_out == 5 and zpe == 0.5 * e[-1]
    T, pos, cell, pbc = vc.morse_dimer()
    assert abs(np.linalg.norm(pos[1] - pos[0]) - vc.MORSE_R0) < 1e-15
    m = structures.ATOMIC_MASSES[[8, 1]]
    assert np.array_equal(m, vc.MORSE_MASS)
    assert cc.LJ_TERMS[0][3] == vc.LJ00[:2] and cc.LJ_TERMS[0][4] == vc.LJ00[2]
