"""The variable-cell restatement (tests/cellrelax_oracle.py) checked on its own -- its row force against the finite-difference gradient of
the enthalpy, which pins the filter algebra independently of anybody's memory of ASE --, the known answer of Stillinger-Weber silicon,
the front end / ABI of ``vssr_batch_relax_cell`` as far as they can be checked without a GPU, and rehearsals of what
tests/test_cellrelax_gpu.py presumes of its lj/cut cases."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cellrelax_cases as cs
import cellrelax_oracle as co
import pair_cases as pc
from cell_cases import brute_neighbors
import strain_fd as sf
import sw_oracle as so
from surface_sampling_amd import backend, calculators, structures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["max_steps", "nmin", "hydrostatic_strain", "mask", "fmax", "scalar_pressure", "cell_factor", "dt", "maxstep", "dtmax", "finc", "fdec",
          "astart", "fa"]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def _fd_gradient(fn, rows, h):
    """-(d fn / d rows) by strain_fd's recipe, per component: central differences at h, 2 h, 4 h, the Richardson extrapolate of the
    two finer ones, and its uncertainty |fine - coarse| + 4 * 2^-52 |fn| / h."""
    e0 = abs(fn(rows))
    g, unc = np.zeros_like(rows), np.zeros_like(rows)
    for idx in np.ndindex(rows.shape):
        D = []
        for step in (h, 2 * h, 4 * h):
            p, m = rows.copy(), rows.copy()
            p[idx] += step
            m[idx] -= step
            D.append((fn(p) - fn(m)) / (2 * step))
        fine, coarse = (4 * D[0] - D[1]) / 3, (4 * D[1] - D[2]) / 3
        g[idx] = -fine
        unc[idx] = abs(fine - coarse) + 4 * sf.EPS64 * e0 / h
    return g, unc


def _triclinic_si():
    """The 8-atom diamond cell of silicon, sheared, rattled by 0.1 A, at a deformation gradient F that is far from I."""
    T, X, Cl = so.diamond_si(5.50)
    C0 = Cl @ cs.SKEW
    rng = np.random.default_rng(12)
    s = (X @ np.linalg.inv(Cl)) @ C0 + rng.normal(0, 0.1, X.shape)
    F = np.eye(3) + np.array([[0.03, 0.02, -0.01], [-0.015, -0.02, 0.012], [0.008, -0.011, 0.025]])
    return T, s, C0, F


@pytest.mark.parametrize("pressure", [0.0, 0.05])
def test_row_force_is_the_negative_gradient_of_the_enthalpy_sw(pressure):
    """Stillinger-Weber (every derivative continuous at the cutoff) on the triclinic 8-atom cell at F != I: the oracle's N + 3 rows
    against central differences of E + p V with respect to (s, c F), within strain_fd's uncertainty of the differences plus, on the
    cell rows, that of the finite-difference stress the rows are formed from."""
    P = so.si_params()
    T, s, C0, F = _triclinic_si()
    pbc, c = np.ones(3, np.uint8), 8.0
    energy = lambda x, C: so.sw(P, T, x, C, pbc)[0]
    x, C = s @ F.T, C0 @ F.T
    E, _, f = so.sw(P, T, x, C, pbc)
    fd = sf.fd_stress(energy, x, C)
    held = np.zeros(8, bool)
    held[2] = True
    G = co.row_forces(f, fd.sigma, F, fd.volume, pressure, cell_factor=c)
    rows = np.vstack([s, c * F])
    g, unc = _fd_gradient(lambda r: co.enthalpy(energy, r, C0, c, pressure), rows, 1e-4)
    unc[-3:] += np.abs(sf.voigt_to_tensor(fd.unc)) @ np.abs(np.linalg.inv(F)) / c       # dW = -d(V sigma) F^-T
    err = np.abs(G - g)
    print(f"p = {pressure}: |G| up to {np.abs(G).max():.3e} (cell rows {np.abs(G[-3:]).max():.3e}); worst error / bound {np.max(err / unc):.3f}; "
          f"largest error {err.max():.3e}, largest bound {unc.max():.3e}")
    assert np.abs(G[-3:]).max() > 0.1 and np.abs(G[:-3]).max() > 0.1          # neither part is a trivial zero
    assert (err <= unc).all()
    # a held atom: its row is zero, the others are untouched
    Gh = co.row_forces(f, fd.sigma, F, fd.volume, pressure, cell_factor=c, fixed=held)
    assert not Gh[2].any() and np.array_equal(np.delete(Gh, 2, axis=0), np.delete(G, 2, axis=0))


def test_row_force_is_the_negative_gradient_of_the_enthalpy_lj_exact_virial():
    """lj/cut with the exact pair virial (no finite-difference stress on the oracle's side) on a rattled fcc cell under a sheared F != I (the
    deformed cell is triclinic).  The unshifted potential jumps at the cutoff: at a = 4.3 A the cutoff lies between the fourth and the
    fifth neighbor shell, so every pair stays further from it than the differences move one."""
    T, s, C0, pbc = cs.fcc((2, 1, 1), 4.3, 0.02, 23)
    F = np.eye(3) + np.array([[0.02, 0.015, -0.01], [-0.01, -0.02, 0.01], [0.005, -0.01, 0.03]])
    c, p = 8.0, 0.03
    x, C = s @ F.T, C0 @ F.T
    rv = brute_neighbors(x, C, pbc, 7.0)[3]
    margin = np.abs(np.linalg.norm(rv, axis=1) - 6.5).min()
    assert margin > 0.02, margin            # 4 h = 4e-4 in F moves a pair at 6.5 A by 3e-3 A
    E, f, sig = co.pair_virial(cs.LJ, None, T, x, C, pbc)
    G = co.row_forces(f, sig, F, abs(np.linalg.det(C)), p, cell_factor=c)
    energy = lambda xx, CC: co.pair_virial(cs.LJ, None, T, xx, CC, pbc)[0]
    g, unc = _fd_gradient(lambda r: co.enthalpy(energy, r, C0, c, p), np.vstack([s, c * F]), 1e-4)
    err = np.abs(G - g)
    print(f"lj/cut: |G| up to {np.abs(G).max():.3e}; worst error / bound {np.max(err / unc):.3f}; largest error {err.max():.3e}")
    assert np.abs(G[-3:]).max() > 0.05 and (err <= unc).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_mask_and_hydrostatic_strain_zero_exactly_the_rows_they_should():
    rng = np.random.default_rng(3)
    f, sig = rng.normal(0, 1, (5, 3)), rng.normal(0, 0.1, 6)
    F = np.eye(3) + rng.normal(0, 0.02, (3, 3))
    full = co.row_forces(f, sig, F, 100.0, 0.01, cell_factor=5.0)
    assert np.all(full[-3:] != 0.0)
    for k, (i, j) in enumerate(sf.VOIGT):
        m = [1] * 6
        m[k] = 0
        G = co.row_forces(f, sig, F, 100.0, 0.01, mask=m, cell_factor=5.0)
        zero = np.zeros((3, 3), bool)
        zero[i, j] = zero[j, i] = True
        assert not G[-3:][zero].any() and np.array_equal(G[-3:][~zero], full[-3:][~zero]) and np.array_equal(G[:-3], full[:-3])
    G = co.row_forces(f, sig, F, 100.0, 0.01, mask=cs.SLAB_MASK, cell_factor=5.0)
    assert not G[-1].any() and not G[-3:, 2].any() and np.all(G[-3:-1, :2] != 0.0)
    H = co.row_forces(f, sig, F, 100.0, 0.01, hydrostatic_strain=True, cell_factor=5.0)
    assert np.array_equal(H[-3:], np.eye(3) * H[-3, 0]) and abs(H[-3, 0] - np.trace(full[-3:]) / 3.0) <= 1e-14 * abs(H[-3, 0])
    assert np.array_equal(H[:-3], full[:-3])
    none = co.row_forces(f, sig, F, 100.0, 0.01, mask=[0] * 6, cell_factor=5.0)
    assert not none[-3:].any()
    for bad in ([1, 1, 1, 1, 1, 2], [0.5] * 6, [1, 1, -1, 0, 0, 0]):
        with pytest.raises(ValueError):
            co.mask33(bad)
    with pytest.raises(ValueError):
        backend.CellRelaxParams.default(mask=[1, 1, 1, 1, 1, 2])
    with pytest.raises(ValueError):
        backend.CellRelaxParams.default(mask=[1, 1, 1])


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_sw_silicon_relaxes_to_its_published_lattice_constant():
    """SW diamond Si, 8 atoms, from a = 5.60 A under hydrostatic_strain: 5.430950 A and -4.3366 eV / atom, to the digits the README
    quotes (half a unit of the last one)."""
    P = so.si_params()
    T, X, Cl = so.diamond_si(5.60)
    pbc = np.ones(3, np.uint8)
    r = co.relax_chain(co.isotropic_fd_eval(lambda x, C: so.sw(P, T, x, C, pbc)), X, Cl, pbc, so.cutoff(P), max_steps=400, fmax=1e-6,
                       hydrostatic_strain=True)
    a = r["cell"][0, 0]
    print(f"{r['n_steps']} steps, reason {r['stop_reason']}: a = {a:.7f} A (5.430950), E / atom = {r['energy'] / 8:.6f} eV (-4.3366)")
    assert r["stop_reason"] == 1 and np.array_equal(r["cell"], np.eye(3) * a)
    assert abs(a - 5.430950) < 5e-7 and abs(a - so.SI_A0) < 5e-7 and abs(r["energy"] / 8 + 4.3366) < 5e-5
    assert np.abs(r["positions"] - so.diamond_si(a)[1]).max() < 1e-9        # the atoms rode the cell


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_library_exports_them():
    header = open(os.path.join(ROOT, "include", "vssr_eval.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"int\s+vssr_batch_relax_cell\s*\(\s*vssr_handle\s*\*h,\s*const\s+vssr_cell_relax_params\s*\*p,\s*const\s+uint8_t\s*\*fixed\s*,\s*"
                     r"uint32_t\s+want,\s*double\s*\*pos_out\s*,\s*double\s*\*cell_out\s*,\s*int32_t\s*\*n_steps\s*,\s*int32_t\s*\*stop_reason\s*,\s*"
                     r"double\s*\*result\s*\)\s*;", flat)
    assert re.search(r"int\s+vssr_batch_get_cell\s*\(\s*vssr_handle\s*\*h,\s*double\s*\*cell\s*\)\s*;", flat)
    assert re.search(r"#define\s+VSSR_ABI_VERSION\s+1\b", header)
    for phrase in ("UnitCellFilter", "not pinned by\n * an executed ASE", "tests/cellrelax_oracle.py", "Out of scope", "pair handles with k-space"):
        assert phrase in header, phrase
    for name in ("vssr_batch_relax_cell", "vssr_batch_get_cell"):
        assert name in backend.EXPORTS
    lib = backend.load_library()
    assert len(lib.vssr_batch_relax_cell.argtypes) == 9 and len(lib.vssr_batch_get_cell.argtypes) == 2
    assert lib.vssr_batch_relax_cell(None, None, None, 0, None, None, None, None, None) == -1     # a null handle: the usual kind check
    assert lib.vssr_batch_get_cell(None, None) == -1
    assert set(backend.CELL_STOP_REASONS) == set(co.STOP_REASONS) == {1, 2, 3, 4}
    for name in ("PainnEngine", "TersoffEngine", "SWEngine", "EAMEngine", "PairEngine", "VashishtaEngine"):
        assert hasattr(getattr(backend, name), "relax_cell") and hasattr(getattr(backend, name), "get_cell"), name
    for calc in (calculators.EnsembleNFFSurface, calculators.NFFPourbaix, calculators.TersoffSurfCalc, calculators.PairSurfCalc,
                 calculators.EAMSurfCalc, calculators.SWSurfCalc, calculators.VashishtaSurfCalc):
        assert hasattr(calc, "relax_cell_batch"), calc.__name__


def _host_compiler():
    for name in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no C compiler for the struct probe")


def test_cell_relax_params_match_the_c_struct(tmp_path):
    """sizeof and every offsetof of vssr_cell_relax_params, from a compiled probe, against the ctypes structure."""
    src = tmp_path / "probe.c"
    lines = "\n".join(f'    printf("{f} %zu\\n", offsetof(vssr_cell_relax_params, {f}));' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vssr_eval.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(vssr_cell_relax_params));\n' + lines + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [n for n, _ in backend.CellRelaxParams._fields_] == FIELDS
    assert int(got["sizeof"]) == ctypes.sizeof(backend.CellRelaxParams) == 120
    for f in FIELDS:
        assert int(got[f]) == getattr(backend.CellRelaxParams, f).offset, f
    p = backend.CellRelaxParams.default()
    assert (p.max_steps, p.nmin, p.hydrostatic_strain, list(p.mask), p.fmax, p.scalar_pressure, p.cell_factor) == (100, 5, 0, [1] * 6, 0.05, 0.0, 0.0)
    assert (p.dt, p.maxstep, p.dtmax, p.finc, p.fdec, p.astart, p.fa) == tuple(co.FIRE_DEFAULTS[k] for k in
                                                                              ("dt", "maxstep", "dtmax", "finc", "fdec", "astart", "fa"))
    q = backend.CellRelaxParams.default(mask=cs.SLAB_MASK, hydrostatic_strain=True, scalar_pressure=0.5)
    assert list(q.mask) == list(cs.SLAB_MASK) and q.hydrostatic_strain == 1 and q.scalar_pressure == 0.5


def test_python_argument_checks_come_before_any_upload():
    def no_engine():
        raise AssertionError("the engine was touched")

    T, X, C, pbc = cs.fcc((2, 1, 1))
    a = structures.Structure(np.full(len(T), 18), X, C, pbc.astype(bool))
    good = dict(fixed_indices=None, mask=None, scalar_pressure=0.0, hydrostatic_strain=False, cell_factor=None, steps=10, fmax=0.05, want=3)

    def call(atoms_list, **over):
        return calculators._relax_cell_batch(no_engine, structures.as_arrays, atoms_list, **{**good, **over})

    nan, inf = float("nan"), float("inf")
    for over in (dict(steps=-1), dict(steps=2.5), dict(steps=True), dict(fmax=0.0), dict(fmax=nan), dict(fmax=inf), dict(scalar_pressure=nan),
                 dict(scalar_pressure=inf), dict(cell_factor=nan), dict(mask=[1, 1, 1]), dict(mask=[1, 1, 1, 1, 1, 3]), dict(mask=[0.5] * 6),
                 dict(hydrostatic_strain=2), dict(fixed_indices=[[0], [1]]), dict(fixed_indices=[[8]]), dict(fixed_indices=[[-1]])):
        with pytest.raises(ValueError):
            call([a], **over)
    with pytest.raises(ValueError):
        call([])
    with pytest.raises(AssertionError, match="engine was touched"):      # a good call gets as far as the engine
        call([a, a], fixed_indices=[[0, 1], None], mask=cs.SLAB_MASK, scalar_pressure=0.01, hydrostatic_strain=True, cell_factor=4.0)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def _lj(terms, s):
    return lambda x, C: co.pair_virial(terms, None, s[0], x, C, s[3])


def test_rehearsal_of_the_lj_cases_of_the_device_test():
    """What tests/test_cellrelax_gpu.py presumes of its lj/cut cases, under the exact pair virial: the stop reason of each, reason 4
    only on the thin cell, the compressing cube crossing the tight handle's capacity, the slab's c vector untouched."""
    assert all(8 <= len(s[0]) <= 32 for s in cs.mixed_batch() + [cs.pressure_case()[0], cs.compressing_cube(), cs.slab(), *cs.thin_case()[:2]])
    for s in cs.mixed_batch():
        r = co.relax_chain(_lj(cs.LJ, s), s[1], s[2], s[3], 6.5, max_steps=10, fmax=1e-4)
        assert (r["n_steps"], r["stop_reason"]) == (10, 2)
    s, p = cs.pressure_case()
    r = co.relax_chain(_lj(cs.LJ, s), s[1], s[2], s[3], 6.5, max_steps=400, fmax=1e-3, scalar_pressure=p)
    sig = co.pair_virial(cs.LJ, None, s[0], r["positions"], r["cell"], s[3])[2]
    F = r["F"]
    bound = 1e-3 * len(s[0]) * np.linalg.norm(F, 2) / r["volume"]
    print(f"pressure: {r['n_steps']} steps, sigma {sig}, bound {bound:.3e}")
    assert r["stop_reason"] == 1 and np.abs(sf.voigt_to_tensor(sig) + p * np.eye(3)).max() <= bound
    assert np.array_equal(co.image_counts(r["cell"], s[3], 6.5), co.image_counts(s[2], s[3], 6.5))
    s = cs.compressing_cube()
    r = co.relax_chain(_lj(cs.LJ, s), s[1], s[2], s[3], 6.5, max_steps=60, fmax=1e-3)
    d0, d1 = pc.degrees(s, 6.5), pc.degrees((s[0], r["positions"], r["cell"], s[3]), 6.5)
    assert r["stop_reason"] == 1 and d0.max() <= 56 < cs.COMPRESS_SLOTS < d1.min()
    a, b, p = cs.thin_case()
    ra = co.relax_chain(_lj(cs.LJ_THIN, a), a[1], a[2], a[3], 7.9, max_steps=cs.THIN_STEPS, fmax=1e-3, scalar_pressure=p)
    rb = co.relax_chain(_lj(cs.LJ_THIN, b), b[1], b[2], b[3], 7.9, max_steps=cs.THIN_STEPS, fmax=1e-3, scalar_pressure=p)
    assert (ra["n_steps"], ra["stop_reason"]) == (3, 4) and (rb["n_steps"], rb["stop_reason"]) == (cs.THIN_STEPS, 2)
    assert np.array_equal(co.image_counts(ra["cell"], a[3], 7.9), [1, 2, 2])
    s, held, terms, rc = cs.wall_case()
    rec = []
    r = co.relax_chain(_lj(terms, s), s[1], s[2], s[3], rc, fixed=held, max_steps=40, fmax=1e-3, record=rec)
    gap = [float(np.linalg.norm(q["positions"][8] - q["positions"][0])) for q in rec]
    assert (r["n_steps"], r["stop_reason"], len(rec)) == (3, 3, 4) and min(gap) > 0.6003 and np.isfinite(r["energy"])
    assert np.array_equal(r["cell"], rec[-1]["cell"]) and np.array_equal(r["positions"], rec[-1]["positions"])
    r = co.relax_chain(_lj(terms, s), s[1], s[2], s[3], rc, fixed=held, max_steps=cs.WALL_STEPS, fmax=1e-3)
    o = (np.ones(8, np.int32),) + cs.thin_case()[1][1:]                 # its neighbour in the device test
    ro = co.relax_chain(_lj(terms, o), o[1], o[2], o[3], rc, max_steps=cs.WALL_STEPS, fmax=1e-3)
    assert (r["n_steps"], r["stop_reason"]) == (3, 3) and (ro["n_steps"], ro["stop_reason"]) == (cs.WALL_STEPS, 2)
    s = cs.slab()
    r = co.relax_chain(_lj(cs.LJ, s), s[1], s[2], s[3], 6.5, max_steps=300, fmax=1e-3, mask=cs.SLAB_MASK)
    assert r["stop_reason"] == 1 and np.array_equal(r["cell"][2], s[2][2]) and not r["cell"][:2, 2].any()
    assert abs(r["cell"][0, 0] / 2 - cs.LJ_A0) < 0.03 and np.array_equal(r["F"][2], [0, 0, 1]) and np.array_equal(r["F"][:, 2], [0, 0, 1])


def test_restatement_stops_and_restores():
    """max_steps = 0 tests and returns; a non-finite value sends the chain back to where its step opened, bit for bit, uncounted."""
    s = cs.mixed_batch()[0]
    r = co.relax_chain(_lj(cs.LJ, s), s[1], s[2], s[3], 6.5, max_steps=0, fmax=1e-4)
    assert (r["n_steps"], r["stop_reason"]) == (0, 2) and np.array_equal(r["positions"], s[1]) and np.array_equal(r["cell"], s[2])
    rec = []
    ref = co.relax_chain(_lj(cs.LJ, s), s[1], s[2], s[3], 6.5, max_steps=3, fmax=1e-4, record=rec)
    calls = []

    def poisoned(x, C):
        calls.append(1)
        E, f, sig = co.pair_virial(cs.LJ, None, s[0], x, C, s[3])
        return (E, f, sig * np.nan) if len(calls) == 4 else (E, f, sig)
    r = co.relax_chain(poisoned, s[1], s[2], s[3], 6.5, max_steps=10, fmax=1e-4)
    assert (r["n_steps"], r["stop_reason"]) == (2, 3)
    assert np.array_equal(r["positions"], rec[2]["positions"]) and np.array_equal(r["cell"], rec[2]["cell"])
    assert ref["n_steps"] == 3 and len(rec) == 4
