"""The nudged-elastic-band restatement (tests/neb_oracle.py) checked on its own, the front end / ABI of ``vssr_batch_neb`` as far as
they can be checked without a GPU, and rehearsals of what tests/test_neb_gpu.py presumes of its cases."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import neb_cases as nc
import neb_oracle as no
from surface_sampling_amd import backend, calculators, structures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["max_steps", "method", "climb", "k", "fmax", "dt", "maxstep", "dtmax", "finc", "fdec", "astart", "fa", "nmin"]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_library_exports_it():
    header = open(os.path.join(ROOT, "include", "vssr_eval.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"enum\s*\{\s*VSSR_NEB_IMPROVED_TANGENT\s*=\s*0,\s*VSSR_NEB_ASENEB\s*=\s*1\s*\}\s*;", flat)
    assert re.search(r"int\s+vssr_batch_neb\s*\(\s*vssr_handle\s*\*h,\s*const\s+vssr_neb_params\s*\*p,\s*const\s+uint8_t\s*\*fixed\s*,\s*"
                     r"const\s+int32_t\s*\*n_img\s*,\s*int32_t\s+n_bands,\s*uint32_t\s+want,\s*double\s*\*pos_out\s*,\s*double\s*\*energy\s*,\s*"
                     r"double\s*\*neb_force\s*,\s*double\s*\*band\s*,\s*int32_t\s*\*info\s*\)\s*;", flat)
    assert re.search(r"#define\s+VSSR_ABI_VERSION\s+1\b", header)
    assert "vssr_batch_neb" in backend.EXPORTS
    fn = backend.load_library().vssr_batch_neb
    assert fn.argtypes is not None and len(fn.argtypes) == 11
    assert fn(None, None, None, None, 0, 0, None, None, None, None, None) == -1     # a null handle: the usual kind check
    assert backend.NEB_METHODS == {"improvedtangent": 0, "aseneb": 1} and set(backend.NEB_STOP_REASONS) == {1, 2, 3, 4}
    assert set(backend.NEB_STOP_REASONS) == set(no.STOP_REASONS)
    for name in ("PainnEngine", "TersoffEngine", "SWEngine", "EAMEngine", "PairEngine", "VashishtaEngine"):
        assert hasattr(getattr(backend, name), "neb"), name
    for calc in (calculators.EnsembleNFFSurface, calculators.NFFPourbaix, calculators.TersoffSurfCalc, calculators.PairSurfCalc,
                 calculators.EAMSurfCalc):
        assert hasattr(calc, "neb_batch"), calc.__name__


def _host_compiler():
    for name in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no C compiler for the struct probe")


def test_neb_params_match_the_c_struct(tmp_path):
    """sizeof and every offsetof of vssr_neb_params, from a compiled probe, against the ctypes structure."""
    src = tmp_path / "probe.c"
    lines = "\n".join(f'    printf("{f} %zu\\n", offsetof(vssr_neb_params, {f}));' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vssr_eval.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(vssr_neb_params));\n' + lines + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [n for n, _ in backend.NebParams._fields_] == FIELDS
    assert int(got["sizeof"]) == ctypes.sizeof(backend.NebParams) == 96
    for f in FIELDS:
        assert int(got[f]) == getattr(backend.NebParams, f).offset, f
    p = backend.NebParams.default()
    assert (p.max_steps, p.method, p.climb, p.k, p.fmax, p.nmin) == (100, 0, 0, 0.1, 0.05, 5)
    assert (p.dt, p.maxstep, p.dtmax, p.finc, p.fdec, p.astart, p.fa) == tuple(no.FIRE_DEFAULTS[k] for k in
                                                                              ("dt", "maxstep", "dtmax", "finc", "fdec", "astart", "fa"))


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _atoms(struct):
    T, X, cell, pbc = struct
    return structures.Structure(np.full(len(T), 29), X, cell, pbc.astype(bool))


def test_python_argument_checks_come_before_any_upload():
    def no_engine():
        raise AssertionError("the engine was touched")

    band = [_atoms(s) for s in nc.anchor_band(4)]
    good = dict(fixed_indices=None, k=0.1, climb=False, method="improvedtangent", fmax=0.05, steps=10, two_stage=False, want=3)

    def call(bands, **over):
        return calculators._neb_batch(no_engine, structures.as_arrays, bands, **{**good, **over})

    for over in (dict(method="eb"), dict(method=0), dict(k=0.0), dict(k=float("nan")), dict(fmax=-1.0), dict(fmax=float("inf")),
                 dict(steps=-1), dict(steps=2.5), dict(climb="yes"), dict(two_stage=2), dict(fixed_indices=[[0], [1]]),
                 dict(fixed_indices=[[7]])):
        with pytest.raises(ValueError):
            call([band], **over)
    other = band[2].copy()
    other.numbers = other.numbers.copy()
    other.numbers[0] = 47
    moved_cell = band[2].copy()
    moved_cell.cell = moved_cell.cell * 1.01
    for bands in ([], [band[:2]], [(band[0], band[-1])], [(band[0], band[-1], 2)], [[band[0], other, band[-1]]], [[band[0], moved_cell, band[-1]]],
                  [[band[0], band[1], structures.Structure([29], [[0, 0, 0]], nc.BOX)]]):
        with pytest.raises(ValueError):
            call(bands)
    with pytest.raises(AssertionError, match="engine was touched"):      # a good call gets as far as the engine
        call([band, (band[0], band[-1], 5)], fixed_indices=[[0, 1, 2], None])
    for bad in ("eb", None, 1):
        with pytest.raises(ValueError):
            backend.neb_method_code(bad)
    with pytest.raises(ValueError):
        backend.NebParams.default(climb=2)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def _brute_mic(d, cell, pbc):
    """The shortest of the 27 neighbouring images of every displacement."""
    best = None
    for n in itertools.product((-1, 0, 1), repeat=3):
        if any(n[a] and not pbc[a] for a in range(3)):
            continue
        c = d + np.asarray(n, float) @ cell
        l = (c * c).sum(axis=1)
        if best is None:
            best, bl = c.copy(), l.copy()
        else:
            m = l < bl
            best[m], bl[m] = c[m], l[m]
    return best


@pytest.mark.parametrize("cell", [np.diag([7.0, 8.0, 9.0]), np.array([[7.0, 0.0, 0.0], [2.1, 7.5, 0.0], [-1.3, 1.7, 9.0]])],
                         ids=["orthorhombic", "skewed"])
def test_interpolate_band_and_band_path_against_the_27_image_minimum(cell):
    rng = np.random.default_rng(3)
    pbc = np.array([True, True, False])
    frac = rng.uniform(0.1, 0.9, (6, 3))
    frac[0] = [0.97, 0.5, 0.5]                           # this atom crosses the periodic face a = 1 between the end images
    x0 = frac @ cell
    d = rng.normal(0, 0.3, (6, 3))
    d[0] = 0.08 * cell[0]
    x1 = x0 + d
    x1[0] -= cell[0]                                     # ... and the final structure holds it wrapped back into the cell
    x1[3] += cell[2]                                     # a whole vector along the open axis is a real displacement
    d[3] += cell[2]
    a, b = (structures.Structure(np.full(6, 29), x, cell, pbc) for x in (x0, x1))
    assert np.abs((x1 - x0)[0]).max() > 3.0
    imgs = structures.interpolate_band(a, b, 5)
    assert len(imgs) == 5 and np.array_equal(imgs[0].positions, x0)
    want = _brute_mic(x1 - x0, cell, pbc)
    assert np.abs(want - d).max() < 1e-12
    for i, img in enumerate(imgs):
        assert np.abs(img.positions - (x0 + want * i / 4)).max() < 1e-12
        assert np.array_equal(img.cell, cell) and np.array_equal(img.pbc, pbc) and np.array_equal(img.numbers, a.numbers)
    raw = structures.interpolate_band(a, b, 5, mic=False)
    assert np.abs(raw[-1].positions - x1).max() < 1e-12 and np.abs(raw[2].positions[0] - imgs[2].positions[0]).max() > 3.0
    # the reaction coordinate of a band whose middle image sits across the face
    band = np.array([x0, x0 + 0.4 * want, x0 + want])
    band[1, 0] -= cell[0]
    path = structures.band_path(band, cell, pbc)
    step = [np.sqrt((_brute_mic(band[i + 1] - band[i], cell, pbc) ** 2).sum()) for i in range(2)]
    assert path[0] == 0.0 and np.abs(path[1:] - np.cumsum(step)).max() < 1e-12
    assert abs(path[2] - np.sqrt((want ** 2).sum())) < 1e-12
    assert np.abs(no.path(band, cell, pbc) - path).max() == 0.0 and np.abs(no.mic(x1 - x0, cell, pbc) - want).max() < 1e-12
    with pytest.raises(ValueError):
        structures.interpolate_band(a, b, 2)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_physics_anchor_on_the_restatement():
    """One lj/cut atom through a fixed triangle: the closed-form barrier 3 (LJ(R) + eps) = 1.7360211026532 eV."""
    assert abs(nc.ANCHOR_BARRIER - 1.7360211026532) < 1e-12 and abs(nc.ANCHOR_ZMIN - 1.2098483400758) < 1e-7
    H = nc.anchor_saddle_hessian()
    lam = np.linalg.eigvalsh(H)
    bound = nc.barrier_bound(nc.ANCHOR["fmax"], H)
    assert (lam < 0).sum() == 1                          # a first-order saddle
    cases = {c.name: c for c in nc.census_cases()}
    plain5 = nc.run_case(nc.Case("anchor5_plain", nc.anchor_band(5), nc.ANCHOR_HELD, dict(nc.ANCHOR, climb=False, method="improvedtangent")))
    plain6 = nc.run_case(cases["anchor6_plain_improved"])
    climb_it = nc.run_case(cases["anchor6_climb_improved"])
    climb_ase = nc.run_case(cases["anchor6_climb_aseneb"])
    for name, r in (("5 images", plain5), ("6 images", plain6), ("6 images climbing, improved tangent", climb_it),
                    ("6 images climbing, aseneb", climb_ase)):
        err = r["barrier_forward"][0] - nc.ANCHOR_BARRIER
        print(f"{name}: {r['n_steps'][0]} steps, reason {r['stop_reason'][0]}, barrier error {err:+.3e} eV (bound {bound:.3e}), "
              f"forward - reverse {r['barrier_forward'][0] - r['barrier_reverse'][0]:+.1e}")
        assert r["stop_reason"][0] == 1 and r["n_steps"][0] <= 200, name
    # an odd band puts its middle image into the plane by symmetry, an even one straddles it
    assert abs(plain5["positions"][4 * 2 + 3, 2] - nc.ANCHOR_CENTRE[2]) < 1e-6 and abs(plain5["barrier_forward"][0] - nc.ANCHOR_BARRIER) < bound
    assert nc.ANCHOR_BARRIER - plain6["barrier_forward"][0] > 0.1
    for r in (climb_it, climb_ase):
        assert abs(r["barrier_forward"][0] - nc.ANCHOR_BARRIER) <= bound
        assert r["imax"][0] in (2, 3) and r["fmax"][0] < nc.ANCHOR["fmax"]
    assert (climb_it["n_steps"][0], climb_ase["n_steps"][0]) == (89, 87)      # the rehearsal the issue quotes


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_visit_every_branch():
    seen = nc.census()
    for b, names in seen.items():
        print(f"{b:26s} {sorted(names)}")
    missing = [b for b in nc.REQUIRED if not seen[b]]
    assert not missing, missing
    assert set(nc.REQUIRED) <= set(no.BRANCHES)
    # the band-norm clamp binds while no image alone would be clamped, and the tie is an exact one
    rec = []
    nc.run_case({c.name: c for c in nc.census_cases()}["bowed9"], record=rec)
    assert any("clip_band_only" in r["branches"] and r["normdr_rel"] > 1.0 for r in rec)


def test_restatement_stops():
    """max_steps = 0 tests and returns; a band at rest converges at once; coincident images stop with reason 4; ends never move."""
    c = nc.census_cases()[0]
    x0 = np.vstack([s[1] for s in c.band])
    r = nc.run_case(c, max_steps=0)
    assert r["n_steps"][0] == 0 and r["stop_reason"][0] == 2 and np.array_equal(r["positions"], x0) and np.abs(r["neb_forces"]).max() > 0.01
    for method in no.METHODS:      # every image at one minimum: all tangents have zero length, and the band has converged as it stands
        rest = nc.Case("rest", [nc.anchor_image(0.0, 0.0, nc.ANCHOR_ZMIN)] * 3, nc.ANCHOR_HELD, dict(nc.ANCHOR, method=method))
        r = nc.run_case(rest)
        assert r["stop_reason"][0] == 1 and r["n_steps"][0] == 0 and r["fmax"][0] < 1e-6
    twin = nc.Case("twin", [c.band[0], c.band[2], c.band[2], c.band[5]], nc.ANCHOR_HELD, dict(nc.ANCHOR, method="improvedtangent"))
    r = nc.run_case(twin)
    assert r["stop_reason"][0] == 4 and r["n_steps"][0] == 0
    full = nc.run_case(c)
    assert np.array_equal(full["positions"][:4], x0[:4]) and np.array_equal(full["positions"][-4:], x0[-4:])
    held = np.tile(nc.ANCHOR_HELD.astype(bool), 6)
    assert np.array_equal(full["positions"][held], x0[held]) and np.abs(full["positions"] - x0).max() > 0.05


def test_a_band_that_runs_into_the_wall_goes_back_to_where_its_step_opened():
    """Rehearsal of the device test: finite at the start, non-finite after the first (clamped) step, back at the input with 0 steps."""
    band = nc.wall_band()
    c = nc.Case("wall", band, nc.WALL_HELD, dict(k=0.1, fmax=0.01, max_steps=12, climb=False, method="improvedtangent"))
    fn = nc.wall_batch_fn(band)
    x0 = np.vstack([s[1] for s in band])
    e0, f0 = fn(x0)
    assert np.isfinite(e0).all() and np.isfinite(f0).all() and abs(f0[4, 0] - 36.1) < 0.1
    rec = []
    r = nc.run_case(c, force_fn=fn, record=rec)
    assert (r["n_steps"][0], r["stop_reason"][0], r["n_eval"]) == (0, 3, 2) and np.array_equal(r["positions"], x0)
    assert "clip" in rec[0]["branches"] and np.array_equal(r["energies"], e0)
    moved = x0.copy()
    moved[4, 0] += 0.2
    assert not np.isfinite(fn(moved)[1]).all()
