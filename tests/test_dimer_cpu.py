"""The dimer restatement (tests/dimer_oracle.py) checked on its own, the front end / ABI of ``vssr_batch_dimer`` as far as they can be
checked without a GPU, and rehearsals of what tests/test_dimer_gpu.py presumes of its cases."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dimer_cases as dc
import dimer_oracle as do
import md_oracle as mo
import neb_cases as nc
from surface_sampling_amd import backend, calculators, structures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["max_steps", "max_rot_first", "max_rot", "nmin", "delta", "phi_tol", "fmax", "displace", "dt", "maxstep", "dtmax", "finc", "fdec",
          "astart", "fa", "seed"]


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_library_exports_it():
    header = open(os.path.join(ROOT, "include", "vssr_eval.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"int\s+vssr_batch_dimer\s*\(\s*vssr_handle\s*\*h,\s*const\s+vssr_dimer_params\s*\*p,\s*const\s+uint8_t\s*\*fixed\s*,\s*"
                     r"const\s+double\s*\*mode_in\s*,\s*const\s+uint64_t\s*\*dimer_id\s*,\s*uint32_t\s+want,\s*double\s*\*pos_out\s*,\s*"
                     r"double\s*\*energy\s*,\s*double\s*\*mode_out\s*,\s*double\s*\*dimer\s*,\s*int32_t\s*\*info\s*\)\s*;", flat)
    assert re.search(r"#define\s+VSSR_ABI_VERSION\s+1\b", header)
    for phrase in ("NOT ASE's MinModeTranslate", "not pinned by any executed library", "tests/dimer_oracle.py", "Out of scope"):
        assert phrase in header, phrase
    assert "vssr_batch_dimer" in backend.EXPORTS
    fn = backend.load_library().vssr_batch_dimer
    assert fn.argtypes is not None and len(fn.argtypes) == 11
    assert fn(None, None, None, None, None, 0, None, None, None, None, None) == -1     # a null handle: the usual kind check
    assert set(backend.DIMER_STOP_REASONS) == set(do.STOP_REASONS) == {1, 2, 3}
    for name in ("PainnEngine", "TersoffEngine", "SWEngine", "EAMEngine", "PairEngine", "VashishtaEngine"):
        assert hasattr(getattr(backend, name), "dimer"), name
    for calc in (calculators.EnsembleNFFSurface, calculators.NFFPourbaix, calculators.TersoffSurfCalc, calculators.PairSurfCalc,
                 calculators.EAMSurfCalc):
        assert hasattr(calc, "dimer_batch"), calc.__name__


def _host_compiler():
    for name in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no C compiler for the struct probe")


def test_dimer_params_match_the_c_struct(tmp_path):
    """sizeof and every offsetof of vssr_dimer_params, from a compiled probe, against the ctypes structure."""
    src = tmp_path / "probe.c"
    lines = "\n".join(f'    printf("{f} %zu\\n", offsetof(vssr_dimer_params, {f}));' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vssr_eval.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(vssr_dimer_params));\n' + lines + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [n for n, _ in backend.DimerParams._fields_] == FIELDS
    assert int(got["sizeof"]) == ctypes.sizeof(backend.DimerParams) == 112
    for f in FIELDS:
        assert int(got[f]) == getattr(backend.DimerParams, f).offset, f
    p = backend.DimerParams.default()
    assert (p.max_steps, p.max_rot_first, p.max_rot, p.nmin, p.delta, p.fmax, p.displace, p.seed) == (100, 8, 1, 5, 0.01, 0.05, 0.0, 0)
    assert p.phi_tol == np.pi / 180.0
    assert (p.dt, p.maxstep, p.dtmax, p.finc, p.fdec, p.astart, p.fa) == tuple(do.FIRE_DEFAULTS[k] for k in
                                                                              ("dt", "maxstep", "dtmax", "finc", "fdec", "astart", "fa"))
    assert backend.DimerParams.default(seed=2 ** 64 - 1).seed == 2 ** 64 - 1
    for bad in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError):
            backend.DimerParams.default(seed=bad)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _atoms(struct):
    T, X, cell, pbc = struct
    return structures.Structure(np.full(len(T), 29), X, cell, pbc.astype(bool))


def test_python_argument_checks_come_before_any_upload():
    def no_engine():
        raise AssertionError("the engine was touched")

    a = _atoms(nc.anchor_image(*dc.ANCHOR_START))
    good = dict(modes=None, fixed_indices=None, n_starts=1, seed=0, steps=10, fmax=0.05, delta=0.01, phi_tol=np.pi / 180.0, max_rot_first=8,
                max_rot=1, displace=0.0, want=3)

    def call(atoms_list, **over):
        return calculators._dimer_batch(no_engine, structures.as_arrays, atoms_list, **{**good, **over})

    nan, inf = float("nan"), float("inf")
    for over in (dict(n_starts=0), dict(n_starts=1.5), dict(n_starts=True), dict(seed=-1), dict(seed=0.5), dict(steps=-1), dict(steps=2.5),
                 dict(fmax=0.0), dict(fmax=nan), dict(delta=0.0), dict(delta=inf), dict(phi_tol=0.0), dict(phi_tol=1.0), dict(phi_tol=nan),
                 dict(max_rot_first=-1), dict(max_rot=-1), dict(max_rot=0.5), dict(displace=nan), dict(displace=inf),
                 dict(fixed_indices=[[0], [1]]), dict(fixed_indices=[[7]]), dict(fixed_indices=[[0, 1, 2, 3]]),
                 dict(modes=[np.zeros((3, 3))]), dict(modes=[np.zeros((4, 3))]), dict(modes=[np.ones((4, 3)), np.ones((4, 3))]),
                 dict(modes=[np.full((4, 3), nan)]), dict(modes=[np.ones((4, 3))], n_starts=2),
                 dict(modes=[np.ones((4, 3)) * [[1], [1], [1], [0]]], fixed_indices=[[0, 1, 2]])):
        with pytest.raises(ValueError):
            call([a], **over)
    with pytest.raises(ValueError):
        call([])
    with pytest.raises(AssertionError, match="engine was touched"):      # a good call gets as far as the engine
        call([a, a], fixed_indices=[[0, 1, 2], None], n_starts=3)
    with pytest.raises(AssertionError, match="engine was touched"):
        call([a], modes=[np.ones((4, 3))], fixed_indices=[[0, 1, 2]])


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_drawn_modes_restate_the_md_generator_under_a_tag_of_their_own():
    """Tag 2 at draw index 0 (MD draws use tags 0 and 1), keyed by (seed, dimer id); unit length over the free atoms, zero on held ones."""
    assert do.TAG_DIMER not in (mo.TAG_MAXWELL, mo.TAG_LANGEVIN)
    z = do.draw_modes(5, [3, 9], [4, 4])
    keys = mo.chain_keys(5, [3, 9])
    for g in range(2):
        assert np.array_equal(z[g], mo.normals3(np.broadcast_to(keys[g], (4, 2)), 0, np.arange(4), 2))
    assert not np.array_equal(z[0], z[1])
    assert not np.array_equal(z[0], mo.normals3(np.broadcast_to(keys[0], (4, 2)), 0, np.arange(4), mo.TAG_MAXWELL))
    c = dc.anchor_case(5, 0, 0, max_steps=0)
    r = dc.run_case(c, dimer_id=[3])
    assert np.array_equal(r["modes"][3], z[0][3] / np.sqrt(np.vdot(z[0][3], z[0][3]))) and not r["modes"][:3].any() and not r["modes"][4:].any()
    assert r["n_steps"][0] == 0 and r["stop_reason"][0] == 2 and r["n_eval"][0] == 1 and r["n_rot"][0] == 0
    # displace moves the midpoint along the mode before the first evaluation, the end follows
    d = dc.run_case(c, dimer_id=[3], displace=0.25)
    assert np.array_equal(d["positions"][3], c.struct[1][3] + 0.25 * r["modes"][3])
    assert np.array_equal(d["positions"][7], d["positions"][3] + 0.01 * r["modes"][3]) and np.array_equal(d["positions"][:3], c.struct[1][:3])


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_closed_form_saddle_on_the_restatement():
    """One lj/cut atom above the held triangle of neb_cases, started at centre + (0.10, -0.05, 0.40) A: six drawn modes under three
    rotation settings all reach the closed-form saddle 3 (LJ(R) + eps) = 1.7360211026532 eV above the minimum.  E0 is the energy of the
    whole structure: the three held-held pairs of the triangle, which the closed form does not count, are taken off."""
    assert abs(nc.ANCHOR_BARRIER - 1.7360211026532) < 1e-12
    H = nc.anchor_saddle_hessian()
    lam = np.linalg.eigvalsh(H)
    assert (lam < 0).sum() == 1
    bound = nc.barrier_bound(dc.ANCHOR["fmax"], H)
    etri = dc.triangle_energy()
    worst_e, worst_c, steps, evals = 0.0, 0.0, [], []
    for c in dc.anchor_cases():
        r = dc.run_case(c)
        err = r["e0"][0] - etri + 3.0 * nc.ANCHOR_EPS - nc.ANCHOR_BARRIER
        N, C = r["modes"][3], r["curvature"][0]
        c_bound = dc.anchor_curvature_bound(N, r["positions"][3] - nc.ANCHOR_CENTRE, H, dc.ANCHOR["delta"], dc.ANCHOR["fmax"])
        print(f"{c.name}: {r['n_steps'][0]} steps, {r['n_rot'][0]} rotations, {r['n_eval'][0]} evaluations, saddle energy error {err:+.3e} eV "
              f"(bound {bound:.3e}), C {C:.6f} - lambda {lam[0]:.6f} = {C - lam[0]:+.3e} (bound {c_bound:.3e}), |N.z| {abs(N[2]):.7f}")
        assert r["stop_reason"][0] == 1 and r["n_steps"][0] <= 200, c.name
        assert abs(err) <= bound, c.name
        assert C < 0.0 and abs(N[2]) > 0.999 and abs(C - lam[0]) <= c_bound, c.name
        assert r["fmax"][0] < dc.ANCHOR["fmax"] and abs(np.vdot(N, N) - 1.0) < 1e-14
        worst_e, worst_c = max(worst_e, abs(err)), max(worst_c, abs(C - lam[0]))
        steps.append(int(r["n_steps"][0]))
        evals.append(int(r["n_eval"][0]))
    print(f"18 runs: {min(steps)} .. {max(steps)} steps, {min(evals)} .. {max(evals)} evaluations, worst |energy error| {worst_e:.3e} eV, "
          f"worst |C - lambda| {worst_c:.3e} eV / A^2")


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_visit_every_branch():
    seen, margins = dc.census()
    for b, names in seen.items():
        print(f"{b:22s} {sorted(names)}")
    missing = [b for b in dc.REQUIRED if not seen[b]]
    assert not missing, missing
    assert set(dc.REQUIRED) <= set(do.BRANCHES)
    # the non-finite value shows at an evaluation R and not only at E, and the clamp binds
    assert seen["reason3_at_R"] == {"wall_at_R"} and "wall_at_E" in seen["reason3_at_E"]
    rec = []
    dc.run_case({c.name: c for c in dc.census_cases()}["anchor_s1_r81"], record=rec)
    assert any("clip" in r["branches"] and r["margins"]["maxstep"] > 0.1 for r in rec)
    # the tie of the line case is exact: f = 0 to the bit
    r = dc.run_case(dc.line_case())
    assert r["f_perp"][0] == 0.0 and r["n_rot"][0] == 0 and r["curvature"][0] > 0.0 and r["stop_reason"][0] == 2
    # every comparison the device test repeats on these cases stands off by more than an ulp of trigonometry could move it
    for name, m in margins.items():
        print(f"{name:18s} {({k: float(f'{v:.2e}') for k, v in m.items()})}")
        assert min(m.values()) >= dc.MARGIN, (name, m)


@pytest.mark.parametrize("kind", dc.PARITY_KINDS)
def test_margins_of_the_parity_cases(kind, golden, oracle_mod):
    """Every comparison (phi1 against phi_tol, Cm against C, C against 0, fmax, FIRE's power against 0, the maxstep clamp) of every
    parity case of tests/test_dimer_gpu.py stands off by a relative margin of at least 1e-6 under the CPU restatements of the
    potentials: an ulp between device and numpy trigonometry cannot flip a branch."""
    fn = dc.cpu_force_fn(kind, golden, oracle_mod)
    structs, held = dc.parity_batch(kind)
    rec = []
    r = do.run(fn(structs), np.vstack([s[1] for s in structs]), dc.start_of(structs), fixed=held, record=rec, **dc.PARITY)
    m = dc.smallest_margins(rec)
    print(f"{kind:10s} steps {r['n_steps']}, rotations {r['n_rot']}, evaluations {r['n_eval']}, margins {({k: float(f'{v:.2e}') for k, v in m.items()})}")
    assert list(r["n_steps"]) == [10] * 3 and list(r["stop_reason"]) == [2] * 3 and r["n_rot"].min() >= 1, kind
    assert min(m.values()) >= dc.MARGIN, (kind, m)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_stops_and_restores():
    """max_steps = 0 tests and returns; the wall cases give x0 and N back bit for bit with 0 steps counted and reason 3."""
    c = dc.anchor_case(0, 8, 1)
    x = c.struct[1]
    r = dc.run_case(c, max_steps=0)
    assert r["n_steps"][0] == 0 and r["stop_reason"][0] == 2 and np.array_equal(r["positions"][:4], x) and r["n_rot"][0] >= 1
    assert np.array_equal(r["positions"][4:], x + 0.01 * r["modes"][:4])
    for case, n_eval, where in ((dc.wall_case_E(), 2, "reason3_at_E"), (dc.wall_case_R(), 3, "reason3_at_R")):
        structs, held, modes = dc.pack([case])
        fn = dc.pair_batch_fn(structs, case.terms)
        x0 = np.vstack([s[1] for s in structs])
        e0, f0 = fn(x0)
        assert np.isfinite(e0).all() and np.isfinite(f0).all()
        rec = []
        r = dc.run_case(case, record=rec)
        N0 = case.mode / np.sqrt(np.vdot(case.mode, case.mode))
        assert (r["n_steps"][0], r["stop_reason"][0], r["n_eval"][0]) == (0, 3, n_eval), case.name
        assert np.array_equal(r["positions"][:3], case.struct[1]) and np.array_equal(r["modes"][:3], N0), case.name
        assert np.array_equal(r["positions"][3:], case.struct[1] + 0.01 * N0) and np.isfinite(r["energies"]).all()
        assert where in rec[-1]["branches"] and any("clip" in x["branches"] for x in rec)
        moved = [x for x in rec if "first" in x["branches"]]
        assert len(moved) == 1 and moved[0]["steps"] == 1                      # a step was taken, and taken back
    with pytest.raises(ValueError):
        dc.run_case(dc.line_case()._replace(mode=np.zeros((3, 3))))
