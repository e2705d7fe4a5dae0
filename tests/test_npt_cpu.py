"""The constant-pressure MD restatement (tests/npt_oracle.py) checked on its own against closed forms, and the front end / ABI of
vssr_batch_md_npt as far as they can be checked without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import md_oracle as mo
import npt_oracle as no
from surface_sampling_amd import backend, calculators, structures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["n_steps", "thermostat", "barostat", "coupling", "thermo_interval", "mask", "dt", "temperature", "temperature_end", "friction", "taut",
          "taup", "pressure", "compressibility", "ramp_steps", "step0", "seed"]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_exports_list_it():
    header = open(os.path.join(ROOT, "include", "vssr_eval.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"enum\s*\{\s*VSSR_NPT_THERMOSTAT_NONE\s*=\s*0,\s*VSSR_NPT_THERMOSTAT_LANGEVIN\s*=\s*1,\s*VSSR_NPT_THERMOSTAT_BERENDSEN\s*=\s*2\s*\}\s*;", flat)
    assert re.search(r"enum\s*\{\s*VSSR_NPT_BAROSTAT_NONE\s*=\s*0,\s*VSSR_NPT_BAROSTAT_BERENDSEN\s*=\s*1,\s*VSSR_NPT_BAROSTAT_CRESCALE\s*=\s*2\s*\}\s*;", flat)
    assert re.search(r"enum\s*\{\s*VSSR_NPT_COUPLING_ISOTROPIC\s*=\s*0,\s*VSSR_NPT_COUPLING_PER_AXIS\s*=\s*1\s*\}\s*;", flat)
    assert re.search(r"int\s+vssr_batch_md_npt\s*\(\s*vssr_handle\s*\*h,\s*const\s+vssr_npt_params\s*\*p,\s*const\s+double\s*\*mass\s*,\s*const\s+uint8_t\s*"
                     r"\*fixed\s*,\s*const\s+uint64_t\s*\*chain_id\s*,\s*uint32_t\s+want,\s*double\s*\*pos_out\s*,\s*double\s*\*cell_out\s*,\s*"
                     r"double\s*\*thermo\s*,\s*int32_t\s*\*n_done,\s*int32_t\s*\*stop_reason\s*\)\s*;", flat)
    assert re.search(r"#define\s+VSSR_ABI_VERSION\s+1\b", header)          # additive: the version stays
    for phrase in ("NVTBerendsen", "Inhomogeneous_NPTBerendsen", "Bernetti & Bussi", "not pinned by an executed library", "tests/npt_oracle.py",
                   "LOCK STEP ONLY", "vssr_batch_md_driver(RESIDENT) does not apply", "draw tag 3", "forces are NOT recomputed"):
        assert phrase in header, phrase
    assert "vssr_batch_md_npt" in backend.EXPORTS
    fn = backend.load_library().vssr_batch_md_npt
    assert fn.argtypes is not None and len(fn.argtypes) == 11
    assert fn(None, None, None, None, None, 0, None, None, None, None, None) == -1     # a null handle: the usual kind check
    assert backend.NPT_THERMOSTATS == {"none": 0, "langevin": 1, "berendsen": 2} and tuple(backend.NPT_THERMOSTATS) == no.THERMOSTATS
    assert backend.NPT_BAROSTATS == {"none": 0, "berendsen": 1, "crescale": 2} and tuple(backend.NPT_BAROSTATS) == no.BAROSTATS
    assert backend.NPT_COUPLINGS == {"isotropic": 0, "per_axis": 1} and tuple(backend.NPT_COUPLINGS) == no.COUPLINGS
    assert set(backend.NPT_STOP_REASONS) == set(no.STOP_REASONS) == {1, 2, 3}
    for name in ("PainnEngine", "TersoffEngine", "SWEngine", "EAMEngine", "PairEngine", "VashishtaEngine"):
        assert hasattr(getattr(backend, name), "npt"), name
    for calc in (calculators.EnsembleNFFSurface, calculators.TersoffSurfCalc, calculators.PairSurfCalc):
        assert hasattr(calc, "npt_batch") and hasattr(calc, "md_batch"), calc.__name__
    # the contract's tags: the cell noise has a tag of its own
    src = open(os.path.join(ROOT, "surface-sampling_amd", "csrc", "md_npt.hip")).read()
    assert re.search(r"NPT_TAG_CRESCALE\s*=\s*3\b", src) and no.TAG_CRESCALE == 3 and mo.TAG_LANGEVIN == 1


def _host_compiler():
    for name in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no C compiler for the struct probe")


def test_npt_params_match_the_c_struct(tmp_path):
    """sizeof and every offsetof of vssr_npt_params, from a compiled probe, against the ctypes structure."""
    src = tmp_path / "probe.c"
    lines = "\n".join(f'    printf("{f} %zu\\n", offsetof(vssr_npt_params, {f}));' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vssr_eval.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(vssr_npt_params));\n' + lines + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call([_host_compiler(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [n for n, _ in backend.NptParams._fields_] == FIELDS
    assert int(got["sizeof"]) == ctypes.sizeof(backend.NptParams) == 120
    for f in FIELDS:
        assert int(got[f]) == getattr(backend.NptParams, f).offset, f
    p = backend.npt_params(7, 0.5, thermostat="berendsen", barostat="crescale", temperature=100.0, temperature_end=200.0, mask=(1, 0, 1), seed=-1)
    assert (p.n_steps, p.thermostat, p.barostat, p.coupling, p.thermo_interval, list(p.mask)) == (7, 2, 2, 0, 1, [1, 0, 1])
    assert (p.dt, p.temperature, p.temperature_end, p.ramp_steps, p.step0, p.seed) == (0.5, 100.0, 200.0, 7, 0, 2 ** 64 - 1)
    assert backend.npt_params(7, 0.5, temperature=100.0).temperature_end == 100.0 and list(backend.npt_params(1, 1.0).mask) == [1, 1, 1]


def test_python_side_argument_checks_come_before_any_device_call():
    for kw, match in ((dict(thermostat="nose"), "thermostat"), (dict(barostat="mtk"), "barostat"), (dict(coupling="full"), "coupling"),
                      (dict(thermostat=1), "thermostat"), (dict(mask=(1, 1)), "mask"), (dict(mask=(1, 2, 0)), "mask")):
        with pytest.raises(ValueError, match=match):
            backend.npt_params(10, 1.0, **kw)
    s = structures.Structure([31, 7], np.array([[0, 0, 0], [0, 0, 1.9]], float), np.eye(3) * 10)

    def no_engine():
        raise AssertionError("the engine was asked for before the arguments were checked")

    for calc in (calculators.TersoffSurfCalc.__new__(calculators.TersoffSurfCalc), calculators.EnsembleNFFSurface.__new__(calculators.EnsembleNFFSurface)):
        calc.parameters, calc.results, calc.atoms = {}, {}, None
        calc.species, calc.all_periodic = ["Ga", "N"], True
        calc._get_engine = no_engine
        for kw, match in ((dict(thermostat="nose"), "thermostat"), (dict(barostat="mtk"), "barostat"), (dict(coupling="full"), "coupling"),
                          (dict(steps=-1), "steps"), (dict(timestep=0.0), "timestep"), (dict(timestep=float("nan")), "timestep"),
                          (dict(thermo_interval=0), "thermo_interval"), (dict(thermostat="langevin", friction=0.0), "friction"),
                          (dict(temperature=-1.0), "temperature"), (dict(temperature_end=-1.0), "temperature"), (dict(taut=0.0), "taut"),
                          (dict(taup=0.0), "taup"), (dict(compressibility=-1.0), "compressibility"), (dict(pressure=float("inf")), "finite"),
                          (dict(mask=(0, 0, 0)), "empty mask"), (dict(mask=(1, 1, 2)), "mask"),
                          (dict(barostat="crescale", thermostat="none"), "stochastic"), (dict(barostat="crescale", coupling="per_axis"), "stochastic"),
                          (dict(barostat="crescale", mask=(1, 1, 0)), "stochastic"), (dict(masses=[[1.0, 2.0], [1.0]]), "mass arrays"),
                          (dict(masses=[[1.0, -2.0]]), "masses"), (dict(velocities=[]), "velocity arrays"), (dict(fixed_indices=[]), "index lists")):
            with pytest.raises(ValueError, match=match):
                calc.npt_batch([s], **kw)
        with pytest.raises(ValueError, match="no structures"):
            calc.npt_batch([])


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------------
def _free_gas(n=20, seed=1, T=500.0):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 30.0, (n, 3))
    mass = np.where(np.arange(n) % 2 == 0, 39.948, 83.798)
    vel = mo.maxwell_boltzmann(mass, [0, n], T, seed=seed)
    return pos, vel, mass


def _none(pos, cells):
    return np.zeros(len(cells)), np.zeros_like(pos), None


def test_berendsen_thermostat_on_free_particles_follows_its_recurrence():
    """No forces: the kinetic temperature after every step is T (1 + (dt / taut)(T0 / T - 1)) of the one before, to rounding (the clamp
    of lambda to [0.9, 1.1] is not reached); a held atom stays out of N_free."""
    pos, vel, mass = _free_gas()
    fixed = np.zeros(20, np.uint8)
    fixed[3] = 1
    T0, dt, taut, n = 300.0, 2.0, 50.0, 40
    r = no.run(pos, vel, np.eye(3) * 30.0, [0, 0, 0], mass, [0, 20], _none, n_steps=n, dt=dt, cutoff=5.0, thermostat="berendsen", temperature=T0,
               taut=taut, fixed=fixed)
    T = 2.0 * r["ekin"][:, 0] / (3.0 * 19 * no.KB)
    want = [T[0]]
    for _ in range(n):
        want.append(want[-1] * (1.0 + (dt / taut) * (T0 / want[-1] - 1.0)))
    err = np.abs(T - np.array(want)).max() / T0
    print(f"Berendsen thermostat: T {T[0]:.2f} -> {T[-1]:.2f} K, max relative deviation from the recurrence {err:.2e}")
    assert err < 1e-13 and abs(T[-1] - T0) < abs(T[0] - T0) * (1 - dt / taut) ** n * 1.01
    assert np.isnan(r["pressure"]).all() and np.array_equal(r["volume"][:, 0], np.full(n + 1, 27000.0)) and not r["velocities"][3].any()
    # far from the target the clamp holds lambda at 1.1 / 0.9
    hot = no.run(pos, vel, np.eye(3) * 30.0, [0, 0, 0], mass, [0, 20], _none, n_steps=1, dt=dt, cutoff=5.0, thermostat="berendsen",
                 temperature=1e5, taut=2.0 * dt)
    cold = no.run(pos, vel, np.eye(3) * 30.0, [0, 0, 0], mass, [0, 20], _none, n_steps=1, dt=dt, cutoff=5.0, thermostat="berendsen",
                  temperature=0.0, taut=0.5 * dt)          # (a negative argument of the square root: lambda 0, clamped)
    assert np.allclose(hot["ekin"][1] / hot["ekin"][0], 1.21, rtol=1e-14) and np.allclose(cold["ekin"][1] / cold["ekin"][0], 0.81, rtol=1e-14)


def test_berendsen_barostat_relaxes_a_harmonic_equation_of_state():
    """Zero velocities, zero forces, a stress callable with P(V) = -K ln(V / V*): with beta = 1 / K the volume contracts to V* and
    |P - P0| falls by (1 - dt / taup) per step to first order."""
    K, Vs, dt, taup, n = 0.5, 900.0, 1.0, 10.0, 60
    pos = np.random.default_rng(2).uniform(0, 10.0, (6, 3))

    def eos(p, cells):
        P = -K * np.log(np.abs(np.linalg.det(cells)) / Vs)
        sig = np.zeros((len(cells), 6))
        sig[:, :3] = -P[:, None]
        return np.zeros(len(cells)), np.zeros_like(p), sig

    for coupling in ("isotropic", "per_axis"):
        r = no.run(pos, np.zeros_like(pos), np.eye(3) * 10.0, [1, 1, 1], np.full(6, 40.0), [0, 6], eos, n_steps=n, dt=dt, cutoff=3.0,
                   barostat="berendsen", coupling=coupling, taup=taup, compressibility=1.0 / K, pressure=0.0)
        P, V = r["pressure"][:, 0], r["volume"][:, 0]
        ratio = P[1:] / P[:-1]
        print(f"{coupling}: V {V[0]:.1f} -> {V[-1]:.4f} (V* {Vs}), |P| {abs(P[0]):.3e} -> {abs(P[-1]):.3e}, decay per step {ratio.min():.5f} .. {ratio.max():.5f}")
        assert abs(V[-1] - Vs) < 0.01 * abs(V[0] - Vs) and np.all(np.abs(np.diff(V)) > 0) and V[-1] > Vs
        assert np.abs(ratio - (1 - dt / taup)).max() < 0.01          # second order in the strain of one step (mu^3 against 1 + 3 (mu - 1))
        assert np.allclose(r["positions"], pos * (r["cells"][0][0, 0] / 10.0), rtol=1e-13) and not r["velocities"].any()
    # the mask: only x and y move, z keeps its bits
    r = no.run(pos, np.zeros_like(pos), np.eye(3) * 10.0, [1, 1, 1], np.full(6, 40.0), [0, 6], eos, n_steps=5, dt=dt, cutoff=3.0,
               barostat="berendsen", taup=taup, compressibility=1.0 / K, mask=(1, 1, 0))
    assert r["cells"][0][2, 2] == 10.0 and np.array_equal(r["positions"][:, 2], pos[:, 2]) and r["cells"][0][0, 0] == r["cells"][0][1, 1] < 10.0


def _ideal_gas(seed):
    pos, cells, mass, start, kw, (v_mean, se) = no.ideal_gas_case(seed=seed)
    v0 = mo.maxwell_boltzmann(mass, start, kw["temperature"], seed=seed)
    out = no.run(pos, v0, cells, [1, 1, 1], mass, start, no.no_forces, cutoff=1.0, **kw)
    return out, v_mean, se


def test_stochastic_cell_rescaling_samples_the_ideal_gas_volume():
    """1024 chains of 8 free particles: <V> = (N + 1) kT / P0 within 5 standard errors of the 1024-chain mean (Var V = (N + 1)(kT / P0)^2),
    with the parameters the device test runs.  The measured deviations of the oracle are in profiles/r36/NOTES_npt.md."""
    out, v_mean, se = _ideal_gas(5)
    V = out["volume"][-1]
    dev = (V.mean() - v_mean) / se
    print(f"ideal gas: <V> {V.mean():.2f} A^3 (wanted {v_mean:.1f}, standard error {se:.2f}): {dev:+.2f} standard errors; std V {V.std(ddof=1):.1f} "
          f"(wanted {se * np.sqrt(len(V)):.1f}); started at 1000")
    assert list(np.unique(out["stop_reason"])) == [1] and np.isfinite(V).all()          # no chain reached the image-count stop
    assert abs(dev) <= 5.0
    assert abs(V.std(ddof=1) / (se * np.sqrt(len(V))) - 1.0) < 0.1                      # (the spread as well: 1 / sqrt(2 x 1024) = 2 % statistical)
    T = 2.0 * out["ekin"][-1] / (3.0 * 8 * no.KB)
    assert abs(T.mean() - 300.0) < 5.0 * 300.0 * np.sqrt(2.0 / 24.0 / 1024.0)


# ---- resume and batch independence -------------------------------------------------------------------------------------------------------
def _lj_case():
    """Two periodic chains under the exact pair virial of a lattice sum (8 and 12 atoms, lj/cut, rc below half the box)."""
    rng = np.random.default_rng(3)
    sizes, L = (8, 12), (9.0, 10.0)
    pos = np.concatenate([rng.uniform(0, 1, (n, 3)) * 0.2 + np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(3)], float)[:n] / 3.0
                          for n in sizes])
    pos = np.concatenate([pos[:8] * L[0], pos[8:] * L[1]])
    cells = np.array([np.eye(3) * l for l in L])
    start = np.array([0, 8, 20])

    def fn(p, C, eps=0.02, sigma=2.6, rc=4.0):
        E, F, S = np.zeros(len(C)), np.zeros_like(p), np.zeros((len(C), 6))
        for b in range(len(C)):
            x = p[start_of[b]:start_of[b + 1]]
            frac = x @ np.linalg.inv(C[b])
            d = frac[None] - frac[:, None]
            d -= np.rint(d)
            d = d @ C[b]
            r2 = (d * d).sum(axis=2)
            np.fill_diagonal(r2, np.inf)
            m = r2 < rc * rc
            s6 = np.where(m, (sigma * sigma / r2) ** 3, 0.0)
            E[b] = 0.5 * (4 * eps * (s6 * s6 - s6)).sum()
            g = np.where(m, -24 * eps * (2 * s6 * s6 - s6) / r2, 0.0)          # dE/dr / r
            F[start_of[b]:start_of[b + 1]] = (g[:, :, None] * d).sum(axis=1)
            W = 0.5 * np.einsum("ij,ija,ijb->ab", g, d, d) / abs(np.linalg.det(C[b]))
            S[b] = [W[0, 0], W[1, 1], W[2, 2], W[1, 2], W[0, 2], W[0, 1]]
        return E, F, S

    start_of = start
    return pos, cells, start, fn


COMBOS = [dict(thermostat="langevin", barostat="crescale", friction=0.02, taup=50.0, compressibility=20.0, pressure=0.01),
          dict(thermostat="berendsen", barostat="berendsen", coupling="per_axis", taut=20.0, taup=50.0, compressibility=20.0, pressure=0.01)]


@pytest.mark.parametrize("combo", COMBOS, ids=["langevin-crescale", "berendsen-per_axis"])
def test_two_calls_equal_one_and_a_chain_does_not_depend_on_its_batch(combo):
    pos, cells, start, fn = _lj_case()
    mass = np.full(20, 39.948)
    ids = np.array([5, 9], np.uint64)
    v0 = mo.maxwell_boltzmann(mass, start, 200.0, seed=4, chain_id=ids)
    kw = dict(dt=2.0, cutoff=4.0, temperature=200.0, seed=4, thermo_interval=2, **combo)
    one = no.run(pos, v0, cells, [1, 1, 1], mass, start, fn, n_steps=20, chain_id=ids, **kw)
    a = no.run(pos, v0, cells, [1, 1, 1], mass, start, fn, n_steps=10, chain_id=ids, **kw)
    b = no.run(a["positions"], a["velocities"], a["cells"], [1, 1, 1], mass, start, fn, n_steps=10, step0=10, chain_id=ids, **kw)
    assert list(one["stop_reason"]) == [1, 1] and np.abs(one["cells"] - cells).max() > 1e-3
    for k in ("positions", "velocities", "cells"):
        assert np.array_equal(b[k], one[k]), k
    for k in ("epot", "ekin", "volume", "pressure"):
        assert np.array_equal(np.concatenate([a[k], b[k][1:]]), one[k]), k

    def alone_fn(p, C):          # chain 1 as a batch of one, through the same callback
        E, F, S = fn(np.concatenate([pos[:8], p]), np.array([cells[0], C[0]]))
        return E[1:], F[8:], S[1:]

    alone = no.run(pos[8:], v0[8:], cells[1:], [1, 1, 1], mass[8:], [0, 12], alone_fn, n_steps=20, chain_id=ids[1:], **kw)
    assert np.array_equal(alone["positions"], one["positions"][8:]) and np.array_equal(alone["cells"][0], one["cells"][1])
    assert np.array_equal(alone["pressure"][:, 0], one["pressure"][:, 1]) and np.array_equal(alone["velocities"], one["velocities"][8:])


def test_without_couplings_the_restatement_is_md_oracle():
    """thermostat none / langevin with no barostat: the positions, velocities and records of tests/md_oracle.py bit for bit."""
    pos = mo.lj_grid(3, 3.9, 0.05, seed=3)
    mass = np.where(np.arange(27) % 2 == 0, 39.948, 83.798)
    v0 = mo.maxwell_boltzmann(mass, [0, 27], 100.0, seed=2)
    f = mo.lj_chain()
    for th, md_th in (("none", "nve"), ("langevin", "langevin")):
        kw = dict(n_steps=15, dt=1.5, temperature=100.0, temperature_end=300.0, ramp_steps=10, friction=0.03, seed=2, thermo_interval=3)
        a = no.run(pos, v0, np.eye(3) * 40.0, [0, 0, 0], mass, [0, 27], lambda p, C: f(p) + (None,), cutoff=8.0, thermostat=th, **kw)
        b = mo.run(pos, v0, mass, [0, 27], f, thermostat=md_th, **kw)
        for k in ("positions", "velocities", "epot", "ekin"):
            assert np.array_equal(a[k], b[k]), (th, k)


# ---- stops ------------------------------------------------------------------------------------------------------------------------------
def test_the_cell_check_and_the_restore_of_the_restatement():
    """A cell whose height sits 0.5 % above cutoff / 2 under a large pressure stops with reason 3 at the state it was evaluated at; a
    non-finite stress at the third evaluation restores positions, velocities and cell of the last completed step."""
    pos = np.random.default_rng(6).uniform(0, 4.0, (5, 3))
    v0 = np.random.default_rng(7).normal(0, 0.01, (5, 3))
    cell = np.eye(3) * 4.02          # cutoff 8: floor(8 / 4.02) + 1 = 2 images; below 4.0 a third one
    kw = dict(dt=1.0, cutoff=8.0, barostat="berendsen", taup=10.0, compressibility=1.0, pressure=0.05, n_steps=30)
    r = no.run(pos, v0, cell, [1, 1, 1], np.full(5, 30.0), [0, 5], no.no_forces, **kw)
    n = int(r["n_done"][0])
    assert r["stop_reason"][0] == 3 and 0 < n < 30 and r["cells"][0][0, 0] >= 4.0 and r["cells"][0][0, 0] * (1 - 0.05 / 30.0) < 4.0
    assert np.isfinite(r["volume"][:n + 1, 0]).all() and np.isnan(r["volume"][n + 1:, 0]).all()
    assert np.array_equal(no.image_counts(r["cells"][0], [1, 1, 1], 8.0)[0], [[2, 2, 2]])
    # open axes never count
    r2 = no.run(pos, v0, cell, [1, 1, 0], np.full(5, 30.0), [0, 5], no.no_forces, mask=(1, 1, 0), **kw)
    assert r2["stop_reason"][0] == 3 and r2["cells"][0][2, 2] == 4.02

    calls = []

    def sick(p, C):
        calls.append((p.copy(), C.copy()))
        E, F, S = no.no_forces(p, C)
        if len(calls) == 3:
            S[0, 1] = np.nan
        return E, F, S

    r = no.run(pos, v0, np.eye(3) * 9.0, [1, 1, 1], np.full(5, 30.0), [0, 5], sick, **{**kw, "cutoff": 3.0})
    assert r["stop_reason"][0] == 2 and r["n_done"][0] == 1 and len(calls) == 3
    assert np.array_equal(r["positions"], calls[1][0]) and np.array_equal(r["cells"], calls[1][1]) and np.array_equal(r["velocities"], v0)


# ---- rehearsal of the device's fcc test (tests/test_npt_gpu.py) ----------------------------------------------------------------------------
def test_the_fcc_cell_reaches_its_target_pressure_in_100_steps():
    """4-atom fcc under lj/cut at T = 0 with zero velocities: Berendsen isotropic with beta = 1 / K of the static lattice and
    dt / taup = 0.1; after 100 steps |P - P0| is below 1e-3 of its start (the linear factor is 0.9^100 = 3e-5)."""
    a0 = no.FCC["a0"]
    P_start, K = no.lj_fcc_pressure_and_modulus(a0, **no.FCC)
    assert K > 0
    pos, cell = no.fcc_cell(a0)
    h = 1e-4

    def fn(p, C):
        a = C[0][0, 0]
        e = no.lj_fcc_energy(a, **no.FCC)
        P = -(no.lj_fcc_energy(a + h, **no.FCC) - no.lj_fcc_energy(a - h, **no.FCC)) / ((a + h) ** 3 - (a - h) ** 3)
        S = np.zeros((1, 6))
        S[0, :3] = -P
        return np.array([e]), np.zeros_like(p), S          # (the perfect lattice: no forces by symmetry)

    r = no.run(pos, np.zeros_like(pos), cell, [1, 1, 1], np.full(4, 39.948), [0, 4], fn, n_steps=100, dt=1.0, cutoff=no.FCC["rc"],
               barostat="berendsen", taup=10.0, compressibility=1.0 / K, pressure=no.FCC_P0)
    P = r["pressure"][:, 0]
    print(f"fcc: a {a0} -> {r['cells'][0][0, 0]:.5f} A, P {P[0]:.4e} -> {P[-1]:.4e} (P0 {no.FCC_P0}), |P - P0| ratio {abs(P[-1] - no.FCC_P0) / abs(P[0] - no.FCC_P0):.2e}, "
          f"K {K:.4f} eV / A^3")
    assert r["stop_reason"][0] == 1 and abs(P[-1] - no.FCC_P0) <= 1e-3 * abs(P[0] - no.FCC_P0)


# ---- rehearsals of the stop and capacity cases of the device tests, under the exact pair virial ---------------------------------------------
def _rehearse(structs, terms, cutoff, fixed=None, draw_at=300.0, seed=3, **kw):
    import npt_cases as nc

    mass, st = nc.masses(structs), nc.start(structs)
    v0 = mo.maxwell_boltzmann(mass, st, draw_at, seed=seed, fixed=fixed)
    return no.run(np.vstack([s[1] for s in structs]), v0, np.array([s[2] for s in structs]), np.array([s[3] for s in structs]), mass, st,
                  nc.pair_fn(terms, structs), cutoff=cutoff, fixed=fixed, seed=seed, **kw)


def test_the_stop_and_capacity_cases_of_the_device_tests():
    import cellrelax_cases as cs
    import npt_cases as nc

    thin = _rehearse(nc.thin_case(), cs.LJ_THIN, nc.THIN_CUTOFF, draw_at=0.0, **nc.THIN)
    assert list(thin["stop_reason"]) == [3, 1] and list(thin["n_done"]) == [3, nc.THIN["n_steps"]]
    assert 3.95 < thin["cells"][0][1, 1] < 3.95 * 1.006 and thin["cells"][1][1, 1] > 4.0          # the step not taken would have crossed 3.95 A
    structs, held, terms, rc = nc.wall_case()
    wall = _rehearse(structs, terms, rc, fixed=held, **nc.WALL)
    assert list(wall["stop_reason"]) == [2, 1] and list(wall["n_done"]) == [5, nc.WALL["n_steps"]]
    assert 0.6 < np.linalg.norm(wall["positions"][8] - wall["positions"][0]) < 0.605 and np.isfinite(wall["pressure"][:6, 0]).all()
    cube = _rehearse([cs.compressing_cube()], cs.LJ, 6.5, draw_at=50.0, **nc.REGROW)
    assert cube["stop_reason"][0] == 1 and 4.0 < cube["cells"][0][0, 0] / 2 < 4.11            # the fifth shell is in
    assert len(nc.COMBOS) == 11 and all(t != "none" for t, b, _ in nc.COMBOS if b == "crescale")
