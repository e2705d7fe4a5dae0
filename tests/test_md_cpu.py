"""The molecular-dynamics restatement (tests/md_oracle.py) checked on its own, and the front end / ABI of the device integrator as far
as they can be checked without a GPU."""
import os
import re

import numpy as np
import pytest

import md_oracle as mo
from surface_sampling_amd import backend, calculators, mc, structures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dimer():
    return np.array([[15.0, 15.0, 15.0], [16.55, 15.1, 14.95]]), np.array([12.011, 15.999])


def _lj27():
    pos = mo.lj_grid(3, 3.9, 0.05, seed=3)
    mass = np.where(np.arange(27) % 2 == 0, 39.948, 83.798)
    return pos, mass


# ---- time reversal -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dimer", "lj27"])
def test_velocity_verlet_is_time_reversible(case):
    if case == "dimer":
        (pos, mass), f, dt, n = _dimer(), mo.morse_dimer(), 0.5, 400
        vel = np.array([[0.002, -0.001, 0.0005], [-0.0015, 0.001, 0.0]])
    else:
        (pos, mass), f, dt, n = _lj27(), mo.lj_chain(), 2.0, 200
        vel = mo.maxwell_boltzmann(mass, [0, 27], 60.0, seed=4)
    a = mo.run(pos, vel, mass, [0, len(pos)], f, n_steps=n, dt=dt)
    assert a["n_done"][0] == n and a["stop_reason"][0] == 1 and a["n_eval"] == n + 1
    assert np.abs(a["positions"] - pos).max() > 1e-3          # it went somewhere
    b = mo.run(a["positions"], -a["velocities"], mass, [0, len(pos)], f, n_steps=n, dt=dt)
    # rounding only: n steps of half an ulp of coordinates of ~16 A each, accumulated (observed: 1e-14 .. 1e-13)
    assert np.abs(b["positions"] - pos).max() < 1e-11
    assert np.abs(b["velocities"] + vel).max() < 1e-13


def test_velocity_verlet_is_second_order():
    pos, mass = _dimer()
    vel = np.zeros((2, 3))
    f = mo.morse_dimer()

    def drift(dt):
        r = mo.run(pos, vel, mass, [0, 2], f, n_steps=int(round(200.0 / dt)), dt=dt)
        e = r["epot"][:, 0] + r["ekin"][:, 0]
        return np.abs(e - e[0]).max()

    ratio = drift(1.0) / drift(0.5)
    assert 3.0 < ratio < 5.0, ratio


# ---- Langevin ------------------------------------------------------------------------------------------------------------------------------
def _free(pos):
    return np.zeros(1), np.zeros_like(pos)


def test_langevin_with_zero_forces_is_the_exact_ornstein_uhlenbeck_update():
    mass = np.array([1.008, 15.999, 47.867, 196.966569])
    pos = np.arange(12, dtype=float).reshape(4, 3)
    vel = np.array([[0.01, 0.0, -0.02], [0.001, 0.002, 0.003], [0.0, 0.0, 0.0], [-0.004, 0.0, 0.001]])
    fixed = np.array([0, 0, 1, 0], bool)
    dt, gamma, T0, T1, ramp, step0, seed, cid = 2.0, 0.05, 300.0, 900.0, 6, 3, 99, 12345678901234
    r = mo.run(pos, vel, mass, [0, 4], _free, n_steps=1, dt=dt, thermostat="langevin", temperature=T0, temperature_end=T1, friction=gamma,
               ramp_steps=ramp, step0=step0, seed=seed, chain_id=[cid], fixed=fixed)
    c1 = np.exp(-gamma * dt)
    T = T0 + (T1 - T0) * (step0 / ramp)
    xi = mo.normals3(np.tile(mo.chain_keys(seed, [cid]), (4, 1)), step0, np.arange(4), mo.TAG_LANGEVIN)
    v_new = c1 * vel + np.sqrt((1 - c1 * c1) * mo.KB * T * mo.ACC / mass)[:, None] * xi
    v_new[fixed] = 0.0
    assert np.allclose(r["velocities"], v_new, rtol=1e-15, atol=0)
    x_new = pos + 0.5 * dt * vel + 0.5 * dt * v_new
    x_new[fixed] = pos[fixed]
    assert np.allclose(r["positions"], x_new, rtol=1e-15, atol=0)
    assert np.array_equal(r["positions"][2], pos[2]) and not r["velocities"][2].any()
    # beyond the ramp the end temperature holds; a chain's numbers depend on its id, the step and the seed
    later = dict(n_steps=1, dt=dt, thermostat="langevin", temperature=T0, temperature_end=T1, friction=gamma, ramp_steps=ramp, seed=seed)
    a = mo.run(pos, 0 * vel, mass, [0, 4], _free, step0=6, chain_id=[cid], **later)["velocities"]
    b = mo.run(pos, 0 * vel, mass, [0, 4], _free, step0=7, chain_id=[cid], **later)["velocities"]
    xa = mo.normals3(np.tile(mo.chain_keys(seed, [cid]), (4, 1)), 6, np.arange(4), mo.TAG_LANGEVIN)
    assert np.allclose(a, np.sqrt((1 - c1 * c1) * mo.KB * T1 * mo.ACC / mass)[:, None] * xa, rtol=1e-15, atol=0)
    assert not np.array_equal(a, b)
    assert not np.array_equal(a, mo.run(pos, 0 * vel, mass, [0, 4], _free, step0=6, chain_id=[cid + 1], **later)["velocities"])


def test_langevin_equilibrium_temperature_of_free_particles():
    n = 4000
    mass = np.full(n, 28.085)
    r = mo.run(np.zeros((n, 3)), np.zeros((n, 3)), mass, [0, n], _free, n_steps=60, dt=1.0, thermostat="langevin", temperature=500.0,
               friction=0.2, seed=1)
    T = 2 * r["ekin"][-1, 0] / (3 * n * mo.KB)
    assert abs(T - 500.0) < 5 * 500.0 * np.sqrt(2.0 / (3 * n))


# ---- resumability, batching, non-finite ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thermostat", ["nve", "langevin"])
def test_two_segments_equal_one_run(thermostat):
    pos, mass = _lj27()
    vel = mo.maxwell_boltzmann(mass, [0, 27], 100.0, seed=8, chain_id=[5])
    fixed = np.arange(27) < 3
    kw = dict(dt=2.0, thermostat=thermostat, temperature=100.0, temperature_end=250.0, friction=0.02, ramp_steps=30, seed=8, chain_id=[5],
              fixed=fixed, thermo_interval=5)
    f = mo.lj_chain()
    one = mo.run(pos, vel, mass, [0, 27], f, n_steps=40, **kw)
    a = mo.run(pos, vel, mass, [0, 27], f, n_steps=20, **kw)
    b = mo.run(a["positions"], a["velocities"], mass, [0, 27], f, n_steps=20, step0=20, **kw)
    assert np.array_equal(b["positions"], one["positions"]) and np.array_equal(b["velocities"], one["velocities"])
    assert np.array_equal(np.concatenate([a["epot"], b["epot"][1:]]), one["epot"])
    assert np.array_equal(np.concatenate([a["ekin"], b["ekin"][1:]]), one["ekin"])
    assert one["epot"].shape == (9, 1) and np.array_equal(pos[:3], one["positions"][:3])


def test_a_chain_does_not_depend_on_its_batch_and_a_blow_up_stops_one_chain_only():
    pos, mass = _lj27()
    f1 = mo.lj_chain()
    dpos, dmass = _dimer()
    fd = mo.morse_dimer()
    calls = [0]

    def both(p):
        calls[0] += 1
        (e0,), f0 = f1(p[:27])
        (e1,), fdim = fd(p[27:])
        if calls[0] == 4:                      # the evaluation that would close the dimer's third step
            fdim = fdim * np.nan
        return np.array([e0, e1]), np.vstack([f0, fdim])

    P, M = np.vstack([pos, dpos]), np.concatenate([mass, dmass])
    V = mo.maxwell_boltzmann(M, [0, 27, 29], 80.0, seed=2, chain_id=[40, 41])
    kw = dict(n_steps=6, dt=1.0, thermostat="langevin", temperature=80.0, friction=0.05, seed=2)
    r = mo.run(P, V, M, [0, 27, 29], both, chain_id=[40, 41], **kw)
    alone = mo.run(pos, V[:27], mass, [0, 27], f1, chain_id=[40], **kw)
    assert np.array_equal(r["positions"][:27], alone["positions"]) and np.array_equal(r["epot"][:, 0], alone["epot"][:, 0])
    assert list(r["n_done"]) == [6, 2] and list(r["stop_reason"]) == [1, 2]
    two = mo.run(dpos, V[27:], dmass, [0, 2], fd, chain_id=[41], **{**kw, "n_steps": 2})
    assert np.array_equal(r["positions"][27:], two["positions"]) and np.array_equal(r["velocities"][27:], two["velocities"])
    assert np.isnan(r["epot"][3:, 1]).all() and np.isfinite(r["epot"][:3, 1]).all()


# ---- the generator -----------------------------------------------------------------------------------------------------------------------
def test_box_muller_moments_and_layout():
    n = 500000
    keys = np.tile(mo.chain_keys(0xDEADBEEFCAFE, [3]), (n, 1))
    z0, z1 = mo.normal_pairs(keys, 17, np.arange(n), mo.TAG_LANGEVIN, 0)
    z = np.concatenate([z0, z1])
    assert len(z) == 10 ** 6 and np.isfinite(z).all()
    assert abs(z.mean()) < 5 / np.sqrt(len(z))
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / len(z))
    assert abs(np.mean(z0 * z1)) < 5 / np.sqrt(n)
    # the layout, word for word, on one draw
    seed, cid, step, atom = 0x0123456789ABCDEF, (7 << 32) | 9, (1 << 33) + 5, 11
    q = mc.philox4x32(np.array([9, 7, 0x4D44, 0]), np.array([0x89ABCDEF, 0x01234567]))[:2]
    assert np.array_equal(q, mo.chain_keys(seed, [cid])[0])
    w = mc.philox4x32(np.array([5, 2, atom, (mo.TAG_LANGEVIN << 8) | 1]), q).astype(np.uint64)
    u1 = (float((int(w[0]) << 21) | (int(w[1]) >> 11)) + 1.0) * 2.0 ** -53
    u2 = (float((int(w[2]) << 21) | (int(w[3]) >> 11)) + 1.0) * 2.0 ** -53
    assert 0.0 < u1 <= 1.0 and 0.0 < u2 <= 1.0
    z = mo.normal_pairs(q[None], step, [atom], mo.TAG_LANGEVIN, 1)
    assert np.isclose(z[0][0], np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2), rtol=1e-12, atol=1e-15)
    assert np.isclose(z[1][0], np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2), rtol=1e-12, atol=1e-15)
    assert mo.ACC == 1.602176634e-19 / 1.66053906660e-27 * 1e-10 and abs(mo.ACC - 9.648533212e-3) < 1e-11


def test_maxwell_boltzmann_draw():
    n = 20000
    mass = np.where(np.arange(n) % 2 == 0, 1.008, 196.966569)
    fixed = np.arange(n) < 10
    v = mo.maxwell_boltzmann(mass, [0, n], 300.0, seed=5, fixed=fixed)
    assert not v[:10].any()
    T = (mass[10:, None] * v[10:] ** 2).sum() / mo.ACC / (3 * (n - 10) * mo.KB)
    assert abs(T - 300.0) < 5 * 300.0 * np.sqrt(2.0 / (3 * (n - 10)))
    assert not np.array_equal(v, mo.maxwell_boltzmann(mass, [0, n], 300.0, seed=6, fixed=fixed))


# ---- front end and ABI ---------------------------------------------------------------------------------------------------------------------
def test_standard_atomic_weights():
    pins = {"H": 1.008, "N": 14.007, "O": 15.999, "Si": 28.085, "Ti": 47.867, "Cu": 63.546, "Ga": 69.723, "Sr": 87.62, "Au": 196.96657}
    for sym, m in pins.items():
        assert abs(structures.ATOMIC_MASSES[structures.ATOMIC_NUMBERS[sym]] / m - 1.0) < 1e-3, sym
    assert len(structures.ATOMIC_MASSES) == len(structures.SYMBOLS) and (structures.ATOMIC_MASSES > 0).all()
    assert (np.diff(structures.ATOMIC_MASSES[1:]) > -1.7).all()      # (the known inversions: Ar/K, Co/Ni, Te/I, Th/Pa, U/Np, Pu/Am)
    s = structures.Structure([31, 7], np.zeros((2, 3)), np.eye(3) * 10)
    assert np.allclose(structures.masses_of(s), [69.723, 14.007])
    assert np.array_equal(structures.masses_of(s, [2.0, 3.0]), [2.0, 3.0])

    class WithMasses(structures.Structure):
        def get_masses(self):
            return np.array([70.0, 15.0])

    assert np.array_equal(structures.masses_of(WithMasses([31, 7], np.zeros((2, 3)), np.eye(3))), [70.0, 15.0])
    for bad in ([1.0], [1.0, 0.0], [1.0, np.nan], [1.0, -2.0]):
        with pytest.raises(ValueError):
            structures.masses_of(s, bad)


def test_header_declares_the_entry_points_and_exports_list_them():
    header = open(os.path.join(ROOT, "include", "vssr_eval.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    assert re.search(r"enum\s*\{\s*VSSR_MD_NVE\s*=\s*0,\s*VSSR_MD_LANGEVIN\s*=\s*1\s*\}\s*;", flat)
    assert re.search(r"typedef\s+struct\s*\{\s*int32_t\s+n_steps,\s*thermostat,\s*thermo_interval;\s*double\s+dt;\s*double\s+temperature,\s*"
                     r"temperature_end,\s*friction;\s*int64_t\s+ramp_steps,\s*step0;\s*uint64_t\s+seed;\s*\}\s*vssr_md_params;", flat)
    assert re.search(r"int\s+vssr_batch_md_set_velocities\s*\(\s*vssr_handle\s*\*h,\s*const\s+double\s*\*vel\s*\)\s*;", flat)
    assert re.search(r"int\s+vssr_batch_md_draw_velocities\s*\(\s*vssr_handle\s*\*h,\s*const\s+double\s*\*mass,\s*const\s+uint8_t\s*\*fixed,\s*"
                     r"const\s+uint64_t\s*\*chain_id,\s*double\s+temperature,\s*uint64_t\s+seed\s*\)\s*;", flat)
    assert re.search(r"int\s+vssr_batch_md_get_velocities\s*\(\s*vssr_handle\s*\*h,\s*double\s*\*vel\s*\)\s*;", flat)
    assert re.search(r"int\s+vssr_batch_md\s*\(\s*vssr_handle\s*\*h,\s*const\s+vssr_md_params\s*\*p,\s*const\s+double\s*\*mass\s*,\s*const\s+uint8_t\s*"
                     r"\*fixed\s*,\s*const\s+uint64_t\s*\*chain_id\s*,\s*uint32_t\s+want,\s*double\s*\*pos_out,\s*double\s*\*thermo\s*,\s*"
                     r"int32_t\s*\*n_done,\s*int32_t\s*\*stop_reason\s*\)\s*;", flat)
    assert re.search(r"int\s+vssr_batch_md_driver\s*\(\s*vssr_handle\s*\*h,\s*int32_t\s+driver,\s*int32_t\s*\*last_used\s*\)\s*;", flat)
    assert re.search(r"#define\s+VSSR_ABI_VERSION\s+1\b", header)
    lib = backend.load_library()
    # every call with a null handle: refused by the usual kind check (no device needed)
    null_calls = {"vssr_batch_md": (None, None, None, None, None, 0, None, None, None, None), "vssr_batch_md_set_velocities": (None, None),
                  "vssr_batch_md_draw_velocities": (None, None, None, None, 0.0, 0), "vssr_batch_md_get_velocities": (None, None),
                  "vssr_batch_md_driver": (None, 0, None)}
    for name, args in null_calls.items():
        assert name in backend.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args), name
        assert fn(*args) == -1, name
    assert [n for n, _ in backend.MdParams._fields_] == ["n_steps", "thermostat", "thermo_interval", "dt", "temperature", "temperature_end",
                                                         "friction", "ramp_steps", "step0", "seed"]
    import ctypes
    assert ctypes.sizeof(backend.MdParams) == 72
    assert backend.MD_THERMOSTATS == {"nve": 0, "langevin": 1} and backend.MD_DRIVERS == {"auto": 0, "lockstep": 1, "resident": 2}
    assert backend.KB_EV == mo.KB
    for name in ("PainnEngine", "TersoffEngine", "SWEngine", "EAMEngine", "PairEngine"):
        eng = getattr(backend, name)
        assert all(hasattr(eng, k) for k in ("md", "set_velocities", "draw_velocities", "get_velocities", "md_driver")), name


def test_python_side_argument_checks_come_before_any_device_call():
    for bad in ("bogus", "NVE", "", None, 1):
        with pytest.raises(ValueError, match="thermostat"):
            backend.md_thermostat_code(bad)
        with pytest.raises(ValueError, match="MD driver"):
            backend.md_driver_code(bad)
    s = structures.Structure([31, 7], np.array([[0, 0, 0], [0, 0, 1.9]], float), np.eye(3) * 10)

    def no_engine():
        raise AssertionError("the engine was asked for before the arguments were checked")

    for calc in (calculators.TersoffSurfCalc.__new__(calculators.TersoffSurfCalc), calculators.EnsembleNFFSurface.__new__(calculators.EnsembleNFFSurface)):
        calc.parameters, calc.results, calc.atoms = {}, {}, None
        calc.species, calc.all_periodic = ["Ga", "N"], True
        calc._get_engine = no_engine
        for kw, match in ((dict(thermostat="nose"), "thermostat"), (dict(md_driver="fast"), "MD driver"), (dict(steps=-1), "steps"),
                          (dict(timestep=0.0), "timestep"), (dict(thermo_interval=0), "thermo_interval"),
                          (dict(thermostat="langevin", friction=0.0), "friction"), (dict(temperature=-1.0), "temperature"),
                          (dict(masses=[[1.0, 2.0], [1.0]]), "mass arrays"), (dict(masses=[[1.0, -2.0]]), "masses"),
                          (dict(velocities=[]), "velocity arrays")):
            with pytest.raises(ValueError, match=match):
                calc.md_batch([s], **kw)


# ---- rehearsals of what the device tests presume (tests/test_md_gpu.py) -------------------------------------------------------------------
def test_the_contracting_cluster_outgrows_its_start_capacity():
    (T, pos, cell, pbc), mass, steps, dt = mo.contracting_cluster()
    r = mo.run(pos, np.zeros_like(pos), mass, [0, 27], mo.lj_chains(**mo.LJ00)(27), n_steps=steps, dt=dt, thermostat="langevin", temperature=50.0,
               friction=0.002)
    (s0, p0), (s1, p1) = mo.padded_slots(pos), mo.padded_slots(r["positions"])
    assert (p0, p1 > 500) == (370, True)
    pool = 27 * mo.TIGHT_SLOTS_PER_ATOM
    assert int(np.ceil(np.log2(s0 / pool))) == 2 and int(np.ceil(np.log2(s1 / pool))) == 3
    assert np.abs(pos[:, None] - pos[None]).max() < 12.0      # the far chain of the device test (x 3) has no pair within the cutoff


def test_two_oracle_runs_with_different_seeds_agree_on_the_long_run_temperature():
    pos, mass, start, kw = mo.sanity_case()
    f = mo.lj_chains(**mo.LJ11)(27)
    T = [mo.second_half_temperature(mo.run(pos, mo.maxwell_boltzmann(mass, start, 300.0, seed=s), mass, start, f, seed=s, **kw)["ekin"], 27)
         for s in (21, 22)]
    ok, a, b, se = mo.agree_within(*T)
    print(f"second-half kinetic temperature: {a:.2f} K and {b:.2f} K, combined standard error {se:.2f} K")
    assert ok and se < 6.0


def test_time_reversal_residual_of_the_gan48_case(golden, oracle_mod):
    """The value tests/test_md_gpu.py::test_time_reversal_on_the_device allows 100 x of."""
    import cg_cases as cc
    from test_md_gpu import GAN48_REVERSAL_RESIDUAL

    worst = 0.0
    for k in range(4):
        c = cc._slab_with_adatoms(golden, 1, 12, 50 + k)
        fn = cc.force_fn(c, golden, oracle_mod)
        mass = np.where(c.types == 0, 69.723, 14.007)
        fixed = np.zeros(48, bool)
        fixed[c.fixed] = True
        v0 = mo.maxwell_boltzmann(mass, [0, 48], 300.0, seed=5, chain_id=[k], fixed=fixed)
        f = lambda p: (lambda E, F: (np.array([E]), F))(*fn(p))
        a = mo.run(c.pos, v0, mass, [0, 48], f, n_steps=50, dt=1.0, fixed=fixed)
        b = mo.run(a["positions"], -a["velocities"], mass, [0, 48], f, n_steps=50, dt=1.0, fixed=fixed)
        worst = max(worst, float(np.abs(b["positions"] - c.pos).max()))
    print(f"gan48 time-reversal residual of the oracle: {worst:.3e} A")
    assert 0.25 * GAN48_REVERSAL_RESIDUAL <= worst <= GAN48_REVERSAL_RESIDUAL
