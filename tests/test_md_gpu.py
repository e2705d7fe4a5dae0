"""Device molecular dynamics (vssr_batch_md: csrc/md_dev.h, md.hip, k_md_chain in chain_min.hip) against the numpy restatement
tests/md_oracle.py, and the two drivers against each other bit for bit."""
import numpy as np
import pytest

import cg_cases as cc
import cg_resident_cases as rc
import md_oracle as mo
import pair_cases as pc

pytestmark = pytest.mark.gpu

TYPE_MASS = np.array([26.9815385, 63.546, 107.8682])
WANT = 1 | 2 | 16   # energy, forces, per-atom energies


def _pack(structs):
    from surface_sampling_amd import backend

    return backend.pack_batch(structs)


def _masses(structs):
    return np.concatenate([TYPE_MASS[np.asarray(s[0]) % 3] for s in structs])


def _start(structs):
    return np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])])


def _device_forces(eng, structs):
    """The device's own single-point evaluation as the oracle's force callback: the potential's tolerance does not enter."""
    n_atoms, T, _, cell, pbc = _pack(structs)

    def fn(pos):
        e, _, f = eng.evaluate_arrays_f64(n_atoms, T, pos, cell, pbc)
        return e, f
    return fn


def _md(eng, structs, mass, fixed, vel=None, ids=None, temperature=300.0, seed=7, driver=None, upload=True, **kw):
    """Upload, velocities (given, else drawn at ``temperature``), one md call; the engine's dict plus final results and counters."""
    if upload:
        eng.upload(structs)
        if vel is None:
            eng.draw_velocities(mass, temperature, seed=seed, fixed=fixed, chain_id=ids)
        else:
            eng.set_velocities(vel)
    v0 = eng.get_velocities()
    out = eng.md(mass, fixed=fixed, chain_id=ids, seed=seed, temperature=temperature, want=WANT, driver=driver, **kw)
    out["v0"], out["driver"], out["counts"], out["regrows"] = v0, eng.last_md_driver, eng.last_relax_counts, eng.debug_capacity()
    if hasattr(eng, "results_f64"):
        out["e"], out["ea"], out["f"] = eng.results_f64()
    return out


KEYS = ("positions", "velocities", "epot", "ekin", "n_done", "stop_reason", "e", "ea", "f")


def _assert_equal(a, b, tag):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k, np.abs(np.asarray(a[k], float) - np.asarray(b[k], float)).max())


def _close(a, b, tol, tag):
    err = float(np.abs(np.asarray(a) - np.asarray(b)).max()) if np.size(a) else 0.0
    print(f"{tag}: max |device - oracle| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol, tag


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_free_particles_pin_generator_coefficients_units_ramp_and_mask():
    """pair_lj handle, chains of 1, 3, 64 and 65 atoms 12 A apart under the 8 A cutoff in an open box: forces are exactly zero, so there
    is no chaos and 200 Langevin steps with a temperature ramp, two masses and a held atom equal the oracle's to 1e-13 of the arrays'
    scale -- the Maxwell-Boltzmann draw included."""
    eng = rc.engine("pair_lj")
    structs = []
    for k, n in enumerate((1, 3, 64, 65)):
        g = np.array([[x, y, z] for z in range(5) for y in range(4) for x in range(4)], float)[:n] * 12.0 + 6.0
        structs.append(((np.arange(n) % 2).astype(np.int32), g, np.eye(3) * 80.0, np.zeros(3, np.uint8)))
    mass, start = _masses(structs), _start(structs)
    fixed = np.zeros(start[-1], np.uint8)
    fixed[5] = 1                                   # an atom of the 64-atom chain
    ids = np.array([3, (1 << 40) + 1, 2, 77], np.uint64)
    kw = dict(steps=200, timestep=1.0, thermostat="langevin", temperature_end=900.0, ramp_steps=120, friction=0.01, thermo_interval=50)
    dev = _md(eng, structs, mass, fixed, ids=ids, temperature=300.0, seed=0x1234567890ABCDEF, **kw)
    pos0 = np.concatenate([s[1] for s in structs])
    v0 = mo.maxwell_boltzmann(mass, start, 300.0, seed=0x1234567890ABCDEF, chain_id=ids, fixed=fixed)
    _close(dev["v0"], v0, 1e-13 * np.abs(v0).max(), "Maxwell-Boltzmann draw")
    ora = mo.run(pos0, v0, mass, start, lambda p: (np.zeros(4), np.zeros_like(p)), n_steps=200, dt=1.0, thermostat="langevin",
                 temperature=300.0, temperature_end=900.0, ramp_steps=120, friction=0.01, seed=0x1234567890ABCDEF, chain_id=ids, fixed=fixed,
                 thermo_interval=50)
    d = ora["positions"][:, None] - ora["positions"][None]
    for a0, a1 in zip(start[:-1], start[1:]):      # still beyond the cutoff: the forces were zero all along
        r = np.sqrt((d[a0:a1, a0:a1] ** 2).sum(axis=2)) + np.eye(a1 - a0) * 100
        assert r.min() > 8.5
    assert np.array_equal(dev["epot"], np.zeros((5, 4))) and not dev["f"].any()
    _close(dev["velocities"], ora["velocities"], 1e-13 * np.abs(ora["velocities"]).max(), "velocities")
    _close(dev["positions"], ora["positions"], 1e-13 * np.abs(ora["positions"]).max(), "positions")
    _close(dev["positions"] - pos0, ora["positions"] - pos0, 1e-12 * np.abs(ora["positions"] - pos0).max(), "displacements")
    _close(dev["ekin"], ora["ekin"], 1e-12 * ora["ekin"].max(), "kinetic energies")
    assert np.array_equal(dev["positions"][5], pos0[5]) and not dev["velocities"][5].any()
    assert list(dev["n_done"]) == [200] * 4 and list(dev["stop_reason"]) == [1] * 4 and dev["driver"] == "lockstep"
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _parity_case(kind, golden):
    """(engine, structures, held mask) of one kind of handle."""
    from surface_sampling_amd import backend, pair

    if kind in rc.KINDS:
        structs, mask = rc.size_batch(kind)
        assert tuple(len(s[0]) for s in structs) == rc.SIZES
        return rc.engine(kind), structs, mask
    if kind == "gan48":
        structs, mask = rc.gan48(golden)
        return backend.TersoffEngine(golden.tersoff_params, device=0), structs, mask
    if kind == "ewald":
        import ewald_cases as ec

        structs = [ec.rattled_cube(), ec.cube()]
        return backend.PairEngine(pair.parse(ec.RAGGED_MODEL, 3), device=0), structs, pc.held_mask(structs)
    import vashishta_oracle as vo

    structs = [vo.rattled_sic(seed=2, sigma=0.08, reps=(3, 1, 1), n_fixed=12), vo.rattled_sic(seed=3, sigma=0.05)]
    mask = np.zeros(32, np.uint8)
    mask[:12] = 1
    return backend.VashishtaEngine(vo.sic_params()[1], device=0), structs, mask


PARITY_KINDS = ("pair_lj", "pair_born_dsf", "sw", "eam_funcfl", "eam_alloy", "gan48", "ewald", "vashishta")


@pytest.mark.parametrize("kind", PARITY_KINDS)
def test_step_for_step_parity_with_the_oracle_on_the_devices_own_forces(kind, golden):
    """10 steps of 1 fs, NVE and Langevin, ragged batches with held atoms, against the oracle driven by the device's single-point
    evaluation.  Positions within 10 n^2 dt^2 dF / (2 m_min) with dF = 1e-12 eV / A (converted to A / fs^2), velocities within the same
    bound over n dt, thermo records to 1e-10 relative (floor 1 eV)."""
    eng, structs, mask = _parity_case(kind, golden)
    mass, start = _masses(structs), _start(structs)
    n, dt, dF = 10, 1.0, 1e-12
    bound_x = 10.0 * n * n * dt * dt * dF * mo.ACC / (2.0 * mass.min())
    bound_v = bound_x / (n * dt)
    pos0 = np.concatenate([s[1] for s in structs])
    fn = _device_forces(eng, structs)
    for thermostat in ("nve", "langevin"):
        kw = dict(thermostat=thermostat, temperature=300.0, temperature_end=500.0, ramp_steps=8, friction=0.02)
        dev = _md(eng, structs, mass, mask, seed=11, steps=n, timestep=dt, thermo_interval=2, **kw)
        assert list(dev["n_done"]) == [n] * len(structs) and list(dev["stop_reason"]) == [1] * len(structs), kind
        ora = mo.run(pos0, dev["v0"], mass, start, fn, n_steps=n, dt=dt, seed=11, fixed=mask, thermo_interval=2, **kw)
        tag = f"{kind} {thermostat}"
        _close(dev["positions"], ora["positions"], bound_x, tag + " positions")
        _close(dev["velocities"], ora["velocities"], bound_v, tag + " velocities")
        for key in ("epot", "ekin"):
            _close(dev[key] / np.maximum(np.abs(ora[key]), 1.0), ora[key] / np.maximum(np.abs(ora[key]), 1.0), 1e-10, f"{tag} {key}")
        held = mask.astype(bool)
        assert np.array_equal(dev["positions"][held], pos0[held]) and not dev["velocities"][held].any()
        assert np.abs(dev["positions"] - pos0).max() > 1e-3
        # the batch is left with a complete evaluation of the final positions
        e, f = fn(dev["positions"])
        assert np.array_equal(e, dev["e"]) and np.array_equal(f, dev["f"]), tag
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_painn_follows_the_oracle_on_its_fp32_forces(golden):
    """The 36-atom GaN slab twice in one batch, 5 steps of 0.5 fs, NVE and Langevin; dF = one fp32 ulp of the largest force component."""
    from surface_sampling_amd import backend, structures

    S = golden.structure("GaN_3x3_pristine")
    assert len(S) == min(len(golden.structures[k]) for k in golden.structures.files if k.endswith(".numbers"))
    structs = [structures.as_arrays(S)] * 2
    eng = backend.PainnEngine(golden.blobs, device=0)
    mass = np.concatenate([structures.masses_of(S)] * 2)
    start = _start(structs)
    mask = np.concatenate([(S.positions[:, 2] < S.positions[:, 2].min() + 1.0).astype(np.uint8)] * 2)
    pos0 = np.concatenate([s[1] for s in structs])

    def fn(pos):
        r = eng.evaluate([(structs[b][0], pos[start[b]:start[b + 1]], structs[b][2], structs[b][3]) for b in range(2)])
        return r["energy_f64"], r["forces"].astype(np.float64)

    f0 = np.abs(fn(pos0)[1]).max()
    n, dt, dF = 5, 0.5, float(np.spacing(np.float32(f0)))
    bound_x = 10.0 * n * n * dt * dt * dF * mo.ACC / (2.0 * mass.min())
    for thermostat in ("nve", "langevin"):
        kw = dict(thermostat=thermostat, temperature=300.0, friction=0.05)
        eng.upload(structs)
        eng.draw_velocities(mass, 300.0, seed=3, fixed=mask, chain_id=[8, 9])
        v0 = eng.get_velocities()
        dev = eng.md(mass, n, dt, fixed=mask, chain_id=[8, 9], seed=3, **kw)
        res = eng.download()
        ora = mo.run(pos0, v0, mass, start, fn, n_steps=n, dt=dt, seed=3, chain_id=[8, 9], fixed=mask, **kw)
        print(f"PaiNN {thermostat}: max |F| {f0:.3f} eV/A, dF {dF:.2e}")
        _close(dev["positions"], ora["positions"], bound_x, f"PaiNN {thermostat} positions")
        _close(dev["velocities"], ora["velocities"], bound_x / (n * dt), f"PaiNN {thermostat} velocities")
        for key in ("epot", "ekin"):
            _close(dev[key] / np.maximum(np.abs(ora[key]), 1.0), ora[key] / np.maximum(np.abs(ora[key]), 1.0), 1e-10, f"PaiNN {thermostat} {key}")
        assert list(dev["n_done"]) == [n, n] and list(dev["stop_reason"]) == [1, 1] and eng.last_md_driver == "lockstep"
        assert np.array_equal(res["forces"], eng.evaluate([(s[0], dev["positions"][a0:a1], s[2], s[3])
                                                           for s, a0, a1 in zip(structs, start[:-1], start[1:])])["forces"])
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
RESIDENT_KINDS = rc.KINDS + ("gan48",)
LANGEVIN40 = dict(steps=40, timestep=1.0, thermostat="langevin", temperature=300.0, temperature_end=600.0, ramp_steps=40, friction=0.02,
                  thermo_interval=4)


@pytest.mark.parametrize("kind", RESIDENT_KINDS)
def test_the_chain_resident_driver_equals_the_lock_step_driver_bit_for_bit(kind, golden):
    eng, structs, mask = _parity_case(kind, golden)
    mass = _masses(structs)
    lock = _md(eng, structs, mass, mask, driver="lockstep", **LANGEVIN40)
    res = _md(eng, structs, mass, mask, driver="resident", **LANGEVIN40)
    print(f"{kind}: lock-step evaluations {lock['counts']}, resident launches / chain evaluations {res['counts']}")
    assert lock["driver"] == "lockstep" and res["driver"] == "resident"
    assert eng.md_driver() == "resident" and list(res["n_done"]) == [40] * len(structs) and list(res["stop_reason"]) == [1] * len(structs)
    # (a regrow repeats the lock-step evaluation that overflowed; a chain-resident evaluation that overflows is not counted)
    assert res["counts"] == (1 + res["regrows"], 41 * len(structs)) and lock["counts"][0] >= 41 and (lock["regrows"] > 0 or lock["counts"][0] == 41)
    _assert_equal(res, lock, kind)
    assert np.abs(res["positions"] - np.concatenate([s[1] for s in structs])).max() > 1e-3
    # the automatic rule: small Tersoff batches take the chain-resident kernel, every other kind the lock-step driver
    auto = _md(eng, structs, mass, mask, driver="auto", **LANGEVIN40)
    assert auto["driver"] == ("resident" if kind == "gan48" else "lockstep")
    _assert_equal(auto, lock, kind + " auto")
    if kind in rc.KINDS:      # one chain of 257 atoms: the whole batch runs in lock step, without an error, and the others keep their bits
        more, mask257 = rc.size_batch(kind, with_257=True)
        big = _md(eng, more, _masses(more), mask257, driver="resident", **LANGEVIN40)
        assert big["driver"] == "lockstep" and list(big["n_done"]) == [40] * 7
        n = len(res["positions"])
        for k in ("positions", "velocities", "f"):
            assert np.array_equal(big[k][:n], res[k]), (kind, k)
        assert np.array_equal(big["epot"][:, :6], res["epot"]) and np.array_equal(big["ekin"][:, :6], res["ekin"])
    eng.close()


def test_resident_is_lock_step_where_the_kernel_does_not_apply(golden):
    for kind in ("ewald", "vashishta"):
        eng, structs, mask = _parity_case(kind, golden)
        out = _md(eng, structs, _masses(structs), mask, driver="resident", steps=3, timestep=1.0)
        assert out["driver"] == "lockstep" and list(out["n_done"]) == [3] * len(structs)
        eng.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pair_lj", "gan48"])
@pytest.mark.parametrize("driver", ["lockstep", "resident"])
def test_two_calls_equal_one_and_a_chain_does_not_depend_on_its_batch(kind, driver, golden):
    eng, structs, mask = _parity_case(kind, golden)
    mass, start = _masses(structs), _start(structs)
    ids = np.arange(len(structs), dtype=np.uint64) + 1000
    one = _md(eng, structs, mass, mask, ids=ids, driver=driver, **LANGEVIN40)
    half = dict(LANGEVIN40, steps=20)
    a = _md(eng, structs, mass, mask, ids=ids, driver=driver, **half)
    b = _md(eng, structs, mass, mask, ids=ids, driver=driver, upload=False, step0=20, **half)      # the state the first call left resident
    assert a["driver"] == b["driver"] == one["driver"] == driver
    assert np.array_equal(b["v0"], a["velocities"])
    for k in ("positions", "velocities", "e", "ea", "f", "n_done", "stop_reason"):
        assert np.array_equal(b[k], one[k] if k != "n_done" else one[k] - 20), (kind, driver, k)
    for k in ("epot", "ekin"):
        assert np.array_equal(np.concatenate([a[k], b[k][1:]]), one[k]), (kind, driver, k)
    # chain k of the ragged batch alone, under its own id
    k = len(structs) - 2
    a0, a1 = start[k], start[k + 1]
    alone = _md(eng, [structs[k]], mass[a0:a1], mask[a0:a1], ids=ids[k:k + 1], driver=driver, **LANGEVIN40)
    assert np.array_equal(alone["positions"], one["positions"][a0:a1]) and np.array_equal(alone["velocities"], one["velocities"][a0:a1])
    assert np.array_equal(alone["epot"][:, 0], one["epot"][:, k]) and np.array_equal(alone["ekin"][:, 0], one["ekin"][:, k])
    assert np.array_equal(alone["f"], one["f"][a0:a1])
    other = _md(eng, [structs[k]], mass[a0:a1], mask[a0:a1], ids=ids[k:k + 1] + 1, driver=driver, **LANGEVIN40)
    assert not np.array_equal(other["positions"], alone["positions"])
    eng.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", ["lockstep", "resident"])
def test_capacity_regrow_in_the_middle_of_a_trajectory(driver):
    """The 27-atom cluster of md_oracle.contracting_cluster falls together: 370 pairs within the cutoff at the start, more than 500
    after 90 steps (rehearsed in tests/test_md_cpu.py).  Under a capacity that is tight for the start the evaluation overflows again
    mid-trajectory; the trajectory equals the roomy run bit for bit."""
    struct, m, steps, dt = mo.contracting_cluster()
    far = (struct[0][:5], struct[1][:5] * 3.0, struct[2] * 3, struct[3])      # a second chain whose rows never grow
    structs, mass = [struct, far], np.concatenate([m, m[:5]])
    kw = dict(steps=steps, timestep=dt, thermostat="langevin", temperature=50.0, friction=0.002, thermo_interval=10)
    vel = np.zeros((32, 3))
    roomy_eng = rc.engine("pair_lj")
    roomy = _md(roomy_eng, structs, mass, None, vel=vel, driver=driver, **kw)
    roomy_eng.close()
    tight_eng = rc.engine("pair_lj")
    tight_eng.debug_capacity(slots_per_atom=mo.TIGHT_SLOTS_PER_ATOM, tight=1)
    tight = _md(tight_eng, structs, mass, None, vel=vel, driver=driver, **kw)
    tight_eng.close()
    print(f"{driver}: roomy counts {roomy['counts']} regrows {roomy['regrows']}; tight counts {tight['counts']} regrows {tight['regrows']}")
    assert roomy["driver"] == tight["driver"] == driver and roomy["regrows"] == 0
    s0, s1 = mo.padded_slots(struct[1])[0], mo.padded_slots(roomy["positions"][:27])[0]
    assert s1 > s0
    if driver == "lockstep":
        # the first evaluation overflows, and so does the first one whose rows outgrow the exact capacity the regrow gave; every regrow
        # repeats at least the evaluation that overflowed: more batch-wide evaluations than the steps need
        assert roomy["counts"][0] == steps + 1 and tight["regrows"] >= 2 and tight["counts"][0] > steps + 1
    else:
        # the pools of 27 x 5 slots double: what the rows need at the start and at the end lie a doubling apart
        pool = 27 * mo.TIGHT_SLOTS_PER_ATOM
        at_start, at_end = int(np.ceil(np.log2(s0 / pool))), int(np.ceil(np.log2(s1 / pool)))
        assert at_end > at_start and tight["regrows"] > at_start and tight["counts"][0] == 1 + tight["regrows"]
    _assert_equal(tight, roomy, driver)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
# max |r - r_start| of the oracle on the CPU for this case (Tersoff from the fp64 CPU oracle): 50 steps forward, v -> -v, 50 steps
# (profiles/r29/NOTES_md.md; rehearsed by tests/test_md_cpu.py::test_time_reversal_residual_of_the_gan48_case)
GAN48_REVERSAL_RESIDUAL = 6.2e-11


def test_time_reversal_on_the_device(golden):
    from surface_sampling_amd import backend

    structs, mask = rc.gan48(golden)
    mass = np.concatenate([np.where(np.asarray(s[0]) == 0, 69.723, 14.007) for s in structs])
    eng = backend.TersoffEngine(golden.tersoff_params, device=0)
    pos0 = np.concatenate([s[1] for s in structs])
    fwd = _md(eng, structs, mass, mask, temperature=300.0, seed=5, steps=50, timestep=1.0)
    assert np.abs(fwd["positions"] - pos0).max() > 0.05
    eng.set_velocities(-fwd["velocities"])
    back = _md(eng, structs, mass, mask, upload=False, steps=50, timestep=1.0)
    err = np.abs(back["positions"] - pos0).max()
    print(f"time reversal, gan48: max |r - r_start| = {err:.3e} A (bound {100 * GAN48_REVERSAL_RESIDUAL:.1e})")
    assert err <= 100 * GAN48_REVERSAL_RESIDUAL
    eng.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_stops_and_refusals():
    from surface_sampling_amd import backend

    eng = rc.engine("pair_lj")
    structs = [rc.grid("pair_lj", n, 60 + k, [0, 0, 0]) for k, n in enumerate((9, 12, 7))]
    mass, start = _masses(structs), _start(structs)
    held = np.zeros(28, np.uint8)
    held[start[2]:] = 1                                            # the third chain: every atom held
    # n_steps = 0: record 0 only, nothing moves
    z = _md(eng, structs, mass, held, steps=0, timestep=1.0)
    e0, _, f0 = eng.evaluate_f64(structs)
    assert z["epot"].shape == (1, 3) and np.array_equal(z["epot"][0], e0) and list(z["n_done"]) == [0, 0, 0] and list(z["stop_reason"]) == [1, 1, 1]
    assert np.array_equal(z["positions"], np.concatenate([s[1] for s in structs])) and np.array_equal(z["velocities"], z["v0"])
    # a chain with every atom held: temperature 0, no division by zero (the calculators' formula on the engine's numbers)
    ref = _md(eng, structs, mass, held, steps=12, timestep=1.0, thermostat="langevin", friction=0.05)
    assert not ref["ekin"][:, 2].any() and np.array_equal(ref["positions"][start[2]:], structs[2][1]) and ref["n_done"][2] == 12
    # two atoms 1e-150 A apart make the middle chain non-finite at its first evaluation (exactly coincident atoms are no neighbors of
    # each other, nbr_dev.h: they would pass unnoticed): reason 2, nothing moved; its neighbors in the batch finish
    T1, X1, C1, p1 = structs[1]
    X1 = X1.copy()
    X1[0], X1[1] = (0.0, 0.0, 0.0), (1e-150, 0.0, 0.0)
    bad = [structs[0], (T1, X1, C1, p1), structs[2]]
    out = _md(eng, bad, mass, held, steps=12, timestep=1.0, thermostat="langevin", friction=0.05)
    print(f"atoms 1e-150 A apart: n_done {out['n_done']}, stop {out['stop_reason']}, E {out['e']}")
    assert list(out["stop_reason"]) == [1, 2, 1] and list(out["n_done"]) == [12, 0, 12]
    assert np.array_equal(out["positions"][start[1]:start[2]], X1) and np.array_equal(out["velocities"][start[1]:start[2]], out["v0"][start[1]:start[2]])
    assert np.isnan(out["epot"][:, 1]).all() and np.isfinite(out["epot"][:, [0, 2]]).all() and not np.isfinite(out["e"][1])
    for k in ("positions", "velocities", "f"):
        assert np.array_equal(out[k][:start[1]], ref[k][:start[1]]) and np.array_equal(out[k][start[2]:], ref[k][start[2]:]), k
    assert np.array_equal(out["epot"][:, 0], ref["epot"][:, 0])
    # a chain that blows up mid-trajectory goes back to its last completed step: two atoms 30 A apart in an open box feel nothing; one
    # flies at 15 A / fs, stands 15 A away after step 1 and 1e-150 A from the other after step 2
    fly = (np.zeros(2, np.int32), np.array([[-30.0, 0.0, 0.0], [1e-150, 0.0, 0.0]]), np.eye(3) * 80.0, np.zeros(3, np.uint8))
    v_fly = np.zeros((11, 3))
    v_fly[0, 0] = 15.0
    m_fly = np.concatenate([[40.0, 40.0], mass[:9]])
    wild = _md(eng, [fly, structs[0]], m_fly, None, vel=v_fly, steps=4, timestep=1.0)
    print(f"collision: n_done {wild['n_done']}, stop {wild['stop_reason']}, x {wild['positions'][0]}, v {wild['velocities'][0]}")
    assert list(wild["stop_reason"]) == [2, 1] and list(wild["n_done"]) == [1, 4]
    assert np.array_equal(wild["positions"][:2], [[-15.0, 0.0, 0.0], [1e-150, 0.0, 0.0]]) and np.array_equal(wild["velocities"][:2], v_fly[:2])
    assert np.array_equal(wild["epot"][:2, 0], [0.0, 0.0]) and np.isnan(wild["epot"][2:, 0]).all() and wild["e"][0] == 0.0
    assert np.isfinite(wild["f"]).all() and np.isfinite(wild["epot"][:, 1]).all()

    # refusals: each leaves the handle serving the next call with unchanged bits
    good = dict(steps=12, timestep=1.0, thermostat="langevin", friction=0.05)
    for over, msg in ((dict(steps=-1), "n_steps"), (dict(thermo_interval=0), "thermo_interval"), (dict(timestep=0.0), "dt"),
                      (dict(timestep=float("nan")), "dt"), (dict(timestep=float("inf")), "dt"), (dict(friction=0.0), "friction"),
                      (dict(friction=-1.0), "friction"), (dict(temperature=-5.0), "temperature"), (dict(temperature_end=-5.0), "temperature"),
                      (dict(ramp_steps=-1), "ramp_steps")):
        eng.upload(structs)
        eng.draw_velocities(mass, 300.0, seed=7, fixed=held)
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*" + msg):
            eng.md(mass, fixed=held, seed=7, **{**good, "temperature": 300.0, **over})
        again = _md(eng, structs, mass, held, upload=False, **good)
        _assert_equal(again, ref, msg)
    for bad_mass in (0.0, -1.0, float("nan"), float("inf")):
        eng.upload(structs)
        eng.draw_velocities(mass, 300.0, seed=7, fixed=held)
        m2 = mass.copy()
        m2[3] = bad_mass
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*mass of atom 3"):
            eng.md(m2, fixed=held, seed=7, temperature=300.0, **good)
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*mass of atom 3"):
            eng.draw_velocities(m2, 300.0)
        eng.draw_velocities(mass, 300.0, seed=7, fixed=held)
        _assert_equal(_md(eng, structs, mass, held, upload=False, **good), ref, "mass")
    import ctypes as C

    p = backend.MdParams(12, 2, 1, 1.0, 300.0, 300.0, 0.05, 0, 0, 7)      # an unknown thermostat; null parameters; null masses
    lib, h = eng._lib, eng._h
    mp = mass.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.vssr_batch_md(h, C.byref(p), mp, None, None, WANT, None, None, None, None) == -1 and b"thermostat" in lib.vssr_last_error(h)
    assert lib.vssr_batch_md(h, None, mp, None, None, WANT, None, None, None, None) == -1
    p.thermostat = 1
    assert lib.vssr_batch_md(h, C.byref(p), None, None, None, WANT, None, None, None, None) == -1 and b"masses" in lib.vssr_last_error(h)
    assert lib.vssr_batch_md_driver(h, 3, None) == -1
    with pytest.raises(backend.BackendError, match="vssr error -1: .*non-finite velocity"):
        eng.set_velocities(np.full((28, 3), np.nan))
    with pytest.raises(backend.BackendError, match="vssr error -1: .*temperature"):
        eng.draw_velocities(mass, -1.0)
    _assert_equal(_md(eng, structs, mass, held, **good), ref, "after the refusals")
    # state: no velocities after an upload; none on a handle that has no batch
    eng.upload(structs)
    with pytest.raises(backend.BackendError, match="vssr error -5: .*no velocities"):
        eng.md(mass, 5, 1.0)
    with pytest.raises(backend.BackendError, match="vssr error -5: .*no velocities"):
        eng.get_velocities()
    _assert_equal(_md(eng, structs, mass, held, **good), ref, "after the state errors")
    fresh = rc.engine("pair_lj")
    with pytest.raises(backend.BackendError, match="vssr error -5"):
        fresh.set_velocities(None)
    fresh.close()
    eng.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_long_run_kinetic_temperature_agrees_with_the_oracle():
    """64 chains of 27 atoms, Langevin at 300 K for 300 steps of 1 fs: the mean kinetic temperature over the second half, device
    against oracle, within 5 standard errors of the chain-to-chain spread (both sides combined).  Two oracle runs with different seeds
    pass the same comparison on the CPU (tests/test_md_cpu.py)."""
    pos, mass, start, kw = mo.sanity_case()
    structs = [(np.ones(27, np.int32), pos[a0:a1], np.eye(3) * 60.0, np.zeros(3, np.uint8)) for a0, a1 in zip(start[:-1], start[1:])]
    eng = rc.engine("pair_lj")
    dev = _md(eng, structs, mass, None, temperature=300.0, seed=21, steps=kw["n_steps"], timestep=kw["dt"], thermostat="langevin",
              friction=kw["friction"])
    eng.close()
    ora = mo.run(pos, mo.maxwell_boltzmann(mass, start, 300.0, seed=22), mass, start, mo.lj_chains(**mo.LJ11)(27), seed=22, **kw)
    ok, Td, To, se = mo.agree_within(mo.second_half_temperature(dev["ekin"], 27), mo.second_half_temperature(ora["ekin"], 27))
    print(f"second-half kinetic temperature: device {Td:.2f} K, oracle {To:.2f} K, combined standard error {se:.2f} K")
    assert ok
