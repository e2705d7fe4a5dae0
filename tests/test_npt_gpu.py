"""Device constant-pressure MD (vssr_batch_md_npt: csrc/md_npt.hip) against the numpy restatement tests/npt_oracle.py driven by the
device's own single-point energies, forces and stresses; its bits under resume, batching, repetition and a capacity regrow; its stops,
refusals and the state it leaves; and two physical checks.  The measured maxima are in profiles/r36/NOTES_npt.md."""
import numpy as np
import pytest

import cellrelax_cases as cs
import cg_resident_cases as rc
import md_oracle as mo
import npt_cases as nc
import npt_oracle as no
import pair_oracle as po

pytestmark = pytest.mark.gpu

WANT = 1 | 2 | 16   # energy, forces, per-atom energies
KEYS = ("positions", "velocities", "cells", "epot", "ekin", "volume", "pressure", "n_done", "stop_reason", "e", "ea", "f")


def _dev_kw(kw):
    """The oracle's keywords as those of ``engine.npt``."""
    kw = dict(kw)
    kw["steps"], kw["timestep"] = kw.pop("n_steps"), kw.pop("dt")
    kw.pop("cutoff", None)
    return kw


def _npt(eng, structs, mass, fixed=None, vel=None, ids=None, draw_at=300.0, seed=7, upload=True, **kw):
    """Upload, velocities (given, else drawn at ``draw_at``), one npt call; the engine's dict plus what the call left on the device."""
    if upload:
        eng.upload(structs)
        if vel is None:
            eng.draw_velocities(mass, draw_at, seed=seed, fixed=fixed, chain_id=ids)
        else:
            eng.set_velocities(vel)
    v0 = eng.get_velocities()
    out = eng.npt(mass, fixed=fixed, chain_id=ids, seed=seed, want=WANT, **_dev_kw(kw))
    out["v0"], out["counts"], out["regrows"], out["resident_cells"] = v0, eng.last_relax_counts, eng.debug_capacity(), eng.get_cell()
    if hasattr(eng, "results_f64"):
        out["e"], out["ea"], out["f"] = eng.results_f64()
        out["stress"], out["stats"] = eng.stress()[0], eng.stats()          # (vssr_batch_stats: served at once as well)
    return out


def _assert_equal(a, b, tag, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def _device_fn(eng, structs, baro):
    """The device's own single-point evaluation and stress as the oracle's callback: the potential's tolerance does not enter."""
    st = nc.start(structs)

    def fn(pos, cells):
        e, _, f = eng.evaluate_f64([(s[0], pos[st[b]:st[b + 1]], cells[b], s[3]) for b, s in enumerate(structs)])
        return e, f, (eng.stress()[0] if baro else None)
    return fn


def _oracle(fn, structs, mass, v0, fixed, cutoff, seed=7, ids=None, **kw):
    return no.run(np.vstack([s[1] for s in structs]), v0, np.array([s[2] for s in structs]), np.array([s[3] for s in structs]), mass, nc.start(structs),
                  fn, fixed=fixed, cutoff=cutoff, seed=seed, chain_id=ids, **kw)


def _bounds(n, dt, dF, mass, x_scale, c_scale):
    """The rule of tests/test_md_gpu.py: positions within 10 n^2 dt^2 dF / (2 m_min) (dF in eV / A, converted to A / fs^2), velocities
    within the same over n dt; cells to the same RELATIVE bound as the positions (both are multiplied by the same mu)."""
    bx = 10.0 * n * n * dt * dt * dF * mo.ACC / (2.0 * mass.min())
    return bx, bx / (n * dt), bx * c_scale / x_scale


def _compare(tag, dev, ora, n, dt, dF, mass, structs, baro):
    x0, c0 = np.vstack([s[1] for s in structs]), np.array([s[2] for s in structs])
    bx, bv, bc = _bounds(n, dt, dF, mass, np.abs(x0).max(), np.abs(c0).max())
    err = {k: float(np.abs(dev[k] - ora[k]).max()) for k in ("positions", "velocities", "cells")}
    rel = {}
    for k, floor in (("epot", 1.0), ("ekin", 1.0), ("volume", 1.0), ("pressure", 1e-3)):
        if k == "pressure" and not baro:
            assert np.isnan(dev[k]).all() and np.isnan(ora[k]).all()
            continue
        rel[k] = float((np.abs(dev[k] - ora[k]) / np.maximum(np.abs(ora[k]), floor)).max())
    print(f"{tag}: max |device - oracle| positions {err['positions']:.3e} (bound {bx:.3e}) velocities {err['velocities']:.3e} (bound {bv:.3e}) "
          f"cells {err['cells']:.3e} (bound {bc:.3e}); records relative " + " ".join(f"{k} {v:.2e}" for k, v in rel.items()) +
          f"; cells moved {np.abs(dev['cells'] - c0).max():.3e} A")
    assert np.array_equal(dev["n_done"], ora["n_done"]) and np.array_equal(dev["stop_reason"], ora["stop_reason"]), tag
    assert list(dev["n_done"]) == [n] * len(structs) and list(dev["stop_reason"]) == [1] * len(structs), tag
    assert err["positions"] <= bx and err["velocities"] <= bv and err["cells"] <= bc, tag
    assert all(v <= 1e-10 for v in rel.values()), (tag, rel)
    assert np.abs(dev["positions"] - x0).max() > 1e-3
    if baro:
        assert np.abs(dev["cells"] - c0).max() > 1e-4          # the cells did move
    else:
        assert np.array_equal(dev["cells"], c0)
    assert np.array_equal(dev["resident_cells"], dev["cells"])


def _state_afterwards(eng, structs, dev, tag):
    """vssr_batch_results_f64 / vssr_batch_stress served at once equal a fresh upload of the final positions and cells."""
    st = nc.start(structs)
    final = [(s[0], dev["positions"][st[b]:st[b + 1]], dev["cells"][b], s[3]) for b, s in enumerate(structs)]
    e, ea, f = eng.evaluate_f64(final)
    assert np.array_equal(e, dev["e"]) and np.array_equal(f, dev["f"]) and np.array_equal(ea, dev["ea"]), tag
    assert np.array_equal(eng.stress()[0], dev["stress"]), tag
    assert eng.stats() == dev["stats"], tag


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", nc.COMBOS, ids=["-".join(c) for c in nc.COMBOS])
def test_every_coupling_combination_step_for_step_on_a_pair_handle(combo):
    """10 steps of 1 fs on the three skewed, rattled lj/cut chains (8, 12, 27 atoms, two held each) of the cell-relaxation parity test."""
    thermostat, barostat, coupling = combo
    eng = rc.engine("pair_lj")
    structs = cs.parity_structs("pair_lj")
    mass, held = nc.masses(structs), rc.held_first_two(structs)
    n, dt, baro = 10, 1.0, barostat != "none"
    kw = dict(n_steps=n, dt=dt, thermostat=thermostat, barostat=barostat, coupling=coupling, thermo_interval=2, **nc.COUPLING)
    ids = np.array([4, (1 << 40) + 2, 9], np.uint64)
    dev = _npt(eng, structs, mass, held, ids=ids, seed=11, **kw)
    ora = _oracle(_device_fn(eng, structs, baro), structs, mass, dev["v0"], held, 8.0, seed=11, ids=ids, **kw)
    _compare("pair_lj " + " ".join(combo), dev, ora, n, dt, 1e-12, mass, structs, baro)
    h = held.astype(bool)
    assert not dev["velocities"][h].any()
    if not baro:
        assert np.array_equal(dev["positions"][h], np.vstack([s[1] for s in structs])[h])
    _state_afterwards(eng, structs, dev, str(combo))
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _kind_case(kind, golden):
    """(engine, structures, held mask, cutoff, couplings) of one handle kind."""
    from surface_sampling_amd import backend

    if kind == "gan48":          # the Tersoff slabs, open along z: the supported surface case, mask 1 1 0
        structs, mask = rc.gan48(golden)
        structs = [(s[0], s[1], s[2], np.array([1, 1, 0], np.uint8)) for s in structs]
        P = golden.tersoff_params
        return (backend.TersoffEngine(P, device=0), structs, mask, float((P[..., 10] + P[..., 11]).max()),
                dict(thermostat="berendsen", barostat="berendsen", coupling="isotropic", mask=(1, 1, 0)))
    if kind == "pair_born_dsf":
        T, X, C = po.rocksalt(5.64)
        T2, X2, C2 = po.rocksalt(5.75)
        structs = [(T, X + np.random.default_rng(21).normal(0, 0.05, X.shape), C, np.ones(3, np.uint8)),
                   (T2, X2 + np.random.default_rng(22).normal(0, 0.08, X2.shape), C2, np.ones(3, np.uint8))]
        return (rc.engine(kind), structs, rc.held_first_two(structs), po.cutoff(po.model_of(rc.born_dsf_model())[0]),
                dict(thermostat="langevin", barostat="crescale"))
    if kind == "vashishta":      # (3.9 A cells: 2 % and more above the height at which the 7.35 A cutoff needs a third image)
        import pair_cases as pc

        structs = [pc.grid_chain(n, 60 + k, [1, 1, 1], n_types=2, spacing=1.95, jitter=0.08) for k, n in enumerate(cs.PARITY_SIZES)]
    else:
        structs = cs.parity_structs(kind)
    combo = {"sw": dict(thermostat="langevin", barostat="berendsen", coupling="per_axis"),
             "eam_alloy": dict(thermostat="berendsen", barostat="crescale"),
             "adp": dict(thermostat="none", barostat="berendsen", coupling="isotropic", mask=(1, 0, 1)),
             "vashishta": dict(thermostat="berendsen", barostat="berendsen", coupling="per_axis")}[kind]
    return cs.parity_engine(kind, golden), structs, rc.held_first_two(structs), cs.parity_cutoff(kind, golden), combo


@pytest.mark.parametrize("kind", ["gan48", "sw", "eam_alloy", "adp", "vashishta", "pair_born_dsf"])
def test_one_combination_step_for_step_on_every_other_kind(kind, golden):
    eng, structs, held, cutoff, combo = _kind_case(kind, golden)
    mass = nc.masses(structs)
    n, dt = 10, 1.0
    kw = dict(n_steps=n, dt=dt, thermo_interval=5, **{**nc.COUPLING, **combo})
    dev = _npt(eng, structs, mass, held, seed=13, **kw)
    ora = _oracle(_device_fn(eng, structs, True), structs, mass, dev["v0"], held, cutoff, seed=13, **kw)
    _compare(f"{kind} {combo}", dev, ora, n, dt, 1e-12, mass, structs, True)
    if "mask" in combo:          # an axis out of the mask keeps its bits: cell column and the coordinates of held atoms
        ax = combo["mask"].index(0)
        assert np.array_equal(dev["cells"][:, :, ax], np.array([s[2] for s in structs])[:, :, ax])
        assert np.array_equal(dev["positions"][held.astype(bool), ax], np.vstack([s[1] for s in structs])[held.astype(bool), ax])
    _state_afterwards(eng, structs, dev, kind)
    eng.close()


@pytest.mark.parametrize("name", ["GaN_3x3_pristine", "SrTiO3_2x2_pristine"])
def test_painn_follows_the_oracle_on_its_fp32_forces(name, golden):
    """A slab of structures.npz twice (once rattled), 5 steps of 0.5 fs, Langevin with the in-plane Berendsen barostat; dF = one fp32 ulp
    of the largest force component.  The 36-atom GaN slab is the smallest structure of the file and the case of tests/test_md_gpu.py; the
    golden weights were trained on SrTiO3 and give it forces of 1e8 eV / A (dF = 8 eV / A, atoms and cell fly apart), so its bound says
    little.  The 60-atom SrTiO3 slab has forces of 1.4 eV / A: dF = 1.2e-7 eV / A, positions within 2.3e-9 A."""
    from surface_sampling_amd import backend, structures

    S = golden.structure(name)
    if name.startswith("GaN"):
        assert len(S) == min(len(golden.structures[k]) for k in golden.structures.files if k.endswith(".numbers"))
    base = structures.as_arrays(S)
    structs = [base, (base[0], base[1] + np.random.default_rng(1).normal(0, 0.02, base[1].shape), base[2], base[3])]
    eng = backend.PainnEngine(golden.blobs, device=0)
    mass = np.concatenate([structures.masses_of(S)] * 2)
    st = nc.start(structs)
    held = np.concatenate([(S.positions[:, 2] < S.positions[:, 2].min() + 1.0).astype(np.uint8)] * 2)

    def fn(pos, cells):
        r = eng.evaluate([(s[0], pos[st[b]:st[b + 1]], cells[b], s[3]) for b, s in enumerate(structs)])
        return r["energy_f64"], r["forces"].astype(np.float64), eng.stress()[0]

    f0 = np.abs(fn(np.vstack([s[1] for s in structs]), np.array([s[2] for s in structs]))[1]).max()
    n, dt, dF = 5, 0.5, float(np.spacing(np.float32(f0)))
    kw = dict(n_steps=n, dt=dt, thermostat="langevin", barostat="berendsen", mask=(1, 1, 0), **nc.COUPLING)
    eng.upload(structs)
    eng.draw_velocities(mass, 300.0, seed=3, fixed=held, chain_id=[8, 9])
    v0 = eng.get_velocities()
    dev = eng.npt(mass, fixed=held, chain_id=[8, 9], seed=3, **_dev_kw(kw))
    dev["resident_cells"] = eng.get_cell()
    res, stress = eng.download(), eng.stress()[0]
    ora = _oracle(fn, structs, mass, v0, held, 5.0, seed=3, ids=[8, 9], **kw)
    print(f"PaiNN {name}: max |F| {f0:.3f} eV/A, dF {dF:.2e}")
    _compare("PaiNN " + name, dev, ora, n, dt, dF, mass, structs, True)
    assert np.array_equal(dev["cells"][:, 2], np.array([s[2][2] for s in structs])) and not dev["cells"][:, :2, 2].any()
    again = eng.evaluate([(s[0], dev["positions"][st[b]:st[b + 1]], dev["cells"][b], s[3]) for b, s in enumerate(structs)])
    assert np.array_equal(again["forces"], res["forces"]) and np.array_equal(eng.stress()[0], stress)
    eng.close()


def test_an_ewald_handle_serves_thermostats_and_refuses_barostats():
    import ewald_cases as ec
    from surface_sampling_amd import backend, pair

    eng = backend.PairEngine(pair.parse(ec.RAGGED_MODEL, 3), device=0)
    structs = [ec.rattled_cube(), ec.cube()]
    mass, held = nc.masses(structs), rc.held_first_two(structs)
    n, dt = 10, 1.0
    kw = dict(n_steps=n, dt=dt, thermostat="berendsen", thermo_interval=2, **nc.COUPLING)
    dev = _npt(eng, structs, mass, held, seed=5, **kw)
    ora = _oracle(_device_fn(eng, structs, False), structs, mass, dev["v0"], held, 8.0, seed=5, **kw)
    _compare("ewald berendsen thermostat", dev, ora, n, dt, 1e-12, mass, structs, False)
    for barostat in ("berendsen", "crescale"):
        eng.upload(structs)
        eng.set_velocities(dev["v0"])
        with pytest.raises(backend.BackendError, match=r"vssr error -5: .*ew_stride"):
            eng.npt(mass, 3, 1.0, thermostat="berendsen", barostat=barostat, temperature=300.0)
        again = _npt(eng, structs, mass, held, upload=False, seed=5, **kw)
        _assert_equal(again, dev, barostat)
    eng.close()


def test_chains_of_1_255_256_and_257_atoms_in_one_batch():
    eng = rc.engine("pair_lj")
    structs = nc.size_batch()
    assert [len(s[0]) for s in structs] == [1, 255, 256, 257]
    mass = nc.masses(structs)
    held = np.zeros(len(mass), np.uint8)
    held[[1, 300, 600]] = 1
    n, dt = 10, 1.0
    for combo in (dict(thermostat="berendsen", barostat="berendsen", coupling="per_axis"), dict(thermostat="langevin", barostat="crescale")):
        kw = dict(n_steps=n, dt=dt, thermo_interval=5, **{**nc.COUPLING, **combo})
        dev = _npt(eng, structs, mass, held, seed=17, **kw)
        ora = _oracle(_device_fn(eng, structs, True), structs, mass, dev["v0"], held, 8.0, seed=17, **kw)
        _compare(f"sizes {combo}", dev, ora, n, dt, 1e-12, mass, structs, True)
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
LONG = [dict(thermostat="langevin", barostat="crescale"), dict(thermostat="berendsen", barostat="berendsen", coupling="per_axis")]


@pytest.mark.parametrize("combo", LONG, ids=["langevin-crescale", "berendsen-per_axis"])
def test_two_calls_equal_one_repeat_and_a_chain_does_not_depend_on_its_batch(combo):
    eng = rc.engine("pair_lj")
    structs = cs.parity_structs("pair_lj")
    mass, held, st = nc.masses(structs), rc.held_first_two(structs), nc.start(structs)
    ids = np.arange(3, dtype=np.uint64) + 1000
    kw = dict(dt=1.0, thermo_interval=2, **{**nc.COUPLING, "ramp_steps": 20, **combo})
    one = _npt(eng, structs, mass, held, ids=ids, n_steps=20, **kw)
    _assert_equal(_npt(eng, structs, mass, held, ids=ids, n_steps=20, **kw), one, "the same call twice")
    a = _npt(eng, structs, mass, held, ids=ids, n_steps=10, **kw)
    b = _npt(eng, structs, mass, held, ids=ids, n_steps=10, upload=False, step0=10, **kw)      # the state the first call left resident
    assert list(one["stop_reason"]) == [1, 1, 1] and np.array_equal(b["v0"], a["velocities"])
    for k in ("positions", "velocities", "cells", "e", "ea", "f", "stress", "stop_reason"):
        assert np.array_equal(b[k], one[k]), (combo, k)
    for k in ("epot", "ekin", "volume", "pressure"):
        assert np.array_equal(np.concatenate([a[k], b[k][1:]]), one[k]), (combo, k)
    k = 1
    a0, a1 = st[k], st[k + 1]
    alone = _npt(eng, [structs[k]], mass[a0:a1], held[a0:a1], ids=ids[k:k + 1], n_steps=20, **kw)
    for key in ("positions", "velocities", "f", "ea"):
        assert np.array_equal(alone[key], one[key][a0:a1]), key
    for key in ("cells", "e", "stress"):
        assert np.array_equal(alone[key][0], one[key][k]), key
    for key in ("epot", "ekin", "volume", "pressure"):
        assert np.array_equal(alone[key][:, 0], one[key][:, k]), key
    other = _npt(eng, [structs[k]], mass[a0:a1], held[a0:a1], ids=ids[k:k + 1] + 1, n_steps=20, **kw)
    assert not np.array_equal(other["positions"], alone["positions"])      # (another chain id: other velocities to begin with, other noise)
    # later runs use the new cells until the next upload
    eng.set_positions(other["positions"])
    eng.run(WANT)
    e, _, f = eng.results_f64()
    assert np.array_equal(e, other["e"]) and np.array_equal(f, other["f"]) and np.array_equal(eng.get_cell(), other["cells"])
    eng.close()


def test_without_couplings_the_call_leaves_the_bits_of_vssr_batch_md():
    eng = rc.engine("pair_lj")
    structs, held = rc.size_batch("pair_lj")
    mass = nc.masses(structs)
    for th, md_th in (("none", "nve"), ("langevin", "langevin")):
        kw = dict(temperature=300.0, temperature_end=600.0, ramp_steps=12, friction=0.02, thermo_interval=4)
        a = _npt(eng, structs, mass, held, n_steps=12, dt=1.0, thermostat=th, **kw)
        eng.upload(structs)
        eng.set_velocities(a["v0"])
        b = eng.md(mass, 12, 1.0, thermostat=md_th, fixed=held, seed=7, want=WANT, driver="lockstep", **kw)
        for k in ("positions", "velocities", "epot", "ekin", "n_done", "stop_reason"):
            assert np.array_equal(a[k], b[k]), (th, k)
        assert np.array_equal(eng.results_f64()[2], a["f"])
    eng.close()


def test_capacity_regrow_in_the_middle_of_a_trajectory():
    """The 32-atom cube at a = 4.20 A under 60 slots per atom, compressed by the barostat: the fifth neighbor shell enters below 4.11 A,
    an evaluation overflows, the run regrows and ends with the bits of the roomy run (rehearsed in tests/test_npt_cpu.py)."""
    from surface_sampling_amd import backend

    s = cs.compressing_cube()
    structs, mass = [s, s], np.full(64, 39.948)
    out = {}
    for name, slots, tight in (("roomy", cs.ROOMY_SLOTS, -1), ("tight", cs.COMPRESS_SLOTS, 1)):
        eng = backend.PairEngine(cs.LJ, n_types=1, device=0)
        eng.debug_capacity(slots_per_atom=slots, tight=tight)
        out[name] = _npt(eng, structs, mass, draw_at=50.0, **nc.REGROW)
        eng.close()
    roomy, tight = out["roomy"], out["tight"]
    print(f"roomy counts {roomy['counts']} regrows {roomy['regrows']}; tight counts {tight['counts']} regrows {tight['regrows']}; "
          f"a {roomy['cells'][0][0, 0] / 2:.4f} A")
    assert roomy["regrows"] == 0 and tight["regrows"] >= 1 and tight["counts"][0] > roomy["counts"][0] == nc.REGROW["n_steps"] + 1
    assert list(roomy["stop_reason"]) == [1, 1] and roomy["cells"][0][0, 0] / 2 < 4.11
    _assert_equal(tight, roomy, "tight against roomy", KEYS + ("stress",))


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_thin_cell_under_pressure_stops_at_the_state_it_was_evaluated_at():
    from surface_sampling_amd import backend

    eng = backend.PairEngine(cs.LJ_THIN, n_types=1, device=0)
    structs = nc.thin_case()
    mass = np.full(16, 39.948)
    vel = np.zeros((16, 3))
    alone = _npt(eng, structs[1:], mass[8:], vel=vel[8:], ids=[1], **nc.THIN)
    r = _npt(eng, structs, mass, vel=vel, **nc.THIN)
    ora = _oracle(_device_fn(eng, structs, True), structs, mass, vel, None, nc.THIN_CUTOFF, **nc.THIN)
    print(f"thin: steps {r['n_done']}, reasons {r['stop_reason']}, lock-step evaluations {r['counts'][0]}, thin cell lengths {np.linalg.norm(r['cells'][0], axis=1)}")
    assert list(r["stop_reason"]) == [3, 1] and list(r["n_done"]) == [3, nc.THIN["n_steps"]]
    assert np.array_equal(ora["stop_reason"], r["stop_reason"]) and np.array_equal(ora["n_done"], r["n_done"])
    # cell and positions are those of the last evaluation: the oracle's, and the image counts are still those of the upload
    bx, bv, bc = _bounds(8, 1.0, 1e-12, mass, 8.1, 8.1)
    assert np.abs(r["cells"] - ora["cells"]).max() <= bc and np.abs(r["positions"] - ora["positions"]).max() <= bx
    assert np.abs(r["velocities"] - ora["velocities"]).max() <= bv
    assert np.array_equal(no.image_counts(r["cells"][0], [1, 1, 1], nc.THIN_CUTOFF)[0], no.image_counts(structs[0][2], [1, 1, 1], nc.THIN_CUTOFF)[0])
    assert np.isfinite(r["volume"][:4, 0]).all() and np.isnan(r["volume"][4:, 0]).all()
    # the batch is complete ...
    _state_afterwards(eng, structs, r, "thin")
    # ... and the neighbour has the bits it has alone
    for key in ("positions", "velocities", "f", "ea"):
        assert np.array_equal(r[key][8:], alone[key]), key
    for key in ("cells", "n_done", "stop_reason", "e", "stress"):
        assert np.array_equal(r[key][1], alone[key][0]), key
    assert np.array_equal(r["pressure"][:, 1], alone["pressure"][:, 0])
    eng.close()


def test_a_non_finite_evaluation_restores_positions_velocities_and_cell():
    from surface_sampling_amd import backend

    structs, held, terms, cutoff = nc.wall_case()
    eng = backend.PairEngine(terms, n_types=2, device=0)
    mass = nc.masses(structs)
    alone = _npt(eng, structs[1:], mass[9:], ids=[1], seed=3, **nc.WALL)
    r = _npt(eng, structs, mass, held, seed=3, **nc.WALL)
    ora = _oracle(_device_fn(eng, structs, True), structs, mass, r["v0"], held, cutoff, seed=3, **nc.WALL)
    print(f"wall: steps {r['n_done']}, reasons {r['stop_reason']}, lock-step evaluations {r['counts'][0]}, held pair {np.linalg.norm(r['positions'][8] - r['positions'][0]):.4f} A")
    assert list(r["stop_reason"]) == [2, 1] and list(r["n_done"]) == [5, nc.WALL["n_steps"]]
    assert np.array_equal(ora["stop_reason"], r["stop_reason"]) and np.array_equal(ora["n_done"], r["n_done"])
    bx, bv, bc = _bounds(8, 1.0, 1e-12, mass, 8.5, 8.5)
    assert np.abs(r["cells"] - ora["cells"]).max() <= bc and np.abs(r["positions"] - ora["positions"]).max() <= bx
    assert np.abs(r["velocities"] - ora["velocities"]).max() <= bv
    assert np.linalg.norm(r["positions"][8] - r["positions"][0]) > 0.6 and np.abs(r["cells"][0] - structs[0][2]).max() > 1e-2
    assert np.isfinite(r["e"]).all() and np.isfinite(r["f"]).all() and np.isfinite(r["stress"]).all()
    _state_afterwards(eng, structs, r, "wall")
    for key in ("positions", "velocities", "f", "ea"):
        assert np.array_equal(r[key][9:], alone[key]), key
    for key in ("cells", "e", "stress"):
        assert np.array_equal(r[key][1], alone[key][0]), key
    eng.close()
    # non-finite at the very first evaluation (the 1e-150 A pair of tests/test_md_gpu.py): reason 2, nothing moved
    eng = rc.engine("pair_lj")
    structs = [rc.grid("pair_lj", n, 60 + k, [1, 1, 1]) for k, n in enumerate((9, 12))]
    T1, X1, C1, p1 = structs[1]
    X1 = X1.copy()
    X1[0], X1[1] = (0.0, 0.0, 0.0), (1e-150, 0.0, 0.0)
    structs[1] = (T1, X1, C1, p1)
    out = _npt(eng, structs, nc.masses(structs), n_steps=6, dt=1.0, thermostat="langevin", barostat="berendsen", **nc.COUPLING)
    assert list(out["stop_reason"]) == [1, 2] and list(out["n_done"]) == [6, 0]
    assert np.array_equal(out["positions"][9:], X1) and np.array_equal(out["velocities"][9:], out["v0"][9:]) and np.array_equal(out["cells"][1], C1)
    assert np.isnan(out["epot"][:, 1]).all() and np.isfinite(out["epot"][:, 0]).all()
    eng.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    import ctypes as C

    from surface_sampling_amd import backend

    eng = rc.engine("pair_lj")
    structs = cs.parity_structs("pair_lj")[:2]
    mass, held = nc.masses(structs), rc.held_first_two(structs)
    good = dict(n_steps=6, dt=1.0, thermostat="berendsen", barostat="berendsen", **nc.COUPLING)
    ref = _npt(eng, structs, mass, held, **good)
    nan, inf = float("nan"), float("inf")
    bad = [(dict(n_steps=-1), "n_steps"), (dict(thermo_interval=0), "thermo_interval"), (dict(dt=0.0), "dt"), (dict(dt=nan), "dt"),
           (dict(dt=inf), "dt"), (dict(taut=0.0), "taut"), (dict(taut=-1.0), "taut"), (dict(taut=nan), "taut"), (dict(taup=0.0), "taup"),
           (dict(taup=inf), "taup"), (dict(compressibility=0.0), "compressibility"), (dict(compressibility=nan), "compressibility"),
           (dict(pressure=nan), "pressure"), (dict(temperature=-5.0), "temperature"), (dict(temperature_end=-5.0), "temperature"),
           (dict(temperature=inf), "temperature"), (dict(ramp_steps=-1), "ramp_steps"), (dict(thermostat="langevin", friction=0.0), "friction"),
           (dict(thermostat="langevin", friction=nan), "friction"),
           (dict(barostat="crescale", thermostat="none"), "thermostat"), (dict(barostat="crescale", coupling="per_axis"), "isotropic"),
           (dict(barostat="crescale", mask=(1, 1, 0)), "isotropic"), (dict(mask=(0, 0, 0)), "empty mask")]
    for over, msg in bad:
        eng.upload(structs)
        eng.set_velocities(ref["v0"])
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*" + msg):
            eng.npt(mass, fixed=held, seed=7, **_dev_kw({**good, **over}))
        _assert_equal(_npt(eng, structs, mass, held, upload=False, **good), ref, msg)
    # what the Python side cannot send: a mask entry of 2, unknown codes, null parameters, null masses, a bad mass
    lib, h = eng._lib, eng._h
    mp = mass.ctypes.data_as(C.POINTER(C.c_double))
    eng.upload(structs)
    eng.set_velocities(ref["v0"])
    for field, value, msg in (("mask", (C.c_int32 * 3)(1, 2, 1), b"mask[1]"), ("thermostat", 3, b"thermostat"), ("barostat", 3, b"barostat"),
                              ("coupling", 2, b"coupling"), ("thermostat", -1, b"thermostat")):
        p = backend.npt_params(**_dev_kw(good))
        setattr(p, field, value)
        assert lib.vssr_batch_md_npt(h, C.byref(p), mp, None, None, WANT, None, None, None, None, None) == -1 and msg in lib.vssr_last_error(h), field
    p = backend.npt_params(**_dev_kw(good))
    assert lib.vssr_batch_md_npt(h, None, mp, None, None, WANT, None, None, None, None, None) == -1 and b"null parameters" in lib.vssr_last_error(h)
    assert lib.vssr_batch_md_npt(h, C.byref(p), None, None, None, WANT, None, None, None, None, None) == -1 and b"masses" in lib.vssr_last_error(h)
    m2 = mass.copy()
    m2[3] = 0.0
    with pytest.raises(backend.BackendError, match=r"vssr error -1: .*mass of atom 3"):
        eng.npt(m2, fixed=held, seed=7, **_dev_kw(good))
    _assert_equal(_npt(eng, structs, mass, held, upload=False, **good), ref, "after the raw refusals")
    # open axes: a slab p p f is served with mask 1 1 0, refused with z masked in, refused by the isotropic stochastic rescaling; a
    # sheared open vector is refused
    slab = cs.slab()
    lj = backend.PairEngine(cs.LJ, n_types=1, device=0)
    ms, hs = np.full(24, 39.948), (np.arange(24) < 8).astype(np.uint8)
    ok = _npt(lj, [slab], ms, hs, **{**good, "mask": (1, 1, 0)})
    assert ok["stop_reason"][0] == 1 and np.array_equal(ok["cells"][0][2], slab[2][2]) and np.array_equal(ok["positions"][:, 2][:8], slab[1][:8, 2])
    assert abs(ok["cells"][0][0, 0] - slab[2][0, 0]) > 1e-4
    sheared = (slab[0], slab[1], slab[2] + np.array([[0, 0, 0], [0, 0, 0], [0.5, 0, 0]]), slab[3])
    tilted = (slab[0], slab[1], slab[2] + np.array([[0, 0, 0.3], [0, 0, 0], [0, 0, 0]]), slab[3])
    for s, over, msg in ((slab, dict(mask=(1, 1, 1)), r"open along axis 2 .*mask\[2\]"), (slab, dict(mask=(0, 0, 1)), r"mask\[2\]"),
                         (slab, dict(barostat="crescale"), "open along axis 2"), (sheared, dict(mask=(1, 1, 0)), "does not lie"),
                         (tilted, dict(mask=(1, 1, 0)), "lattice vector 0 has the component")):
        lj.upload([s])
        lj.set_velocities(ok["v0"])
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*" + msg):
            lj.npt(ms, fixed=hs, seed=7, **_dev_kw({**good, **over}))
        assert np.array_equal(lj.get_cell()[0], s[2])
    _assert_equal(_npt(lj, [slab], ms, hs, **{**good, "mask": (1, 1, 0)}), ok, "after the open-axis refusals")
    lj.close()
    # state: no velocities after an upload; no batch at all
    eng.upload(structs)
    with pytest.raises(backend.BackendError, match="vssr error -5: .*no velocities"):
        eng.npt(mass, **_dev_kw(good))
    _assert_equal(_npt(eng, structs, mass, held, **good), ref, "after the state error")
    fresh = rc.engine("pair_lj")
    assert fresh._lib.vssr_batch_md_npt(fresh._h, C.byref(p), mp, None, None, WANT, None, None, None, None, None) == -5
    fresh.close()
    eng.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_stochastic_cell_rescaling_samples_the_ideal_gas_volume_on_the_device():
    """The case of tests/test_npt_cpu.py on a pair handle with zero well depth and a 1 A cutoff: 1024 chains of 8 atoms, the same
    parameters and the same bound of 5 standard errors of the 1024-chain mean."""
    from surface_sampling_amd import backend

    pos, cells, mass, start, kw, (v_mean, se) = no.ideal_gas_case(seed=6)
    eng = backend.PairEngine([(0, 0, "lj/cut", (0.0, 0.5), 1.0, 0)], n_types=1, device=0)
    structs = [(np.zeros(8, np.int32), pos[a0:a1], cells[b], np.ones(3, np.uint8)) for b, (a0, a1) in enumerate(zip(start[:-1], start[1:]))]
    seed = kw.pop("seed")
    dev = _npt(eng, structs, mass, draw_at=kw["temperature"], seed=seed, **kw)
    V = dev["volume"][-1]
    d = (V.mean() - v_mean) / se
    print(f"ideal gas on the device: <V> {V.mean():.2f} A^3 (wanted {v_mean:.1f}, standard error {se:.2f}): {d:+.2f} standard errors; std V {V.std(ddof=1):.1f}; "
          f"lock-step evaluations {dev['counts'][0]}")
    assert list(np.unique(dev["stop_reason"])) == [1] and not dev["f"].any() and not dev["epot"][-1].any()      # no chain reached the image-count stop
    assert np.allclose(V, np.abs(np.linalg.det(dev["cells"])), rtol=1e-12)
    assert abs(d) <= 5.0
    eng.close()


def test_the_fcc_cell_reaches_its_target_pressure_and_the_volume_of_the_cell_relaxation():
    """4-atom fcc under lj/cut, T = 0, zero velocities, Berendsen isotropic with beta = 1 / K of the numpy restatement and
    dt / taup = 0.1: after 100 steps |P - P0| <= 1e-3 of its start; the volume agrees with the hydrostatic cell relaxation under P0
    to (the two pressure residuals) / K."""
    from surface_sampling_amd import backend

    F = no.FCC
    P_start, K = no.lj_fcc_pressure_and_modulus(F["a0"], **F)
    pos, cell = no.fcc_cell(F["a0"])
    s = (np.zeros(4, np.int32), pos, cell, np.ones(3, np.uint8))
    eng = backend.PairEngine([(0, 0, "lj/cut", (F["eps"], F["sigma"]), F["rc"], 0)], n_types=1, device=0)
    r = _npt(eng, [s], np.full(4, 39.948), vel=np.zeros((4, 3)), n_steps=100, dt=1.0, barostat="berendsen", taup=10.0, compressibility=1.0 / K,
             pressure=no.FCC_P0)
    P = r["pressure"][:, 0]
    ratio = abs(P[-1] - no.FCC_P0) / abs(P[0] - no.FCC_P0)
    print(f"fcc: a {F['a0']} -> {r['cells'][0][0, 0]:.6f} A, P {P[0]:.5e} (restatement {P_start:.5e}) -> {P[-1]:.6e}, |P - P0| ratio {ratio:.2e}")
    assert r["stop_reason"][0] == 1 and abs(P[0] - P_start) < 1e-6 and ratio <= 1e-3
    # (the lattice sums of the forces cancel to rounding, not to the bit: velocities of 1e-20 A / fs)
    assert np.abs(r["velocities"]).max() < 1e-15 and np.allclose(r["positions"], pos * (r["cells"][0][0, 0] / F["a0"]), atol=1e-9)
    eng.upload([s])
    rel = eng.relax_cell(max_steps=400, fmax=1e-5, hydrostatic_strain=True, scalar_pressure=no.FCC_P0, want=WANT)
    p_rel = -eng.stress()[0][0, :3].mean()
    V_npt, V_rel = r["volume"][-1, 0], abs(np.linalg.det(rel["cells"][0]))
    bound = (abs(P[-1] - no.FCC_P0) + abs(p_rel - no.FCC_P0)) / K
    print(f"volume: NPT {V_npt:.6f}, cell relaxation {V_rel:.6f} A^3 ({rel['n_steps'][0]} steps, reason {rel['stop_reason'][0]}, residual {abs(p_rel - no.FCC_P0):.2e}); "
          f"relative difference {abs(V_npt - V_rel) / V_rel:.2e} (bound {bound:.2e})")
    assert rel["stop_reason"][0] == 1 and abs(V_npt - V_rel) / V_rel <= bound
    eng.close()
