"""``npt_batch`` of the calculators (one of the analytic family and EnsembleNFFSurface) on the device: it returns structures that carry
the new cells, matches the engine call it wraps bit for bit, honours ``fixed_indices`` and ``first_chain``, and leaves ``md_batch`` and
the calculator's evaluations as they were."""
import numpy as np
import pytest

import md_oracle as mo

pytestmark = pytest.mark.gpu

KW = dict(steps=6, timestep=0.5, thermostat="langevin", barostat="berendsen", pressure=0.01, compressibility=0.1, taup=20.0, mask=(1, 1, 0),
          temperature=250.0, temperature_end=400.0, friction=0.03, seed=9, thermo_interval=2)


def _check_against_engine(calc, eng_structs, slabs, fixed, want):
    from surface_sampling_amd import structures

    res = calc.npt_batch(slabs, fixed_indices=fixed, first_chain=40, **KW)
    assert len(res) == len(slabs)
    eng = calc._get_engine()
    mass = np.concatenate([structures.masses_of(s) for s in slabs])
    mask = np.zeros(len(mass), np.uint8)
    start = np.concatenate([[0], np.cumsum([len(s) for s in slabs])])
    for b, idx in enumerate(fixed):
        mask[start[b] + idx] = 1
    ids = np.arange(len(slabs), dtype=np.uint64) + 40
    eng.upload(eng_structs)
    eng.draw_velocities(mass, 250.0, seed=9, fixed=mask, chain_id=ids)
    kw = {k: v for k, v in KW.items() if k not in ("steps", "timestep")}
    ref = eng.npt(mass, KW["steps"], KW["timestep"], fixed=mask, chain_id=ids, want=want, **kw)
    for b, (r, s) in enumerate(zip(res, slabs)):
        a0, a1 = start[b], start[b + 1]
        assert np.array_equal(r["atoms"].positions, ref["positions"][a0:a1]) and np.array_equal(r["velocities"], ref["velocities"][a0:a1])
        assert np.array_equal(np.asarray(r["atoms"].cell), ref["cells"][b]) and np.array_equal(r["cell"], ref["cells"][b])
        for k in ("epot", "ekin", "volume", "pressure"):
            assert np.array_equal(r[k], ref[k][:, b]) and r[k].shape == (4,), k
        assert (r["n_done"], r["stop_reason"]) == (6, 1)
        n_free = len(s) - len(fixed[b])
        assert np.array_equal(r["temperature"], 2.0 * r["ekin"] / (3.0 * n_free * mo.KB))
        # the structure that comes back carries the new cell: in plane it moved, the vacuum axis kept its bits; the input is untouched
        c0 = np.asarray(s.cell)
        assert np.abs(r["cell"][:2, :2] - c0[:2, :2]).max() > 1e-5 and np.array_equal(r["cell"][2], c0[2]) and np.array_equal(r["cell"][:, 2], c0[:, 2])
        assert abs(r["volume"][-1] - abs(np.linalg.det(r["cell"]))) < 1e-9 * r["volume"][-1]
        assert not r["velocities"][fixed[b]].any() and np.array_equal(r["atoms"].positions[fixed[b], 2], s.positions[fixed[b], 2])
        assert np.array_equal(r["atoms"].numbers, s.numbers) and np.array_equal(s.positions, slabs[b].positions)
    again = calc.npt_batch(slabs[1:], fixed_indices=fixed[1:], first_chain=41, **KW)
    assert np.array_equal(again[0]["atoms"].positions, res[1]["atoms"].positions) and np.array_equal(again[0]["cell"], res[1]["cell"])
    other = calc.npt_batch(slabs[1:], fixed_indices=fixed[1:], first_chain=0, **KW)
    assert not np.array_equal(other[0]["atoms"].positions, res[1]["atoms"].positions)
    # without couplings: md_batch's trajectory, bit for bit, and the cell it started with
    md = calc.md_batch(slabs[:1], fixed_indices=fixed[:1], steps=4, timestep=0.5, thermostat="nve", temperature=250.0, seed=9, md_driver="lockstep")
    nve = calc.npt_batch(slabs[:1], fixed_indices=fixed[:1], steps=4, timestep=0.5, thermostat="none", barostat="none", temperature=250.0, seed=9)
    assert np.array_equal(md[0]["atoms"].positions, nve[0]["atoms"].positions) and np.array_equal(md[0]["ekin"], nve[0]["ekin"])
    assert np.array_equal(nve[0]["cell"], np.asarray(slabs[0].cell)) and np.isnan(nve[0]["pressure"]).all()
    return res


def test_npt_batch_of_the_tersoff_calculator(golden):
    from surface_sampling_amd.calculators import TersoffSurfCalc

    base = golden.structure("GaN_3x3_pristine")
    slabs = []
    for k in range(3):
        s = base.copy()
        s.set_positions(base.positions + np.random.default_rng(k).normal(0, 0.03, base.positions.shape))
        slabs.append(s)
    fixed = [np.flatnonzero(base.positions[:, 2] < base.positions[:, 2].min() + 1.0)] * 3
    calc = TersoffSurfCalc(golden.tersoff_params, ["Ga", "N"], device="cuda:0")
    before = calc.calculate_batch(slabs)
    _check_against_engine(calc, [calc._pack(s) for s in slabs], slabs, fixed, 1 | 2 | 16)
    for a, b in zip(before, calc.calculate_batch(slabs)):
        assert a["energy"] == b["energy"] and np.array_equal(a["forces"], b["forces"])


def test_npt_batch_of_the_painn_calculator(golden):
    from surface_sampling_amd import structures
    from surface_sampling_amd.calculators import EnsembleNFFSurface

    base = golden.structure("GaN_3x3_pristine")
    slabs = []
    for k in range(2):
        s = base.copy()
        s.set_positions(base.positions + np.random.default_rng(k).normal(0, 0.02, base.positions.shape))
        slabs.append(s)
    fixed = [np.flatnonzero(base.positions[:, 2] < base.positions[:, 2].min() + 1.0)] * 2
    calc = EnsembleNFFSurface(golden.blobs, device="cuda:0", model_units="kcal/mol", prediction_units="eV", offset_units="atomic")
    before = calc.calculate_batch(slabs)
    _check_against_engine(calc, [structures.as_arrays(s) for s in slabs], slabs, fixed, 31)
    for a, b in zip(before, calc.calculate_batch(slabs)):
        assert np.array_equal(a["energy"], b["energy"]) and np.array_equal(a["forces"], b["forces"])
