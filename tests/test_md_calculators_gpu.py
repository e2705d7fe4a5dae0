"""``md_batch`` of the calculators (EnsembleNFFSurface and one of the analytic family) on the device: it returns what the engine
returns, honours ``fixed_indices`` and ``first_chain``, and leaves the calculator's other entry points as they were."""
import numpy as np
import pytest

import md_oracle as mo

pytestmark = pytest.mark.gpu


def _gan_slabs(golden, n=3):
    base = golden.structure("GaN_3x3_pristine")
    out = []
    for k in range(n):
        s = base.copy()
        s.set_positions(base.positions + np.random.default_rng(k).normal(0, 0.03, base.positions.shape))
        out.append(s)
    fixed = [np.flatnonzero(base.positions[:, 2] < base.positions[:, 2].min() + 1.0)] * n
    return out, fixed


def _check_against_engine(calc, eng_structs, slabs, fixed, want):
    from surface_sampling_amd import structures

    kw = dict(steps=8, timestep=0.5, thermostat="langevin", temperature=250.0, temperature_end=400.0, friction=0.03, seed=9, thermo_interval=2)
    res = calc.md_batch(slabs, fixed_indices=fixed, first_chain=40, **kw)
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
    ref = eng.md(mass, 8, 0.5, thermostat="langevin", temperature=250.0, temperature_end=400.0, friction=0.03, seed=9, fixed=mask, chain_id=ids,
                 thermo_interval=2, want=want)
    for b, (r, s) in enumerate(zip(res, slabs)):
        a0, a1 = start[b], start[b + 1]
        assert np.array_equal(r["atoms"].positions, ref["positions"][a0:a1]) and np.array_equal(r["velocities"], ref["velocities"][a0:a1])
        assert np.array_equal(r["epot"], ref["epot"][:, b]) and np.array_equal(r["ekin"], ref["ekin"][:, b])
        assert (r["n_done"], r["stop_reason"]) == (8, 1) and r["epot"].shape == (5,)
        n_free = len(s) - len(fixed[b])
        assert np.array_equal(r["temperature"], 2.0 * r["ekin"] / (3.0 * n_free * mo.KB))
        # fixed_indices: held atoms stay and carry no velocity; the others moved
        assert np.array_equal(r["atoms"].positions[fixed[b]], s.positions[fixed[b]]) and not r["velocities"][fixed[b]].any()
        assert np.abs(r["atoms"].positions - s.positions).max() > 1e-4
        assert np.array_equal(r["atoms"].numbers, s.numbers) and np.array_equal(s.positions, slabs[b].positions)
    # first_chain: slab 1 of that call is global chain 41 -- the same slab first in a batch that starts at 41 gives the same bits,
    # under another chain id it does not
    again = calc.md_batch(slabs[1:], fixed_indices=fixed[1:], first_chain=41, **kw)
    assert np.array_equal(again[0]["atoms"].positions, res[1]["atoms"].positions) and np.array_equal(again[0]["ekin"], res[1]["ekin"])
    other = calc.md_batch(slabs[1:], fixed_indices=fixed[1:], first_chain=0, **kw)
    assert not np.array_equal(other[0]["atoms"].positions, res[1]["atoms"].positions)
    # a chain with every atom held: temperature 0; given velocities and masses are taken as they are
    v = [np.full((len(s), 3), 1e-3) for s in slabs[:1]]
    held = calc.md_batch(slabs[:1], fixed_indices=[np.arange(len(slabs[0]))], velocities=v, masses=[np.full(len(slabs[0]), 10.0)],
                         steps=3, timestep=1.0)
    assert not held[0]["temperature"].any() and not held[0]["velocities"].any() and np.array_equal(held[0]["atoms"].positions, slabs[0].positions)
    nve = calc.md_batch(slabs[:1], velocities=v, masses=[np.full(len(slabs[0]), 10.0)], steps=1, timestep=1.0, thermo_interval=1)
    assert np.isclose(nve[0]["ekin"][0], 0.5 * 10.0 * 3e-6 * len(slabs[0]) / mo.ACC, rtol=1e-12)
    return res


def test_md_batch_of_the_tersoff_calculator(golden):
    from surface_sampling_amd.calculators import TersoffSurfCalc

    slabs, fixed = _gan_slabs(golden)
    calc = TersoffSurfCalc(golden.tersoff_params, ["Ga", "N"], device="cuda:0")
    before = calc.calculate_batch(slabs)
    relaxed_before = calc.relax_batch(slabs, fixed_indices=fixed, relax_steps=5)
    _check_against_engine(calc, [calc._pack(s) for s in slabs], slabs, fixed, 1 | 2 | 16)
    after = calc.calculate_batch(slabs)
    relaxed_after = calc.relax_batch(slabs, fixed_indices=fixed, relax_steps=5)
    for a, b in zip(before, after):
        assert a["energy"] == b["energy"] and np.array_equal(a["forces"], b["forces"])
    for a, b in zip(relaxed_before, relaxed_after):
        assert np.array_equal(a[0].positions, b[0].positions) and a[2] == b[2]


def test_md_batch_of_the_painn_calculator(golden):
    from surface_sampling_amd import structures
    from surface_sampling_amd.calculators import EnsembleNFFSurface

    base = golden.structure("SrTiO3_2x2_pristine")
    slabs = [structures.synth_chain(base, c, grid=(4, 4)) for c in (1, 2, 3)]
    fixed = [np.flatnonzero(s.positions[:, 2] < base.positions[:, 2].max() - 4.0) for s in slabs]
    calc = EnsembleNFFSurface(golden.blobs, device="cuda:0", model_units="kcal/mol", prediction_units="eV", offset_units="atomic")
    calc.set(offset=True, offset_data=golden.offset_data)
    before = calc.calculate_batch(slabs)
    relaxed_before = calc.relax_batch(slabs, fixed_indices=fixed, relax_steps=3, optimizer="BFGS")
    _check_against_engine(calc, [structures.as_arrays(s) for s in slabs], slabs, fixed, 31)
    after = calc.calculate_batch(slabs)
    relaxed_after = calc.relax_batch(slabs, fixed_indices=fixed, relax_steps=3, optimizer="BFGS")
    for a, b in zip(before, after):
        assert np.array_equal(a["energy"], b["energy"]) and np.array_equal(a["forces"], b["forces"])
    for a, b in zip(relaxed_before, relaxed_after):
        assert np.array_equal(a[0].positions, b[0].positions) and a[2] == b[2]
