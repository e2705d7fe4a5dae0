"""The three relaxation front ends of an analytic calculator on the device -- ``relax_batch`` (slab objects), ``evaluate_packed``
(packed arrays) and ``run_lammps_opt`` (one slab) -- give the same chains the same numbers bit for bit, and the device line search
of ``relax_batch`` does not depend on whether a trajectory is recorded.  Potential: ``PairSurfCalc`` with the one-type lj/cut
model of ``tests/pair_cases.py``; batch: open clusters of 2, 7 and 12 atoms, the first atom of each held."""
import numpy as np
import pytest

import pair_cases as pc
from surface_sampling_amd import backend
from surface_sampling_amd.calculators import PairSurfCalc
from surface_sampling_amd.structures import Structure

pytestmark = pytest.mark.gpu

SIZES = (2, 7, 12)
STEPS = 30


@pytest.fixture(scope="module")
def calc():
    c = PairSurfCalc(commands=pc.CUT_LJ, species=["Ar"], device="cuda:0")
    c.set(relax_steps=STEPS)
    yield c
    if c._engine is not None:
        c._engine.close()


@pytest.fixture(scope="module")
def slabs():
    out = []
    for n, seed in zip(SIZES, (71, 72, 73)):
        _, X, cell, pbc = pc.grid_chain(n, seed, [0, 0, 0], n_types=1, spacing=3.7)
        out.append(Structure(np.full(n, 18), X, cell, pbc.astype(bool)))
    return out


FIXED = [[0]] * len(SIZES)


def _packed(slabs):
    n = np.array([len(s) for s in slabs], np.int32)
    mask = np.concatenate([(np.arange(len(s)) == 0) for s in slabs]).astype(np.uint8)
    return (n, np.concatenate([s.numbers for s in slabs]), np.concatenate([s.positions for s in slabs]),
            np.stack([s.cell.reshape(9) for s in slabs]), np.stack([s.pbc for s in slabs]).astype(np.uint8)), mask


@pytest.mark.parametrize("optimizer", ["CG", "FIRE", "BFGS"])
def test_the_three_relaxation_front_ends_agree_bit_for_bit(calc, slabs, optimizer):
    per_slab = calc.relax_batch(slabs, fixed_indices=FIXED, optimizer=optimizer, fmax=0.01)
    arrays, mask = _packed(slabs)
    res = calc.evaluate_packed(*arrays, relax=True, fixed_mask=mask, optimizer=optimizer, fmax=0.01)
    s = res["cfg_start"]
    assert s.tolist() == [0, 2, 9, 21] and not res["oob"].any()
    moved = 0.0
    for b, (slab, (relaxed, traj, energy, oob, r)) in enumerate(zip(slabs, per_slab)):
        a0, a1 = int(s[b]), int(s[b + 1])
        assert traj is None and oob is False and energy == r["energy"] == float(res["energy"][b])
        assert np.array_equal(r["per_atom_energies"], res["energy_atoms"][a0:a1]) and np.array_equal(r["forces"], res["forces"][a0:a1])
        assert np.array_equal(relaxed.positions, res["positions"][a0:a1])
        assert np.array_equal(relaxed.positions[0], slab.positions[0])                      # the held atom
        moved = max(moved, float(np.abs(relaxed.positions - slab.positions).max()))
        alone, e1, ea1 = calc.run_lammps_opt(slab, fixed_indices=FIXED[b], optimizer=optimizer, fmax=0.01)
        assert e1 == energy and np.array_equal(ea1, r["per_atom_energies"]) and np.array_equal(alone.positions, relaxed.positions)
        if optimizer == "CG":
            counts = (int(res["iterations"][b]), int(res["evaluations"][b]), backend.CG_STOP_REASONS[int(res["stop"][b])])
            assert (r["iterations"], r["evaluations"], r["stop"]) == counts
            assert (calc.last_opt["iterations"], calc.last_opt["evaluations"], calc.last_opt["stop"]) == counts
            assert counts[0] >= 1
        else:
            counts = (int(res["n_steps"][b]), bool(res["converged"][b]))
            assert (r["n_steps"], r["converged"]) == counts == (calc.last_opt["iterations"], calc.last_opt["converged"])
            assert counts[0] >= 1
        print(f"{optimizer} chain {b}: E = {energy:.9f} eV, counts {counts}")
    assert moved > 1e-3          # (the clusters were not at rest: the comparison is of relaxations, not of single points)


def test_device_line_search_is_the_same_with_and_without_a_trajectory(calc, slabs):
    k = 2
    plain = calc.relax_batch(slabs, fixed_indices=FIXED, optimizer="BFGSLineSearch", linesearch_driver="device", relax_steps=12, fmax=0.01)
    traced = calc.relax_batch(slabs, fixed_indices=FIXED, optimizer="BFGSLineSearch", linesearch_driver="device", relax_steps=12, fmax=0.01,
                              save_traj=True, record_interval=k)
    for b, (slab, (relaxed, none, energy, oob, r), (relaxed_t, traj, energy_t, oob_t, r_t)) in enumerate(zip(slabs, plain, traced)):
        assert none is None and oob is False and oob_t is False and energy == energy_t
        assert np.array_equal(relaxed.positions, relaxed_t.positions) and np.array_equal(r["forces"], r_t["forces"])
        assert np.array_equal(r["per_atom_energies"], r_t["per_atom_energies"])
        print(f"BFGSLineSearch chain {b}: E = {energy:.9f} eV, steps {r['n_steps']}, evaluations {r['n_eval']}, stop {r['stop_reason']}")
        assert all(r[key] == r_t[key] for key in ("n_steps", "n_eval", "stop_reason", "converged"))
        # the points at which steps 0, k, 2k, ... open
        assert len(traj["atoms"]) == len(traj["energies"]) == len(traj["forces"]) == r["n_steps"] // k + 1
        assert np.array_equal(traj["atoms"][0].positions, slab.positions) and traj["forces"][0].shape == (len(slab), 3)
        assert not np.any(traj["forces"][0][0]) and energy <= traj["energies"][0]
    assert max(t[4]["n_steps"] for t in plain) >= k          # (some trajectory holds more than its starting point)
