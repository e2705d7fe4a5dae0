"""The calculators' front-end paths pinned without a device: a recording fake analytic engine under a minimal ``_AnalyticSurfCalc``
(and a ``LAMMPSSurfCalc`` with its default bulk group), and a recording fake PaiNN engine under ``EnsembleNFFSurface``.  The fakes
compute every output from their inputs chain by chain (integer-valued coordinates, binary fractions: all sums are exact) and log
the packed-array engine calls -- the struct-list forms delegate through ``backend.pack_batch`` as the real engines' do -- with
every argument resolved, so a default that is spelled out and one that is left out give the same entry.  The expected logs are
literal.  Pinned: (a) the engine calls of every public method per optimizer name and kind of ``fixed_indices``; (b) equal numbers
from ``relax_batch``, ``evaluate_packed`` and a per-chain ``run_lammps_opt``; (c) the +-1000 guard at each of its conditions, equal
between the per-slab and the packed methods, with an empty chain in the batch; (d) the Z -> type error; (e) ``relax_batch``'s
signature names ``optimizer``."""
import inspect
import re

import numpy as np
import pytest

from surface_sampling_amd import backend, calculators, structures

WANT_F64 = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
BFGSLS = "BFGSLineSearch"


def _start(n_atoms):
    return np.concatenate([[0], np.cumsum(np.asarray(n_atoms, dtype=np.int64))]).astype(np.int64)


def _per_chain(w, n_atoms):
    s = _start(n_atoms)
    return np.array([w[s[b]:s[b + 1]].sum() for b in range(len(s) - 1)], dtype=np.float64)


def _mask(fixed):
    return None if fixed is None else [int(x) for x in np.asarray(fixed).reshape(-1)]


def _moved(pos, fixed):
    free = np.ones(len(pos)) if fixed is None else 1.0 - np.asarray(fixed, dtype=np.float64)
    return np.asarray(pos, dtype=np.float64).reshape(-1, 3) + 0.5 * free[:, None]


def _fake_traj(n_atoms, pos, record_interval):
    B, N = len(n_atoms), len(pos)
    return {"n_records": np.asarray(n_atoms, np.int32) % 2 + 1, "positions": np.stack([pos, pos + 1.0]),
            "forces": np.ones((2, N, 3), np.float32), "energies": np.arange(2.0 * B).reshape(2, B), "record_interval": int(record_interval)}


class FakeAnalyticEngine:
    """fp64 engine: E_b = sum over the chain of (x + y + z + type / 4), e_atom the summands, F = 1/2 - pos / 8; a relaxation moves
    every free atom by +1/2 in x, y and z.  ``tamper(e, ea, f)`` edits an evaluation's results in place."""

    def __init__(self):
        self.log, self.tamper, self.last_relax_counts = [], None, (7, 11)

    def _results(self, n_atoms, T, pos):
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        ea = pos.sum(axis=1) + 0.25 * np.asarray(T, dtype=np.float64)
        e, f = _per_chain(ea, n_atoms), 0.5 - 0.125 * pos
        if self.tamper is not None:
            self.tamper(e, ea, f)
        return e, ea, f

    def _batch(self, n_atoms, T, pos, cell, pbc):
        n_atoms, T, pos = np.asarray(n_atoms), np.asarray(T), np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        assert n_atoms.dtype == np.int32 and len(T) == len(pos) == int(n_atoms.sum())
        assert np.asarray(cell).size == 9 * len(n_atoms) and np.asarray(pbc).size == 3 * len(n_atoms)
        self._resident = (n_atoms, T, pos)
        return [int(n) for n in n_atoms], [int(t) for t in T], float(pos.sum()), [int(x) for x in np.asarray(pbc).reshape(-1)]

    # packed-array calls: logged
    def upload_arrays(self, n_atoms, T, pos, cell, pbc):
        self.log.append(("upload_arrays", *self._batch(n_atoms, T, pos, cell, pbc)))

    def evaluate_arrays_f64(self, n_atoms, T, pos, cell, pbc, want=WANT_F64):
        self.log.append(("evaluate_arrays_f64", *self._batch(n_atoms, T, pos, cell, pbc), int(want)))
        return self._results(n_atoms, T, pos)

    def relax_arrays_f64(self, n_atoms, T, pos, cell, pbc, fixed=None, max_steps=100, fmax=0.01, optimizer="FIRE"):
        self.log.append(("relax_arrays_f64", *self._batch(n_atoms, T, pos, cell, pbc), _mask(fixed),
                         {"max_steps": max_steps, "fmax": fmax, "optimizer": optimizer}))
        if any(k in str(optimizer) for k in (BFGSLS, "CG", "LAMMPS")):   # (backend._Handle.relax)
            raise backend.BackendError(f"optimizer {optimizer!r} is not available on the device (FIRE and BFGS are)")
        new = _moved(pos, fixed)
        n = np.asarray(n_atoms, np.int32)
        return (*self._results(n_atoms, T, new), new, n + 3, n % 2 == 0)

    def relax_cg_arrays_f64(self, n_atoms, T, pos, cell, pbc, fixed=None, max_iter=100, max_eval=10000, etol=1e-5, ftol=1e-5, dmax=0.1,
                            rerun=True, driver="auto"):
        backend.cg_driver_code(driver)
        self.log.append(("relax_cg_arrays_f64", *self._batch(n_atoms, T, pos, cell, pbc), _mask(fixed),
                         {"max_iter": max_iter, "max_eval": max_eval, "etol": etol, "ftol": ftol, "dmax": dmax, "rerun": rerun,
                          "driver": driver}))
        new = _moved(pos, fixed)
        n = np.asarray(n_atoms, np.int32)
        return (*self._results(n_atoms, T, new), new, n + 1, n + 2, n % 3 + 1)

    def relax_bfgs_linesearch(self, fixed=None, max_steps=20, fmax=0.01, max_eval=None, want=backend.WANT_ALL, params=None, record_interval=0):
        self.log.append(("relax_bfgs_linesearch", _mask(fixed), {"max_steps": max_steps, "fmax": fmax, "max_eval": max_eval,
                                                                   "want": int(want), "record_interval": record_interval}))
        n_atoms, T, pos = self._resident
        new = _moved(pos, fixed)
        self._resident = (n_atoms, T, new)
        why = n_atoms % 2 + 1
        out = {"positions": new, "n_steps": n_atoms + 4, "converged": why == 1, "n_eval": n_atoms + 5, "stop_reason": why}
        if record_interval:
            out["traj"] = _fake_traj(n_atoms, new, record_interval)
        return out

    def results_f64(self):
        self.log.append(("results_f64",))
        return self._results(*self._resident)

    def stress(self):
        self.log.append(("stress",))
        B = len(self._resident[0])
        return np.arange(6.0 * B).reshape(B, 6), np.zeros((B, 6))

    # struct-list calls: the real engines' delegations
    def upload(self, structs):
        self.upload_arrays(*backend.pack_batch(structs))

    def evaluate_f64(self, structs, want=WANT_F64):
        return self.evaluate_arrays_f64(*backend.pack_batch(structs), want=want)

    def relax_f64(self, structs, fixed=None, max_steps=100, fmax=0.01, optimizer="FIRE"):
        return self.relax_arrays_f64(*backend.pack_batch(structs), fixed=fixed, max_steps=max_steps, fmax=fmax, optimizer=optimizer)

    def relax_cg_f64(self, structs, fixed=None, max_iter=100, max_eval=10000, etol=1e-5, ftol=1e-5, dmax=0.1, rerun=True, driver="auto"):
        backend.cg_driver_code(driver)
        return self.relax_cg_arrays_f64(*backend.pack_batch(structs), fixed=fixed, max_iter=max_iter, max_eval=max_eval, etol=etol,
                                        ftol=ftol, dmax=dmax, rerun=rerun, driver=driver)

    def close(self):
        pass


class Calc(calculators._AnalyticSurfCalc):
    species = ["Ga", "N"]

    def __init__(self, **kwargs):
        self.fake = FakeAnalyticEngine()
        self._init_common("cuda:0", False, None)
        super().__init__(**kwargs)

    def _make_engine(self):
        return self.fake


class BulkCalc(calculators.LAMMPSSurfCalc):
    """``LAMMPSSurfCalc`` as a run directory with ``atoms: [Ga, N]``, ``bulk_index: 2`` and ``pair_style tersoff`` configures it."""

    def __init__(self, **kwargs):
        self.fake = FakeAnalyticEngine()
        super().__init__(device="cuda:0", **kwargs)
        self.species, self.bulk_index, self.pair_style = ["Ga", "N"], 2, "tersoff"

    def _configure(self):
        pass

    def _make_engine(self):
        return self.fake


def chains(sizes=(2, 5, 3)):
    """Chain b: atoms i at (i, b, 1), Ga and N alternating (types 0, 1), periodic in x and y."""
    return [structures.Structure(np.where(np.arange(n) % 2 == 0, 31, 7), np.array([[i, b, 1.0] for i in range(n)]).reshape(-1, 3),
                                 np.eye(3) * 20.0, [True, True, False]) for b, n in enumerate(sizes)]


def packed(slabs):
    return backend.pack_batch([structures.as_arrays(a) for a in slabs])


# the batch (2, 5, 3) as the fakes log it: n_atoms, types, sum of all coordinates, pbc (Calc: the atoms' own; BulkCalc: p p p)
N3, T3, SUM3 = [2, 5, 3], [0, 1, 0, 1, 0, 1, 0, 0, 1, 0], 35.0
PBC3, PPP3 = [1, 1, 0] * 3, [1, 1, 1] * 3
ONE = {0: ([2], [0, 1], 3.0), 1: ([5], [0, 1, 0, 1, 0], 20.0), 2: ([3], [0, 1, 0], 12.0)}      # its chains alone
# fixed_indices -> the mask the engine must see
FIXED = {
    "none": (None, None),
    "holes": ([None, [], [0, 2]], [0, 0, 0, 0, 0, 0, 0, 1, 0, 1]),
    "full": ([[1], [0, 4], [0, 1, 2]], [0, 1, 1, 0, 0, 0, 1, 1, 1, 1]),
}
BULK3 = [1, 1, 1, 1, 0, 0, 0, 1, 1, 0]        # bulk_index 2: the first two atoms of every slab
CG_KW = {"max_iter": 100, "max_eval": 10000, "etol": 1e-5, "ftol": 1e-5, "dmax": 0.1, "rerun": True, "driver": "auto"}


def relax_entries(optimizer, mask, pbc=PBC3, batch=(N3, T3, SUM3), steps=100, fmax=0.01, record_interval=0, linesearch="ase"):
    """The engine calls of one relaxation of ``batch``: the optimizer table as the calculators document it."""
    if optimizer.upper() in ("CG", "LAMMPS"):
        return [("relax_cg_arrays_f64", *batch, pbc, mask, {**CG_KW, "max_iter": steps})]
    if optimizer == BFGSLS and linesearch == "device":
        return [("upload_arrays", *batch, pbc),
                ("relax_bfgs_linesearch", mask, {"max_steps": steps, "fmax": fmax, "max_eval": None, "want": WANT_F64,
                                                 "record_interval": record_interval}),
                ("results_f64",)]
    return [("relax_arrays_f64", *batch, pbc, mask, {"max_steps": steps, "fmax": fmax, "optimizer": optimizer})]


# ---- (a) engine calls --------------------------------------------------------------------------------------------------------------
def test_single_point_methods_call_one_evaluation():
    calc, slabs = Calc(), chains()
    calc.calculate(slabs[1], properties=("energy", "forces"))
    assert calc.fake.log == [("evaluate_arrays_f64", [5], [0, 1, 0, 1, 0], 20.0, [1, 1, 0], WANT_F64)]
    assert calc.results["energy"] == 20.5 and calc.results["forces"].shape == (5, 3) and "stress" not in calc.results
    calc.fake.log.clear()
    calc.calculate(slabs[1], properties=("energy", "stress", "surface_energy"))
    assert calc.fake.log == [("evaluate_arrays_f64", [5], [0, 1, 0, 1, 0], 20.0, [1, 1, 0], WANT_F64), ("stress",)]
    assert calc.results["surface_energy"] == 20.5 and np.array_equal(calc.results["stress"], np.arange(6.0))
    calc.fake.log.clear()
    calc.calculate(slabs[1])          # the default properties hold "relaxed_energy": run_lammps_opt with its defaults follows
    assert calc.fake.log == [("evaluate_arrays_f64", [5], [0, 1, 0, 1, 0], 20.0, [1, 1, 0], WANT_F64),
                             ("relax_cg_arrays_f64", [5], [0, 1, 0, 1, 0], 20.0, [1, 1, 0], None, CG_KW)]
    assert calc.results["energy"] == 20.5 and calc.results["relaxed_energy"] == 28.0 and "stress" not in calc.results
    calc.fake.log.clear()
    slab, e, ea = calc.run_lammps_energy(slabs[0])
    assert calc.fake.log == [("evaluate_arrays_f64", [2], [0, 1], 3.0, [1, 1, 0], WANT_F64)]
    assert slab is slabs[0] and e == 3.25 and np.array_equal(ea, [1.0, 2.25])
    calc.fake.log.clear()
    out = calc.calculate_batch(slabs)
    assert calc.fake.log == [("evaluate_arrays_f64", N3, T3, SUM3, PBC3, WANT_F64)]
    assert [r["energy"] for r in out] == [3.25, 20.5, 12.25] and [sorted(r) for r in out] == [["energy", "forces", "per_atom_energies"]] * 3
    assert [r["forces"].shape for r in out] == [(2, 3), (5, 3), (3, 3)] and np.array_equal(out[2]["per_atom_energies"], [3.0, 4.25, 5.0])
    calc.fake.log.clear()
    out = calc.calculate_batch(slabs, want_stress=True)
    assert calc.fake.log == [("evaluate_arrays_f64", N3, T3, SUM3, PBC3, WANT_F64), ("stress",)]
    assert np.array_equal(out[1]["stress"], np.arange(6.0, 12.0))
    calc.fake.log.clear()
    out = calc.evaluate_packed(*packed(slabs))
    assert calc.fake.log == [("evaluate_arrays_f64", N3, T3, SUM3, PBC3, WANT_F64)]
    assert sorted(out) == ["cfg_start", "energy", "energy_atoms", "energy_std", "forces", "oob", "positions", "saturated"]
    assert np.array_equal(out["energy"], [3.25, 20.5, 12.25]) and np.array_equal(out["cfg_start"], [0, 2, 7, 10])
    assert out["cfg_start"].dtype == np.int64 and out["oob"].dtype == bool and not out["oob"].any() and out["saturated"].dtype == bool
    bulk = BulkCalc()                 # the template's boundary p p p; single points hold nothing
    bulk.calculate_batch(slabs)
    bulk.run_lammps_energy(slabs[0])
    bulk.evaluate_packed(*packed(slabs))
    assert bulk.fake.log == [("evaluate_arrays_f64", N3, T3, SUM3, PPP3, WANT_F64), ("evaluate_arrays_f64", [2], [0, 1], 3.0, [1, 1, 1], WANT_F64),
                             ("evaluate_arrays_f64", N3, T3, SUM3, PPP3, WANT_F64)]


@pytest.mark.parametrize("fixed", ["none", "holes", "full"])
@pytest.mark.parametrize("optimizer", ["CG", "LAMMPS", "cg", "FIRE", "BFGS"])
def test_relaxations_call_the_engine_once_per_request(optimizer, fixed):
    indices, mask = FIXED[fixed]
    calc, slabs = Calc(), chains()
    out = calc.relax_batch(slabs, fixed_indices=indices, optimizer=optimizer)
    assert calc.fake.log == relax_entries(optimizer, mask)
    assert len(out) == 3 and all(len(t) == 5 and t[1] is None for t in out)
    calc.fake.log.clear()
    calc.relax_batch(slabs, fixed_indices=indices, optimizer=optimizer, relax_steps=7, fmax=0.25, want_stress=True, etol=1e-3, ftol=1e-4,
                     cg_driver="lockstep", ignored_keyword=1)
    cg = optimizer.upper() in ("CG", "LAMMPS")
    assert calc.fake.log == ([("relax_cg_arrays_f64", N3, T3, SUM3, PBC3, mask, {**CG_KW, "max_iter": 7, "etol": 1e-3, "ftol": 1e-4,
                                                                                  "driver": "lockstep"})] if cg else
                             [("relax_arrays_f64", N3, T3, SUM3, PBC3, mask, {"max_steps": 7, "fmax": 0.25, "optimizer": optimizer})]) \
        + [("stress",)]
    calc.fake.log.clear()
    n, Z, pos, cell, pbc = packed(slabs)
    res = calc.evaluate_packed(n, Z, pos, cell, pbc, relax=True, fixed_mask=None if mask is None else np.array(mask, np.uint8),
                               optimizer=optimizer)
    assert calc.fake.log == relax_entries(optimizer, mask)
    assert sorted(res) == sorted(["cfg_start", "energy", "energy_atoms", "energy_std", "forces", "oob", "positions", "saturated"]
                                 + (["iterations", "evaluations", "stop", "lockstep_evaluations", "dispatched_chain_evaluations"] if cg
                                    else ["n_steps", "converged"]))
    if cg:
        assert (res["lockstep_evaluations"], res["dispatched_chain_evaluations"]) == (7, 11)
    calc.fake.log.clear()
    for b, slab in enumerate(slabs):
        calc.run_lammps_opt(slab, fixed_indices=indices if indices is None else indices[b], optimizer=optimizer)
    one_mask = [None] * 3 if mask is None else [mask[0:2], mask[2:7], mask[7:10]]
    if fixed == "holes":
        one_mask[0] = one_mask[1] = None          # (one slab's None / empty list: no mask at all)
    assert calc.fake.log == [e for b in range(3) for e in relax_entries(optimizer, one_mask[b], [1, 1, 0], ONE[b])]
    assert calc.last_opt == ({"optimizer": "CG", "iterations": 4, "evaluations": 5, "stop": "energy tolerance"} if cg else
                             {"optimizer": optimizer, "iterations": 6, "converged": False})


@pytest.mark.parametrize("fixed", ["none", "holes", "full"])
def test_device_line_search_is_chosen_by_relax_batch_alone(fixed):
    indices, mask = FIXED[fixed]
    calc, slabs = Calc(), chains()
    out = calc.relax_batch(slabs, fixed_indices=indices, optimizer=BFGSLS, linesearch_driver="device", relax_steps=9, fmax=0.125)
    assert calc.fake.log == relax_entries(BFGSLS, mask, steps=9, fmax=0.125, linesearch="device")
    assert [t[1] for t in out] == [None] * 3
    assert [{k: t[4][k] for k in ("n_steps", "n_eval", "stop_reason", "converged")} for t in out] == [
        {"n_steps": 6, "n_eval": 7, "stop_reason": 1, "converged": True}, {"n_steps": 9, "n_eval": 10, "stop_reason": 2, "converged": False},
        {"n_steps": 7, "n_eval": 8, "stop_reason": 2, "converged": False}]
    calc.fake.log.clear()
    calc.set(linesearch_driver="device")          # the setting instead of the keyword; a trajectory; an evaluation budget
    out = calc.relax_batch(slabs, fixed_indices=indices, optimizer=BFGSLS, save_traj=True, record_interval=3, max_eval=40)
    assert calc.fake.log == [("upload_arrays", N3, T3, SUM3, PBC3),
                             ("relax_bfgs_linesearch", mask, {"max_steps": 100, "fmax": 0.01, "max_eval": 40, "want": WANT_F64, "record_interval": 3}),
                             ("results_f64",)]
    assert [len(t[1]["atoms"]) for t in out] == [1, 2, 2] and [t[1]["energies"] for t in out] == [[0.0], [1.0, 4.0], [2.0, 5.0]]
    assert all(f.calc is None and len(f) == len(s) for t, s in zip(out, slabs) for f in t[1]["atoms"])
    assert np.array_equal(out[1][1]["atoms"][1].positions, out[1][0].positions + 1.0) and out[2][1]["forces"][0].shape == (3, 3)
    calc.fake.log.clear()
    out = calc.relax_batch(slabs, fixed_indices=indices, optimizer=BFGSLS, record_interval=3)      # (save_traj is what records)
    assert calc.fake.log[1][2]["record_interval"] == 0 and [t[1] for t in out] == [None] * 3
    # the other methods never take the device line search, whatever the setting: the engine refuses the name
    for call in (lambda: calc.run_lammps_opt(slabs[1], optimizer=BFGSLS),
                 lambda: Calc().relax_batch(slabs, optimizer=BFGSLS)):
        with pytest.raises(backend.BackendError, match="not available on the device"):
            call()
    calc.fake.log.clear()
    assert not calc.packed_supported(True, BFGSLS)
    with pytest.raises(backend.BackendError, match="evaluate_packed relaxes on the device only"):
        calc.evaluate_packed(*packed(slabs), relax=True, optimizer=BFGSLS, linesearch_driver="device")
    assert calc.fake.log == []
    with pytest.raises(ValueError, match="linesearch driver"):
        calc.relax_batch(slabs, optimizer="FIRE", linesearch_driver="host")


def test_packed_supported_answers():
    for cls in (Calc, BulkCalc, calculators._AnalyticSurfCalc):
        assert [cls.packed_supported(True, o) for o in ("CG", "LAMMPS", "cg", "FIRE", "BFGS", None, BFGSLS, "MDMin", FakeAnalyticEngine)] \
            == [True, True, True, True, True, True, False, False, False]
        assert cls.packed_supported(False, BFGSLS) and cls.packed_supported(False, FakeAnalyticEngine)
    ps = calculators.EnsembleNFFSurface.packed_supported
    assert [ps(True, o) for o in ("FIRE", "BFGS", None, "MDMin", "CG", "LAMMPS", BFGSLS, FakeAnalyticEngine)] \
        == [True, True, True, True, False, False, False, False]
    assert ps(False, "CG") and ps(False, FakeAnalyticEngine)


@pytest.mark.parametrize("optimizer", ["CG", "LAMMPS", "FIRE", "BFGS"])
def test_default_bulk_group_is_held_where_no_indices_are_given(optimizer):
    calc, slabs = BulkCalc(), chains()
    calc.relax_batch(slabs, optimizer=optimizer)
    assert calc.fake.log == relax_entries(optimizer, BULK3, PPP3)
    calc.fake.log.clear()
    calc.relax_batch(slabs, fixed_indices=FIXED["holes"][0], optimizer=optimizer)        # given indices replace the group
    assert calc.fake.log == relax_entries(optimizer, FIXED["holes"][1], PPP3)
    calc.fake.log.clear()
    calc.evaluate_packed(*packed(slabs), relax=True, optimizer=optimizer)
    calc.evaluate_packed(*packed(slabs), relax=True, optimizer=optimizer, fixed_mask=np.array(FIXED["full"][1], np.uint8))
    assert calc.fake.log == relax_entries(optimizer, BULK3, PPP3) + relax_entries(optimizer, FIXED["full"][1], PPP3)
    calc.fake.log.clear()
    for slab in slabs:
        calc.run_lammps_opt(slab, optimizer=optimizer)
    calc.run_lammps_opt(slabs[1], optimizer=optimizer, fixed_indices=[4])
    assert calc.fake.log == [e for b, m in ((0, [1, 1]), (1, [1, 1, 0, 0, 0]), (2, [1, 1, 0]), (1, [0, 0, 0, 0, 1]))
                             for e in relax_entries(optimizer, m, [1, 1, 1], ONE[b])]
    calc.fake.log.clear()
    calc.bulk_index = 0
    calc.relax_batch(slabs, optimizer=optimizer)
    calc.evaluate_packed(*packed(slabs), relax=True, optimizer=optimizer)
    calc.run_lammps_opt(slabs[0], optimizer=optimizer)
    assert calc.fake.log == relax_entries(optimizer, None, PPP3) * 2 + relax_entries(optimizer, None, [1, 1, 1], ONE[0])
    calc.relax_refused = "SRS"
    for call in (lambda: calc.relax_batch(slabs), lambda: calc.run_lammps_opt(slabs[0]), lambda: calc.evaluate_packed(*packed(slabs), relax=True)):
        with pytest.raises(backend.BackendError, match="relaxes with SRS"):
            call()


def test_defaults_come_from_the_settings():
    calc, slabs = Calc(), chains()
    calc.set(relax_steps=30, cg_driver="resident")
    calc.relax_batch(slabs)
    calc.evaluate_packed(*packed(slabs), relax=True)
    calc.run_lammps_opt(slabs[0])
    cg = {**CG_KW, "max_iter": 30, "driver": "resident"}
    assert calc.fake.log == [("relax_cg_arrays_f64", N3, T3, SUM3, PBC3, None, cg)] * 2 + [("relax_cg_arrays_f64", [2], [0, 1], 3.0, [1, 1, 0], None, cg)]
    calc.fake.log.clear()
    calc.set(optimizer="BFGS")                     # relax_batch / evaluate_packed read it; run_lammps_opt has its own default
    calc.relax_batch(slabs, relax_steps=4)
    calc.evaluate_packed(*packed(slabs), relax=True, relax_steps=4)
    calc.run_lammps_opt(slabs[0], fmax=0.5, optimizer="FIRE", etol=1.0)
    assert calc.fake.log == [("relax_arrays_f64", N3, T3, SUM3, PBC3, None, {"max_steps": 4, "fmax": 0.01, "optimizer": "BFGS"})] * 2 \
        + [("relax_arrays_f64", [2], [0, 1], 3.0, [1, 1, 0], None, {"max_steps": 30, "fmax": 0.5, "optimizer": "FIRE"})]
    calc.fake.log.clear()
    for call in (lambda: calc.relax_batch(slabs, cg_driver="fused"), lambda: calc.evaluate_packed(*packed(slabs), relax=True, cg_driver="fused"),
                 lambda: calc.run_lammps_opt(slabs[0], cg_driver="fused")):
        with pytest.raises(ValueError, match="CG driver"):
            call()
    all_p = Calc()
    all_p.all_periodic = True
    all_p.relax_batch(slabs)
    all_p.evaluate_packed(*packed(slabs), relax=True)
    assert all_p.fake.log == [("relax_cg_arrays_f64", N3, T3, SUM3, PPP3, None, CG_KW)] * 2


def test_cg_driver_none_means_the_setting_in_all_three_methods():
    calc, slabs = Calc(), chains()
    calc.set(cg_driver="lockstep")
    calc.relax_batch(slabs, cg_driver=None)
    calc.evaluate_packed(*packed(slabs), relax=True, cg_driver=None)
    calc.run_lammps_opt(slabs[0], cg_driver=None)
    assert [e[-1]["driver"] for e in calc.fake.log] == ["lockstep"] * 3


def test_single_point_methods_do_not_go_through_an_overridden_calculate_batch():
    class Doubled(Calc):
        def calculate_batch(self, atoms_list, want_stress=False):
            raise AssertionError("calculate / run_lammps_energy must not dispatch through the public calculate_batch")

    calc, slabs = Doubled(), chains()
    calc.calculate(slabs[0], properties=("energy",))
    assert calc.results["energy"] == 3.25 and calc.run_lammps_energy(slabs[0])[1] == 3.25


# ---- (b) the three relaxation methods return the same numbers ----------------------------------------------------------------------
@pytest.mark.parametrize("fixed", ["none", "holes", "full"])
@pytest.mark.parametrize("optimizer", ["CG", "FIRE", "BFGS"])
@pytest.mark.parametrize("sizes", [(2, 5, 3), (2, 5, 0), (2, 5, 7)])
def test_relax_batch_evaluate_packed_and_run_lammps_opt_agree(sizes, optimizer, fixed):
    indices, _ = FIXED[fixed]
    if indices is not None:
        indices = [ix if ix is None else [i for i in ix if i < n] for ix, n in zip(indices, sizes)]
    calc, slabs = Calc(), chains(sizes)

    def huge(e, ea, f):          # the five atoms at y = 1 (and seven at y = 2) sum to more than 20: out of the guard's range
        e[e > 20.0] *= 100.0

    calc.fake.tamper = huge
    per_slab = calc.relax_batch(slabs, fixed_indices=indices, optimizer=optimizer)
    n, Z, pos, cell, pbc = packed(slabs)
    mask = None
    if indices is not None:
        mask = np.zeros(int(n.sum()), np.uint8)
        for b, ix in enumerate(indices):
            if ix:
                mask[int(n[:b].sum()) + np.array(ix)] = 1
    res = calc.evaluate_packed(n, Z, pos, cell, pbc, relax=True, fixed_mask=mask, optimizer=optimizer)
    s = res["cfg_start"]
    assert res["oob"].tolist() == [False, True, sizes[2] == 7]
    for b, (slab, (relaxed, traj, energy, oob, r)) in enumerate(zip(slabs, per_slab)):
        a0, a1 = int(s[b]), int(s[b + 1])
        assert traj is None and type(energy) is float and type(oob) is bool and type(r["energy"]) is float
        assert oob == bool(res["oob"][b]) and energy == (1000.0 if oob else float(res["energy"][b])) and r["energy"] == float(res["energy"][b])
        assert np.array_equal(r["per_atom_energies"], res["energy_atoms"][a0:a1]) and np.array_equal(r["forces"], res["forces"][a0:a1])
        assert np.array_equal(relaxed.positions, res["positions"][a0:a1]) and np.array_equal(relaxed.numbers, slab.numbers)
        alone, e1, ea1 = calc.run_lammps_opt(slab, fixed_indices=None if indices is None else indices[b], optimizer=optimizer)
        assert type(e1) is float and e1 == r["energy"] and np.array_equal(ea1, r["per_atom_energies"])
        assert np.array_equal(alone.positions, relaxed.positions)
        if optimizer == "CG":
            assert {k: r[k] for k in ("iterations", "evaluations", "stop")} == {k: calc.last_opt[k] for k in ("iterations", "evaluations", "stop")} \
                == {"iterations": int(res["iterations"][b]), "evaluations": int(res["evaluations"][b]),
                    "stop": backend.CG_STOP_REASONS[int(res["stop"][b])]}
        else:
            assert (r["n_steps"], r["converged"]) == (calc.last_opt["iterations"], calc.last_opt["converged"]) \
                == (int(res["n_steps"][b]), bool(res["converged"][b]))
            assert type(r["n_steps"]) is int and type(r["converged"]) is bool


# ---- (c) the out-of-bounds guard ---------------------------------------------------------------------------------------------------
def _set(name, chain, atom):
    def tamper(e, ea, f):
        if name == "energy_nan":
            e[chain] = np.nan
        elif name == "energy_inf":
            e[chain] = -np.inf
        elif name == "force_nan":
            f[atom, 1] = np.nan
        elif name == "energy_large":
            e[chain] = -1000.5
        elif name == "force_large":
            f[atom, 2] = -1000.5
        elif name == "at_the_bounds":      # (the guard is strict)
            e[chain], f[atom, 0] = -1000.0, 1000.0
    return tamper


OOB_CASES = [("energy_nan", True), ("energy_inf", True), ("force_nan", True), ("energy_large", True), ("force_large", True),
             ("at_the_bounds", False)]


@pytest.mark.parametrize("name,flag", OOB_CASES)
@pytest.mark.parametrize("chain,atom", [(0, 1), (2, 2), (2, 6)])
def test_analytic_guard_fires_at_each_condition(name, flag, chain, atom):
    calc, slabs = Calc(), chains((2, 0, 5))        # an empty chain between the two
    calc.fake.tamper = _set(name, chain, atom)
    expect = [flag and b == chain for b in range(3)]
    for relax in (False, True):
        res = calc.evaluate_packed(*packed(slabs), relax=relax, optimizer="FIRE")
        assert res["oob"].tolist() == expect and res["oob"].dtype == bool
    for optimizer in ("CG", "FIRE"):
        out = calc.relax_batch(slabs, optimizer=optimizer)
        assert [t[3] for t in out] == expect and [t[2] == 1000.0 for t in out] == expect
    calc.ENERGY_THRESHOLD = calc.MAX_FORCE_THRESHOLD = 2000.0       # per instance, as the reference's module constants are patched
    finite = name in ("energy_large", "force_large")
    assert calc.evaluate_packed(*packed(slabs))["oob"].tolist() == [e and not finite for e in expect]
    assert [t[3] for t in calc.relax_batch(slabs)] == [e and not finite for e in expect]


def test_thresholds_are_the_reference_values_on_both_families():
    for cls in (calculators.EnsembleNFFSurface, calculators.NFFPourbaix, calculators._AnalyticSurfCalc, calculators.LAMMPSSurfCalc, Calc):
        assert cls.ENERGY_THRESHOLD == 1000.0 and cls.MAX_FORCE_THRESHOLD == 1000.0


# ---- (d) Z -> type -----------------------------------------------------------------------------------------------------------------
def test_uncovered_elements_are_refused_by_name():
    calc, slabs = Calc(), chains()
    slabs[1].numbers[3] = 14
    slabs[1].numbers[4] = 8
    msg = re.escape("element Z=14 is not covered by the potential ['Ga', 'N']")
    for call in (lambda: calc.relax_batch(slabs), lambda: calc.calculate_batch(slabs), lambda: calc.calculate(slabs[1]),
                 lambda: calc.run_lammps_energy(slabs[1]), lambda: calc.run_lammps_opt(slabs[1]),
                 lambda: calc.evaluate_packed(*packed(slabs)), lambda: calc.evaluate_packed(*packed(slabs), relax=True)):
        with pytest.raises(ValueError, match=msg):
            call()
    assert calc.fake.log == []
    assert calc._types_of(np.array([7, 31, 31])).tolist() == [1, 0, 0] and calc._types_of(np.array([7, 31, 31])).dtype == np.int32
    assert calc._types_of(np.zeros(0, np.int64)).shape == (0,)
    assert [t.tolist() for t in calc._pack(chains()[0])[:1]] == [[0, 1]] and calc._pack(chains()[0])[0].dtype == np.int32


def test_an_atomic_number_outside_the_table_is_refused_not_clipped():
    calc = Calc()
    calc.species = ["Ga", "Fm"]                   # Fm (Z = 100) is the last symbol of the table
    assert calc._types_of(np.array([100, 31])).tolist() == [1, 0]
    for bad in (101, 250, -3):
        with pytest.raises(ValueError, match=re.escape(f"element Z={bad} is not covered by the potential ['Ga', 'Fm']")):
            calc._types_of(np.array([31, bad, 100]))
    calc.species = ["Ga", "X"]                    # the placeholder symbol of Z = 0
    assert calc._types_of(np.array([0, 31])).tolist() == [1, 0]
    slab = chains()[0]
    slab.numbers[1] = -3
    with pytest.raises(ValueError, match=re.escape("element Z=-3 is not covered by the potential ['Ga', 'X']")):
        calc._pack(slab)
    # THE assertion that differs from the parent commit: there ``_types_of`` clipped atomic numbers into its table, which has a spare
    # slot above Fm (so Z > 100 was refused) but none below X: a negative Z was evaluated as X where X is among the species, although
    # ``_pack`` refused it
    with pytest.raises(ValueError, match=re.escape("element Z=-3 is not covered by the potential ['Ga', 'X']")):
        calc._types_of(np.array([31, -3, 0]))


# ---- (e) what mc.ChainEnsemble inspects --------------------------------------------------------------------------------------------
def test_relax_batch_signatures_name_the_optimizer():
    assert "optimizer" in inspect.signature(Calc().relax_batch).parameters
    # (LAMMPSSurfCalc forwards its keywords: mc.ChainEnsemble leaves the optimizer to the calculator's own setting there)
    assert list(inspect.signature(BulkCalc().relax_batch).parameters) == ["atoms_list", "fixed_indices", "kwargs"]
    assert "optimizer" in inspect.signature(Calc().evaluate_packed).parameters
    assert "optimizer" in inspect.signature(calculators.EnsembleNFFSurface.relax_batch).parameters


# ---- the PaiNN family --------------------------------------------------------------------------------------------------------------
def _e_atom(pos):
    return ((np.asarray(pos, dtype=np.float64).reshape(-1, 3) - 4.0) ** 2).sum(axis=1) / 16.0


class FakePainnEngine:
    """fp32 ensemble engine: e_atom = |pos - (4, 4, 4)|^2 / 16 (``_e_atom``), E_b their sum over the chain, F = 1/2 - pos / 8 its
    gradient; a device relaxation moves every free atom by +1/2.  One instance per ``backend.PainnEngine(...)``, kept in ``made``."""

    made = []
    tamper = None

    def __init__(self, blobs, **kw):
        self.n_models, self.log = len(blobs), []
        FakePainnEngine.made.append(self)

    def upload_arrays(self, n_atoms, Z, pos, cell, pbc):
        n_atoms, pos = np.ascontiguousarray(n_atoms, dtype=np.int32), np.array(pos, dtype=np.float64).reshape(-1, 3)
        assert len(Z) == len(pos) == int(n_atoms.sum()) and np.asarray(cell).size == 9 * len(n_atoms) and np.asarray(pbc).size == 3 * len(n_atoms)
        self._n, self._pos = n_atoms, pos
        self.log.append(("upload_arrays", [int(n) for n in n_atoms], float(pos.sum())))

    def upload(self, structs):
        self.upload_arrays(*backend.pack_batch(structs))

    def set_positions(self, pos):
        self._pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
        assert len(self._pos) == int(self._n.sum())
        self.log.append(("set_positions", float(self._pos.sum())))

    def run(self, want=backend.WANT_ALL):
        self.log.append(("run", int(want)))

    def download(self, want=backend.WANT_ALL):
        self.log.append(("download", int(want)))
        B, N, M = len(self._n), len(self._pos), self.n_models
        ea = _e_atom(self._pos)
        e64 = _per_chain(ea, self._n)
        res = {"energy": e64.astype(np.float32), "energy_std": np.full(B, 0.5, np.float32), "forces": (0.5 - 0.125 * self._pos).astype(np.float32),
               "forces_std": np.zeros((N, 3), np.float32), "energy_models": np.tile(e64[:, None], (1, M)).astype(np.float32),
               "energy_atoms": ea.astype(np.float32), "cfg_start": _start(self._n), "saturated": np.zeros(B, bool),
               "energy_f64": e64.copy(), "energy_std_f64": np.full(B, 0.5), "energy_models_f64": np.tile(e64[:, None], (1, M))}
        if FakePainnEngine.tamper is not None:
            FakePainnEngine.tamper(res)
        return res

    def evaluate(self, structs, want=backend.WANT_ALL):
        self.upload(structs)
        self.run(want)
        return self.download(want)

    def _relaxed(self, fixed, record_interval, **more):
        self._pos = _moved(self._pos, fixed)
        out = {"positions": self._pos.copy(), "n_steps": self._n + 4, "converged": self._n % 2 == 0, **more}
        if record_interval:
            out["traj"] = _fake_traj(self._n, self._pos, record_interval)
        return out

    def relax(self, optimizer="FIRE", fixed=None, max_steps=20, fmax=0.01, want=backend.WANT_ALL, params=None, record_interval=0):
        self.log.append(("relax", optimizer, _mask(fixed), {"max_steps": max_steps, "fmax": fmax, "record_interval": record_interval}))
        if any(k in str(optimizer) for k in (BFGSLS, "CG", "LAMMPS")):
            raise backend.BackendError(f"optimizer {optimizer!r} is not available on the device (FIRE and BFGS are)")
        return self._relaxed(fixed, record_interval)

    def relax_bfgs_linesearch(self, fixed=None, max_steps=20, fmax=0.01, max_eval=None, want=backend.WANT_ALL, params=None, record_interval=0):
        self.log.append(("relax_bfgs_linesearch", _mask(fixed), {"max_steps": max_steps, "fmax": fmax, "max_eval": max_eval,
                                                                   "record_interval": record_interval}))
        return self._relaxed(fixed, record_interval, n_eval=self._n + 5, stop_reason=self._n % 2 + 1)

    def stress(self):
        self.log.append(("stress",))
        B = len(self._n)
        return np.arange(6.0 * B).reshape(B, 6), np.ones((B, 6))

    def embedding(self, model=None):
        self.log.append(("embedding", model))
        return np.arange(self.n_models * len(self._pos) * 2, dtype=np.float32).reshape(self.n_models, len(self._pos), 2)

    def close(self):
        pass


@pytest.fixture
def painn(monkeypatch, golden):
    FakePainnEngine.made, FakePainnEngine.tamper = [], None
    monkeypatch.setattr(backend, "PainnEngine", FakePainnEngine)
    calc = calculators.EnsembleNFFSurface(golden.blobs[:2], device="cuda:0")
    yield calc
    FakePainnEngine.made, FakePainnEngine.tamper = [], None


ALL = int(backend.WANT_ALL)
E3 = [4.6875, 7.5, 4.25]            # the fake's energies of the chains (2, 5, 3)
EVALUATION = [("run", ALL), ("download", ALL)]


def test_painn_single_points(painn):
    slabs = chains()
    painn.calculate(slabs[1], properties=("energy", "forces"))
    eng = FakePainnEngine.made[0]
    assert eng.log == [("upload_arrays", [5], 20.0)] + EVALUATION
    assert painn.results["energy"].shape == (1,) and painn.results["energy"].dtype == np.float32 and painn.results["energy_f64"] == E3[1]
    assert painn.results["forces"].shape == (5, 3) and painn.results["saturated"] is False and slabs[1].results["energy"][0] == np.float32(E3[1])
    eng.log.clear()
    painn.calculate(slabs[1], properties=("energy", "stress", "embedding"))
    assert eng.log == [("upload_arrays", [5], 20.0)] + EVALUATION + [("stress",), ("embedding", None)]
    assert painn.results["embedding"].shape == (5, 2) and painn.results["embedding_models"].shape == (2, 5, 2)
    eng.log.clear()
    out = painn.calculate_batch(slabs, want_embedding=True, want_stress=True)
    assert eng.log == [("upload_arrays", N3, SUM3)] + EVALUATION + [("stress",), ("embedding", None)]
    assert [r["energy_f64"] for r in out] == E3 and [r["forces"].shape for r in out] == [(2, 3), (5, 3), (3, 3)]
    assert np.array_equal(out[1]["embedding"], np.arange(4.0, 14.0).reshape(5, 2)) and out[2]["embedding_models"].shape == (2, 3, 2)
    assert np.array_equal(out[2]["per_atom_energies"], [1.8125, 1.375, 1.0625]) and np.array_equal(out[1]["stress_std"], np.ones(6))
    eng.log.clear()
    n, Z, pos, cell, pbc = packed(slabs)
    res = painn.evaluate_packed(n, Z, pos, cell, pbc)
    assert eng.log == [("upload_arrays", N3, SUM3)] + EVALUATION
    assert sorted(res) == ["cfg_start", "energy", "energy_atoms", "energy_f64", "energy_std", "energy_std_f64", "forces", "oob", "positions", "saturated"]
    assert res["energy"].dtype == np.float32 and res["energy_f64"].tolist() == E3 and np.array_equal(res["positions"], pos)
    assert res["cfg_start"].tolist() == [0, 2, 7, 10] and res["cfg_start"].dtype == np.int64 and not res["oob"].any()


@pytest.mark.parametrize("fixed", ["none", "holes", "full"])
@pytest.mark.parametrize("optimizer", ["FIRE", "BFGS", None])
def test_painn_device_relaxations(painn, optimizer, fixed):
    indices, mask = FIXED[fixed]
    slabs = chains()
    name = "FIRE" if optimizer is None else optimizer
    out = painn.relax_batch(slabs, fixed_indices=indices, optimizer=optimizer, relax_steps=8, fmax=0.25, record_interval=2)
    eng = FakePainnEngine.made[0]
    assert eng.log == [("upload_arrays", N3, SUM3), ("relax", name, mask, {"max_steps": 8, "fmax": 0.25, "record_interval": 0}), ("download", ALL)]
    assert [t[1] for t in out] == [None] * 3 and [(t[4]["n_steps"], t[4]["converged"]) for t in out] == [(6, True), (9, False), (7, False)]
    assert all("n_eval" not in t[4] for t in out)
    eng.log.clear()
    traj = painn.relax_batch(slabs, fixed_indices=indices, optimizer=optimizer, save_traj=True, record_interval=2)
    assert eng.log == [("upload_arrays", N3, SUM3), ("relax", name, mask, {"max_steps": 20, "fmax": 0.01, "record_interval": 2}), ("download", ALL)]
    assert [len(t[1]["atoms"]) for t in traj] == [1, 2, 2] and [t[1]["energies"] for t in traj] == [[0.0], [1.0, 4.0], [2.0, 5.0]]
    assert all(f.calc is None for t in traj for f in t[1]["atoms"])
    eng.log.clear()
    n, Z, pos, cell, pbc = packed(slabs)
    res = painn.evaluate_packed(n, Z, pos, cell, pbc, relax=True, fixed_mask=None if mask is None else np.array(mask, np.uint8),
                                optimizer=optimizer, relax_steps=8, fmax=0.25)
    assert eng.log == [("upload_arrays", N3, SUM3), ("relax", name, mask, {"max_steps": 8, "fmax": 0.25, "record_interval": 0}), ("download", ALL)]
    # (b) for this family: per slab and packed give the same numbers
    s = res["cfg_start"]
    for b, (relaxed, _, energy, oob, r) in enumerate(out):
        a0, a1 = int(s[b]), int(s[b + 1])
        assert energy == float(res["energy_f64"][b]) and oob == bool(res["oob"][b]) and r["n_steps"] == int(res["n_steps"][b])
        assert np.array_equal(relaxed.positions, res["positions"][a0:a1]) and np.array_equal(r["forces"], res["forces"][a0:a1])
        assert np.array_equal(r["per_atom_energies"], res["energy_atoms"][a0:a1]) and r["converged"] == bool(res["converged"][b])
        assert np.array_equal(r["energy"], res["energy"][b:b + 1]) and r["energy_std_f64"] == float(res["energy_std_f64"][b])


@pytest.mark.parametrize("fixed", ["none", "holes", "full"])
def test_painn_device_line_search(painn, fixed):
    indices, mask = FIXED[fixed]
    slabs = chains()
    out = painn.relax_batch(slabs, fixed_indices=indices, optimizer=BFGSLS, linesearch_driver="device", relax_steps=8)
    eng = FakePainnEngine.made[0]
    assert eng.log == [("upload_arrays", N3, SUM3),
                       ("relax_bfgs_linesearch", mask, {"max_steps": 8, "fmax": 0.01, "max_eval": None, "record_interval": 0}), ("download", ALL)]
    assert [(t[4]["n_steps"], t[4]["n_eval"], t[4]["stop_reason"], t[4]["converged"]) for t in out] == [(6, 7, 1, True), (9, 10, 2, False), (7, 8, 2, False)]
    eng.log.clear()
    painn.set(linesearch_driver="device")
    out = painn.relax_batch(slabs, fixed_indices=indices, optimizer=BFGSLS, save_traj=True, record_interval=3)
    assert eng.log[1] == ("relax_bfgs_linesearch", mask, {"max_steps": 20, "fmax": 0.01, "max_eval": None, "record_interval": 3})
    assert [len(t[1]["atoms"]) for t in out] == [1, 2, 2]
    painn.set(linesearch_driver="ase")
    if not calculators.HAVE_ASE:
        with pytest.raises(backend.BackendError, match="ASE is not importable"):
            painn.relax_batch(slabs, optimizer=BFGSLS)
    with pytest.raises(ValueError, match="linesearch driver"):
        painn.relax_batch(slabs, linesearch_driver="host")
    eng.log.clear()
    for name in ("CG", "LAMMPS", BFGSLS):          # evaluate_packed hands host-driven names to the engine, which refuses them
        with pytest.raises(backend.BackendError, match="not available on the device"):
            painn.evaluate_packed(*packed(slabs), relax=True, optimizer=name)
    assert [e[0] for e in eng.log] == ["upload_arrays", "relax"] * 3


class TwoSteps:
    """An optimizer of the ASE protocol: two steepest-descent steps, whatever ``fmax`` says."""

    def __init__(self, atoms, **kwargs):
        self.atoms, self.nsteps, self.observers = atoms, 0, []

    def attach(self, fn, interval=1):
        self.observers.append((fn, interval))

    def run(self, fmax=0.05, steps=100):
        for _ in range(2):
            f = self.atoms.get_forces()
            for fn, interval in self.observers:
                if self.nsteps % interval == 0:
                    fn()
            self.atoms.set_positions(self.atoms.get_positions() + 2.0 * f)
            self.nsteps += 1


@pytest.mark.parametrize("fixed", ["none", "holes", "full"])
def test_painn_optimizer_class_runs_over_lockstep_evaluations(painn, fixed):
    indices, mask = FIXED[fixed]
    slabs = chains()
    out = painn.relax_batch(slabs, fixed_indices=indices, optimizer=TwoSteps, save_traj=True, record_interval=1)
    eng = FakePainnEngine.made[0]
    free = 10 - (0 if mask is None else sum(mask))
    # F = 1/2 - pos / 8 and a step of 2 F: pos -> 3/4 pos + 1, so the sum of the free coordinates s goes to 3/4 s + 3 per free atom
    fixed_sum = 0.0 if mask is None else float(sum(np.asarray(packed(slabs)[2])[np.array(mask, bool)].sum(axis=1)))
    s0 = SUM3 - fixed_sum
    s1 = 0.75 * s0 + 3.0 * free
    s2 = 0.75 * s1 + 3.0 * free
    cycle = lambda s: [("set_positions", s + fixed_sum), ("run", ALL), ("download", ALL)]     # noqa: E731
    assert eng.log == [("upload_arrays", N3, SUM3)] + cycle(s0) + cycle(s1) + cycle(s2)
    assert [t[4]["n_steps"] for t in out] == [2, 2, 2] and [len(t[1]["atoms"]) for t in out] == [2, 2, 2]
    assert float(sum(t[0].positions.sum() for t in out)) == s2 + fixed_sum
    if mask is not None:
        held = np.array(mask, bool)
        assert np.array_equal(np.concatenate([t[0].positions for t in out])[held], packed(slabs)[2][held])
    assert [t[4]["converged"] for t in out] == [False, False, fixed == "full"]     # free atoms keep |F| near 1/2; "full" holds all of chain 2


@pytest.mark.parametrize("fixed", ["none", "holes", "full"])
def test_painn_host_cg_runs_over_lockstep_evaluations(painn, fixed):
    indices, mask = FIXED[fixed]
    slabs = chains()
    out = painn.relax_batch(slabs, fixed_indices=indices, optimizer="CG", relax_steps=2, save_traj=True, record_interval=1)
    eng = FakePainnEngine.made[0]
    names = [e[0] for e in eng.log]
    # scipy decides how many evaluations its line searches ask for: upload, rounds of (set_positions, run, download), then the
    # final geometries are set, run and downloaded
    assert names[0] == "upload_arrays" and len(names) % 3 == 1 and len(names) >= 10
    assert names[1:] == ["set_positions", "run", "download"] * (len(names) // 3) and len(names) < 100
    assert eng.log[1] == ("set_positions", SUM3)
    final = np.concatenate([t[0].positions for t in out])
    assert eng.log[-3] == ("set_positions", float(final.sum()))
    if mask is not None:
        held = np.array(mask, bool)
        assert np.array_equal(final[held], packed(slabs)[2][held])
    for t, slab in zip(out, slabs):
        assert sorted(t[1]) == ["atoms", "energies", "forces"] and len(t[1]["atoms"]) == len(t[1]["energies"]) == len(t[1]["forces"]) >= 1
        assert all(f.calc is None and len(f) == len(slab) for f in t[1]["atoms"]) and t[1]["forces"][0].dtype == np.float32
        assert np.array_equal(t[1]["atoms"][0].positions, slab.positions) and type(t[1]["energies"][0]) is float


def _painn_set(name, chain, atom):
    def tamper(res):
        if name == "energy_nan":
            res["energy"][chain] = res["energy_f64"][chain] = np.nan
        elif name == "force_nan":
            res["forces"][atom, 1] = np.nan
        elif name == "energy_large":
            res["energy"][chain] = res["energy_f64"][chain] = -1000.5
        elif name == "force_large":
            res["forces"][atom, 2] = 1000.5
        elif name == "saturated":
            res["saturated"][chain] = True
        elif name == "at_the_bounds":
            res["energy"][chain] = res["energy_f64"][chain] = -1000.0
            res["forces"][atom, 0] = 1000.0
    return tamper


@pytest.mark.parametrize("name,flag", [("energy_nan", True), ("force_nan", True), ("energy_large", True), ("force_large", True),
                                       ("saturated", True), ("at_the_bounds", False)])
@pytest.mark.parametrize("chain,atom", [(0, 1), (2, 2), (2, 6)])
def test_painn_guard_fires_at_each_condition(painn, name, flag, chain, atom):
    slabs = chains((2, 0, 5))
    FakePainnEngine.tamper = _painn_set(name, chain, atom)
    expect = [flag and b == chain for b in range(3)]
    for relax in (False, True):
        res = painn.evaluate_packed(*packed(slabs), relax=relax)
        assert res["oob"].tolist() == expect and res["oob"].dtype == bool
        assert res["saturated"].tolist() == [name == "saturated" and b == chain for b in range(3)]
    for optimizer in ("FIRE", BFGSLS, TwoSteps):
        out = painn.relax_batch(slabs, optimizer=optimizer, linesearch_driver="device")
        assert [t[3] for t in out] == expect and [t[2] == 1000.0 for t in out] == expect and all(type(t[3]) is bool for t in out)
    painn.ENERGY_THRESHOLD = painn.MAX_FORCE_THRESHOLD = 2000.0
    finite = name in ("energy_large", "force_large")
    assert painn.evaluate_packed(*packed(slabs))["oob"].tolist() == [e and not finite for e in expect]
    assert [t[3] for t in painn.relax_batch(slabs)] == [e and not finite for e in expect]


def test_painn_evaluate_packed_splits_large_relaxations_over_two_engines(painn):
    sizes = [1 + b % 3 for b in range(64)]
    slabs = chains(sizes)
    n, Z, pos, cell, pbc = packed(slabs)
    mask = (np.arange(len(Z)) % 4 == 0).astype(np.uint8)
    res = painn.evaluate_packed(n, Z, pos, cell, pbc, relax=True, fixed_mask=mask, optimizer="BFGS", relax_steps=5)
    assert len(FakePainnEngine.made) == 2
    first, second = FakePainnEngine.made
    half = sum(sizes[:32])
    kw = {"max_steps": 5, "fmax": 0.01, "record_interval": 0}
    assert first.log == [("upload_arrays", sizes[:32], float(pos[:half].sum())), ("relax", "BFGS", _mask(mask[:half]), kw), ("download", ALL)]
    assert second.log == [("upload_arrays", sizes[32:], float(pos[half:].sum())), ("relax", "BFGS", _mask(mask[half:]), kw), ("download", ALL)]
    assert np.array_equal(res["cfg_start"], _start(sizes)) and res["cfg_start"].dtype == np.int64
    assert np.array_equal(res["positions"], _moved(pos, mask)) and np.array_equal(res["energy_f64"], _per_chain(_e_atom(_moved(pos, mask)), sizes))
    assert np.array_equal(res["n_steps"], np.array(sizes) + 4) and res["forces"].shape == (len(Z), 3) and res["oob"].shape == (64,)
    first.log.clear()
    painn.evaluate_packed(n, Z, pos, cell, pbc)                      # single points and 63 chains stay on one engine
    painn.evaluate_packed(n[:63], Z[:-1], pos[:-1], cell[:63], pbc[:63], relax=True)
    assert [e[0] for e in first.log] == ["upload_arrays", "run", "download", "upload_arrays", "relax", "download"] and len(second.log) == 3
