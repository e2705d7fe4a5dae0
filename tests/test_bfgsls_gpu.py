"""The device BFGSLineSearch (csrc/bfgsls_dev.h, csrc/relax_bfgsls.hip, vssr_batch_relax_bfgs_linesearch) on the cases of
tests/bfgsls_cases.py against the numpy restatement tests/bfgsls_oracle.py (which is NOT pinned by an executed ASE: see its
docstring), what the driver leaves on the device, PaiNN by properties, budgets, the trajectory observer, the calculators'
``linesearch_driver`` and the raw ABI.  Bounds against the restatement are those of tests/test_cg.py: equal (n_steps, n_eval,
stop_reason), |dE| < 1e-9 eV, max|dpos| < 1e-9 A."""

import ctypes as C
import os

import numpy as np
import pytest

import bfgsls_cases as bc
import bfgsls_oracle as bo
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _split(cases, flat):
    o, out = 0, []
    for c in cases:
        out.append(flat[o:o + len(c.types)])
        o += len(c.types)
    return out


class Bench:
    """One engine per kind, the restatement's result per (case, parameters) and the device's result per batch: each is computed once
    and shared by the tests of this module."""

    def __init__(self, golden, oracle_mod):
        from surface_sampling_amd import backend
        import cg_cases as cc

        self.golden, self.oracle, self.backend = golden, oracle_mod, backend
        self.eng = {"tersoff": backend.TersoffEngine(golden.tersoff_params, device=0),
                    "pair": backend.PairEngine(cc.LJ_TERMS, n_types=cc.LJ_NTYPES, device=0)}
        self._ref, self._run = {}, {}

    def close(self):
        for e in self.eng.values():
            e.close()

    def ref(self, case, record_interval=0):
        key = (case.name, bc._key(case.params), record_interval)
        if key not in self._ref:
            self._ref[key] = bc.run_restatement(case, self.golden, self.oracle, record_interval=record_interval)
        return self._ref[key]

    def relax(self, eng, cases, params, record_interval=0):
        """vssr_batch_relax_bfgs_linesearch on the packed cases; what it left on the device (no upload, no run), the stress served
        from that, then a fresh static evaluation of the returned positions on the same engine."""
        B = self.backend
        structs, mask = bc.pack(cases)
        eng.upload(structs)
        info = eng.relax_bfgs_linesearch(fixed=mask, want=B.WANT_ENERGY | B.WANT_FORCES | B.WANT_PER_ATOM,
                                         params=B.BfgsLsParams.default(**params), record_interval=record_interval)
        counts = eng.last_relax_counts
        e, ea, f = eng.results_f64()
        stress = eng.stress()[0]
        n_atoms, T, _, cell, pbc = B.pack_batch(structs)
        fresh = eng.evaluate_arrays_f64(n_atoms, T, info["positions"], cell, pbc)
        return dict(info, e=e, ea=ea, f=f, stress=stress, fresh=fresh, fresh_stress=eng.stress()[0], counts=counts,
                    mask=mask.astype(bool), start=np.concatenate([c.pos for c in cases]))

    def run(self, kind, k):
        if (kind, k) not in self._run:
            params, cases = bc.batches(kind, self.golden)[k]
            self._run[(kind, k)] = self.relax(self.eng[kind], cases, params)
        return self._run[(kind, k)]


@pytest.fixture(scope="module")
def bench(golden, oracle_mod):
    b = Bench(golden, oracle_mod)
    yield b
    b.close()


def _compare(tag, cases, r, refs):
    """Device against restatement, chain by chain; prints the figures before it asserts."""
    worst_e = worst_x = 0.0
    for b, (c, p) in enumerate(zip(cases, _split(cases, r["positions"]))):
        pref, eref, steps, neval, reason, _ = refs[b]
        got = (int(r["n_steps"][b]), int(r["n_eval"][b]), int(r["stop_reason"][b]))
        de, dx = abs(r["e"][b] - eref), float(np.abs(p - pref).max())
        print(f"{tag} {c.name}: device (steps, eval, stop) {got}  restatement {(steps, neval, reason)}  |dE| {de:.3e}  max|dpos| {dx:.3e}")
        assert got == (steps, neval, reason), (c.name, got, (steps, neval, reason))
        assert de < 1e-9 and dx < 1e-9, (c.name, de, dx)
        assert bool(r["converged"][b]) == (reason == 1)
        worst_e, worst_x = max(worst_e, de), max(worst_x, dx)
    return worst_e, worst_x


@pytest.mark.parametrize("kind", ["tersoff", "pair"])
def test_exact_cases_follow_the_restatement(bench, kind):
    """One ragged batch per parameter set: chains that stop at their first evaluation next to chains that search on.  Same counts and
    stop reason as the restatement, energies and positions to 1e-9, held atoms untouched bit for bit."""
    reasons = set()
    for k, (params, cases) in enumerate(bc.batches(kind, bench.golden)):
        r = bench.run(kind, k)
        assert np.array_equal(r["positions"][r["mask"]], r["start"][r["mask"]]), (kind, k)
        we, wx = _compare(kind, cases, r, [bench.ref(c) for c in cases])
        reasons |= set(r["stop_reason"].tolist())
        assert len(set(zip(r["n_steps"].tolist(), r["n_eval"].tolist(), r["stop_reason"].tolist()))) > 1 or params["max_steps"] == 0
        # evaluation-counted: the launches are those of the longest chain (up to the poll window) plus the closing evaluation
        assert r["counts"][0] <= int(r["n_eval"].max()) + 4 + 1
    assert reasons >= {1, 2, 3, 4}


@pytest.mark.parametrize("kind", ["tersoff", "pair"])
def test_the_driver_leaves_the_static_results_of_the_final_geometry(bench, kind):
    """Results downloaded without a rerun (vssr_batch_results_f64) against a fresh upload + evaluation of the returned positions: the
    same bits, also for chains switched off long before the batch finished; ``stress()`` is served from what the driver left."""
    for k, _ in enumerate(bc.batches(kind, bench.golden)):
        r = bench.run(kind, k)
        for name, a, b in zip(("energy", "e_atom", "forces"), (r["e"], r["ea"], r["f"]), r["fresh"]):
            assert np.array_equal(a, b), (kind, k, name, np.abs(a - b).max())
        # (the same kernels on the same positions: only a summation order could differ)
        assert np.isfinite(r["stress"]).all() and np.allclose(r["stress"], r["fresh_stress"], rtol=1e-12, atol=1e-15)


def _sw_batch():
    import sw_oracle as so

    P = so.si_params()
    T, X, Cl = so.diamond_si(so.SI_A0)
    pbc = np.ones(3, np.uint8)
    out = []
    for seed, held in ((1, [0]), (2, [0, 5]), (3, np.arange(len(T)))):
        pos = X + np.random.default_rng(seed).normal(0, 0.06, X.shape)
        out.append(bc.Case(f"sw:diamond_8_seed{seed}", "sw", "exact", np.asarray(T, np.int32), pos, np.array(Cl, float), pbc,
                           np.asarray(held, np.int64), bc._params(max_steps=6), None, ()))

    def fn(c):
        def f(p):
            E, _, F = so.sw(P, c.types, p, c.cell, c.pbc)
            return E, F
        return f
    return P, out, fn


def _eam_batch():
    import eam_alloy_oracle as ao
    from surface_sampling_amd import eam

    cu, au = eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))
    tab = eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au))), ["Cu", "Au"])
    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    out = []
    for k in range(3):
        sub = [(2 + 3 * k) % len(d["ads_coords"]), (9 + 5 * k) % len(d["ads_coords"])]
        pos = np.vstack([d["positions"], d["ads_coords"][sub]]) + np.random.default_rng(k).normal(0, 0.03, (10, 3))
        t = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1, k % 2], np.int32)
        held = np.arange(10) if k == 2 else np.arange(4)
        out.append(bc.Case(f"eam:cu100_ads_{k}", "eam", "exact", t, pos, np.array(d["cell"], float), d["pbc"].astype(np.uint8), held,
                           bc._params(max_steps=6), None, ()))

    def fn(c):
        def f(p):
            E, _, F = ao.eam_typed(tab, c.types, p, c.cell, c.pbc)
            return E, F
        return f
    return tab, out, fn


@pytest.mark.parametrize("kind", ["sw", "eam"])
def test_sw_and_eam_follow_the_restatement(bench, kind):
    """One small batch each (two running chains and one with every atom held) on the project's own fp64 restatements of the
    potentials.  The restatement's tracer vouches for the comparison first: decision margins above 1e-7."""
    B = bench.backend
    pot, cases, fn = _sw_batch() if kind == "sw" else _eam_batch()
    refs = []
    for c in cases:
        tr = bo.Trace()
        refs.append(bo.bfgs_linesearch(fn(c), c.pos, fixed=c.fixed, trace=tr, **c.params))
        assert tr.margin > bc.EXACT_MARGIN, (c.name, tr.margin, tr.margin_at)
    eng = B.SWEngine(pot, device=0) if kind == "sw" else B.EAMEngine(pot, device=0)
    try:
        r = bench.relax(eng, cases, cases[0].params)
    finally:
        eng.close()
    assert np.array_equal(r["positions"][r["mask"]], r["start"][r["mask"]])
    _compare(kind, cases, r, refs)
    assert r["n_steps"].max() >= 3 and r["n_steps"][2] == 0
    for a, b in zip((r["e"], r["ea"], r["f"]), r["fresh"]):
        assert np.array_equal(a, b)


def test_budgets_and_a_start_at_a_minimum(bench):
    """max_steps = 0, max_eval = 1 and a start at a minimum: reasons 2, 4 and 1 at unchanged positions, one evaluation each."""
    eng, B = bench.eng["tersoff"], bench.backend
    c = [k for k in bc.all_cases(bench.golden) if k.name == "tersoff:defaults_7_three_held"][0]
    structs, mask = bc.pack([c, c])
    want = B.WANT_ENERGY | B.WANT_FORCES | B.WANT_PER_ATOM
    for kw, reason in ((dict(max_steps=0), 2), (dict(max_eval=1), 4)):
        eng.upload(structs)
        info = eng.relax_bfgs_linesearch(fixed=mask, want=want, **kw)
        assert info["stop_reason"].tolist() == [reason] * 2 and info["n_steps"].tolist() == [0, 0] and info["n_eval"].tolist() == [1, 1]
        assert np.array_equal(info["positions"], np.concatenate([c.pos, c.pos]))
    eng.upload(structs)
    relaxed = eng.relax_bfgs_linesearch(fixed=mask, want=want, max_steps=40, fmax=0.01)
    assert relaxed["stop_reason"].tolist() == [1, 1] and (relaxed["n_steps"] > 0).all()
    n = len(c.types)
    eng.upload([(c.types, relaxed["positions"][:n], c.cell, c.pbc), (c.types, relaxed["positions"][n:], c.cell, c.pbc)])
    again = eng.relax_bfgs_linesearch(fixed=mask, want=want, max_steps=40, fmax=0.02)
    assert again["stop_reason"].tolist() == [1, 1] and again["n_steps"].tolist() == [0, 0] and again["n_eval"].tolist() == [1, 1]
    assert np.array_equal(again["positions"], relaxed["positions"])


# (lock-step evaluations roomy, tight; regrows) of the run below as commit 809cdf4 returns them
REGROW_COUNTS_809CDF4 = (41, 45, 1)


def test_capacity_regrow_in_the_middle_of_a_relaxation(bench):
    """Pools of 4 slots per atom, regrown to the exact need (a row takes at least 8, and the rows grow as the chains contract): the
    evaluations overflow, the driver regrows, gives the poll window back and ends with the bits of the roomy run."""
    import cg_cases as cc

    params, cases = bc.batches("pair", bench.golden)[0]
    roomy = bench.run("pair", 0)
    eng = bench.backend.PairEngine(cc.LJ_TERMS, n_types=cc.LJ_NTYPES, device=0)
    eng.debug_capacity(slots_per_atom=4, tight=1)
    tight = bench.relax(eng, cases, params)
    regrows = eng.debug_capacity()
    eng.close()
    print(f"roomy counts {roomy['counts']}; tight counts {tight['counts']} regrows {regrows}")
    assert regrows >= 1 and tight["counts"][0] > roomy["counts"][0]
    for key in ("positions", "n_steps", "n_eval", "stop_reason", "e", "ea", "f"):
        assert np.array_equal(tight[key], roomy[key]), key
    assert (roomy["counts"][0], tight["counts"][0], regrows) == REGROW_COUNTS_809CDF4


def test_the_trajectory_holds_the_step_opens_and_no_trial_point(bench):
    """record_interval = 2: the records are those of steps 0, 2, 4, ... of the restatement's trajectory (positions, energies, forces
    with FixAtoms applied); a line-search trial is never recorded."""
    kind = "tersoff"
    params, cases = bc.batches(kind, bench.golden)[0]
    assert params == bc.DEFAULTS
    r = bench.relax(bench.eng[kind], cases, params, record_interval=2)
    plain = bench.run(kind, 0)
    assert np.array_equal(r["positions"], plain["positions"]) and np.array_equal(r["n_eval"], plain["n_eval"])   # the observer only watches
    tr = r["traj"]
    assert tr["positions"].shape[0] == params["max_steps"] // 2 + 1
    o, total = 0, 0
    for b, c in enumerate(cases):
        n = len(c.types)
        recs = bench.ref(c, record_interval=2)[5]
        assert int(tr["n_records"][b]) == len(recs) == int(r["n_steps"][b]) // 2 + 1, (c.name, tr["n_records"][b], len(recs))
        for k, (step, pos, E, F) in enumerate(recs):
            assert step == 2 * k
            assert np.abs(tr["positions"][k, o:o + n] - pos).max() < 1e-9, (c.name, k)
            assert abs(tr["energies"][k, b] - E) < 1e-9
            assert np.abs(tr["forces"][k, o:o + n] - F).max() < 1e-6 * max(1.0, np.abs(F).max())      # (the ring holds fp32 forces)
            assert not tr["forces"][k, o:o + n][c.fixed].any()
        total += len(recs)
        o += n
    assert total > len(cases) + 10


def test_painn_by_properties(golden):
    """fp32 evaluations: no count parity with an fp64 restatement.  Two ragged chains of the 60-atom slab, bulk held, 6 steps: held
    atoms bit-identical, the energy of every recorded step non-increasing within 2e-4 eV (the wrapper tolerance of the project), the
    returned energy that of a fresh calculate_batch within 2e-4, n_eval >= n_steps + 1."""
    from surface_sampling_amd import structures
    from surface_sampling_amd.calculators import EnsembleNFFSurface

    base = golden.structure("SrTiO3_2x2_pristine")
    slabs = [structures.synth_chain(base, c, grid=(4, 4)) for c in (1, 2)]
    assert len(slabs[0]) != len(slabs[1]) and max(len(s) for s in slabs) <= 80
    fixed = [np.flatnonzero(s.positions[:, 2] < base.positions[:, 2].max() - 4.0) for s in slabs]
    calc = EnsembleNFFSurface(golden.blobs, device="cuda:0", model_units="kcal/mol", prediction_units="eV", offset_units="atomic")
    calc.set(offset=True, offset_data=golden.offset_data, linesearch_driver="device")
    e0 = [float(r["energy"][0]) for r in calc.calculate_batch(slabs)]
    res = calc.relax_batch(slabs, fixed_indices=fixed, relax_steps=6, fmax=0.01, optimizer="BFGSLineSearch", save_traj=True,
                           record_interval=1)
    for b, (relaxed, traj, energy, oob, r) in enumerate(res):
        E = np.array(traj["energies"])
        print(f"PaiNN chain {b}: steps {r['n_steps']} eval {r['n_eval']} stop {r['stop_reason']}  E0 {e0[b]:.6f}  recorded {E}  final {energy:.6f}")
        assert not oob and r["stop_reason"] in (1, 2, 3) and r["n_steps"] <= 6
        assert r["n_eval"] >= r["n_steps"] + 1
        assert np.array_equal(relaxed.positions[fixed[b]], slabs[b].positions[fixed[b]])
        assert len(E) == r["n_steps"] + 1 and abs(E[0] - e0[b]) <= 2e-4
        assert (np.diff(E) <= 2e-4).all(), E
        assert energy < e0[b] - 1e-3
        assert abs(float(calc.calculate_batch([relaxed])[0]["energy"][0]) - energy) <= 2e-4
        assert abs(E[-1] - energy) <= 2e-4 or r["stop_reason"] == 3
        for k, frame in enumerate(traj["atoms"]):
            assert np.array_equal(frame.positions[fixed[b]], slabs[b].positions[fixed[b]])


def test_front_ends_reach_the_device_optimizer(golden, oracle_mod):
    """relax_batch(optimizer="BFGSLineSearch", linesearch_driver="device") on a LAMMPS-family calculator follows the restatement;
    the default driver still refuses the name; set(linesearch_driver="device") is what mc.ChainEnsemble picks up."""
    from surface_sampling_amd import backend, mc, structures
    from surface_sampling_amd.calculators import EnsembleNFFSurface, TersoffSurfCalc

    c = bc.gan_slab_adatoms(golden)
    numbers = np.where(c.types == 0, 31, 7)
    slab = structures.Structure(numbers, c.pos, c.cell, c.pbc.astype(bool))
    calc = TersoffSurfCalc(golden.tersoff_params, ["Ga", "N"], device="cuda:0")
    with pytest.raises(Exception, match="BFGSLineSearch"):
        calc.relax_batch([slab], fixed_indices=[c.fixed], relax_steps=8, optimizer="BFGSLineSearch")
    out = calc.relax_batch([slab, slab], fixed_indices=[c.fixed, c.fixed], relax_steps=8, fmax=0.01, optimizer="BFGSLineSearch",
                           linesearch_driver="device", save_traj=True, record_interval=4)
    pref, eref, steps, neval, reason, recs = bc.run_restatement(c, golden, oracle_mod, record_interval=4)
    for relaxed, traj, energy, oob, r in out:
        assert (r["n_steps"], r["n_eval"], r["stop_reason"]) == (steps, neval, reason) and not oob
        assert abs(energy - eref) < 1e-9 and np.abs(relaxed.positions - pref).max() < 1e-9
        assert len(traj["atoms"]) == len(recs) == steps // 4 + 1 and abs(traj["energies"][0] - recs[0][2]) < 1e-9
    calc.set(linesearch_driver="device")
    (_, _, energy, _, r), = calc.relax_batch([slab], fixed_indices=[c.fixed], relax_steps=8, optimizer="BFGSLineSearch")
    assert abs(energy - eref) < 1e-9 and r["n_eval"] == neval

    base = golden.structure("SrTiO3_2x2_pristine")
    nff = EnsembleNFFSurface(golden.blobs, device="cuda:0", model_units="kcal/mol", prediction_units="eV", offset_units="atomic")
    nff.set(offset=True, offset_data=golden.offset_data, chem_pots={"Sr": -2, "Ti": 0, "O": 0})
    try:
        import ase.optimize  # noqa: F401
    except Exception:
        with pytest.raises(Exception, match="BFGSLineSearch"):         # the default driver is ASE's class, which is not here
            nff.relax_batch([base], optimizer="BFGSLineSearch")
    nff.set(linesearch_driver="device")
    ztop = base.positions[:, 2].max()
    a, b = base.cell[0], base.cell[1]
    coords = np.array([(i + 0.5) / 2 * a + (j + 0.5) / 2 * b for i in range(2) for j in range(2)], float)
    coords[:, 2] = ztop + 1.5
    fixed = np.flatnonzero(base.positions[:, 2] < ztop - 4.0)
    ens = mc.ChainEnsemble(base, coords, ("Sr", "O"), 3, nff, seed=5, relax=True, relax_steps=2, fmax=0.05, fixed_indices=fixed,
                           temperature=0.5, optimizer="BFGSLineSearch")
    assert not ens._packed_supported()
    e_init = ens.initialize()
    ens.step_semigrand()
    assert np.isfinite(e_init).all() and np.isfinite(ens.state.energy).all()
    lockstep, dispatched = nff._get_engine().last_relax_counts
    assert lockstep >= 3 and dispatched == 3 * lockstep         # the device optimizer ran the three chains in lock step
    assert ens.n_evaluations == 6


def test_raw_abi_null_out_pointers_and_bad_arguments(bench):
    eng, B = bench.eng["pair"], bench.backend
    c = [k for k in bc.all_cases(bench.golden) if k.name == "pair:defaults_4"][0]
    eng.upload([(c.types, c.pos, c.cell, c.pbc)])
    lib, h = eng._lib, eng._h
    good = B.BfgsLsParams.default(max_steps=3)
    assert lib.vssr_batch_relax_bfgs_linesearch(h, C.byref(good), None, 3, None, None, None, None) == 0
    e = eng.results_f64()[0]
    assert np.isfinite(e).all()
    for field, value, word in (("max_steps", -1, b"max_steps"), ("max_eval", 0, b"max_eval"), ("c1", 1.5, b"c1"), ("c1", 0.0, b"c1"),
                               ("c2", 1.0, b"c2"), ("stpmax", 0.5, b"stpmax"), ("fmax", 0.0, b"fmax"), ("alpha", -1.0, b"alpha"),
                               ("maxstep", float("nan"), b"maxstep")):
        p = B.BfgsLsParams.default(max_steps=3)
        setattr(p, field, value)
        assert lib.vssr_batch_relax_bfgs_linesearch(h, C.byref(p), None, 3, None, None, None, None) == -1, field
        assert word in lib.vssr_last_error(h), (field, lib.vssr_last_error(h))
    assert lib.vssr_batch_relax_bfgs_linesearch(h, None, None, 3, None, None, None, None) == -1
    # the handle is still good
    steps = np.zeros(1, np.int32)
    assert lib.vssr_batch_relax_bfgs_linesearch(h, C.byref(good), None, 3, None, steps.ctypes.data_as(C.POINTER(C.c_int32)), None, None) == 0
    assert 0 <= steps[0] <= 3
