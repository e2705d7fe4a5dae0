"""Relaxations, capacity regrows and handle reuse of the pair potentials on the MI355X: the lock-step CG, FIRE and BFGS drivers on a
ragged, charged, three-type batch (OVERLAY5) step for step against tests/cg_oracle.py, fire_oracle.py and bfgs_oracle.py over the
restatement tests/pair_oracle.py; the active mask of k_pair_site and live-chain compaction; trajectory records; stress after a
relaxation; neighbor capacities that overflow and regrow; one engine over several batches.  Tolerances are those of
tests/test_eam_alloy_gpu.py for the same drivers and precision, and of tests/test_pair_gpu.py for single points."""
import numpy as np
import pytest

import pair_cases as pc
import pair_oracle as po
import strain_fd as sf
from test_pair_gpu import STRESS_FACTOR, _check, _engine, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def overlay():
    m = _model(pc.OVERLAY5, 3)
    terms, q = po.model_of(m)
    return m, terms, q


def _fn(terms, q, T, Cl, pbc):
    def fn(p):
        E, _, F = po.pair(terms, q, T, p, Cl, pbc)
        return E, F
    return fn


def _split(chains, flat):
    o, out = 0, []
    for c in chains:
        out.append(flat[o:o + len(c[0])])
        o += len(c[0])
    return out


def _rocksalt():
    T, X, C = po.rocksalt(5.64)
    return T, X + np.random.default_rng(21).normal(0, 0.05, X.shape), C, np.ones(3, np.uint8)


# 4 --------------------------------------------------------------------------------------------------------------------------------
def test_cg_follows_the_restatement(overlay):
    from cg_oracle import cg_minimize

    m, terms, q = overlay
    chains, mask = pc.relax_batch()
    eng = _engine(m)
    e, ea, f, pos, it, ev, why = eng.relax_cg_f64(chains, fixed=mask, max_iter=30)
    print(f"CG: lock-step evaluations {eng.last_relax_counts}")
    assert eng.last_relax_counts[0] > 1                           # the lock-step driver serves this kind
    for b, ((T, X, Cl, pbc), p) in enumerate(zip(chains, _split(chains, pos))):
        fn = _fn(terms, q, T, Cl, pbc)
        pref, eref, niter, neval, reason, _ = cg_minimize(fn, X, fixed=np.arange(2), max_iter=30)
        e0 = fn(X)[0]
        print(f"CG chain {b}: device (iter, eval, stop) {(it[b], ev[b], why[b])}  restatement {(niter, neval, reason)}  E {e0:.9f} -> {eref:.9f}"
              f"  |dE| {abs(e[b] - eref):.2e}  max|dpos| {np.abs(p - pref).max():.2e}")
        assert (it[b], ev[b], why[b]) == (niter, neval, reason), (b, it[b], ev[b], why[b], niter, neval, reason)
        assert abs(e[b] - eref) < 1e-9 and np.abs(p - pref).max() < 1e-9
        assert eref < e0 - 0.1 and np.array_equal(p[:2], X[:2])
    eng.close()


@pytest.mark.parametrize("optimizer", ["FIRE", "BFGS"])
def test_fire_and_bfgs_follow_the_restatements(overlay, optimizer):
    """12 steps, equal step counts, positions to 1e-7 A and |E - restatement(reference positions)| < 1e-7 eV, the bounds of
    tests/test_eam_alloy_gpu.py for the same drivers.  The restatement runs with the optimizer parameters the device runs with:
    vssr_fire_params / vssr_bfgs_params carry them as C floats, so dt = 0.1 arrives as 0.100000001490116 and maxstep = 0.2 as
    0.200000002980232.  With fp64 values on one side only, these chains (0.7 - 0.9 A of travel in 12 steps, 5 - 10 eV/A from rest)
    end 2e-8 A apart and 1.2e-7 eV apart in energy: measured, and no property of either implementation."""
    from bfgs_oracle import bfgs_relax
    from fire_oracle import fire_relax
    from surface_sampling_amd import backend

    m, terms, q = overlay
    chains, mask = pc.relax_batch()
    eng = _engine(m)
    e, ea, f, pos, nst, conv = eng.relax_f64(chains, fixed=mask, max_steps=12, fmax=0.01, optimizer=optimizer)
    relax = fire_relax if optimizer == "FIRE" else bfgs_relax
    p0 = backend.FireParams.default(12, 0.01) if optimizer == "FIRE" else backend.BfgsParams.default(12, 0.01)
    given = {k: getattr(p0, k) for k, _ in p0._fields_ if k != "max_steps"}          # the values as the ABI's floats hold them
    assert given["maxstep"] == float(np.float32(0.2)) and given["fmax"] == float(np.float32(0.01))
    for b, ((T, X, Cl, pbc), p) in enumerate(zip(chains, _split(chains, pos))):
        fn = _fn(terms, q, T, Cl, pbc)
        pref, _, steps, _ = relax(fn, X, fixed=np.arange(2), max_steps=12, **given)
        eref = fn(pref)[0]
        print(f"{optimizer} chain {b}: steps {nst[b]} / {steps}  E {eref:.9f}  |dE| {abs(e[b] - eref):.2e}  max|dpos| {np.abs(p - pref).max():.2e}")
        assert nst[b] == steps
        assert np.abs(p - pref).max() < 1e-7 and abs(e[b] - eref) < 1e-7
        assert np.array_equal(p[:2], X[:2])
    eng.close()


def _eight_chains(eng):
    """Seven fresh chains of the three ragged shapes and an already relaxed copy of the first (CG to its energy tolerance on the
    device): the copy stops after a few evaluations, the others run on."""
    chains = [pc.grid_chain(pc.RELAX_SHAPES[k % 3][0], 80 + k, pc.RELAX_SHAPES[k % 3][1]) for k in range(7)]
    T, X, Cl, pbc = chains[0]
    _, _, _, pos, it, _, why = eng.relax_cg_f64([chains[0]], fixed=pc.held_mask(chains[:1]), max_iter=60)
    print(f"relaxed copy: {it[0]} iterations, stop {why[0]}")
    assert it[0] < 60                                             # (it met a tolerance; it did not run out of iterations)
    chains.append((T, pos.copy(), Cl, pbc))
    return chains, pc.held_mask(chains)


def test_compaction_the_active_mask_and_trajectory_records_change_nothing(overlay, monkeypatch):
    """Eight chains that stop at different times (asserted): VSSR_RELAX_COMPACT=0 against 2 bit for bit, every chain relaxed alone
    (CG and FIRE) against the same chain in the batch bit for bit -- a stopped chain's atoms are masked out of k_pair_site while its
    neighbors in the batch go on -- and FIRE trajectory records whose energies are the restatement's at the recorded positions.
    FIRE's force tolerance is 1e-4 eV/A so that no chain, the relaxed copy included, converges before the second record."""
    from surface_sampling_amd import backend

    m, terms, q = overlay
    eng = _engine(m)
    chains, mask = _eight_chains(eng)
    runs = []
    for flag in ("0", "2"):
        monkeypatch.setenv("VSSR_RELAX_COMPACT", flag)
        runs.append(eng.relax_cg_f64(chains, fixed=mask, max_iter=30))
    monkeypatch.delenv("VSSR_RELAX_COMPACT")
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    ev = runs[0][5]
    print(f"compaction: evaluations per chain {ev.tolist()}, iterations {runs[0][4].tolist()}, stop {runs[0][6].tolist()}")
    assert ev.min() < ev.max()
    fire = eng.relax_f64(chains, fixed=mask, max_steps=12, fmax=0.01, optimizer="FIRE")
    o = 0
    for b, c in enumerate(chains):
        n = len(c[0])
        alone = eng.relax_cg_f64([c], fixed=mask[o:o + n], max_iter=30)
        for k, (x, y) in enumerate(zip(alone, runs[0])):
            assert np.array_equal(x, y[b:b + 1] if y.shape[0] == len(chains) else y[o:o + n]), ("CG", b, k)
        alone = eng.relax_f64([c], fixed=mask[o:o + n], max_steps=12, fmax=0.01, optimizer="FIRE")
        for k, (x, y) in enumerate(zip(alone, fire)):
            assert np.array_equal(x, y[b:b + 1] if y.shape[0] == len(chains) else y[o:o + n]), ("FIRE", b, k)
        o += n
    eng.upload(chains)
    info = eng.relax_fire(fixed=mask, max_steps=12, fmax=1e-4, want=backend.WANT_ENERGY | backend.WANT_FORCES, record_interval=4)
    tr = info["traj"]
    print(f"trajectory: records per chain {tr['n_records'].tolist()}, steps {info['n_steps'].tolist()}")
    assert (tr["n_records"] >= 2).all()
    worst = 0.0
    for b, (T, _, Cl, pbc) in enumerate(chains):
        for r in range(int(tr["n_records"][b])):
            E = po.pair(terms, q, T, _split(chains, tr["positions"][r])[b], Cl, pbc)[0]
            worst = max(worst, abs(E - tr["energies"][r, b]) / abs(E))
            assert abs(E - tr["energies"][r, b]) <= 1e-9 * abs(E), (b, r)
    print(f"trajectory: max relative |dE| of a record {worst:.2e}")
    eng.close()


def test_stress_after_a_lock_step_fire_is_that_of_the_final_geometry(overlay):
    """12 FIRE steps towards a force tolerance no chain reaches: the relaxation ends with its batch-wide evaluation of the final
    positions, so the stress call succeeds directly, equals a fresh engine's for those positions bit for bit and is the strain
    derivative of the restatement there (OVERLAY5 shifts its energies, and no pair is within 0.005 A of a cutoff: asserted)."""
    from surface_sampling_amd import backend

    m, terms, q = overlay
    chains, mask = pc.relax_batch(pc.STRESS_SEEDS)
    eng = _engine(m)
    eng.upload(chains)
    info = eng.relax_fire(fixed=mask, max_steps=12, fmax=1e-9, want=backend.WANT_ENERGY | backend.WANT_FORCES)
    assert not info["converged"].any() and np.abs(info["positions"] - np.concatenate([c[1] for c in chains])).max() > 1e-2
    st = eng.stress()[0]
    eng.close()
    relaxed = [(T, p, Cl, pbc) for (T, _, Cl, pbc), p in zip(chains, _split(chains, info["positions"]))]
    fresh = _engine(m)
    fresh.evaluate_f64(relaxed)
    assert np.array_equal(st, fresh.stress()[0])
    fresh.close()
    for b, (T, X, Cl, pbc) in enumerate(relaxed):
        assert pc.cutoff_margin(m, relaxed[b]) > 0.005
        chk = sf.fd_stress(lambda x, c: po.pair(terms, q, T, x, c, pbc)[0], X, Cl)
        dev = st[b] * chk.volume
        print(f"stress after FIRE chain {b}: device {dev}  checker {chk.virial}  unc {chk.unc}  max ratio {(np.abs(dev - chk.virial) / chk.unc).max():.3f}")
        assert (np.abs(dev - chk.virial) <= STRESS_FACTOR * chk.unc).all(), (b, dev, chk.virial, chk.unc)


# 5 --------------------------------------------------------------------------------------------------------------------------------
def test_a_neighbor_capacity_that_overflows_regrows_and_changes_no_bit(overlay):
    """debug_capacity(slots_per_atom=1, tight=1): the rattled rocksalt cube (rows of more than 300 slots) overflows at its first run
    and regrows to the exact need; stress() right after is where the per-slot gradient buffer has to follow the new capacity.  The
    same setting in front of a 12-step FIRE and a lock-step CG of the ragged batch: every returned array as without it."""
    m, _, _ = overlay
    rock_m = _model(po.ROCKSALT_COMMANDS, 2)
    rock = _rocksalt()
    assert pc.degrees(rock, 12.0).min() > 300
    ref = _engine(rock_m)
    want = _check(ref, rock_m, [rock], "rocksalt untight") + (ref.stress()[0],)
    ref.close()
    eng = _engine(rock_m)
    eng.debug_capacity(slots_per_atom=1, tight=1)
    got = eng.evaluate_f64([rock])
    got = got + (eng.stress()[0],)
    stats = eng.stats()
    print(f"tight single point: {stats}")
    # one slot per atom to start with: a first run that needs more slots than atoms has overflowed, and it ended with rows for every edge
    assert stats["slots"] >= stats["edges"] > stats["atoms"] == 8
    eng.close()
    for k, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a, b), k
    chains, mask = pc.relax_batch()
    plain, tight = _engine(m), _engine(m)
    for name, run in (("FIRE", lambda e: e.relax_f64(chains, fixed=mask, max_steps=12, fmax=0.01, optimizer="FIRE")),
                      ("CG", lambda e: e.relax_cg_f64(chains, fixed=mask, max_iter=30))):
        a = run(plain)
        tight.debug_capacity(slots_per_atom=1, tight=1)
        b = run(tight)
        print(f"tight {name}: regrows {tight.debug_capacity()} (untight {plain.debug_capacity()})")
        assert tight.debug_capacity() >= 1
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (name, k)
    plain.close(); tight.close()


def test_one_engine_serves_three_batches_and_stress_leaves_the_results_alone(overlay):
    """The ragged batch, the rocksalt cube (another type count in use, rows ten times as long), the ragged batch again: the third
    result is the first bit for bit and stress() after each is a fresh engine's.  stress() launches the site kernel once more in
    its gradient form: a download after it returns what a download before it returned."""
    from surface_sampling_amd import backend

    m, _, _ = overlay
    chains, _ = pc.relax_batch()
    rock = _rocksalt()                                            # (its types 0 and 1 are two of OVERLAY5's three)
    eng = _engine(m)
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    out = []
    for batch in (chains, [rock], chains):
        res = eng.evaluate_f64(batch)
        before = eng.download(want)
        st = eng.stress()[0]
        after = eng.download(want)
        for k in ("energy", "energy_f64", "forces", "energy_atoms"):
            assert np.array_equal(before[k], after[k]), k
        fresh = _engine(m)
        res_f = fresh.evaluate_f64(batch)
        st_f = fresh.stress()[0]
        fresh.close()
        for a, b in zip(res + (st,), res_f + (st_f,)):
            assert np.array_equal(a, b)
        assert np.isfinite(st).all() and np.abs(st).max() > 0
        out.append(res + (st,))
    for a, b in zip(out[0], out[2]):
        assert np.array_equal(a, b)
    eng.close()
