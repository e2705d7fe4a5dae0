"""The lock-step FIRE and BFGS step kernels (csrc/relax.hip::k_fire_step, k_bfgs_step) on the cases of tests/relax_cases.py: every
branch that tests/test_relax_cases_cpu.py shows these inputs to reach, step for step against the numpy restatements
(tests/fire_oracle.py, tests/bfgs_oracle.py: forces rounded to float32 as k_narrow_forces does, the ABI's float parameters, a dense
Hessian with numpy's eigh and the device's basis capacity).

Bounds: n_steps and converged exactly; every trajectory record within relax_cases.bound(case) of the restatement's step of the same
index (1e-7 A, the bound of tests/test_pair_gpu_relax.py for these drivers, or 10 x the restatement's own spread under a 1e-12 A
change of the start where that is larger: measured on the CPU, never on the device); held atoms bit for bit; recorded energies within
1e-9 relative (floor 1 eV) of the restatement's potential at the recorded positions, the single-point bound of tests/test_pair_gpu.py.
The CPU file shows that the other branch at any listed step moves the next record by 100 bounds or more."""

import numpy as np
import pytest

import relax_cases as rc

pytestmark = pytest.mark.gpu


def _split(cases, flat):
    o, out = 0, []
    for c in cases:
        out.append(flat[o:o + len(c.types)])
        o += len(c.types)
    return out


class Bench:
    """One pair engine, the restatement's records per (case, parameters) and the device's result per batch: each computed once."""

    def __init__(self):
        from surface_sampling_amd import backend

        self.backend = backend
        self.eng = backend.PairEngine(rc.cc.LJ_TERMS, n_types=rc.cc.LJ_NTYPES, device=0)
        self.want = backend.WANT_ENERGY | backend.WANT_FORCES
        self._ref, self._run = {}, {}

    def ref(self, case):
        key = (case.name, rc._key(case.params))
        if key not in self._ref:
            self._ref[key] = rc.traced(case)
        return self._ref[key]

    def relax(self, eng, cases, params, record_interval=1):
        structs, mask = rc.pack(cases)
        eng.upload(structs)
        call = eng.relax_fire if cases[0].opt == "FIRE" else eng.relax_bfgs
        info = call(fixed=mask, want=self.want, params=rc.c_params(params, self.backend), record_interval=record_interval)
        e, _, f = eng.results_f64()                              # as the relaxation left them on the device: no upload or run in between
        return dict(info, energy=e, forces=f, mask=mask.astype(bool), start=np.concatenate([c.pos for c in cases]))

    def run(self, opt, k):
        if (opt, k) not in self._run:
            params, cases = rc.batches(opt)[k]
            self._run[(opt, k)] = self.relax(self.eng, cases, params)
        return self._run[(opt, k)]


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.eng.close()


def _same(a, b, keys=("positions", "n_steps", "converged", "energy", "forces")):
    return [k for k in keys if not np.array_equal(a[k], b[k])]


def _follow(cases, r, ref_of, fn_of, label):
    """Per-step parity of one relaxed batch.  Returns the worst position and energy figures."""
    tr = r["traj"]
    worst_x = worst_e = 0.0
    assert np.array_equal(r["positions"][r["mask"]], r["start"][r["mask"]]), label
    for b, (c, p_end) in enumerate(zip(cases, _split(cases, r["positions"]))):
        res, rec = ref_of(c)
        got, want = (int(r["n_steps"][b]), bool(r["converged"][b])), (res[2], bool(res[3]))
        nrec = int(tr["n_records"][b])
        print(f"{label} {c.name}: device (steps, converged) {got}  restatement {want}  records {nrec} / {len(rec)}")
        assert got == want, (c.name, got, want)
        assert nrec == len(rec) == res[2] + 1, (c.name, nrec, len(rec))
        held = np.zeros(len(c.types), bool)
        held[c.fixed] = True
        fn, bound = fn_of(c), rc.bound(c)
        dx_case = de_case = 0.0
        for k in range(nrec):
            p = _split(cases, tr["positions"][k])[b]
            assert np.array_equal(p[held], c.pos[held]), (c.name, k)
            dx = float(np.abs(p - rec[k]["pos"]).max())
            E = fn(p)[0]
            de = abs(E - tr["energies"][k, b]) / max(1.0, abs(E))
            if dx > bound or de > 1e-9:
                print(f"{label} {c.name}: record {k}: max|dpos| {dx:.3e} A (bound {bound:.1e})  rel|dE| {de:.3e}")
            assert dx <= bound, (c.name, k, dx, bound)
            assert de <= 1e-9, (c.name, k, de)
            dx_case, de_case = max(dx_case, dx), max(de_case, de)
        dx = float(np.abs(p_end - res[0]).max())
        print(f"{label} {c.name}: max|dpos| over {nrec} records {dx_case:.3e} A, final {dx:.3e} A (bound {bound:.1e})  max rel|dE| {de_case:.3e}")
        assert dx <= bound, (c.name, "final", dx, bound)
        worst_x, worst_e = max(worst_x, dx_case / bound, dx / bound), max(worst_e, de_case)
    return worst_x, worst_e


# a ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["FIRE", "BFGS"])
def test_every_batch_follows_the_restatement_step_for_step(bench, opt):
    """One ragged batch per parameter set: chains that stop before their first step next to chains that run, 2 .. 257 atoms."""
    worst_x = worst_e = 0.0
    for k, (params, cases) in enumerate(rc.batches(opt)):
        r = bench.run(opt, k)
        x, e = _follow(cases, r, bench.ref, rc.force_fn, f"{opt} batch {k}")
        worst_x, worst_e = max(worst_x, x), max(worst_e, e)
        assert (r["n_steps"][-3:] == 0).all() and r["converged"][-3:].all()
        assert r["n_steps"].max() > 0 or params["max_steps"] == 0
    print(f"{opt}: {len(rc.batches(opt))} batches, worst max|dpos| / bound {worst_x:.3f}, worst rel|dE| {worst_e:.3e}")


# b ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["FIRE", "BFGS"])
def test_recording_a_second_run_and_running_alone_change_no_bit(bench, opt):
    """record_interval = 0 against 1, the same batch twice, and every chain that takes a step relaxed alone against the same chain in
    its batch: positions, counts, energies and forces bit for bit."""
    n_alone = 0
    for k, (params, cases) in enumerate(rc.batches(opt)):
        r = bench.run(opt, k)
        assert _same(r, bench.relax(bench.eng, cases, params, record_interval=0)) == [], (opt, k, "record_interval 0")
        again = bench.relax(bench.eng, cases, params)
        assert _same(r, again) == [] and np.array_equal(r["traj"]["n_records"], again["traj"]["n_records"]), (opt, k, "second run")
        for b, (x, y) in enumerate(zip(_split(cases, r["traj"]["positions"].transpose(1, 0, 2)), _split(cases, again["traj"]["positions"].transpose(1, 0, 2)))):
            n = int(r["traj"]["n_records"][b])                   # (entries of a chain beyond its records are unused)
            assert np.array_equal(x[:, :n], y[:, :n]), (opt, k, b, "records of the second run")
        if cases[0].name.split(":")[1].startswith("steps") and params["max_steps"] not in (1, 5):
            continue                                             # (the same chains as in the batches of 1 and 5 steps)
        o = 0
        for b, c in enumerate(cases):
            n = len(c.types)
            if r["n_steps"][b] > 0:
                alone = bench.relax(bench.eng, [c], params, record_interval=0)
                for key in ("positions", "forces"):
                    assert np.array_equal(alone[key], r[key][o:o + n]), (c.name, key)
                for key in ("n_steps", "converged", "energy"):
                    assert np.array_equal(alone[key], r[key][b:b + 1]), (c.name, key)
                n_alone += 1
            o += n
    print(f"{opt}: {n_alone} chains relaxed alone, all bits equal")
    assert n_alone >= 10


# c ---------------------------------------------------------------------------------------------------------------------------------
def test_the_factored_hessian_holds_one_column_per_update_until_98_are_full(bench):
    """40 free atoms (n = 120 > mmax = 98), fmax out of reach, 108 steps: the device follows the dense restatement, whose update is
    skipped once the span of its update vectors leaves fewer than two of 98 dimensions free, through step 50 (a basis that took two
    columns per update would be full there), through iteration 97, where the restatement's basis is full, and for 11 steps behind it.
    Skipping the update of iteration 97 as well as making it moves record 98 by 1e-3 A (tests/test_relax_cases_cpu.py): 1e4 bounds."""
    k, (params, cases) = [(k, b) for k, b in enumerate(rc.batches("BFGS")) if b[1][0].name == "bfgs:capacity_40"][0]
    c = cases[0]
    res, rec = bench.ref(c)
    full = [x["it"] for x in rec if "full_basis" in x["branches"]]
    assert rc.mmax_of(c) == 98 and full and full[0] == 97 and len(full) >= 8 and res[2] == 108 and not res[3]
    assert all("update" in rec[i]["branches"] for i in range(1, 97))
    r = bench.run("BFGS", k)
    tr = r["traj"]
    assert int(r["n_steps"][0]) == 108 and not r["converged"][0] and int(tr["n_records"][0]) == 109
    dx = np.array([np.abs(tr["positions"][i][:len(c.types)] - rec[i]["pos"]).max() for i in range(109)])
    for lo, hi in ((0, 47), (47, 52), (52, 98), (98, 109)):
        print(f"capacity: records {lo} .. {hi - 1}: max|dpos| {dx[lo:hi].max():.3e} A (bound {rc.bound(c):.1e}), restatement m {rec[lo]['m']} .. {rec[hi - 1]['m']}")
    bad = np.flatnonzero(dx > rc.bound(c))
    assert bad.size == 0, f"the device leaves the restatement at record {bad[0]} (max|dpos| {dx[bad[0]]:.3e} A); m of the restatement there: {rec[bad[0] - 1]['m']}"


# d ---------------------------------------------------------------------------------------------------------------------------------
def test_fire_on_tersoff_fragments_resets_uphill_like_the_restatement(bench, golden, oracle_mod):
    """A second fp64 kind: rattled GaN fragments and the Tersoff chains that stop at once, 20 FIRE steps with an uphill reset in every
    running chain (asserted on the restatement's records)."""
    params, cases = rc.tersoff_fire_batch(golden)
    eng = bench.backend.TersoffEngine(golden.tersoff_params, device=0)
    r = bench.relax(eng, cases, params)
    eng.close()
    refs = {c.name: rc.traced(c, fn=rc.tersoff_force_fn(c, golden, oracle_mod)) for c in cases}
    for c in cases[:3]:
        assert "uphill_reset" in rc.reached(c, refs[c.name][1])
    x, e = _follow(cases, r, lambda c: refs[c.name], lambda c: rc.tersoff_force_fn(c, golden, oracle_mod), "FIRE tersoff")
    print(f"FIRE tersoff: worst max|dpos| / bound {x:.3f}, worst rel|dE| {e:.3e}")
    assert r["n_steps"].tolist()[3:] == [0, 0, 0] and r["n_steps"][:3].min() > 3
