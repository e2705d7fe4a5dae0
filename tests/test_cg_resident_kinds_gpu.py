"""The chain-resident CG minimiser (csrc/chain_min.hip) on Stillinger-Weber, EAM (funcfl: untyped bodies; alloy and fs: typed bodies)
and pair (lj/cut; hybrid/overlay born + coul/dsf with charges) handles, selected with ``driver="resident"``
(vssr_batch_relax_cg_driver), against the lock-step driver of the same library (``driver="lockstep"``).

The bound is bit equality of everything a relaxation returns -- positions, energies, per-atom energies, forces, n_iter, n_eval,
stop_reason -- so no tolerance is involved; the lock-step driver is pinned to the numpy restatements for these kinds by
tests/test_sw_gpu.py, test_eam_alloy_gpu.py, test_pair_gpu_relax.py and test_cg_gpu_branches.py.  Inputs: tests/cg_resident_cases.py.
Every relaxation runs with ``rerun=False``: the results are downloaded as the driver left them on the device."""
import ctypes as C

import numpy as np
import pytest

import cell_cases as cl
import cg_resident_cases as rc
import sw_oracle as so

pytestmark = pytest.mark.gpu

KEYS = ("e", "ea", "f", "pos", "it", "ev", "why")


def _relax(eng, structs, mask, driver, max_iter, **kw):
    out = dict(zip(KEYS, eng.relax_cg_f64(structs, fixed=mask, max_iter=max_iter, rerun=False, driver=driver, **kw)))
    out["counts"], out["driver"] = eng.last_relax_counts, eng.last_cg_driver
    return out


def _assert_equal(a, b, tag):
    for key in KEYS:
        if not np.array_equal(a[key], b[key]):
            d = np.abs(np.asarray(a[key], float) - np.asarray(b[key], float))
            raise AssertionError(f"{tag}: {key} differs, max |d| {np.nanmax(d):.3e} at {int(np.nanargmax(d))} of {d.size}")
    assert np.isfinite(a["e"]).all() and np.isfinite(a["f"]).all(), tag


class Bench:
    """One engine per kind; the lock-step and the chain-resident relaxation of its ragged batch, computed once and shared."""

    def __init__(self, golden):
        self.golden, self.eng, self._ragged = golden, {}, {}

    def engine(self, kind):
        if kind not in self.eng:
            self.eng[kind] = rc.engine(kind)
        return self.eng[kind]

    def ragged(self, kind):
        if kind not in self._ragged:
            structs, mask, max_iter = rc.ragged(kind, self.golden)
            eng = self.engine(kind)
            lock = _relax(eng, structs, mask, "lockstep", max_iter)
            res = _relax(eng, structs, mask, "resident", max_iter)
            self._ragged[kind] = (structs, mask, max_iter, lock, res)
        return self._ragged[kind]

    def close(self):
        for e in self.eng.values():
            e.close()


@pytest.fixture(scope="module")
def bench(golden):
    b = Bench(golden)
    yield b
    b.close()


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.KINDS)
def test_ragged_batch_with_held_atoms_equals_the_lock_step_driver(bench, kind):
    """Chains of different sizes that stop at >= 3 different evaluation counts, some atoms held: the same bits from both drivers, one
    launch against many, and exactly the chains' own evaluations dispatched (every chain makes one setup evaluation that n_eval,
    like LAMMPS, does not count)."""
    structs, mask, max_iter, lock, res = bench.ragged(kind)
    print(f"{kind}: atoms {[len(s[0]) for s in structs]}  n_iter {res['it'].tolist()}  n_eval {res['ev'].tolist()}  stop {res['why'].tolist()}"
          f"  counts lock-step {lock['counts']} resident {res['counts']}")
    assert len(set(res["ev"].tolist())) >= 3
    _assert_equal(res, lock, kind)
    assert res["driver"] == "resident" and lock["driver"] == "lockstep"
    assert res["counts"][0] == 1 and lock["counts"][0] > 1
    assert res["counts"][1] == int(res["ev"].sum()) + len(structs)
    assert lock["counts"][1] >= res["counts"][1]
    held = mask.astype(bool)
    start = np.concatenate([s[1] for s in structs])
    assert held.any() and np.array_equal(res["pos"][held], start[held])
    assert np.abs(res["pos"][~held] - start[~held]).max() > 1e-3          # (something was minimised)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.KINDS)
def test_tile_limits(bench, kind):
    """Chains of 1, 63, 64, 65, 255 and 256 atoms in one batch (64-centre site tiles, one atom per thread in the row scan), max_iter = 5:
    bit-equal; one more chain of 257 atoms sends the whole batch to the lock-step driver and leaves the shared chains unchanged."""
    eng = bench.engine(kind)
    structs, mask = rc.size_batch(kind)
    assert [len(s[0]) for s in structs] == [1, 63, 64, 65, 255, 256]
    lock = _relax(eng, structs, mask, "lockstep", 5)
    res = _relax(eng, structs, mask, "resident", 5)
    print(f"{kind}: n_iter {res['it'].tolist()}  n_eval {res['ev'].tolist()}  stop {res['why'].tolist()}  regrows {eng.debug_capacity()}")
    assert res["driver"] == "resident" and lock["driver"] == "lockstep"
    _assert_equal(res, lock, kind)
    assert (res["it"][1:] >= 1).all()
    more, mask257 = rc.size_batch(kind, with_257=True)
    big = _relax(eng, more, mask257, "resident", 5)
    assert big["driver"] == "lockstep" and big["counts"][0] > 1
    n = len(res["ea"])
    for key in KEYS:
        m = n if key in ("pos", "ea", "f") else len(structs)
        assert np.array_equal(big[key][:m], res[key]), (kind, key)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_sw_rows_beyond_the_lds_tile_take_the_long_row_form_inside_the_kernel(bench):
    structs, mask = rc.sw_crowded()
    for s in structs:
        deg = np.bincount(cl.brute_neighbors(s[1], s[2], s[3], so.cutoff(so.si_params()))[0], minlength=len(s[0]))
        assert deg.max() > 16 and deg.min() <= 16, (deg.min(), deg.max())
    eng = bench.engine("sw")
    lock = _relax(eng, structs, mask, "lockstep", 10)
    res = _relax(eng, structs, mask, "resident", 10)
    assert res["driver"] == "resident"
    _assert_equal(res, lock, "sw crowded")


def test_pair_rows_of_hundreds_of_slots_regrow_the_pools(bench):
    """born 8 A + coul/dsf 12 A on the 5.64 A rocksalt cube: rows of more than 300 slots over several images of the cell against pools of
    64 slots per atom.  The pools double until the rows fit, the chains resume, and no bit differs from the lock-step run."""
    import pair_cases as pc

    structs, mask = rc.rocksalt_long_rows()
    assert pc.degrees(structs[0], 12.0).min() > 300
    lock = _relax(bench.engine("pair_born_dsf"), structs, mask, "lockstep", 10)
    fresh = rc.engine("pair_born_dsf")
    res = _relax(fresh, structs, mask, "resident", 10)
    regrows = fresh.debug_capacity()
    again = _relax(fresh, structs, mask, "resident", 10)       # (the grown pools stay with the driver: no regrow the second time)
    regrows_again = fresh.debug_capacity()
    fresh.close()
    print(f"rocksalt: regrows {regrows}, then {regrows_again}; launches {res['counts'][0]}, then {again['counts'][0]}")
    assert res["driver"] == "resident" and regrows >= 1 and res["counts"][0] == 1 + regrows
    assert regrows_again == 0 and again["counts"][0] == 1
    _assert_equal(res, lock, "rocksalt")
    _assert_equal(again, lock, "rocksalt, grown pools")


@pytest.mark.parametrize("kind", rc.KINDS)
def test_pools_of_four_slots_per_atom_overflow_regrow_and_resume(bench, kind):
    """debug_capacity(slots_per_atom=4): a row takes at least 8 slots, so every chain overflows at its first evaluation; the pools are
    regrown and the chains resume.  Bit-equal to the runs without overflow."""
    structs, mask, max_iter, lock, res = bench.ragged(kind)
    small = rc.engine(kind)
    small.debug_capacity(slots_per_atom=4)
    again = _relax(small, structs, mask, "resident", max_iter)
    regrows = small.debug_capacity()
    small.close()
    print(f"{kind}: regrows {regrows}, launches {again['counts'][0]}")
    assert again["driver"] == "resident" and regrows >= 1 and again["counts"][0] == 1 + regrows
    _assert_equal(again, res, kind)
    _assert_equal(again, lock, kind)


# (lock-step evaluations roomy, tight; regrows) of the run below as commit 809cdf4 returns them
LOCKSTEP_REGROW_COUNTS_809CDF4 = (57, 81, 3)


def test_the_lock_step_driver_regrows_and_gives_its_poll_window_back(bench):
    """The same pools under the lock-step driver, regrown to the exact need: the evaluations of a poll window overflow, the driver
    regrows and repeats the window.  Bit-equal to the run without overflow."""
    kind = rc.KINDS[0]
    structs, mask, max_iter, lock, _ = bench.ragged(kind)
    small = rc.engine(kind)
    small.debug_capacity(slots_per_atom=4, tight=1)
    again = _relax(small, structs, mask, "lockstep", max_iter)
    regrows = small.debug_capacity()
    small.close()
    print(f"{kind}: roomy counts {lock['counts']}; tight counts {again['counts']} regrows {regrows}")
    assert again["driver"] == "lockstep" and regrows >= 1 and again["counts"][0] > lock["counts"][0]
    _assert_equal(again, lock, kind)
    assert (lock["counts"][0], again["counts"][0], regrows) == LOCKSTEP_REGROW_COUNTS_809CDF4


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.KINDS)
def test_a_different_cell_on_every_chain(bench, kind):
    """A skewed slab cell, a partly periodic cell with a sheared open vector and two thin cells whose neighbors are their own images
    (one beyond 64 images) in one batch: bit-equal to the lock-step driver and to every chain relaxed alone."""
    eng = bench.engine(kind)
    structs, mask = rc.cell_batch(kind)
    rcut = rc.cutoff(kind)
    imgs = [cl.n_images(cl.face_nimg(s[2], s[3].astype(bool), rcut)) for s in structs]
    assert max(imgs) > 64 and any(max(cl.face_nimg(s[2], s[3].astype(bool), rcut)) >= 2 for s in structs)
    assert any(not s[3].all() for s in structs) and any(abs(s[2][0, 1]) + abs(s[2][1, 0]) > 1e-6 for s in structs)
    lock = _relax(eng, structs, mask, "lockstep", 10)
    res = _relax(eng, structs, mask, "resident", 10)
    print(f"{kind}: images {imgs}  n_iter {res['it'].tolist()}  n_eval {res['ev'].tolist()}  stop {res['why'].tolist()}")
    assert res["driver"] == "resident"
    _assert_equal(res, lock, kind)
    o = 0
    for b, s in enumerate(structs):
        n = len(s[0])
        alone = _relax(eng, [s], mask[o:o + n], "resident", 10)
        assert alone["driver"] == "resident"
        for key in KEYS:
            want = res[key][o:o + n] if key in ("pos", "ea", "f") else res[key][b:b + 1]
            assert np.array_equal(alone[key], want), (kind, b, key)
        o += n


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.KINDS)
def test_post_state_of_the_handle(bench, kind):
    """Behind a chain-resident relaxation, without upload or run: vssr_batch_results_f64 serves the static results of the returned
    positions bit for bit; vssr_batch_stress and vssr_batch_stats (no batch-wide graph) return VSSR_E_STATE until one run(), then work."""
    from surface_sampling_amd import backend

    structs, mask, max_iter, lock, _ = bench.ragged(kind)
    eng = bench.engine(kind)
    res = _relax(eng, structs, mask, "resident", max_iter)
    assert res["driver"] == "resident"
    for a, b in zip(eng.results_f64(), (res["e"], res["ea"], res["f"])):
        assert np.array_equal(a, b)
    for call in (eng.stress, eng.stats, eng.neighbors):
        with pytest.raises(backend.BackendError, match=r"vssr error -5: .*run the batch once"):
            call()
    eng.run(backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM)
    st = eng.stress()[0]
    stats = eng.stats()
    assert np.isfinite(st).all() and st.shape == (len(structs), 6)
    assert stats["atoms"] == len(mask) and stats["slots"] >= stats["edges"] > 0
    after_run = eng.results_f64()
    n_atoms, T, _, cell, pbc = backend.pack_batch(structs)
    fresh = eng.evaluate_arrays_f64(n_atoms, T, res["pos"], cell, pbc)
    for name, a, b, c in zip(("energy", "per-atom energy", "forces"), (res["e"], res["ea"], res["f"]), fresh, after_run):
        assert np.array_equal(a, b), (kind, name, "fresh evaluation")
        assert np.array_equal(a, c), (kind, name, "run on the resident batch")
    assert np.array_equal(st, eng.stress()[0])                                # (the stress of those geometries, from either graph)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_precedence_of_environment_handle_setting_and_automatic_rule(bench, golden, monkeypatch):
    from surface_sampling_amd import backend

    monkeypatch.delenv("VSSR_CG_FUSED", raising=False)
    small = {}
    for kind in ("sw", "eam_funcfl", "eam_fs", "pair_lj"):
        structs, mask, max_iter, lock, res = bench.ragged(kind)
        eng = bench.engine(kind)
        auto = _relax(eng, structs, mask, "auto", max_iter)                   # the automatic rule is Tersoff's alone
        assert auto["driver"] == "lockstep" and auto["counts"][0] > 1, kind
        _assert_equal(auto, lock, kind)
        small[kind] = (eng, structs, mask, max_iter, lock)
    eng, structs, mask, max_iter, lock = small["sw"]
    monkeypatch.setenv("VSSR_CG_FUSED", "0")                                   # 0: lock step, whatever the handle says
    off = _relax(eng, structs, mask, "resident", max_iter)
    assert off["driver"] == "lockstep" and off["counts"][0] > 1
    _assert_equal(off, lock, "sw, VSSR_CG_FUSED=0")
    monkeypatch.setenv("VSSR_CG_FUSED", "1")                                   # 1: Tersoff only; the other kinds follow their handle
    eng, structs, mask, max_iter, lock = small["pair_lj"]
    on = _relax(eng, structs, mask, "auto", max_iter)
    assert on["driver"] == "lockstep" and on["counts"][0] > 1
    on = _relax(eng, structs, mask, "resident", max_iter)
    assert on["driver"] == "resident" and on["counts"][0] == 1
    monkeypatch.delenv("VSSR_CG_FUSED")
    # a 48-atom Tersoff batch: chain-resident by the automatic rule, lock step on request, the same bits
    gan = backend.TersoffEngine(golden.tersoff_params, device=0)
    assert gan.cg_driver() is None                                             # (no CG relaxation yet)
    structs, mask = rc.gan48(golden)
    auto = _relax(gan, structs, mask, "auto", 20)
    lock = _relax(gan, structs, mask, "lockstep", 20)
    assert auto["driver"] == "resident" and auto["counts"][0] == 1 and lock["driver"] == "lockstep" and lock["counts"][0] > 1
    _assert_equal(auto, lock, "GaN 48")
    monkeypatch.setenv("VSSR_CG_FUSED", "1")                                   # today's meaning for Tersoff: the knob goes first
    forced = _relax(gan, structs, mask, "lockstep", 20)
    assert forced["driver"] == "resident"
    monkeypatch.delenv("VSSR_CG_FUSED")
    # refusals of the entry point: the value 3, a PaiNN handle (VSSR_E_BADARG = -1); a negative value only reads
    lib, last = gan._lib, C.c_int32(-7)
    assert lib.vssr_batch_relax_cg_driver(gan._h, 3, C.byref(last)) == -1 and b"driver 3" in lib.vssr_last_error(gan._h)
    assert lib.vssr_batch_relax_cg_driver(gan._h, -1, C.byref(last)) == 0 and last.value == 2
    gan.close()
    table, const = golden.offset_table()
    painn = backend.PainnEngine(golden.blobs, device=0, offset_per_z=table, offset_const=const)
    for value in (0, 2, -1):
        assert lib.vssr_batch_relax_cg_driver(painn._h, value, None) == -1
        assert b"PaiNN" in lib.vssr_last_error(painn._h)
    painn.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_chain_ensemble_with_cg_driver_resident_reproduces_the_lock_step_trajectory():
    """8 chains of semigrand MC on the Si adatom sites (tests/test_sw_gpu.py), a CG relaxation per proposal through the packed path:
    ``cg_driver="resident"`` gives the occupations, accept flags and energies of ``cg_driver="lockstep"`` exactly."""
    from surface_sampling_amd import mc
    from surface_sampling_amd.calculators import SWSurfCalc
    from surface_sampling_amd.structures import Structure
    from test_sw_gpu import _adatom_sites

    Z, X, Cl, pbc, fixed = so.si_slab()
    g = Structure(Z, X, Cl, pbc)
    held = np.flatnonzero(fixed)
    sites = _adatom_sites(X, Cl)
    runs = {}
    for driver in ("lockstep", "resident"):
        calc = SWSurfCalc(so.SI_1985, device="cuda:0")
        calc.set(relax_steps=25, cg_driver=driver)
        ens = mc.ChainEnsemble(g, sites, ("Si",), 8, calc, seed=3, relax=True, relax_steps=25, fixed_indices=held, temperature=0.5,
                               optimizer="LAMMPS")
        ens.initialize()
        accepts = [np.asarray(ens.step_semigrand()).copy() for _ in range(3)]
        eng = calc._get_engine()
        assert eng.last_cg_driver == driver and (eng.last_relax_counts[0] == 1) == (driver == "resident")
        runs[driver] = (ens.state.species.copy(), ens.state.energy.copy(), np.array(accepts),
                        np.concatenate([ens.relaxed[b].positions for b in range(8)]))
        assert (ens.num_adsorbates() > 0).any()
        eng.close()
    for a, b in zip(runs["lockstep"], runs["resident"]):
        assert np.array_equal(a, b)
