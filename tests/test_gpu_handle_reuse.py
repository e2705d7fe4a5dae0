"""A long-lived handle gives every call the bits of a fresh one (MI355X).  Every driver of the library runs on one ``vssr_handle`` that
keeps scratch, arenas, flags and sizes between calls; the other device tests run each driver on a handle of its own, or repeat one
driver.  Here ONE engine per kind runs a schedule of episodes of tests/handle_reuse_cases.py -- every ordered pair of the drivers that
share the optimizer workspaces adjacent at least once, batches that grow and shrink, the hit masks switched on and off, a tight and
regrowing neighbor pool from the K episode on -- and every episode's result is compared, byte for byte (NaNs included), with the
result of the same episode on a brand-new engine, computed once per distinct (kind, episode type, inputs).  So that "fresh" is not
merely self-consistent, the fresh single-point results are pinned to the kind's fp64 oracle at the bounds of the kind's own test file.
``relax_counts()`` and the regrow count depend on the history by design: printed, not compared."""
import numpy as np
import pytest

import handle_reuse_cases as hc

pytestmark = pytest.mark.gpu

_REFS = {}


def _fresh(kind, etype, size, golden):
    """The result of an episode on a brand-new engine: computed once, then left unchanged."""
    inp = hc.inputs(kind, etype, size, golden)
    key = (kind, etype, size)
    if key not in _REFS:
        eng = hc.engine(kind, golden)
        try:
            print(f"  fresh {kind} {etype}/{size}:")
            _REFS[key] = hc.run_episode(eng, kind, etype, inp)
        finally:
            eng.close()
        for _, a in _REFS[key]:
            a.setflags(write=False)
    return _REFS[key], inp


def _run_schedule(kind, golden):
    sched = hc.schedule(kind)
    eng = hc.engine(kind, golden)
    try:
        before = None
        for step, (etype, size) in enumerate(sched):
            ref, inp = _fresh(kind, etype, size, golden)
            print(f"  step {step} {kind} {etype}/{size} {hc.totals(inp)}:")
            got = hc.run_episode(eng, kind, etype, inp)
            diff = hc.first_difference(got, ref, inp)
            assert diff is None, (f"{kind}: step {step}, episode {etype}/{size} after {before}: output {diff[0]!r} differs from the fresh "
                                  f"handle's ({diff[1]}), first differing chain {diff[2]}")
            before = f"{etype}/{size}"
        return eng, sched
    except BaseException:
        eng.close()
        raise


# ---- the fresh results against the fp64 oracles -----------------------------------------------------------------------------------------
# (E relative with a floor of 1 eV, per-atom energies in eV, forces in eV / A): the bounds of the kind's own device test file
BOUNDS = {"pair_lj": (1e-10, 1e-9, 1e-8),         # tests/test_pair_gpu.py: E_REL, EA_ABS, F_ABS
          "pair_born_dsf": (1e-10, 1e-9, 1e-8),   # tests/test_pair_gpu.py
          "tersoff": (1e-9, 1e-9, 1e-8),          # tests/test_gpu_cells.py::test_analytic_cases_and_variants_match_the_oracle
          "sw": (1e-10, 1e-9, 1e-8),              # tests/test_sw_gpu.py::_check
          "eam_alloy": (1e-9, 1e-9, 1e-8),        # tests/test_eam_alloy_gpu.py::_check
          "adp": (1e-9, 1e-9, 1e-8),              # tests/test_adp_gpu.py: E_REL, EA_ABS, F_ABS
          "vashishta": (1e-10, 1e-9, 1e-8),       # tests/test_vashishta_gpu.py::_check
          "ewald": (1e-10, 1e-9, 1e-8)}           # tests/test_ewald_gpu.py: E_REL, EA_ABS, F_ABS
PAINN_E_TOL, PAINN_F_TOL = 1e-4, 2e-4             # tests/test_gpu_parity.py: E_TOL, F_TOL (eV, eV / A); tests/test_gpu_painn_widths.py has the same


def _oracle(kind, golden, oracle_mod):
    """struct -> (E, per-atom energies, forces) of the kind's fp64 oracle."""
    import cg_cases as cc
    import cg_resident_cases as rc
    import pair_oracle as po

    if kind == "pair_lj":
        return lambda s: po.pair(cc.LJ_TERMS, None, *s)
    if kind == "pair_born_dsf":
        terms, q = po.model_of(rc.born_dsf_model())
        return lambda s: po.pair(terms, q, *s)
    if kind == "tersoff":
        P = hc.cl.gan_params()
        return lambda s: oracle_mod.tersoff(P, *s)
    if kind == "sw":
        import sw_oracle as so

        P = so.si_params()
        return lambda s: so.sw(P, *s)[:3]
    if kind == "eam_alloy":
        import eam_alloy_oracle as ao

        tab = rc.eam_tables("eam_alloy")
        return lambda s: ao.eam_typed(tab, *s)[:3]
    if kind == "adp":
        import adp_oracle as adp

        tab = hc._adp_tables()
        return lambda s: adp.adp(tab, *s)[:3]
    if kind == "vashishta":
        import vashishta_oracle as vo

        P = vo.sic_params()[1]
        return lambda s: vo.vashishta(P, *s)[:3]
    import ewald_oracle as eo

    terms, q, ks = eo.model_of(hc._ewald_model())
    return lambda s: eo.ewald(terms, q, ks, s[0], s[1], s[2])[:3]


@pytest.mark.parametrize("size", ["S", "G"])
@pytest.mark.parametrize("kind", hc.KINDS)
def test_fresh_single_points_match_the_fp64_oracle(kind, size, golden, oracle_mod):
    ref, inp = _fresh(kind, "E", size, golden)
    out = dict(ref)
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in inp.structs])])
    if kind in hc.PAINN_KINDS:
        blobs, hp = hc.painn_blobs(kind, golden)
        ohp = oracle_mod.default_hparams(**{k: hp[k] for k in ("feat_dim", "n_rbf", "num_conv", "readout_hidden")}) if hp else None
        for b, s in enumerate(inp.structs):
            o = oracle_mod.ensemble(blobs, *s, 64, hp=ohp)
            de = abs(float(out["download.energy_f64"][b]) - o["energy"])
            df = float(np.abs(out["download.forces"][start[b]:start[b + 1]] - o["forces"]).max())
            print(f"{kind} {size} chain {b} ({len(s[0])} atoms): |dE| {de:.2e}  max|dF| {df:.2e}")
            if kind == "painn_gen" and not (de <= PAINN_E_TOL and df <= PAINN_F_TOL):
                # tests/test_gpu_painn_widths.py::_check: beyond the bound, twice the oracle's own fp32 deviation
                o32 = oracle_mod.ensemble(blobs, *s, 32, hp=ohp)
                assert de <= max(PAINN_E_TOL, 2 * abs(o32["energy"] - o["energy"])), (b, de)
                assert df <= max(PAINN_F_TOL, 2 * float(np.abs(o32["forces"] - o["forces"]).max())), (b, df)
                continue
            assert de <= PAINN_E_TOL and df <= PAINN_F_TOL, (kind, size, b, de, df)
        return
    e_rel, ea_abs, f_abs = BOUNDS[kind]
    fn = _oracle(kind, golden, oracle_mod)
    for b, s in enumerate(inp.structs):
        E, EA, F = fn(s)
        a = slice(start[b], start[b + 1])
        de, dea, df = abs(out["e"][b] - E), float(np.abs(out["ea"][a] - EA).max()), float(np.abs(out["f"][a] - F).max())
        print(f"{kind} {size} chain {b} ({len(s[0])} atoms): E {E:+.12e}  |dE| {de:.2e}  max|d pe/atom| {dea:.2e}  max|dF| {df:.2e}")
        assert de <= e_rel * max(1.0, abs(E)), (kind, size, b, out["e"][b], E)
        assert dea <= ea_abs and df <= f_abs, (kind, size, b, dea, df)


# ---- the schedules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hc.REDUCED_KINDS + hc.PAINN_KINDS)
def test_reduced_schedule_on_one_engine_repeats_the_fresh_bits(kind, golden):
    eng, sched = _run_schedule(kind, golden)
    eng.close()
    print(f"{kind}: {len(sched)} episodes, {sum(1 for k in _REFS if k[0] == kind)} fresh references")


def _state_errors(eng):
    from surface_sampling_amd import backend

    n = 0
    for call in (eng.stats, eng.neighbors, eng.stress):
        with pytest.raises(backend.BackendError, match=r"vssr error -5: .*run the batch once"):
            call()
        n += 1
    return n


@pytest.mark.parametrize("kind", hc.FULL_KINDS)
def test_full_schedule_on_one_engine_repeats_the_fresh_bits(kind, golden):
    eng, sched = _run_schedule(kind, golden)
    try:
        # the rule of vssr_eval.h after a history: a partial graph (the chain-resident CG leaves one) refuses stats / neighbors / stress
        # until run(), then they are the fresh handle's
        ref, inp = _fresh(kind, "E", "G", golden)
        with hc.Env(VSSR_CG_FUSED="1"):
            eng.relax_cg_f64(inp.structs, fixed=inp.held, rerun=False, driver="resident", **hc.CG)
        assert eng.last_cg_driver == "resident"
        assert _state_errors(eng) == 3
        eng.set_positions(np.vstack([s[1] for s in inp.structs]))
        eng.run(hc.WANT_EF)
        out = dict(ref)
        assert eng.stress()[0].tobytes() == out["stress"].tobytes()
        for name, a in zip(("nbr.i", "nbr.j", "nbr.S", "nbr.r"), eng.neighbors()):
            assert a.tobytes() == out[name].tobytes(), name
        assert list(eng.stats().values()) == out["stats"].tolist()
    finally:
        eng.close()
    # a second life: another engine gives the first episode's cached bits again
    etype, size = sched[0]
    ref, inp = _fresh(kind, etype, size, golden)
    eng = hc.engine(kind, golden)
    try:
        assert hc.first_difference(hc.run_episode(eng, kind, etype, inp), ref, inp) is None
    finally:
        eng.close()
    print(f"{kind}: {len(sched)} episodes, {sum(1 for k in _REFS if k[0] == kind)} fresh references")


@pytest.mark.parametrize("kind", hc.FULL_KINDS)
def test_the_lock_step_cg_of_the_ragged_batch_drops_chains(kind, golden):
    """The Cl episode is there for the live-chain compaction: its chains stop at different polls, so fewer chain evaluations are
    dispatched than lock-step evaluations x chains."""
    inp = hc.inputs(kind, "Cl", "G", golden)
    eng = hc.engine(kind, golden)
    try:
        with hc.Env(VSSR_CG_FUSED="0", VSSR_RELAX_COMPACT="2"):
            res = eng.relax_cg_f64(inp.structs, fixed=inp.held, rerun=False, driver="lockstep", **hc.CG)
        lock, chains = eng.last_relax_counts
        print(f"{kind}: n_eval {res[5].tolist()}, stop {res[6].tolist()}, {lock} lock-step evaluations, {chains} chain evaluations")
        assert eng.last_cg_driver == "lockstep" and len(set(res[5].tolist())) >= 3
        assert chains < lock * len(inp.structs)
    finally:
        eng.close()
