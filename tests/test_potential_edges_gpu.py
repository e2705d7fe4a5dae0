"""The fp64 many-body kernels on the MI355X at their cutoff, clamp and table edges: Tersoff (csrc/tersoff_dev.h), Stillinger-Weber
(sw_dev.h), EAM funcfl / alloy / fs / mixed funcfl (eam_dev.h), ADP (adp_dev.h) and Vashishta (vashishta_dev.h) on the inputs of
tests/edge_cases.py.  What is presumed about those inputs -- which branch every term enters, in which kernel form, and that a kernel
wrong in one of those branches would miss the bounds below by a factor of 1000 or more -- is asserted on the CPU in
tests/test_potential_edges_cpu.py.

References: the C oracle for Tersoff, the numpy restatements for the others (eam_oracle, eam_alloy_oracle, adp_oracle, sw_oracle,
vashishta_oracle).  Bounds: those of the existing device test of the same kernel (edge_cases.*_TOL, with the pointers there); for
Tersoff, EAM and ADP scaled by max(1, max|F|) and max(1, max|pe/atom|) as tests/test_gpu_parity.py scales the Tersoff ones, for SW
and Vashishta unscaled.  Stress: ten times the uncertainty of the strain derivative of the reference energy (tests/strain_fd.py).
Every figure is printed before it is asserted; every value must be finite.
"""
import numpy as np
import pytest

import adp_oracle
import eam_alloy_oracle as ao
import eam_oracle
import edge_cases as ec
import strain_fd as sf
import sw_oracle
import tersoff_census as tc
import vashishta_oracle as vo

pytestmark = pytest.mark.gpu

STRESS_FACTOR = 10.0


def _parity(tag, got, structs, ref, tol, scaled):
    """Energy, pe/atom and forces of a batch against ``ref(structure) -> (E, pe/atom, F)``, chain by chain."""
    e, ea, f = got
    assert np.isfinite(e).all() and np.isfinite(ea).all() and np.isfinite(f).all(), tag
    o, bad = 0, []
    for b, s in enumerate(structs):
        n = len(s[0])
        E, EA, F = ref(s)
        assert np.isfinite(E) and np.isfinite(EA).all() and np.isfinite(F).all(), (tag, b)
        se, sa, sF = max(1.0, abs(E)), (max(1.0, np.abs(EA).max()) if scaled else 1.0), (max(1.0, np.abs(F).max()) if scaled else 1.0)
        de, da, df = abs(e[b] - E), np.abs(ea[o:o + n] - EA).max(), np.abs(f[o:o + n] - F).max()
        print(f"{tag} chain {b} ({n} atoms): E {E:+.12e} |dE| {de:.2e} (bound {tol['E'] * se:.2e})  max|d pe/atom| {da:.2e} "
              f"({tol['EA'] * sa:.2e})  max|dF| {df:.2e} ({tol['F'] * sF:.2e})  max|F| {np.abs(F).max():.3e}")
        if not (de <= tol["E"] * se and da <= tol["EA"] * sa and df <= tol["F"] * sF):
            bad.append((b, de, da, df))
        o += n
    assert not bad, (tag, bad)


def _alone_equals_batch(tag, eng, structs, got):
    e, ea, f = got
    o = 0
    for b, s in enumerate(structs):
        n = len(s[0])
        e1, ea1, f1 = eng.evaluate_f64([s])
        assert e1[0] == e[b] and np.array_equal(ea1, ea[o:o + n]) and np.array_equal(f1, f[o:o + n]), (tag, b)
        o += n


def _device_rows(eng, structs):
    """Slots of every atom's row in the batch the engine holds (the device neighbour list)."""
    ei = eng.neighbors()[0]
    return np.bincount(ei, minlength=sum(len(s[0]) for s in structs))


def _stress(tag, eng, structs, energy_of):
    """``eng`` holds an evaluation of ``structs``; the virial of every chain against the strain derivative of ``energy_of``."""
    st = eng.stress()[0]
    assert np.isfinite(st).all()
    for b, (T, X, Cl, pbc) in enumerate(structs):
        chk = sf.fd_stress(lambda x, c: energy_of((T, x, c, pbc)), X, Cl)
        dev = st[b] * chk.volume
        ratio = np.abs(dev - chk.virial) / chk.unc
        print(f"{tag} chain {b} virial: device {dev}  checker {chk.virial}  unc {chk.unc}  max ratio {ratio.max():.3f}")
        assert (np.abs(dev - chk.virial) <= STRESS_FACTOR * chk.unc).all(), (tag, b, dev, chk.virial, chk.unc)
        assert np.abs(chk.virial).max() > 1000 * chk.unc.max()           # the virial is resolved


# ---- EAM / ADP -----------------------------------------------------------------------------------------------------------------------
EAM_NAMES = ("Cu funcfl", "alloy", "fs", "funcfl", "adp")


@pytest.fixture(scope="module")
def eam_sets():
    """{name: (what the engine takes, tables for the host density, reference, typed?)} for the full tables and the edge tables."""
    cu, _ = ec.funcfl_pair()
    forms = ec.typed_forms()

    def entry(name, edge):
        if name == "Cu funcfl":
            f = ec.edge_funcfl(cu) if edge else cu
            return f, ec.as_tables(f), (lambda s: eam_oracle.eam(f, *s[1:])), False
        t = ec.edge_tables(forms[name]) if edge else forms[name]
        if name == "adp":
            return t, t, (lambda s: adp_oracle.adp(t, *s)), True
        return t, t, (lambda s: ao.eam_typed(t, *s)), True

    return {name: {"full": entry(name, False), "edge": entry(name, True)} for name in EAM_NAMES}


def _lone(t):
    return np.array([t], np.int32), np.array([[1.0, 2.0, 3.0]]), np.diag([9.0, 10.0, 11.0]), np.array([1, 1, 0], np.uint8)


@pytest.mark.parametrize("name", EAM_NAMES)
def test_eam_beyond_the_f_table_at_rho_zero_and_in_the_cutoff_places(eam_sets, name):
    """Compressed slab and fragment (rho beyond the F table for the core, inside it for the surface), an isolated atom in the batch;
    then, on the tables cut short, the dimers one ulp inside / on / one ulp outside the cutoff, in the last table interval and
    between the table end and the cutoff, and eight isolated atoms.  Batch independence and the virial of the compressed slab."""
    from surface_sampling_amd import backend

    arg, tab, ref, typed = eam_sets[name]["full"]
    seed = 3 if typed else None
    structs = [ec.compressed_slab(types_seed=seed), _lone(1 if typed else 0), ec.fcc_fragment(types_seed=seed)]
    eng = backend.EAMEngine(arg, device=0)
    got = eng.evaluate_f64(structs)
    for b in (0, 2):
        rho, rhomax = ec.eam_rho(tab, *structs[b])
        assert (rho > rhomax).sum() >= ec.MIN_TERMS and (rho < rhomax).sum() >= ec.MIN_TERMS
    _parity(name, got, structs, ref, ec.EAM_TOL, scaled=True)
    _alone_equals_batch(name, eng, structs, got)
    eng.evaluate_f64(structs[:1])
    _stress(name, eng, structs[:1], lambda s: ref(s)[0])
    eng.close()

    arg, tab, ref, typed = eam_sets[name]["edge"]
    chain, where = ec.eam_edge_chain(tab, (0, 1) if typed else (0, 0))
    structs = [chain, _lone(0)]
    eng = backend.EAMEngine(arg, device=0)
    got = eng.evaluate_f64(structs)
    _parity(name + " edge tables", got, structs, ref, ec.EAM_TOL, scaled=True)
    f = got[2]
    for i, j in where["at"] + where["outside"]:
        assert not f[i].any() and not f[j].any()                         # d >= cutoff: no interaction at all
    for i, j in where["inside"]:
        assert abs(f[i][0]) > 1e-3                                       # one ulp inside: the full (non-zero) edge value
    _alone_equals_batch(name + " edge tables", eng, structs, got)
    eng.close()


def _cg(eng, structs, driver, max_iter):
    e, ea, f, pos, it, ev, why = eng.relax_cg_f64(structs, max_iter=max_iter, rerun=False, driver=driver)
    return {"e": e, "ea": ea, "f": f, "pos": pos, "it": it, "ev": ev, "why": why, "driver": eng.last_cg_driver}


@pytest.mark.parametrize("name", EAM_NAMES)
def test_cg_expands_a_compressed_fragment_across_the_end_of_the_f_table(eam_sets, name):
    """Free fcc fragments (pbc = 0) at a = 2.3 and 2.2 A: the core starts beyond the F table (the linear continuation and its F'
    drive the first steps), the fragment expands, and every atom ends inside the table -- the trajectory evaluates F on both sides of
    the table end.  EAM: the chain-resident minimiser gives the bits of the lock-step driver; ADP: lock step only.  The energy the
    minimiser leaves is that of a fresh evaluation of its positions and of the restatement."""
    from surface_sampling_amd import backend

    arg, tab, ref, typed = eam_sets[name]["full"]
    seed = 3 if typed else None
    structs = [ec.fcc_fragment(a, types_seed=seed) for a in (ec.FRAGMENT_A, 2.2)]
    eng = backend.EAMEngine(arg, device=0)
    lock = _cg(eng, structs, "lockstep", 25)
    assert lock["driver"] == "lockstep"
    if name != "adp":
        res = _cg(eng, structs, "resident", 25)
        assert res["driver"] == "resident"
        for k in ("e", "ea", "f", "pos", "it", "ev", "why"):
            assert np.array_equal(res[k], lock[k]), (name, k)
    o = 0
    final = []
    for b, (T, X, Cl, pbc) in enumerate(structs):
        n = len(T)
        rho0, rhomax = ec.eam_rho(tab, T, X, Cl, pbc)
        rho1, _ = ec.eam_rho(tab, T, lock["pos"][o:o + n], Cl, pbc)
        print(f"{name} fragment {b}: {lock['it'][b]} iterations, {lock['ev'][b]} evaluations, stop {lock['why'][b]}; rho max {rho0.max():.4f} -> "
              f"{rho1.max():.4f}, table end {rhomax:.4f}; atoms beyond it {(rho0 > rhomax).sum()} -> {(rho1 > rhomax).sum()}")
        assert (rho0 > rhomax).sum() >= ec.MIN_TERMS and (rho0 < rhomax).sum() >= ec.MIN_TERMS and (rho1 < rhomax).all()
        final.append((T, lock["pos"][o:o + n].copy(), Cl, pbc))
        o += n
    _parity(name + " after CG", (lock["e"], lock["ea"], lock["f"]), final, ref, ec.EAM_TOL, scaled=True)
    fresh = eng.evaluate_f64(final)
    _parity(name + " fresh evaluation", fresh, final, ref, ec.EAM_TOL, scaled=True)
    print(f"{name}: |E left by the minimiser - E of a fresh evaluation| {np.abs(fresh[0] - lock['e']).max():.2e}")
    for k, x in zip(("e", "ea", "f"), fresh):
        assert np.array_equal(x, lock[k]), (name, k)                     # the same kernels on the same positions: the same bits
    eng.close()


# ---- Tersoff -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tersoff_engine():
    from surface_sampling_amd import backend

    eng = backend.TersoffEngine(ec.tersoff_edge_table(), device=0)
    yield eng
    eng.close()


def test_tersoff_clamps_and_shell_ends_in_both_kernel_forms(tersoff_engine, oracle_mod):
    """The eight edge chains in one batch: both exp clamps through m = 1 and m = 3 with beta = 1e-30 (the value 1e30 and dex = 0 enter
    E and F), pairs one ulp inside / on / one ulp outside R - D and R + D as j and as k, at centres whose rows take the 16-slot tile
    (chains 0, 1) and at centres whose rows take the long form (chains 2 .. 7)."""
    P, chains = ec.tersoff_edge_chains()
    structs = [s for s, _ in chains]
    got = tersoff_engine.evaluate_f64(structs)
    rows = _device_rows(tersoff_engine, structs)
    o = 0
    for b, (s, centres) in enumerate(chains):
        deg = rows[o:o + len(s[0])]
        print(f"tersoff chain {b}: rows of the cluster centres {deg[centres]}, longest other row {np.delete(deg, centres).max()}")
        assert ((deg[centres] > tc.TILE_SLOTS).all() if b >= 2 else (deg <= tc.TILE_SLOTS).all()), b
        o += len(s[0])
    _parity("tersoff", got, structs, lambda s: oracle_mod.tersoff(P, *s), ec.TERSOFF_TOL, scaled=True)
    _alone_equals_batch("tersoff", tersoff_engine, structs, got)


def test_tersoff_stress_of_a_clamp_state(tersoff_engine, oracle_mod):
    """A periodic box with terms in both clamps whose strained copies (every one the strain derivative evaluates) keep every term in its
    branch -- asserted with the census -- so that the energy is smooth where it is differentiated."""
    P = ec.tersoff_edge_table()
    s = ec.tersoff_clamp_box()
    t0 = tc.census(P, *s)[2]
    t0.pop(("all", "margin", "ex"))
    assert t0["tile", "ex", "high"] > 0 and t0["tile", "ex", "low"] > 0 and t0["tile", "bij_after_high", "n=1"] > 0
    for c in ec.strained_copies(s):
        t = tc.census(P, *c)[2]
        t.pop(("all", "margin", "ex"))
        assert t == t0
    got = tersoff_engine.evaluate_f64([s])
    _parity("tersoff clamp box", got, [s], lambda x: oracle_mod.tersoff(P, *x), ec.TERSOFF_TOL, scaled=True)
    _stress("tersoff clamp box", tersoff_engine, [s], lambda x: oracle_mod.tersoff(P, *x, want_forces=False)[0])


def test_tersoff_cg_on_the_clamp_table_resident_equals_lock_step(tersoff_engine, oracle_mod):
    P, chains = ec.tersoff_edge_chains()
    structs = [ec.tersoff_clamp_box(), chains[0][0]]
    lock = _cg(tersoff_engine, structs, "lockstep", 10)
    res = _cg(tersoff_engine, structs, "resident", 10)
    assert (lock["driver"], res["driver"]) == ("lockstep", "resident")
    for k in ("e", "ea", "f", "pos", "it", "ev", "why"):
        assert np.array_equal(res[k], lock[k]), k
    print(f"tersoff CG: iterations {lock['it']}, evaluations {lock['ev']}, stop {lock['why']}, E {lock['e']}")
    assert np.isfinite(lock["pos"]).all() and (lock["it"] >= 1).all()
    o, final = 0, []
    for T, X, Cl, pbc in structs:
        final.append((T, lock["pos"][o:o + len(T)].copy(), Cl, pbc))
        o += len(T)
    _parity("tersoff after CG", (lock["e"], lock["ea"], lock["f"]), final, lambda s: oracle_mod.tersoff(P, *s), ec.TERSOFF_TOL, scaled=True)


# ---- Stillinger-Weber ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Si", "three species"])
def test_sw_cutoff_places_and_underflowed_factors_in_both_kernel_forms(name):
    """Pairs one ulp inside a sigma (exp(sigma / (r - a sigma)) = 0 and d ln f / dr ~ -1e31: 0 x dlf must stay 0), on it, one ulp
    outside (three-species set: inside the row, the kernel skips it), and where exp(gamma sigma x) has underflowed while exp(sigma x)
    has not; at tile centres (chains 0, 1) and long-row centres (chains 2 .. 5)."""
    from surface_sampling_amd import backend

    P = ec.sw_set(name)
    chains = ec.sw_edge_chains(P, ec.SW_SETS[name], ec.SW_SEED)
    structs = [s for s, _ in chains]
    eng = backend.SWEngine(P, device=0)
    got = eng.evaluate_f64(structs)
    rows = _device_rows(eng, structs)
    o = 0
    for b, (s, centres) in enumerate(chains):
        deg = rows[o:o + len(s[0])]
        print(f"sw {name} chain {b}: rows of the cluster centres {deg[centres]}")
        assert ((deg[centres] > 16).all() if b >= 2 else (deg <= 16).all()), b
        o += len(s[0])
    _parity("sw " + name, got, structs, lambda s: sw_oracle.sw(P, *s), ec.SW_TOL, scaled=False)
    _alone_equals_batch("sw " + name, eng, structs, got)
    eng.close()


# ---- Vashishta -----------------------------------------------------------------------------------------------------------------------
def test_vashishta_r0_and_rc_places_with_16_and_17_short_slots():
    """Built-in SiC: centres with exactly 16 short slots (the LDS tile) and with 17 (the long form), one of them one ulp inside r0
    (f = exp(gamma / (r - r0)) = 0), a neighbour one ulp beyond r0, and neighbours one ulp on either side of rc."""
    from surface_sampling_amd import backend

    _, P = vo.sic_params()
    chains = ec.vashishta_edge_chains(P)
    structs = [s for s, _ in chains]
    eng = backend.VashishtaEngine(P, device=0)
    got = eng.evaluate_f64(structs)
    _parity("vashishta", got, structs, lambda s: vo.vashishta(P, *s), ec.VASHISHTA_TOL, scaled=False)
    _alone_equals_batch("vashishta", eng, structs, got)
    eng.close()
