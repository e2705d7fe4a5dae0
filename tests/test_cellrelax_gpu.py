"""Device variable-cell relaxation (vssr_batch_relax_cell: csrc/relax_cell.hip) against the numpy restatement tests/cellrelax_oracle.py
driven by the device's own single-point evaluation and stress, the known answers on the device, and the invariants of the call.  Every
cell has 8 to 32 atoms (tests/cellrelax_cases.py; the lj/cut ones are rehearsed on the CPU by tests/test_cellrelax_cpu.py).

Bounds of the step-for-step comparison.  fp64 kinds: the larger of the 1e-7 A that tests/relax_cases.py uses for the lock-step FIRE of
the fp64 kinds (BOUND_FLOOR) and ten times the oracle's own spread, measured in the test as the difference between two runs of the
oracle whose atoms (and so every sum over atoms, on the device and in numpy) are taken in another order.  PaiNN: the 2e-3 A over 8
steps of tests/test_relax.py's fixed-cell FIRE comparison, scaled to the steps compared here."""

import numpy as np
import pytest

import cellrelax_cases as cs
import cellrelax_oracle as co
import pair_cases as pc
import relax_cases as rcs
import strain_fd as sf
import sw_oracle as so

pytestmark = pytest.mark.gpu

WANT = 1 | 2 | 16   # energy, forces, per-atom energies
KEYS = ("positions", "cells", "n_steps", "stop_reason", "fmax", "energy", "volume", "e", "ea", "f", "stress")


def _relax(eng, structs, fixed=None, upload=True, **kw):
    if upload:
        eng.upload(structs)
    out = eng.relax_cell(fixed=fixed, want=WANT, **kw)
    out["counts"], out["regrows"] = eng.last_relax_counts, eng.debug_capacity()
    out["e"], out["ea"], out["f"] = eng.results_f64()          # at once, from what the call left on the device
    out["stress"] = eng.stress()[0]
    return out


def _device_eval(eng, structs):
    """The device's own single-point evaluation and stress as the oracle's callback: the potential's tolerance does not enter."""
    def fn(b, x, C):
        e, _, f = eng.evaluate_f64([(structs[b][0], x, C, structs[b][3])])
        return e[0], f, eng.stress()[0][0]
    return fn


def _start(structs):
    return np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])]).astype(np.int64)


def _assert_equal(a, b, tag, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def _lj_engine(terms=cs.LJ):
    from surface_sampling_amd import backend

    return backend.PairEngine(terms, n_types=1, device=0)


def _fresh(eng, structs, r):
    """(e, ea, f) of a fresh upload of the relaxed positions and cells."""
    st = _start(structs)
    return eng.evaluate_f64([(s[0], r["positions"][st[b]:st[b + 1]], r["cells"][b], s[3]) for b, s in enumerate(structs)])


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def _parity(eng, fn, structs, held, cutoff, kw):
    """(device result, oracle result, spread of the oracle under a permutation of the atoms)."""
    dev = _relax(eng, structs, held, **kw)
    ora = co.run(fn(structs), structs, fixed=held, cutoff=cutoff, **kw)
    st = _start(structs)
    perm = [cs.permuted(s, 70 + b) for b, s in enumerate(structs)]
    structs_p = [p[0] for p in perm]
    held_p = None if held is None else np.concatenate([held[st[b]:st[b + 1]][p[1]] for b, p in enumerate(perm)])
    ora_p = co.run(fn(structs_p), structs_p, fixed=held_p, cutoff=cutoff, **kw)
    spread = 0.0
    for b, (_, p) in enumerate(perm):
        back = np.empty_like(ora_p["positions"][st[b]:st[b + 1]])
        back[p] = ora_p["positions"][st[b]:st[b + 1]]
        spread = max(spread, float(np.abs(back - ora["positions"][st[b]:st[b + 1]]).max()), float(np.abs(ora_p["cells"][b] - ora["cells"][b]).max()))
    assert np.array_equal(ora_p["n_steps"], ora["n_steps"]) and np.array_equal(ora_p["stop_reason"], ora["stop_reason"])
    return dev, ora, spread


@pytest.mark.parametrize("kind", cs.PARITY_KINDS)
def test_step_for_step_parity_with_the_oracle(kind, golden):
    eng = cs.parity_engine(kind, golden)
    structs = cs.parity_structs(kind)
    assert [len(s[0]) for s in structs] == list(cs.PARITY_SIZES)
    held = pc.held_mask(structs)
    x0, c0 = np.vstack([s[1] for s in structs]), np.array([s[2] for s in structs])
    dev, ora, spread = _parity(eng, lambda ss: _device_eval(eng, ss), structs, held, cs.parity_cutoff(kind, golden), cs.PARITY)
    bound = max(rcs.BOUND_FLOOR, 10.0 * spread)
    dx, dc = float(np.abs(dev["positions"] - ora["positions"]).max()), float(np.abs(dev["cells"] - ora["cells"]).max())
    print(f"{kind}: max |device - oracle| positions {dx:.3e} A, cells {dc:.3e} A; oracle spread under permutation {spread:.3e} A; bound {bound:.3e} A; "
          f"moved positions {np.abs(dev['positions'] - x0).max():.3e} A, cells {np.abs(dev['cells'] - c0).max():.3e} A")
    assert np.array_equal(dev["n_steps"], ora["n_steps"]) and np.array_equal(dev["stop_reason"], ora["stop_reason"])
    assert list(dev["n_steps"]) == [cs.PARITY["max_steps"]] * 3 and list(dev["stop_reason"]) == [2] * 3
    assert dx <= bound and dc <= bound
    assert np.abs(dev["positions"] - x0).max() > 1e-3 and np.abs(dev["cells"] - c0).max() > 1e-4      # atoms and cells did move
    for k, key in enumerate(("fmax", "energy", "volume")):
        scale = np.maximum(np.abs(ora["result"][:, k]), 1.0)
        assert (np.abs(dev[key] - ora["result"][:, k]) <= 1e-6 * scale).all(), key
    # the batch is left with a complete evaluation of the final cells and positions
    e, ea, f = _fresh(eng, structs, dev)
    assert np.array_equal(e, dev["e"]) and np.array_equal(f, dev["f"]) and np.array_equal(eng.stress()[0], dev["stress"])
    eng.close()


def test_painn_follows_the_oracle_on_its_own_forces(golden):
    """20 atoms of sheared, rattled SrTiO3, three chains (two of them rattled further), 6 steps with fp32 forces; the oracle is fed the
    energy (fp64 ensemble mean), forces (fp32, widened) and mean stress the device returns for the same structure."""
    from surface_sampling_amd import backend

    Z, X, C, pbc = cs.painn_struct()
    structs = [(Z, X + np.random.default_rng(40 + k).normal(0, 0.02 * k, X.shape), C, pbc) for k in range(3)]
    held = pc.held_mask(structs)
    eng = backend.PainnEngine(golden.blobs, device=0)

    def fn(ss):
        def one(b, x, Cc):
            r = eng.evaluate([(ss[b][0], x, Cc, ss[b][3])])
            return r["energy_f64"][0], r["forces"].astype(np.float64), eng.stress()[0][0]
        return one

    kw = dict(max_steps=6, fmax=1e-4)
    eng.upload(structs)
    dev = eng.relax_cell(fixed=held, **kw)
    res, stress = eng.download(), eng.stress()[0]
    ora = co.run(fn(structs), structs, fixed=held, cutoff=5.0, **kw)
    bound = 2e-3 * kw["max_steps"] / 8.0
    dx, dc = float(np.abs(dev["positions"] - ora["positions"]).max()), float(np.abs(dev["cells"] - ora["cells"]).max())
    print(f"PaiNN: max |device - oracle| positions {dx:.3e} A, cells {dc:.3e} A (bound {bound:.3e} A); cells moved by {np.abs(dev['cells'] - C).max():.3e} A")
    assert list(dev["n_steps"]) == [6] * 3 and list(dev["stop_reason"]) == [2] * 3 and np.array_equal(ora["n_steps"], dev["n_steps"])
    assert dx <= bound and dc <= bound and np.abs(dev["cells"] - C).max() > 1e-4
    st = _start(structs)
    again = eng.evaluate([(Z, dev["positions"][st[b]:st[b + 1]], dev["cells"][b], pbc) for b in range(3)])
    assert np.array_equal(again["forces"], res["forces"]) and np.array_equal(eng.stress()[0], stress)
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_sw_silicon_lattice_constant_on_the_device():
    """SW diamond Si, 8 atoms, from a = 5.60 A under hydrostatic_strain: the project's published 5.430950 A / -4.3366 eV per atom."""
    from surface_sampling_amd import backend

    eng = backend.SWEngine(so.si_params(), device=0)
    T, X, Cl = so.diamond_si(5.60)
    r = _relax(eng, [(T, X, Cl, np.ones(3, np.uint8))], max_steps=400, fmax=1e-6, hydrostatic_strain=True)
    a = r["cells"][0][0, 0]
    print(f"{r['n_steps'][0]} steps, reason {r['stop_reason'][0]}: a = {a:.7f} A, E / atom = {r['energy'][0] / 8:.6f} eV, |sigma| {np.abs(r['stress']).max():.2e} eV / A^3")
    assert r["stop_reason"][0] == 1 and r["fmax"][0] < 1e-6
    assert abs(a - 5.430950) < 5e-7 and abs(r["energy"][0] / 8 + 4.3366) < 5e-5 and r["energy"][0] == r["e"][0]
    assert np.array_equal(np.diag(np.diag(r["cells"][0])), r["cells"][0]) and r["cells"][0][1, 1] == a and r["cells"][0][2, 2] == a
    eng.close()


def test_scalar_pressure_leaves_minus_p_as_stress():
    eng = _lj_engine()
    s, p = cs.pressure_case()
    fmax = 1e-3
    r = _relax(eng, [s], max_steps=400, fmax=fmax, scalar_pressure=p)
    Ft = np.linalg.inv(s[2]) @ r["cells"][0]                       # C = C0 F^T
    bound = fmax * len(s[0]) * np.linalg.norm(Ft, 2) / r["volume"][0]       # rows of sigma + p I = -(W F^T) / V, |W row| < fmax c
    sig = sf.voigt_to_tensor(r["stress"][0])
    print(f"pressure {p}: {r['n_steps'][0]} steps, sigma {r['stress'][0]}, |sigma + p I| {np.abs(sig + p * np.eye(3)).max():.3e} (bound {bound:.3e})")
    assert r["stop_reason"][0] == 1 and np.abs(sig + p * np.eye(3)).max() <= bound
    assert r["volume"][0] < abs(np.linalg.det(s[2])) and abs(r["volume"][0] - abs(np.linalg.det(r["cells"][0]))) < 1e-9
    eng.close()


def test_slab_with_the_in_plane_mask_keeps_its_vacuum_axis():
    """p p f with mask (1, 1, 0, 0, 0, 1): the c vector and the z components of a and b do not change by a bit, and the z coordinate of
    an atom is its reference coordinate s_z bit for bit (x = s F^T with the third row and column of F those of I): the held bottom
    layer, whose s never moves, keeps its z exactly while it rides the in-plane strain."""
    eng = _lj_engine()
    s = cs.slab()
    held = (np.arange(24) < 8).astype(np.uint8)
    r = _relax(eng, [s], held, max_steps=300, fmax=1e-3, mask=cs.SLAB_MASK)
    C = r["cells"][0]
    print(f"slab: {r['n_steps'][0]} steps, reason {r['stop_reason'][0]}, in-plane lattice constant {C[0, 0] / 2:.5f}, {C[1, 1] / 2:.5f} A")
    assert r["stop_reason"][0] == 1 and np.array_equal(C[2], s[2][2]) and not C[:2, 2].any()
    assert abs(C[0, 0] / 2 - cs.LJ_A0) < 0.05 and abs(C[0, 0] - s[2][0, 0]) > 0.1
    assert np.array_equal(r["positions"][:8, 2], s[1][:8, 2])
    frac0, frac1 = s[1][:8] @ np.linalg.inv(s[2]), r["positions"][:8] @ np.linalg.inv(C)
    assert np.abs(frac1 - frac0).max() < 1e-13 and np.abs(r["positions"][:8, :2] - s[1][:8, :2]).max() > 1e-2
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_fixed_atoms_bits_repeat_and_a_chain_does_not_depend_on_its_batch():
    eng = _lj_engine()
    structs = cs.mixed_batch()
    held = pc.held_mask(structs)
    kw = dict(max_steps=10, fmax=1e-4)
    a = _relax(eng, structs, held, **kw)
    b = _relax(eng, structs, held, **kw)
    _assert_equal(a, b, "the same call twice")
    assert list(a["n_steps"]) == [10] * 3 and list(a["stop_reason"]) == [2] * 3
    st = _start(structs)
    for k, s in enumerate(structs):
        # a fixed atom keeps its fractional coordinates (to the rounding of x = s F^T and of the inverse) while its cell changes
        f0, f1 = s[1][:2] @ np.linalg.inv(s[2]), a["positions"][st[k]:st[k] + 2] @ np.linalg.inv(a["cells"][k])
        assert np.abs(f1 - f0).max() < 1e-13 and np.abs(a["cells"][k] - s[2]).max() > 1e-3
        alone = _relax(eng, [s], held[st[k]:st[k + 1]], **kw)
        for key in ("positions", "f", "ea"):
            assert np.array_equal(alone[key], a[key][st[k]:st[k + 1]]), (k, key)
        for key in ("cells", "n_steps", "stop_reason", "fmax", "energy", "volume", "e", "stress"):
            assert np.array_equal(alone[key][0], a[key][k]), (k, key)
    # the resident cells after the call; a later set_positions / run uses them
    assert np.array_equal(eng.get_cell(), alone["cells"])
    eng.set_positions(alone["positions"])
    eng.run(WANT)
    e, _, f = eng.results_f64()
    assert np.array_equal(e, alone["e"]) and np.array_equal(f, alone["f"])
    eng.close()


def test_capacity_regrow_under_compression():
    """The 32-atom cube at a = 4.20 A under 60 slots per atom: the fifth neighbor shell enters on the way to the minimum, an evaluation
    overflows, the run regrows and ends with the bits of the roomy run."""
    s = cs.compressing_cube()
    kw = dict(max_steps=60, fmax=1e-3)
    roomy_eng = _lj_engine()
    roomy_eng.debug_capacity(slots_per_atom=cs.ROOMY_SLOTS)      # (the default of 64 slots per atom is below the 80 of the end as well)
    roomy = _relax(roomy_eng, [s, s], **kw)
    roomy_eng.close()
    tight_eng = _lj_engine()
    tight_eng.debug_capacity(slots_per_atom=cs.COMPRESS_SLOTS, tight=1)
    tight = _relax(tight_eng, [s, s], **kw)
    tight_eng.close()
    print(f"roomy counts {roomy['counts']} regrows {roomy['regrows']}; tight counts {tight['counts']} regrows {tight['regrows']}; "
          f"steps {roomy['n_steps']}, reasons {roomy['stop_reason']}")
    assert roomy["regrows"] == 0 and tight["regrows"] >= 1 and tight["counts"][0] > roomy["counts"][0]
    _assert_equal(tight, roomy, "tight against roomy")
    assert list(roomy["stop_reason"]) == [1, 1] and abs(roomy["cells"][0][0, 0] / 2 - cs.LJ_A0) < 0.01


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_thin_cell_under_pressure_stops_where_its_step_opened():
    eng = _lj_engine(cs.LJ_THIN)
    thin, other, p = cs.thin_case()
    kw = dict(max_steps=cs.THIN_STEPS, fmax=1e-3, scalar_pressure=p)
    alone = _relax(eng, [other], **kw)
    structs = [thin, other]
    r = _relax(eng, structs, **kw)
    rec = []
    ora = co.run(_device_eval(eng, structs), structs, cutoff=7.9, record=rec, **kw)
    print(f"thin: steps {r['n_steps']}, reasons {r['stop_reason']}, lock-step evaluations {r['counts'][0]}, thin cell lengths {np.linalg.norm(r['cells'][0], axis=1)}")
    assert list(r["stop_reason"]) == [4, 2] and list(r["n_steps"]) == [3, cs.THIN_STEPS]
    assert np.array_equal(ora["stop_reason"], r["stop_reason"]) and np.array_equal(ora["n_steps"], r["n_steps"])
    # the cell is that of the opening of the step that was not taken: the state of the oracle's last test
    assert np.abs(r["cells"][0] - rec[0][-1]["cell"]).max() <= rcs.BOUND_FLOOR and np.abs(r["positions"][:8] - rec[0][-1]["positions"]).max() <= rcs.BOUND_FLOOR
    assert np.array_equal(co.image_counts(r["cells"][0], thin[3], 7.9), co.image_counts(thin[2], thin[3], 7.9))
    # the batch is complete ...
    e, ea, f = _fresh(eng, structs, r)
    assert np.array_equal(e, r["e"]) and np.array_equal(f, r["f"]) and np.isfinite(r["stress"]).all()
    # ... and the neighbour has the bits it has alone
    for key in ("positions", "f", "ea"):
        assert np.array_equal(r[key][8:], alone[key]), key
    for key in ("cells", "n_steps", "stop_reason", "fmax", "energy", "volume", "e", "stress"):
        assert np.array_equal(r[key][1], alone[key][0]), key
    eng.close()


def test_a_non_finite_evaluation_sends_the_chain_back_to_where_its_step_opened():
    """The wall case: the fourth step carries a held pair inside the overflowing 0 - 1 term; the chain goes back to the state its
    fourth step opened at (the oracle's last complete test), counts three steps, stops with reason 3; the batch is complete and
    finite, and the neighbour has the bits it has alone."""
    from surface_sampling_amd import backend

    wall, held_w, terms, rc = cs.wall_case()
    other = (np.ones(8, np.int32),) + cs.thin_case()[1][1:]
    eng = backend.PairEngine(terms, n_types=2, device=0)
    kw = dict(max_steps=cs.WALL_STEPS, fmax=1e-3)
    alone = _relax(eng, [other], **kw)
    structs, held = [wall, other], np.concatenate([held_w, np.zeros(8, np.uint8)])
    r = _relax(eng, structs, held, **kw)
    rec = []
    ora = co.run(_device_eval(eng, structs), structs, fixed=held, cutoff=rc, record=rec, **kw)
    print(f"wall: steps {r['n_steps']}, reasons {r['stop_reason']}, lock-step evaluations {r['counts'][0]}")
    assert list(r["stop_reason"]) == [3, 2] and list(r["n_steps"]) == [3, cs.WALL_STEPS]
    assert np.array_equal(ora["stop_reason"], r["stop_reason"]) and np.array_equal(ora["n_steps"], r["n_steps"])
    assert np.abs(r["cells"][0] - rec[0][-1]["cell"]).max() <= rcs.BOUND_FLOOR and np.abs(r["positions"][:9] - rec[0][-1]["positions"]).max() <= rcs.BOUND_FLOOR
    assert abs(r["fmax"][0] - rec[0][-1]["fmax"]) <= 1e-6 * rec[0][-1]["fmax"]          # the record of the last complete test
    e, ea, f = _fresh(eng, structs, r)
    assert np.isfinite(r["e"]).all() and np.isfinite(r["f"]).all() and np.array_equal(e, r["e"]) and np.array_equal(f, r["f"])
    for key in ("positions", "f", "ea"):
        assert np.array_equal(r[key][9:], alone[key]), key
    for key in ("cells", "n_steps", "stop_reason", "fmax", "energy", "volume", "e", "stress"):
        assert np.array_equal(r[key][1], alone[key][0]), key
    eng.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_kspace_handle_is_refused():
    import ewald_cases as ec
    from surface_sampling_amd import backend, pair

    eng = backend.PairEngine(pair.parse(ec.RAGGED_MODEL, 3), device=0)
    s = ec.rattled_cube()
    e0 = eng.evaluate_f64([s])[0]
    eng.upload([s])
    with pytest.raises(backend.BackendError, match=r"vssr error -5: .*ew_stride"):
        eng.relax_cell(max_steps=3)
    assert np.array_equal(eng.get_cell()[0], s[2]) and np.array_equal(eng.evaluate_f64([s])[0], e0)
    eng.close()


def test_refusals_leave_the_handle_usable():
    from surface_sampling_amd import backend

    eng = _lj_engine()
    structs = cs.mixed_batch()[:2]
    good = dict(max_steps=4, fmax=1e-4)
    ref = _relax(eng, structs, **good)
    fields = [n for n, _ in backend.CellRelaxParams._fields_]

    def params(**over):
        p = backend.CellRelaxParams.default(**good)
        for k, v in over.items():
            assert k in fields
            setattr(p, k, v)
        return p

    nan, inf = float("nan"), float("inf")
    bad = [(dict(max_steps=-1), "max_steps"), (dict(nmin=-1), "nmin"), (dict(finc=0.9), "finc"), (dict(fdec=0.0), "fdec"), (dict(fdec=1.0), "fdec"),
           (dict(fa=0.0), "fa"), (dict(fa=1.0), "fa"), (dict(astart=0.0), "astart"), (dict(astart=1.5), "astart"),
           (dict(scalar_pressure=nan), "scalar_pressure"), (dict(scalar_pressure=inf), "scalar_pressure"), (dict(cell_factor=nan), "cell_factor"),
           (dict(mask=(backend.C.c_int32 * 6)(1, 1, 1, 1, 1, 2)), "mask"), (dict(mask=(backend.C.c_int32 * 6)(-1, 1, 1, 1, 1, 1)), "mask")]
    for name in ("fmax", "dt", "maxstep", "dtmax"):
        bad += [({name: v}, name) for v in (0.0, -1.0, nan, inf)]
    for over, msg in bad:
        eng.upload(structs)
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*" + msg):
            eng.relax_cell(params=params(**over))
        assert np.array_equal(eng.get_cell(), np.array([s[2] for s in structs]))          # nothing moved
        _assert_equal(_relax(eng, structs, upload=False, **good), ref, msg)
    lib, h = eng._lib, eng._h
    eng.upload(structs)
    assert lib.vssr_batch_relax_cell(h, None, None, WANT, None, None, None, None, None) == -1 and b"parameters" in lib.vssr_last_error(h)
    _assert_equal(_relax(eng, structs, upload=False, **good), ref, "after the null refusal")
    # open axes: the default mask frees zz; a sheared vacuum vector; an in-plane vector with a z component
    T, X, C, pbc = cs.slab()
    sheared, tilted = C.copy(), C.copy()
    sheared[2, 0] = 0.5
    tilted[0, 2] = 0.1
    for struct, mask, msg in (((T, X, C, pbc), None, "mask"), ((T, X, sheared, pbc), cs.SLAB_MASK, "Cartesian axis"),
                              ((T, X, tilted, pbc), cs.SLAB_MASK, "component"), ((T, X, C, pbc), (1, 1, 0, 1, 0, 1), "mask")):
        eng.upload([struct])
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*" + msg):
            eng.relax_cell(mask=mask, **good)
        assert np.array_equal(eng.get_cell()[0], struct[2]) and np.isfinite(eng.evaluate_f64([struct])[0]).all()
    _assert_equal(_relax(eng, structs, **good), ref, "after the open-axis refusals")
    fresh = _lj_engine()
    with pytest.raises(backend.BackendError, match="vssr error -5"):
        fresh.relax_cell()
    with pytest.raises(backend.BackendError, match="vssr error -5"):
        fresh.get_cell()
    fresh.close()
    eng.close()


def test_get_cell_after_upload_and_after_a_relaxation():
    eng = _lj_engine()
    structs = cs.mixed_batch() + [cs.slab()]
    eng.upload(structs)
    assert np.array_equal(eng.get_cell(), np.array([s[2] for s in structs]))
    r = eng.relax_cell(max_steps=3, fmax=1e-4, mask=cs.SLAB_MASK)
    cells = eng.get_cell()
    assert np.array_equal(cells, r["cells"]) and np.abs(cells[:, :2, :2] - np.array([s[2] for s in structs])[:, :2, :2]).max() > 1e-4
    assert np.array_equal(cells[:, :, 2], np.array([s[2][:, 2] for s in structs]))  # (the mask holds every strain that involves z)
    eng.upload(structs[:1])
    assert np.array_equal(eng.get_cell()[0], structs[0][2])
    eng.close()
