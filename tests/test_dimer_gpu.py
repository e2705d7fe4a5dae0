"""Device dimer method (vssr_batch_dimer: csrc/dimer.hip) against the numpy restatement tests/dimer_oracle.py driven by the device's own
single-point evaluation, the physics anchor on the device, and the invariants of the call."""

import numpy as np
import pytest

import cg_resident_cases as rc
import dimer_cases as dc
import dimer_oracle as do
import neb_cases as nc
import vib_cases as vc
from test_neb_gpu import _device_forces, _parity_engine      # the device's own evaluation as force callback; the six engines

pytestmark = pytest.mark.gpu

WANT = 1 | 2 | 16   # energy, forces, per-atom energies
DF = 1e-12          # eV / A: what two fp64 evaluations of positions that agree to rounding may differ by (tests/test_md_gpu.py)
KEYS = ("positions", "energies", "modes", "fmax", "curvature", "e0", "f_perp", "n_steps", "stop_reason", "n_rot", "n_eval", "e", "ea", "f")


def _dimer(eng, structs, held, modes=None, upload=True, **kw):
    if upload:
        eng.upload(structs)
    out = eng.dimer(fixed=held, modes=modes, want=WANT, **kw)
    out["counts"], out["regrows"] = eng.last_relax_counts, eng.debug_capacity()
    out["e"], out["ea"], out["f"] = eng.results_f64()
    return out


def _oracle(fn, structs, held, modes=None, record=None, **kw):
    return do.run(fn, np.vstack([s[1] for s in structs]), dc.start_of(structs), fixed=held, modes=modes, record=record, **kw)


def _assert_equal(a, b, tag, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def _close(a, b, tol, tag):
    err = float(np.abs(np.asarray(a) - np.asarray(b)).max()) if np.size(a) else 0.0
    print(f"{tag}: max |device - oracle| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol, tag


def _bounds(rec, g, n_free, n_steps, delta, dF=DF, dtmax=1.0):
    """What a force error of dF per component may make of dimer g, from the restatement's own record of its run.
    eF = sqrt(3 n_free) dF bounds |dF.u| for any unit vector u over the dimer.
    C of an evaluation E, (F0.N - F1.N) / delta:                 dC0 = 2 eF / delta        (the 1 / delta amplification)
    b1 = -|Fp| / (2 delta), Fp from Fd = 2 (F1 - F0):            db1 = 4 eF / (2 delta)
    a1 = (C - C1 + b1 sin 2 phi1) / (1 - cos 2 phi1):            da1 = (2 dC0 + db1) / (1 - cos 2 phi1)
    phim = atan(b1 / a1) / 2, an angle in the (a1, b1) plane:    dphi = (da1 + db1) / (2 hypot(a1, b1))
    T = Fp / |Fp|:                                               dT = 2 (4 eF) / f
    N <- N cos phim + T sin phim:                                dN += dT + dphi per rotation made, on top of 16 eps for the drawn mode
    Cm = a0 / 2 + a1 cos 2 phim + b1 sin 2 phim, a0 = 2 (C - a1): dCm = dC0 + 2 da1 + db1 + 2 (|a1| + |b1|) dphi
    and C under a mode error dN:                                 + |F0 - F1| / delta dN
    x: n steps, each at most dtmax^2 times a force error, doubled by the velocity it leaves: the 10 n^2 dtmax^2 dF of
    tests/test_neb_gpu.py, as it stands there (what dN makes of G = F0 - 2 (F0.N) N is not in it: with dN bounded as loosely as above
    it would leave no test of x at all); the moving end x0 + delta N adds delta dN.
    Returns (bound on x, on N, on C, on f_perp)."""
    eF = np.sqrt(3.0 * n_free) * dF
    dC0 = 2.0 * eF / delta
    dN, dC, hn, f0 = 16.0 * np.finfo(np.float64).eps, dC0, 0.0, 0.0
    for r in rec:
        if r["dimer"] != g:
            continue
        f0 = max(f0, np.sqrt(n_free) * r["fmax_atom"])
        c = r["closed"]
        if c is None:
            continue
        db1 = 2.0 * eF / delta
        da1 = (2.0 * dC0 + db1) / (1.0 - np.cos(2.0 * c["phi1"]))
        dphi = 0.5 * (da1 + db1) / np.hypot(c["a1"], c["b1"])
        dN += 8.0 * eF / c["f"] + dphi
        dC = max(dC, dC0 + 2.0 * da1 + db1 + 2.0 * (abs(c["a1"]) + abs(c["b1"])) * dphi)
        hn = max(hn, c["hn"])
    dC += hn * dN
    n = max(n_steps, 1)
    dx = 10.0 * n * n * dtmax * dtmax * dF + delta * dN
    return dx, dN, dC, 4.0 * eF + 4.0 * delta * hn * dN + 4.0 * f0 * dN


def _compare(dev, ora, rec, structs, held, delta, tag, dF=DF, measured=None):
    start = dc.start_of(structs)
    for key in ("n_steps", "stop_reason", "n_rot", "n_eval"):
        assert np.array_equal(dev[key], ora[key]), (tag, key, dev[key], ora[key])
    for g in range(len(structs) // 2):
        a0, a1, a2 = start[2 * g], start[2 * g + 1], start[2 * g + 2]
        n_free = int((np.asarray(held[a0:a1]) == 0).sum()) if held is not None else a1 - a0
        bx, bn, bc, bf = _bounds(rec, g, n_free, int(ora["n_steps"][g]), delta, dF)
        t = f"{tag} dimer {g} ({a1 - a0} atoms)"
        _close(dev["positions"][a0:a2], ora["positions"][a0:a2], bx, t + " positions")
        _close(dev["modes"][a0:a2], ora["modes"][a0:a2], bn, t + " N")
        assert not dev["modes"][a1:a2].any(), t
        if ora["stop_reason"][g] == 3:
            continue
        _close(dev["curvature"][g], ora["curvature"][g], bc, t + " C")
        _close(dev["fmax"][g], ora["fmax"][g], 2.0 * dF + 1e-10 * abs(ora["fmax"][g]), t + " fmax")
        _close(dev["f_perp"][g], ora["f_perp"][g], bf, t + " f_perp")
        s = max(abs(ora["e0"][g]), 1.0)
        _close(dev["e0"][g] / s, ora["e0"][g] / s, 1e-10, t + " E0")
        if measured is not None:
            for k, a, b in (("x", dev["positions"][a0:a2], ora["positions"][a0:a2]), ("N", dev["modes"][a0:a2], ora["modes"][a0:a2]),
                            ("C", dev["curvature"][g], ora["curvature"][g])):
                measured[k] = max(measured.get(k, 0.0), float(np.abs(np.asarray(a) - np.asarray(b)).max()))


def _margins(rec, tag):
    m = dc.smallest_margins(rec)
    print(f"{tag}: smallest relative margins {({k: float(f'{v:.2e}') for k, v in m.items()})}")
    return m


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dc.PARITY_KINDS)
def test_step_for_step_parity_with_the_oracle_on_the_devices_own_forces(kind, golden):
    eng = _parity_engine(kind, golden)
    structs, held = dc.parity_batch(kind)
    assert [len(s[0]) for s in structs] == [3, 3, 65, 65, 257, 257]
    fn = _device_forces(eng, structs)
    x0 = np.vstack([s[1] for s in structs])
    rec, measured = [], {}
    dev = _dimer(eng, structs, held, **dc.PARITY)
    stress = eng.stress()[0]              # at once, from what the call left on the device
    ora = _oracle(fn, structs, held, record=rec, **dc.PARITY)
    m = _margins(rec, kind)
    assert min(m.values()) >= dc.MARGIN, (kind, m)
    _compare(dev, ora, rec, structs, held, dc.PARITY["delta"], kind, measured=measured)
    print(f"{kind}: measured maxima {measured}; steps {dev['n_steps']}, rotations {dev['n_rot']}, evaluations {dev['n_eval']}")
    assert list(dev["n_steps"]) == [10] * 3 and list(dev["stop_reason"]) == [2] * 3 and dev["n_rot"].min() >= 1
    still = held.astype(bool)
    assert np.array_equal(dev["positions"][still], x0[still]) and np.abs(dev["positions"] - x0).max() > 1e-3
    assert not dev["modes"][still].any()
    # chain 2 g + 1 holds x0 + delta N, and the batch is left with a complete evaluation of the final positions
    start = dc.start_of(structs)
    for g in range(3):
        a0, a1, a2 = start[2 * g], start[2 * g + 1], start[2 * g + 2]
        assert np.array_equal(dev["positions"][a1:a2], dev["positions"][a0:a1] + dc.PARITY["delta"] * dev["modes"][a0:a1])
        assert abs(np.vdot(dev["modes"][a0:a1], dev["modes"][a0:a1]) - 1.0) < 1e-14
    e, f = fn(dev["positions"])
    assert np.array_equal(e, dev["e"]) and np.array_equal(f, dev["f"]) and np.array_equal(dev["energies"], dev["e"])
    assert np.isfinite(stress).all() and np.array_equal(eng.stress()[0], stress)
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _case_engine(case):
    from surface_sampling_amd import backend

    return backend.PairEngine(nc.WALL_TERMS, n_types=2, device=0) if case.terms is nc.WALL_TERMS else rc.engine("pair_lj")


def test_the_census_cases_on_the_device():
    """Every case of dimer_cases.census_cases (tests/test_dimer_cpu.py asserts that together they visit every branch), each under its
    own parameters, against the oracle on the device's forces.  The f = 0 tie of the line case is an exact zero on both sides."""
    for c in dc.census_cases():
        eng = _case_engine(c)
        structs, held, modes = dc.pack([c])
        rec = []
        dev = _dimer(eng, structs, held, modes, **c.params)
        ora = _oracle(_device_forces(eng, structs), structs, held, modes, record=rec, **c.params)
        _compare(dev, ora, rec, structs, held, c.params["delta"], c.name)
        seen = set().union(*[r["branches"] for r in rec])
        print(f"{c.name}: steps {dev['n_steps'][0]}, reason {dev['stop_reason'][0]}, rotations {dev['n_rot'][0]}, evaluations {dev['n_eval'][0]}; {sorted(seen)}")
        if c.name in dc.EXACT:
            assert dev["f_perp"][0] == 0.0 and ora["f_perp"][0] == 0.0 and dev["n_rot"][0] == 0 and "no_rotate_f_zero" in seen
            assert np.array_equal(dev["modes"], ora["modes"])
        if dev["stop_reason"][0] == 3:      # x0 and N back bit for bit, no step counted
            n = len(c.struct[0])
            assert dev["n_steps"][0] == 0 and np.array_equal(dev["positions"][:n], c.struct[1])
            assert np.array_equal(dev["modes"][:n], c.mode / np.sqrt(np.vdot(c.mode, c.mode)))
            assert np.array_equal(dev["positions"][n:], dev["positions"][:n] + c.params["delta"] * dev["modes"][:n])
            assert np.isfinite(dev["e"]).all()
        eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_anchor_on_the_device():
    """The closed-form saddle of neb_cases from one structure: two seeds under the three rotation settings end within the barrier
    bound of 3 (LJ(R) + eps), with the lowest Hessian eigenvalue as curvature and the mode along z; vssr_batch_vibrations on the resident
    batch right after reports exactly one imaginary mode on chain 2 g."""
    eng = rc.engine("pair_lj")
    H = nc.anchor_saddle_hessian()
    lam = np.linalg.eigvalsh(H)
    bound = nc.barrier_bound(dc.ANCHOR["fmax"], H)
    etri = dc.triangle_energy()
    cases = dc.anchor_cases(seeds=(0, 3))
    for c in cases:
        structs, held, modes = dc.pack([c])
        r = _dimer(eng, structs, held, modes, **c.params)
        err = r["e0"][0] - etri + 3.0 * nc.ANCHOR_EPS - nc.ANCHOR_BARRIER
        N = r["modes"][3]
        c_bound = dc.anchor_curvature_bound(N, r["positions"][3] - nc.ANCHOR_CENTRE, H, dc.ANCHOR["delta"], dc.ANCHOR["fmax"])
        print(f"{c.name}: {r['n_steps'][0]} steps, {r['n_rot'][0]} rotations, {r['n_eval'][0]} evaluations, saddle energy error {err:+.3e} eV "
              f"(bound {bound:.3e}), C {r['curvature'][0]:.6f} against lambda {lam[0]:.6f} (difference {r['curvature'][0] - lam[0]:+.3e}, "
              f"bound {c_bound:.3e}), |N.z| {abs(N[2]):.7f}")
        assert r["stop_reason"][0] == 1 and r["n_steps"][0] <= 200 and abs(err) <= bound
        assert r["curvature"][0] < 0.0 and abs(N[2]) > 0.999 and abs(r["curvature"][0] - lam[0]) <= c_bound
        mask = np.zeros(8, np.uint8)
        mask[3] = mask[7] = 1
        assert eng.stats()["atoms"] == 8
        vib = eng.vibrations(np.full(8, 39.948), vib=mask)
        assert vib["n_imag"][0] == 1
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def _eight():
    return [dc.anchor_case(s, a, b, max_steps=25) for s, (a, b) in zip(range(8), dc.ANCHOR_ROTATIONS * 3)]


def test_bits_repeat_and_a_dimer_does_not_depend_on_its_batch():
    eng = rc.engine("pair_lj")
    cases = _eight()
    kw = dict(dc.ANCHOR, max_steps=25, max_rot_first=3, max_rot=1, seed=11)
    structs, held, _ = dc.pack(cases)
    x0 = np.vstack([s[1] for s in structs])
    a = _dimer(eng, structs, held, **kw)
    b = _dimer(eng, structs, held, **kw)
    _assert_equal(a, b, "the same call twice")
    assert list(a["n_steps"]) == [25] * 8 and np.abs(a["positions"] - x0).max() > 0.05
    # eight different drawn modes from one structure
    assert len({tuple(np.round(a["modes"][8 * g + 3], 12)) for g in range(8)}) == 8
    # results_f64 equals a fresh evaluation of pos_out bit for bit; stats work at once
    assert eng.stats()["atoms"] == 64
    e, _, f = eng.evaluate_f64([(s[0], a["positions"][4 * i:4 * i + 4], s[2], s[3]) for i, s in enumerate(structs)])
    assert np.array_equal(e, a["e"]) and np.array_equal(f, a["f"])
    # dimer 5 alone, under its id: the bits it has inside the batch of eight
    alone = _dimer(eng, structs[10:12], held[40:48], dimer_id=[5], **kw)
    for key in ("positions", "modes", "f"):
        assert np.array_equal(alone[key], a[key][40:48]), key
    assert np.array_equal(alone["energies"], a["energies"][10:12])
    for key in ("fmax", "curvature", "e0", "f_perp", "n_steps", "stop_reason", "n_rot", "n_eval"):
        assert alone[key][0] == a[key][5], key
    # dimer_id decides the drawn mode, not the position in the batch
    rev = _dimer(eng, structs, held, dimer_id=list(range(7, -1, -1)), **kw)
    for g in range(8):
        assert np.array_equal(rev["modes"][8 * g:8 * g + 8], a["modes"][8 * (7 - g):8 * (7 - g) + 8]), g
        assert np.array_equal(rev["positions"][8 * g:8 * g + 8], a["positions"][8 * (7 - g):8 * (7 - g) + 8]), g
    # held atoms: not by a bit, in either chain
    still = held.astype(bool)
    assert np.array_equal(a["positions"][still], x0[still])
    eng.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def _wall_batch(middle):
    """Two healthy dimers on the wall handle (type-1 atoms under the 1 - 1 lj/cut term) around `middle` (None: without it)."""
    T = np.ones(4, np.int32)
    healthy = [dc.Case(f"healthy{k}", (T,) + nc.anchor_image(*xyz)[1:], nc.ANCHOR_HELD, m, {}, nc.WALL_TERMS)
               for k, (xyz, m) in enumerate((((0.10, -0.05, 0.40), np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0.3, 0.1, 0.9]], float)),
                                             ((-0.08, 0.12, -0.35), np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0.2, -0.4, 0.8]], float))))]
    return [healthy[0]] + ([middle] if middle is not None else []) + [healthy[1]]


def test_stops_and_restore():
    """Reasons 1 and 2; reason 3 at the first evaluation, at an evaluation E after a step and at an evaluation R after a step; in every
    reason-3 case the neighbouring dimers have the bits of the batch without it."""
    from surface_sampling_amd import backend

    eng = backend.PairEngine(nc.WALL_TERMS, n_types=2, device=0)
    kw = dict(dc.ANCHOR, max_steps=12, max_rot_first=0, max_rot=1)
    s0, h0, m0 = dc.pack(_wall_batch(None))
    ref = _dimer(eng, s0, h0, m0, **kw)
    assert list(ref["stop_reason"]) == [2, 2] and list(ref["n_steps"]) == [12, 12] and ref["n_rot"].min() >= 6
    z = _dimer(eng, s0, h0, m0, **dict(kw, max_steps=0))
    assert list(z["stop_reason"]) == [2, 2] and list(z["n_steps"]) == [0, 0] and list(z["n_eval"]) == [1, 1] and z["counts"][0] == 1
    assert np.array_equal(z["positions"][:4], s0[0][1])
    # an overflowing start: the free atom inside the wall's cutoff at the first evaluation
    first = dc.wall_case_E()
    X = first.struct[1].copy()
    X[1, 0] = 12.6
    first = first._replace(name="wall_at_first", struct=(first.struct[0], X) + first.struct[2:])
    for middle, n_eval in ((first, 1), (dc.wall_case_E(), 2), (dc.wall_case_R(), 3)):
        over = {k: v for k, v in middle.params.items() if k in ("max_rot_first", "max_rot", "maxstep")}
        kw_m = dict(kw, **over)
        ref_m = _dimer(eng, s0, h0, m0, **kw_m)
        structs, held, modes = dc.pack(_wall_batch(middle))
        fn = _device_forces(eng, structs)
        rec = []
        dev = _dimer(eng, structs, held, modes, **kw_m)
        ora = _oracle(fn, structs, held, modes, record=rec, **kw_m)
        print(f"{middle.name}: steps {dev['n_steps']}, stop {dev['stop_reason']}, evaluations {dev['n_eval']}, lock-step evaluations {dev['counts'][0]}")
        _compare(dev, ora, rec, structs, held, kw["delta"], middle.name)
        assert list(dev["stop_reason"]) == [2, 3, 2] and dev["n_steps"][1] == 0 and dev["n_eval"][1] == n_eval
        n = 3
        assert np.array_equal(dev["positions"][8:8 + n], middle.struct[1])
        assert np.array_equal(dev["modes"][8:8 + n], middle.mode / np.sqrt(np.vdot(middle.mode, middle.mode)))
        assert np.array_equal(dev["positions"][8 + n:8 + 2 * n], middle.struct[1] + kw["delta"] * dev["modes"][8:8 + n])
        if middle.name != "wall_at_first":
            assert np.isfinite(dev["e"]).all()
        e, f = fn(dev["positions"])
        assert np.array_equal(e, dev["e"], equal_nan=True) and np.array_equal(f, dev["f"], equal_nan=True)
        for key in ("positions", "modes", "f"):
            assert np.array_equal(dev[key][:8], ref_m[key][:8]) and np.array_equal(dev[key][14:], ref_m[key][8:]), (middle.name, key)
        for key in ("curvature", "e0", "fmax", "n_rot", "n_eval"):
            assert dev[key][0] == ref_m[key][0] and dev[key][2] == ref_m[key][1], (middle.name, key)
    eng.close()
    # reason 1 beside reason 2: the anchor with and without the steps it needs
    eng = rc.engine("pair_lj")
    cases = [dc.anchor_case(0, 8, 1), dc.anchor_case(0, 8, 1)]
    structs, held, _ = dc.pack(cases)
    full = _dimer(eng, structs, held, **dict(dc.ANCHOR, max_rot_first=8, max_rot=1, seed=0))
    short = _dimer(eng, structs, held, **dict(dc.ANCHOR, max_rot_first=8, max_rot=1, seed=0, max_steps=20))
    assert list(full["stop_reason"]) == [1, 1] and list(short["stop_reason"]) == [2, 2] and list(short["n_steps"]) == [20, 20]
    assert full["fmax"][0] < dc.ANCHOR["fmax"] and full["curvature"][0] < 0 and short["fmax"][0] > dc.ANCHOR["fmax"]
    eng.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_capacity_regrow_in_the_middle_of_a_search():
    """The 27-atom cluster of vib_cases.tight_cluster (second neighbours at the cutoff) under 5 slots per atom: an evaluation
    overflows, the run regrows and ends with the bits of the roomy run."""
    s = vc.tight_cluster()
    structs = [s, s, s, s]
    kw = dict(dc.ANCHOR, max_steps=20, max_rot_first=3, max_rot=1, fmax=1e-4, seed=5, displace=0.3)
    roomy_eng = rc.engine("pair_lj")
    roomy = _dimer(roomy_eng, structs, None, **kw)
    roomy_eng.close()
    tight_eng = rc.engine("pair_lj")
    tight_eng.debug_capacity(slots_per_atom=vc.TIGHT_SLOTS_PER_ATOM, tight=1)
    tight = _dimer(tight_eng, structs, None, **kw)
    tight_eng.close()
    print(f"roomy counts {roomy['counts']} regrows {roomy['regrows']}; tight counts {tight['counts']} regrows {tight['regrows']}")
    assert roomy["regrows"] == 0 and tight["regrows"] >= 1 and tight["counts"][0] > roomy["counts"][0]
    _assert_equal(tight, roomy, "tight against roomy")
    assert list(roomy["n_steps"]) == [20, 20]


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_painn_follows_the_oracle_on_its_own_forces(golden):
    """The SrTiO3 2 x 2 slab as two dimers, 3 steps, delta = 0.01; the oracle is fed the energies (fp64 ensemble mean) and forces (fp32,
    widened) the device returns for the same batch; dF = one fp32 ulp of the largest force component."""
    from surface_sampling_amd import backend, structures

    S = golden.structure("SrTiO3_2x2_pristine")
    T, X, cell, pbc = structures.as_arrays(S)
    structs = [(T, X, cell, pbc)] * 4
    held = np.tile((X[:, 2] < X[:, 2].min() + 1.0).astype(np.uint8), 4)
    start = dc.start_of(structs)
    eng = backend.PainnEngine(golden.blobs, device=0)

    def fn(pos):
        r = eng.evaluate([(T, pos[start[b]:start[b + 1]], cell, pbc) for b in range(4)])
        return r["energy_f64"], r["forces"].astype(np.float64)

    dF = float(np.spacing(np.float32(np.abs(fn(np.vstack([X] * 4))[1]).max())))
    kw = dict(max_steps=3, max_rot_first=3, max_rot=1, delta=0.01, phi_tol=np.pi / 180.0, fmax=1e-4, seed=3)
    eng.upload(structs)
    dev = eng.dimer(fixed=held, **kw)
    res = eng.download()
    rec = []
    ora = _oracle(fn, structs, held, record=rec, **kw)
    _margins(rec, "PaiNN")
    _compare(dev, ora, rec, structs, held, 0.01, "PaiNN", dF=dF)
    assert list(dev["n_steps"]) == [3, 3] and not np.array_equal(dev["modes"][:len(X)], dev["modes"][2 * len(X):3 * len(X)])
    assert np.array_equal(res["forces"], eng.evaluate([(T, dev["positions"][start[b]:start[b + 1]], cell, pbc) for b in range(4)])["forces"])
    eng.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from surface_sampling_amd import backend

    eng = rc.engine("pair_lj")
    cases = _eight()[:3]
    structs, held, _ = dc.pack(cases)
    good = dict(dc.ANCHOR, max_steps=6, max_rot_first=3, max_rot=1, seed=2)
    ref = _dimer(eng, structs, held, **good)
    fields = [n for n, _ in backend.DimerParams._fields_]

    def params(**over):
        p = backend.DimerParams.default(**{k: v for k, v in good.items()})
        for k, v in over.items():
            assert k in fields
            setattr(p, k, v)
        return p

    nan, inf = float("nan"), float("inf")
    bad = [(dict(max_steps=-1), "max_steps"), (dict(max_rot_first=-1), "max_rot_first"), (dict(max_rot=-1), "max_rot"), (dict(nmin=-1), "nmin"),
           (dict(finc=0.9), "finc"), (dict(fdec=0.0), "fdec"), (dict(fdec=1.0), "fdec"), (dict(fa=0.0), "fa"), (dict(fa=1.0), "fa"),
           (dict(astart=0.0), "astart"), (dict(astart=1.5), "astart"), (dict(phi_tol=0.0), "phi_tol"), (dict(phi_tol=-0.1), "phi_tol"),
           (dict(phi_tol=0.8), "phi_tol"), (dict(phi_tol=nan), "phi_tol"), (dict(displace=nan), "displace"), (dict(displace=inf), "displace")]
    for name in ("delta", "fmax", "dt", "maxstep", "dtmax"):
        bad += [({name: v}, name) for v in (0.0, -1.0, nan, inf)]
    for over, msg in bad:
        eng.upload(structs)
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*" + msg):
            eng.dimer(fixed=held, params=params(**over))
        _assert_equal(_dimer(eng, structs, held, upload=False, **good), ref, msg)
    lib, h = eng._lib, eng._h
    eng.upload(structs)
    assert lib.vssr_batch_dimer(h, None, None, None, None, WANT, None, None, None, None, None) == -1 and b"parameters" in lib.vssr_last_error(h)
    _assert_equal(_dimer(eng, structs, held, upload=False, **good), ref, "after the null refusal")
    # an odd number of chains
    eng.upload(structs[:3])
    with pytest.raises(backend.BackendError, match=r"vssr error -1: .*even"):
        eng.dimer(fixed=held[:12], **good)
    assert np.isfinite(eng.evaluate_f64(structs[:3])[0]).all()
    # a mode without length over the free atoms, a non-finite one, and no free atom to draw for
    zero = np.zeros((24, 3))
    zero[:3] = 1.0                                   # (held rows only)
    zero[11] = zero[19] = [0.0, 0.0, 1.0]
    for m, fx, msg in ((zero, held, "mode_in"), (np.where(np.arange(24)[:, None] == 3, nan, 1.0) * np.ones((24, 3)), held, "mode_in"),
                       (None, np.ones(24, np.uint8), "no free atom")):
        eng.upload(structs)
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*" + msg):
            eng.dimer(fixed=fx, modes=m, **good)
        _assert_equal(_dimer(eng, structs, held, upload=False, **good), ref, msg)
    # chains of a dimer that differ in more than positions: atom count, species, cell, pbc, fixed mask
    T, X, cell, pbc = structs[0]
    for other, msg in (((T[:3], X[:3], cell, pbc), "atom counts"), ((np.array([0, 0, 0, 1], np.int32), X, cell, pbc), "species"),
                       ((T, X, cell * (1.0 + 2.0 ** -40), pbc), "cell"), ((T, X, cell, np.array([0, 0, 1], np.uint8)), "pbc")):
        eng.upload([structs[0], other])
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*(dimer)"):
            eng.dimer(fixed=None, **good)
        assert np.isfinite(eng.evaluate_f64([structs[0], other])[0]).all()      # the handle serves the next call
    eng.upload(structs)
    mask = held.copy()
    mask[4] = 0
    with pytest.raises(backend.BackendError, match=r"vssr error -1: .*fixed mask"):
        eng.dimer(fixed=mask, **good)
    _assert_equal(_dimer(eng, structs, held, **good), ref, "after the chain refusals")
    fresh = rc.engine("pair_lj")
    with pytest.raises(backend.BackendError, match="vssr error -5"):
        fresh.dimer()
    fresh.close()
    eng.close()
