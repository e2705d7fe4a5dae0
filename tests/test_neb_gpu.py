"""Device nudged elastic band (vssr_batch_neb: csrc/neb.hip) against the numpy restatement tests/neb_oracle.py driven by the device's own
single-point evaluation, the physics anchor on the device, and the invariants of the call."""
import ctypes as C

import numpy as np
import pytest

import cg_resident_cases as rc
import neb_cases as nc
import neb_oracle as no
import pair_cases as pc
import vib_cases as vc

pytestmark = pytest.mark.gpu

WANT = 1 | 2 | 16   # energy, forces, per-atom energies
DF = 1e-12          # eV / A: what two fp64 evaluations of positions that agree to rounding may differ by (tests/test_md_gpu.py)
N_STEPS = 10


def _start(structs):
    return np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])]).astype(np.int64)


def _device_forces(eng, structs):
    """The device's own single-point evaluation as the oracle's force callback: the potential's tolerance does not enter."""
    from surface_sampling_amd import backend

    n_atoms, T, _, cell, pbc = backend.pack_batch(structs)

    def fn(pos):
        e, _, f = eng.evaluate_arrays_f64(n_atoms, T, pos, cell, pbc)
        return e, f
    return fn


def _neb(eng, structs, n_img, held, upload=True, **kw):
    if upload:
        eng.upload(structs)
    out = eng.neb(n_img, fixed=held, want=WANT, **kw)
    out["counts"], out["regrows"] = eng.last_relax_counts, eng.debug_capacity()
    out["e"], out["ea"], out["f"] = eng.results_f64()
    return out


def _oracle(fn, structs, n_img, held, **kw):
    kw = dict(kw)
    if "max_steps" not in kw:
        kw["max_steps"] = 100
    return no.run(fn, np.vstack([s[1] for s in structs]), _start(structs), n_img, [s[2] for s in structs], [s[3] for s in structs],
                  fixed=held, **kw)


KEYS = ("positions", "energies", "neb_forces", "fmax", "barrier_forward", "barrier_reverse", "n_steps", "stop_reason", "imax", "e", "ea", "f")


def _assert_equal(a, b, tag, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)


def _close(a, b, tol, tag):
    err = float(np.abs(np.asarray(a) - np.asarray(b)).max()) if np.size(a) else 0.0
    print(f"{tag}: max |device - oracle| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol, tag


def _bounds(structs, n_img, k, n_steps, dtmax=1.0):
    """Positions: 10 n^2 dtmax^2 dF (n steps, each at most dtmax^2 times a force error, doubled by the velocity it leaves; tests/test_md_gpu.py
    derives its own the same way).  G: dF (1 + k path length), the force error plus what the spring term makes of position errors."""
    longest, b = 0.0, 0
    for n in n_img:
        x = np.array([structs[b + i][1] for i in range(n)])
        longest = max(longest, no.path(x, structs[b][2], structs[b][3])[-1])
        b += n
    return 10.0 * n_steps * n_steps * dtmax * dtmax * DF, DF * (1.0 + k * longest)


def _compare(dev, ora, structs, n_img, k, n_steps, tag, positions_bound=None):
    bx, bg = _bounds(structs, n_img, k, max(n_steps, 1))
    assert np.array_equal(dev["n_steps"], ora["n_steps"]) and np.array_equal(dev["stop_reason"], ora["stop_reason"]), \
        (tag, dev["n_steps"], ora["n_steps"], dev["stop_reason"], ora["stop_reason"])
    assert np.array_equal(dev["imax"], ora["imax"]), tag
    _close(dev["positions"], ora["positions"], positions_bound or bx, tag + " positions")
    _close(dev["neb_forces"], ora["neb_forces"], bg, tag + " NEB forces")
    _close(dev["fmax"], ora["fmax"], bg, tag + " fmax")
    for key in ("energies", "barrier_forward", "barrier_reverse"):
        s = np.maximum(np.abs(ora[key]), 1.0)
        _close(dev[key] / s, ora[key] / s, 1e-10, f"{tag} {key}")


# 1 ---------------------------------------------------------------------------------------------------------------------------------
PARITY_KINDS = ("pair_lj", "sw", "eam_alloy", "tersoff", "vashishta", "ewald")
PARITY_SIZES, PARITY_IMAGES = (3, 65, 257), (3, 4, 7)
# (types in use, grid spacing in A) of the kinds cg_resident_cases does not know
EXTRA_SHAPE = {"tersoff": (2, 1.95), "vashishta": (2, 1.9), "ewald": (2, 2.7)}
# Geometry of the parity bands.  Device and oracle positions agree to an ulp (1.8e-15 .. 3.6e-15 A at coordinates of 10 .. 20 A), never
# to the bit: the band sums are reduced in another order.  dF = 1e-12 eV / A covers what that does to the forces of well-conditioned
# structures (force constants up to ~5e2 eV / A^2), and the bound on G, dF (1 + k L), what it does to the spring term.  The projection
# adds 2 |F.t| ulp / |t|: the tangent is a difference of positions divided by its length.  The bands are built so that this term stays
# an order below dF: grids rattled by PARITY_JITTER only (forces of a few eV / A) and images a rigid PARITY_SHIFT of the free atoms
# apart (|t| >= 0.3 A for the one free atom of the smallest chain, > 1 A for the others), plus N(0, PARITY_MOVE) per atom.
PARITY_JITTER, PARITY_MOVE, PARITY_SHIFT = 0.05, 0.05, np.array([0.5, 0.3, 0.2])


def _parity_engine(kind, golden):
    from surface_sampling_amd import backend, pair

    if kind in ("pair_lj", "sw", "eam_alloy", "tersoff"):
        return vc.engine(kind, golden)
    if kind == "ewald":
        import ewald_cases as ec

        return backend.PairEngine(pair.parse(ec.RAGGED_MODEL, 3), device=0)
    import vashishta_oracle as vo

    return backend.VashishtaEngine(vo.sic_params()[1], device=0)


def _parity_batch(kind):
    """One ragged batch: bands of 3, 4 and 7 images over chains of 3, 65 and 257 atoms (below one wave, across the 64-lane edge, beyond
    one 256-thread pass); the first two atoms of every chain held; the largest chain periodic in x and y (an Ewald sum wants three
    periodic axes on every chain).  The last image is the first with every free atom displaced by PARITY_SHIFT + N(0, PARITY_MOVE), linear in between."""
    structs, n_img = [], list(PARITY_IMAGES)
    for k, (n, m) in enumerate(zip(PARITY_SIZES, PARITY_IMAGES)):
        pbc = [1, 1, 1] if kind == "ewald" else ([1, 1, 0] if n == 257 else [0, 0, 0])
        if kind in EXTRA_SHAPE:
            nt, spacing = EXTRA_SHAPE[kind]
            T, X, cell, p = pc.grid_chain(n, 80 + k, pbc, n_types=nt, spacing=spacing, jitter=PARITY_JITTER)
        else:
            T, X, cell, p = rc.grid(kind, n, 80 + k, pbc, jitter=PARITY_JITTER)
        d = np.random.default_rng(90 + k).normal(0, PARITY_MOVE, X.shape) + PARITY_SHIFT
        d[:2] = 0.0
        structs += [(T, X + d * (i / (m - 1)), cell, p) for i in range(m)]
    return structs, n_img, pc.held_mask(structs)


@pytest.mark.parametrize("kind", PARITY_KINDS)
def test_step_for_step_parity_with_the_oracle_on_the_devices_own_forces(kind, golden):
    eng = _parity_engine(kind, golden)
    structs, n_img, held = _parity_batch(kind)
    assert [len(s[0]) for s in structs] == [3] * 3 + [65] * 4 + [257] * 7
    fn = _device_forces(eng, structs)
    x0 = np.vstack([s[1] for s in structs])
    start, first = _start(structs), np.concatenate([[0], np.cumsum(n_img)])
    for method in no.METHODS:
        for climb in (False, True):
            kw = dict(k=0.1, climb=climb, method=method, fmax=1e-4, max_steps=N_STEPS)
            dev = _neb(eng, structs, n_img, held, **kw)
            stress = eng.stress()[0]              # at once, from what the call left on the device
            ora = _oracle(fn, structs, n_img, held, **kw)
            tag = f"{kind} {method} climb={int(climb)}"
            _compare(dev, ora, structs, n_img, 0.1, N_STEPS, tag)
            assert list(dev["n_steps"]) == [N_STEPS] * 3 and list(dev["stop_reason"]) == [2] * 3, tag
            still = held.astype(bool)
            for g in range(3):      # the end images too
                still[start[first[g]]:start[first[g] + 1]] = True
                still[start[first[g + 1] - 1]:start[first[g + 1]]] = True
            assert np.array_equal(dev["positions"][still], x0[still]) and np.abs(dev["positions"] - x0).max() > 1e-3, tag
            assert not dev["neb_forces"][still].any()
            # the batch is left with a complete evaluation of the final positions
            e, f = fn(dev["positions"])
            assert np.array_equal(e, dev["e"]) and np.array_equal(f, dev["f"]) and np.array_equal(dev["energies"], dev["e"]), tag
            assert np.isfinite(stress).all() and np.array_equal(eng.stress()[0], stress), tag
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_census_cases_on_the_device():
    """Every case of neb_cases.census_cases (tests/test_neb_cpu.py asserts that together they visit every branch), each under its own
    parameters, against the oracle on the device's forces."""
    eng = rc.engine("pair_lj")
    for c in nc.census_cases():
        structs, n_img, held = nc.pack([c])
        dev = _neb(eng, structs, n_img, held, **c.params)
        ora = _oracle(_device_forces(eng, structs), structs, n_img, held, **c.params)
        n = int(ora["n_steps"][0])
        _compare(dev, ora, structs, n_img, c.params["k"], n, c.name)
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_anchor_on_the_device():
    """The 6-image climbing band reaches the closed-form barrier within 2 fmax^2 / (2 min |lambda|); without climbing it misses by more
    than 0.1 eV; the climbing image has exactly one imaginary mode."""
    eng = rc.engine("pair_lj")
    bound = nc.barrier_bound(nc.ANCHOR["fmax"], nc.anchor_saddle_hessian())
    cases = {c.name: c for c in nc.census_cases()}
    structs, n_img, held = nc.pack([cases["anchor6_plain_improved"]])
    plain = _neb(eng, structs, n_img, held, **cases["anchor6_plain_improved"].params)
    miss = nc.ANCHOR_BARRIER - plain["barrier_forward"][0]
    print(f"6 images without climbing: {plain['n_steps'][0]} steps, barrier misses by {miss:.4f} eV")
    assert plain["stop_reason"][0] == 1 and miss > 0.1
    for name in ("anchor6_climb_improved", "anchor6_climb_aseneb"):
        structs, n_img, held = nc.pack([cases[name]])
        r = _neb(eng, structs, n_img, held, **cases[name].params)
        err = r["barrier_forward"][0] - nc.ANCHOR_BARRIER
        print(f"{name}: {r['n_steps'][0]} steps, barrier error {err:+.3e} eV (bound {bound:.3e})")
        assert r["stop_reason"][0] == 1 and r["n_steps"][0] <= 200 and abs(err) <= bound
        assert abs(r["barrier_forward"][0] - r["barrier_reverse"][0]) <= 1e-9
        # vibrations at once on the resident batch: the climbing image is a first-order saddle of the free atom
        imax = int(r["imax"][0])
        mask = np.zeros(24, np.uint8)
        mask[4 * imax + 3] = 1
        stats = eng.stats()
        assert stats["atoms"] == 24
        vib = eng.vibrations(np.full(24, 39.948), vib=mask)
        assert vib["n_imag"][imax] == 1 and [int(v) for v in vib["n_imag"]] == [1 if g == imax else 0 for g in range(6)]
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def _three_bands():
    cases = {c.name: c for c in nc.census_cases()}
    return [cases["bowed9"], cases["anchor6_climb_improved"], cases["tie3"]]


def test_bits_repeat_and_a_band_does_not_depend_on_its_batch():
    eng = rc.engine("pair_lj")
    bands = _three_bands()
    kw = dict(k=0.1, climb=True, method="improvedtangent", fmax=0.01, max_steps=25)
    structs, n_img, held = nc.pack(bands)
    x0 = np.vstack([s[1] for s in structs])
    a = _neb(eng, structs, n_img, held, **kw)
    b = _neb(eng, structs, n_img, held, **kw)
    _assert_equal(a, b, "the same call twice")
    assert list(a["n_steps"]) == [25, 25, 25] and np.abs(a["positions"] - x0).max() > 0.05
    # results_f64 equals a fresh evaluation of pos_out bit for bit; stats work at once
    assert eng.stats()["atoms"] == 72
    e, _, f = eng.evaluate_f64([(s[0], a["positions"][4 * i:4 * i + 4], s[2], s[3]) for i, s in enumerate(structs)])
    assert np.array_equal(e, a["e"]) and np.array_equal(f, a["f"])
    s1, n1, h1 = nc.pack(bands[1:2])
    alone = _neb(eng, s1, n1, h1, **kw)
    a0, a1 = 4 * 9, 4 * 15
    for key in ("positions", "neb_forces", "f"):
        assert np.array_equal(alone[key], a[key][a0:a1]), key
    assert np.array_equal(alone["energies"], a["energies"][9:15])
    for key in ("fmax", "barrier_forward", "barrier_reverse", "n_steps", "stop_reason", "imax"):
        assert alone[key][0] == a[key][1], key
    # ends and held atoms: not by a bit
    still = np.tile(nc.ANCHOR_HELD.astype(bool), 18)
    for f, n in zip((0, 9, 15), n_img):
        still[4 * f:4 * f + 4] = True
        still[4 * (f + n - 1):4 * (f + n)] = True
    assert np.array_equal(a["positions"][still], x0[still])
    eng.close()


def test_stops():
    """max_steps = 0; a band at rest; coincident images; a non-finite image between two healthy bands."""
    eng = rc.engine("pair_lj")
    bands = _three_bands()
    structs, n_img, held = nc.pack(bands)
    x0 = np.vstack([s[1] for s in structs])
    kw = dict(k=0.1, climb=False, method="improvedtangent", fmax=0.01)
    z = _neb(eng, structs, n_img, held, max_steps=0, **kw)
    ora = _oracle(_device_forces(eng, structs), structs, n_img, held, max_steps=0, **kw)
    assert np.array_equal(z["positions"], x0) and list(z["n_steps"]) == [0, 0, 0] and list(z["stop_reason"]) == [2, 2, 2]
    _compare(z, ora, structs, n_img, 0.1, 0, "max_steps = 0")
    assert np.abs(z["neb_forces"]).max() > 0.01 and z["counts"][0] == 1
    # every image at one relaxed minimum: 0 steps, reason 1 (all tangents have zero length, and the band has converged as it stands)
    rest = [nc.anchor_image(0.0, 0.0, nc.ANCHOR_ZMIN)] * 4
    r = _neb(eng, rest, [4], np.tile(nc.ANCHOR_HELD, 4), max_steps=20, **kw)
    print(f"band at rest: fmax {r['fmax'][0]:.2e} eV / A")
    assert (r["n_steps"][0], r["stop_reason"][0]) == (0, 1) and r["fmax"][0] < 1e-6
    # two coincident images off the minimum: reason 4, nothing moves; the neighbours in the batch run on
    ref = _neb(eng, structs, n_img, held, max_steps=12, **kw)
    b6 = bands[1].band
    twin = nc.Case("twin", [b6[0], b6[2], b6[2], b6[5]], nc.ANCHOR_HELD, {})
    s2, n2, h2 = nc.pack([bands[0], twin, bands[2]])
    t = _neb(eng, s2, n2, h2, max_steps=12, **kw)
    assert list(t["stop_reason"]) == [2, 4, ref["stop_reason"][2]] and t["n_steps"][1] == 0
    assert np.array_equal(t["positions"][36:52], np.vstack([s[1] for s in twin.band]))
    assert np.array_equal(t["positions"][:36], ref["positions"][:36]) and np.array_equal(t["positions"][52:], ref["positions"][60:])
    # an end image whose free atom sits 1e-150 A from a held one (exactly coincident atoms are no neighbors, these are, and lj/cut
    # overflows; the pair stands at z = 0, where 1e-150 is not rounded away): reason 3 at the first test, nothing moved, and the
    # neighbours are unaffected
    broken = [(s[0], s[1].copy(), s[2], s[3]) for s in b6]
    broken[5][1][0, 2] = 0.0
    broken[5][1][3] = broken[5][1][0] + [0.0, 0.0, 1e-150]
    s3, n3, h3 = nc.pack([bands[0], nc.Case("broken", broken, nc.ANCHOR_HELD, {}), bands[2]])
    w = _neb(eng, s3, n3, h3, max_steps=12, **kw)
    print(f"non-finite image: steps {w['n_steps']}, stop {w['stop_reason']}, E {w['energies'][9:15]}")
    assert list(w["stop_reason"]) == [2, 3, ref["stop_reason"][2]] and w["n_steps"][1] == 0
    assert np.array_equal(w["positions"][36:60], np.vstack([s[1] for s in broken])) and not np.isfinite(w["energies"][14])
    for key in ("positions", "neb_forces", "f"):
        assert np.array_equal(w[key][:36], ref[key][:36]) and np.array_equal(w[key][60:], ref[key][60:]), key
    eng.close()


def test_a_band_that_runs_into_a_wall_goes_back_to_where_its_step_opened():
    """neb_cases.wall_band between two healthy bands: finite at the start, non-finite after its first step (a term that overflows
    everywhere inside its 0.6 A cutoff), reason 3 with 0 steps standing and the input positions back bit for bit; the neighbours run on
    as they do without it, and the batch is left evaluated at the final positions."""
    from surface_sampling_amd import backend

    eng = backend.PairEngine(nc.WALL_TERMS, n_types=2, device=0)
    bands = _three_bands()
    wall = nc.Case("wall", nc.wall_band(), nc.WALL_HELD, {})
    kw = dict(k=0.1, climb=False, method="improvedtangent", fmax=0.01, max_steps=12)
    structs, n_img, held = nc.pack([bands[0], wall, bands[2]])
    x0 = np.vstack([s[1] for s in structs])
    fn = _device_forces(eng, structs)
    e0, f0 = fn(x0)
    assert np.isfinite(e0).all() and np.isfinite(f0).all()
    dev = _neb(eng, structs, n_img, held, **kw)
    ora = _oracle(fn, structs, n_img, held, **kw)
    print(f"wall band: steps {dev['n_steps']}, stop {dev['stop_reason']}, lock-step evaluations {dev['counts'][0]}")
    assert list(dev["n_steps"]) == [12, 0, 12] and list(dev["stop_reason"]) == [2, 3, 2]
    assert np.array_equal(dev["n_steps"], ora["n_steps"]) and np.array_equal(dev["stop_reason"], ora["stop_reason"])
    assert np.array_equal(dev["positions"][36:45], x0[36:45]) and np.array_equal(dev["energies"][9:12], e0[9:12])
    _close(dev["positions"], ora["positions"], _bounds(structs, n_img, 0.1, 12)[0], "wall batch positions")
    e, f = fn(dev["positions"])
    assert np.array_equal(e, dev["e"]) and np.array_equal(f, dev["f"]) and np.isfinite(e).all()
    # the neighbours: the bits of the same batch without the wall band
    s2, n2, h2 = nc.pack([bands[0], bands[2]])
    ref = _neb(eng, s2, n2, h2, **kw)
    for key in ("positions", "neb_forces", "f"):
        assert np.array_equal(dev[key][:36], ref[key][:36]) and np.array_equal(dev[key][45:], ref[key][36:]), key
    eng.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_capacity_regrow_in_the_middle_of_a_band():
    """The 27-atom cluster of vib_cases.tight_cluster (second neighbours at the cutoff) as a 4-image band under 5 slots per atom: the
    evaluation overflows, the run regrows and ends with the bits of the roomy run."""
    T, X, cell, pbc = vc.tight_cluster()
    d = np.random.default_rng(5).normal(0, 0.25, X.shape)
    structs = [(T, X + d * (i / 3), cell, pbc) for i in range(4)]
    kw = dict(k=0.1, climb=True, method="improvedtangent", fmax=1e-4, max_steps=20)
    roomy_eng = rc.engine("pair_lj")
    roomy = _neb(roomy_eng, structs, [4], None, **kw)
    roomy_eng.close()
    tight_eng = rc.engine("pair_lj")
    tight_eng.debug_capacity(slots_per_atom=vc.TIGHT_SLOTS_PER_ATOM, tight=1)
    tight = _neb(tight_eng, structs, [4], None, **kw)
    tight_eng.close()
    print(f"roomy counts {roomy['counts']} regrows {roomy['regrows']}; tight counts {tight['counts']} regrows {tight['regrows']}")
    assert roomy["regrows"] == 0 and tight["regrows"] >= 1 and tight["counts"][0] > roomy["counts"][0]
    _assert_equal(tight, roomy, "tight against roomy")
    assert list(roomy["n_steps"]) == [20]


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_painn_follows_the_oracle_on_its_own_forces(golden):
    """The SrTiO3 2 x 2 slab and a copy with one top-layer atom moved 0.8 A, 4 images, 3 steps; the oracle is fed the energies (fp64
    ensemble mean) and forces (fp32, widened) the device returns for the same band."""
    from surface_sampling_amd import backend, structures

    S = golden.structure("SrTiO3_2x2_pristine")
    T, X, cell, pbc = structures.as_arrays(S)
    top = int(np.argmax(X[:, 2]))
    d = np.zeros_like(X)
    d[top] = [0.8 * np.cos(0.3), 0.8 * np.sin(0.3), 0.0]
    structs = [(T, X + d * (i / 3), cell, pbc) for i in range(4)]
    held = np.tile((X[:, 2] < X[:, 2].min() + 1.0).astype(np.uint8), 4)
    start = _start(structs)
    eng = backend.PainnEngine(golden.blobs, device=0)

    def fn(pos):
        r = eng.evaluate([(T, pos[start[b]:start[b + 1]], cell, pbc) for b in range(4)])
        return r["energy_f64"], r["forces"].astype(np.float64)

    for method in no.METHODS:
        kw = dict(k=0.1, climb=True, method=method, fmax=1e-4, max_steps=3)
        eng.upload(structs)
        dev = eng.neb([4], fixed=held, **kw)
        res = eng.download()
        ora = _oracle(fn, structs, [4], held, **kw)
        _compare(dev, ora, structs, [4], 0.1, 3, f"PaiNN {method}")
        assert list(dev["n_steps"]) == [3] and np.array_equal(dev["positions"][:len(X)], X)
        assert np.array_equal(res["forces"], eng.evaluate([(T, dev["positions"][start[b]:start[b + 1]], cell, pbc) for b in range(4)])["forces"])
    eng.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from surface_sampling_amd import backend

    eng = rc.engine("pair_lj")
    bands = _three_bands()
    structs, n_img, held = nc.pack(bands)
    good = dict(k=0.1, climb=True, method="improvedtangent", fmax=0.01, max_steps=6)
    ref = _neb(eng, structs, n_img, held, **good)
    fire = ("dt", "maxstep", "dtmax", "finc", "fdec", "astart", "fa", "nmin")

    def params(**over):
        base = dict(max_steps=6, method="improvedtangent", climb=True, k=0.1, fmax=0.01)
        p = backend.NebParams.default(**{**base, **{k: v for k, v in over.items() if k in base or k in fire}})
        for k, v in over.items():
            if k not in base and k not in fire:
                setattr(p, k, v)
        return p

    nan, inf = float("nan"), float("inf")
    cases = [(dict(max_steps=-1), "max_steps"), (dict(nmin=-1), "nmin"), (dict(finc=0.9), "finc"), (dict(fdec=0.0), "fdec"), (dict(fdec=1.0), "fdec"),
             (dict(fa=0.0), "fa"), (dict(fa=1.0), "fa"), (dict(astart=0.0), "astart"), (dict(astart=1.5), "astart")]
    for name in ("k", "fmax", "dt", "maxstep", "dtmax"):
        cases += [({name: v}, name) for v in (0.0, -1.0, nan, inf)]
    for over, msg in cases:
        eng.upload(structs)
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*" + msg):
            eng.neb(n_img, fixed=held, params=params(**over))
        _assert_equal(_neb(eng, structs, n_img, held, upload=False, **good), ref, msg)
    lib, h = eng._lib, eng._h
    eng.upload(structs)
    ip = lambda a: np.asarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    call = lambda p, imgs, nb: lib.vssr_batch_neb(h, C.byref(p) if p is not None else None, None, ip(imgs) if imgs is not None else None, nb, WANT,
                                                  None, None, None, None, None)
    p = params()
    assert call(None, n_img, 3) == -1 and b"parameters" in lib.vssr_last_error(h)
    assert call(p, None, 3) == -1 and b"n_img" in lib.vssr_last_error(h)
    assert call(p, n_img, 0) == -1 and b"n_bands" in lib.vssr_last_error(h)
    assert call(p, [9, 7, 2], 3) == -1 and b">= 3" in lib.vssr_last_error(h)
    assert call(p, [9, 6], 2) == -1 and b"sum" in lib.vssr_last_error(h)
    assert call(p, [9, 6, 4], 3) == -1 and b"sum" in lib.vssr_last_error(h)
    for field, value, msg in (("method", 2, b"method"), ("method", -1, b"method"), ("climb", 2, b"climb"), ("climb", -1, b"climb")):
        q = params()
        setattr(q, field, value)
        assert call(q, n_img, 3) == -1 and msg in lib.vssr_last_error(h)
    _assert_equal(_neb(eng, structs, n_img, held, upload=False, **good), ref, "after the null / count refusals")
    # images that differ in more than positions: atom count, species, cell, pbc, fixed mask
    b6 = bands[1].band
    T, X, cell, pbc = b6[2]
    for other, msg in (((T[:3], X[:3], cell, pbc), "atom counts"), ((np.array([0, 0, 0, 1], np.int32), X, cell, pbc), "species"),
                       ((T, X, cell * (1.0 + 2.0 ** -40), pbc), "cell"), ((T, X, cell, np.array([0, 0, 1], np.uint8)), "pbc")):
        bad = [b6[0], b6[1], other, b6[3], b6[4], b6[5]]
        eng.upload(bad)
        with pytest.raises(backend.BackendError, match=r"vssr error -1: .*(images|image)"):
            eng.neb([6], fixed=None, **good)
        e, _, f = eng.evaluate_f64(bad)      # the handle serves the next call
        assert np.isfinite(e).all()
    eng.upload(b6)
    mask = np.tile(nc.ANCHOR_HELD, 6)
    mask[4 * 3] = 0
    with pytest.raises(backend.BackendError, match=r"vssr error -1: .*fixed mask"):
        eng.neb([6], fixed=mask, **good)
    _assert_equal(_neb(eng, structs, n_img, held, **good), ref, "after the image refusals")
    fresh = rc.engine("pair_lj")
    with pytest.raises(backend.BackendError, match="vssr error -5"):
        fresh.neb([3])
    fresh.close()
    eng.close()
