"""Inputs, episodes and schedules of tests/test_gpu_handle_reuse.py and their CPU rehearsal tests/test_handle_reuse_cpu.py (test
infrastructure).  The device test runs a long schedule of different driver calls on ONE handle per kind and compares every call with
the same call on a brand-new handle, bit for bit: a chain's bits depend neither on the rest of its batch, nor on the run, nor on the
neighbor capacity, so the fresh handle is an exact reference.

An EPISODE is ``upload(batch)`` followed by one to three calls on that resident batch; ``run_episode`` returns everything those calls
return as an ordered list of ``(name, array)``.  Episode types (``TYPES``):

    E   evaluate (energy, per-atom, forces) -> stress() -> neighbors()          Eo  energy-only run, then a forces run (last_want)
    F   relax_fire with a FixAtoms mask, record_interval = 2, the trajectory    B   relax_bfgs without mask and without recording
    Cl  CG lock-step, VSSR_CG_FUSED=0 VSSR_RELAX_COMPACT=2                       Cr  CG chain-resident, VSSR_CG_FUSED=1
    L   relax_bfgs_linesearch                                                   M   draw_velocities -> md Langevin -> md -> velocities
    Mr  M with driver="resident"                                                P   npt with a barostat -> get_cell()
    X   relax_cell -> get_cell()                                                V   vibrations with replicas
    N   neb                                                                     D   dimer
    K   debug_capacity(4, tight) then F (the run regrows)                       R   a refused upload and refused driver arguments

Sizes: ``S`` (small: two 8-atom periodic chains, every image grid <= 64 so the 64-bit hit masks are on; the structured drivers V / N / D
take an input with fewer atoms than that), ``G`` (large: a ragged batch of five chains, one in a cell so thin that its image grid exceeds
64 and the whole batch searches without hit masks; V / N / D: more atoms and more chains than S) and ``W`` (E only: more than 4096 atoms
in chains of <= 256, two scan tiles).  Every structure is ``(types or atomic numbers, positions, cell, pbc)``.

Generic chains are the jittered grids of ``pair_cases.grid_chain`` at the spacings the existing device tests of each kind use
(cg_resident_cases.SHAPE, cellrelax_cases.PARITY_SHAPE, dimer_cases.EXTRA_SHAPE); the S cells are widened to 1.08 x the cutoff / 2 where
the kind's spacing would need a second image.  The thin cell of G is a one-atom cell of one grid spacing (the shape of
cell_cases' ``si_simple_cubic`` / ``cu_fcc_primitive``: every neighbor is an own image); Ewald handles take the cells of
ewald_cases, PaiNN handles the SrTiO3 cells of cell_cases and the golden structures."""
import os
from collections import namedtuple

import numpy as np

import cell_cases as cl
import pair_cases as pc

FULL_KINDS = ("pair_lj", "tersoff")
REDUCED_KINDS = ("sw", "eam_alloy", "adp", "vashishta", "ewald", "pair_born_dsf")
PAINN_KINDS = ("painn", "painn_gen")
KINDS = FULL_KINDS + REDUCED_KINDS + PAINN_KINDS

SHARED = ("E", "Eo", "F", "B", "Cl", "Cr", "L", "M")          # the types that share d_opt_state / d_opt_vec / d_fixed / d_active
SPECIAL = ("P", "X", "V", "N", "D", "K", "R")                 # each directly before and after an F and an E in the full schedule
STRUCTURED = ("V", "N", "D")
TYPES = SHARED + ("Mr",) + SPECIAL

# the episode types the existing device tests of a kind already run on it (test_pair_gpu_relax / test_relax_gpu_branches /
# test_cg_resident_kinds_gpu / test_bfgsls_gpu / test_md_gpu / test_npt_gpu / test_cellrelax_gpu / test_vib_gpu / test_neb_gpu /
# test_dimer_gpu / test_adp_gpu / test_vashishta_gpu / test_ewald_gpu / test_gpu_painn_widths and the *_calculators_gpu files)
APPLICABLE = {
    "pair_lj": TYPES, "tersoff": TYPES,
    "sw": ("E", "Eo", "F", "B", "Cl", "Cr", "L", "M", "Mr", "P", "X", "V", "N", "D", "K", "R"),
    "eam_alloy": ("E", "Eo", "F", "B", "Cl", "Cr", "M", "Mr", "P", "X", "V", "N", "D", "K", "R"),
    "adp": ("E", "Eo", "F", "B", "Cl", "P", "X", "K", "R"),
    "vashishta": ("E", "Eo", "F", "B", "Cl", "L", "M", "P", "X", "V", "N", "D", "K", "R"),
    "ewald": ("E", "Eo", "F", "B", "Cl", "M", "V", "N", "D", "K", "R"),      # (P with a barostat and X are refusals there: part of R)
    "pair_born_dsf": ("E", "Eo", "F", "B", "Cl", "Cr", "M", "Mr", "P", "K", "R"),
    "painn": ("E", "Eo", "F", "B", "L", "M", "V", "N", "K", "R"),
    "painn_gen": ("E", "Eo", "F", "B", "L", "M", "V", "N", "K", "R"),
}

# (types in use, grid spacing in A) of the analytic kinds
SHAPE = {"pair_lj": (2, 2.9), "tersoff": (2, 1.95), "sw": (1, 2.5), "eam_alloy": (2, 2.7), "adp": (2, 2.7), "vashishta": (2, 1.9),
         "pair_born_dsf": (2, 2.82)}
G_SIZES = (1, 3, 8, 38, 66)
W_CHAINS, W_ATOMS = 17, 250
PAINN_GEN_SHAPE = (64, 16)
BIG_CHAIN_RANGE = (788, 1462)       # the chain sizes that take the multi-pass forward and reverse classes (csrc/painn_edge_mfma.hip)

Inputs = namedtuple("Inputs", "structs held mass extra")


# ---- engines, cutoffs ------------------------------------------------------------------------------------------------------------------
def _adp_tables():
    import adp_oracle as adp
    import cg_resident_cases as rc
    from surface_sampling_amd import eam

    return eam.tables_from_adp(eam.parse_adp(eam.write_adp(adp.cuau_adp(*rc._funcfl()))), ["Cu", "Au"])


def _ewald_model():
    import ewald_cases as ec
    from surface_sampling_amd import pair

    return pair.parse(ec.RAGGED_MODEL, 3)


def painn_blobs(kind, golden):
    """(weights, hparams or None) of the PaiNN kinds: the golden 128 / 20 ensemble, or its 64 / 16 reshaping (the general path)."""
    if kind == "painn":
        return golden.blobs, None
    from painn_shapes import reshape_ensemble

    return reshape_ensemble(golden.blobs, *PAINN_GEN_SHAPE)


def engine(kind, golden):
    """A brand-new handle of ``kind``."""
    import cg_resident_cases as rc
    from surface_sampling_amd import backend

    if kind in PAINN_KINDS:
        blobs, hp = painn_blobs(kind, golden)
        return backend.PainnEngine(blobs, device=0, hparams=hp)
    if kind == "tersoff":
        return backend.TersoffEngine(cl.gan_params(), device=0)
    if kind == "adp":
        return backend.EAMEngine(_adp_tables(), device=0)
    if kind == "vashishta":
        import vashishta_oracle as vo

        return backend.VashishtaEngine(vo.sic_params()[1], device=0)
    if kind == "ewald":
        return backend.PairEngine(_ewald_model(), device=0)
    return rc.engine(kind)


def cutoff(kind):
    """The cutoff the handle searches neighbors with (what decides the image grids)."""
    import cg_resident_cases as rc

    if kind in PAINN_KINDS:
        return cl.PAINN_RC
    if kind == "tersoff":
        return cl.tersoff_cutoff(cl.gan_params())
    if kind == "vashishta":
        import vashishta_oracle as vo

        return float(vo.cutoff(vo.sic_params()[1]))
    if kind == "adp":
        return float(rc.eam_tables("eam_alloy").cutoff)
    if kind == "ewald":
        return 8.0
    return float(rc.cutoff(kind))


def term_cutoffs(kind):
    """Every distance at which a term of the kind's potential switches on or off (the pairs of the inputs stay clear of them)."""
    if kind == "tersoff":
        P = cl.gan_params()
        return sorted(set(np.concatenate([(P[..., 10] + P[..., 11]).ravel(), (P[..., 10] - P[..., 11]).ravel()]).tolist()))
    if kind == "pair_born_dsf":
        import cg_resident_cases as rc

        return sorted({float(t.rc) for t in rc.born_dsf_model().terms})
    if kind == "vashishta":
        import vashishta_oracle as vo

        P = vo.sic_params()[1]
        return sorted(x for x in set(P[..., 8].ravel().tolist() + P[..., 11].ravel().tolist()) if x > 0)      # rc and r0 of every entry
    return [cutoff(kind)]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
W_MARGIN = 1e-5


def cutoff_margin(kind, struct):
    """The smallest | d / rc - 1 | over the pairs of a structure and the switching distances of the kind."""
    cuts = term_cutoffs(kind)
    _, _, _, rv = cl.brute_neighbors(struct[1], struct[2], struct[3], max(cuts) * 1.01)
    d = np.linalg.norm(rv, axis=1)
    return min(float(np.abs(d / rc - 1.0).min()) for rc in cuts) if len(d) else np.inf


def image_grid(struct, rc):
    return cl.n_images(cl.face_nimg(struct[2], np.asarray(struct[3], bool), rc))


def _s_spacing(kind):
    """The kind's grid spacing, widened until the 2 x 2 x 2 cell of 8 atoms is higher than the cutoff along every axis."""
    _, spacing = SHAPE[kind]
    return max(spacing, 1.08 * cutoff(kind) / 2.0)


def _rattled(struct, sigma, seed):
    T, X, C, pbc = struct
    return T, X + np.random.default_rng(seed).normal(0.0, sigma, X.shape), C, pbc


def _thin_one_atom(kind):
    """One atom in a periodic, slightly skewed cell of one grid spacing: every neighbor is an image of the atom itself."""
    _, spacing = SHAPE[kind]
    cell = np.eye(3) * spacing + np.array([[0, 0, 0], [0.05, 0, 0], [0.03, -0.04, 0]])
    return np.zeros(1, np.int32), np.array([[0.3, -0.2, 0.1]]), cell, np.ones(3, np.uint8)


def _generic(kind, size, periodic):
    nt, spacing = SHAPE[kind]
    if size == "S":
        a = pc.grid_chain(8, 11, [1, 1, 1], n_types=nt, spacing=_s_spacing(kind), jitter=0.15)
        return [a, _rattled(a, 0.05, 3)]
    if size == "W":       # (among ~1e5 pairs one lands within 1e-6 of a cutoff now and then: such seeds are passed over)
        out, seed = [], 300
        while len(out) < W_CHAINS:
            c = pc.grid_chain(W_ATOMS, seed, [1, 1, 0], n_types=nt, spacing=spacing, jitter=0.1)
            if cutoff_margin(kind, c) > W_MARGIN:
                out.append(c)
            seed += 1
        return out
    pbcs = [[1, 1, 1]] * 5 if periodic else [None, [0, 0, 0], [1, 1, 1], [1, 1, 0], [1, 1, 1]]
    out = [_thin_one_atom(kind)]
    for k, (n, pbc) in enumerate(zip(G_SIZES[1:], pbcs[1:])):
        # (the 8-atom chain at the S spacing; the larger ones at the kind's own: three and more cells per axis)
        out.append(pc.grid_chain(n, 20 + k, pbc, n_types=nt, spacing=_s_spacing(kind) if n == 8 else spacing, jitter=0.12))
    return out


def _ewald(size):
    import ewald_cases as ec
    import pair_oracle as po

    if size == "S":
        T, X, C = po.rocksalt(8.7)       # 8 ions in a cell higher than the 8 A cutoff
        a = (T, X, C, ec.PBC)
        return [_rattled(a, 0.05, 35), _rattled(a, 0.08, 36)]
    return [ec.small(), ec.skewed(), ec.thin(), ec.rattled_cube(), ec.rattled64()]


def _painn_structs(golden):
    by = cl.by_name()
    slab = golden.structure("SrTiO3_2x2_pristine")
    return by, slab


def _arr(s):
    return (np.asarray(s.numbers, np.int32), np.asarray(s.positions, float), np.asarray(s.cell, float), np.asarray(s.pbc).astype(np.uint8))


def _painn(size, golden):
    from surface_sampling_amd import structures

    by, slab = _painn_structs(golden)
    if size == "S":
        a = _arr(slab)
        return [a, _rattled(a, 0.03, 4)]
    return [by["sto_bulk"].arrays(), by["tri_FFF"].arrays(), by["sto_221_rattled"].arrays(), _rattled(_arr(slab), 0.02, 6),
            _arr(structures.synth_chain(slab, 0))]


PAINN_SPECIES9 = (38, 22, 8, 31, 7, 14, 29, 13, 12)


def painn_extra(name, golden):
    """The E-only batches that flip what upload decides on the 128 / 20 handle."""
    by, slab = _painn_structs(golden)
    Z, X, C, pbc = by["sto_221_rattled"].arrays()
    if name == "big960":
        return [_arr(slab.repeat((4, 4, 1)))]
    if name == "sp1":
        return [(np.full(len(Z), 8, np.int32), X, C, pbc)]
    if name == "sp2":
        return [(np.where(Z == 38, 22, Z).astype(np.int32), X, C, pbc), _rattled((np.where(Z == 38, 22, Z).astype(np.int32), X, C, pbc), 0.02, 8)]
    if name == "sp9":
        return [(np.asarray(PAINN_SPECIES9, np.int32)[np.arange(len(Z)) % 9], X, C, pbc)]
    raise ValueError(name)


PAINN_EXTRA = ("big960", "sp1", "sp2", "sp9")
# on the 128 / 20 handle, behind the shuffled schedule: the 960-atom chain directly followed by S; then 2 species, 9 species, the
# 3-species slab and 1 species, each directly followed by the previous kind of batch
PAINN_TAIL = (("E", "big960"), ("E", "S"), ("E", "sp2"), ("E", "S"), ("E", "sp9"), ("E", "sp2"), ("E", "S"), ("E", "sp9"), ("E", "sp1"),
              ("E", "S"))


def _masses(kind, structs):
    if kind in PAINN_KINDS:
        from surface_sampling_amd import structures

        return np.concatenate([structures.ATOMIC_MASSES[np.asarray(s[0], np.int64)] for s in structs])
    import vib_cases as vc

    return vc.masses(structs)


def _band(a, b, n):
    """n images from a to b (structures that differ in positions only), linear in the positions."""
    return [(a[0], a[1] + (b[1] - a[1]) * k / (n - 1), a[2], a[3]) for k in range(n)]


def _structured(kind, etype, size, golden):
    """(structures, extra) of V / N / D: small = fewer atoms than S, large = more atoms and more chains than S."""
    small = size == "S"
    if kind in PAINN_KINDS:
        by, slab = _painn_structs(golden)
        a, b = by["sto_bulk"].arrays(), by["sto_221_rattled"].arrays()
        c = _arr(slab)
        if etype == "V":
            bases, reps = ([a], [2]) if small else ([c, b], [2, 3])
        else:
            base, n = (b, 3) if small else (c, 5)
            return _band(base, _rattled(base, 0.05, 9), n), {"n_img": [n]}
    elif kind == "ewald":
        import ewald_cases as ec

        a, b, c = ec.small(), ec.rattled_cube(), ec.thin()
        if etype == "V":
            bases, reps = ([a], [2]) if small else ([b, c], [3, 2])
        elif etype == "N":
            base, n = (a, 3) if small else (c, 5)
            return _band(base, _rattled(base, 0.05, 9), n), {"n_img": [n]}
        else:
            bases, reps = ([a], [2]) if small else ([c, b], [2, 2])
    else:
        nt, spacing = SHAPE[kind]
        grid = lambda n, seed, pbc: pc.grid_chain(n, seed, pbc, n_types=nt, spacing=spacing, jitter=0.05)     # noqa: E731
        if etype == "V":
            bases, reps = ([grid(3, 41, [0, 0, 0])], [2]) if small else ([grid(12, 42, [1, 1, 0]), grid(5, 43, [0, 0, 0])], [3, 2])
        elif etype == "N":
            base, n = (grid(4, 44, [0, 0, 0]), 3) if small else (grid(12, 45, [1, 1, 0]), 5)
            return _band(base, _rattled(base, 0.05, 9), n), {"n_img": [n]}
        else:
            bases, reps = ([grid(3, 46, [0, 0, 0])], [2]) if small else ([grid(12, 47, [1, 1, 0]), grid(9, 48, [0, 0, 0])], [2, 2])
    structs = [s for s, n in zip(bases, reps) for _ in range(n)]
    return structs, ({"n_rep": list(reps)} if etype == "V" else {})


_INPUTS = {}


def inputs(kind, etype, size, golden=None):
    """The inputs of an episode: cached, so that the long-lived handle and the fresh one see the same arrays."""
    key = (kind, "generic" if etype not in STRUCTURED + ("P", "X") else etype, size)
    if key in _INPUTS:
        return _INPUTS[key]
    extra = {}
    base_kind = "painn" if kind in PAINN_KINDS else kind
    if size in PAINN_EXTRA:
        structs = painn_extra(size, golden)
    elif etype in STRUCTURED:
        structs, extra = _structured(kind, etype, size, golden)
    elif base_kind == "painn":
        structs = _painn(size, golden)
    elif kind == "ewald":
        structs = _ewald(size)
    else:
        structs = _generic(kind, size, periodic=etype in ("P", "X"))
    # the first two atoms of every chain of three and more are held (a one-atom chain with its atom held would never be stepped)
    held = np.concatenate([(np.arange(len(s[0])) < 2) & (len(s[0]) >= 3) for s in structs]).astype(np.uint8)
    out = Inputs(structs, held, _masses(kind, structs), extra)
    _INPUTS[key] = out
    return out


def totals(inp):
    return sum(len(s[0]) for s in inp.structs), len(inp.structs)


# ---- the parameters of every call (constructed through the front end's own constructors) -----------------------------------------------
FIRE = dict(max_steps=6, fmax=1e-4)
BFGS = dict(max_steps=6, fmax=1e-4)
# (on the ragged batches the restatement tests/cg_oracle.py stops the one-atom chain at its first evaluation, the three-atom chain after
# 10 .. 26 and the others at max_iter, 32 .. 65 evaluations: chains leave at different polls of the driver, which polls every 8)
CG = dict(max_iter=30, max_eval=300, etol=1e-4, ftol=1e-2, dmax=0.1)
BFGSLS = dict(max_steps=4, fmax=1e-4)
MD = dict(steps=5, timestep=1.0, thermostat="langevin", temperature=300.0, friction=0.02, thermo_interval=2, seed=5)
NPT = dict(steps=5, timestep=1.0, thermostat="berendsen", barostat="berendsen", temperature=300.0, taut=20.0, taup=20.0,
           compressibility=0.1, pressure=0.01, thermo_interval=2, seed=5)
CELL = dict(max_steps=6, fmax=1e-4)
VIB = dict(delta=0.01, nfree=2, method="standard", temperature=300.0)
NEB = dict(max_steps=6, fmax=1e-4, k=0.1, climb=True, method="improvedtangent")
DIMER = dict(max_steps=5, max_rot_first=3, max_rot=1, fmax=1e-4, seed=7)
RECORD_INTERVAL = 2
TIGHT = dict(slots_per_atom=4, tight=1)


def c_params(backend):
    """Every parameter set above through the ``*Params`` constructors of the front end: {name: ctypes struct}."""
    return {"fire": backend.FireParams.default(**FIRE), "bfgs": backend.BfgsParams.default(**BFGS), "cg": backend.CgParams.default(**CG),
            "bfgsls": backend.BfgsLsParams.default(**BFGSLS),
            "npt": backend.npt_params(**NPT), "cell": backend.CellRelaxParams.default(**CELL),
            "neb": backend.NebParams.default(**{k: NEB[k] for k in ("max_steps", "method", "climb", "k", "fmax")}),
            "dimer": backend.DimerParams.default(**DIMER),
            "vib": backend.VibParams(VIB["nfree"], backend.vib_method_code(VIB["method"]), VIB["delta"], VIB["temperature"], 0.0),
            "md": backend.MdParams(MD["steps"], backend.md_thermostat_code(MD["thermostat"]), MD["thermo_interval"], MD["timestep"],
                                   MD["temperature"], MD["temperature"], MD["friction"], 0, 0, MD["seed"])}


# ---- episodes --------------------------------------------------------------------------------------------------------------------------
WANT_EF = 1 | 2 | 16          # energy, forces, per-atom energies (backend.WANT_ENERGY | WANT_FORCES | WANT_PER_ATOM)


class Env:
    """Environment variables for the length of one call (the CG knobs are read per call)."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _flat(prefix, d, out):
    for k, v in d.items():
        if isinstance(v, dict):
            _flat(f"{prefix}{k}.", v, out)
        elif isinstance(v, (list, tuple)):
            for i, a in enumerate(v):
                out.append((f"{prefix}{k}[{i}]", np.asarray(a)))
        else:
            out.append((prefix + k, np.asarray(v)))


def blank_unused_records(traj, structs):
    """The entries of chain b beyond n_records[b] are unused by contract (backend.relax_fire): the ring is not cleared between calls,
    so they are set to zero before the bytes are compared."""
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])])
    for b, n in enumerate(traj["n_records"]):
        traj["positions"][n:, start[b]:start[b + 1]] = 0.0
        traj["forces"][n:, start[b]:start[b + 1]] = 0.0
        traj["energies"][n:, b] = 0.0


def _refusal(fn):
    """The error a refused call raises, as bytes (code and message)."""
    from surface_sampling_amd import backend

    try:
        fn()
    except backend.BackendError as exc:
        return np.frombuffer(str(exc).encode(), np.uint8)
    raise AssertionError("the call was not refused")


def _state(eng, painn, out, tag=""):
    """What the last call left on the device: results, and -- where the graph is complete -- stress."""
    if painn:
        _flat(tag + "download.", {k: v for k, v in eng.download().items() if k != "cfg_start"}, out)
    else:
        e, ea, f = eng.results_f64()
        out += [(tag + "e", e), (tag + "ea", ea), (tag + "f", f)]


def run_episode(eng, kind, etype, inp):
    """Upload ``inp`` to ``eng`` and run the calls of episode type ``etype``: [(output name, array)].  ``relax_counts()`` and the regrow
    count depend on the handle's history by design: they go to stdout, not into the result."""
    from surface_sampling_amd import backend

    painn = kind in PAINN_KINDS
    structs, held, mass = inp.structs, inp.held, inp.mass
    out = []
    if etype == "R":
        x = structs[0]
        thin = (x[0], x[1], np.diag([6.0, 6.0, 0.01]), np.ones(3, np.uint8))
        out.append(("refused upload", _refusal(lambda: eng.upload([structs[0], thin]))))
        eng.upload(structs)
        out.append(("refused vibrations nfree=3", _refusal(lambda: eng.vibrations(mass, nfree=3))))
        out.append(("refused vibrations delta=0", _refusal(lambda: eng.vibrations(mass, delta=0.0))))
        if kind == "ewald":
            eng.set_velocities(None)
            out.append(("refused npt barostat", _refusal(lambda: eng.npt(mass, **NPT))))
            out.append(("refused relax_cell", _refusal(lambda: eng.relax_cell(**CELL))))
        return out
    if etype in ("E", "Eo"):
        eng.upload(structs)
        if etype == "Eo":
            want = backend.WANT_ENERGY | ((backend.WANT_STD | backend.WANT_PER_MODEL) if painn else 0)
            eng.run(want)
            _flat("energy-only.", {k: v for k, v in eng.download(want).items() if k.startswith("energy") or k == "saturated"}, out)
        eng.run(backend.WANT_ALL if painn else WANT_EF)
        _state(eng, painn, out)
        if painn:
            out += [("embedding", eng.embedding()), ("saturated", eng.saturated())]
        st, sd = eng.stress()
        out += [("stress", st), ("stress_std", sd)]
        if etype == "E":
            out += list(zip(("nbr.i", "nbr.j", "nbr.S", "nbr.r"), eng.neighbors()))
            out.append(("stats", np.array(list(eng.stats().values()), np.int64)))
        return out
    if etype in ("Cl", "Cr"):
        env = dict(VSSR_CG_FUSED="0", VSSR_RELAX_COMPACT="2") if etype == "Cl" else dict(VSSR_CG_FUSED="1")
        with Env(**env):
            res = eng.relax_cg_f64(structs, fixed=held, rerun=False, driver="lockstep" if etype == "Cl" else "resident", **CG)
        print(f"    {etype}: driver {eng.last_cg_driver}, counts {eng.last_relax_counts}, n_iter {res[4].tolist()}, stop {res[6].tolist()}")
        return list(zip(("e", "ea", "f", "positions", "n_iter", "n_eval", "stop_reason"), res))
    eng.upload(structs)
    if etype == "K":
        eng.debug_capacity(**TIGHT)
    if etype in ("F", "K"):
        res = eng.relax_fire(fixed=held, record_interval=RECORD_INTERVAL, **FIRE)
        blank_unused_records(res["traj"], structs)
        _flat("", res, out)
        if etype == "K":
            n = eng.debug_capacity()
            print(f"    K: {n} regrows")
            assert n >= 1, "the tight pool did not regrow"
    elif etype == "B":
        _flat("", eng.relax_bfgs(**BFGS), out)
    elif etype == "L":
        _flat("", eng.relax_bfgs_linesearch(fixed=held, **BFGSLS), out)
    elif etype in ("M", "Mr"):
        ids = np.arange(len(structs), dtype=np.uint64) + 3
        eng.draw_velocities(mass, MD["temperature"], seed=MD["seed"], fixed=held, chain_id=ids)
        out.append(("v0", eng.get_velocities()))
        kw = dict(MD, fixed=held, chain_id=ids, driver="resident" if etype == "Mr" else "lockstep")
        _flat("md1.", eng.md(mass, **kw), out)
        _flat("md2.", eng.md(mass, step0=MD["steps"], **kw), out)
        out.append(("velocities", eng.get_velocities()))
        print(f"    {etype}: driver {eng.last_md_driver}")
    elif etype == "P":
        eng.draw_velocities(mass, NPT["temperature"], seed=NPT["seed"], fixed=held)
        _flat("", eng.npt(mass, fixed=held, **NPT), out)
        out.append(("get_cell", eng.get_cell()))
    elif etype == "X":
        _flat("", eng.relax_cell(fixed=held, **CELL), out)
        out.append(("get_cell", eng.get_cell()))
    elif etype == "V":
        _flat("", eng.vibrations(mass, vib=held, n_rep=inp.extra["n_rep"], return_hessian=True, return_modes=True, **VIB), out)
    elif etype == "N":
        _flat("", eng.neb(inp.extra["n_img"], fixed=held, **NEB), out)
    elif etype == "D":
        _flat("", eng.dimer(fixed=held, **DIMER), out)
    else:
        raise ValueError(etype)
    print(f"    {etype}: counts {eng.relax_counts()}, regrows {eng.debug_capacity()}")
    _state(eng, painn, out, "after.")      # (every chain's last evaluation: served whether or not the graph is complete)
    return out


def first_difference(got, ref, inp):
    """None, or (output name, what differs, first differing chain or None)."""
    if [n for n, _ in got] != [n for n, _ in ref]:
        return "(the list of outputs)", f"{[n for n, _ in got]} != {[n for n, _ in ref]}", None
    N, B = totals(inp)
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in inp.structs])])
    for (name, a), (_, b) in zip(got, ref):
        if a.dtype != b.dtype or a.shape != b.shape:
            return name, f"{a.dtype}{a.shape} != {b.dtype}{b.shape}", None
        if a.tobytes() == b.tobytes():
            continue
        chain = None
        for axis in range(min(a.ndim, 2)):
            if a.shape[axis] in (N, B) and (N != B or axis == 0):
                rows = np.moveaxis(a, axis, 0).reshape(a.shape[axis], -1)
                ref_rows = np.moveaxis(b, axis, 0).reshape(a.shape[axis], -1)
                bad = np.nonzero([x.tobytes() != y.tobytes() for x, y in zip(rows, ref_rows)])[0]
                if len(bad):
                    chain = int(bad[0]) if a.shape[axis] == B else int(np.searchsorted(start, bad[0], side="right") - 1)
                    break
        return name, "bytes differ", chain
    return None


# ---- schedules -------------------------------------------------------------------------------------------------------------------------
def euler_walk(nodes):
    """A closed walk over ``nodes`` that uses every ordered pair (a, b), a == b included, exactly once (Hierholzer on the complete
    digraph with loops): len(nodes)^2 + 1 entries."""
    left = {a: list(reversed(nodes)) for a in nodes}
    stack, walk = [nodes[0]], []
    while stack:
        a = stack[-1]
        if left[a]:
            stack.append(left[a].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def full_schedule(kind):
    """[(episode type, size)]: the Eulerian walk over SHARED; at the F nearest to a third of it the block F Z E E Z F for every Z of
    SPECIAL (K first: the rest of the schedule runs on the tight pool); sizes alternate S, G, ...; behind it W, E(S), W, F(S)."""
    walk = euler_walk(list(SHARED))
    at = min((i for i, t in enumerate(walk) if t == "F"), key=lambda i: abs(i - len(walk) // 3))
    block = []
    for z in ("K",) + tuple(t for t in SPECIAL if t != "K") + ("Mr",):      # (Mr, the resident MD kernel, rides in the same way)
        block += [z, "E", "E", z, "F"]
    types = walk[:at + 1] + block + walk[at + 1:]
    types = [t for t in types if t in APPLICABLE[kind]]
    first = "S" if len(types) % 2 == 1 else "G"          # (the walk ends on a small batch: W follows a smaller one)
    other = {"S": "G", "G": "S"}
    sched, size = [], first
    for t in types:
        sched.append((t, size))
        size = other[size]
    return sched + [("E", "W"), ("E", "S"), ("E", "W"), ("F", "S")]


def reduced_schedule(kind, seed=38):
    """Every applicable type in both sizes, sizes alternating, in an order fixed by a seeded shuffle, K somewhere in the first half."""
    rng = np.random.default_rng(seed)
    types = list(APPLICABLE[kind])
    a, b = list(rng.permutation(types)), list(rng.permutation(types))
    sched = [x for pair in zip([(t, "S") for t in a], [(t, "G") for t in b]) for x in pair]
    half = len(sched) // 2
    if not any(t == "K" for t, _ in sched[:half]):
        i = next(i for i, (t, s) in enumerate(sched) if t == "K")
        j = i % 2          # the first slot of the same size
        sched[i], sched[j] = sched[j], sched[i]
    if kind == "painn":
        sched += list(PAINN_TAIL)
    return sched


def schedule(kind):
    return full_schedule(kind) if kind in FULL_KINDS else reduced_schedule(kind)


def size_class(size):
    return "small" if size in ("S", "sp1", "sp2", "sp9") else "large"
