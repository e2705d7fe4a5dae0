"""Inputs of tests/test_cg_resident_kinds_gpu.py (test infrastructure): for every kind of fp64 handle the chain-resident CG minimiser
serves besides Tersoff -- Stillinger-Weber, EAM funcfl (the untyped bodies), EAM alloy and fs (the typed bodies), pair lj/cut and
pair hybrid/overlay born + coul/dsf with charges -- an engine and the batches of the test's seven properties.  Structures are
``(types, positions, cell, pbc)``; a batch is ``(structures, held mask [sum N] uint8)``.

Generic chains are jittered grids (``pair_cases.grid_chain``) at a spacing near the kind's nearest-neighbor distance; the cells of
``cell_cases`` are scaled to that distance, which keeps what they are there for (the skewed basis, the open axis with a sheared
vector, the thin cell whose neighbors are its own images)."""
import os

import numpy as np

import cell_cases as cl
import cg_cases as cc
import eam_alloy_oracle as ao
import pair_cases as pc
import pair_oracle as po
import sw_oracle as so
from conftest import GOLDEN

KINDS = ("sw", "eam_funcfl", "eam_alloy", "eam_fs", "pair_lj", "pair_born_dsf")
# (types in use, grid spacing / nearest-neighbor distance in A, largest cutoff in A)
SHAPE = {"sw": (1, 2.5, None), "eam_funcfl": (1, 2.6, 4.95), "eam_alloy": (2, 2.7, None), "eam_fs": (2, 2.7, None),
         "pair_lj": (2, 2.9, 8.0), "pair_born_dsf": (2, 2.82, 12.0)}
SIZES = (1, 63, 64, 65, 255, 256)


def _funcfl():
    from surface_sampling_amd import eam

    return eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), eam.read_funcfl(os.path.join(GOLDEN, "Au_u3.eam"))


def eam_tables(kind):
    """EamTables of "eam_alloy" / "eam_fs" through the file readers (tests/test_eam_alloy_gpu.py::_forms)."""
    from surface_sampling_amd import eam

    cu, au = _funcfl()
    if kind == "eam_alloy":
        return eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au))), ["Cu", "Au"])
    return eam.tables_from_setfl(eam.parse_setfl(eam.write_setfl(ao.cuau_setfl(cu, au, (0.7, 1.3))), fs=True), ["Cu", "Au"])


def born_dsf_model():
    from surface_sampling_amd import pair

    return pair.parse(po.ROCKSALT_COMMANDS, 2)


def engine(kind):
    from surface_sampling_amd import backend

    if kind == "sw":
        return backend.SWEngine(so.si_params(), device=0)
    if kind == "eam_funcfl":
        return backend.EAMEngine(_funcfl()[0], device=0)
    if kind in ("eam_alloy", "eam_fs"):
        return backend.EAMEngine(eam_tables(kind), device=0)
    if kind == "pair_lj":
        return backend.PairEngine(cc.LJ_TERMS, n_types=cc.LJ_NTYPES, device=0)
    return backend.PairEngine(born_dsf_model(), device=0)


def cutoff(kind):
    rc = SHAPE[kind][2]
    if rc is not None:
        return rc
    return so.cutoff(so.si_params()) if kind == "sw" else float(eam_tables(kind).cutoff)


def grid(kind, n, seed, pbc, jitter=0.15):
    nt, spacing, _ = SHAPE[kind]
    return pc.grid_chain(n, seed, pbc, n_types=nt, spacing=spacing, jitter=jitter)


def held_first_two(structs):
    return pc.held_mask(structs)


def one_atom():
    return np.zeros(1, np.int32), np.array([[15.0, 15.0, 15.0]]), np.eye(3) * 30.0, np.zeros(3, np.uint8)


# ---- 1: ragged batches whose chains stop at different evaluation counts, rows within the default 64 slots per atom --------------------
def _si_slabs(sigmas, seed=8):
    Z, X, Cl, pbc, fixed = so.si_slab()
    rng = np.random.default_rng(seed)
    T = np.zeros(len(Z), np.int32)
    return [(T, X + np.where(fixed[:, None], 0.0, rng.normal(0, s, X.shape)), Cl, pbc.astype(np.uint8)) for s in sigmas], fixed.astype(np.uint8)


def _cu_chains(nt, n_chains=4):
    """The Cu(100) toy with two adatoms (tests/test_eam_alloy_gpu.py::_relax_case), the four slab atoms held."""
    d = np.load(os.path.join(GOLDEN, "cu100.npz"))
    out = []
    for k in range(n_chains):
        sub = [(2 + 3 * k) % len(d["ads_coords"]), (9 + 5 * k) % len(d["ads_coords"])]
        pos = np.vstack([d["positions"], d["ads_coords"][sub]]) + np.random.default_rng(k).normal(0, 0.03 + 0.02 * k, (10, 3))
        t = np.array([0, 1, 0, 0, 1, 0, 0, 0, 1, k % 2], np.int32) % nt
        out.append((t, pos, d["cell"], d["pbc"].astype(np.uint8)))
    return out, [np.array([1] * 4 + [0] * 6, np.uint8)] * n_chains


def ragged(kind, golden):
    """(structures, mask, max_iter): chains of different sizes and distances from their minima, held atoms, a one-atom chain that
    stops behind its first evaluation."""
    nt = SHAPE[kind][0]
    if kind == "sw":
        slabs, fixed = _si_slabs((0.02, 0.08, 0.2))
        box = so.dense_box(n=30, box=9.0, min_dist=2.1, seed=9)
        small = grid(kind, 16, 71, [1, 1, 0])
        structs = slabs + [box, small, one_atom()]
        mask = [fixed] * 3 + [np.zeros(30, np.uint8), (np.arange(16) < 2).astype(np.uint8), np.zeros(1, np.uint8)]
        return structs, np.concatenate(mask), 30
    if kind.startswith("eam"):
        chains, masks = _cu_chains(nt)
        pos, cell, pbc = ao.cu100_slab(3, 3, 4)
        pos = pos + np.random.default_rng(5).normal(0, 0.06, pos.shape)
        T = ao.random_alloy(pos, 0.3, 2) % nt
        structs = chains + [(T.astype(np.int32), pos, cell, np.asarray(pbc, np.uint8)), one_atom()]
        mask = masks + [(pos[:, 2] < pos[:, 2].min() + 0.5).astype(np.uint8), np.zeros(1, np.uint8)]
        return structs, np.concatenate(mask), 60
    if kind == "pair_lj":
        params, cases = cc.batches("pair", "exact", golden)[0]
        assert cc._key(params) == cc._key(cc.DEFAULTS)
        structs, mask = cc.pack(cases)
        return structs, mask, params["max_iter"]
    T, X, C = po.rocksalt(5.64)
    rng = np.random.default_rng(21)
    cube = (T, X + rng.normal(0, 0.08, X.shape), np.eye(3) * 30.0, np.zeros(3, np.uint8))     # an open 8-atom cluster
    structs = [grid(kind, n, seed, [0, 0, 0], jitter=j) for n, seed, j in ((7, 40, 0.1), (16, 41, 0.15), (23, 42, 0.2))] + [cube, one_atom()]
    return structs, held_first_two(structs), 30


# ---- 2: the tile limits -----------------------------------------------------------------------------------------------------------------
def size_batch(kind, with_257=False):
    """Chains of 1, 63, 64, 65, 255 and 256 atoms (with_257: one more of 257), periodic in x and y, the first two atoms held."""
    structs = [grid(kind, n, 30 + k, [1, 1, 0]) for k, n in enumerate(SIZES + ((257,) if with_257 else ()))]
    return structs, held_first_two(structs)


# ---- 3: row lengths -----------------------------------------------------------------------------------------------------------------------
def sw_crowded():
    """The Si(111) slab under a close-packed pile of 19 adatoms (an fcc fragment of two neighbor shells, 2.4 A apart, rattled, its
    lowest atom 1.6 A above the surface): the pile's centre has 18 slots, more than SW_MAXD = 16.  And the dense box of
    tests/test_sw_gpu.py.  Each chain holds centres beyond and within the tile (asserted by the caller)."""
    Z, X, Cl, pbc, fixed = so.si_slab()
    a = 2.4 * np.sqrt(2.0)
    frac = [(i + bx, j + by, k + bz) for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3)
            for bx, by, bz in ((0, 0, 0), (0, .5, .5), (.5, 0, .5), (.5, .5, 0))]
    pile = np.array([p for p in np.array(frac, float) * a if np.linalg.norm(p) <= a + 1e-9])
    assert len(pile) == 19
    centre = 0.5 * (Cl[0] + Cl[1])
    centre[2] = X[:, 2].max() + 5.0
    ads = pile + centre + np.random.default_rng(17).normal(0, 0.05, pile.shape)
    pos = np.vstack([X, ads])
    slab = (np.zeros(len(pos), np.int32), pos, Cl, pbc.astype(np.uint8))
    structs = [slab, so.dense_box()]
    mask = np.concatenate([fixed.astype(np.uint8), np.zeros(len(ads), np.uint8), np.zeros(len(structs[1][0]), np.uint8)])
    return structs, mask


def rocksalt_long_rows():
    """The rattled 8-atom rocksalt cube under the 12 A cutoff of born + coul/dsf: every row holds more than 300 slots over several
    images of the cell (tests/test_pair_gpu_relax.py), next to a short open chain."""
    T, X, C = po.rocksalt(5.64)
    rock = (T, X + np.random.default_rng(21).normal(0, 0.05, X.shape), C, np.ones(3, np.uint8))
    structs = [rock, grid("pair_born_dsf", 7, 40, [0, 0, 0], jitter=0.1)]
    return structs, held_first_two(structs)


# ---- 4: a different cell on every chain ---------------------------------------------------------------------------------------------------
CELL_NAMES = ("gan_slab_skewed", "sto_slab_open_c_plus_a", "gan_wurtzite_rattled", "cu_fcc_primitive_rattled2")


def cell_batch(kind):
    """A skewed slab cell, a partly periodic cell whose open vector is sheared, and two thin cells whose neighbors are their own images
    (one of them beyond 64 images: the neighbor search without hit masks), scaled to the kind's nearest-neighbor distance."""
    nt, spacing, _ = SHAPE[kind]
    by = cl.by_name()
    structs = []
    for name in CELL_NAMES:
        c = by[name]
        _, _, _, rv = cl.brute_neighbors(c.pos, c.cell, c.pbc, 4.0)
        s = spacing / float(np.linalg.norm(rv, axis=1).min())
        structs.append(((np.arange(len(c)) % nt).astype(np.int32), c.pos * s, c.cell * s, c.pbc.astype(np.uint8)))
    return structs, held_first_two(structs)


# ---- 6: the 48-atom Tersoff batch of the automatic rule -------------------------------------------------------------------------------------
def gan48(golden, n_chains=4):
    cases = [cc._slab_with_adatoms(golden, 1, 12, 50 + k) for k in range(n_chains)]
    assert all(len(c.types) == 48 for c in cases)
    return cc.pack(cases)
