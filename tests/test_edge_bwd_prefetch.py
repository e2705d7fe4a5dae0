"""GPU (-m gpu): the bundle walk of the reverse neighbor-sum kernel (painn_edge_mfma.hip, k_edge_bwd_mfma) at the shapes where its
switch from one bundle to the next can go wrong.

The kernel keeps the current centre's record (phi_c, v_c) in registers; at a bundle switch the record of the next bundle, in flight since
the previous switch, is moved in and the one after it is requested, next to the bundle-table entry of the bundle after next.  What these
cases exercise: a wave that owns several consecutive 2-step bundles (every switch follows the previous one at the minimum distance, so
the values it moves were requested two steps earlier), a wave without any bundle, long bundles followed by 2-step ones in one wave (with
per-wave step totals of every residue modulo 3, the period of a three-deep table ring), masked evaluations, the rerun after a capacity
overflow, and the other instantiations (8-wave launches, narrower slices, the multi-pass form) under the knob sets of tools/dump_painn.py.

A launch takes the 4-wave form the benchmark runs only with more than 256 workgroups, i.e. more than 10 chains of the class: the first
three cases batch 12 small chains.  Every case is held against the fp64 oracle at the tolerances of tests/test_edge_fwd_persistent.py."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_TOL = 1e-4      # eV, GPU fp32 vs fp64 oracle        (tests/test_edge_fwd_persistent.py, tests/test_gpu_parity.py)
F_TOL = 2e-4      # eV/A
STD_TOL = 2e-4
CUTOFF = 5.0
NW = 4            # waves of the workgroup form under test


def _arrays(s):
    return (s.numbers, s.positions, s.cell, s.pbc)


def _engine(golden, monkeypatch=None, knobs=None):
    from surface_sampling_amd import backend

    table, const = golden.offset_table()
    knobs = knobs or {}
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    try:
        return backend.PainnEngine(golden.blobs, device=0, offset_per_z=table, offset_const=const)
    finally:
        for k in knobs:
            monkeypatch.delenv(k)


def _oracle(golden, oracle_mod, s):
    table, const = golden.offset_table()
    return oracle_mod.ensemble(golden.blobs, s.numbers, s.positions, s.cell, s.pbc, 64, table, const)


def _against_oracle(res, chains, refs, which=None):
    for b, s in enumerate(chains):
        if which is not None and b not in which:
            continue
        a0, a1 = res["cfg_start"][b], res["cfg_start"][b + 1]
        ref = refs[b]
        de, df = abs(float(res["energy"][b]) - ref["energy"]), np.abs(res["forces"][a0:a1] - ref["forces"]).max()
        print(f"chain {b} ({len(s)} atoms): |dE| {de:.2e} eV  max|dF| {df:.2e} eV/A")
        assert de <= E_TOL and df <= F_TOL, (b, len(s), de, df)
        assert abs(float(res["energy_std"][b]) - ref["energy_std"]) <= STD_TOL
        assert np.abs(res["forces_std"][a0:a1] - ref["forces_std"]).max() <= STD_TOL


def _neighbor_counts(oracle_mod, s):
    i = oracle_mod.neighbors(s.positions, s.cell, s.pbc, CUTOFF)[0]
    return np.bincount(i, minlength=len(s))


def _wave_steps(counts, nw=NW):
    """The bundle deal on the CPU (profiles/r33/bundle_balance.py): rows padded to 4 slots with a minimum of 8, centres sorted by padded
    slot count (descending), bundles of 4, steps = slots of the longest / 4, snake deal.  Returns (steps per bundle, list of the step
    sequences of the nw waves)."""
    slots = np.maximum((counts + 3) // 4 * 4, 8)
    order = np.sort(slots)[::-1]
    steps = [max(int(order[4 * b]) // 4, 2) for b in range((len(counts) + 3) // 4)]
    waves = [[] for _ in range(nw)]
    for b, st in enumerate(steps):
        jj, r = divmod(b, nw)
        waves[nw - 1 - r if jj & 1 else r].append(st)
    return steps, waves


def _four_wave_form(chains):
    """More than 256 workgroups (chains x 8 slices x 3 models) and two tiles per CU: launch_edge_bwd_mfma takes 4-wave workgroups."""
    return len(chains) * 8 * 3 > 256 and max(len(c) for c in chains) <= 301


@pytest.fixture(scope="module")
def slab(golden):
    return golden.structure("SrTiO3_2x2_pristine")


def _sparse(slab, n, seed):
    """n atoms with the slab's species on a simple cubic lattice of 3.7 A (4 x 4 x 3 sites, periodic in the plane): 6 neighbors at most
    inside 5 A (the second shell is at 5.2 A), so every row is the 8-slot minimum."""
    from surface_sampling_amd import structures

    a = 3.7
    sites = np.array([(i, j, k) for k in range(3) for j in range(4) for i in range(4)], dtype=np.float64)[:n] * a
    pos = sites + np.array([0.5 * a, 0.5 * a, 6.0]) + np.random.default_rng(seed).normal(0.0, 0.05, (n, 3))
    cell = np.diag([4 * a, 4 * a, 3 * a + 15.0])
    return structures.Structure(slab.numbers[:n].copy(), pos, cell, np.array([True, True, True]))


@pytest.fixture(scope="module")
def sparse_batch(golden, oracle_mod, slab):
    """11 chains of 44 atoms and the same lattice cut to 12 atoms, their oracle results and one evaluation of the batch."""
    chains = [_sparse(slab, 44, 100 + k) for k in range(11)] + [_sparse(slab, 12, 7)]
    refs = [_oracle(golden, oracle_mod, s) for s in chains]
    eng = _engine(golden)
    res = eng.evaluate([_arrays(s) for s in chains])
    eng.close()
    return chains, refs, res


def test_consecutive_two_step_bundles(oracle_mod, sparse_batch):
    """44 atoms with at most 8 neighbors each: 11 bundles of 2 steps for 4 waves, so three waves own three consecutive 2-step bundles
    and every switch follows the previous one two steps later."""
    chains, refs, res = sparse_batch
    assert _four_wave_form(chains)
    for s in chains[:11]:
        counts = _neighbor_counts(oracle_mod, s)
        assert 1 <= counts.min() and counts.max() <= 8, counts
        steps, waves = _wave_steps(counts)
        assert steps == [2] * 11 and sorted(len(w) for w in waves) == [2, 3, 3, 3]
    _against_oracle(res, chains, refs, which=range(11))


def test_wave_without_a_bundle(oracle_mod, sparse_batch):
    """The lattice cut to 12 atoms, in the same 4-wave launch: 3 bundles for 4 waves, one wave returns before the loop."""
    chains, refs, res = sparse_batch
    assert _four_wave_form(chains) and len(chains[11]) == 12
    counts = _neighbor_counts(oracle_mod, chains[11])
    assert counts.max() <= 8
    steps, waves = _wave_steps(counts)
    assert steps == [2, 2, 2] and sorted(len(w) for w in waves) == [0, 1, 1, 1]
    _against_oracle(res, chains, refs, which=[11])


def _with_adsorbates(slab, k, seed):
    """The 60-atom slab with k oxygen atoms 4.5 A above its top layer, 3.9 A apart: they keep the 8-slot minimum."""
    from surface_sampling_amd import structures

    rng = np.random.default_rng(seed)
    frac = np.array([(0.25, 0.25), (0.75, 0.75), (0.75, 0.25), (0.25, 0.75)])[:k]
    ads = np.zeros((k, 3))
    ads[:, :2] = frac @ slab.cell[:2, :2]
    ads[:, 2] = slab.positions[:, 2].max() + 4.5
    pos = np.concatenate([slab.positions + rng.normal(0.0, 0.03, slab.positions.shape), ads + rng.normal(0.0, 0.03, ads.shape)])
    return structures.Structure(np.concatenate([slab.numbers, np.full(k, 8, slab.numbers.dtype)]), pos, slab.cell, slab.pbc)


def test_long_bundles_followed_by_two_step_ones(golden, oracle_mod, slab):
    """The slab's 15 bundles of 8 .. 13 steps and a last bundle of 1 .. 4 adsorbate atoms with 2 steps, dealt to 4 waves: the wave
    that walks the 2-step bundle has walked long ones before it, and the waves' step totals take every residue modulo 3."""
    distinct = [_with_adsorbates(slab, k, 40 + k) for k in (1, 2, 3, 4)]
    chains = [distinct[b % 4] for b in range(12)]
    assert _four_wave_form(chains)
    residues = set()
    for s in distinct:
        counts = _neighbor_counts(oracle_mod, s)
        assert counts[60:].max() <= 8 and counts[:60].min() > 8, counts
        steps, waves = _wave_steps(counts)
        assert len(steps) == 16 and steps[-1] == 2 and min(steps[:-1]) > 2
        last = [w for w in waves if w and w[-1] == 2]
        assert len(last) == 1 and len(last[0]) == 4 and max(last[0]) > 2   # long bundles first, then the 2-step one, in one wave
        residues |= {sum(w) % 3 for w in waves}
    print(f"residues of the per-wave step totals modulo 3: {sorted(residues)}")
    assert residues == {0, 1, 2}
    refs = [_oracle(golden, oracle_mod, s) for s in distinct]
    eng = _engine(golden)
    res = eng.evaluate([_arrays(s) for s in chains])
    eng.close()
    _against_oracle(res, chains, [refs[b % 4] for b in range(12)])


@pytest.fixture(scope="module")
def ragged(golden, slab):
    """272, 248, 60 and 12 atoms (the ragged batch of tests/test_edge_fwd_persistent.py)."""
    from surface_sampling_amd import structures

    big = slab.repeat((2, 2, 1))
    keep = np.sort(np.random.default_rng(11).choice(len(slab), size=12, replace=False))
    chains = [structures.synth_chain(big, 24), structures.synth_chain(big, 25), slab,
              structures.Structure(slab.numbers[keep], slab.positions[keep], slab.cell, slab.pbc)]
    assert [len(c) for c in chains] == [272, 248, 60, 12]
    return chains


@pytest.fixture(scope="module")
def ragged_refs(golden, oracle_mod, ragged):
    return [_oracle(golden, oracle_mod, s) for s in ragged]


def test_ragged_batch(golden, ragged, ragged_refs):
    eng = _engine(golden)
    res = eng.evaluate([_arrays(s) for s in ragged])
    eng.close()
    _against_oracle(res, ragged, ragged_refs)


def test_active_mask_with_a_converged_chain_between_two_live_ones(golden, oracle_mod, ragged):
    """Lock-step FIRE on the ragged batch with the 248-atom chain held fixed entirely: after the driver's first poll the evaluations run
    under the activity mask, the reverse launches skip the chain between two live ones."""
    from surface_sampling_amd import structures

    fixed = np.zeros(sum(len(c) for c in ragged), np.uint8)
    fixed[len(ragged[0]):len(ragged[0]) + len(ragged[1])] = 1
    eng = _engine(golden)
    eng.upload([_arrays(c) for c in ragged])
    info = eng.relax("FIRE", fixed=fixed, max_steps=6, fmax=0.01)
    res = eng.download()
    eng.close()
    assert info["converged"][1] and info["n_steps"][0] == 6 and info["n_steps"][2] == 6
    for b in (0, 2):   # the last evaluation (masked) at the relaxed geometry of the live chains on both sides
        a0, a1 = res["cfg_start"][b], res["cfg_start"][b + 1]
        s = structures.Structure(ragged[b].numbers, info["positions"][a0:a1], ragged[b].cell, ragged[b].pbc)
        ref = _oracle(golden, oracle_mod, s)
        de, df = abs(float(res["energy"][b]) - ref["energy"]), np.abs(res["forces"][a0:a1] - ref["forces"]).max()
        print(f"live chain {b} after 6 FIRE steps: |dE| {de:.2e} eV  max|dF| {df:.2e} eV/A")
        assert de <= E_TOL and df <= F_TOL
        assert abs(float(res["energy_std"][b]) - ref["energy_std"]) <= STD_TOL
        assert np.abs(res["forces_std"][a0:a1] - ref["forces_std"]).max() <= STD_TOL


def test_capacity_overflow_and_the_rerun_is_right(golden, ragged, ragged_refs):
    """A slot capacity too small for the first evaluation: the reverse launches return on the overflow flag, the host regrows the
    buffers and the rerun is right."""
    eng = _engine(golden)
    eng.debug_capacity(slots_per_atom=16, tight=1)
    res = eng.evaluate([_arrays(s) for s in ragged])
    eng.close()
    _against_oracle(res, ragged, ragged_refs)


def _knob_sets():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dump_painn.py")
    spec = importlib.util.spec_from_file_location("_dump_painn_knobs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.KNOB_SETS


KNOB_SETS = _knob_sets()


@pytest.fixture(scope="module")
def small(golden, oracle_mod, slab):
    """120 atoms: a single chain launches 8-wave workgroups, and ranges of 100 and 70 atoms cut it into two passes."""
    s = slab.repeat((2, 1, 1))
    s.positions = s.positions + np.random.default_rng(3).normal(0.0, 0.04, s.positions.shape)
    assert len(s) == 120
    return s, _oracle(golden, oracle_mod, s)


@pytest.mark.parametrize("name", sorted(KNOB_SETS))
def test_small_case_under_every_knob_set(golden, monkeypatch, small, name):
    s, ref = small
    eng = _engine(golden, monkeypatch, KNOB_SETS[name])
    res = eng.evaluate([_arrays(s)])
    eng.close()
    _against_oracle(res, [s], [ref])
