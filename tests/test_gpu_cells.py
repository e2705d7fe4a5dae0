"""Device parity on skewed, thin and partly periodic cells (tests/cell_cases.py): nimg >= 2, batches of more than 64 images
(the neighbor search without hit masks), self-image edges, strongly skewed bases, open axes with sheared cell vectors, atoms
on the cell faces and far outside the cell, a pair at exactly the cutoff -- on PaiNN, Tersoff and EAM handles, in evaluation,
stress, CG (lock-step, compacted, chain-resident) and BFGS.  tests/test_cells_cpu.py pins the checker."""

import numpy as np
import pytest

import cell_cases as cc
from cg_oracle import cg_minimize

pytestmark = pytest.mark.gpu

E_TOL, F_TOL, STD_TOL = 1e-4, 2e-4, 2e-4      # tests/test_gpu_parity.py: fp32 PaiNN against the fp64 oracle


@pytest.fixture(scope="module")
def cases():
    return cc.battery()


@pytest.fixture(scope="module")
def painn(golden):
    from surface_sampling_amd import backend

    table, const = golden.offset_table()
    eng = backend.PainnEngine(golden.blobs, device=0, offset_per_z=table, offset_const=const)
    yield eng
    eng.close()


def _engine(kind):
    from surface_sampling_amd import backend

    if kind == "gan":
        return backend.TersoffEngine(cc.gan_params(), device=0)
    if kind == "si":
        return backend.TersoffEngine(cc.si_params(), device=0)
    return backend.EAMEngine(cc.cu_funcfl(), device=0)


def _run(eng, batch, kind):
    """One evaluation of ``batch`` (cases) on a PaiNN ("painn") or analytic handle: (energy [B], forces [N, 3], edges)."""
    if kind == "painn":
        r = eng.evaluate([c.arrays() for c in batch])
        e, f = r["energy"], r["forces"]
    else:
        nt = getattr(eng, "n_types", 1)
        e, _, f = eng.evaluate_f64([(c.types % nt, c.pos, c.cell, c.pbc.astype(np.uint8)) for c in batch])
    return e, f, eng.neighbors()


def _split_edges(edges, batch):
    """Per-chain edge sequences (row order of the device list) with chain-local atom indices."""
    ei, ej, eS, er = edges
    start = np.cumsum([0] + [len(c) for c in batch])
    out = []
    for b in range(len(batch)):
        m = (ei >= start[b]) & (ei < start[b + 1])
        out.append((ei[m] - start[b], ej[m] - start[b], eS[m], er[m]))
    return out


@pytest.mark.parametrize("kind", ["painn", "gan", "eam"])
def test_device_neighbor_lists_equal_the_brute_enumeration(cases, painn, kind):
    """Every case of the battery in ONE ragged batch (up to 343 images: no hit masks) on a PaiNN, a Tersoff and an EAM handle:
    engine.neighbors() gives exactly the (i, j, S) set of brute_neighbors at the handle's cutoff, fp32 edge vectors to 2e-6."""
    eng = painn if kind == "painn" else _engine(kind)
    rc = cc.PAINN_RC if kind == "painn" else cc.cutoff_of(kind)
    _, _, edges = _run(eng, cases, kind)
    assert max(cc.n_images(cc.face_nimg(c.cell, c.pbc, rc)) for c in cases) > 64
    worst = 0.0
    for c, (i, j, S, r) in zip(cases, _split_edges(edges, cases)):
        bi, bj, bS, br = cc.brute_neighbors(c.pos, c.cell, c.pbc, rc)
        assert cc.edge_keys(i, j, S) == cc.edge_keys(bi, bj, bS), c.name
        _, _, _, r = cc.sort_edges(i, j, S, r)
        d = float(np.abs(r - br).max()) if len(br) else 0.0
        assert d < 2e-6, (c.name, d)
        worst = max(worst, d)
    print(f"{kind}: {len(cases)} cases, {len(edges[0])} edges, max |er - r| {worst:.2e}")
    if kind != "painn":
        eng.close()


@pytest.mark.parametrize("kind", ["painn", "gan", "si", "eam"])
def test_hit_mask_and_re_search_paths_agree_bit_for_bit(cases, painn, kind):
    """Each case of a potential evaluated alone, in a batch whose largest image grid is <= 64 (the fill pass replays the hit
    masks of the count pass) and in the batch of all its cases with a > 64-image chain (the fill pass repeats the unpruned
    search): edge lists, energies and forces identical bit for bit."""
    eng = painn if kind == "painn" else _engine(kind)
    own = [c for c in cases if c.pot == kind]
    rc = cc.cutoff_of(kind)
    imgs = [cc.n_images(cc.face_nimg(c.cell, c.pbc, rc)) for c in own]
    assert max(imgs) > 64
    alone = []
    for c in own:
        e, f, edges = _run(eng, [c], kind)
        alone.append((e[0], f, _split_edges(edges, [c])[0]))
    small = [c for c, n in zip(own, imgs) if n <= 64]
    for batch in ([small] if len(small) > 1 else []) + [own, own[::-1]]:
        e, f, edges = _run(eng, batch, kind)
        per = _split_edges(edges, batch)
        start = np.cumsum([0] + [len(c) for c in batch])
        for b, c in enumerate(batch):
            e1, f1, ed1 = alone[own.index(c)]
            assert e[b] == e1, (kind, c.name)
            assert np.array_equal(f[start[b]:start[b + 1]], f1), (kind, c.name)
            for x, y in zip(per[b], ed1):
                assert np.array_equal(x, y), (kind, c.name)
    if kind != "painn":
        eng.close()


def test_painn_cases_and_variants_match_the_oracle(golden, oracle_mod, cases, painn):
    """Every PaiNN case and every transformed variant (new periodic basis, periodic vectors added to an open axis, rotation,
    atoms far outside the cell, 2x supercell) in one batch against the fp64 oracle of the UNTRANSFORMED structure (the
    supercell against its own oracle, whose forces are the tiled ones), forces rotated back."""
    table, const = golden.offset_table()
    batch, refs = [], []
    for c in (c for c in cases if c.pot == "painn"):
        ref = oracle_mod.ensemble(golden.blobs, *c.arrays(), 64, table, const)
        for v in [c] + cc.variants(c):
            if getattr(v, "n", 1) > 1:
                r2 = oracle_mod.ensemble(golden.blobs, *v.arrays(), 64, table, const)
                assert np.abs(r2["forces"] - np.tile(ref["forces"], (v.n, 1))).max() < 1e-9
                batch.append(v); refs.append(r2)
            else:
                batch.append(v); refs.append(ref)
    res = painn.evaluate([v.arrays() for v in batch])
    assert not painn.saturated().any()
    start = np.cumsum([0] + [len(v) for v in batch])
    de = df = ds = 0.0
    for b, (v, ref) in enumerate(zip(batch, refs)):
        F = res["forces"][start[b]:start[b + 1]].astype(np.float64)
        e_dev = abs(float(res["energy"][b]) - ref["energy"])
        f_dev = float(np.abs(cc.rotated_back(v, F) - ref["forces"]).max())
        s_dev = abs(float(res["energy_std"][b]) - ref["energy_std"])
        assert e_dev <= E_TOL, (v.name, e_dev)
        assert f_dev <= F_TOL, (v.name, f_dev)
        assert s_dev <= STD_TOL, (v.name, s_dev)
        if getattr(v, "rot", None) is None:       # (a component-wise spread is not a vector: compared unrotated only)
            fs = float(np.abs(res["forces_std"][start[b]:start[b + 1]] - ref["forces_std"]).max())
            assert fs <= STD_TOL, (v.name, fs)
        de, df, ds = max(de, e_dev), max(df, f_dev), max(ds, s_dev)
    print(f"painn: {len(batch)} chains, max |dE| {de:.2e} eV, max |dF| {df:.2e} eV/A, max |d std| {ds:.2e}")


def _strained(c, eps):
    d = np.eye(3) + eps
    return c.with_(pos=c.pos @ d.T, cell=c.cell @ d.T)


def test_painn_stress_on_sheared_bulk_and_rotated_slab(golden, oracle_mod, cases):
    """The device virial on the sheared bulk SrTiO3 (175 images) and on a rotated slab (a full, non-triangular cell matrix)
    against central differences of the fp64 oracle energy (the tolerance of test_stress_is_the_strain_derivative_of_the_oracle_energy);
    EnsembleNFFSurface.calculate on the rotated slab equals the engine."""
    from surface_sampling_amd import backend, calculators as calcs
    from surface_sampling_amd.structures import Structure

    table, const = golden.offset_table()
    Zs, Xs, Cs, Ps = cc._golden_structure("SrTiO3_2x2_pristine")
    slab = cc.rotate(cc.Case("sto_slab", "painn", Zs, Xs, Cs, Ps, (1, 1, 1), 27), seed=3, name="sto_slab_rot")
    batch = [cc.by_name(cases)["sto_bulk_sheared"], slab]
    eng = backend.PainnEngine(golden.blobs, device=0, offset_per_z=table, offset_const=const)
    res = eng.evaluate([c.arrays() for c in batch])
    st, sd = eng.stress()
    voigt = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
    delta = 2e-4
    for b, c in enumerate(batch):
        vol = abs(np.linalg.det(c.cell))
        for k, (i, j) in enumerate(voigt):
            eps = np.zeros((3, 3))
            eps[i, j] += 0.5 * delta
            eps[j, i] += 0.5 * delta
            ep, em = (oracle_mod.ensemble(golden.blobs, *t.arrays(), 64, table, const) for t in (_strained(c, eps), _strained(c, -eps)))
            want = (ep["energy"] - em["energy"]) / (2 * delta) / vol
            want_m = (np.asarray(ep["energy_models"], float) - np.asarray(em["energy_models"], float)) / (2 * delta) / vol
            print(f"{c.name} voigt {k}: device {st[b, k]:+.6e}  oracle FD {want:+.6e} eV/A^3")
            assert abs(st[b, k] - want) * vol <= 3e-3 + 2e-4 * abs(want) * vol
            assert abs(sd[b, k] - want_m.std()) * vol <= 3e-3 + 2e-4 * want_m.std() * vol
    eng.close()
    calc = calcs.EnsembleNFFSurface(golden.blobs, device="cuda:0", model_units="kcal/mol", prediction_units="eV")
    calc.set(offset=True, offset_data=golden.offset_data)
    calc.calculate(Structure(slab.numbers, slab.pos, slab.cell, slab.pbc), properties=("energy", "forces", "stress"))
    n0 = len(batch[0])
    assert float(np.ravel(calc.results["energy"])[0]) == float(res["energy"][1])
    assert np.array_equal(np.asarray(calc.results["forces"], np.float32), res["forces"][n0:])
    assert np.array_equal(calc.results["stress"], st[1])


@pytest.mark.parametrize("kind", ["gan", "si", "eam"])
def test_analytic_cases_and_variants_match_the_oracle(oracle_mod, cases, kind):
    """Tersoff (GaN.tersoff, Si(C)) and EAM (Cu_u3), fp64 on the device: every case and variant against the oracle of the
    untransformed structure, energies to 1e-9 relative, per-atom energies to 1e-9, forces to 1e-8.  Known answers on
    non-orthogonal cells: Si(C) diamond in its 2-atom primitive cell (-4.63 eV per atom), Cu_u3 fcc in its 1-atom primitive
    cell (-3.54 eV, 343 images, zero force)."""
    import eam_oracle
    from conftest import SI_T3_ECOH

    eng = _engine(kind)
    if kind == "eam":
        fl = cc.cu_funcfl()
        oracle = lambda c: eam_oracle.eam(fl, c.pos, c.cell, c.pbc)                      # noqa: E731
    else:
        P = cc.gan_params() if kind == "gan" else cc.si_params()
        oracle = lambda c: oracle_mod.tersoff(P, *c.typed())                             # noqa: E731
    batch, refs = [], []
    for c in (c for c in cases if c.pot == kind):
        E0, ea0, F0 = oracle(c)
        for v in [c] + cc.variants(c):
            n = getattr(v, "n", 1)
            batch.append(v)
            refs.append((n * E0, np.tile(ea0, n), np.tile(F0, (n, 1))))
    e, ea, F = eng.evaluate_f64([v.typed() for v in batch])
    start = np.cumsum([0] + [len(v) for v in batch])
    de = df = 0.0
    for b, (v, (E0, ea0, F0)) in enumerate(zip(batch, refs)):
        s = slice(start[b], start[b + 1])
        assert abs(e[b] - E0) <= 1e-9 * max(1.0, abs(E0)), (v.name, e[b], E0)
        assert np.abs(ea[s] - ea0).max() <= 1e-9, v.name
        d = float(np.abs(cc.rotated_back(v, F[s]) - F0).max())
        assert d <= 1e-8, (v.name, d)
        de, df = max(de, abs(e[b] - E0) / max(1.0, abs(E0))), max(df, d)
    print(f"{kind}: {len(batch)} chains, max |dE|/|E| {de:.2e}, max |dF| {df:.2e} eV/A")
    names = [v.name for v in batch]
    if kind == "si":
        k = names.index("si_diamond_primitive")
        assert abs(e[k] / 2 - SI_T3_ECOH) <= 5e-4 and np.abs(F[start[k]:start[k + 1]]).max() < 1e-9
    if kind == "eam":
        k = names.index("cu_fcc_primitive")
        assert abs(e[k] - (-3.54)) <= 2e-3 and np.abs(F[start[k]:start[k + 1]]).max() < 1e-10
    eng.close()


def _cg_batch(cases):
    """Five Tersoff GaN chains, each with a cell of its own and a different start: the 3x3 slab, its skewed-basis twin, a
    rotated copy, the rattled wurtzite primitive cell (75 images) and a pbc TTF chain with c' = c + a.  The rattles spread the
    stop times (7 .. ~35 iterations): three of the five chains are done at the driver's poll after 16 iterations."""
    nm = cc.by_name(cases)
    slab = nm["gan_slab"]
    ztop = slab.pos[:, 2].max()
    held = (slab.pos[:, 2] < ztop - 3.0).astype(np.uint8)
    r = lambda sigma, seed: cc._rattle(slab.pos, sigma, seed)                           # noqa: E731
    chains = [slab.with_("cg_slab", pos=r(0.05, 4)),
              cc.skew_basis(slab.with_(pos=r(0.02, 9)), "cg_skewed"),
              cc.rotate(slab.with_(pos=r(0.15, 5)), seed=2, name="cg_rot"),
              nm["gan_wurtzite_rattled"].with_("cg_wurtzite"),
              cc.shear_open_axis(slab.with_(pos=r(0.12, 4)), "cg_open")]
    masks = [held, held, held, np.zeros(4, np.uint8), held]
    return chains, masks


def test_cg_with_a_different_cell_on_every_chain(oracle_mod, cases, monkeypatch):
    """Device CG on five chains with five different cells: lock-step without compaction, lock-step with
    VSSR_RELAX_COMPACT=2 (cell, inverse, nimg and pbc gathered per live chain), the chain-resident minimiser and every chain
    relaxed alone agree bit for bit; the skewed chain and the wurtzite chain follow cg_oracle.cg_minimize on the fp64 oracle
    (same iteration / evaluation counts and stop reason, energies to 1e-9)."""
    from surface_sampling_amd import backend

    chains, masks = _cg_batch(cases)
    P = cc.gan_params()
    packs = [c.typed() for c in chains]
    mask = np.concatenate(masks)
    eng = backend.TersoffEngine(P, device=0)
    runs = {}
    for tag, env in (("lock", {"VSSR_CG_FUSED": "0", "VSSR_RELAX_COMPACT": "0"}),
                     ("compact", {"VSSR_CG_FUSED": "0", "VSSR_RELAX_COMPACT": "2"}),
                     ("resident", {"VSSR_CG_FUSED": "1", "VSSR_RELAX_COMPACT": "0"})):
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        runs[tag] = (eng.relax_cg_f64(packs, fixed=mask, max_iter=100), eng.last_relax_counts)
    monkeypatch.delenv("VSSR_CG_FUSED")
    monkeypatch.delenv("VSSR_RELAX_COMPACT")
    ref, ca = runs["lock"]
    for tag in ("compact", "resident"):
        for k, (x, y) in enumerate(zip(ref, runs[tag][0])):
            assert np.array_equal(x, y), (tag, k)
    ev = ref[5]
    assert len(set(ev.tolist())) >= 3, ev                                  # the chains stop at different times ...
    cb = runs["compact"][1]
    assert cb[0] == ca[0] and cb[1] < ca[1], (ca, cb)                      # ... and the compaction really dropped chains
    start = np.cumsum([0] + [len(c) for c in chains])
    for b, c in enumerate(chains):
        one = eng.relax_cg_f64([packs[b]], fixed=masks[b], max_iter=100)
        s = slice(start[b], start[b + 1])
        for k, (x, y) in enumerate(zip(one, ref)):
            want = y[s] if k in (1, 2, 3) else y[b:b + 1]
            assert np.array_equal(x, want), (c.name, k)
    for b in (1, 3):
        c = chains[b]

        def fn(p, c=c):
            E, _, F = oracle_mod.tersoff(P, c.types, p, c.cell, c.pbc.astype(np.uint8))
            return E, F

        pref, eref, niter, neval, reason, _ = cg_minimize(fn, c.pos, fixed=np.flatnonzero(masks[b]), max_iter=100)
        s = slice(start[b], start[b + 1])
        assert (ref[4][b], ref[5][b], ref[6][b]) == (niter, neval, reason), (c.name, ref[4][b], ref[5][b], ref[6][b], niter, neval, reason)
        assert abs(ref[0][b] - eref) < 1e-9 and np.abs(ref[3][s] - pref).max() < 1e-9, c.name
    eng.close()


def test_bfgs_on_the_two_bulk_srtio3_twins(golden, cases, painn):
    """PaiNN BFGS on the rattled cubic SrTiO3 cell and its sheared-basis twin (125 / 175 images): the same crystal, so the
    relaxed energies agree to E_TOL, below the start."""
    nm = cc.by_name(cases)
    twins = [nm["sto_bulk"], nm["sto_bulk_sheared"]]
    e0 = painn.evaluate([c.arrays() for c in twins])["energy"]
    assert abs(float(e0[0]) - float(e0[1])) <= E_TOL
    painn.upload([c.arrays() for c in twins])
    info = painn.relax_bfgs(max_steps=30, fmax=0.01)
    pos = info["positions"]
    e1 = painn.evaluate([c.with_(pos=pos[5 * b:5 * b + 5]).arrays() for b, c in enumerate(twins)])["energy"]
    assert abs(float(e1[0]) - float(e1[1])) <= E_TOL, (e1, info["n_steps"])
    assert float(e1[0]) < float(e0[0]) - 1e-3


@pytest.mark.parametrize("kind", ["painn", "gan", "eam"])
def test_degenerate_cells_are_refused_by_name(cases, painn, kind):
    """A cell too thin for the cutoff (nimg > 100), a zero-volume cell and pbc TTF with a zero third vector: BackendError naming
    the configuration and the fault; the same handle then evaluates a normal batch exactly as before."""
    from surface_sampling_amd import backend

    eng = painn if kind == "painn" else _engine(kind)
    good = [c for c in cases if c.pot == ("painn" if kind == "painn" else kind)][:2]
    before = _run(eng, good, kind)
    x = good[0]
    bad = [(x.with_(cell=np.diag([6.0, 6.0, 0.01]), pbc=(1, 1, 1)), "configuration 1: cell too thin for the cutoff"),
           (x.with_(cell=np.array([[4.0, 0, 0], [0, 4.0, 0], [4.0, 4.0, 0]]), pbc=(1, 0, 0)), "configuration 1: periodic but singular cell"),
           (x.with_(cell=np.array([[5.0, 0, 0], [0, 5.0, 0], [0, 0, 0]]), pbc=(1, 1, 0)), "configuration 1: periodic but singular cell")]
    for c, msg in bad:
        with pytest.raises(backend.BackendError, match=msg):
            _run(eng, [good[0], c], kind)
        after = _run(eng, good, kind)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
        for a, b in zip(after[2], before[2]):
            assert np.array_equal(a, b)
    if kind != "painn":
        eng.close()
