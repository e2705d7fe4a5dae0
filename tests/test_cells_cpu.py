"""The checker of tests/test_gpu_cells.py, pinned on the CPU: the battery of skewed, thin and partly periodic cells
(tests/cell_cases.py) really holds what it claims, the fp64 oracle's neighbor list equals an enumerator written without its
image formula, and the oracles' energies and forces do not change under transforms that keep the physics."""

import numpy as np
import pytest

import cell_cases as cc


@pytest.fixture(scope="module")
def cases():
    return cc.battery()


def test_battery_states_its_image_grid_and_reaches_the_thin_cell_paths(cases):
    """Every case states nimg / image count for its potential's cutoff; the battery holds nimg >= 2, > 64 images, shifts of
    |S| >= 2 between a pair, self-image edges (i, i, S != 0), all eight pbc combinations and a pair at exactly the cutoff."""
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    many, far, self_img, only_self, exact = set(), set(), set(), set(), set()
    for c in cases:
        rc = cc.cutoff_of(c.pot)
        assert cc.face_nimg(c.cell, c.pbc, rc) == tuple(c.nimg), c.name
        assert cc.n_images(c.nimg) == c.images, c.name
        i, j, S, r = cc.brute_neighbors(c.pos, c.cell, c.pbc, rc)
        assert len(i) > 0, c.name
        if c.images > 64:
            many.add(c.name)
        if np.abs(S).max() >= 2:
            far.add(c.name)
        if (i == j).any():
            self_img.add(c.name)
            assert (np.abs(S[i == j]).sum(axis=1) > 0).all()
        if (i == j).all():
            only_self.add(c.name)
        if (np.sum(r * r, axis=1) == rc * rc).any():
            exact.add(c.name)
    assert max(max(c.nimg) for c in cases) >= 3 and len(many) >= 5 and len(far) >= 5, (many, far)
    assert {"cu_fcc_primitive", "si_simple_cubic"} <= only_self and len(self_img) >= 8
    assert "painn_exact_cutoff" in exact
    assert {tuple(c.pbc) for c in cases if c.name.startswith("tri_")} == set(cc.PBC8)
    for pot in ("painn", "gan", "si", "eam"):       # every potential has a case beyond the 27-image grid
        assert any(c.images > 27 for c in cases if c.pot == pot), pot


def test_oracle_neighbors_equal_the_brute_enumeration(oracle_mod, cases):
    """orc_neighbors (wrapped positions, floor(rc / h) + 1 images) against brute_neighbors (raw positions, a bound of its own):
    the same (i, j, S) set exactly, edge vectors to 1e-12, on every case and every transformed variant."""
    n = 0
    for c in cases:
        rc = cc.cutoff_of(c.pot)
        for v in [c] + cc.variants(c):
            bi, bj, bS, br = cc.brute_neighbors(v.pos, v.cell, v.pbc, rc)
            oi, oj, oS, orr = cc.sort_edges(*oracle_mod.neighbors(v.pos, v.cell, v.pbc, rc))
            assert cc.edge_keys(bi, bj, bS) == cc.edge_keys(oi, oj, oS), v.name
            assert np.abs(br - orr).max() <= 1e-12, v.name
            n += 1
    assert n > 80


def _check_variants(case, fn, e_rel=1e-10, f_abs=1e-9):
    """fn(case) -> (E, F): every variant gives E (n E for the supercell) and F (rotated back / tiled)."""
    E0, F0 = fn(case)
    worst = 0.0
    for v in cc.variants(case):
        E, F = fn(v)
        n = getattr(v, "n", 1)
        assert abs(E - n * E0) <= e_rel * max(1.0, abs(n * E0)), (v.name, E, n * E0)
        want = np.tile(F0, (n, 1)) if n > 1 else F0
        dF = np.abs(cc.rotated_back(v, F) - want).max()
        assert dF <= f_abs, (v.name, dF)
        worst = max(worst, dF)
    return E0, F0, worst


def test_painn_oracle_is_invariant_under_the_cell_transforms(golden, oracle_mod, cases):
    """The fp64 PaiNN ensemble (offset table without the constant, so that E is extensive): a new basis of the periodic vectors,
    periodic vectors added to an open axis, a rotation, atoms far outside the cell, a 2x supercell; the atoms on cell faces
    give the bulk energy."""
    table, _ = golden.offset_table()

    def fn(v):
        r = oracle_mod.ensemble(golden.blobs, v.numbers, v.pos, v.cell, v.pbc, 64, table, 0.0)
        return r["energy"], r["forces"]

    got = {}
    for c in cases:
        if c.pot == "painn":
            got[c.name] = _check_variants(c, fn)
    E_bulk, F_bulk, _ = got["sto_bulk"]
    assert abs(got["sto_bulk_sheared"][0] - E_bulk) <= 1e-10 * abs(E_bulk)     # the sheared twin is the same crystal
    assert np.abs(got["sto_bulk_sheared"][1] - F_bulk).max() <= 1e-9
    assert abs(got["sto_221_rattled"][0] - 4 * E_bulk) < 1.0                   # (a rattled 2 x 2 x 1 repeat is close to 4 cells)


def test_tersoff_oracle_is_invariant_under_the_cell_transforms(oracle_mod, cases):
    """GaN.tersoff, Tersoff's Si(C) set and a synthetic three-species set on the fp64 oracle; the literature known answer
    of Si(C) in the 2-atom diamond primitive cell (4.63 eV per atom at 5.432 A)."""
    from conftest import SI_T3_ECOH, synthetic_tersoff

    params = {"gan": cc.gan_params(), "si": cc.si_params()}
    got = {}
    for c in cases:
        if c.pot in params:
            P = params[c.pot]
            got[c.name] = _check_variants(c, lambda v, P=P: oracle_mod.tersoff(P, *v.typed())[::2])
    assert abs(got["si_diamond_primitive"][0] / 2 - SI_T3_ECOH) <= 5e-4
    assert np.abs(got["si_diamond_primitive"][1]).max() < 1e-10 and np.abs(got["si_simple_cubic"][1]).max() < 1e-10
    assert abs(got["gan_slab"][0] - got["gan_slab_skewed"][0]) <= 1e-10 * abs(got["gan_slab"][0])
    P = synthetic_tersoff(3, 5)
    tri = next(c for c in cases if c.name == "tri_TTT")
    syn = tri.with_("syn_tri", types=np.array([0, 1, 2, 1, 0], np.int32))
    E, F, _ = _check_variants(syn, lambda v: oracle_mod.tersoff(P, *v.typed())[::2])
    assert np.isfinite(E) and np.abs(F).max() > 1e-3


def test_eam_oracle_is_invariant_under_the_cell_transforms(cases):
    """Cu_u3 EAM on the numpy oracle; the 1-atom fcc primitive cell (343 images, every neighbor a self image) gives the
    potential's cohesive energy with zero force."""
    import eam_oracle

    f = cc.cu_funcfl()
    got = {}
    for c in cases:
        if c.pot == "eam":
            got[c.name] = _check_variants(c, lambda v: eam_oracle.eam(f, v.pos, v.cell, v.pbc)[::2])
    assert abs(got["cu_fcc_primitive"][0] - (-3.54)) <= 2e-3 and np.abs(got["cu_fcc_primitive"][1]).max() < 1e-12
