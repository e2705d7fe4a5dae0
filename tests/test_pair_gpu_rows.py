"""The pair kernel (csrc/pair.hip: k_pair_site) on the MI355X where a 4-lane strided row loop, a packed LDS term table and a strict
cutoff test can go wrong without a bulk test noticing: rows of 0 .. 9 slots and chains that straddle 64-centre workgroups; 8 and 5
types with coefficients that differ for every pair and three terms on some pairs; dimers exactly at, one ulp inside and one ulp
outside a cutoff.  Reference, tolerances and printing as tests/test_pair_gpu.py; the inputs (tests/pair_cases.py) are rehearsed on
the CPU in tests/test_pair_cpu.py."""
import numpy as np
import pytest

import pair_cases as pc
import pair_oracle as po
from test_pair_gpu import E_REL, _check, _engine, _model

pytestmark = pytest.mark.gpu


# 1 --------------------------------------------------------------------------------------------------------------------------------
def test_rows_of_zero_to_nine_slots_and_chains_that_straddle_workgroups():
    """The hand-placed cluster (rows of 0, 1, 2, 3, 4, 5, 6 and 9 slots), then a 65-atom and a 63-atom periodic chain: the first
    workgroup serves two chains with different cells, the 65-atom chain lies in two workgroups.  The lone atom has no slot: its
    force is exactly zero and its pe/atom is the coul/dsf self term alone (both sides build it from five fp64 operations on their
    libm's erfc: 4 ulp bounds that).  Every chain evaluated alone gives the bits it gives in the batch."""
    m = _model(pc.ROWS_MODEL, 2)
    batch = pc.rows_batch()
    deg = pc.degrees(batch[0], pc.ROWS_RC)
    assert deg.tolist() == pc.ROWS_DEGREES and {0, 1, 2, 3, 4, 5, 9} <= set(deg.tolist())
    assert [len(s[0]) for s in batch] == [31, 65, 63]
    eng = _engine(m)
    e, ea, f = _check(eng, m, batch, "rows")
    terms, q = po.model_of(m)
    self_e = po.pair(terms, q, *batch[0])[1][0]
    print(f"rows: lone atom F {f[0]}  pe/atom {ea[0]:+.17e}  self term {self_e:+.17e}  degrees {deg.tolist()}")
    assert (f[0] == 0.0).all() and abs(ea[0] - self_e) <= 4 * 2.0 ** -52 * abs(self_e) and self_e < -0.1
    o = 0
    for b, s in enumerate(batch):
        n = len(s[0])
        e1, ea1, f1 = eng.evaluate_f64([s])
        assert e1[0] == e[b] and np.array_equal(ea1, ea[o:o + n]) and np.array_equal(f1, f[o:o + n]), b
        o += n
    eng.close()


# 2 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [8, 5])
def test_every_pair_of_eight_and_five_types_reads_its_own_terms(nt):
    """nt (nt + 1) / 2 unordered pairs with coefficients that differ by a formula in (a, b), styles cycling through lj/cut, morse,
    buck and born, and lj/cut + morse + coul/dsf with three different cutoffs on the pairs (0, nt - 1), (nt - 1, nt - 1) and (3, 4):
    nt = 8 fills the whole table in LDS, nt = 5 packs it with a stride that is no power of two.  Swapping two type labels moves the
    restatement's energy by at least 2.9e-2 eV (tests/test_pair_cpu.py), eight orders above the tolerance.  The model goes in through
    the parser and as plain term tuples: the same bits."""
    from surface_sampling_amd import backend

    m = _model(pc.table_lines(nt), nt)
    s = pc.table_chain(nt)
    assert len(s[0]) == 40 and set(s[0].tolist()) == set(range(nt)) and pc.cutoff_margin(m, s) > 0.005
    by_pair = {}
    for t in m.terms:
        by_pair.setdefault((t.type_a, t.type_b), []).append(t.style)
    assert len(by_pair) == nt * (nt + 1) // 2 and all(by_pair[p] == [1, 2, 5] for p in ((0, nt - 1), (nt - 1, nt - 1), (3, 4)))
    eng = _engine(m)
    res = _check(eng, m, [s], f"table nt={nt}", stress=True)
    st = eng.stress()[0]
    eng.close()
    plain = backend.PairEngine([tuple(t) for t in m.terms], charges=m.charges, n_types=nt, device=0)
    res2 = plain.evaluate_f64([s])
    st2 = plain.stress()[0]
    plain.close()
    assert all(np.array_equal(a, b) for a, b in zip(res + (st,), res2 + (st2,)))


# 3 --------------------------------------------------------------------------------------------------------------------------------
def _dimer_energies(lines, rc, tag):
    m = _model(lines, 1)
    structs, sep = pc.cutoff_dimers(rc)
    assert sep[1] == rc and sep[0] == np.nextafter(rc, 0.0) and sep[2] == np.nextafter(rc, 100.0)
    eng = _engine(m)
    e, ea, f = _check(eng, m, structs, tag)
    eng.close()
    assert np.isfinite(e).all() and np.isfinite(f).all()
    return m, e, f.reshape(3, 2, 3)


def test_lj_cut_keeps_a_pair_one_ulp_inside_the_cutoff_and_drops_it_at_the_cutoff():
    """lj/cut 6.0, shift no, atoms at x = 1 and x = 7 (and the two fp64 neighbours of 7): r < rc is strict, as in LAMMPS (rsq <
    cutsq).  At rc and beyond the energy and the forces are exactly zero; one ulp inside, the pair counts with E(rc) = -1.33e-3 eV."""
    m, e, f = _dimer_energies(pc.CUT_LJ, 6.0, "cutoff lj/cut")
    E_rc = po.term_energy("lj/cut", m.terms[0].c, 6.0, np.nextafter(6.0, 0.0))[0]
    print(f"cutoff lj/cut: E {e.tolist()}  E(rc) {E_rc:+.6e}")
    assert e[1] == 0.0 and e[2] == 0.0 and not f[1:].any()
    assert abs(E_rc) > 1e-3 and abs(e[0] - E_rc) <= E_REL and np.abs(f[0]).max() > 1e-3


def test_overlay_terms_switch_off_at_their_own_cutoffs():
    """hybrid/overlay lj/cut 5.0 + morse 6.0 on the same pair.  At r = 5 and one ulp beyond only the Morse term counts, one ulp inside
    both; at 5.5 the inner term is off and the outer on; at r = 6 and beyond nothing is left."""
    m, e, f = _dimer_energies(pc.CUT_OVERLAY, 5.0, "cutoff overlay inner")
    lj, mo = m.terms
    assert (lj.style, lj.rc, mo.style, mo.rc) == (1, 5.0, 2, 6.0)
    e_lj = po.term_energy("lj/cut", lj.c, 5.0, np.nextafter(5.0, 0.0))[0]
    e_mo = po.term_energy("morse", mo.c, 6.0, 5.0)[0]
    print(f"cutoff overlay inner: E {e.tolist()}  lj(5) {e_lj:+.6e}  morse(5) {e_mo:+.6e}")
    assert abs(e_lj) > 1e-3 and abs(e[1] - e_mo) <= E_REL and abs(e[2] - e_mo) <= E_REL and abs(e[0] - (e_lj + e_mo)) <= E_REL
    _, e, f = _dimer_energies(pc.CUT_OVERLAY, 6.0, "cutoff overlay outer")
    e_mo = po.term_energy("morse", mo.c, 6.0, np.nextafter(6.0, 0.0))[0]
    print(f"cutoff overlay outer: E {e.tolist()}  morse(6) {e_mo:+.6e}")
    assert e[1] == 0.0 and e[2] == 0.0 and not f[1:].any() and abs(e_mo) > 1e-3 and abs(e[0] - e_mo) <= E_REL
    between = (np.zeros(2, np.int32), np.array([[1.0, 3.0, 3.0], [6.5, 3.0, 3.0]]), pc.CUT_BOX, pc.OPEN)
    eng = _engine(m)
    eb, _, _ = _check(eng, m, [between], "cutoff overlay between")
    eng.close()
    assert abs(eb[0] - po.term_energy("morse", mo.c, 6.0, 5.5)[0]) <= E_REL


def test_coul_dsf_vanishes_with_its_force_one_ulp_inside_the_cutoff():
    """coul/dsf 0.2 6.0, q = 1: energy and force of the pair are damped and shifted to zero at rc, so one ulp inside they are below
    1e-12 in magnitude (and finite): what is left of the chain energy is the two self terms."""
    m, e, f = _dimer_energies(pc.CUT_DSF, 6.0, "cutoff coul/dsf")
    self_e = po.pair(*po.model_of(m), *pc.cutoff_dimers(6.0)[0][1])[1]
    pair_e = e - self_e.sum()
    print(f"cutoff coul/dsf: E - self terms {pair_e.tolist()}  max|F| {np.abs(f).max(axis=(1, 2)).tolist()}")
    assert self_e.sum() < -1.0 and (np.abs(pair_e) < 1e-12).all() and (np.abs(f) < 1e-12).all()
    assert not f[1:].any()
