"""Stillinger-Weber on the host: the .sw parsers (Python and the library's C parser), the numpy restatement against the published
1985 silicon values, finite-difference forces, and LAMMPSSurfCalc configured from a Si(111)-tutorial-shaped run directory."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sw_oracle as so
from conftest import ROOT
from surface_sampling_amd import backend, calculators as calcs, sw as sw_io


# -- parser ------------------------------------------------------------------------------------------------------------------------
def test_builtin_si_model_is_the_published_1985_set():
    P = so.si_params()
    assert P.shape == (1, 1, 1, 11)
    assert P[0, 0, 0].tolist() == [2.1683, 2.0951, 1.80, 21.0, 1.20, -1.0 / 3.0, 7.049556277, 0.6022245584, 4.0, 0.0, 0.0]
    assert sw_io.max_cutoff(P) == pytest.approx(3.77118, abs=1e-5)
    assert sw_io.builtin_species(so.SI_1985) == ["Si"] and not sw_io.is_builtin("SW_Other__MO_000")


def test_parser_species_order_multiline_entries_and_foreign_elements():
    sp, P, text = so.three_species()
    assert np.array_equal(sw_io.parse_sw(text, sp), P)                      # every entry spans two lines
    perm = [2, 0, 1]
    Q = sw_io.parse_sw(text, [sp[t] for t in perm])
    assert np.array_equal(Q, P[np.ix_(perm, perm, perm)])                   # type order = the given species order
    # entries of elements not asked for are skipped; a subset of the species is enough
    sub = sw_io.parse_sw(text, ["Ge"])
    assert np.array_equal(sub[0, 0, 0], P[1, 1, 1])
    # comments anywhere, tokens spread over lines
    body = text.split("\n", 1)[1]
    odd = "# head\n" + body.replace("  ", "\n\n", 3).replace("\n        ", "   # tail comment\n ")
    assert np.array_equal(sw_io.parse_sw(odd, sp), P)


def test_parser_refuses_truncated_text():
    sp, P, text = so.three_species()
    with pytest.raises(ValueError, match="not a multiple of 14"):
        sw_io.parse_sw(text.replace("C C C", "# C C C", 1), sp)
    with pytest.raises(ValueError, match="not a multiple of 14"):
        sw_io.parse_sw("# nothing but a comment\n", sp)


def _entry_line(sp, i, j, k, vals):
    return f"{sp[i]} {sp[j]} {sp[k]} " + " ".join(repr(float(v)) for v in vals)


def _text_of(sp, P):
    n = len(sp)
    return "\n".join(_entry_line(sp, i, j, k, P[i, j, k]) for i in range(n) for j in range(n) for k in range(n)) + "\n"


def test_parser_names_the_missing_triplet():
    sp, P, _ = so.three_species()
    lines = _text_of(sp, P).strip().split("\n")
    lines = [l for l in lines if not l.startswith("Ge C Si ")]
    with pytest.raises(ValueError, match="lacks the entry Ge C Si"):
        sw_io.parse_sw("\n".join(lines), sp)


@pytest.mark.parametrize("field,value,match", [
    (1, 0.0, "Si Ge C: bad sig = 0.0"), (2, -1.8, "bad a = -1.8"), (0, 0.0, "bad eps"), (8, -4.0, "bad p = -4.0"),
    (9, -0.5, "bad q"), (3, float("nan"), "bad lambda"), (6, float("inf"), "bad A"), (10, -1.0, "bad tol"),
])
def test_parser_refuses_bad_numbers_by_name(field, value, match):
    sp, P, _ = so.three_species()
    Q = P.copy()
    Q[0, 1, 2, field] = value
    Q[0, 2, 1, field] = value      # keep the (i,j,k) / (i,k,j) symmetry: the value itself is what is refused
    with pytest.raises(ValueError, match=match.replace("(", r"\(")):
        sw_io.parse_sw(_text_of(sp, Q), sp)
    with pytest.raises(ValueError, match="bad"):
        sw_io.check_params(Q, sp)


def test_parser_refuses_words_where_numbers_belong():
    sp, P, _ = so.three_species()
    text = _text_of(sp, P).replace(repr(float(P[2, 2, 2, 3])), "lots", 1)
    with pytest.raises(ValueError, match="bad number 'lots' for lambda"):
        sw_io.parse_sw(text, sp)


@pytest.mark.parametrize("field", [0, 3, 5])
def test_parser_refuses_order_dependent_three_body_columns(field):
    sp, P, _ = so.three_species()
    Q = P.copy()
    Q[1, 0, 2, field] *= 1.01
    with pytest.raises(ValueError, match=f"Ge Si C and Ge C Si differ in {sw_io.FIELD_NAMES[field]}"):
        sw_io.parse_sw(_text_of(sp, Q), sp)
    # the columns of the radial factors and the two-body term may differ between (i,j,k) and (i,k,j): they are not used there
    R = P.copy()
    R[1, 0, 2, 4] += 0.3
    sw_io.parse_sw(_text_of(sp, R), sp)


# The library's own parser (vssr_sw_create_from_text) and checks (vssr_sw_create): the input is checked before any device is
# touched, so bad input ends in VSSR_E_BADARG with a message here too.  In a child process: a crash must not take pytest down.
CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, ROOT); sys.path.insert(0, TESTS)
import numpy as np
import sw_oracle as so
from surface_sampling_amd import backend
L = backend.load_library()
sp, P, text = so.three_species()
arr = (C.c_char_p * 3)(*[s.encode() for s in sp])
def from_text(t, species=arr, n=3):
    h = C.c_void_p(None)
    rc = L.vssr_sw_create_from_text(0, t.encode() if isinstance(t, str) else t, n, species, C.byref(h))
    if rc == 0:
        L.vssr_destroy(h)
    return rc, (L.vssr_last_error(None) or b"").decode("utf-8", "replace")
def from_params(Q, n=3):
    h = C.c_void_p(None)
    Q = np.ascontiguousarray(Q, np.float64)
    rc = L.vssr_sw_create(0, n, Q.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
    if rc == 0:
        L.vssr_destroy(h)
    return rc, (L.vssr_last_error(None) or b"").decode("utf-8", "replace")
out = {}
out["good"] = from_text(text)
out["missing"] = from_text(text.replace("Ge C Si ", "Ge C Xx ", 1))   # an entry of another element: skipped
lines = text.split("\n")
out["truncated"] = from_text("\n".join(lines[:-2]))
out["word"] = from_text(text.replace(repr(float(P[2, 2, 2, 3])), "lots", 1))
Q = P.copy(); Q[0, 1, 2, 1] = 0.0; Q[0, 2, 1, 1] = 0.0
out["sig0"] = from_params(Q)
Q = P.copy(); Q[0, 0, 0, 8] = -4.0
out["pneg"] = from_params(Q)
Q = P.copy(); Q[1, 0, 2, 5] += 0.01
out["asym"] = from_params(Q)
Q = P.copy(); Q[2, 2, 2, 0] = float("nan")
out["nan"] = from_params(Q)
out["noname"] = from_text(text, (C.c_char_p * 3)(b"Si", b"", b"C"))
rng = np.random.default_rng(0)
fuzz = []
raw = text.encode()
for t in range(200):
    b = bytearray(raw)
    k = int(rng.integers(0, 4))
    if k == 0:
        b = b[:int(rng.integers(0, len(b)))]
    elif k == 1:
        for _ in range(int(rng.integers(1, 20))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(1, 256))
    elif k == 2:
        p = int(rng.integers(0, len(b)))
        b = b[:p] + b[p:p + 200] + b[p:]
    else:
        b = bytes(b).replace(b"e", b"e9999", 3)
    fuzz.append(from_text(bytes(b))[0])
out["fuzz"] = sorted(set(fuzz))
print("RESULT" + json.dumps(out))
'''


def test_library_parser_and_checks_refuse_bad_input_by_name():
    code = CHILD.replace("ROOT)", repr(ROOT) + ")", 1).replace("TESTS)", repr(os.path.join(ROOT, "tests")) + ")", 1)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.split("RESULT", 1)[1])
    assert out["good"][0] in (0, -2), out["good"]                 # parsed; -2: no HIP device on this machine
    for key, match in (("missing", "lacks the entry Ge C Si"), ("truncated", "not a multiple of 14"),
                       ("word", "bad number 'lots' for lambda"), ("sig0", "bad sig = 0"), ("pneg", "bad p = -4"),
                       ("asym", "differ in costheta0"), ("nan", "bad eps = nan"), ("noname", "species 1 has no name")):
        rc, msg = out[key]
        assert rc == -1 and match in msg, (key, rc, msg)
    assert set(out["fuzz"]) <= {-1, -2, 0}, out["fuzz"]           # never a crash, only codes


# -- the restatement against the literature ---------------------------------------------------------------------------------------
def test_restatement_reproduces_the_published_diamond_values():
    """E = -2 eps per atom at a0 = 2^(1/6) 4 sig / sqrt(3), zero forces, B = 101.4, C11 = 151.4, C12 = 76.4 GPa (+-0.2) from
    energies under +-1e-3 volumetric / uniaxial / biaxial strains (no internal displacements for these)."""
    P = so.si_params()
    assert so.SI_A0 == pytest.approx(5.430950, abs=1e-6)
    T, X, Cl = so.diamond_si(so.SI_A0)
    E0, ea, F = so.sw(P, T, X, Cl, [1, 1, 1])
    assert E0 / 8 == pytest.approx(-4.3366, abs=1e-9) and np.allclose(ea, -4.3366, atol=1e-9)
    assert np.abs(F).max() < 1e-12
    V0, h = np.linalg.det(Cl), 1e-3

    def d2(s):
        M = lambda e: np.eye(3) + np.diag(e * np.asarray(s, float))        # noqa: E731
        Ep, Em = (so.sw(P, T, X @ M(e), Cl @ M(e), [1, 1, 1])[0] for e in (h, -h))
        return (Ep + Em - 2.0 * E0) / h ** 2 / V0 * so.EV_A3_GPA

    B, C11, C11pC12 = d2([1, 1, 1]) / 9.0, d2([1, 0, 0]), d2([1, 1, 0]) / 2.0
    assert B == pytest.approx(101.4, abs=0.2) and C11 == pytest.approx(151.4, abs=0.2)
    assert C11pC12 - C11 == pytest.approx(76.4, abs=0.2)
    # the lattice-constant scan has its minimum at a0
    scan = [so.sw(P, *so.diamond_si(so.SI_A0 * (1 + s))[0:2], so.diamond_si(so.SI_A0 * (1 + s))[2], [1, 1, 1])[0]
            for s in (-0.01, -0.002, 0.0, 0.002, 0.01)]
    assert int(np.argmin(scan)) == 2


def _fd_forces(P, T, X, Cl, pbc, h=1e-5):
    fd = np.zeros_like(X)
    for k in range(len(X)):
        for x in range(3):
            Xp, Xm = X.copy(), X.copy()
            Xp[k, x] += h
            Xm[k, x] -= h
            fd[k, x] = -(so.sw(P, T, Xp, Cl, pbc)[0] - so.sw(P, T, Xm, Cl, pbc)[0]) / (2 * h)
    return fd


@pytest.mark.parametrize("which", ["rattled_si", "three_species", "slab"])
def test_restatement_forces_match_finite_differences(which):
    if which == "rattled_si":
        P = so.si_params()
        T, X, Cl = so.diamond_si(so.SI_A0)
        X = X + np.random.default_rng(1).normal(0, 0.12, X.shape)
        pbc = [1, 1, 1]
    elif which == "three_species":
        _, P, _ = so.three_species()
        T, X, Cl, pbc = so.dense_box(n=24, box=7.0, min_dist=2.0, seed=5, nt=3)
    else:
        P = so.si_params()
        Z, X, Cl, pbc, _ = so.si_slab()
        T = np.zeros(len(Z), np.int32)
        X = X + np.random.default_rng(2).normal(0, 0.05, X.shape)
        sel = np.argsort(X[:, 2])[-12:]                    # the top of the slab (FD on a subset keeps the test short)
    E, ea, F = so.sw(P, T, X, Cl, pbc)
    assert abs(ea.sum() - E) < 1e-10 * max(1.0, abs(E))
    fd = _fd_forces(P, T, X, Cl, pbc)
    if which == "slab":
        fd, F = fd[sel], F[sel]
    assert np.abs(fd - F).max() < 2e-7 * max(1.0, np.abs(F).max())
    assert np.abs(F).max() > 0.1


# -- LAMMPSSurfCalc on a Si(111)-tutorial-shaped run directory -------------------------------------------------------------------
SRS = "ThreeBodyCluster_SRS_StephensonRadnySmith_1996_Si__MO_604248666067_000"


def _si_run_dir(path, energy_model=so.SI_1985, opt_model=SRS, boundary="p p f", config=None):
    """A run directory shaped like the reference's tutorials/Si_111_5x5 one (KIM pair styles, no potential_file, bulk_index 75);
    only the lines this backend reads are meaningful."""
    path.mkdir(parents=True, exist_ok=True)
    cfg = config or {"atoms": ["Si"], "atomic_numbers_dict": {"1": 14}, "bulk_index": 75}
    (path / "lammps_config.json").write_text(json.dumps(cfg))
    head = f"units metal\n# kim_init {energy_model} metal\nboundary         {boundary}\nread_data {{}}\ngroup bulk id <= {{}}\n"
    (path / "lammps_energy_template.txt").write_text(
        head + f"# kim_interactions Si\npair_style kim {energy_model}\n# pair_coeff * * /path/to/potential Atom1 Atom2 {{}}\n"
        "pair_coeff * * {}\nrun 0\nwrite_data {}\n")
    (path / "lammps_opt_template.txt").write_text(
        head + f"pair_style kim {opt_model}\npair_coeff * * {{}}\nfix 2 bulk setforce 0.0 0.0 0.0\nmin_style cg\n"
        "minimize 1e-3 1e-3 {} 10000\nwrite_data {}\n")
    return path


def _si_structure():
    from surface_sampling_amd.structures import Structure

    Z, X, Cl, pbc, _ = so.si_slab()
    return Structure(Z, X, Cl, pbc)


def test_lammps_surf_calc_picks_sw_for_the_si_kim_run_directory(tmp_path):
    rd = _si_run_dir(tmp_path / "si")
    calc = calcs.LAMMPSSurfCalc()
    calc.set(calc_name="LAMMPS", optimizer="LAMMPS", relax_steps=50, run_dir=rd, kim_potential=True)
    calc._configure()
    assert calc.pair_style == "kim" and calc.kim_model == so.SI_1985 and calc.species == ["Si"] and calc.bulk_index == 75
    assert np.array_equal(calc.params, so.si_params())
    s = _si_structure()
    s.pbc = np.array([True, True, True])              # the template's boundary decides, not the atoms' flags
    types, pos, cell, pbc = calc._pack(s)
    assert pbc.tolist() == [1, 1, 0] and set(types.tolist()) == {0}
    assert calc.relax_refused == SRS
    for call in (lambda: calc.run_lammps_opt(s), lambda: calc.relax_batch([s, s]),
                 lambda: calc.evaluate_packed([len(s)], s.numbers, s.positions, s.cell.reshape(1, 9), s.pbc.reshape(1, 3),
                                              relax=True)):
        with pytest.raises(backend.BackendError, match=SRS):
            call()
    # boundary spellings
    for bnd, want in (("p p p", [1, 1, 1]), ("p s m", [1, 0, 0]), ("fs p p", [0, 1, 1])):
        c = calcs.LAMMPSSurfCalc()
        c.set(run_dir=_si_run_dir(tmp_path / bnd.replace(" ", "_"), boundary=bnd))
        assert c._pack(s)[3].tolist() == want
    # the same model in both templates: relaxations are not refused
    same = calcs.LAMMPSSurfCalc()
    same.set(run_dir=_si_run_dir(tmp_path / "same", opt_model=so.SI_1985))
    same._configure()
    assert same.relax_refused is None


def test_lammps_surf_calc_pair_style_sw_with_a_potential_file(tmp_path):
    sp, P, text = so.three_species()
    rd = tmp_path / "sw"
    rd.mkdir()
    (rd / "SiGeC.sw").write_text(text)
    (rd / "lammps_config.json").write_text(json.dumps({"potential_file": "SiGeC.sw", "atoms": ["C", "Si"], "bulk_index": 4}))
    body = "units metal\nboundary p f p\nread_data {}\ngroup bulk id <= {}\npair_style sw\npair_coeff * * {} {} {}\n"
    (rd / "lammps_energy_template.txt").write_text(body + "run 0\n")
    (rd / "lammps_opt_template.txt").write_text(body + "minimize 1e-5 1e-5 {} 10000\n")
    calc = calcs.LAMMPSSurfCalc()
    calc.set(run_dir=rd)
    calc._configure()
    assert calc.pair_style == "sw" and calc.species == ["C", "Si"] and calc.relax_refused is None
    assert np.array_equal(calc.params, P[np.ix_([2, 0], [2, 0], [2, 0])])
    assert calc.boundary.tolist() == [1, 0, 1]
    (rd / "lammps_config.json").write_text(json.dumps({"atoms": ["Si"], "bulk_index": 4}))
    os.utime(rd / "lammps_config.json", (1, 1))
    with pytest.raises(KeyError, match="potential_file"):
        _configure_fresh(rd)


def _configure_fresh(rd):
    c = calcs.LAMMPSSurfCalc()
    c.set(run_dir=rd)
    c._configure()


def test_unknown_kim_models_still_raise_by_name(tmp_path):
    rd = _si_run_dir(tmp_path / "srs", energy_model=SRS)
    with pytest.raises(backend.BackendError, match=SRS):
        _configure_fresh(rd)
    # kim_potential set while the template names no KIM model
    rd2 = tmp_path / "flag"
    rd2.mkdir()
    (rd2 / "lammps_config.json").write_text(json.dumps({"potential_file": "x.tersoff", "atoms": ["Si"], "bulk_index": 1}))
    (rd2 / "lammps_energy_template.txt").write_text("pair_style tersoff\n")
    c = calcs.LAMMPSSurfCalc()
    c.set(run_dir=rd2, kim_potential=True)
    with pytest.raises(backend.BackendError, match="KIM model"):
        c._configure()
    # a KIM model whose species do not cover the run directory's atoms
    rd3 = _si_run_dir(tmp_path / "ge", config={"atoms": ["Si", "Ge"], "bulk_index": 1})
    with pytest.raises(ValueError, match="covers"):
        _configure_fresh(rd3)


def test_sw_surf_calc_accepts_every_potential_spelling(tmp_path):
    sp, P, text = so.three_species()
    (tmp_path / "x.sw").write_text(text)
    for pot, species in ((so.SI_1985, None), (text, sp), (str(tmp_path / "x.sw"), sp), (P, sp)):
        c = calcs.SWSurfCalc(pot, species)
        assert c.params.shape[-1] == 11 and c._engine is None
    assert calcs.SWSurfCalc(so.SI_1985).species == ["Si"] and not calcs.SWSurfCalc(so.SI_1985).all_periodic
    with pytest.raises(ValueError):
        calcs.SWSurfCalc(P)                              # an array needs its species
    bad = P.copy()
    bad[0, 1, 2, 3] += 1.0
    with pytest.raises(ValueError, match="differ in lambda"):
        calcs.SWSurfCalc(bad, sp)
