"""LAMMPS ``pair_style eam`` / ``eam/alloy`` / ``eam/fs`` / ``adp`` potential files (host side, data formats only).

The reference hands ``mcmc/potentials/Cu_u3.eam`` to LAMMPS through ``LAMMPSRunSurfCalc.set(pair_style="eam",
pair_coeff=["* * Cu_u3.eam"])`` (``tests/test_Cu.py:41,65-70``, ``tutorials/example.ipynb`` cell 3).  Layout of a funcfl
file: line 1 comment; line 2 ``Z mass lattice-constant lattice-type``; line 3 ``Nrho drho Nr dr cutoff``; then ``Nrho``
values of the embedding energy F(rho) [eV], ``Nr`` values of the effective charge Z(r) [sqrt(Hartree Bohr)] and ``Nr``
values of the electron density rho(r), free format.

Several elements (``setfl``, ``eam/alloy``; ``eam/fs``; funcfl files mixed per type as LAMMPS ``pair_coeff i i file``) end in one
:class:`EamTables`: the typed arrays of ``vssr_eam_create_alloy`` on one common grid (restated from LAMMPS ``pair_eam.cpp``,
``pair_eam_alloy.cpp``, ``pair_eam_fs.cpp`` ``read_file`` / ``file2array``).

An ``adp`` file (restated from the LAMMPS documentation of ``pair_style adp``) is a setfl file followed, after the r * phi blocks,
by one u(r) block per element pair and then one w(r) block per element pair, in the same lower-triangle order, ``Nr`` values
each and NOT scaled by r: the ``u`` / ``w`` fields of :class:`Setfl` and :class:`EamTables`, ``None`` for the other styles.
"""

from __future__ import annotations

import dataclasses

import numpy as np


@dataclasses.dataclass
class Funcfl:
    atomic_number: int
    mass: float
    lattice_constant: float
    lattice: str
    nrho: int
    drho: float
    nr: int
    dr: float
    cutoff: float
    frho: np.ndarray
    zr: np.ndarray
    rhor: np.ndarray
    comment: str = ""


def parse_funcfl(text: str) -> Funcfl:
    lines = text.splitlines()
    if len(lines) < 4:
        raise ValueError("funcfl file: too short")
    head = lines[1].split()
    grid = lines[2].split()
    if len(head) < 3 or len(grid) < 5:
        raise ValueError("funcfl file: malformed header")
    nrho, drho, nr, dr, cutoff = int(grid[0]), float(grid[1]), int(grid[2]), float(grid[3]), float(grid[4])
    vals = np.array(" ".join(lines[3:]).split(), dtype=np.float64)
    if vals.size < nrho + 2 * nr:
        raise ValueError(f"funcfl file: {vals.size} table values, need {nrho + 2 * nr}")
    if nrho < 5 or nr < 5 or not (drho > 0 and dr > 0 and cutoff > 0):
        raise ValueError("funcfl file: bad grid")
    return Funcfl(int(float(head[0])), float(head[1]), float(head[2]), head[3] if len(head) > 3 else "",
                  nrho, drho, nr, dr, cutoff, vals[:nrho].copy(), vals[nrho:nrho + nr].copy(),
                  vals[nrho + nr:nrho + 2 * nr].copy(), lines[0].strip())


def read_funcfl(path) -> Funcfl:
    with open(path) as fh:
        return parse_funcfl(fh.read())


# ---- several elements -------------------------------------------------------------------------------------------------------
HARTREE_BOHR = 27.2 * 0.529   # funcfl Z(r) Z(r) -> r * phi in eV A (pair_eam.cpp)


@dataclasses.dataclass
class Setfl:
    """A setfl file (``eam/alloy``) or its Finnis-Sinclair variant (``fs=True``).  ``rhor``: [N][Nr] (alloy) or [N][N][Nr]
    (fs: block I, entry J = the density an atom of element I contributes at a site of element J); ``z2r``: [N (N + 1) / 2][Nr]
    r * phi in eV A of the pairs (1,1), (2,1), (2,2), (3,1), ... (lower triangle, file order)."""
    elements: list
    atomic_numbers: list
    masses: list
    lattice_constants: list
    lattices: list
    nrho: int
    drho: float
    nr: int
    dr: float
    cutoff: float
    frho: np.ndarray
    rhor: np.ndarray
    z2r: np.ndarray
    fs: bool = False
    comments: tuple = ("", "", "")
    u: np.ndarray | None = None   # adp: [N (N + 1) / 2][Nr] dipole function u(r) of the pairs, in the order of z2r
    w: np.ndarray | None = None   # adp: likewise the quadrupole function w(r)


@dataclasses.dataclass
class EamTables:
    """What the device evaluates: one grid and per-TYPE tables (LAMMPS type order).  ``frho`` [n][nrho]; ``rhor`` [n][nr]
    (alloy) or [n * n][nr] (fs: row a * n + b = density of type a at a site of type b); ``z2r`` [n (n + 1) / 2][nr] (r * phi,
    pair (a, b) at max(a,b) (max(a,b) + 1) / 2 + min(a,b)); ``elements``: element symbol of every type."""
    elements: list
    fs: bool
    nrho: int
    drho: float
    nr: int
    dr: float
    cutoff: float
    frho: np.ndarray
    rhor: np.ndarray
    z2r: np.ndarray
    u: np.ndarray | None = None   # adp: [n (n + 1) / 2][nr] in the pair order of z2r (vssr_eam_create_adp), else None
    w: np.ndarray | None = None


def pair_index(a: int, b: int) -> int:
    hi, lo = max(a, b), min(a, b)
    return hi * (hi + 1) // 2 + lo


class _Lines:
    """LAMMPS PotentialFileReader: header lines are read whole, tables fill from as many lines as they need (values left over
    on a table's last line are dropped, as there)."""

    def __init__(self, text, what):
        self.lines = text.splitlines()
        self.k = 0
        self.what = what

    def line(self):
        while self.k < len(self.lines):
            ln = self.lines[self.k]
            self.k += 1
            if ln.strip():
                return ln.split()
        raise ValueError(f"{self.what}: file ends early")

    def values(self, n):
        out = []
        while len(out) < n:
            out.extend(self.line()[:n - len(out)])
        try:
            v = np.array(out, dtype=np.float64)
        except ValueError:
            raise ValueError(f"{self.what}: bad number in a table") from None
        if not np.isfinite(v).all():
            raise ValueError(f"{self.what}: non-finite table value")
        return v


def parse_setfl(text: str, fs: bool = False) -> Setfl:
    return _parse_setfl(text, "eam/fs file" if fs else "setfl file", fs=fs)


def parse_adp(text: str) -> Setfl:
    """An ``adp`` file: the setfl blocks, then u(r) and w(r) of every element pair (``Setfl.u`` / ``Setfl.w``)."""
    return _parse_setfl(text, "adp file", adp=True)


def _parse_setfl(text, what, fs=False, adp=False):
    rd = _Lines(text, what)
    lines = text.splitlines()
    if len(lines) < 5:
        raise ValueError(f"{what}: too short")
    comments = tuple(ln.rstrip("\n") for ln in lines[:3])
    rd.k = 3
    head = rd.line()
    try:
        n = int(head[0])
    except ValueError:
        raise ValueError(f"{what}: line 4 must be 'N el1 ... elN'") from None
    if n < 1 or len(head) != n + 1:
        raise ValueError(f"{what}: line 4 announces {head[0]} elements and lists {len(head) - 1}")
    elements = head[1:]
    grid = rd.line()
    if len(grid) < 5:
        raise ValueError(f"{what}: malformed grid line")
    try:
        nrho, drho, nr, dr, cutoff = int(grid[0]), float(grid[1]), int(grid[2]), float(grid[3]), float(grid[4])
    except ValueError:
        raise ValueError(f"{what}: malformed grid line") from None
    if nrho < 5 or nr < 5 or not (np.isfinite([drho, dr, cutoff]).all() and drho > 0 and dr > 0 and cutoff > 0):
        raise ValueError(f"{what}: bad grid")
    zs, masses, lats, ltypes = [], [], [], []
    frho = np.zeros((n, nrho))
    rhor = np.zeros((n, n, nr) if fs else (n, nr))
    for i in range(n):
        h = rd.line()
        if len(h) < 2:
            raise ValueError(f"{what}: malformed header of element {elements[i]}")
        try:
            zs.append(int(float(h[0])))
            masses.append(float(h[1]))
            lats.append(float(h[2]) if len(h) > 2 else 0.0)
        except ValueError:
            raise ValueError(f"{what}: malformed header of element {elements[i]}") from None
        ltypes.append(h[3] if len(h) > 3 else "")
        frho[i] = rd.values(nrho)
        if fs:
            for j in range(n):
                rhor[i, j] = rd.values(nr)
        else:
            rhor[i] = rd.values(nr)
    z2r = np.zeros((n * (n + 1) // 2, nr))
    for p in range(len(z2r)):
        z2r[p] = rd.values(nr)
    u = w = None
    if adp:
        u, w = np.zeros_like(z2r), np.zeros_like(z2r)
        for tab in (u, w):
            for p in range(len(tab)):
                tab[p] = rd.values(nr)
    return Setfl(list(elements), zs, masses, lats, ltypes, nrho, drho, nr, dr, cutoff, frho, rhor, z2r, bool(fs), comments, u, w)


def read_setfl(path, fs: bool = False) -> Setfl:
    with open(path) as fh:
        return parse_setfl(fh.read(), fs=fs)


def read_adp(path) -> Setfl:
    with open(path) as fh:
        return parse_adp(fh.read())


def write_adp(setfl: Setfl, path=None) -> str:
    """The text of an ``adp`` file: ``write_setfl`` followed by the u and the w blocks (``setfl.u`` / ``setfl.w`` are required)."""
    n = len(setfl.elements)
    if setfl.fs or setfl.u is None or setfl.w is None:
        raise ValueError("adp file: needs alloy densities and the u and w tables")
    if np.shape(setfl.u) != (n * (n + 1) // 2, setfl.nr) or np.shape(setfl.w) != (n * (n + 1) // 2, setfl.nr):
        raise ValueError("adp file: u and w must be [N (N + 1) / 2][Nr]")
    return _write(_setfl_lines(setfl) + _table_lines(setfl.u) + _table_lines(setfl.w), path)


def write_setfl(setfl: Setfl, path=None) -> str:
    """The text of ``setfl`` (values as ``%.16e``, five per line, so that parse_setfl gives back the same doubles); also
    written to ``path`` when given."""
    return _write(_setfl_lines(setfl), path)


def _write(lines, path):
    text = "\n".join(lines) + "\n"
    if path is not None:
        with open(path, "w") as fh:
            fh.write(text)
    return text


def _table_lines(tables):
    """One block per row of ``tables``, five values per line."""
    out = []
    for v in tables:
        v = np.asarray(v, np.float64).reshape(-1)
        out += ["".join(f" {x:.16e}" for x in v[k:k + 5]).strip() for k in range(0, len(v), 5)]
    return out


def _setfl_lines(setfl):
    def table(v):
        return _table_lines([v])

    n = len(setfl.elements)
    out = [str(c) for c in (list(setfl.comments) + ["", "", ""])[:3]]
    out.append(" ".join([str(n), *setfl.elements]))
    out.append(f"{setfl.nrho} {setfl.drho:.16e} {setfl.nr} {setfl.dr:.16e} {setfl.cutoff:.16e}")
    for i in range(n):
        lt = setfl.lattices[i] if setfl.lattices[i] else "fcc"
        out.append(f"{setfl.atomic_numbers[i]} {setfl.masses[i]:.16e} {setfl.lattice_constants[i]:.16e} {lt}")
        out += table(setfl.frho[i])
        if setfl.fs:
            for j in range(n):
                out += table(setfl.rhor[i][j])
        else:
            out += table(setfl.rhor[i])
    return out + _table_lines(setfl.z2r)


def funcfl_to_setfl(f: Funcfl, element: str | None = None) -> Setfl:
    """One funcfl file as a one-element setfl on the file's own grid: F and rho as they are, r * phi = 27.2 * 0.529 * Z^2."""
    from .structures import SYMBOLS

    el = element or SYMBOLS[f.atomic_number]
    return Setfl([el], [f.atomic_number], [f.mass], [f.lattice_constant], [f.lattice or "fcc"], f.nrho, f.drho, f.nr, f.dr,
                 f.cutoff, f.frho[None, :].copy(), f.rhor[None, :].copy(), (HARTREE_BOHR * f.zr ** 2)[None, :],
                 False, (f.comment, "converted from funcfl", ""))


def _check_names(names, what):
    if not names:
        raise ValueError(f"{what}: pair_coeff names no element")
    if len(names) > 8:
        raise ValueError(f"{what}: {len(names)} types (at most 8 are supported)")
    if any(str(x).upper() == "NULL" for x in names):
        raise ValueError(f"{what}: NULL types (pair_style hybrid) are not supported")


def tables_from_adp(setfl: Setfl, elements) -> EamTables:
    """``tables_from_setfl`` for a parsed ``adp`` file: the tables carry ``u`` / ``w`` of the chosen types."""
    if setfl.fs or setfl.u is None or setfl.w is None:
        raise ValueError("adp: the file holds no u and w tables (parse it with parse_adp)")
    return _tables(setfl, elements, "adp", True)


def tables_from_setfl(setfl: Setfl, elements) -> EamTables:
    """LAMMPS ``pair_coeff * * file el_1 ... el_n``: type t is element ``elements[t]`` of the file."""
    return _tables(setfl, elements, "eam/fs" if setfl.fs else "eam/alloy", False)


def _tables(setfl, elements, what, adp):
    names = [str(x) for x in elements]
    _check_names(names, what)
    idx = []
    for x in names:
        if x not in setfl.elements:
            raise ValueError(f"{what}: element {x!r} is not in the potential file (it has {setfl.elements})")
        idx.append(setfl.elements.index(x))
    n = len(idx)
    frho = np.stack([setfl.frho[a] for a in idx])
    if setfl.fs:
        rhor = np.stack([setfl.rhor[a][b] for a in idx for b in idx])
    else:
        rhor = np.stack([setfl.rhor[a] for a in idx])
    pairs = [pair_index(idx[a], idx[b]) for a in range(n) for b in range(a + 1)]
    z2r = np.stack([setfl.z2r[k] for k in pairs])
    u, w = (np.stack([t[k] for k in pairs]) for t in (setfl.u, setfl.w)) if adp else (None, None)
    return EamTables(names, setfl.fs, setfl.nrho, setfl.drho, setfl.nr, setfl.dr, setfl.cutoff, frho, rhor, z2r, u, w)


def _lagrange(f, delta_file, n_file, x):
    """LAMMPS file2array's 4-point Lagrange resampling of a 1-based table f[1..n_file] (numpy f[0..n_file-1]) at x."""
    p = np.asarray(x, np.float64) / delta_file + 1.0
    k = p.astype(np.int64)
    k = np.maximum(np.minimum(k, n_file - 2), 2)
    p = np.minimum(p - k, 2.0)
    sixth = 1.0 / 6.0
    c1 = -sixth * p * (p - 1.0) * (p - 2.0)
    c2 = 0.5 * (p * p - 1.0) * (p - 2.0)
    c3 = -0.5 * p * (p + 1.0) * (p - 2.0)
    c4 = sixth * p * (p * p - 1.0)
    f = np.asarray(f, np.float64)
    return c1 * f[k - 2] + c2 * f[k - 1] + c3 * f[k] + c4 * f[k + 1]


def tables_from_funcfl(files) -> EamTables:
    """LAMMPS ``pair_style eam`` with ``pair_coeff t t file_t`` for every type t (``files``: one :class:`Funcfl` per type):
    ``file2array`` for several files -- the largest dr / drho and r / rho ranges, every table resampled onto that grid with the
    4-point Lagrange formula, r * phi_ab = 27.2 * 0.529 Z_a(r) Z_b(r), cutoff = the largest file cutoff.  The element of a type
    is its file's atomic number."""
    from .structures import SYMBOLS

    files = list(files)
    if not files:
        raise ValueError("eam: no funcfl file")
    if len(files) > 8:
        raise ValueError(f"eam: {len(files)} types (at most 8 are supported)")
    dr = max(f.dr for f in files)
    drho = max(f.drho for f in files)
    rmax = max((f.nr - 1) * f.dr for f in files)
    rhomax = max((f.nrho - 1) * f.drho for f in files)
    nr = int(rmax / dr + 0.5)
    nrho = int(rhomax / drho + 0.5)
    if nr < 5 or nrho < 5:
        raise ValueError("eam: common grid too small")
    r = np.arange(nr) * dr
    rho = np.arange(nrho) * drho
    frho = np.stack([_lagrange(f.frho, f.drho, f.nrho, rho) for f in files])
    rhor = np.stack([_lagrange(f.rhor, f.dr, f.nr, r) for f in files])
    zr = [_lagrange(f.zr, f.dr, f.nr, r) for f in files]
    n = len(files)
    z2r = np.stack([HARTREE_BOHR * zr[a] * zr[b] for a in range(n) for b in range(a + 1)])
    return EamTables([SYMBOLS[f.atomic_number] for f in files], False, nrho, drho, nr, dr, max(f.cutoff for f in files),
                     frho, rhor, z2r)
