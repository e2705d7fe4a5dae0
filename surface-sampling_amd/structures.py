"""Plain-array slab structures: the minimal stand-in for ``ase.Atoms`` on the hot path.

The calculators accept anything exposing ``get_positions()``, ``get_atomic_numbers()``,
``get_cell()`` and ``get_pbc()`` (``ase.Atoms`` does; ASE itself is optional).  This
module also reads the reference's structure files without ase/catkit
(SURVEY.md Appendix B): ASE-written P1 CIFs (``tests/data/SrTiO3_001/*.cif``) and the
pickled ``catkit.gratoms.Gratoms`` slabs (``tutorials/data/*/*.pkl``), and builds the
synthetic benchmark inputs of SURVEY.md §8(d).
"""

from __future__ import annotations

import io
import pickle
from dataclasses import dataclass, field

import numpy as np

SYMBOLS = (
    "X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn "
    "Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr "
    "Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra "
    "Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm"
).split()
ATOMIC_NUMBERS = {s: z for z, s in enumerate(SYMBOLS)}

# Standard atomic weights in amu, indexed by atomic number (IUPAC abridged values; an element without one carries the mass of its
# longest-lived isotope; index 0, the dummy "X", is 1).  What molecular dynamics takes when neither the caller nor the Atoms object
# supplies masses (``masses_of``).
ATOMIC_MASSES = np.array([
    1.0, 1.008, 4.002602, 6.94, 9.0121831, 10.81, 12.011, 14.007, 15.999, 18.998403163, 20.1797, 22.98976928, 24.305, 26.9815385,
    28.085, 30.973761998, 32.06, 35.45, 39.948, 39.0983, 40.078, 44.955908, 47.867, 50.9415, 51.9961, 54.938044, 55.845, 58.933194,
    58.6934, 63.546, 65.38, 69.723, 72.630, 74.921595, 78.971, 79.904, 83.798, 85.4678, 87.62, 88.90584, 91.224, 92.90637, 95.95,
    97.90721, 101.07, 102.90550, 106.42, 107.8682, 112.414, 114.818, 118.710, 121.760, 127.60, 126.90447, 131.293, 132.90545196,
    137.327, 138.90547, 140.116, 140.90766, 144.242, 144.91276, 150.36, 151.964, 157.25, 158.92535, 162.500, 164.93033, 167.259,
    168.93422, 173.054, 174.9668, 178.49, 180.94788, 183.84, 186.207, 190.23, 192.217, 195.084, 196.966569, 200.592, 204.38, 207.2,
    208.98040, 208.98243, 209.98715, 222.01758, 223.01974, 226.02541, 227.02775, 232.0377, 231.03588, 238.02891, 237.04817,
    244.06421, 243.06138, 247.07035, 247.07031, 251.07959, 252.0830, 257.09511])
assert len(ATOMIC_MASSES) == len(SYMBOLS)


def masses_of(atoms, masses=None) -> np.ndarray:
    """Masses [N] in amu of an Atoms-like: ``masses`` where given, else ``atoms.get_masses()`` where the object has it, else the
    standard atomic weights of its atomic numbers.  ``ValueError`` for a wrong length or a mass that is not finite and positive."""
    if masses is not None:
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
    elif hasattr(atoms, "get_masses"):
        m = np.asarray(atoms.get_masses(), dtype=np.float64).reshape(-1)
    else:
        m = ATOMIC_MASSES[np.asarray(atoms.get_atomic_numbers(), dtype=np.int64)]
    if len(m) != len(atoms):
        raise ValueError(f"{len(m)} masses for {len(atoms)} atoms")
    if not (np.isfinite(m).all() and (m > 0).all()):
        raise ValueError("masses must be finite and positive")
    return np.ascontiguousarray(m, dtype=np.float64)


@dataclass
class Structure:
    """Positions [N,3] (Å, float64), atomic numbers [N], cell [3,3] (rows = lattice vectors), pbc [3]."""

    numbers: np.ndarray
    positions: np.ndarray
    cell: np.ndarray
    pbc: np.ndarray = field(default_factory=lambda: np.array([True, True, True]))
    constraints_fixed: np.ndarray | None = None  # indices held by FixAtoms, if any
    info: dict = field(default_factory=dict)

    def __post_init__(self):
        self.numbers = np.ascontiguousarray(self.numbers, dtype=np.int32)
        self.positions = np.ascontiguousarray(self.positions, dtype=np.float64).reshape(-1, 3)
        self.cell = np.ascontiguousarray(self.cell, dtype=np.float64).reshape(3, 3)
        self.pbc = np.ascontiguousarray(self.pbc, dtype=bool).reshape(3)
        if len(self.numbers) != len(self.positions):
            raise ValueError("numbers and positions differ in length")
        self.results: dict = {}
        self.calc = None

    # --- the subset of the ase.Atoms surface the calculators use -------------------------
    def __len__(self):
        return len(self.numbers)

    def get_positions(self):
        return self.positions.copy()

    def set_positions(self, pos):
        self.positions = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)

    def get_atomic_numbers(self):
        return self.numbers.copy()

    def get_chemical_symbols(self):
        return [SYMBOLS[z] for z in self.numbers]

    def get_cell(self):
        return self.cell.copy()

    def get_pbc(self):
        return self.pbc.copy()

    def get_potential_energy(self):
        return self.calc.get_potential_energy(self)

    def get_forces(self):
        return self.calc.get_forces(self)

    def copy(self):
        s = Structure(self.numbers.copy(), self.positions.copy(), self.cell.copy(), self.pbc.copy(),
                      None if self.constraints_fixed is None else self.constraints_fixed.copy(),
                      dict(self.info))
        return s

    def formula_counts(self) -> dict:
        out: dict[str, int] = {}
        for z in self.numbers:
            out[SYMBOLS[z]] = out.get(SYMBOLS[z], 0) + 1
        return out

    def repeat(self, reps) -> "Structure":
        """Tile the cell (like ``ase.Atoms.repeat``): image-major ordering, i0 slowest."""
        reps = tuple(int(r) for r in reps)
        pos, num = [], []
        for i0 in range(reps[0]):
            for i1 in range(reps[1]):
                for i2 in range(reps[2]):
                    shift = i0 * self.cell[0] + i1 * self.cell[1] + i2 * self.cell[2]
                    pos.append(self.positions + shift)
                    num.append(self.numbers)
        cell = self.cell * np.array(reps)[:, None]
        return Structure(np.concatenate(num), np.concatenate(pos), cell, self.pbc.copy())


def as_arrays(atoms):
    """(numbers int32 [N], positions f64 [N,3], cell f64 [3,3], pbc uint8 [3]) from Atoms-like."""
    numbers = np.ascontiguousarray(atoms.get_atomic_numbers(), dtype=np.int32)
    positions = np.ascontiguousarray(atoms.get_positions(), dtype=np.float64).reshape(-1, 3)
    cell = np.ascontiguousarray(np.asarray(atoms.get_cell()), dtype=np.float64).reshape(3, 3)
    pbc = np.ascontiguousarray(np.asarray(atoms.get_pbc()), dtype=np.uint8).reshape(3)
    return numbers, positions, cell, pbc


# --------------------------------------------------------------------------------------
# Bands of images for the nudged elastic band (backend.neb, calculators.neb_batch)
# --------------------------------------------------------------------------------------
def wrap_displacements(d, cell, pbc) -> np.ndarray:
    """Displacements [N, 3] taken to the nearest image along the periodic axes, by the rule of ``vssr_batch_neb``: with
    s = d cell^-1, the whole lattice vectors rint(s_a) are subtracted for every periodic axis a.  This is the minimum image while every
    atom moves less than half the smallest periodic cell height; it is no full minimum-image search over skewed cells."""
    d = np.array(d, dtype=np.float64).reshape(-1, 3)
    pbc = np.asarray(pbc).astype(bool).reshape(3)
    if not pbc.any():
        return d
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    n = np.rint(d @ np.linalg.inv(cell))
    n[:, ~pbc] = 0.0
    return d - n @ cell


def interpolate_band(initial, final, n_images: int, mic: bool = True) -> list:
    """``n_images`` >= 3 copies of ``initial`` from its positions to those of ``final`` (both ends included), linear in the
    displacement; ``mic`` wraps the displacement by :func:`wrap_displacements` first, so an atom that crosses a periodic face goes
    the short way.  The images keep the cell, pbc and species of ``initial``; the last image holds ``final`` minus the whole lattice
    vectors the wrap took off (``final`` itself, bit for bit, where no atom wrapped)."""
    n_images = int(n_images)
    if n_images < 3:
        raise ValueError(f"interpolate_band: {n_images} images (>= 3 wanted)")
    if len(initial) != len(final) or not np.array_equal(np.asarray(initial.get_atomic_numbers()), np.asarray(final.get_atomic_numbers())):
        raise ValueError("interpolate_band: the end images differ in their atoms")
    x0 = np.asarray(initial.get_positions(), dtype=np.float64).reshape(-1, 3)
    x1 = np.asarray(final.get_positions(), dtype=np.float64).reshape(-1, 3)
    d = x1 - x0
    if mic:
        raw = d
        d = wrap_displacements(raw, initial.get_cell(), initial.get_pbc())
        x1 = x1 - (raw - d)
    out = []
    for i in range(n_images):
        img = initial.copy()
        img.set_positions(x1 if i == n_images - 1 else x0 + d * (i / (n_images - 1)))
        out.append(img)
    return out


def band_path(positions, cell, pbc) -> np.ndarray:
    """The reaction coordinate of a band: cumulative |d(i)| [n] in A over images ``positions`` [n, N, 3], with the displacements
    wrapped as ``vssr_batch_neb`` wraps them and |d| over all atoms and components."""
    x = np.asarray(positions, dtype=np.float64)
    out = np.zeros(len(x))
    for i in range(len(x) - 1):
        d = wrap_displacements(x[i + 1] - x[i], cell, pbc)
        out[i + 1] = out[i] + np.sqrt(np.vdot(d, d))
    return out


# --------------------------------------------------------------------------------------
# CIF (ASE-written, P1, orthorhombic or general angles)
# --------------------------------------------------------------------------------------
def read_cif(path: str) -> Structure:
    a = b = c = None
    alpha = beta = gamma = 90.0
    cols: list[str] = []
    rows: list[list[str]] = []
    in_loop = False
    in_atom_loop = False
    with open(path) as fh:
        for raw in fh:
            line = raw.strip()
            if not line or line.startswith("#"):
                if in_atom_loop and rows:
                    in_atom_loop = False
                continue
            if line.startswith("_cell_length_a"):
                a = float(line.split()[1])
            elif line.startswith("_cell_length_b"):
                b = float(line.split()[1])
            elif line.startswith("_cell_length_c"):
                c = float(line.split()[1])
            elif line.startswith("_cell_angle_alpha"):
                alpha = float(line.split()[1])
            elif line.startswith("_cell_angle_beta"):
                beta = float(line.split()[1])
            elif line.startswith("_cell_angle_gamma"):
                gamma = float(line.split()[1])
            elif line == "loop_":
                in_loop, in_atom_loop, cols = True, False, []
            elif in_loop and line.startswith("_"):
                cols.append(line.split()[0])
                in_atom_loop = any(cn.startswith("_atom_site_") for cn in cols)
            elif in_loop and in_atom_loop and "_atom_site_fract_x" in cols:
                parts = line.split()
                if len(parts) >= len(cols):
                    rows.append(parts)
            else:
                in_loop = False
    if a is None or not rows:
        raise ValueError(f"{path}: no cell or atom loop found")
    ca, cb, cg = (np.cos(np.deg2rad(x)) for x in (alpha, beta, gamma))
    sg = np.sin(np.deg2rad(gamma))
    if alpha == beta == gamma == 90.0:
        cell = np.diag([a, b, c])
    else:
        cx = c * cb
        cy = c * (ca - cb * cg) / sg
        cz = np.sqrt(max(c * c - cx * cx - cy * cy, 0.0))
        cell = np.array([[a, 0, 0], [b * cg, b * sg, 0], [cx, cy, cz]])
    isym = cols.index("_atom_site_type_symbol")
    ix, iy, iz = (cols.index(f"_atom_site_fract_{k}") for k in "xyz")
    numbers = [ATOMIC_NUMBERS[r[isym]] for r in rows]
    frac = np.array([[float(r[ix]), float(r[iy]), float(r[iz])] for r in rows])
    return Structure(np.array(numbers), frac @ cell, cell, np.array([True, True, True]))


# --------------------------------------------------------------------------------------
# catkit Gratoms / ase Atoms pickles, decoded with inert stubs (never executed)
# --------------------------------------------------------------------------------------
class _PStub:
    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)
        else:
            self._state = state


class _SlabUnpickler(pickle.Unpickler):
    _NUMPY_OK = {
        ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
        ("numpy", "ndarray"), ("numpy", "dtype"),
        ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
    }

    def find_class(self, module, name):
        if (module, name) in self._NUMPY_OK:
            import numpy._core.multiarray as ma  # numpy 2 home of _reconstruct / scalar

            if name in ("_reconstruct", "scalar"):
                return getattr(ma, name)
            return getattr(np, name)
        if module == "collections" and name == "OrderedDict":
            from collections import OrderedDict

            return OrderedDict
        if module in ("builtins", "__builtin__") and name in ("dict", "list", "set", "tuple", "frozenset"):
            return {"dict": dict, "list": list, "set": set, "tuple": tuple, "frozenset": frozenset}[name]
        if module.split(".")[0] in ("ase", "catkit", "networkx", "nff", "torch", "pymatgen", "mcmc"):
            return type(name, (_PStub,), {"__module__": module})
        raise pickle.UnpicklingError(f"global {module}.{name} is not allowed in a slab pickle")


def read_slab_pickle(path: str) -> Structure:
    with open(path, "rb") as fh:
        obj = _SlabUnpickler(io.BytesIO(fh.read())).load()
    d = vars(obj)
    arrays = d["arrays"]
    cellobj = d.get("_cellobj", d.get("_cell"))
    cell = np.asarray(getattr(cellobj, "array", cellobj), dtype=np.float64)
    pbc = np.asarray(d.get("_pbc", [True, True, True]), dtype=bool)
    fixed = None
    for con in d.get("_constraints", []) or []:
        idx = getattr(con, "index", None)
        if idx is not None:
            fixed = np.asarray(idx, dtype=np.int64)
    return Structure(np.asarray(arrays["numbers"]), np.asarray(arrays["positions"]), cell, pbc, fixed)


# --------------------------------------------------------------------------------------
# Synthetic benchmark inputs; deterministic in (base, chain index)
# --------------------------------------------------------------------------------------
def synth_chain(base: Structure, chain: int, species=(38, 22, 8), grid=(8, 8),
                jitter_xy=0.3, min_dist=1.5, sigma=0.05) -> Structure:
    """Chain ``c`` of the throughput workload: ``base`` plus ``8 + (c mod 25)`` adsorbates.

    Adsorbates are drawn with ``default_rng(1234 + c)`` uniformly from ``species`` and placed at
    z_top + 1.5 Å on a jittered in-plane grid, rejecting any pair closer than ``min_dist``
    (mirrors ``planar_distance`` / ``filter_distances``, reference ``mcmc/utils/misc.py:118-135``);
    then every atom is displaced by N(0, sigma) to emulate a mid-relaxation state.
    """
    rng = np.random.default_rng(1234 + int(chain))
    k = 8 + (int(chain) % 25)
    ztop = base.positions[:, 2].max()
    a, b = base.cell[0], base.cell[1]
    sites = [(i, j) for i in range(grid[0]) for j in range(grid[1])]
    order = rng.permutation(len(sites))
    ads_pos: list[np.ndarray] = []
    ads_num: list[int] = []
    for s in order:
        if len(ads_pos) == k:
            break
        i, j = sites[s]
        p = (i + 0.5) / grid[0] * a + (j + 0.5) / grid[1] * b
        p = p + np.array([rng.uniform(-jitter_xy, jitter_xy), rng.uniform(-jitter_xy, jitter_xy), 0.0])
        p[2] = ztop + 1.5
        ok = True
        for q in ads_pos:
            dv = p - q
            # in-plane minimum image
            f = np.linalg.solve(base.cell.T, dv)
            f[:2] -= np.round(f[:2])
            if np.linalg.norm(f @ base.cell) < min_dist:
                ok = False
                break
        if ok:
            ads_pos.append(p)
            ads_num.append(int(species[rng.integers(len(species))]))
    numbers = np.concatenate([base.numbers, np.array(ads_num, dtype=np.int32)])
    positions = np.concatenate([base.positions, np.array(ads_pos).reshape(-1, 3)])
    positions = positions + rng.normal(0.0, sigma, size=positions.shape)
    return Structure(numbers, positions, base.cell.copy(), base.pbc.copy())


# ---- LAMMPS data files (atom_style atomic) ----------------------------------------------------------------------------------
def _lammps_prism(cell):
    """LAMMPS' restricted triclinic box of a general cell: a along x, b in the xy plane (ASE ``Prism``): returns
    ``(lx, ly, lz, xy, xz, yz)`` and the matrix that rotates Cartesian vectors into that frame."""
    cell = np.asarray(cell, float).reshape(3, 3)
    a, b, c = cell
    lx = np.linalg.norm(a)
    ah = a / lx
    xy = float(np.dot(b, ah))
    ly = float(np.sqrt(max(np.dot(b, b) - xy * xy, 0.0)))
    xz = float(np.dot(c, ah))
    yz = float((np.dot(b, c) - xy * xz) / ly)
    lz = float(np.sqrt(max(np.dot(c, c) - xz * xz - yz * yz, 0.0)))
    new = np.array([[lx, 0.0, 0.0], [xy, ly, 0.0], [xz, yz, lz]])
    rot = np.linalg.solve(cell, new)          # x_lammps = x_cart @ rot   (fractional coordinates are preserved)
    return (float(lx), ly, lz, xy, xz, yz), rot


def write_lammps_data(path, atoms, specorder=None, name="lammps.data") -> list:
    """Write ``atoms`` as a LAMMPS data file, ``atom_style atomic`` -- what the reference's LAMMPS calculators produce
    with ``slab.write(lammps_data_file, format="lammps-data", atom_style="atomic")`` before every LAMMPS call (reference
    ``mcmc/calculators/calculators.py:548``; ``mcmc/calculators/lammpsrun.py:356-366``).  Atom types are numbered by
    ``specorder`` (symbols; default: the species present, sorted alphabetically like ASE).  Returns the species order.
    ``path`` may be a file name or an open text file."""
    Z, pos, cell, _ = as_arrays(atoms)
    symbols = [SYMBOLS[int(z)] for z in Z]
    species = list(specorder) if specorder is not None else sorted(set(symbols))
    missing = set(symbols) - set(species)
    if missing:
        raise ValueError(f"specorder lacks {sorted(missing)}")
    (lx, ly, lz, xy, xz, yz), rot = _lammps_prism(cell)
    x = np.asarray(pos, float) @ rot
    out = [f"{name} (written by surface_sampling_amd, ASE lammps-data layout)", "", f"{len(Z)} atoms",
           f"{len(species)} atom types", "", f"0.0 {lx:23.17g}  xlo xhi", f"0.0 {ly:23.17g}  ylo yhi",
           f"0.0 {lz:23.17g}  zlo zhi"]
    if max(abs(xy), abs(xz), abs(yz)) > 1e-12:
        out.append(f"{xy:23.17g} {xz:23.17g} {yz:23.17g}  xy xz yz")
    out += ["", "Atoms # atomic", ""]
    for i, (s, p) in enumerate(zip(symbols, x)):
        out.append(f"{i + 1:>6} {species.index(s) + 1:>3} {p[0]:23.17g} {p[1]:23.17g} {p[2]:23.17g}")
    text = "\n".join(out) + "\n"
    if hasattr(path, "write"):
        path.write(text)
    else:
        with open(path, "w") as fh:
            fh.write(text)
    return species


def read_lammps_data(path, species, pbc=(True, True, True)) -> Structure:
    """Read an ``atom_style atomic`` data file (the reference reads LAMMPS' ``write_data`` output back after a
    minimisation, ``mcmc/calculators/calculators.py:586``).  ``species``: symbol of type 1, 2, ..."""
    text = path.read() if hasattr(path, "read") else open(path).read()
    lines = [l.split("#")[0].strip() for l in text.splitlines()]
    n = lx = ly = lz = None
    xy = xz = yz = 0.0
    start = None
    for k, l in enumerate(lines):
        t = l.split()
        if len(t) == 2 and t[1] == "atoms":
            n = int(t[0])
        elif len(t) == 4 and t[2:] == ["xlo", "xhi"]:
            x0, lx = float(t[0]), float(t[1]) - float(t[0])
        elif len(t) == 4 and t[2:] == ["ylo", "yhi"]:
            y0, ly = float(t[0]), float(t[1]) - float(t[0])
        elif len(t) == 4 and t[2:] == ["zlo", "zhi"]:
            z0, lz = float(t[0]), float(t[1]) - float(t[0])
        elif len(t) == 6 and t[3:] == ["xy", "xz", "yz"]:
            xy, xz, yz = (float(v) for v in t[:3])
        elif t[:1] == ["Atoms"]:
            start = k + 1
            break
    if None in (n, lx, ly, lz, start):
        raise ValueError("not a LAMMPS data file with an Atoms section")
    rows = [l.split() for l in lines[start:] if l][:n]
    rows.sort(key=lambda r: int(r[0]))
    Z = np.array([ATOMIC_NUMBERS[species[int(r[1]) - 1]] for r in rows], np.int32)
    pos = np.array([[float(v) for v in r[2:5]] for r in rows]) - np.array([x0, y0, z0])
    cell = np.array([[lx, 0, 0], [xy, ly, 0], [xz, yz, lz]], float)
    return Structure(Z, pos, cell, np.array(pbc, bool))
