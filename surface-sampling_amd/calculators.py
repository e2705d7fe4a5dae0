"""ASE-Calculator-shaped front ends of the MI355X backend, mirroring the reference's classes.

Reference interfaces mirrored (``mcmc/calculators/calculators.py``):
  * ``EnsembleNFFSurface`` (:366-489)  -> :class:`EnsembleNFFSurface` here (same name, ctor kwargs
    ``device, model_units, prediction_units, offset_units``, ``set(**kw)``, ``parameters``,
    ``implemented_properties``, ``calculate``, ``get_surface_energy``, ``results`` keys/shapes,
    ``atoms.results.update`` side effect, ``models`` list).
  * ``LAMMPSSurfCalc`` / ``LAMMMPSCalc`` (:492-752) with ``pair_style tersoff``
                                       -> :class:`TersoffSurfCalc` (``energy``, ``per_atom_energies``,
    ``forces``, ``surface_energy``; no files, no LAMMPS process).
Callers on the reference side: ``SurfaceSystem.get_surface_energy`` (``mcmc/system.py:450-470``),
``optimize_slab`` (``mcmc/dynamics.py:83-170``), ``get_results_single`` (``calculators.py:34-47``).

ASE is optional: with ASE installed the classes derive from ``ase.calculators.calculator.Calculator``;
without it they derive from a small stand-in implementing the same caching protocol
(``get_property`` / ``check_state`` / ``get_potential_energy`` / ``get_forces``).
All numerical work happens in ``libvssr_eval.so``; there is no CPU fallback.
"""

from __future__ import annotations

import copy
import dataclasses
import json
import logging
import os
import re
from collections import Counter

import numpy as np

from . import backend, checkpoint, host_opt, pair as pair_io, structures, sw as sw_io, tersoff as tersoff_io, vashishta as vashishta_io

EV_TO_KCAL_MOL = 23.0605   # nff/utils/constants.py
HARTREE_TO_EV = 27.2114    # nff/utils/constants.py (reference import: calculators.py:21)

all_changes = ["positions", "numbers", "cell", "pbc", "initial_charges", "initial_magmoms"]

try:  # pragma: no cover - ASE is not installed in the build container
    from ase.calculators.calculator import Calculator as _AseCalculator
    from ase.calculators.calculator import all_changes as _ase_all_changes

    all_changes = list(_ase_all_changes)
    HAVE_ASE = True
except Exception:  # ImportError or a broken ASE install
    _AseCalculator = None
    HAVE_ASE = False


class _MiniCalculator:
    """The part of ``ase.calculators.calculator.Calculator`` the reference's callers rely on."""

    implemented_properties: tuple = ()
    default_parameters: dict = {}
    name = "calculator"

    def __init__(self, restart=None, label=None, atoms=None, **kwargs):
        self.atoms = None
        self.results: dict = {}
        self.parameters: dict = dict(self.default_parameters)
        self.label = label
        if atoms is not None:
            atoms.calc = self
        self.set(**kwargs)

    def set(self, **kwargs) -> dict:
        changed = {}
        for key, value in kwargs.items():
            old = self.parameters.get(key, None)
            same = False
            try:
                same = key in self.parameters and bool(np.all(old == value))
            except Exception:
                same = False
            if not same:
                changed[key] = value
                self.parameters[key] = value
        if changed:
            self.reset()
        return changed

    def reset(self):
        self.atoms = None
        self.results = {}

    @staticmethod
    def _snapshot(atoms):
        Z, pos, cell, pbc = structures.as_arrays(atoms)
        return structures.Structure(Z.copy(), pos.copy(), cell.copy(), pbc.astype(bool))

    def check_state(self, atoms, tol=1e-15):
        if self.atoms is None:
            return list(all_changes)
        old, new = structures.as_arrays(self.atoms), structures.as_arrays(atoms)
        changes = []
        for key, a, b in zip(("numbers", "positions", "cell", "pbc"), old, new):
            if a.shape != b.shape or not np.allclose(a, b, rtol=0, atol=tol):
                changes.append(key)
        return changes

    def calculate(self, atoms=None, properties=("energy",), system_changes=all_changes):
        if atoms is not None:
            self.atoms = self._snapshot(atoms)

    def get_property(self, name, atoms=None, allow_calculation=True):
        if name not in self.implemented_properties:
            raise NotImplementedError(f"{name} property not implemented")
        if atoms is None:
            raise ValueError("atoms is required")
        changes = self.check_state(atoms)
        if changes:
            self.results = {}
        if name not in self.results:
            if not allow_calculation:
                return None
            self.calculate(atoms, [name], changes)
        result = self.results[name]
        if isinstance(result, np.ndarray):
            result = result.copy()
        return result

    def get_potential_energy(self, atoms=None, force_consistent=False):
        return self.get_property("energy", atoms)

    def get_forces(self, atoms=None):
        return self.get_property("forces", atoms)

    def calculation_required(self, atoms, properties):
        if self.check_state(atoms):
            return True
        return any(p not in self.results for p in properties)


_Base = _AseCalculator if HAVE_ASE else _MiniCalculator


def _device_index(device) -> int:
    """'cuda', 'cuda:1', 1 -> ordinal; 'cpu' is rejected (the product has no CPU path)."""
    if isinstance(device, (int, np.integer)):
        return int(device)
    s = str(device).lower()
    if s.startswith("cpu"):
        raise backend.BackendError("device='cpu' requested: this backend only runs on an MI355X (HIP) device")
    if ":" in s:
        return int(s.split(":", 1)[1])
    return 0


def _units_per_ev(model_units: str, prediction_units: str) -> float:
    mu, pu = model_units.lower(), prediction_units.lower()
    if pu != "ev":
        raise ValueError("prediction_units must be 'eV'")
    if mu in ("kcal/mol", "kcal"):
        return EV_TO_KCAL_MOL
    if mu == "ev":
        return 1.0
    if mu in ("atomic", "hartree", "ha"):
        return 1.0 / HARTREE_TO_EV
    raise ValueError(f"unknown model_units {model_units!r}")


def stoich_offset_table(offset_data: dict, n_embed: int = 100, offset_units: str = "atomic"):
    """``stoidict`` -> per-species eV table + constant, as EnsembleNFF adds it to every prediction when ``offset_data`` is
    configured.  ``offset_units="atomic"`` (the PaiNN configuration,
    ``scripts/sample_surface.py:173``): the entries are Hartree; any other unit string ("eV"): taken as eV."""
    stoidict = offset_data["stoidict"]
    factor = HARTREE_TO_EV if offset_units == "atomic" else 1.0
    table = np.zeros(n_embed)
    for sym, val in stoidict.items():
        if sym == "offset":
            continue
        table[structures.ATOMIC_NUMBERS[sym]] = float(val) * factor
    return table, float(stoidict.get("offset", 0.0)) * factor


def surface_energy_from_energy(energy: float, symbols, chem_pots: dict, offset_data: dict,
                               offset_units: str = "atomic") -> float:
    """Bulk-reference and chemical-potential bookkeeping of
    ``EnsembleNFFSurface.get_surface_energy`` (reference ``calculators.py:379-446``)."""
    ads_count = Counter(symbols)
    bulk_energies = offset_data["bulk_energies"]
    stoics = offset_data["stoics"]
    ref_formula = offset_data["ref_formula"]
    ref_element = offset_data["ref_element"]
    bulk_ref_en = ads_count[ref_element] * bulk_energies[ref_formula]
    for ele in ads_count:
        if ele != ref_element:
            bulk_ref_en += (ads_count[ele] - stoics[ele] / stoics[ref_element] * ads_count[ref_element]) \
                * bulk_energies[ele]
    surface_energy = energy - (bulk_ref_en * HARTREE_TO_EV if offset_units == "atomic" else bulk_ref_en)
    pot = 0.0
    for ele in ads_count:
        if ele != ref_element:
            pot += (ads_count[ele] - stoics[ele] / stoics[ref_element] * ads_count[ref_element]) * chem_pots[ele]
    return surface_energy - pot


# thresholds of the reference's out-of-bounds guard (mcmc/dynamics.py:17-18,159-168): class attributes of both calculator families
ENERGY_THRESHOLD = 1000.0
MAX_FORCE_THRESHOLD = 1000.0


def _cfg_start(n_atoms) -> np.ndarray:
    """int64 prefix sum ``[B + 1]`` of the chains' atom counts: chain b holds the atoms ``start[b]:start[b + 1]``."""
    return np.concatenate([[0], np.cumsum(n_atoms)]).astype(np.int64)


def _fixed_mask(sizes, fixed_indices):
    """uint8 mask ``[sum N]`` (1 = held, FixAtoms) of per-slab index lists, ``fixed_indices[b]`` counting inside slab b; a slab whose
    entry is None or empty holds nothing.  ``fixed_indices=None``: no mask at all (None)."""
    if fixed_indices is None:
        return None
    start = _cfg_start(sizes)
    mask = np.zeros(int(start[-1]), np.uint8)
    held = [o + np.asarray(idx, dtype=np.int64) for o, idx in zip(start, fixed_indices) if idx is not None and len(idx)]
    if held:
        mask[np.concatenate(held)] = 1
    return mask


def _md_batch(get_engine, packs, atoms_list, fixed_indices, steps, timestep, thermostat, temperature, temperature_end, friction, seed, first_chain,
              velocities, masses, thermo_interval, md_driver, want):
    """``md_batch`` of every calculator: the argument checks, then on the calculator's engine (``get_engine()``, not touched before) the
    packed slabs, velocities (given, else Maxwell-Boltzmann at ``temperature``) and ``backend.md``; the per-slab dicts."""
    backend.md_thermostat_code(thermostat)   # (ValueError before anything is uploaded)
    if md_driver is not None:
        backend.md_driver_code(md_driver)
    if int(steps) < 0 or not float(timestep) > 0 or int(thermo_interval) < 1:
        raise ValueError(f"md_batch: steps {steps} >= 0, timestep {timestep} > 0 fs and thermo_interval {thermo_interval} >= 1 wanted")
    if thermostat == "langevin" and not float(friction) > 0:
        raise ValueError(f"md_batch: Langevin friction {friction} > 0 (1 / fs) wanted")
    if float(temperature) < 0 or (temperature_end is not None and float(temperature_end) < 0):
        raise ValueError("md_batch: a temperature is negative")
    B = len(atoms_list)
    if masses is not None and len(masses) != B:
        raise ValueError(f"md_batch: {len(masses)} mass arrays for {B} slabs")
    if velocities is not None and len(velocities) != B:
        raise ValueError(f"md_batch: {len(velocities)} velocity arrays for {B} slabs")
    start = _cfg_start([len(p[0]) for p in packs])
    m = np.concatenate([structures.masses_of(a, None if masses is None else masses[b]) for b, a in enumerate(atoms_list)])
    fixed = _fixed_mask(np.diff(start), fixed_indices)
    ids = np.arange(B, dtype=np.uint64) + np.uint64(int(first_chain))
    eng = get_engine()
    eng.upload(packs)
    if velocities is not None:
        eng.set_velocities(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in velocities]))
    else:
        eng.draw_velocities(m, temperature, seed=seed, fixed=fixed, chain_id=ids)
    info = eng.md(m, steps, timestep, thermostat=thermostat, temperature=temperature, temperature_end=temperature_end, friction=friction,
                  seed=seed, fixed=fixed, chain_id=ids, thermo_interval=thermo_interval, want=want, driver=md_driver)
    out = []
    for b, atoms in enumerate(atoms_list):
        a0, a1 = int(start[b]), int(start[b + 1])
        final = atoms.copy()
        final.set_positions(info["positions"][a0:a1])
        n_free = (a1 - a0) - (int(fixed[a0:a1].sum()) if fixed is not None else 0)
        ekin = info["ekin"][:, b].copy()
        out.append({"atoms": final, "velocities": info["velocities"][a0:a1].copy(), "epot": info["epot"][:, b].copy(), "ekin": ekin,
                    "temperature": 2.0 * ekin / (3.0 * n_free * backend.KB_EV) if n_free else np.zeros_like(ekin),
                    "n_done": int(info["n_done"][b]), "stop_reason": int(info["stop_reason"][b])})
    return out


_MD_DOC = """Molecular dynamics of B independent slabs at once on the device (``backend.md``): ``steps`` steps of ``timestep`` fs of velocity
        Verlet (``thermostat="nve"``) or Langevin BAOAB (``"langevin"``: ``temperature`` K, running linearly to ``temperature_end``
        over the call when that is given; ``friction`` in 1 / fs).  ``fixed_indices``: per slab, the atom indices FixAtoms holds (they
        never move and carry no velocity).  ``velocities``: per slab [N, 3] in A / fs; None draws Maxwell-Boltzmann velocities at
        ``temperature`` on the device.  ``masses``: per slab [N] in amu; None takes ``atoms.get_masses()`` where the object has it, else
        the standard atomic weights (``structures.ATOMIC_MASSES``).  Random numbers are keyed by ``seed`` and the global chain id
        ``first_chain + b``, so a slab's trajectory does not depend on the batch it runs in.  ``md_driver``: "auto" / "lockstep" /
        "resident" (None: the engine's setting).  Returns per slab a dict: ``atoms`` (a copy at the final positions), ``velocities``,
        ``epot`` / ``ekin`` / ``temperature`` (= 2 ekin / (3 n_free kB), 0 when nothing is free) after 0, k, 2k, ... steps with
        k = ``thermo_interval``, ``n_done``, ``stop_reason`` (``backend.MD_STOP_REASONS``)."""


def _vib_indices(sizes, indices):
    """Per structure, the sorted atom indices that vibrate: ``indices`` None (all atoms), one index list for every structure, or one
    list per structure.  ``ValueError`` for an index out of range or a wrong count of lists."""
    B = len(sizes)
    if indices is None:
        per = [np.arange(n) for n in sizes]
    else:
        idx = list(indices)
        nested = len(idx) > 0 and all(hasattr(i, "__len__") for i in idx)
        if nested and len(idx) != B:
            raise ValueError(f"vibrations_batch: {len(idx)} index lists for {B} structures")
        per = [np.asarray(idx[b] if nested else idx, dtype=np.int64).reshape(-1) for b in range(B)]
    out = []
    for b, (n, ix) in enumerate(zip(sizes, per)):
        if ix.size and (ix.min() < -n or ix.max() >= n):
            raise ValueError(f"vibrations_batch: structure {b} has {n} atoms, index out of range in {ix.tolist()}")
        out.append(np.unique(ix % n if n else ix))
    return out


# chains ``replicas="auto"`` fills the batch to: every structure is repeated until the batch has about this many chains, never more
# often than it has degrees of freedom
VIB_AUTO_CHAINS = 256


def _vibrations_batch(get_engine, pack, atoms_list, indices, masses, delta, nfree, method, temperature, e_min, replicas, return_hessian,
                      return_modes, want):
    """``vibrations_batch`` of every calculator: the argument checks, then on the calculator's engine (``get_engine()``, not touched
    before) every structure uploaded as its replicas and ``backend.vibrations``; the per-structure dicts."""
    backend.vib_method_code(method)   # (ValueError before anything is uploaded)
    if int(nfree) not in (2, 4):
        raise ValueError(f"vibrations_batch: nfree {nfree} (2 or 4 wanted)")
    if not (np.isfinite(float(delta)) and float(delta) > 0):
        raise ValueError(f"vibrations_batch: delta {delta} > 0 (A) wanted")
    T = 0.0 if temperature is None else float(temperature)
    if not (np.isfinite(T) and T >= 0) or not (np.isfinite(float(e_min)) and float(e_min) >= 0):
        raise ValueError(f"vibrations_batch: temperature {temperature} >= 0 (K) and e_min {e_min} >= 0 (eV) wanted")
    if replicas != "auto" and (isinstance(replicas, (str, bool)) or int(replicas) != replicas or int(replicas) < 1):
        raise ValueError(f"vibrations_batch: replicas {replicas!r} ('auto' or an integer >= 1 wanted)")
    B = len(atoms_list)
    if masses is not None and len(masses) != B:
        raise ValueError(f"vibrations_batch: {len(masses)} mass arrays for {B} structures")
    sizes = [len(a) for a in atoms_list]
    per = _vib_indices(sizes, indices)
    ms = [structures.masses_of(a, None if masses is None else masses[b]) for b, a in enumerate(atoms_list)]
    dof = [3 * len(ix) for ix in per]
    if max(dof + [0]) > backend.VIB_MAX_DOF:
        raise ValueError(f"vibrations_batch: {max(dof)} degrees of freedom in one structure (at most {backend.VIB_MAX_DOF}: 85 atoms)")
    if replicas == "auto":
        per_struct = max(1, VIB_AUTO_CHAINS // max(B, 1))
        reps = [max(1, min(per_struct, m)) for m in dof]
    else:
        reps = [max(1, min(int(replicas), m)) for m in dof]
    packs, mass, mask = [], [], []
    for b, a in enumerate(atoms_list):
        pk = pack(a)
        v = np.zeros(sizes[b], np.uint8)
        v[per[b]] = 1
        for _ in range(reps[b]):
            packs.append(pk); mass.append(ms[b]); mask.append(v)
    eng = get_engine()
    eng.upload(packs)
    r = eng.vibrations(np.concatenate(mass), vib=np.concatenate(mask), n_rep=reps, delta=delta, nfree=nfree, method=method, temperature=T,
                       e_min=e_min, want=want, return_hessian=return_hessian, return_modes=return_modes)
    out = []
    for b in range(B):
        d = {"energies": r["energies"][b], "frequencies": r["energies"][b] / backend.EV_PER_INV_CM, "zpe": float(r["zpe"][b]),
             "helmholtz_vib": float(r["f_vib"][b]), "n_imag": int(r["n_imag"][b]), "n_left_out": int(r["n_left_out"][b]),
             "energy": float(r["energy"][b]), "stop_reason": int(r["stop_reason"][b]), "indices": per[b], "replicas": reps[b]}
        if return_hessian:
            d["hessian"] = r["hessian"][b]
        if return_modes:
            d["modes"] = r["modes"][b]
        out.append(d)
    return out


_VIB_DOC = """Harmonic vibrations of B structures at once on the device (``backend.vibrations``): what ASE's ``Vibrations(atoms, indices,
        delta=, nfree=)`` + ``HarmonicThermo.get_helmholtz_energy`` (minus the potential energy) give, with every displacement a
        lock-step evaluation and the eigen-solve on the device.  ``indices``: the atoms that vibrate, one list for all structures or
        one per structure (None: all atoms; at most 85 per structure).  Held atoms are simply left out (forces are the raw forces).
        ``masses``: per structure [N] in amu (None: ``structures.masses_of``).  ``delta`` in A, ``nfree`` 2 or 4, ``method``
        "standard" / "frederiksen", ``temperature`` in K (None: 0), modes with energy <= ``e_min`` eV (imaginary ones included) stay
        out of the sums.  ``replicas``: how many identical chains share one structure's displacements -- "auto" fills the batch to
        about ``VIB_AUTO_CHAINS`` chains, never more replicas than degrees of freedom; an integer forces a count.  Returns per
        structure a dict: ``energies`` (eV, ascending, negative = imaginary), ``frequencies`` (cm^-1 = energies / 1.239841984e-4),
        ``zpe``, ``helmholtz_vib``, ``n_imag``, ``n_left_out``, ``energy`` (the potential energy), ``stop_reason``
        (``backend.VIB_STOP_REASONS``), ``indices``, ``replicas``, and with the flags ``hessian`` (eV / A^2) and ``modes``
        (mass-weighted unit eigenvectors in rows)."""


def _neb_batch(get_engine, pack, bands, fixed_indices, k, climb, method, fmax, steps, two_stage, want):
    """``neb_batch`` of every calculator: the argument checks and the interpolation of ``(initial, final, n_images)`` tuples, then on
    the calculator's engine (``get_engine()``, not touched before) every band uploaded as consecutive chains and ``backend.neb``
    (twice for ``two_stage``: the resident band goes on with the climbing image and a fresh FIRE state); the per-band dicts."""
    backend.neb_method_code(method)   # (ValueError before anything is uploaded)
    if climb not in (False, True, 0, 1) or two_stage not in (False, True, 0, 1):
        raise ValueError(f"neb_batch: climb {climb!r} and two_stage {two_stage!r} are bools")
    if not (np.isfinite(float(k)) and float(k) > 0) or not (np.isfinite(float(fmax)) and float(fmax) > 0):
        raise ValueError(f"neb_batch: k {k} > 0 (eV / A^2) and fmax {fmax} > 0 (eV / A) wanted")
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 0:
        raise ValueError(f"neb_batch: steps {steps!r} (an integer >= 0 wanted)")
    bands = list(bands)
    if not bands:
        raise ValueError("neb_batch: no bands")
    images = []
    for g, band in enumerate(bands):
        if isinstance(band, tuple):
            if len(band) != 3:
                raise ValueError(f"neb_batch: band {g} is a tuple of {len(band)} entries ((initial, final, n_images) wanted)")
            band = structures.interpolate_band(band[0], band[1], band[2])
        band = list(band)
        if len(band) < 3:
            raise ValueError(f"neb_batch: band {g} has {len(band)} images (>= 3 wanted)")
        a0 = structures.as_arrays(band[0])
        for i, img in enumerate(band[1:], 1):
            a = structures.as_arrays(img)
            if len(a[0]) != len(a0[0]) or any(not np.array_equal(u, v) for u, v in ((a[0], a0[0]), (a[2], a0[2]), (a[3], a0[3]))):
                raise ValueError(f"neb_batch: image {i} of band {g} differs from its first image in more than positions")
        images.append(band)
    G = len(images)
    if fixed_indices is not None and len(fixed_indices) != G:
        raise ValueError(f"neb_batch: {len(fixed_indices)} index lists for {G} bands")
    n_img = [len(b) for b in images]
    flat = [img for b in images for img in b]
    sizes = [len(img) for img in flat]
    per_image = None if fixed_indices is None else [fixed_indices[g] for g, b in enumerate(images) for _ in b]
    if per_image is not None:
        for n, idx in zip(sizes, per_image):
            if idx is not None and len(idx) and (np.min(idx) < 0 or np.max(idx) >= n):
                raise ValueError(f"neb_batch: a fixed index outside 0 .. {n - 1}")
    fixed = _fixed_mask(sizes, per_image)
    start = _cfg_start(sizes)
    eng = get_engine()
    eng.upload([pack(img) for img in flat])
    r = eng.neb(n_img, fixed=fixed, k=k, climb=bool(climb) and not two_stage, method=method, fmax=fmax, max_steps=int(steps), want=want)
    n_steps = r["n_steps"].copy()
    if two_stage:
        r = eng.neb(n_img, fixed=fixed, k=k, climb=True, method=method, fmax=fmax, max_steps=int(steps), want=want)
        n_steps = n_steps + r["n_steps"]
    out, b = [], 0
    for g, band in enumerate(images):
        a0, a1 = int(start[b]), int(start[b + n_img[g]])
        x = r["positions"][a0:a1].reshape(n_img[g], -1, 3).copy()
        _, _, cell, pbc = structures.as_arrays(band[0])
        out.append({"images": x, "energies": r["energies"][b:b + n_img[g]].copy(), "path": structures.band_path(x, cell, pbc),
                    "neb_forces": r["neb_forces"][a0:a1].reshape(n_img[g], -1, 3).copy(),
                    "barrier_forward": float(r["barrier_forward"][g]), "barrier_reverse": float(r["barrier_reverse"][g]),
                    "imax": int(r["imax"][g]), "fmax": float(r["fmax"][g]), "n_steps": int(n_steps[g]),
                    "stop_reason": int(r["stop_reason"][g]), "converged": int(r["stop_reason"][g]) == 1})
        b += n_img[g]
    return out


_NEB_DOC = """Nudged elastic bands of G paths at once on the device (``backend.neb``): what ASE's ``NEB(images, k=, climb=, method=)`` with
        ``FIRE(neb).run(fmax, steps)`` gives, with every image of every band a chain of one lock-step evaluation.  ``bands``: per band
        a list of >= 3 Atoms-like images that differ in positions only, or a tuple ``(initial, final, n_images)`` that
        ``structures.interpolate_band`` fills in linearly (displacements wrapped to the nearest image).  The end images never move.
        ``fixed_indices``: per band, the atom indices FixAtoms holds in every image.  ``k`` in eV / A^2, ``method``
        "improvedtangent" / "aseneb", ``fmax`` in eV / A on the NEB force, at most ``steps`` FIRE steps.  ``two_stage`` runs
        ``steps`` without the climbing image and then ``steps`` with it, FIRE restarting as a new ASE optimizer would.  Returns per
        band a dict: ``images`` [n, N, 3], ``energies`` [n], ``path`` [n] (cumulative |d|, the reaction coordinate),
        ``neb_forces`` [n, N, 3], ``barrier_forward`` / ``barrier_reverse`` (E_max - E_first / E_last over the interior images),
        ``imax``, ``fmax``, ``n_steps``, ``stop_reason`` (``backend.NEB_STOP_REASONS``), ``converged``.  The saddle's prefactor side
        is ``vibrations_batch`` on image ``imax`` (one imaginary mode)."""


def _dimer_batch(get_engine, pack, atoms_list, modes, fixed_indices, n_starts, seed, steps, fmax, delta, phi_tol, max_rot_first, max_rot,
                 displace, want):
    """``dimer_batch`` of every calculator: the argument checks, then on the calculator's engine (``get_engine()``, not touched before)
    every structure uploaded ``n_starts`` times as the two chains of a dimer and ``backend.dimer``; the per-search dicts."""
    def whole(v, name, low):
        if isinstance(v, bool) or int(v) != v or int(v) < low:
            raise ValueError(f"dimer_batch: {name} {v!r} (an integer >= {low} wanted)")
        return int(v)

    n_starts, steps = whole(n_starts, "n_starts", 1), whole(steps, "steps", 0)
    max_rot_first, max_rot = whole(max_rot_first, "max_rot_first", 0), whole(max_rot, "max_rot", 0)
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"dimer_batch: seed {seed!r} (an integer in [0, 2^64) wanted)")
    for name, v in (("fmax (eV / A)", fmax), ("delta (A)", delta)):
        if not (np.isfinite(float(v)) and float(v) > 0):
            raise ValueError(f"dimer_batch: {name} {v} (finite and > 0 wanted)")
    if not 0.0 < float(phi_tol) <= np.pi / 4:
        raise ValueError(f"dimer_batch: phi_tol {phi_tol} rad outside (0, pi / 4]")
    if not np.isfinite(float(displace)):
        raise ValueError(f"dimer_batch: displace {displace} A is not finite")
    atoms_list = list(atoms_list)
    S = len(atoms_list)
    if not S:
        raise ValueError("dimer_batch: no structures")
    if fixed_indices is not None and len(fixed_indices) != S:
        raise ValueError(f"dimer_batch: {len(fixed_indices)} index lists for {S} structures")
    if modes is not None and (len(modes) != S or n_starts != 1):
        raise ValueError(f"dimer_batch: modes are one [n, 3] array per structure ({S}) and go with n_starts = 1")
    sizes = [len(a) for a in atoms_list]
    free = []
    for i, n in enumerate(sizes):
        idx = None if fixed_indices is None else fixed_indices[i]
        m = np.ones(n, bool)
        if idx is not None and len(idx):
            if np.min(idx) < 0 or np.max(idx) >= n:
                raise ValueError(f"dimer_batch: a fixed index outside 0 .. {n - 1}")
            m[np.asarray(idx, int)] = False
        if not m.any():
            raise ValueError(f"dimer_batch: structure {i} has no free atom to carry a mode")
        if modes is not None:
            v = np.asarray(modes[i], np.float64)
            if v.shape != (n, 3):
                raise ValueError(f"dimer_batch: mode {i} has shape {v.shape} ([{n}, 3] wanted)")
            nn = float((v[m] ** 2).sum())
            if not (np.isfinite(nn) and nn > 0):
                raise ValueError(f"dimer_batch: mode {i} has no finite length over the free atoms")
        free.append(m)
    # structure i as searches i n_starts .. (i + 1) n_starts - 1, each two chains; dimer ids 0 .. n_starts - 1 per structure
    flat_sizes = [n for n in sizes for _ in range(2 * n_starts)]
    per_chain = None if fixed_indices is None else [fixed_indices[i] for i in range(S) for _ in range(2 * n_starts)]
    fixed = _fixed_mask(flat_sizes, per_chain)
    start = _cfg_start(flat_sizes)
    mode_in = None
    if modes is not None:
        mode_in = np.vstack([np.vstack([np.asarray(modes[i], np.float64), np.zeros((sizes[i], 3))]) for i in range(S)])
    ids = np.tile(np.arange(n_starts, dtype=np.uint64), S)
    eng = get_engine()
    eng.upload([pack(a) for a in atoms_list for _ in range(2 * n_starts)])
    r = eng.dimer(fixed=fixed, modes=mode_in, dimer_id=ids, seed=int(seed), max_steps=steps, max_rot_first=max_rot_first, max_rot=max_rot,
                  delta=float(delta), phi_tol=float(phi_tol), fmax=float(fmax), displace=float(displace), want=want)
    out = []
    for g in range(S * n_starts):
        a0, a1 = int(start[2 * g]), int(start[2 * g + 1])
        out.append({"structure": g // n_starts, "dimer_id": int(ids[g]), "positions": r["positions"][a0:a1].copy(),
                    "mode": r["modes"][a0:a1].copy(), "e0": float(r["e0"][g]), "curvature": float(r["curvature"][g]),
                    "fmax": float(r["fmax"][g]), "n_steps": int(r["n_steps"][g]), "n_rot": int(r["n_rot"][g]), "n_eval": int(r["n_eval"][g]),
                    "stop_reason": int(r["stop_reason"][g]), "converged": int(r["stop_reason"][g]) == 1})
    return out


_DIMER_DOC = """Saddle searches from single structures on the device (``backend.dimer``): the dimer method (min-mode following) with one
        gradient per rotation and ASE's FIRE for the translation, every search two chains of one lock-step evaluation.  Every
        structure of ``atoms_list`` is searched ``n_starts`` times, start k under dimer id k: its starting mode is drawn from
        (``seed``, k, atom, component), so the starts of a structure differ and a search does not depend on what else is in the
        call.  ``modes``: one [n, 3] starting mode per structure instead (``n_starts`` = 1).  ``fixed_indices``: per structure, the
        atom indices FixAtoms holds.  ``fmax`` in eV / A on the midpoint force (with a negative curvature), ``delta`` the dimer
        half-length in A, ``phi_tol`` in rad, ``max_rot_first`` / ``max_rot`` rotations before the first / every later of at most
        ``steps`` translations, ``displace`` in A along the mode before the first evaluation.  Returns per search (structure-major)
        a dict: ``structure``, ``dimer_id``, ``positions`` [n, 3], ``mode`` [n, 3] (unit, zero on held atoms), ``e0``,
        ``curvature`` (eV / A^2 along the mode), ``fmax``, ``n_steps``, ``n_rot``, ``n_eval``, ``stop_reason``
        (``backend.DIMER_STOP_REASONS``), ``converged``.  A converged search is a first-order saddle if ``vibrations_batch`` on
        ``positions`` finds one imaginary mode; several starts may find the same saddle (no deduplication).  Restated from the
        papers, not ASE's ``MinModeTranslate``."""


def _relax_cell_batch(get_engine, pack, atoms_list, fixed_indices, mask, scalar_pressure, hydrostatic_strain, cell_factor, steps, fmax, want):
    """``relax_cell_batch`` of every calculator: the argument checks, then on the calculator's engine (``get_engine()``, not touched
    before) the packed structures and ``backend.relax_cell``; the per-structure dicts."""
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 0:
        raise ValueError(f"relax_cell_batch: steps {steps!r} (an integer >= 0 wanted)")
    if not (np.isfinite(float(fmax)) and float(fmax) > 0):
        raise ValueError(f"relax_cell_batch: fmax {fmax} eV / A (finite and > 0 wanted)")
    if not np.isfinite(float(scalar_pressure)):
        raise ValueError(f"relax_cell_batch: scalar_pressure {scalar_pressure} eV / A^3 is not finite")
    if cell_factor is not None and not np.isfinite(float(cell_factor)):
        raise ValueError(f"relax_cell_batch: cell_factor {cell_factor} is not finite")
    atoms_list = list(atoms_list)
    B = len(atoms_list)
    if not B:
        raise ValueError("relax_cell_batch: no structures")
    if fixed_indices is not None and len(fixed_indices) != B:
        raise ValueError(f"relax_cell_batch: {len(fixed_indices)} index lists for {B} structures")
    sizes = [len(a) for a in atoms_list]
    for n, idx in zip(sizes, fixed_indices or ()):
        if idx is not None and len(idx) and (np.min(idx) < 0 or np.max(idx) >= n):
            raise ValueError(f"relax_cell_batch: a fixed index outside 0 .. {n - 1}")
    p = backend.CellRelaxParams.default(int(steps), float(fmax), float(scalar_pressure), mask, hydrostatic_strain,
                                        0.0 if cell_factor is None else float(cell_factor))   # (ValueError for a bad mask)
    start = _cfg_start(sizes)
    fixed = _fixed_mask(sizes, fixed_indices)
    eng = get_engine()
    eng.upload([pack(a) for a in atoms_list])
    r = eng.relax_cell(fixed=fixed, params=p, want=want)
    out = []
    for b, atoms in enumerate(atoms_list):
        a0, a1 = int(start[b]), int(start[b + 1])
        final = atoms.copy()
        if hasattr(final, "set_cell"):
            final.set_cell(r["cells"][b].copy(), scale_atoms=False)
        else:
            final.cell = r["cells"][b].copy()
        final.set_positions(r["positions"][a0:a1])
        out.append({"atoms": final, "cell": r["cells"][b].copy(), "energy": float(r["energy"][b]), "volume": float(r["volume"][b]),
                    "fmax": float(r["fmax"][b]), "n_steps": int(r["n_steps"][b]), "stop_reason": int(r["stop_reason"][b]),
                    "converged": int(r["stop_reason"][b]) == 1})
    return out


_CELL_DOC = """Atoms and cells of B structures relaxed together on the device (``backend.relax_cell``): ASE's ``UnitCellFilter`` under ASE's
        FIRE, every structure a chain of one lock-step evaluation, its stress consumed where it is computed.  ``fixed_indices``: per
        structure, the atom indices FixAtoms holds (their fractional coordinates stay).  ``mask``: six 0 / 1 in Voigt order xx yy zz
        yz xz xy, the strain components that are free (None: all; a slab periodic in x and y takes (1, 1, 0, 0, 0, 1));
        ``scalar_pressure`` in eV / A^3; ``hydrostatic_strain``: the cell only scales; ``cell_factor``: None = the atom count, as
        ASE; ``fmax`` in eV / A over atoms and cell rows; at most ``steps`` FIRE steps.  Returns per structure a dict: ``atoms`` (a
        copy with the relaxed cell and positions), ``cell`` [3, 3], ``energy`` / ``volume`` / ``fmax`` as of the last convergence
        test, ``n_steps``, ``stop_reason`` (``backend.CELL_STOP_REASONS``), ``converged``.  Served by every calculator but pair
        models with k-space.  The contract is the numpy restatement tests/cellrelax_oracle.py, not an executed ASE; constant_volume,
        ExpCellFilter / FrechetCellFilter and other optimizers over the filter are out of scope."""


def _npt_batch(get_engine, pack, atoms_list, fixed_indices, steps, timestep, thermostat, barostat, pressure, compressibility, taut, taup, mask,
               coupling, temperature, temperature_end, friction, seed, first_chain, velocities, masses, thermo_interval, want):
    """``npt_batch`` of every calculator: the argument checks, then on the calculator's engine (``get_engine()``, not touched before)
    the packed structures, velocities (given, else Maxwell-Boltzmann at ``temperature``) and ``backend.npt``; the per-structure dicts."""
    p = backend.npt_params(steps, timestep, thermostat=thermostat, barostat=barostat, coupling=coupling, temperature=temperature,
                           temperature_end=temperature_end, friction=friction, taut=taut, taup=taup, pressure=pressure,
                           compressibility=compressibility, mask=mask, seed=seed, thermo_interval=thermo_interval)   # (ValueError: names, mask)
    finite = all(np.isfinite(float(v)) for v in (timestep, temperature, friction, taut, taup, pressure, compressibility))
    if int(steps) < 0 or not (finite and float(timestep) > 0) or int(thermo_interval) < 1:
        raise ValueError(f"npt_batch: steps {steps} >= 0, timestep {timestep} > 0 fs, thermo_interval {thermo_interval} >= 1 and finite parameters wanted")
    if float(temperature) < 0 or (temperature_end is not None and not float(temperature_end) >= 0):
        raise ValueError("npt_batch: a temperature is negative")
    if thermostat == "langevin" and not float(friction) > 0:
        raise ValueError(f"npt_batch: Langevin friction {friction} > 0 (1 / fs) wanted")
    if thermostat == "berendsen" and not float(taut) > 0:
        raise ValueError(f"npt_batch: taut {taut} > 0 (fs) wanted")
    if barostat != "none":
        if not (float(taup) > 0 and float(compressibility) > 0):
            raise ValueError(f"npt_batch: taup {taup} > 0 (fs) and compressibility {compressibility} > 0 (A^3 / eV) wanted")
        if not any(p.mask):
            raise ValueError("npt_batch: a barostat with an empty mask")
        if barostat == "crescale" and (thermostat == "none" or coupling != "isotropic" or not all(p.mask)):
            raise ValueError("npt_batch: stochastic cell rescaling is isotropic (coupling 'isotropic', mask (1, 1, 1)) and needs a thermostat")
    atoms_list = list(atoms_list)
    B = len(atoms_list)
    if not B:
        raise ValueError("npt_batch: no structures")
    for name, per in (("index lists", fixed_indices), ("mass arrays", masses), ("velocity arrays", velocities)):
        if per is not None and len(per) != B:
            raise ValueError(f"npt_batch: {len(per)} {name} for {B} structures")
    sizes = [len(a) for a in atoms_list]
    start = _cfg_start(sizes)
    m = np.concatenate([structures.masses_of(a, None if masses is None else masses[b]) for b, a in enumerate(atoms_list)])
    fixed = _fixed_mask(sizes, fixed_indices)
    ids = np.arange(B, dtype=np.uint64) + np.uint64(int(first_chain))
    eng = get_engine()
    eng.upload([pack(a) for a in atoms_list])
    if velocities is not None:
        eng.set_velocities(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in velocities]))
    else:
        eng.draw_velocities(m, temperature, seed=seed, fixed=fixed, chain_id=ids)
    r = eng.npt(m, steps, timestep, fixed=fixed, chain_id=ids, want=want, params=p)
    out = []
    for b, atoms in enumerate(atoms_list):
        a0, a1 = int(start[b]), int(start[b + 1])
        final = atoms.copy()
        if hasattr(final, "set_cell"):
            final.set_cell(r["cells"][b].copy(), scale_atoms=False)
        else:
            final.cell = r["cells"][b].copy()
        final.set_positions(r["positions"][a0:a1])
        n_free = (a1 - a0) - (int(fixed[a0:a1].sum()) if fixed is not None else 0)
        ekin = r["ekin"][:, b].copy()
        out.append({"atoms": final, "cell": r["cells"][b].copy(), "velocities": r["velocities"][a0:a1].copy(), "epot": r["epot"][:, b].copy(),
                    "ekin": ekin, "temperature": 2.0 * ekin / (3.0 * n_free * backend.KB_EV) if n_free else np.zeros_like(ekin),
                    "volume": r["volume"][:, b].copy(), "pressure": r["pressure"][:, b].copy(), "n_done": int(r["n_done"][b]),
                    "stop_reason": int(r["stop_reason"][b])})
    return out


_NPT_DOC = """Constant-pressure / weakly coupled MD of B independent structures at once on the device (``backend.npt``, lock step): the step
        of ``md_batch`` with ``thermostat`` "none" / "langevin" (``friction`` 1 / fs) / "berendsen" (``taut`` fs) and ``barostat``
        "none" / "berendsen" (``coupling`` "isotropic" = ASE's NPTBerendsen, "per_axis" = Inhomogeneous_NPTBerendsen) / "crescale"
        (stochastic cell rescaling, isotropic, needs a thermostat).  ``pressure`` in eV / A^3, ``compressibility`` in A^3 / eV, ``taup``
        in fs, ``mask``: three 0 / 1 per Cartesian axis (a slab periodic in x and y takes (1, 1, 0)).  Held atoms keep v = 0 and ride
        the cell.  ``velocities`` / ``masses`` / ``seed`` / ``first_chain`` / ``thermo_interval`` as ``md_batch``.  Returns per structure
        a dict: ``atoms`` (a copy with the final cell and positions), ``cell`` [3, 3], ``velocities``, ``epot`` / ``ekin`` /
        ``temperature`` / ``volume`` / ``pressure`` after 0, k, 2k, ... steps (pressure NaN without a barostat), ``n_done``,
        ``stop_reason`` (``backend.NPT_STOP_REASONS``).  Served by every calculator; a barostat not by pair models with k-space.  The
        contract is the numpy restatement tests/npt_oracle.py, not an executed ASE."""


class _DynamicsFrontEnds:
    """``md_batch`` / ``vibrations_batch`` / ``neb_batch`` / ``dimer_batch`` / ``relax_cell_batch`` / ``npt_batch`` of a calculator with ``_get_engine``, in terms of two
    hooks of the class: ``_pack(atoms) -> (Z or types, pos, cell, pbc)`` and ``_dynamics_want``, the outputs an evaluation produces."""

    _dynamics_want = 0

    def md_batch(self, atoms_list, fixed_indices=None, steps: int = 100, timestep: float = 1.0, thermostat: str = "nve",
                 temperature: float = 300.0, temperature_end=None, friction: float = 0.01, seed: int = 0, first_chain: int = 0,
                 velocities=None, masses=None, thermo_interval: int = 1, md_driver=None):
        return _md_batch(self._get_engine, [self._pack(a) for a in atoms_list], atoms_list, fixed_indices, steps, timestep, thermostat,
                         temperature, temperature_end, friction, seed, first_chain, velocities, masses, thermo_interval, md_driver,
                         self._dynamics_want)

    md_batch.__doc__ = _MD_DOC

    def vibrations_batch(self, atoms_list, indices=None, masses=None, delta: float = 0.01, nfree: int = 2, method: str = "standard",
                         temperature=None, e_min: float = 0.0, replicas="auto", return_hessian: bool = False, return_modes: bool = False):
        return _vibrations_batch(self._get_engine, self._pack, atoms_list, indices, masses, delta, nfree, method, temperature, e_min, replicas,
                                 return_hessian, return_modes, self._dynamics_want)

    vibrations_batch.__doc__ = _VIB_DOC

    def neb_batch(self, bands, fixed_indices=None, k: float = 0.1, climb: bool = False, method: str = "improvedtangent", fmax: float = 0.05,
                  steps: int = 100, two_stage: bool = False):
        return _neb_batch(self._get_engine, self._pack, bands, fixed_indices, k, climb, method, fmax, steps, two_stage, self._dynamics_want)

    neb_batch.__doc__ = _NEB_DOC

    def dimer_batch(self, atoms_list, modes=None, fixed_indices=None, n_starts: int = 1, seed: int = 0, steps: int = 100, fmax: float = 0.05,
                    delta: float = 0.01, phi_tol: float = np.pi / 180.0, max_rot_first: int = 8, max_rot: int = 1, displace: float = 0.0):
        return _dimer_batch(self._get_engine, self._pack, atoms_list, modes, fixed_indices, n_starts, seed, steps, fmax, delta, phi_tol,
                            max_rot_first, max_rot, displace, self._dynamics_want)

    dimer_batch.__doc__ = _DIMER_DOC

    def relax_cell_batch(self, atoms_list, fixed_indices=None, mask=None, scalar_pressure: float = 0.0, hydrostatic_strain: bool = False,
                         cell_factor=None, steps: int = 100, fmax: float = 0.05):
        return _relax_cell_batch(self._get_engine, self._pack, atoms_list, fixed_indices, mask, scalar_pressure, hydrostatic_strain, cell_factor,
                                 steps, fmax, self._dynamics_want)

    relax_cell_batch.__doc__ = _CELL_DOC

    def npt_batch(self, atoms_list, fixed_indices=None, steps: int = 100, timestep: float = 1.0, thermostat: str = "berendsen",
                  barostat: str = "berendsen", pressure: float = 0.0, compressibility: float = 1.0, taut: float = 100.0, taup: float = 1000.0,
                  mask=None, coupling: str = "isotropic", temperature: float = 300.0, temperature_end=None, friction: float = 0.01,
                  seed: int = 0, first_chain: int = 0, velocities=None, masses=None, thermo_interval: int = 1):
        return _npt_batch(self._get_engine, self._pack, atoms_list, fixed_indices, steps, timestep, thermostat, barostat, pressure,
                          compressibility, taut, taup, mask, coupling, temperature, temperature_end, friction, seed, first_chain, velocities,
                          masses, thermo_interval, self._dynamics_want)

    npt_batch.__doc__ = _NPT_DOC


def _oob_flags(energy, forces, cfg_start, saturated=None, *, e_max, f_max) -> np.ndarray:
    """bool ``[B]``: the reference's out-of-bounds guard (``mcmc/dynamics.py:159-168``) for every chain of a batch -- a non-finite energy
    or force, ``|E| > e_max``, a force component beyond ``f_max``, or a ``saturated`` evaluation."""
    fabs = np.abs(forces).max(axis=1) if len(forces) else np.zeros(0, forces.dtype)
    nonempty = cfg_start[1:] > cfg_start[:-1]
    max_force = np.zeros(len(cfg_start) - 1, fabs.dtype)
    if nonempty.any():
        max_force[nonempty] = np.maximum.reduceat(fabs, cfg_start[:-1][nonempty])
    with np.errstate(invalid="ignore"):
        oob = (~np.isfinite(energy)) | (~np.isfinite(max_force)) | (np.abs(energy) > e_max) | (max_force > f_max)
    return oob if saturated is None else oob | np.asarray(saturated, dtype=bool)


def _chain_counts(counts, b) -> dict:
    """Chain b's entries of a relaxation's per-chain count arrays as Python values, a CG ``stop`` code as its text."""
    out = {}
    for key, values in counts.items():
        if key == "stop":
            out[key] = backend.CG_STOP_REASONS.get(int(values[b]), str(int(values[b])))
        else:
            out[key] = bool(values[b]) if key == "converged" else int(values[b])
    return out


def _lockstep_evaluate(eng):
    """``evaluate(pos_all) -> (fp64 energies [B], fp64 forces [N, 3])`` of the engine's resident batch, for host_opt.py's drivers."""
    def evaluate(pos_all):
        eng.set_positions(pos_all)
        eng.run()
        r = eng.download()
        return np.asarray(r.get("energy_f64", r["energy"]), dtype=np.float64), np.asarray(r["forces"], dtype=np.float64)

    return evaluate


class _LockstepProxy(_Base):
    """Calculator of ONE chain inside a host-driven optimizer (host_opt.optimizer_class_batch): energy and forces come from the
    lock-step evaluation of the whole resident batch."""

    implemented_properties = ("energy", "forces")
    name = "vssr_lockstep_proxy"

    def __init__(self, request, **kwargs):
        super().__init__(**kwargs)
        self._request = request

    def calculate(self, atoms=None, properties=("energy",), system_changes=all_changes):
        super().calculate(atoms, properties, system_changes)
        e, f = self._request(atoms)
        self.results = {"energy": float(e), "forces": np.asarray(f, dtype=np.float64)}


class EnsembleNFFSurface(_DynamicsFrontEnds, _Base):
    """PaiNN-ensemble surface calculator on MI355X (drop-in for the reference class of the same name).

    Args:
        models: list of checkpoints — paths to nff ``best_model`` files / canonical ``.f32`` blobs, or
            float32 arrays already in the canonical layout (``include/vssr_eval.h``).
        device: ``"cuda"``, ``"cuda:N"`` or an int ordinal.
        model_units / prediction_units / offset_units: as in the reference (``"kcal/mol"``, ``"eV"``,
            ``"atomic"``).
        cutoff: neighbor cutoff in Å (the reference passes it through ``get_atoms_batch``); default 5.0, or with
            ``hparams="auto"`` the models' own cutoff (``params.json`` / the checkpoint's module attribute).  A cutoff that
            differs from the one the models were trained with raises ``ValueError``.
        position_dtype: ``"float64"`` (default: the caller's positions as they are) or ``"float32"``: positions are rounded to
            float32 before an evaluation, the way nff's ``AtomsBatch`` holds them (``nxyz`` is a float32 tensor, reference
            ``mcmc/utils/misc.py:34-42``) -- single-point results then reproduce the reference's prints to the last printed
            digit of fmax (1e-5 eV/A).  Applies to ``calculate``, ``calculate_batch`` and the
            single-point form of ``evaluate_packed``; relaxations move fp64 positions on the device either way.
        properties: like nff's ``NeuralFF(properties=[...])``; with ``"embedding"`` in it ``results["embedding"]`` holds the
            per-atom latent features ``[N, F]`` (final scalar state, F = the models' ``feat_dim``) of the first model -- the
            reference computes them with ``NeuralFF(models[0], properties=["energy", "forces", "embedding"])`` -- and
            ``results["embedding_models"]`` those of every ensemble member ``[M, N, F]``.
        hparams: PaiNN hyper-parameters (``checkpoint.DEFAULT_HPARAMS`` keys), or ``"auto"``: every model must then be a
            checkpoint (path or module) and its shapes are read from its tensors (``checkpoint.infer_hparams``), with a
            ``params.json`` next to a ``best_model`` file read as well; all models must agree.
    """

    # "stress" / "stress_std" like nff's EnsembleNFF (the reference's class attribute, calculators.py:369, inherits them): the
    # virial of the same evaluation, Voigt 6-vector in eV / A^3 (what ase.Atoms.get_stress asks a calculator for)
    implemented_properties = ("energy", "forces", "stress", "energy_std", "forces_std", "stress_std", "surface_energy", "embedding")
    name = "ensemble_nff_surface_mi355x"
    _pack = staticmethod(structures.as_arrays)   # the hooks of _DynamicsFrontEnds
    _dynamics_want = backend.WANT_ALL

    def __init__(self, models, device="cuda", model_units="kcal/mol", prediction_units="eV",
                 offset_units="atomic", cutoff=None, hparams=None, logger=None, properties=("energy", "forces"),
                 position_dtype="float64", **kwargs):
        # a single model is accepted as well: the reference's NFFPourbaix is a NeuralFF and is constructed with ONE module,
        # NFFPourbaix(models[0], device=..., model_units=..., prediction_units="eV") (scripts/sample_pourbaix_surface.py:253-258)
        if isinstance(models, (str, bytes)) or hasattr(models, "__fspath__") or hasattr(models, "state_dict") \
                or (isinstance(models, np.ndarray) and models.ndim == 1):
            models = [models]
        if isinstance(hparams, str):
            if hparams != "auto":
                raise ValueError(f"hparams must be a dict, None or 'auto', not {hparams!r}")
            loaded = [self._load_model_auto(m) for m in models]
            hparams = loaded[0][1]
            for _, hp in loaded[1:]:
                if hp != hparams:
                    raise ValueError(f"ensemble members disagree on their hyper-parameters: {hparams} vs {hp}")
            self.models = [blob for blob, _ in loaded]
            model_cutoff = float(hparams["cutoff"])
            if cutoff is None:
                cutoff = model_cutoff
            elif abs(float(cutoff) - model_cutoff) > 1e-9:
                raise ValueError(f"cutoff={cutoff!r} differs from the models' cutoff {model_cutoff!r} (hparams='auto')")
        else:
            self.models = [self._load_model(m, hparams) for m in models]
        # like NeuralFF(properties=[...]) in the reference's clustering script (scripts/clustering.py:150-158): "embedding" in
        # this list makes every calculate() also return the latent features
        self.properties = tuple(properties)
        self.device = device
        self.model_units = model_units
        self.prediction_units = prediction_units
        self.offset_units = offset_units
        self.cutoff = 5.0 if cutoff is None else float(cutoff)
        if str(np.dtype(position_dtype)) not in ("float64", "float32"):
            raise ValueError(f"position_dtype must be float64 or float32, not {position_dtype!r}")
        self.position_dtype = str(np.dtype(position_dtype))
        self.hparams = dict(hparams or {})
        self.chem_pots: dict = {}
        self.offset_data: dict = {}
        self.logger = logger or logging.getLogger(__name__)
        self._engine = None
        self._engine_key = None
        super().__init__(**kwargs)

    @staticmethod
    def _load_model(m, hparams):
        """A model may be a checkpoint path (nff ``best_model`` or canonical ``.f32``), a float32 blob in the canonical
        layout, or -- what ``scripts/sample_surface.py:164-174`` passes -- an nff ``Painn`` module (anything with
        ``state_dict()``): its tensors are taken over, its excluded-volume / cutoff attributes are checked against
        ``hparams`` like those of a checkpoint file."""
        if isinstance(m, (str, bytes)) or hasattr(m, "__fspath__"):
            return checkpoint.load_painn_blob(str(m), hparams)
        if hasattr(m, "state_dict") and callable(m.state_dict):
            sd = {}
            for k, v in m.state_dict().items():
                for attr in ("detach", "cpu", "numpy"):
                    if hasattr(v, attr):
                        v = getattr(v, attr)()
                sd[k] = np.asarray(v, dtype=np.float32)
            attrs = {a: getattr(m, a) for a in ("excl_vol", "power", "sigma", "cutoff") if hasattr(m, a)}
            checkpoint.check_model_against_hparams(type(m).__name__, sd, hparams, attrs=attrs)
            return checkpoint.state_dict_to_blob(sd, hparams)
        blob = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
        checkpoint.blob_to_fields(blob, hparams)
        return blob

    @staticmethod
    def _load_model_auto(m):
        """(blob, hparams) of a checkpoint path or an nff ``Painn`` module, shapes inferred from the tensors."""
        if isinstance(m, (str, bytes)) or hasattr(m, "__fspath__"):
            return checkpoint.load_painn_blob_auto(str(m))
        if hasattr(m, "state_dict") and callable(m.state_dict):
            sd = {}
            for k, v in m.state_dict().items():
                for attr in ("detach", "cpu", "numpy"):
                    if hasattr(v, attr):
                        v = getattr(v, attr)()
                sd[k] = np.asarray(v, dtype=np.float32)
            hp = checkpoint.infer_hparams(sd)
            attrs = {a: getattr(m, a) for a in ("excl_vol", "power", "sigma", "cutoff") if hasattr(m, a)}
            for attr, key in (("excl_vol", "excl_vol"), ("power", "V_ex_power"), ("sigma", "V_ex_sigma"), ("cutoff", "cutoff")):
                if attr in attrs and attrs[attr] is not None:
                    hp[key] = attrs[attr]
            checkpoint.check_model_against_hparams(type(m).__name__, sd, hp, attrs=attrs)
            return checkpoint.state_dict_to_blob(sd, hp), hp
        raise ValueError("hparams='auto' needs checkpoints (paths or modules): a raw blob does not carry its shape")

    # -- engine lifetime (lazy: created on first use, re-created when the offset config changes) ----
    def _offset_config(self):
        if self.parameters.get("offset", False) and self.offset_data and "stoidict" in self.offset_data:
            table, const = stoich_offset_table(self.offset_data, offset_units=self.offset_units)
            return table, const
        return None, 0.0

    def _get_engine(self):
        table, const = self._offset_config()
        key = (None if table is None else table.tobytes(), const, _device_index(self.device), self.cutoff)
        if self._engine is None or key != self._engine_key:
            if self._engine is not None:
                self._engine.close()
            self._engine = backend.PainnEngine(
                self.models, device=_device_index(self.device), cutoff=self.cutoff,
                model_units_per_ev=_units_per_ev(self.model_units, self.prediction_units),
                offset_per_z=table, offset_const=const, hparams=self.hparams)
            self._engine_key = key
        return self._engine

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k in ("_engine", "_engine_key"):
                setattr(new, k, None)
            elif k in ("_extra_engines", "_extra_key"):
                continue
            elif k in ("models", "logger"):
                setattr(new, k, v)  # weights are immutable: share
            else:
                setattr(new, k, copy.deepcopy(v, memo))
        return new

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        state["_engine_key"] = None
        state.pop("_extra_engines", None)
        state.pop("_extra_key", None)
        state["logger"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        if self.logger is None:
            self.logger = logging.getLogger(__name__)

    # -- reference surface -----------------------------------------------------------------------------
    def set(self, **kwargs) -> dict:
        """Set parameters; ``chem_pots`` / ``offset_data`` are mirrored onto attributes
        (reference ``calculators.py:448-466``)."""
        if "linesearch_driver" in kwargs:
            backend.linesearch_driver_check(kwargs["linesearch_driver"])   # (ValueError before anything is stored)
        changed = _Base.set(self, **kwargs)
        if "chem_pots" in self.parameters:
            self.chem_pots = self.parameters["chem_pots"]
            self.logger.info("chemical potentials: %s are set from parameters", self.chem_pots)
        if "offset_data" in self.parameters:
            self.offset_data = self.parameters["offset_data"]
            self.logger.info("offset data: %s is set from parameters", self.offset_data)
        return changed

    def get_surface_energy(self, atoms=None, chem_pots: dict | None = None, offset_data: dict | None = None) -> float:
        """Surface energy = E_slab - bulk reference - chemical-potential deviation
        (reference ``calculators.py:379-446``).  Raises ValueError when the chemical potentials or the
        offset data are not set."""
        if atoms is None:
            atoms = self.atoms
        if chem_pots is None:
            chem_pots = self.chem_pots
        if not chem_pots:
            raise ValueError("chemical potentials are not set")
        if offset_data is None:
            offset_data = self.offset_data
        if not offset_data:
            raise ValueError("offset data is not set")
        energy = self.get_potential_energy(atoms=atoms)
        return surface_energy_from_energy(energy, atoms.get_chemical_symbols(), chem_pots, offset_data,
                                          self.offset_units)

    def surface_energy_of(self, energy, atoms):
        """Surface energy of a configuration whose potential energy is already known (used by the batched paths and by
        ``mc.ChainEnsemble``); subclasses override the arithmetic (``NFFPourbaix``)."""
        return surface_energy_from_energy(energy, atoms.get_chemical_symbols(),
                                          self._require(self.chem_pots, "chemical potentials"),
                                          self._require(self.offset_data, "offset data"), self.offset_units)

    def _arrays(self, atoms):
        """(numbers, positions, cell, pbc) of an Atoms-like for the ABI, positions rounded as ``position_dtype`` says."""
        Z, pos, cell, pbc = structures.as_arrays(atoms)
        if self.__dict__.get("position_dtype", "float64") == "float32":
            pos = np.asarray(pos, dtype=np.float64).astype(np.float32).astype(np.float64)
        return Z, pos, cell, pbc

    def _fill_results(self, res, b, a0, a1):
        """The results dict of configuration ``b`` (atoms ``a0:a1``) of a downloaded batch."""
        return {
            "energy": res["energy"][b:b + 1].copy(),            # shape (1,), like the reference
            "energy_std": res["energy_std"][b:b + 1].copy(),
            "forces": res["forces"][a0:a1].copy(),
            "forces_std": res["forces_std"][a0:a1].copy(),
            "energy_models": res["energy_models"][b].copy(),
            # ensemble-mean per-atom energies in eV (the stoichiometric offset is not distributed over atoms); what the
            # reference's Boltzmann-weighted switch proposal reads from results["per_atom_energies"] (mcmc/slab.py:92)
            "per_atom_energies": res["energy_atoms"][a0:a1].copy(),
            # the evaluation left the range of the fp16-split arithmetic (backend.saturated): finite, but not the model's
            "saturated": bool(res["saturated"][b]) if "saturated" in res else False,
            # the same ensemble mean / spread without the float32 result word (vssr_batch_energy_f64): the reference's
            # results["energy"] is a float32 tensor (calculators.py:484) and stays one; acceptance tests and relaxation drivers
            # of this package compare these
            **({"energy_f64": float(res["energy_f64"][b]), "energy_std_f64": float(res["energy_std_f64"][b])}
               if "energy_f64" in res else {}),
        }

    def calculate(self, atoms=None, properties=implemented_properties, system_changes=all_changes):
        """One ensemble energy+force evaluation (reference ``calculators.py:468-489``)."""
        if atoms is None:
            atoms = self.atoms
        _Base.calculate(self, atoms, properties, system_changes)
        eng = self._get_engine()
        res = eng.evaluate([self._arrays(atoms)])
        # a fresh dict per calculation, like nff's NeuralFF / EnsembleNFF.calculate: entries of an earlier structure that this
        # call does not produce (surface_energy, stress, embedding) must not survive a direct calculate() on another one
        self.results = self._fill_results(res, 0, 0, int(res["cfg_start"][1]))
        if "stress" in properties or "stress_std" in properties:
            st, sd = eng.stress()
            self.results["stress"], self.results["stress_std"] = st[0], sd[0]
        if "embedding" in self.properties or "embedding" in tuple(properties) and tuple(properties) != tuple(self.implemented_properties):
            emb = eng.embedding()
            self.results["embedding"] = emb[0]
            self.results["embedding_models"] = emb
        if self.results["saturated"]:
            self.logger.warning("activations left the fp16-split range (|x| > 65504): energy %.6g eV is not reliable",
                                float(self.results["energy"][0]))
        if "surface_energy" in properties:
            self.results["surface_energy"] = self.surface_energy_of(self.results["energy"], atoms)
        if hasattr(atoms, "results") and isinstance(atoms.results, dict):
            atoms.results.update(self.results)

    @staticmethod
    def _require(value, what):
        if not value:
            raise ValueError(f"{what} are not set" if what.endswith("s") else f"{what} is not set")
        return value

    # -- new capability: many independent chains in one lock-step evaluation ----------------------------
    def calculate_batch(self, atoms_list, want_surface_energy: bool = False, want_embedding: bool | None = None,
                        want_stress: bool = False, uncertainty=None, uncertainty_rows: str = "atoms",
                        uncertainty_model: int = 0) -> list[dict]:
        """Evaluate B independent configurations at once; returns one results dict per configuration
        (``want_embedding``: default = ``"embedding" in self.properties``; ``want_stress``: also ``stress`` / ``stress_std``).
        ``uncertainty``: a fitted ``uncertainty.GMMUncertainty``; adds ``results["uncertainty"]`` per structure, scored on the
        GPU from the resident embedding of ensemble member ``uncertainty_model`` (``uncertainty_rows``: "atoms" = every atom,
        reduced by the instance's order; "mean" = the structure's mean embedding row) -- what the instance returns for the
        same batch on the host.  The embedding is not downloaded for it."""
        eng = self._get_engine()
        res = eng.evaluate([self._arrays(a) for a in atoms_list])
        stress = eng.stress() if want_stress else None
        if want_embedding is None:
            want_embedding = "embedding" in self.properties
        emb = eng.embedding() if want_embedding else None
        unc = None
        if uncertainty is not None:
            _, unc = uncertainty.score_resident(eng, model=uncertainty_model, rows=uncertainty_rows)
            unc = unc.numpy()
        per_atom_unc = unc is not None and uncertainty_rows == "atoms" and "system" not in uncertainty.order
        out = []
        for b, atoms in enumerate(atoms_list):
            a0, a1 = int(res["cfg_start"][b]), int(res["cfg_start"][b + 1])
            r = self._fill_results(res, b, a0, a1)
            if want_surface_energy:
                r["surface_energy"] = self.surface_energy_of(r["energy"], atoms)
            if stress is not None:
                r["stress"], r["stress_std"] = stress[0][b].copy(), stress[1][b].copy()
            if emb is not None:
                r["embedding"] = emb[0, a0:a1].copy()
                r["embedding_models"] = emb[:, a0:a1].copy()
            if unc is not None:
                r["uncertainty"] = unc[a0:a1].copy() if per_atom_unc else np.float64(unc.reshape(-1)[b])
            out.append(r)
        return out


    ENERGY_THRESHOLD, MAX_FORCE_THRESHOLD = ENERGY_THRESHOLD, MAX_FORCE_THRESHOLD   # (the module's; an instance may override them)
    # evaluate_packed: engines (HIP streams) the chains of a batch are split over, and the smallest part worth a stream
    streams = 2
    MIN_CHAINS_PER_STREAM = 32

    def _get_engines(self, n: int):
        """``n`` engines with this calculator's configuration: the first is the calculator's own, the others are created on
        first use (weights are shared on the host, every engine holds its own device copy and workspaces)."""
        first = self._get_engine()
        extra = self.__dict__.setdefault("_extra_engines", [])
        if self.__dict__.get("_extra_key") != self._engine_key:
            for e in extra:
                e.close()
            extra.clear()
            self.__dict__["_extra_key"] = self._engine_key
        table, const = self._offset_config()
        while len(extra) < n - 1:
            extra.append(backend.PainnEngine(
                self.models, device=_device_index(self.device), cutoff=self.cutoff,
                model_units_per_ev=_units_per_ev(self.model_units, self.prediction_units),
                offset_per_z=table, offset_const=const, hparams=self.hparams))
        return [first] + extra[: n - 1]

    @staticmethod
    def packed_supported(relax: bool, optimizer) -> bool:
        """Whether ``evaluate_packed`` serves this request: everything but relaxations with a host-driven optimizer (an optimizer
        class, "BFGSLineSearch", the LAMMPS-style "CG")."""
        return not relax or optimizer is None or (isinstance(optimizer, str)
                                                  and not any(k in optimizer for k in ("CG", "LAMMPS", "BFGSLineSearch")))

    def evaluate_packed(self, n_atoms, Z, pos, cell, pbc, relax: bool = False, fixed_mask=None, relax_steps: int = 20,
                        fmax: float = 0.01, optimizer=None) -> dict:
        """Arrays in, arrays out: the batched evaluation (``relax=False``: ``calculate_batch``) or lock-step relaxation
        (``relax=True``: ``relax_batch`` with a device optimizer, "BFGS" / "FIRE") of B slabs given as the ABI's packed arrays
        (``n_atoms [B]``, ``Z [sum N]``, ``pos [sum N, 3]``, ``cell [B, 9]``, ``pbc [B, 3]``; ``fixed_mask [sum N]`` = FixAtoms).
        No per-slab Python objects on either side -- what ``mc.ChainEnsemble`` calls every MC step.  Returns ``energy [B]``
        (float32, the TRUE energies of the final geometries), ``energy_std``, ``forces``, ``energy_atoms``, ``positions``
        (relaxed, or the input), ``cfg_start``, ``saturated [B]``, ``oob [B]`` (the reference's +-1000 guard,
        ``mcmc/dynamics.py:159-168``; a saturated evaluation counts), and for relaxations ``n_steps`` / ``converged``."""
        if relax and optimizer is None:
            optimizer = self.parameters.get("optimizer", "FIRE")
        n_atoms = np.ascontiguousarray(n_atoms, dtype=np.int64)
        Z = np.asarray(Z)
        B = len(n_atoms)

        def one(eng, c0, c1, a0, a1):
            eng.upload_arrays(n_atoms[c0:c1], Z[a0:a1], pos[a0:a1], cell[c0:c1], pbc[c0:c1])
            inf = None
            if relax:
                inf = eng.relax(optimizer, fixed=None if fixed_mask is None else fixed_mask[a0:a1], max_steps=relax_steps,
                                fmax=fmax)   # (raises for host-driven optimizers)
            else:
                eng.run()
            return eng.download(), inf

        pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        if not relax and self.__dict__.get("position_dtype", "float64") == "float32":
            pos = pos.astype(np.float32).astype(np.float64)   # single points on nff's float32 nxyz (see the class docstring)
        cell, pbc = np.asarray(cell, dtype=np.float64).reshape(B, 9), np.asarray(pbc).reshape(B, 3)
        # (a single lock-step evaluation is too short to pay for the second host thread: measured 15.4 vs 15.0 ms per MC step)
        n_str = self.streams if (relax and B >= 2 * self.MIN_CHAINS_PER_STREAM) else 1
        if n_str <= 1:
            res, info = one(self._get_engine(), 0, B, 0, int(n_atoms.sum()))
        else:
            # the chains split over n_str engines (own HIP streams) that run concurrently: the latency-bound node kernels of one
            # part fill issue slots under the neighbor-sum kernels of the other (+3 % on 256 chains).  ctypes
            # releases the GIL inside the C calls, one host thread per engine drives its relaxation; a chain's results do not
            # depend on the split (bit-identical, tests/test_mc_gpu.py).
            from concurrent.futures import ThreadPoolExecutor

            cb = [(k * B) // n_str for k in range(n_str + 1)]
            ab = _cfg_start(n_atoms)
            engines = self._get_engines(n_str)
            with ThreadPoolExecutor(max_workers=n_str) as pool:
                parts = list(pool.map(lambda k: one(engines[k], cb[k], cb[k + 1], int(ab[cb[k]]), int(ab[cb[k + 1]])), range(n_str)))
            res = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0] if k != "cfg_start"}
            res["cfg_start"] = ab
            info = None
            if relax:
                info = {k: np.concatenate([p[1][k] for p in parts]) for k in ("positions", "n_steps", "converged")}
        start = np.asarray(res["cfg_start"], dtype=np.int64)
        energy = res["energy"]
        e64 = np.asarray(res["energy_f64"] if "energy_f64" in res else energy, dtype=np.float64)
        saturated = np.asarray(res["saturated"], dtype=bool)
        out = {"energy": energy, "energy_std": res["energy_std"], "forces": res["forces"], "energy_atoms": res["energy_atoms"],
               "positions": info["positions"] if info is not None else np.asarray(pos, dtype=np.float64).reshape(-1, 3),
               "cfg_start": start, "saturated": saturated, "energy_f64": e64,
               "oob": _oob_flags(energy, res["forces"], start, saturated, e_max=self.ENERGY_THRESHOLD, f_max=self.MAX_FORCE_THRESHOLD),
               "energy_std_f64": np.asarray(res["energy_std_f64"] if "energy_std_f64" in res else res["energy_std"], dtype=np.float64)}
        if info is not None:
            out["n_steps"], out["converged"] = info["n_steps"], info["converged"]
        return out

    # -- who drives relax_batch's resident batch.  Each returns ``(info, trajs)``: ``info`` = ``positions``, the count arrays ``n_steps`` /
    # ``converged`` (line search: also ``n_eval`` / ``stop_reason``), ``results`` (the final download); ``trajs`` per chain, or None ----
    def _relax_by_class(self, eng, opt_cls, atoms_list, start, fixed_indices, fixed, steps, fmax, record_interval, quiet):
        """Any optimizer of the ASE protocol, one per chain on the host, served by lock-step evaluations (host_opt.py)."""
        info = host_opt.optimizer_class_batch(opt_cls, atoms_list, _LockstepProxy, _lockstep_evaluate(eng), start, fixed_indices=fixed_indices,
                                              steps=steps, fmax=fmax, record_interval=record_interval,
                                              optimizer_kwargs={"logfile": None} if quiet else {})
        eng.set_positions(info["positions"])
        eng.run()
        res = eng.download()
        # ASE optimizers count their steps; converged: ASE's criterion on the final forces (constraints applied)
        ff = np.array(res["forces"], dtype=np.float64, copy=True)
        if fixed is not None:
            ff[fixed.astype(bool)] = 0.0
        f2 = (ff ** 2).sum(axis=1)
        return {"positions": info["positions"], "n_steps": np.array([int(getattr(d, "nsteps", -1)) for d in info["optimizers"]], np.int32),
                "converged": np.array([a1 == a0 or bool(f2[a0:a1].max() < fmax ** 2) for a0, a1 in zip(start[:-1], start[1:])], bool),
                "results": res}, info["traj"]

    def _relax_by_host_cg(self, eng, atoms_list, start, fixed, steps, fmax, record_interval):
        """The reference maps "CG" to ASE's SciPyFminCG (mcmc/dynamics.py:123-124): scipy owns the control flow, so every chain's
        optimizer runs on the host and their energy / force requests are served by lock-step evaluations (host_opt.py)."""
        pos0 = np.concatenate([np.asarray(a.get_positions(), dtype=np.float64).reshape(-1, 3) for a in atoms_list])
        info = host_opt.scipy_cg_batch(_lockstep_evaluate(eng), start, pos0, fixed=fixed, steps=steps, fmax=fmax, record_interval=record_interval)
        eng.set_positions(info["positions"])
        eng.run()
        info["results"] = eng.download()
        return info, [{"atoms": _traj_frames(atoms, [p for p, _, _ in recs]), "energies": [float(e) for _, e, _ in recs],
                       "forces": [np.asarray(f, dtype=np.float32) for _, _, f in recs]} for atoms, recs in zip(atoms_list, info["traj"] or [])]

    def _relax_by_linesearch(self, eng, atoms_list, start, fixed, steps, fmax, record_interval):
        """The device's lock-step BFGSLineSearch (``backend.relax_bfgs_linesearch``)."""
        info = eng.relax_bfgs_linesearch(fixed=fixed, max_steps=steps, fmax=fmax, record_interval=record_interval)
        info["results"] = eng.download()
        return info, [_traj_of_chain(info.get("traj"), b, int(start[b]), int(start[b + 1]), a) for b, a in enumerate(atoms_list)]

    def _relax_by_device(self, eng, optimizer, atoms_list, start, fixed, steps, fmax, record_interval):
        """The device's lock-step FIRE / BFGS, chosen by the optimizer's name (``backend.relax``)."""
        info = eng.relax(optimizer, fixed=fixed, max_steps=steps, fmax=fmax, record_interval=record_interval)
        info["results"] = eng.download()
        return info, [_traj_of_chain(info.get("traj"), b, int(start[b]), int(start[b + 1]), a) for b, a in enumerate(atoms_list)]

    def relax_batch(self, atoms_list, fixed_indices=None, relax_steps: int = 20, fmax: float = 0.01, optimizer=None,
                    save_traj: bool = False, record_interval: int = 5, linesearch_driver=None):
        """Relax B independent slabs at once on the device — the batched counterpart of
        ``optimize_slab(slab, optimizer=..., relax_steps=..., save_traj=..., record_interval=...)`` (reference
        ``mcmc/dynamics.py:83-170``).  ``optimizer``: "BFGS" (ASE BFGS, the reference's SrTiO3 setting,
        ``scripts/configs/sample_config_painn.json:26``), "FIRE" (the reference's default) or "CG" (ASE SciPyFminCG: host-driven scipy
        optimizers over lock-step device evaluations, ``host_opt.py``); None takes
        ``parameters["optimizer"]`` (how ``calc_settings`` reach ``optimize_slab``), else "FIRE".
        ``fixed_indices``: per slab, the atom indices held by FixAtoms (or None).
        Returns, per slab, the reference's tuple ``(relaxed_slab, traj, energy, energy_oob)`` where ``energy_oob`` follows
        the same +-1000 guard (a saturated evaluation counts as out of bounds), plus the results dict of the final
        evaluation.  ``save_traj=True``: ``traj`` is the reference's dict ``{"atoms", "energies", "forces"}`` recorded like
        its TrajectoryObserver attached with ``interval=record_interval`` (after 0, k, 2k, ... optimizer steps; forces with
        FixAtoms applied); otherwise None.
        ``linesearch_driver`` (default: ``set(linesearch_driver=...)``, else "ase"): who runs ``optimizer="BFGSLineSearch"`` --
        "ase": ASE's class, one host optimizer per chain (an error where ASE is not importable); "device": the lock-step device
        optimizer (``backend.relax_bfgs_linesearch``), whose results dicts also carry ``n_eval`` and ``stop_reason``."""
        ls_driver = backend.linesearch_driver_check(self.parameters.get("linesearch_driver", "ase") if linesearch_driver is None
                                                    else linesearch_driver)
        eng = self._get_engine()
        packs = [structures.as_arrays(a) for a in atoms_list]
        eng.upload(packs)
        start = _cfg_start([len(p[0]) for p in packs])
        fixed = _fixed_mask(np.diff(start), fixed_indices)
        if optimizer is None:
            optimizer = self.parameters.get("optimizer", "FIRE")
        record = int(record_interval) if save_traj else 0
        opt_cls = optimizer if callable(optimizer) else None
        line_search = opt_cls is None and "BFGSLineSearch" in str(optimizer)
        if line_search and ls_driver != "device":
            try:   # the reference's import (mcmc/dynamics.py:7): only where ASE is installed
                from ase.optimize import BFGSLineSearch as opt_cls
            except Exception as exc:
                raise backend.BackendError('optimizer "BFGSLineSearch" is ASE\'s class and ASE is not importable here; pass an '
                                           "optimizer class, or use BFGS / FIRE / CG") from exc
        if opt_cls is not None:
            info, trajs = self._relax_by_class(eng, opt_cls, atoms_list, start, fixed_indices, fixed, relax_steps, fmax, record,
                                               quiet=HAVE_ASE and not callable(optimizer))
        elif "CG" in str(optimizer) and "LAMMPS" not in str(optimizer):
            info, trajs = self._relax_by_host_cg(eng, atoms_list, start, fixed, relax_steps, fmax, record)
        elif line_search:
            info, trajs = self._relax_by_linesearch(eng, atoms_list, start, fixed, relax_steps, fmax, record)
        else:
            info, trajs = self._relax_by_device(eng, optimizer, atoms_list, start, fixed, relax_steps, fmax, record)
        res = info["results"]
        e64 = np.asarray(res["energy_f64"] if "energy_f64" in res else res["energy"], dtype=np.float64)
        oob = _oob_flags(e64, res["forces"], start, res.get("saturated"), e_max=self.ENERGY_THRESHOLD, f_max=self.MAX_FORCE_THRESHOLD)
        out = []
        for b, atoms in enumerate(atoms_list):
            a0, a1 = int(start[b]), int(start[b + 1])
            relaxed = atoms.copy()
            relaxed.set_positions(info["positions"][a0:a1])
            r = self._fill_results(res, b, a0, a1)
            r["n_steps"], r["converged"] = int(info["n_steps"][b]), bool(info["converged"][b])
            if "n_eval" in info:
                r["n_eval"], r["stop_reason"] = int(info["n_eval"][b]), int(info["stop_reason"][b])
            out.append((relaxed, trajs[b] if trajs else None, self.ENERGY_THRESHOLD if oob[b] else float(e64[b]), bool(oob[b]), r))
        return out


def surface_energy_from_counts(energy, counts: dict, chem_pots: dict, offset_data: dict, offset_units: str = "atomic"):
    """:func:`surface_energy_from_energy` for MANY slabs at once: ``energy`` ``[B]`` and ``counts`` = element symbol ->
    ``[B]`` atom counts, the dict's key order being the order in which the elements first appear in the slabs' atom lists
    (the scalar function walks a ``Counter`` in that order).  Same operations in the same order per slab, so every entry
    equals the scalar result bit for bit (``tests/test_mc.py``)."""
    energy = np.asarray(energy, dtype=np.float64)
    bulk_energies, stoics = offset_data["bulk_energies"], offset_data["stoics"]
    ref_formula, ref_element = offset_data["ref_formula"], offset_data["ref_element"]
    n = {k: np.asarray(v, dtype=np.float64) for k, v in counts.items()}
    n_ref = n.get(ref_element, np.zeros_like(energy))
    bulk_ref_en = n_ref * bulk_energies[ref_formula]
    for ele, n_e in n.items():
        if ele != ref_element:
            bulk_ref_en = bulk_ref_en + (n_e - stoics[ele] / stoics[ref_element] * n_ref) * bulk_energies[ele]
    surface_energy = energy - (bulk_ref_en * HARTREE_TO_EV if offset_units == "atomic" else bulk_ref_en)
    pot = np.zeros_like(energy)
    for ele, n_e in n.items():
        if ele != ref_element:
            pot = pot + (n_e - stoics[ele] / stoics[ref_element] * n_ref) * chem_pots[ele]
    return surface_energy - pot


def _traj_frames(atoms, positions):
    """Copies of ``atoms`` at each of ``positions``, without the calculator (the reference's observer stores such copies)."""
    frames = []
    for pos in positions:
        frame = atoms.copy()
        frame.set_positions(pos)
        if hasattr(frame, "calc"):
            frame.calc = None
        frames.append(frame)
    return frames


def _traj_of_chain(traj, b, a0, a1, atoms):
    """Records of chain b of a device trajectory in the layout of the reference's ``optimize_slab`` (``mcmc/dynamics.py:145-151``)."""
    if traj is None:
        return None
    n = int(traj["n_records"][b])
    return {"atoms": _traj_frames(atoms, traj["positions"][:n, a0:a1]), "energies": [float(traj["energies"][r, b]) for r in range(n)],
            "forces": [traj["forces"][r, a0:a1].copy() for r in range(n)]}


# ---- helpers of the reference's clustering / uncertainty scripts (mcmc/calculators/calculators.py:34-135) ------------------
def get_results_single(atoms_batch, calc) -> dict:
    """One calculation of ``atoms_batch`` with ``calc``; returns ``calc.results`` (reference ``:34-47``)."""
    atoms_batch.calc = calc
    calc.calculate(atoms_batch)
    return calc.results


def get_embeddings_single(atoms_batch, calc, results_cache: dict | None = None, flatten: bool = True,
                          flatten_axis: int = 0) -> np.ndarray:
    """Latent-space embedding of one structure (reference ``:67-93``): the per-atom features ``results["embedding"]``
    averaged over ``flatten_axis`` (atoms) when ``flatten``; ``results_cache`` avoids a second evaluation.  The calculator
    must provide the embedding (``EnsembleNFFSurface(..., properties=[..., "embedding"])``)."""
    results = results_cache if results_cache is not None and "embedding" in results_cache \
        else get_results_single(atoms_batch, calc)
    if "embedding" not in results:
        raise KeyError('the calculator returns no "embedding": construct it with properties=(..., "embedding")')
    emb = np.asarray(results["embedding"])
    return emb.mean(axis=flatten_axis).squeeze() if flatten else emb.squeeze()


def get_embeddings(atoms_batches, calc) -> np.ndarray:
    """One embedding row per structure (reference ``:50-64``)."""
    return np.stack([get_embeddings_single(a, calc) for a in atoms_batches])


def get_std_devs_single(atoms_batch, calc):
    """Mean ensemble standard deviation of the force components of one structure, 0.0 for a single model (reference
    ``:117-135``)."""
    if len(calc.models) > 1:
        atoms_batch.calc = calc
        calc.calculate(atoms_batch)
        return calc.results.get("forces_std", np.array([0.0])).mean()
    return 0.0


def get_std_devs(atoms_batches, calc) -> np.ndarray:
    """Force standard deviation of every structure (reference ``:96-114``)."""
    return np.stack([get_std_devs_single(a, calc) for a in atoms_batches])


@dataclasses.dataclass
class PourbaixAtom:
    """Per-element data of the Pourbaix dissolution reaction (reference ``mcmc/pourbaix/atoms.py:25-66``)."""

    symbol: str
    dominant_species: str = ""
    species_conc: float = 1e-6
    num_e: int = 0
    num_H: int = 0
    atom_std_state_energy: float = 0.0
    delta_G2_std: float = 0.0


def _formula_counts(formula: str) -> Counter:
    """Element counts of a plain formula string such as ``"OH"`` or ``"H2O"``."""
    out = Counter()
    for sym, num in re.findall(r"([A-Z][a-z]?)(\d*)", formula):
        out[sym] += int(num) if num else 1
    return out


def pourbaix_delta_G1(energy: float, symbols, pourbaix_atoms: dict, adsorbate_corrections: dict | None = None) -> float:
    """``NFFPourbaix.get_delta_G1`` (reference ``calculators.py:235-272``): ``sum_atoms E_std(atom) - (E_slab + adsorbate
    corrections)``.  Adsorbate corrections count how many times the adsorbate formula fits into the slab formula; for O-H
    adsorbates the hydrogens in excess of the oxygens are first attributed to water and removed (``:254-268``)."""
    counts = Counter(symbols)
    sum_std = sum(n * pourbaix_atoms[a].atom_std_state_energy for a, n in counts.items())
    slab_energy = float(np.ravel(energy)[0])
    formula = Counter(counts)
    for adsorbate, correction in (adsorbate_corrections or {}).items():
        if "O" in adsorbate and "H" in adsorbate:
            ho_diff = max(formula["H"] - formula["O"], 0)
            if ho_diff > 0:
                formula = Counter({k: v - {"H": 2, "O": 1}.get(k, 0) * ho_diff for k, v in formula.items()})
        ads = _formula_counts(adsorbate)
        div = min(formula[k] // n for k, n in ads.items()) if ads else 0
        slab_energy += div * correction
    return sum_std - slab_energy


def pourbaix_delta_G2(symbols, pourbaix_atoms: dict, temp: float = 0.0257, phi: float = 0.0, pH: float = 7.0) -> float:
    """``NFFPourbaix.get_delta_G2`` (reference ``calculators.py:197-233``): ``sum_atoms [dG2_std - n_e phi - ln(10) n_H kT pH +
    kT ln(conc)]``."""
    dg2 = 0.0
    for a, n in Counter(symbols).items():
        pa = pourbaix_atoms[a]
        dg2 += n * (pa.delta_G2_std - pa.num_e * phi - np.log(10) * pa.num_H * temp * pH + temp * np.log(pa.species_conc))
    return dg2


def pourbaix_potential_from_energy(energy: float, symbols, pourbaix_atoms: dict, temp: float = 0.0257, phi: float = 0.0,
                                   pH: float = 7.0, adsorbate_corrections: dict | None = None) -> float:
    """Pourbaix ("grand") potential of a slab with known potential energy — the arithmetic of the reference's
    ``NFFPourbaix`` (``calculators.py:197-305``): ``-(dG1 + dG2)`` with :func:`pourbaix_delta_G1` and :func:`pourbaix_delta_G2`."""
    return -(pourbaix_delta_G1(energy, symbols, pourbaix_atoms, adsorbate_corrections)
             + pourbaix_delta_G2(symbols, pourbaix_atoms, temp, phi, pH))


class NFFPourbaix(EnsembleNFFSurface):
    """Surface calculator whose ``surface_energy`` is the Pourbaix potential (reference ``NFFPourbaix``,
    ``calculators.py:121-357``; there a single-model ``NeuralFF``, here any ensemble size on the same engine).
    Parameters through ``set``: ``temperature`` (kT in eV), ``phi``, ``pH``, ``pourbaix_atoms`` (symbol ->
    ``PourbaixAtom``), ``adsorbate_corrections`` (formula -> eV)."""

    implemented_properties = (*EnsembleNFFSurface.implemented_properties, "pourbaix_potential")
    name = "nff_pourbaix_mi355x"

    def __init__(self, *args, temp: float = 0.0257, phi: float = 0.0, pH: float = 7.0, **kwargs):
        super().__init__(*args, **kwargs)
        self.temp, self.phi, self.pH = temp, phi, pH
        self.pourbaix_atoms: dict = {}
        self.adsorbate_corrections: dict = {}

    def set(self, **kwargs) -> dict:
        changed = super().set(**kwargs)
        for key, attr in (("temperature", "temp"), ("phi", "phi"), ("pH", "pH"), ("pourbaix_atoms", "pourbaix_atoms"),
                          ("adsorbate_corrections", "adsorbate_corrections")):
            if key in self.parameters:
                setattr(self, attr, self.parameters[key])
        return changed

    def get_delta_G2_individual(self, atom) -> float:
        pa = self.pourbaix_atoms[atom] if isinstance(atom, str) else atom
        return pa.delta_G2_std - pa.num_e * self.phi - np.log(10) * pa.num_H * self.temp * self.pH \
            + self.temp * np.log(pa.species_conc)

    def get_delta_G2(self, atoms=None) -> float:
        atoms = self.atoms if atoms is None else atoms
        return sum(self.get_delta_G2_individual(a) for a in atoms.get_chemical_symbols())

    def get_delta_G1(self, atoms=None) -> float:
        """Dissociation energy of all atoms incl. the adsorbate corrections (reference ``calculators.py:235-272``)."""
        atoms = self.atoms if atoms is None else atoms
        return pourbaix_delta_G1(self.get_potential_energy(atoms=atoms), atoms.get_chemical_symbols(),
                                 self._require(self.pourbaix_atoms, "Pourbaix atoms"), self.adsorbate_corrections)

    def surface_energy_of(self, energy, atoms):
        return pourbaix_potential_from_energy(energy, atoms.get_chemical_symbols(),
                                              self._require(self.pourbaix_atoms, "Pourbaix atoms"), self.temp, self.phi,
                                              self.pH, self.adsorbate_corrections)

    def get_pourbaix_potential(self, atoms=None) -> float:
        atoms = self.atoms if atoms is None else atoms
        return self.surface_energy_of(self.get_potential_energy(atoms=atoms), atoms)

    def get_surface_energy(self, atoms=None, **kwargs) -> float:
        return self.get_pourbaix_potential(atoms)

    def calculate(self, atoms=None, properties=implemented_properties, system_changes=all_changes):
        super().calculate(atoms, properties, system_changes)
        if "pourbaix_potential" in properties or "surface_energy" in properties:
            self.results["pourbaix_potential"] = self.results.get(
                "surface_energy", self.surface_energy_of(self.results["energy"], self.atoms if atoms is None else atoms))


class _AnalyticSurfCalc(_DynamicsFrontEnds, _Base):
    """Shared front end of the analytic potentials that the reference evaluates through LAMMPS (Tersoff, EAM): fp64
    ``energy`` / ``per_atom_energies`` / ``forces`` from the device, ``surface_energy`` = potential energy
    (reference ``calculators.py:707-719,766-777``), batched evaluation and lock-step relaxation for ``mc.ChainEnsemble``.
    ``stress`` (Voigt 6-vector, eV / A^3, ASE's sign: what ``ase.Atoms.get_stress`` asks for and the reference's ``lammpsrun``
    fills from ``pxx .. pxy``) is the device virial of the same evaluation (``vssr_batch_stress``), computed only when a call
    asks for it.  ``cg_driver`` (``set(cg_driver=...)``, or a keyword of ``relax_batch`` / ``run_lammps_opt`` / ``evaluate_packed``):
    ``"auto"`` (default), ``"lockstep"`` or ``"resident"`` -- the driver of the device CG minimiser (``backend.relax_cg_f64``)."""

    # what a calculate() without ``properties`` produces (its default argument); "stress" is served on request only
    _default_properties = ("energy", "relaxed_energy", "forces", "per_atom_energies", "surface_energy")
    implemented_properties = (*_default_properties, "stress")
    species: list = []
    _dynamics_want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM   # (_DynamicsFrontEnds; its other hook is _pack)

    def _init_common(self, device, all_periodic, logger):
        self.device = device
        self.all_periodic = bool(all_periodic)
        self.run_dir = None
        self.relax_steps = 100
        self.cg_driver = "auto"      # driver of the device CG minimiser: "auto" | "lockstep" | "resident" (backend.relax_cg_f64)
        self.linesearch_driver = "ase"   # who runs optimizer="BFGSLineSearch": "ase" | "device" (backend.relax_bfgs_linesearch)
        self.logger = logger or logging.getLogger(__name__)
        self._engine = None

    def _make_engine(self):
        raise NotImplementedError

    def _get_engine(self):
        if self._engine is None:
            self._engine = self._make_engine()
        return self._engine

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            setattr(new, k, None if k == "_engine" else (v if k in ("params", "funcfl", "tables", "logger") else copy.deepcopy(v, memo)))
        return new

    def set(self, **kwargs) -> dict:
        if "cg_driver" in kwargs:
            backend.cg_driver_code(kwargs["cg_driver"])   # (ValueError before anything is stored)
        if "linesearch_driver" in kwargs:
            backend.linesearch_driver_check(kwargs["linesearch_driver"])
        changed = _Base.set(self, **kwargs)
        if "run_dir" in self.parameters:
            self.run_dir = self.parameters["run_dir"]
        if "relax_steps" in self.parameters:
            self.relax_steps = self.parameters["relax_steps"]
        if "cg_driver" in self.parameters:
            self.cg_driver = self.parameters["cg_driver"]
        if "linesearch_driver" in self.parameters:
            self.linesearch_driver = self.parameters["linesearch_driver"]
        return changed

    def _cg_driver_of(self, kwargs) -> str:
        """The CG driver of one relaxation call, validated: its ``cg_driver`` keyword, else (absent or None) the calculator's setting."""
        driver = self.cg_driver if kwargs.get("cg_driver") is None else kwargs["cg_driver"]
        backend.cg_driver_code(driver)
        return driver

    def _pack(self, atoms):
        Z, pos, cell, pbc = structures.as_arrays(atoms)
        types = self._types_of(Z)
        fixed_pbc = self._fixed_pbc()
        if fixed_pbc is not None:
            pbc = fixed_pbc.copy()
        return types, pos, cell, pbc

    def _types_of(self, Z) -> np.ndarray:
        """LAMMPS types of atomic numbers (the order of ``species``), vectorised; an element outside ``species`` or the symbol table raises."""
        table = np.full(len(structures.SYMBOLS) + 1, -1, np.int32)   # (the last slot: where atomic numbers beyond the symbols land)
        for t, sym in enumerate(self.species):
            table[structures.ATOMIC_NUMBERS[sym]] = t
        Z = np.asarray(Z, dtype=np.int64)
        types = table[np.clip(Z, 0, len(table) - 1)]
        if len(Z) and (types.min() < 0 or Z.min() < 0):   # (a negative Z was clipped onto X, which may be among the species)
            raise ValueError(f"element Z={int(Z[np.argmax((types < 0) | (Z < 0))])} is not covered by the potential {self.species}")
        return types

    def _fixed_pbc(self):
        """The boundary the run directory's template (or ``all_periodic``) imposes on every slab, None: the atoms' own ``pbc``."""
        return np.ones(3, np.uint8) if self.all_periodic else None

    def get_surface_energy(self, atoms=None) -> float:
        """Currently the same as the potential energy (reference ``calculators.py:707-719``)."""
        if atoms is None:
            atoms = self.atoms
        return self.get_potential_energy(atoms=atoms)

    def _evaluate_slabs(self, atoms_list, want_stress: bool = False) -> list[dict]:
        """One device evaluation of the slabs: per slab ``energy`` / ``per_atom_energies`` / ``forces``, with ``want_stress`` also the
        virial of that evaluation.  ``calculate``, ``run_lammps_energy`` and ``calculate_batch`` return it in their own shapes."""
        packs = [self._pack(a) for a in atoms_list]
        eng = self._get_engine()
        e, ea, f = eng.evaluate_f64(packs)
        stress = eng.stress()[0] if want_stress else None
        start = _cfg_start([len(p[0]) for p in packs])
        out = []
        for b, (a0, a1) in enumerate(zip(start[:-1], start[1:])):
            out.append({"energy": float(e[b]), "per_atom_energies": ea[a0:a1].copy(), "forces": f[a0:a1].copy()})
            if stress is not None:
                out[-1]["stress"] = stress[b].copy()
        return out

    def calculate(self, atoms=None, properties=_default_properties, system_changes=all_changes):
        if atoms is None:
            atoms = self.atoms
        _Base.calculate(self, atoms, properties, system_changes)
        # the virial of THIS evaluation, or none: an entry an earlier call left behind must not answer a later get_stress()
        self.results.pop("stress", None)
        self.results.update(self._evaluate_slabs([atoms], want_stress="stress" in properties)[0])
        if "relaxed_energy" in properties:   # reference calculators.py:688-691
            _, e_rel, ea_rel = self.run_lammps_opt(atoms)
            self.results["relaxed_energy"] = e_rel
            self.results["per_atom_energies"] = ea_rel
        if "surface_energy" in properties:
            self.results["surface_energy"] = self.results["energy"]

    def run_lammps_energy(self, slab, run_dir=None, **kwargs):
        """``LAMMMPSCalc.run_lammps_energy`` (reference ``calculators.py:621-640``: the static energy through the run
        directory's ``lammps_energy_template.txt``): one device evaluation; returns the reference's tuple
        ``(slab, energy, per_atom_energies)``."""
        r = self._evaluate_slabs([slab])[0]
        return slab, r["energy"], r["per_atom_energies"]

    def calculate_batch(self, atoms_list, want_stress: bool = False) -> list[dict]:
        return self._evaluate_slabs(atoms_list, want_stress)

    def _relax_packed(self, n_atoms, types, pos, cell, pbc, fixed, optimizer, steps, fmax, *, etol, ftol, cg_driver, linesearch_driver,
                      max_eval, record_interval):
        """THE optimizer table of the analytic calculators, on the ABI's packed arrays: "CG" / "LAMMPS" (any case) -> the device CG
        minimiser (``etol`` / ``ftol`` / ``cg_driver``); a name with "BFGSLineSearch" where ``linesearch_driver`` is "device" -> the device
        line search (``fmax`` / ``max_eval`` / ``record_interval``); anything else -> FIRE / BFGS with ``fmax`` (the engine refuses other
        names).  Every branch ends with a complete evaluation of the relaxed geometries.  Returns fp64 ``(energy [B], e_atom [N], forces,
        positions, counts, traj)``: ``counts`` the per-chain arrays ``iterations`` / ``evaluations`` / ``stop`` (CG) or ``n_steps`` /
        ``converged`` (line search: also ``n_eval`` / ``stop_reason``), ``traj`` the device trajectory or None."""
        eng = self._get_engine()
        if str(optimizer).upper() in ("CG", "LAMMPS"):
            e, ea, f, new_pos, it, ev, why = eng.relax_cg_arrays_f64(n_atoms, types, pos, cell, pbc, fixed=fixed, max_iter=steps, etol=etol,
                                                                     ftol=ftol, driver=cg_driver)
            return e, ea, f, new_pos, {"iterations": it, "evaluations": ev, "stop": why}, None
        if "BFGSLineSearch" in str(optimizer) and linesearch_driver == "device":
            eng.upload_arrays(n_atoms, types, pos, cell, pbc)
            info = eng.relax_bfgs_linesearch(fixed=fixed, max_steps=steps, fmax=fmax, max_eval=max_eval, record_interval=record_interval,
                                             want=backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM)
            e, ea, f = eng.results_f64()   # (the driver ends with a complete evaluation of the final positions)
            return e, ea, f, info["positions"], {k: info[k] for k in ("n_steps", "n_eval", "stop_reason", "converged")}, info.get("traj")
        e, ea, f, new_pos, nst, conv = eng.relax_arrays_f64(n_atoms, types, pos, cell, pbc, fixed=fixed, max_steps=steps, fmax=fmax,
                                                            optimizer=optimizer)
        return e, ea, f, new_pos, {"n_steps": nst, "converged": conv}, None

    def run_lammps_opt(self, slab, run_dir=None, fixed_indices=None, optimizer="CG", **kwargs):
        """Relaxation counterpart of ``LAMMMPSCalc.run_lammps_opt`` (reference ``calculators.py:600-619``: LAMMPS
        ``min_style cg``, ``minimize 1e-5 1e-5 {relax_steps} 10000``, bulk atoms with ``setforce 0``): the same minimiser on
        the device (``vssr_batch_relax_cg``; ``etol`` / ``ftol`` keywords override 1e-5).  ``optimizer="FIRE"`` / ``"BFGS"``
        select the ASE-style optimizers with ``fmax`` (default 0.01) instead.  Returns the reference's tuple
        ``(relaxed_slab, energy, per_atom_energies)``; ``self.last_opt`` holds iteration / evaluation counts and the stop reason."""
        n_atoms, types, pos, cell, pbc = backend.pack_batch([self._pack(slab)])
        fixed = _fixed_mask(n_atoms, [fixed_indices] if fixed_indices is not None and len(fixed_indices) else None)
        e, ea, _, new_pos, counts, _ = self._relax_packed(
            n_atoms, types, pos, cell, pbc, fixed, optimizer, int(self.relax_steps),
            kwargs.get("fmax", 0.01), etol=kwargs.get("etol", 1e-5), ftol=kwargs.get("ftol", 1e-5), cg_driver=self._cg_driver_of(kwargs),
            linesearch_driver="ase", max_eval=None, record_interval=0)   # (one slab: no device line search, no trajectory)
        c = _chain_counts(counts, 0)
        self.last_opt = {"optimizer": "CG", **c} if "stop" in c else \
            {"optimizer": str(optimizer), "iterations": c["n_steps"], "converged": c["converged"]}
        relaxed = slab.copy()
        relaxed.set_positions(new_pos)
        relaxed.calc = getattr(slab, "calc", None)
        return relaxed, float(e[0]), ea

    ENERGY_THRESHOLD, MAX_FORCE_THRESHOLD = ENERGY_THRESHOLD, MAX_FORCE_THRESHOLD   # (the module's; an instance may override them)

    def relax_batch(self, atoms_list, fixed_indices=None, relax_steps: int | None = None, fmax: float = 0.01,
                    optimizer=None, want_stress: bool = False, *, etol: float = 1e-5, ftol: float = 1e-5, cg_driver=None,
                    linesearch_driver=None, max_eval=None, save_traj: bool = False, record_interval: int = 5, **kwargs):
        """Relax B slabs in ONE lock-step call -- what ``mc.ChainEnsemble(relax=True)`` needs from a calculator.  Default
        ``optimizer`` "LAMMPS" / "CG": the reference's GaN minimiser (``optimize_slab(optimizer="LAMMPS")`` ->
        ``run_lammps_opt``, ``mcmc/dynamics.py:107-116``) for all slabs at once (``vssr_batch_relax_cg``; ``etol`` / ``ftol``); "FIRE" /
        "BFGS" use the ASE-style optimizers with ``fmax`` (the table: ``_relax_packed``).  ``relax_steps`` defaults to
        ``self.relax_steps`` (the reference takes it from ``calc.relax_steps``).  Returns per slab ``(relaxed, None, energy,
        energy_oob, results)`` like ``EnsembleNFFSurface.relax_batch``; results carry ``per_atom_energies`` of the relaxed slab, with
        ``want_stress`` also its ``stress``.  ``cg_driver="auto" | "lockstep" | "resident"`` (None: the calculator's setting) selects the
        driver of the CG minimiser (``backend.relax_cg_f64``): same results bit for bit.  ``optimizer="BFGSLineSearch"`` runs on the device
        (``backend.relax_bfgs_linesearch``, at most ``max_eval`` evaluations per chain; results carry ``n_steps`` / ``n_eval`` /
        ``stop_reason``, and with ``save_traj`` / ``record_interval`` the tuple's trajectory) where ``linesearch_driver="device"`` says so --
        the keyword, else ``set(linesearch_driver=...)``; with the default "ase" the name is refused.  Other keywords are ignored."""
        ls_driver = backend.linesearch_driver_check(getattr(self, "linesearch_driver", "ase") if linesearch_driver is None
                                                    else linesearch_driver)
        if optimizer is None:
            optimizer = self.parameters.get("optimizer", "LAMMPS")
        steps = int(self.relax_steps if relax_steps is None else relax_steps)
        driver = self._cg_driver_of({"cg_driver": cg_driver})
        n_atoms, types, pos, cell, pbc = backend.pack_batch([self._pack(a) for a in atoms_list])
        e, ea, f, new_pos, counts, traj = self._relax_packed(
            n_atoms, types, pos, cell, pbc, _fixed_mask(n_atoms, fixed_indices), optimizer, steps, fmax, etol=etol, ftol=ftol,
            cg_driver=driver, linesearch_driver=ls_driver, max_eval=max_eval, record_interval=int(record_interval) if save_traj else 0)
        # (every relaxation, the chain-resident CG too, ends with one plain evaluation of the relaxed slabs: the virial is theirs)
        stress = self._get_engine().stress()[0] if want_stress else None
        start = _cfg_start(n_atoms)
        oob = _oob_flags(e, f, start, e_max=self.ENERGY_THRESHOLD, f_max=self.MAX_FORCE_THRESHOLD)
        out = []
        for b, atoms in enumerate(atoms_list):
            a0, a1 = int(start[b]), int(start[b + 1])
            relaxed = atoms.copy()
            relaxed.set_positions(new_pos[a0:a1])
            r = {"energy": float(e[b]), "per_atom_energies": ea[a0:a1].copy(), "forces": f[a0:a1].copy(), **_chain_counts(counts, b)}
            if stress is not None:
                r["stress"] = stress[b].copy()
            out.append((relaxed, _traj_of_chain(traj, b, a0, a1, atoms), self.ENERGY_THRESHOLD if oob[b] else r["energy"], bool(oob[b]), r))
        return out

    @staticmethod
    def packed_supported(relax: bool, optimizer) -> bool:
        """``evaluate_packed`` relaxes with the device optimizers only: "LAMMPS" / "CG" (the default), "FIRE", "BFGS"."""
        return not relax or optimizer is None or (isinstance(optimizer, str)
                                                  and optimizer.upper() in ("CG", "LAMMPS", "FIRE", "BFGS"))

    def evaluate_packed(self, n_atoms, Z, pos, cell, pbc, relax: bool = False, fixed_mask=None, relax_steps: int | None = None,
                        fmax: float = 0.01, optimizer=None, *, etol: float = 1e-5, ftol: float = 1e-5, cg_driver=None,
                        linesearch_driver=None, max_eval=None, save_traj: bool = False, record_interval: int = 5, **kwargs) -> dict:
        """``calculate_batch`` (``relax=False``) / ``relax_batch`` (``relax=True``) with the ABI's packed arrays on both sides
        (``n_atoms [B]``, atomic numbers ``Z [sum N]``, ``pos [sum N, 3]``, ``cell [B, 9]``, ``pbc [B, 3]``, ``fixed_mask
        [sum N]``): what ``mc.ChainEnsemble`` calls every MC step -- no per-slab objects (4 096 GaN chains: the per-slab
        bookkeeping was 41 % of an MC step, ``profiles/r04/bench_gan.jsonl``).  Returns fp64 ``energy [B]`` (the static energies of
        the final geometries), ``forces``, ``energy_atoms``, ``positions``, ``cfg_start``, ``oob [B]`` (the +-1000 guard of
        ``mcmc/dynamics.py:159-168``), ``energy_std`` / ``saturated`` (zeros: one deterministic fp64 potential), and for
        relaxations ``iterations`` / ``evaluations`` / ``stop`` (CG, with ``lockstep_evaluations`` / ``dispatched_chain_evaluations``) or
        ``n_steps`` / ``converged`` (FIRE, BFGS).  ``etol`` / ``ftol`` / ``cg_driver`` as in ``relax_batch``; "BFGSLineSearch" is refused and
        nothing is recorded: ``linesearch_driver``, ``max_eval``, ``save_traj``, ``record_interval`` and other keywords are ignored."""
        if optimizer is None:
            optimizer = self.parameters.get("optimizer", "LAMMPS")
        if relax and not self.packed_supported(True, optimizer):
            raise backend.BackendError(f"evaluate_packed relaxes on the device only (CG / LAMMPS, FIRE, BFGS), not with {optimizer!r}")
        driver = self._cg_driver_of({"cg_driver": cg_driver})
        n_atoms = np.ascontiguousarray(n_atoms, dtype=np.int32)
        B = len(n_atoms)
        types = self._types_of(Z)
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        cell = np.asarray(cell, dtype=np.float64).reshape(B, 9)
        fixed_pbc = self._fixed_pbc()
        pbc = np.tile(fixed_pbc, (B, 1)) if fixed_pbc is not None else np.asarray(pbc).astype(np.uint8).reshape(B, 3)
        extra = {}
        if not relax:
            (e, ea, f), new_pos = self._get_engine().evaluate_arrays_f64(n_atoms, types, pos, cell, pbc), pos
        else:
            e, ea, f, new_pos, extra, _ = self._relax_packed(
                n_atoms, types, pos, cell, pbc, fixed_mask, optimizer, int(self.relax_steps if relax_steps is None else relax_steps), fmax,
                etol=etol, ftol=ftol, cg_driver=driver, linesearch_driver="ase", max_eval=None, record_interval=0)
            if "stop" in extra:   # CG: how much of the lock-step work the chains needed (tools/bench_gan.py)
                ls, ce = getattr(self._get_engine(), "last_relax_counts", (0, 0))
                extra = {**extra, "lockstep_evaluations": ls, "dispatched_chain_evaluations": ce}
        start = _cfg_start(n_atoms)
        oob = _oob_flags(e, f, start, e_max=self.ENERGY_THRESHOLD, f_max=self.MAX_FORCE_THRESHOLD)
        return {"energy": e, "energy_std": np.zeros(B), "forces": f, "energy_atoms": ea, "positions": new_pos, "cfg_start": start,
                "saturated": np.zeros(B, bool), "oob": oob, **extra}


class TersoffSurfCalc(_AnalyticSurfCalc):
    """Tersoff energy / per-atom energies / forces on MI355X (drop-in for ``LAMMPSSurfCalc`` with
    ``pair_style tersoff``, reference ``calculators.py:492-752``): ``energy`` is the static energy,
    ``per_atom_energies`` is LAMMPS' ``pe/atom``; periodic in all directions like the reference's
    ``boundary p p p`` template."""

    name = "tersoff_mi355x"

    def __init__(self, potential, species, device="cuda", all_periodic=True, logger=None, **kwargs):
        """potential: path or text of a LAMMPS tersoff file, or a params array [nt,nt,nt,14];
        species: symbols in LAMMPS type order (e.g. ["Ga", "N"])."""
        if isinstance(potential, np.ndarray):
            self.params = np.ascontiguousarray(potential, dtype=np.float64)
        else:
            text = potential
            if "\n" not in str(potential):
                with open(potential) as fh:
                    text = fh.read()
            self.params = tersoff_io.parse_tersoff(text, list(species))
        self.species = list(species)
        self._init_common(device, all_periodic, logger)
        super().__init__(**kwargs)

    def _make_engine(self):
        return backend.TersoffEngine(self.params, device=_device_index(self.device))


class SWSurfCalc(_AnalyticSurfCalc):
    """Stillinger-Weber energy / per-atom energies / forces on MI355X (LAMMPS ``pair_style sw``, or ``pair_style kim`` with a
    built-in SW model such as ``SW_StillingerWeber_1985_Si__MO_405512056662_005`` of the reference's Si(111) 5x5 run directory).
    ``per_atom_energies`` follow LAMMPS ``pe/atom`` for ``pair_style sw`` (pair terms half / half, three-body terms in thirds).
    Relaxations (``run_lammps_opt``, ``relax_batch``, ``evaluate_packed(relax=True)``) use the lock-step CG / FIRE / BFGS drivers;
    ``set(cg_driver="resident")`` selects the chain-resident CG minimiser instead (same results bit for bit).
    ``all_periodic=False`` keeps the atoms' own ``pbc`` (the Si templates say ``boundary p p f``)."""

    name = "sw_mi355x"

    def __init__(self, potential, species=None, device="cuda", all_periodic=False, logger=None, **kwargs):
        """potential: path or text of a ``.sw`` file, a params array [nt,nt,nt,11], or a built-in model name (``sw.MODELS``);
        species: symbols in LAMMPS type order (e.g. ["Si"]; a built-in model's own species when omitted)."""
        if isinstance(potential, np.ndarray):
            if species is None:
                raise ValueError("species (LAMMPS type order) are required with a params array")
            self.params = np.ascontiguousarray(potential, dtype=np.float64)
            sw_io.check_params(self.params, list(species))
        elif sw_io.is_builtin(potential):
            species = sw_io.builtin_species(potential) if species is None else species
            self.params = sw_io.parse_sw(sw_io.builtin_text(potential), list(species))
        else:
            if species is None:
                raise ValueError("species (LAMMPS type order) are required with a .sw file")
            text = potential
            if "\n" not in str(potential):
                with open(potential) as fh:
                    text = fh.read()
            self.params = sw_io.parse_sw(text, list(species))
        self.species = list(species)
        self._init_common(device, all_periodic, logger)
        super().__init__(**kwargs)

    def _make_engine(self):
        return backend.SWEngine(self.params, device=_device_index(self.device))


class VashishtaSurfCalc(_AnalyticSurfCalc):
    """Vashishta energy / per-atom energies / forces on MI355X (LAMMPS ``pair_style vashishta``: SiC, SiO2, InP, GaAs, Al2O3).
    ``per_atom_energies`` follow LAMMPS ``pe/atom`` (pair terms half / half, three-body terms in thirds).  Relaxations
    (``run_lammps_opt``, ``relax_batch``, ``evaluate_packed(relax=True)``) use the lock-step CG / FIRE / BFGS drivers; the
    chain-resident CG minimiser does not serve this potential: ``set(cg_driver="resident")`` runs in lock step (same results).
    ``all_periodic=False`` keeps the atoms' own ``pbc``."""

    name = "vashishta_mi355x"

    def __init__(self, potential, species=None, device="cuda", all_periodic=False, logger=None, **kwargs):
        """potential: path or text of a ``.vashishta`` file, a params array [nt,nt,nt,14], or a built-in model name
        (``vashishta.MODELS``, e.g. ``SiC_Vashishta_2007``); species: symbols in LAMMPS type order (a built-in model's own species
        when omitted)."""
        if isinstance(potential, np.ndarray):
            if species is None:
                raise ValueError("species (LAMMPS type order) are required with a params array")
            self.params = np.ascontiguousarray(potential, dtype=np.float64)
            vashishta_io.check_params(self.params, list(species))
        elif vashishta_io.is_builtin(potential):
            species = vashishta_io.builtin_species(potential) if species is None else species
            self.params = vashishta_io.parse_vashishta(vashishta_io.builtin_text(potential), list(species))
        else:
            if species is None:
                raise ValueError("species (LAMMPS type order) are required with a .vashishta file")
            text = potential
            if "\n" not in str(potential):
                with open(potential) as fh:
                    text = fh.read()
            self.params = vashishta_io.parse_vashishta(text, list(species))
        self.species = list(species)
        self._init_common(device, all_periodic, logger)
        super().__init__(**kwargs)

    def _make_engine(self):
        return backend.VashishtaEngine(self.params, device=_device_index(self.device))


class PairSurfCalc(_AnalyticSurfCalc):
    """Pair potentials with damped-shifted-force Coulomb on MI355X: LAMMPS ``pair_style lj/cut``, ``morse``, ``buck``, ``born``,
    ``coul/dsf`` and ``hybrid`` / ``hybrid/overlay`` of them, given as the LAMMPS commands a template would carry (``pair_style``,
    ``pair_coeff``, ``pair_modify shift | mix``, ``set type N charge q``; ``pair.parse``).  ``per_atom_energies`` follow LAMMPS
    ``pe/atom`` (pair energies half / half, the coul/dsf self term on its atom).  Relaxations use the lock-step CG / FIRE / BFGS
    drivers; ``set(cg_driver="resident")`` selects the chain-resident CG minimiser instead (same results bit for bit).
    ``all_periodic=False`` keeps the atoms' own ``pbc``.

    ``coul/long``, ``buck/coul/long``, ``born/coul/long`` and ``lj/cut/coul/long`` with ``kspace_style ewald A`` run an Ewald sum on
    the device (periodic in three directions, charged cells with the neutralising background): g = sqrt(-ln A) / rc and
    k_cut = 2 g sqrt(-ln A) unless ``kspace_modify gewald`` / the ``g_ewald=`` and ``k_cut=`` keywords say otherwise.  Energies agree
    with LAMMPS to the accuracy asked for, not digit for digit (LAMMPS picks its k vectors from the atom count and the charges);
    ``cg_driver="resident"`` runs in lock step for such a model.

    Slabs: ``boundary p p f`` + ``kspace_modify slab F`` among the commands, or the ``slab=F`` keyword, run the Ewald sum of the cell
    extended to F times its height with the dipole correction (Yeh & Berkowitz; charged cells as Ballenegger et al.).  Such a model
    imposes pbc (1, 1, 0) on every structure, whatever the atoms' flags say; the cell needs a and b in the xy plane and c along z."""

    name = "pair_mi355x"

    def __init__(self, commands=None, text=None, species=None, device="cuda", all_periodic=False, logger=None, g_ewald=None, k_cut=None,
                 slab=None, **kwargs):
        """commands: list of LAMMPS command lines, or ``text``: the same as one string; species: symbols in LAMMPS type order;
        g_ewald / k_cut (1 / A): override what ``kspace_style ewald`` / ``kspace_modify gewald`` give; slab: the factor of
        ``kspace_modify slab`` (overrides the parsed one; 0.0 switches the correction off)."""
        if (commands is None) == (text is None):
            raise ValueError("give the pair commands either as commands=[...] or as text=...")
        if not species:
            raise ValueError("species (LAMMPS type order) are required")
        self.species = list(species)
        self.pair_model = pair_io.parse(text if commands is None else list(commands), len(self.species))
        if g_ewald is not None or k_cut is not None or slab is not None:
            ks = self.pair_model.kspace
            if ks is None:
                raise ValueError("g_ewald / k_cut / slab need a */coul/long pair_style with kspace_style ewald")
            rc = next(t.rc for t in self.pair_model.terms if t.style == pair_io.STYLES["coul/long"])
            self.pair_model = self.pair_model._replace(kspace=pair_io.ewald_defaults(
                ks.accuracy, rc, g_ewald=ks.g_ewald if g_ewald is None else g_ewald, k_cut=k_cut,
                slab=ks.slab if slab is None else slab))
        self._init_common(device, all_periodic, logger)
        super().__init__(**kwargs)

    def _make_engine(self):
        return backend.PairEngine(self.pair_model, device=_device_index(self.device))

    def _fixed_pbc(self):
        ks = self.pair_model.kspace
        if ks is not None and ks.slab > 0:
            return np.array([1, 1, 0], np.uint8)
        return super()._fixed_pbc()


EAM_STYLES = ("eam", "eam/alloy", "eam/fs", "adp")


def _parse_pair_coeff(lines):
    """``pair_coeff`` lines -> list of (i, j, file, element names) with LAMMPS type fields as given (``*`` or integers)."""
    out = []
    for ln in ([lines] if isinstance(lines, str) else list(lines or [])):
        tok = str(ln).split()
        if len(tok) < 3:
            raise ValueError(f"pair_coeff {ln!r}: expected 'i j file [elements]'")
        out.append((tok[0], tok[1], tok[2], tok[3:]))
    return out


def eam_tables(style, pair_coeff, resolve, specorder=None):
    """The potential of ``pair_style eam | eam/alloy | eam/fs | adp`` with LAMMPS ``pair_coeff`` lines: ``(species, source)`` where
    ``species`` are the symbols of the types (``specorder`` when given, else the elements the lines name) and ``source`` is a
    ``eam.Funcfl`` (pair_style eam with one funcfl element: the one-element path) or ``eam.EamTables``.  ``resolve(name)``
    returns a file's text.  Refused with ValueError: other styles, NULL types, unknown elements, malformed files, a type without a
    file, two types of one symbol (atoms map to types by symbol)."""
    from . import eam as eam_io

    style = str(style).split()[0]
    if style not in EAM_STYLES:
        raise ValueError(f"pair_style {style!r}: this calculator evaluates pair_style {', '.join(EAM_STYLES)}")
    coeffs = _parse_pair_coeff(pair_coeff)
    if not coeffs:
        raise ValueError(f"pair_style {style}: pair_coeff is required")
    if style in ("eam/alloy", "eam/fs", "adp"):
        if len(coeffs) != 1 or coeffs[0][:2] != ("*", "*"):
            raise ValueError(f"pair_style {style}: expected one 'pair_coeff * * file el_1 ... el_n'")
        if style == "adp":
            setfl = eam_io.parse_adp(resolve(coeffs[0][2]))
            tables = eam_io.tables_from_adp(setfl, coeffs[0][3] or setfl.elements)
        else:
            setfl = eam_io.parse_setfl(resolve(coeffs[0][2]), fs=style == "eam/fs")
            tables = eam_io.tables_from_setfl(setfl, coeffs[0][3] or setfl.elements)
        source, names = tables, list(tables.elements)
    else:
        per_type = {}
        for i, j, name, rest in coeffs:
            if "NULL" in [x.upper() for x in rest]:
                raise ValueError("pair_style eam: NULL types (pair_style hybrid) are not supported")
            if i != j:
                raise ValueError(f"pair_style eam: pair_coeff {i} {j}: LAMMPS accepts only i i (one funcfl file per type)")
            f = eam_io.parse_funcfl(resolve(name))
            if i == "*":
                per_type = {"*": f}
            else:
                try:
                    t = int(i)
                except ValueError:
                    raise ValueError(f"pair_style eam: bad type {i!r}") from None
                if t < 1 or t > 8:
                    raise ValueError(f"pair_style eam: type {t} outside 1 .. 8")
                per_type.pop("*", None)
                per_type[t] = f
        if "*" in per_type:
            source = per_type["*"]
            n = len(specorder) if specorder else 1
            files = [source] * n
        else:
            n = max(per_type)
            missing = [t for t in range(1, n + 1) if t not in per_type]
            if missing:
                raise ValueError(f"pair_style eam: types {missing} have no pair_coeff file")
            files = [per_type[t] for t in range(1, n + 1)]
        names = [structures.SYMBOLS[f.atomic_number] for f in files]
        source = files[0] if len(files) == 1 else eam_io.tables_from_funcfl(files)
    species = list(specorder) if specorder else names
    if len(species) != len(names):
        raise ValueError(f"specorder {list(specorder)} has {len(species)} symbols, pair_coeff names {len(names)} types")
    unknown = [x for x in species if x not in structures.ATOMIC_NUMBERS]
    if unknown:
        raise ValueError(f"unknown elements {unknown}")
    dup = sorted({x for x in species if species.count(x) > 1})
    if dup:
        raise ValueError(f"several types are {dup}: atoms map to types by symbol")
    return species, source


class EAMSurfCalc(_AnalyticSurfCalc):
    """EAM on MI355X: drop-in for ``LAMMPSRunSurfCalc`` (reference ``calculators.py:755-811``, a modified ASE ``lammpsrun``
    that pipes ``pair_style eam`` / ``pair_coeff * * Cu_u3.eam`` to an ``lmp`` subprocess; used by ``tests/test_Cu.py`` and
    ``tutorials/example.ipynb``).  Constructor keeps the reference's keywords: ``files=[potential files]``, ``keep_tmp_files``
    / ``keep_alive`` / ``tmp_dir`` are accepted and unused (nothing is written to disk).  Without ``pair_coeff`` the first file is
    one funcfl element.  ``set(pair_style=..., pair_coeff=[...], specorder=[...])`` selects the potential as LAMMPS would:

    * ``eam`` with ``* * file`` (one funcfl element) or ``i i file_i`` per type (funcfl files mixed on one grid);
    * ``eam/alloy`` / ``eam/fs`` with ``* * file el_1 ... el_n`` (setfl / Finnis-Sinclair file, up to 8 types);
    * ``adp`` with ``* * file el_1 ... el_n`` (angular-dependent potential: a setfl file with u(r) and w(r) blocks).

    Atoms map to types by symbol: ``specorder`` (ASE's keyword) when given, else the elements ``pair_coeff`` names; an atom of
    another element is refused.  ``pair_coeff`` file names are matched against ``files`` (path or base name), else opened as
    given.  Boundary conditions follow the atoms' ``pbc`` (ASE lammpsrun derives ``boundary`` from it).  ``free_energy`` (= ``energy``)
    and ``energies`` (= ``per_atom_energies``) are the names the reference's class lists (``lammpsrun.py:125``), filled on request."""

    name = "eam_mi355x"
    implemented_properties = (*_AnalyticSurfCalc.implemented_properties, "free_energy", "energies")

    def __init__(self, files=None, potential=None, device="cuda", all_periodic=False, logger=None, keep_tmp_files=False,
                 keep_alive=False, tmp_dir=None, **kwargs):
        from . import eam as eam_io

        src = potential if potential is not None else (list(files)[0] if files else None)
        if src is None:
            raise ValueError("EAMSurfCalc needs files=[<potential file>]")
        self.files = [src] if potential is not None else list(files)
        self.tables = None
        try:   # the reference's default: the first file is one funcfl element
            self.funcfl = src if isinstance(src, eam_io.Funcfl) else (
                eam_io.parse_funcfl(src) if "\n" in str(src) else eam_io.read_funcfl(src))
            self.species = [structures.SYMBOLS[self.funcfl.atomic_number]]
        except ValueError:   # a setfl / fs file: set(pair_style=..., pair_coeff=[...]) says how to read it
            self.funcfl = None
            self.species = []
        self._init_common(device, all_periodic, logger)
        super().__init__(**kwargs)

    def calculate(self, atoms=None, properties=_AnalyticSurfCalc._default_properties, system_changes=all_changes):
        super().calculate(atoms, properties, system_changes)
        for name, source in (("free_energy", "energy"), ("energies", "per_atom_energies")):
            self.results.pop(name, None)
            if name in properties:
                self.results[name] = self.results[source]

    def _file_text(self, name):
        from . import eam as eam_io

        for f in self.files:
            if isinstance(f, eam_io.Funcfl):
                continue
            f = str(f)
            if "\n" not in f and (f == name or os.path.basename(f) == os.path.basename(name)):
                with open(f, encoding="utf-8") as fh:
                    return fh.read()
        if os.path.isfile(name):
            with open(name, encoding="utf-8") as fh:
                return fh.read()
        if len(self.files) == 1 and "\n" in str(self.files[0]):
            return str(self.files[0])
        raise ValueError(f"pair_coeff names {name!r}, which is neither among files={self.files} nor a file")

    def set(self, **kwargs) -> dict:
        style = kwargs.get("pair_style")
        if style is not None and str(style).split()[0] not in EAM_STYLES:
            raise ValueError(f"pair_style {style!r}: this calculator evaluates pair_style {', '.join(EAM_STYLES)}")
        if "files" in kwargs:
            self.files = list(kwargs.pop("files"))
        changed = super().set(**kwargs)
        if self.parameters.get("pair_coeff") and any(k in kwargs for k in ("pair_style", "pair_coeff", "specorder")):
            self._configure_potential()
        return changed

    def _configure_potential(self):
        from . import eam as eam_io

        p = self.parameters
        self.species, source = eam_tables(p.get("pair_style", "eam"), p["pair_coeff"], self._file_text, p.get("specorder"))
        self.funcfl, self.tables = (source, None) if isinstance(source, eam_io.Funcfl) else (None, source)
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    def _make_engine(self):
        if self.funcfl is None and self.tables is None:
            raise ValueError(f"{self.files[0]} is no funcfl file: set(pair_style=..., pair_coeff=[...]) first")
        return backend.EAMEngine(self.funcfl if self.tables is None else self.tables, device=_device_index(self.device))


LAMMPSRunSurfCalc = EAMSurfCalc   # the reference's class name for this role


class LAMMPSSurfCalc(_AnalyticSurfCalc):
    """Drop-in for the reference's ``LAMMPSSurfCalc`` / ``LAMMMPSCalc`` (``calculators.py:492-752``) the way its GaN tutorial
    uses them: constructed WITHOUT arguments and configured through ``set(run_dir=..., relax_steps=..., optimizer="LAMMPS",
    ...)`` (``tutorials/GaN_0001.ipynb``: ``lammps_surf_calc = LAMMPSSurfCalc(); lammps_surf_calc.set(**calc_settings)``).
    Instead of writing ``lammps.in`` / ``lammps.data`` and calling LAMMPS, the run directory's own files say what to evaluate:

    * ``lammps_config.json``: ``potential_file``, ``atoms`` (species in LAMMPS type order), ``bulk_index`` (atoms with id <=
      bulk_index form the group the relaxation template holds with ``fix ... setforce 0``);
    * ``lammps_energy_template.txt`` / ``lammps_opt_template.txt``: the ``pair_style`` line selects the potential -- ``tersoff``
      (multi-element file), ``eam`` (one funcfl element, or a list ``potential_file`` of one funcfl file per species),
      ``eam/alloy`` / ``eam/fs`` (setfl / Finnis-Sinclair file, elements = ``atoms``), ``sw`` (Stillinger-Weber file), ``vashishta`` (Vashishta file; the energy template's ``boundary`` applies as for ``sw``) or ``kim <model>`` with a built-in SW
      model (``sw.MODELS``: the Si(111) 5x5 tutorial's ``SW_StillingerWeber_1985_Si__MO_405512056662_005``; no
      ``potential_file`` needed, the species come from ``atoms``) are evaluated on the device, anything else raises.  For the SW
      styles the energy template's ``boundary`` applies (``p`` periodic; ``f``, ``s``, ``m`` open) and pe/atom follows LAMMPS
      ``pair_style sw`` (a KIM model's own per-particle split is not reproduced; totals do not depend on it).  ``lj/cut``,
      ``morse``, ``buck``, ``born``, ``coul/dsf`` and ``hybrid`` / ``hybrid/overlay`` of them take their ``pair_coeff`` /
      ``pair_modify`` / ``set type N charge q`` lines and the ``boundary`` from the energy template (``pair.parse``; no
      ``potential_file``); the ``*/coul/long`` styles with ``kspace_style ewald`` need ``boundary p p p``, or ``boundary p p f`` with
      ``kspace_modify slab F`` (the dipole-corrected slab sum, pbc (1, 1, 0)).  When the opt
      template names another potential the backend lacks (the Si tutorial's SRS model), relaxations raise; single points work.

    The potential file is looked up like LAMMPS does (as given, in the run directory, in the working directory, in
    ``$LAMMPS_POTENTIALS``) and additionally in ``potential_dirs`` and in the reference's ``mcmc/potentials`` when that package
    is importable.  ``boundary p p p`` of the templates = periodic in all directions."""

    name = "lammps_surf_mi355x"

    def __init__(self, device="cuda", potential_dirs=(), logger=None, **kwargs):
        self.potential_dirs = [str(d) for d in potential_dirs]
        self.species = []
        self.bulk_index = 0
        self.pair_style = None
        self.boundary = None          # SW styles: the energy template's boundary as pbc flags
        self.relax_refused = None     # SW styles: the opt template's potential when the backend lacks it
        self.kim_model = None
        self.tables = None            # EAM with several elements (eam/alloy, eam/fs, funcfl files per species)
        self.pair_model = None        # the pair styles: what pair.parse read from the energy template
        self._cfg_key = None
        self._init_common(device, True, logger)
        self.run_dir = os.getcwd()        # the reference's default (calculators.py:502)
        super().__init__(**kwargs)

    # -- configuration from the run directory ----------------------------------------------------------------------------------
    def _find_potential(self, name, run_dir):
        cands = [name] if os.path.isabs(name) else [os.path.join(d, name) for d in
                                                    [str(run_dir), os.getcwd(),
                                                     *[x for x in os.environ.get("LAMMPS_POTENTIALS", "").split(os.pathsep) if x],
                                                     *self.potential_dirs]]
        if not os.path.isabs(name):
            try:
                import importlib.util

                spec = importlib.util.find_spec("mcmc")
                for loc in (spec.submodule_search_locations or []) if spec else []:
                    cands.append(os.path.join(loc, "potentials", name))
            except (ImportError, ValueError):
                pass
        for c in cands:
            if os.path.isfile(c):
                return c
        raise FileNotFoundError(f"potential file {name!r} not found; looked in: " + ", ".join(cands))

    @staticmethod
    def _template_lines(run_dir):
        """{template name: (pair_style arguments or None, boundary tokens or None)} of the run directory's templates."""
        out = {}
        for tmpl in ("lammps_energy_template.txt", "lammps_opt_template.txt"):
            tp = os.path.join(run_dir, tmpl)
            if os.path.isfile(tp):
                with open(tp, encoding="utf-8") as fh:
                    text = fh.read()
                m = re.search(r"^\s*pair_style\s+([^#\n]+)", text, re.M)
                b = re.search(r"^\s*boundary\s+([^#\n]+)", text, re.M)
                out[tmpl] = (m.group(1).split() if m else None, b.group(1).split() if b else None)
        return out

    @staticmethod
    def _boundary_pbc(tokens):
        """LAMMPS ``boundary`` (one token per axis): ``p`` periodic; ``f``, ``s``, ``m`` (or lower / upper pairs of them) not."""
        if tokens is None:
            return np.ones(3, np.uint8)          # the LAMMPS default: p p p
        if len(tokens) != 3 or not all(t == "p" or (t and set(t) <= set("fsm") and len(t) <= 2) for t in tokens):
            raise ValueError(f"boundary {' '.join(tokens)!r}: expected three of p, f, s, m")
        return np.array([t == "p" for t in tokens], np.uint8)

    def _sw_source(self, args, cfg):
        """(params source, key) of an SW pair style (``sw`` + potential_file, ``kim <built-in model>``) or of ``vashishta`` +
        potential_file, which is configured the same way; None for other styles."""
        kp = self.parameters.get("kim_potential")
        if (args and args[0] == "kim") or kp:
            model = args[1] if args and args[0] == "kim" and len(args) > 1 else (kp if isinstance(kp, str) else None)
            if model is None or not sw_io.is_builtin(model):
                raise backend.BackendError(f"KIM model {model!r} is not provided by this backend (built in: "
                                           + ", ".join(sorted(sw_io.MODELS)) + "; pair styles tersoff, eam and sw are)")
            return ("kim", model)
        if args and args[0] == "sw":
            if "potential_file" not in cfg:
                raise KeyError("lammps_config.json: pair_style sw needs potential_file")
            return ("sw", self._find_potential(cfg["potential_file"], str(self.run_dir)))
        if args and args[0] == "vashishta":
            if "potential_file" not in cfg:
                raise KeyError("lammps_config.json: pair_style vashishta needs potential_file")
            return ("vashishta", self._find_potential(cfg["potential_file"], str(self.run_dir)))
        return None

    def _configure(self):
        run_dir = str(self.run_dir)
        cfg_path = os.path.join(run_dir, "lammps_config.json")
        if not os.path.isfile(cfg_path):
            raise FileNotFoundError(f"{cfg_path}: the run directory needs the reference's lammps_config.json "
                                    "(potential_file, atoms, bulk_index)")
        with open(cfg_path, encoding="utf-8") as fh:
            cfg = json.load(fh)
        tmpls = self._template_lines(run_dir)
        args = next((a for a, _ in tmpls.values() if a), None)
        if args is None:
            raise FileNotFoundError(f"{run_dir}: no lammps_energy_template.txt / lammps_opt_template.txt with a pair_style line")
        src = self._sw_source(args, cfg)
        if src is not None:
            self._configure_sw(cfg_path, cfg, tmpls, args, src)
            return
        style = args[0]
        if style in pair_io.PAIR_STYLES:
            self._configure_pair(run_dir, cfg_path, cfg)
            return
        pf = cfg["potential_file"]
        pots = [self._find_potential(x, run_dir) for x in (pf if isinstance(pf, (list, tuple)) else [pf])]
        pot = pots[0]
        key = (cfg_path, os.path.getmtime(cfg_path), tuple(pots), style)
        if key == self._cfg_key:
            return
        self.species = list(cfg["atoms"])
        self.bulk_index = int(cfg.get("bulk_index", 0))
        self.pair_style = style
        self.boundary = None
        self.relax_refused = None
        self.tables = None
        if len(pots) > 1 and style != "eam":
            raise ValueError(f"pair_style {style}: lammps_config.json lists {len(pots)} potential files, the style reads one")
        with open(pot, encoding="utf-8") as fh:
            text = fh.read()
        if style == "tersoff":
            self.params = tersoff_io.parse_tersoff(text, self.species)
            self.funcfl = None
        elif style == "eam" and len(pots) == 1:
            from . import eam as eam_io

            self.funcfl = eam_io.parse_funcfl(text)
            self.params = None
            if self.species != [structures.SYMBOLS[self.funcfl.atomic_number]]:
                raise ValueError(f"pair_style eam (funcfl) holds one element, lammps_config.json lists {self.species}")
        elif style == "eam":   # one funcfl file per species (pair_coeff t t file_t), mixed on one grid
            from . import eam as eam_io

            if len(pots) != len(self.species):
                raise ValueError(f"pair_style eam: {len(pots)} funcfl files for the species {self.species}")
            files = []
            for name, sym in zip(pots, self.species):
                with open(name, encoding="utf-8") as fh:
                    f = eam_io.parse_funcfl(fh.read())
                if structures.SYMBOLS[f.atomic_number] != sym:
                    raise ValueError(f"pair_style eam: {name} holds {structures.SYMBOLS[f.atomic_number]}, not {sym}")
                files.append(f)
            self.tables = eam_io.tables_from_funcfl(files)
            self.funcfl = self.params = None
        elif style in ("eam/alloy", "eam/fs"):
            from . import eam as eam_io

            self.tables = eam_io.tables_from_setfl(eam_io.parse_setfl(text, fs=style == "eam/fs"), self.species)
            self.funcfl = self.params = None
        elif style == "adp":
            from . import eam as eam_io

            self.tables = eam_io.tables_from_adp(eam_io.parse_adp(text), self.species)
            self.funcfl = self.params = None
        else:
            raise backend.BackendError(f"pair_style {style!r} is not provided by this backend "
                                       "(tersoff, eam, eam/alloy, eam/fs, adp, sw, vashishta, lj/cut, morse, buck, born, coul/dsf and "
                                       "hybrid / hybrid/overlay of the last five are)")
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        self._cfg_key = key

    def _configure_pair(self, run_dir, cfg_path, cfg):
        """``pair_style lj/cut | morse | buck | born | coul/dsf | hybrid | hybrid/overlay``: the pair commands (``pair.parse``) and the
        ``boundary`` come from the energy template (the opt template when there is no other), the species from ``atoms``; no
        ``potential_file``.  Commands that cannot be read raise ``BackendError``."""
        name = next(t for t in ("lammps_energy_template.txt", "lammps_opt_template.txt") if os.path.isfile(os.path.join(run_dir, t)))
        path = os.path.join(run_dir, name)
        with open(path, encoding="utf-8") as fh:
            text = fh.read()
        key = (cfg_path, os.path.getmtime(cfg_path), path, os.path.getmtime(path), "pair")
        if key == self._cfg_key:
            return
        species = list(cfg["atoms"])
        try:
            model = pair_io.parse(text, len(species))
            b = re.search(r"^\s*boundary\s+([^#\n]+)", text, re.M)
            boundary = self._boundary_pbc(b.group(1).split() if b else None)
            if model.kspace is not None and model.kspace.slab > 0:
                # (pair.parse took the factor only after a 'boundary p p f' line; the first boundary line is the one that applies here)
                if boundary is None or list(boundary) != [1, 1, 0]:
                    raise ValueError(f"boundary {b.group(1).strip() if b else None!r}: kspace_modify slab needs 'boundary p p f'")
            elif model.kspace is not None and boundary is not None and not all(boundary):
                raise ValueError(f"boundary {b.group(1).strip()!r}: kspace_style ewald needs 'boundary p p p' (the Ewald sum is periodic in "
                                 "three directions) or kspace_modify slab F under 'boundary p p f'")
        except ValueError as e:
            raise backend.BackendError(f"{path}: the pair commands cannot be read: {e}") from None
        self.pair_model = model
        self.params = self.funcfl = self.tables = None
        self.species = species
        self.bulk_index = int(cfg.get("bulk_index", 0))
        self.pair_style = "pair"
        self.kim_model = None
        self.boundary = boundary
        self.relax_refused = None
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        self._cfg_key = key

    def _configure_sw(self, cfg_path, cfg, tmpls, args, src):
        """``pair_style sw`` / ``pair_style vashishta`` (``potential_file`` + ``atoms``) or ``pair_style kim <built-in SW model>`` (species from ``atoms``: the
        reference's KIM templates write ``pair_coeff * * {}`` with the element names).  The energy template's ``boundary`` applies.
        An opt template that names another potential the backend lacks makes relaxations refuse (single points still work)."""
        energy_args, energy_bnd = tmpls.get("lammps_energy_template.txt", (None, None))
        if energy_args is None:
            energy_args, energy_bnd = args, tmpls.get("lammps_opt_template.txt", (None, None))[1]
        opt_args = tmpls.get("lammps_opt_template.txt", (None, None))[0]
        key = (cfg_path, os.path.getmtime(cfg_path), src, tuple(energy_args), tuple(opt_args or ()), tuple(energy_bnd or ()))
        if key == self._cfg_key:
            return
        species = list(cfg["atoms"])
        if src[0] == "kim":
            text = sw_io.builtin_text(src[1])
            if not set(species) <= set(sw_io.builtin_species(src[1])):
                raise ValueError(f"KIM model {src[1]} covers {sw_io.builtin_species(src[1])}, lammps_config.json lists {species}")
        else:
            with open(src[1], encoding="utf-8") as fh:
                text = fh.read()
        refused = None
        if opt_args is not None and opt_args != energy_args:
            name = opt_args[1] if opt_args[0] == "kim" and len(opt_args) > 1 else " ".join(opt_args)
            if not (opt_args[0] == "kim" and len(opt_args) > 1 and sw_io.is_builtin(opt_args[1])):
                refused = name
        self.params = vashishta_io.parse_vashishta(text, species) if src[0] == "vashishta" else sw_io.parse_sw(text, species)
        self.funcfl = self.tables = None
        self.species = species
        self.bulk_index = int(cfg.get("bulk_index", 0))
        self.pair_style = src[0]
        self.kim_model = src[1] if src[0] == "kim" else None
        self.boundary = self._boundary_pbc(energy_bnd)
        self.relax_refused = refused
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        self._cfg_key = key

    def _fixed_pbc(self):
        if self.pair_style in ("sw", "kim", "pair", "vashishta") and self.boundary is not None:
            return self.boundary
        return super()._fixed_pbc()

    def _check_relax(self):
        self._configure()
        if self.relax_refused is not None:
            raise backend.BackendError(f"the run directory's lammps_opt_template.txt relaxes with {self.relax_refused}, which this "
                                       f"backend does not provide (single-point energies use the energy template's potential; "
                                       f"an SW relaxation is available through SWSurfCalc)")

    def _make_engine(self):
        if self.pair_style in ("sw", "kim"):
            return backend.SWEngine(self.params, device=_device_index(self.device))
        if self.pair_style == "vashishta":
            return backend.VashishtaEngine(self.params, device=_device_index(self.device))
        if self.pair_style == "pair":
            return backend.PairEngine(self.pair_model, device=_device_index(self.device))
        if self.pair_style == "tersoff":
            return backend.TersoffEngine(self.params, device=_device_index(self.device))
        return backend.EAMEngine(self.funcfl if self.tables is None else self.tables, device=_device_index(self.device))

    def _get_engine(self):
        self._configure()
        return super()._get_engine()

    def _pack(self, atoms):
        self._configure()
        return super()._pack(atoms)

    def run_lammps_opt(self, slab, run_dir=None, fixed_indices=None, optimizer="CG", **kwargs):
        """As the base class; without ``fixed_indices`` the template's ``group bulk id <= bulk_index`` + ``setforce 0`` applies:
        the first ``bulk_index`` atoms are held."""
        if run_dir is not None and str(run_dir) != str(self.run_dir):
            self.run_dir = run_dir
        self._check_relax()
        if fixed_indices is None and self.bulk_index > 0:
            fixed_indices = np.arange(min(self.bulk_index, len(slab)))
        return super().run_lammps_opt(slab, run_dir=run_dir, fixed_indices=fixed_indices, optimizer=optimizer, **kwargs)

    def run_lammps_energy(self, slab, run_dir=None, **kwargs):
        if run_dir is not None and str(run_dir) != str(self.run_dir):
            self.run_dir = run_dir
        return super().run_lammps_energy(slab, run_dir=run_dir, **kwargs)

    def relax_batch(self, atoms_list, fixed_indices=None, **kwargs):
        self._check_relax()
        if fixed_indices is None and self.bulk_index > 0:
            fixed_indices = [np.arange(min(self.bulk_index, len(a))) for a in atoms_list]
        return super().relax_batch(atoms_list, fixed_indices=fixed_indices, **kwargs)

    def evaluate_packed(self, n_atoms, Z, pos, cell, pbc, relax: bool = False, fixed_mask=None, **kwargs) -> dict:
        """As the base class; relaxations without a mask hold the template's bulk group (the first ``bulk_index`` atoms of every slab)."""
        self._configure()
        if relax:
            self._check_relax()
        if relax and fixed_mask is None and self.bulk_index > 0:
            start = _cfg_start(n_atoms)   # (vectorised: every MC step of a run-directory ensemble without fixed_indices comes here)
            fixed_mask = ((np.arange(int(start[-1])) - np.repeat(start[:-1], n_atoms)) < self.bulk_index).astype(np.uint8)
        return super().evaluate_packed(n_atoms, Z, pos, cell, pbc, relax=relax, fixed_mask=fixed_mask, **kwargs)


LAMMMPSCalc = LAMMPSSurfCalc      # (the reference's base class name, spelled as there)
