"""ctypes binding of ``libvssr_eval.so`` (the C ABI in ``include/vssr_eval.h``).

There is no CPU fallback: if the HIP library is missing or no GPU is visible, every entry
point raises.  The oracle under ``oracle/`` is test infrastructure and is never imported here.
"""

from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VSSR_EVAL_LIB selects another build of the same library (A/B measurements, tools/gpu_ab.sh); there is still no fallback
LIB_PATH = os.environ.get("VSSR_EVAL_LIB") or os.path.join(_HERE, "libvssr_eval.so")

WANT_ENERGY, WANT_FORCES, WANT_STD, WANT_PER_MODEL, WANT_PER_ATOM = 1, 2, 4, 8, 16
WANT_ALL = WANT_ENERGY | WANT_FORCES | WANT_STD | WANT_PER_MODEL | WANT_PER_ATOM

EXPORTS = (
    "vssr_abi_version", "vssr_create", "vssr_destroy", "vssr_last_error", "vssr_eval", "vssr_eval_batch",
    "vssr_batch_upload", "vssr_batch_set_positions", "vssr_batch_run", "vssr_batch_download",
    "vssr_synchronize", "vssr_profile_enable", "vssr_profile_reset", "vssr_profile_read",
    "vssr_batch_stats", "vssr_batch_neighbors", "vssr_debug_read", "vssr_tersoff_create",
    "vssr_tersoff_eval_batch", "vssr_batch_relax_fire", "vssr_batch_relax_bfgs", "vssr_debug_capacity",
    "vssr_batch_device_results", "vssr_eam_create", "vssr_eam_eval_batch",
    "vssr_tersoff_create_from_text", "vssr_batch_relax_cg", "vssr_batch_saturated",
    "vssr_batch_embedding", "vssr_batch_traj_configure", "vssr_batch_traj_read",
    "vssr_device_context", "vssr_batch_stress", "vssr_batch_energy_f64", "vssr_batch_device_results_f64",
    "vssr_batch_relax_counts", "vssr_sw_create", "vssr_sw_create_from_text", "vssr_sw_eval_batch",
    "vssr_gmm_create", "vssr_gmm_score_rows", "vssr_gmm_score_batch", "vssr_eam_create_alloy",
    "vssr_gmm_fit_create", "vssr_gmm_fit_append_rows", "vssr_gmm_fit_append_batch", "vssr_gmm_fit_clear",
    "vssr_gmm_fit_set_init", "vssr_gmm_fit_run", "vssr_gmm_fit_params", "vssr_gmm_fit_scorer",
    "vssr_cluster_create", "vssr_cluster_append_rows", "vssr_cluster_append_batch", "vssr_cluster_clear", "vssr_cluster_pca",
    "vssr_cluster_pca_params", "vssr_cluster_projected", "vssr_cluster_set_points", "vssr_cluster_linkage",
    "vssr_pair_create", "vssr_pair_create_kspace", "vssr_pair_create_kspace_slab", "vssr_pair_eval_batch", "vssr_batch_results_f64", "vssr_batch_relax_cg_driver",
    "vssr_batch_relax_bfgs_linesearch", "vssr_eam_create_adp",
    "vssr_vashishta_create", "vssr_vashishta_create_from_text", "vssr_vashishta_eval_batch",
    "vssr_batch_md", "vssr_batch_md_set_velocities", "vssr_batch_md_draw_velocities", "vssr_batch_md_get_velocities",
    "vssr_batch_md_driver", "vssr_batch_vibrations", "vssr_batch_neb", "vssr_batch_dimer",
    "vssr_batch_relax_cell", "vssr_batch_get_cell", "vssr_batch_md_npt",
)


class BackendError(RuntimeError):
    pass


class PainnConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("n_models", C.c_int32),
        ("weights", C.POINTER(C.POINTER(C.c_float))), ("weights_len", C.c_uint64),
        ("feat_dim", C.c_int32), ("n_rbf", C.c_int32), ("num_conv", C.c_int32), ("n_embed", C.c_int32),
        ("readout_hidden", C.c_int32), ("cutoff", C.c_float), ("excl_vol", C.c_int32),
        ("excl_power", C.c_int32), ("excl_sigma", C.c_float), ("model_units_per_ev", C.c_double),
        ("offset_per_z", C.POINTER(C.c_double)), ("offset_const", C.c_double),
    ]


class FireParams(C.Structure):
    """vssr_fire_params; defaults = ASE FIRE defaults and the reference's relax_steps / fmax."""
    _fields_ = [("max_steps", C.c_int32), ("fmax", C.c_float), ("dt", C.c_float), ("maxstep", C.c_float),
                ("dtmax", C.c_float), ("finc", C.c_float), ("fdec", C.c_float), ("astart", C.c_float),
                ("fa", C.c_float), ("nmin", C.c_int32)]

    @classmethod
    def default(cls, max_steps=20, fmax=0.01):
        return cls(int(max_steps), float(fmax), 0.1, 0.2, 1.0, 1.1, 0.5, 0.1, 0.99, 5)


class EamGrid(C.Structure):
    _fields_ = [("nrho", C.c_int32), ("nr", C.c_int32), ("drho", C.c_double), ("dr", C.c_double), ("cutoff", C.c_double)]


class KSpace(C.Structure):
    """vssr_kspace: Ewald damping and reciprocal cutoff (1 / A)."""
    _fields_ = [("g_ewald", C.c_double), ("k_cut", C.c_double)]


class PairTerm(C.Structure):
    """vssr_pair_term: 0-based types, style code (``pair.STYLES``), coefficients in LAMMPS order, cutoff, shift flag."""
    _fields_ = [("type_a", C.c_int32), ("type_b", C.c_int32), ("style", C.c_int32), ("c", C.c_double * 5), ("rc", C.c_double),
                ("shift", C.c_int32)]


class CgParams(C.Structure):
    """vssr_cg_params; defaults = the reference's LAMMPS template (minimize 1e-5 1e-5 {relax_steps} 10000, dmax 0.1)."""
    _fields_ = [("max_iter", C.c_int32), ("max_eval", C.c_int32), ("etol", C.c_double), ("ftol", C.c_double), ("dmax", C.c_double)]

    @classmethod
    def default(cls, max_iter=100, max_eval=10000, etol=1e-5, ftol=1e-5, dmax=0.1):
        return cls(int(max_iter), int(max_eval), float(etol), float(ftol), float(dmax))


CG_STOP_REASONS = {1: "energy tolerance", 2: "force tolerance", 3: "max iterations", 4: "max force evaluations",
                   5: "search direction is not downhill", 6: "forces are zero", 7: "linesearch: zero quadratic step",
                   8: "linesearch alpha is zero"}


# vssr_batch_relax_cg_driver: which driver vssr_batch_relax_cg takes ("auto": the library's rule)
CG_DRIVERS = {"auto": 0, "lockstep": 1, "resident": 2}
CG_DRIVER_NAMES = {0: None, 1: "lockstep", 2: "resident"}


def cg_driver_code(driver) -> int:
    """The VSSR_CG_DRIVER_* value of ``"auto"`` / ``"lockstep"`` / ``"resident"``; ``ValueError`` for anything else."""
    if not isinstance(driver, str) or driver not in CG_DRIVERS:
        raise ValueError(f"CG driver {driver!r}: one of {', '.join(repr(k) for k in CG_DRIVERS)}")
    return CG_DRIVERS[driver]


class BfgsParams(C.Structure):
    """vssr_bfgs_params; defaults = ASE BFGS defaults and the reference's relax_steps / fmax."""
    _fields_ = [("max_steps", C.c_int32), ("fmax", C.c_float), ("alpha", C.c_float), ("maxstep", C.c_float)]

    @classmethod
    def default(cls, max_steps=20, fmax=0.01):
        return cls(int(max_steps), float(fmax), 70.0, 0.2)


class BfgsLsParams(C.Structure):
    """vssr_bfgsls_params; defaults = ASE BFGSLineSearch defaults (alpha 10, maxstep 0.2, c1 0.23, c2 0.46, stpmax 50), the reference's
    relax_steps / fmax, and an evaluation budget of ``20 * max_steps + 20`` per chain.  Doubles: the numpy restatement
    (tests/bfgsls_oracle.py) sees the same values."""
    _fields_ = [("max_steps", C.c_int32), ("max_eval", C.c_int32), ("fmax", C.c_double), ("alpha", C.c_double), ("maxstep", C.c_double),
                ("c1", C.c_double), ("c2", C.c_double), ("stpmax", C.c_double)]

    @classmethod
    def default(cls, max_steps=20, fmax=0.01, max_eval=None, alpha=10.0, maxstep=0.2, c1=0.23, c2=0.46, stpmax=50.0):
        if max_eval is None:
            max_eval = 20 * int(max_steps) + 20
        return cls(int(max_steps), int(max_eval), float(fmax), float(alpha), float(maxstep), float(c1), float(c2), float(stpmax))


BFGSLS_STOP_REASONS = {1: "converged", 2: "max steps", 3: "line search failed", 4: "max force evaluations",
                       5: "non-finite energy or force"}


class MdParams(C.Structure):
    """vssr_md_params: fs, K, 1 / fs; ``thermostat`` one of ``MD_THERMOSTATS``."""
    _fields_ = [("n_steps", C.c_int32), ("thermostat", C.c_int32), ("thermo_interval", C.c_int32), ("dt", C.c_double),
                ("temperature", C.c_double), ("temperature_end", C.c_double), ("friction", C.c_double), ("ramp_steps", C.c_int64),
                ("step0", C.c_int64), ("seed", C.c_uint64)]


MD_THERMOSTATS = {"nve": 0, "langevin": 1}
MD_STOP_REASONS = {1: "all steps taken", 2: "non-finite energy or force"}
# vssr_batch_md_driver: which driver vssr_batch_md takes ("auto": the library's rule -- chain-resident for small Tersoff batches)
MD_DRIVERS = {"auto": 0, "lockstep": 1, "resident": 2}
MD_DRIVER_NAMES = {0: None, 1: "lockstep", 2: "resident"}
KB_EV = 8.617333262e-5   # eV / K, the constant of csrc/md_dev.h


def md_driver_code(driver) -> int:
    """The VSSR_MD_DRIVER_* value of ``"auto"`` / ``"lockstep"`` / ``"resident"``; ``ValueError`` for anything else."""
    if not isinstance(driver, str) or driver not in MD_DRIVERS:
        raise ValueError(f"MD driver {driver!r}: one of {', '.join(repr(k) for k in MD_DRIVERS)}")
    return MD_DRIVERS[driver]


def md_thermostat_code(thermostat) -> int:
    """The VSSR_MD_* value of ``"nve"`` / ``"langevin"``; ``ValueError`` for anything else."""
    if not isinstance(thermostat, str) or thermostat not in MD_THERMOSTATS:
        raise ValueError(f"thermostat {thermostat!r}: one of {', '.join(repr(k) for k in MD_THERMOSTATS)}")
    return MD_THERMOSTATS[thermostat]


class NptParams(C.Structure):
    """vssr_npt_params: fs, K, 1 / fs, eV / A^3, A^3 / eV; ``thermostat`` / ``barostat`` / ``coupling`` one of ``NPT_THERMOSTATS`` /
    ``NPT_BAROSTATS`` / ``NPT_COUPLINGS``; ``mask`` 0 / 1 per Cartesian axis."""
    _fields_ = [("n_steps", C.c_int32), ("thermostat", C.c_int32), ("barostat", C.c_int32), ("coupling", C.c_int32),
                ("thermo_interval", C.c_int32), ("mask", C.c_int32 * 3), ("dt", C.c_double), ("temperature", C.c_double),
                ("temperature_end", C.c_double), ("friction", C.c_double), ("taut", C.c_double), ("taup", C.c_double),
                ("pressure", C.c_double), ("compressibility", C.c_double), ("ramp_steps", C.c_int64), ("step0", C.c_int64),
                ("seed", C.c_uint64)]


NPT_THERMOSTATS = {"none": 0, "langevin": 1, "berendsen": 2}
NPT_BAROSTATS = {"none": 0, "berendsen": 1, "crescale": 2}
NPT_COUPLINGS = {"isotropic": 0, "per_axis": 1}
NPT_STOP_REASONS = {1: "all steps taken", 2: "non-finite energy, force or stress",
                    3: "cell left the image range it began with or degenerated"}


def _npt_code(table, what, value) -> int:
    if not isinstance(value, str) or value not in table:
        raise ValueError(f"{what} {value!r}: one of {', '.join(repr(k) for k in table)}")
    return table[value]


def npt_params(steps, timestep, thermostat="none", barostat="none", coupling="isotropic", temperature=0.0, temperature_end=None,
               friction=0.0, taut=100.0, taup=1000.0, pressure=0.0, compressibility=1.0, mask=None, ramp_steps=None, step0=0, seed=0,
               thermo_interval=1) -> NptParams:
    """The ``NptParams`` of ``_Handle.npt``; ``ValueError`` for an unknown name or a mask that is not three 0 / 1 (before any library
    call; the numeric ranges are the library's to refuse)."""
    m = [1, 1, 1] if mask is None else list(mask)
    if len(m) != 3 or any(v not in (0, 1) for v in m):
        raise ValueError(f"mask {mask!r}: three entries 0 or 1 (Cartesian x y z)")
    t_end = temperature if temperature_end is None else temperature_end
    if ramp_steps is None:
        ramp_steps = 0 if temperature_end is None else int(steps)
    return NptParams(int(steps), _npt_code(NPT_THERMOSTATS, "thermostat", thermostat), _npt_code(NPT_BAROSTATS, "barostat", barostat),
                     _npt_code(NPT_COUPLINGS, "coupling", coupling), int(thermo_interval), (C.c_int32 * 3)(*[int(v) for v in m]),
                     float(timestep), float(temperature), float(t_end), float(friction), float(taut), float(taup), float(pressure),
                     float(compressibility), int(ramp_steps), int(step0), int(seed) & 0xFFFFFFFFFFFFFFFF)


class VibParams(C.Structure):
    """vssr_vib_params: A, K, eV; ``method`` one of ``VIB_METHODS``."""
    _fields_ = [("nfree", C.c_int32), ("method", C.c_int32), ("delta", C.c_double), ("temperature", C.c_double), ("e_min", C.c_double)]


VIB_METHODS = {"standard": 0, "frederiksen": 1}
VIB_STOP_REASONS = {1: "done", 2: "non-finite energy or force at a displacement", 3: "eigen-solver sweep limit"}
VIB_MAX_DOF = 256        # degrees of freedom per structure the device eigen-solver takes (85 vib atoms)
# eV per sqrt(eV / A^2 / amu): hbar 1e10 / sqrt(e amu) from the CODATA 2018 values of csrc/md_dev.h and csrc/vib.hip
VIB_ENERGY_UNIT = 1.054571817e-34 * 1e10 / (1.602176634e-19 * 1.66053906660e-27) ** 0.5
EV_PER_INV_CM = 1.239841984e-4


def vib_method_code(method) -> int:
    """The VSSR_VIB_* value of ``"standard"`` / ``"frederiksen"``; ``ValueError`` for anything else."""
    if not isinstance(method, str) or method not in VIB_METHODS:
        raise ValueError(f"vibrations method {method!r}: one of {', '.join(repr(k) for k in VIB_METHODS)}")
    return VIB_METHODS[method]


class NebParams(C.Structure):
    """vssr_neb_params: eV / A^2, eV / A; ``method`` one of ``NEB_METHODS``; the FIRE fields as ``FireParams``."""
    _fields_ = [("max_steps", C.c_int32), ("method", C.c_int32), ("climb", C.c_int32), ("k", C.c_double), ("fmax", C.c_double),
                ("dt", C.c_double), ("maxstep", C.c_double), ("dtmax", C.c_double), ("finc", C.c_double), ("fdec", C.c_double),
                ("astart", C.c_double), ("fa", C.c_double), ("nmin", C.c_int32)]

    @classmethod
    def default(cls, max_steps=100, method="improvedtangent", climb=False, k=0.1, fmax=0.05, dt=0.1, maxstep=0.2, dtmax=1.0, finc=1.1,
                fdec=0.5, astart=0.1, fa=0.99, nmin=5):
        if climb not in (False, True, 0, 1):
            raise ValueError(f"climb {climb!r}: a bool")
        return cls(int(max_steps), neb_method_code(method), int(bool(climb)), float(k), float(fmax), float(dt), float(maxstep), float(dtmax),
                   float(finc), float(fdec), float(astart), float(fa), int(nmin))


NEB_METHODS = {"improvedtangent": 0, "aseneb": 1}
NEB_STOP_REASONS = {1: "converged", 2: "max steps", 3: "non-finite energy or force", 4: "zero tangent (coincident images)"}


def neb_method_code(method) -> int:
    """The VSSR_NEB_* value of ``"improvedtangent"`` / ``"aseneb"``; ``ValueError`` for anything else."""
    if not isinstance(method, str) or method not in NEB_METHODS:
        raise ValueError(f"NEB method {method!r}: one of {', '.join(repr(k) for k in NEB_METHODS)}")
    return NEB_METHODS[method]


class DimerParams(C.Structure):
    """vssr_dimer_params: A, rad, eV / A; the FIRE fields as ``NebParams``."""
    _fields_ = [("max_steps", C.c_int32), ("max_rot_first", C.c_int32), ("max_rot", C.c_int32), ("nmin", C.c_int32), ("delta", C.c_double),
                ("phi_tol", C.c_double), ("fmax", C.c_double), ("displace", C.c_double), ("dt", C.c_double), ("maxstep", C.c_double),
                ("dtmax", C.c_double), ("finc", C.c_double), ("fdec", C.c_double), ("astart", C.c_double), ("fa", C.c_double),
                ("seed", C.c_uint64)]

    @classmethod
    def default(cls, max_steps=100, max_rot_first=8, max_rot=1, delta=0.01, phi_tol=np.pi / 180.0, fmax=0.05, displace=0.0, seed=0, dt=0.1,
                maxstep=0.2, dtmax=1.0, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, nmin=5):
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed {seed!r}: an integer in [0, 2^64)")
        return cls(int(max_steps), int(max_rot_first), int(max_rot), int(nmin), float(delta), float(phi_tol), float(fmax), float(displace),
                   float(dt), float(maxstep), float(dtmax), float(finc), float(fdec), float(astart), float(fa), int(seed))


DIMER_STOP_REASONS = {1: "converged", 2: "max steps", 3: "non-finite energy or force"}


class CellRelaxParams(C.Structure):
    """vssr_cell_relax_params: eV / A, eV / A^3; ``mask`` in Voigt order xx yy zz yz xz xy; the FIRE fields as ``NebParams``."""
    _fields_ = [("max_steps", C.c_int32), ("nmin", C.c_int32), ("hydrostatic_strain", C.c_int32), ("mask", C.c_int32 * 6),
                ("fmax", C.c_double), ("scalar_pressure", C.c_double), ("cell_factor", C.c_double), ("dt", C.c_double),
                ("maxstep", C.c_double), ("dtmax", C.c_double), ("finc", C.c_double), ("fdec", C.c_double), ("astart", C.c_double),
                ("fa", C.c_double)]

    @classmethod
    def default(cls, max_steps=100, fmax=0.05, scalar_pressure=0.0, mask=None, hydrostatic_strain=False, cell_factor=0.0, dt=0.1,
                maxstep=0.2, dtmax=1.0, finc=1.1, fdec=0.5, astart=0.1, fa=0.99, nmin=5):
        m = [1] * 6 if mask is None else list(mask)
        if len(m) != 6 or any(v not in (0, 1) for v in m):
            raise ValueError(f"mask {mask!r}: six entries 0 or 1 (Voigt order xx yy zz yz xz xy)")
        if hydrostatic_strain not in (False, True, 0, 1):
            raise ValueError(f"hydrostatic_strain {hydrostatic_strain!r}: a bool")
        return cls(int(max_steps), int(nmin), int(bool(hydrostatic_strain)), (C.c_int32 * 6)(*[int(v) for v in m]), float(fmax),
                   float(scalar_pressure), float(cell_factor), float(dt), float(maxstep), float(dtmax), float(finc), float(fdec),
                   float(astart), float(fa))


CELL_STOP_REASONS = {1: "converged", 2: "max steps", 3: "non-finite energy, force or stress",
                     4: "cell left the image range of the upload or degenerated"}


# who runs optimizer="BFGSLineSearch" for a calculator: ASE's class on the host, one optimizer per chain ("ase", the default), or the
# lock-step device optimizer (vssr_batch_relax_bfgs_linesearch)
LINESEARCH_DRIVERS = ("ase", "device")


def linesearch_driver_check(driver) -> str:
    """``driver`` if it is ``"ase"`` or ``"device"``; ``ValueError`` for anything else."""
    if not isinstance(driver, str) or driver not in LINESEARCH_DRIVERS:
        raise ValueError(f"linesearch driver {driver!r}: one of {', '.join(repr(k) for k in LINESEARCH_DRIVERS)}")
    return driver


class GmmConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_components", C.c_int32), ("dim", C.c_int32),
                ("means", C.POINTER(C.c_double)), ("prec_chol", C.POINTER(C.c_double)), ("weights", C.POINTER(C.c_double)),
                ("log_2pi", C.c_double)]


class GmmFitConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_components", C.c_int32), ("dim", C.c_int32),
                ("covariance_type", C.c_int32), ("max_iter", C.c_int32), ("n_init", C.c_int32), ("init", C.c_int32),
                ("tol", C.c_double), ("reg_covar", C.c_double), ("seed", C.c_uint64)]


class GmmFitResult(C.Structure):
    _fields_ = [("n_iter", C.c_int32), ("converged", C.c_int32), ("best_init", C.c_int32), ("n_lower_bounds", C.c_int32),
                ("lower_bound", C.c_double), ("lower_bounds", C.POINTER(C.c_double)), ("lower_bounds_cap", C.c_int32)]


class ClusterConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("dim", C.c_int32), ("n_components", C.c_int32),
                ("whiten", C.c_int32), ("cluster_dims", C.c_int32)]


class ClusterPcaResult(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("n_sweeps", C.c_int32), ("converged", C.c_int32)]


GMM_COV_TYPES = {"full": 0, "tied": 1, "diag": 2, "spherical": 3}
GMM_INITS = {"given": 0, "kmeans": 1, "random_from_data": 2}
GMM_ILL_DEFINED = "ill-defined empirical covariance"   # (in the message of the reference's ValueError)

# order / rows codes of vssr_gmm_score_batch
GMM_ORDERS = {"atomic": 0, "system_sum": 1, "system_mean": 2, "system_max": 3, "system_min": 4, "system_mean_squared": 5,
              "system_root_mean_squared": 6}
GMM_ROWS = {"atoms": 0, "mean": 1}


class Out(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_float)) for n in
                ("energy", "energy_std", "forces", "forces_std", "energy_models", "energy_atoms")]


_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  The PyTorch wheel carries its own ``libamdhip64.so`` / ``libhsa-runtime64.so``; if
    ``libvssr_eval.so`` has already brought up the system copy (``/opt/rocm``), a later ``import torch`` loads the second
    copy and finds no devices ("No HIP GPUs are available": the sharding path, which hands the engine's buffers to
    ``torch.distributed``, would fail whenever torch is imported after the first engine).  Loading torch's copy first --
    without importing torch -- makes both sides resolve the same runtime whatever the import order
    (``VSSR_SYSTEM_HIP=1`` skips this)."""
    if os.environ.get("VSSR_SYSTEM_HIP") == "1" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for loc in (spec.submodule_search_locations or []) if spec else []:
        p = os.path.join(loc, "lib", "libamdhip64.so")
        if os.path.exists(p):
            try:
                C.CDLL(p, mode=C.RTLD_GLOBAL)
            except OSError:
                pass   # (an unusable bundled copy: the system runtime serves the library)
            return


def load_library():
    """Load libvssr_eval.so; raise BackendError (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). This backend has no CPU fallback.")
    _share_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    vp, ip, dp, fp, u8p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), \
        C.POINTER(C.c_uint8)
    i64p = C.POINTER(C.c_int64)
    L.vssr_abi_version.restype = C.c_int
    L.vssr_create.restype = C.c_int
    L.vssr_create.argtypes = [C.POINTER(PainnConfig), C.POINTER(vp)]
    L.vssr_destroy.restype = None
    L.vssr_destroy.argtypes = [vp]
    L.vssr_last_error.restype = C.c_char_p
    L.vssr_last_error.argtypes = [vp]
    L.vssr_eval.restype = C.c_int
    L.vssr_eval.argtypes = [vp, C.c_int32, ip, dp, dp, u8p, C.c_uint32, C.POINTER(Out)]
    L.vssr_eval_batch.restype = C.c_int
    L.vssr_eval_batch.argtypes = [vp, C.c_int32, ip, ip, dp, dp, u8p, C.c_uint32, C.POINTER(Out)]
    L.vssr_batch_upload.restype = C.c_int
    L.vssr_batch_upload.argtypes = [vp, C.c_int32, ip, ip, dp, dp, u8p]
    L.vssr_batch_set_positions.restype = C.c_int
    L.vssr_batch_set_positions.argtypes = [vp, dp]
    L.vssr_batch_run.restype = C.c_int
    L.vssr_batch_run.argtypes = [vp, C.c_uint32]
    L.vssr_batch_download.restype = C.c_int
    L.vssr_batch_download.argtypes = [vp, C.c_uint32, C.POINTER(Out)]
    L.vssr_synchronize.restype = C.c_int
    L.vssr_synchronize.argtypes = [vp]
    L.vssr_profile_enable.restype = C.c_int
    L.vssr_profile_enable.argtypes = [vp, C.c_int]
    L.vssr_profile_reset.restype = C.c_int
    L.vssr_profile_reset.argtypes = [vp]
    L.vssr_profile_read.restype = C.c_int
    L.vssr_profile_read.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), i64p, dp, ip]
    L.vssr_batch_stats.restype = C.c_int
    L.vssr_batch_stats.argtypes = [vp, i64p, i64p, i64p]
    L.vssr_batch_neighbors.restype = C.c_int
    L.vssr_batch_neighbors.argtypes = [vp, C.c_int64, ip, ip, ip, fp, i64p]
    L.vssr_debug_read.restype = C.c_int
    L.vssr_debug_read.argtypes = [vp, C.c_char_p, C.c_int32, fp, C.c_int64, i64p]
    L.vssr_tersoff_create.restype = C.c_int
    L.vssr_tersoff_create.argtypes = [C.c_int32, C.c_int32, dp, C.POINTER(vp)]
    L.vssr_tersoff_eval_batch.restype = C.c_int
    L.vssr_tersoff_eval_batch.argtypes = [vp, C.c_int32, ip, ip, dp, dp, u8p, C.c_uint32, C.POINTER(Out), dp, dp, dp]
    L.vssr_tersoff_create_from_text.restype = C.c_int
    L.vssr_tersoff_create_from_text.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.vssr_batch_relax_cg.restype = C.c_int
    L.vssr_batch_relax_cg.argtypes = [vp, C.POINTER(CgParams), u8p, C.c_uint32, dp, ip, ip, ip]
    L.vssr_batch_relax_cg_driver.restype = C.c_int
    L.vssr_batch_relax_cg_driver.argtypes = [vp, C.c_int32, ip]
    L.vssr_batch_relax_bfgs_linesearch.restype = C.c_int
    L.vssr_batch_relax_bfgs_linesearch.argtypes = [vp, C.POINTER(BfgsLsParams), u8p, C.c_uint32, dp, ip, ip, ip]
    u64p = C.POINTER(C.c_uint64)
    L.vssr_batch_md.restype = C.c_int
    L.vssr_batch_md.argtypes = [vp, C.POINTER(MdParams), dp, u8p, u64p, C.c_uint32, dp, dp, ip, ip]
    L.vssr_batch_md_set_velocities.restype = C.c_int
    L.vssr_batch_md_set_velocities.argtypes = [vp, dp]
    L.vssr_batch_md_draw_velocities.restype = C.c_int
    L.vssr_batch_md_draw_velocities.argtypes = [vp, dp, u8p, u64p, C.c_double, C.c_uint64]
    L.vssr_batch_md_get_velocities.restype = C.c_int
    L.vssr_batch_md_get_velocities.argtypes = [vp, dp]
    L.vssr_batch_md_driver.restype = C.c_int
    L.vssr_batch_md_driver.argtypes = [vp, C.c_int32, ip]
    L.vssr_batch_neb.restype = C.c_int
    L.vssr_batch_neb.argtypes = [vp, C.POINTER(NebParams), u8p, ip, C.c_int32, C.c_uint32, dp, dp, dp, dp, ip]
    L.vssr_batch_dimer.restype = C.c_int
    L.vssr_batch_dimer.argtypes = [vp, C.POINTER(DimerParams), u8p, dp, C.POINTER(C.c_uint64), C.c_uint32, dp, dp, dp, dp, ip]
    L.vssr_batch_relax_cell.restype = C.c_int
    L.vssr_batch_relax_cell.argtypes = [vp, C.POINTER(CellRelaxParams), u8p, C.c_uint32, dp, dp, ip, ip, dp]
    L.vssr_batch_get_cell.restype = C.c_int
    L.vssr_batch_get_cell.argtypes = [vp, dp]
    L.vssr_batch_md_npt.restype = C.c_int
    L.vssr_batch_md_npt.argtypes = [vp, C.POINTER(NptParams), dp, u8p, u64p, C.c_uint32, dp, dp, dp, ip, ip]
    L.vssr_batch_vibrations.restype = C.c_int
    L.vssr_batch_vibrations.argtypes = [vp, C.POINTER(VibParams), dp, u8p, ip, C.c_int32, C.c_int32, C.c_uint32, dp, dp, dp, dp, ip]
    L.vssr_eam_create.restype = C.c_int
    L.vssr_eam_create.argtypes = [C.c_int32, C.POINTER(EamGrid), dp, dp, dp, C.POINTER(vp)]
    L.vssr_eam_create_alloy.restype = C.c_int
    L.vssr_eam_create_alloy.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(EamGrid), dp, dp, dp, C.POINTER(vp)]
    L.vssr_eam_create_adp.restype = C.c_int
    L.vssr_eam_create_adp.argtypes = [C.c_int32, C.c_int32, C.POINTER(EamGrid), dp, dp, dp, dp, dp, C.POINTER(vp)]
    L.vssr_eam_eval_batch.restype = C.c_int
    L.vssr_eam_eval_batch.argtypes = L.vssr_tersoff_eval_batch.argtypes
    L.vssr_sw_create.restype = C.c_int
    L.vssr_sw_create.argtypes = [C.c_int32, C.c_int32, dp, C.POINTER(vp)]
    L.vssr_sw_create_from_text.restype = C.c_int
    L.vssr_sw_create_from_text.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.vssr_sw_eval_batch.restype = C.c_int
    L.vssr_sw_eval_batch.argtypes = L.vssr_tersoff_eval_batch.argtypes
    L.vssr_vashishta_create.restype = C.c_int
    L.vssr_vashishta_create.argtypes = [C.c_int32, C.c_int32, dp, C.POINTER(vp)]
    L.vssr_vashishta_create_from_text.restype = C.c_int
    L.vssr_vashishta_create_from_text.argtypes = [C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.vssr_vashishta_eval_batch.restype = C.c_int
    L.vssr_vashishta_eval_batch.argtypes = L.vssr_tersoff_eval_batch.argtypes
    L.vssr_pair_create.restype = C.c_int
    L.vssr_pair_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PairTerm), dp, C.POINTER(vp)]
    L.vssr_pair_create_kspace.restype = C.c_int
    L.vssr_pair_create_kspace.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PairTerm), dp, C.POINTER(KSpace), C.POINTER(vp)]
    L.vssr_pair_create_kspace_slab.restype = C.c_int
    L.vssr_pair_create_kspace_slab.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PairTerm), dp, C.POINTER(KSpace), C.c_double,
                                               C.POINTER(vp)]
    L.vssr_pair_eval_batch.restype = C.c_int
    L.vssr_pair_eval_batch.argtypes = L.vssr_tersoff_eval_batch.argtypes
    L.vssr_batch_relax_fire.restype = C.c_int
    L.vssr_batch_relax_fire.argtypes = [vp, C.POINTER(FireParams), u8p, C.c_uint32, dp, ip, u8p]
    L.vssr_batch_relax_bfgs.restype = C.c_int
    L.vssr_batch_relax_bfgs.argtypes = [vp, C.POINTER(BfgsParams), u8p, C.c_uint32, dp, ip, u8p]
    L.vssr_batch_device_results.restype = C.c_int
    L.vssr_batch_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.vssr_batch_device_results_f64.restype = C.c_int
    L.vssr_batch_device_results_f64.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.vssr_batch_relax_counts.restype = C.c_int
    L.vssr_batch_relax_counts.argtypes = [vp, i64p, i64p]
    L.vssr_batch_energy_f64.restype = C.c_int
    L.vssr_batch_energy_f64.argtypes = [vp, dp, dp, dp]
    L.vssr_batch_results_f64.restype = C.c_int
    L.vssr_batch_results_f64.argtypes = [vp, dp, dp, dp]
    L.vssr_batch_traj_configure.restype = C.c_int
    L.vssr_batch_traj_configure.argtypes = [vp, C.c_int32]
    L.vssr_batch_traj_read.restype = C.c_int
    L.vssr_batch_traj_read.argtypes = [vp, C.c_int32, ip, dp, fp, dp, ip]
    L.vssr_batch_embedding.restype = C.c_int
    L.vssr_batch_embedding.argtypes = [vp, C.c_int32, fp, C.c_int64, i64p]
    L.vssr_batch_saturated.restype = C.c_int
    L.vssr_batch_saturated.argtypes = [vp, u8p, ip]
    L.vssr_batch_stress.restype = C.c_int
    L.vssr_batch_stress.argtypes = [vp, dp, dp]
    L.vssr_device_context.restype = C.c_int
    L.vssr_device_context.argtypes = [vp, ip, C.POINTER(vp), C.POINTER(vp)]
    L.vssr_debug_capacity.restype = C.c_int
    L.vssr_debug_capacity.argtypes = [vp, C.c_int32, C.c_int32, ip]
    L.vssr_gmm_create.restype = C.c_int
    L.vssr_gmm_create.argtypes = [C.POINTER(GmmConfig), C.POINTER(vp)]
    L.vssr_gmm_score_rows.restype = C.c_int
    L.vssr_gmm_score_rows.argtypes = [vp, C.c_int64, dp, dp, dp]
    L.vssr_gmm_score_batch.restype = C.c_int
    L.vssr_gmm_score_batch.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, dp, dp]
    L.vssr_gmm_fit_create.restype = C.c_int
    L.vssr_gmm_fit_create.argtypes = [C.POINTER(GmmFitConfig), C.POINTER(vp)]
    L.vssr_gmm_fit_append_rows.restype = C.c_int
    L.vssr_gmm_fit_append_rows.argtypes = [vp, C.c_int64, dp]
    L.vssr_gmm_fit_append_batch.restype = C.c_int
    L.vssr_gmm_fit_append_batch.argtypes = [vp, vp, C.c_int32, C.c_int32]
    L.vssr_gmm_fit_clear.restype = C.c_int
    L.vssr_gmm_fit_clear.argtypes = [vp]
    L.vssr_gmm_fit_set_init.restype = C.c_int
    L.vssr_gmm_fit_set_init.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_int32)]
    L.vssr_gmm_fit_run.restype = C.c_int
    L.vssr_gmm_fit_run.argtypes = [vp, C.POINTER(GmmFitResult)]
    L.vssr_gmm_fit_params.restype = C.c_int
    L.vssr_gmm_fit_params.argtypes = [vp, dp, dp, dp, dp]
    L.vssr_gmm_fit_scorer.restype = C.c_int
    L.vssr_gmm_fit_scorer.argtypes = [vp, C.c_double, C.POINTER(vp)]
    L.vssr_cluster_create.restype = C.c_int
    L.vssr_cluster_create.argtypes = [C.POINTER(ClusterConfig), C.POINTER(vp)]
    L.vssr_cluster_append_rows.restype = C.c_int
    L.vssr_cluster_append_rows.argtypes = [vp, C.c_int64, dp]
    L.vssr_cluster_append_batch.restype = C.c_int
    L.vssr_cluster_append_batch.argtypes = [vp, vp, C.c_int32]
    L.vssr_cluster_clear.restype = C.c_int
    L.vssr_cluster_clear.argtypes = [vp]
    L.vssr_cluster_pca.restype = C.c_int
    L.vssr_cluster_pca.argtypes = [vp, C.POINTER(ClusterPcaResult)]
    L.vssr_cluster_pca_params.restype = C.c_int
    L.vssr_cluster_pca_params.argtypes = [vp, dp, dp, dp, dp]
    L.vssr_cluster_projected.restype = C.c_int
    L.vssr_cluster_projected.argtypes = [vp, C.c_int64, C.c_int64, dp]
    L.vssr_cluster_set_points.restype = C.c_int
    L.vssr_cluster_set_points.argtypes = [vp, C.c_int64, dp]
    L.vssr_cluster_linkage.restype = C.c_int
    L.vssr_cluster_linkage.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    if L.vssr_abi_version() != 1:
        raise BackendError("libvssr_eval.so ABI version mismatch")
    _lib = L
    return L


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def pack_batch(structs):
    """List of (numbers, positions, cell, pbc) -> concatenated ABI arrays."""
    n_atoms = np.array([len(s[0]) for s in structs], dtype=np.int32)
    Z = np.ascontiguousarray(np.concatenate([np.asarray(s[0]) for s in structs]), dtype=np.int32)
    pos = np.ascontiguousarray(np.concatenate([np.asarray(s[1], dtype=np.float64).reshape(-1, 3) for s in structs]))
    cell = np.ascontiguousarray(np.stack([np.asarray(s[2], dtype=np.float64).reshape(9) for s in structs]))
    pbc = np.ascontiguousarray(np.stack([np.asarray(s[3]).astype(np.uint8).reshape(3) for s in structs]))
    return n_atoms, Z, pos, cell, pbc


def _batch_arrays(n_atoms, Z, pos, cell, pbc):
    """The five batch arrays in the ABI's dtypes, C-contiguous (``n_atoms`` int32 [B], ``Z`` -- atomic numbers or types -- int32 [N],
    ``pos`` float64 [N, 3], ``cell`` float64 [B, 9], ``pbc`` uint8 [B, 3]); ``ValueError`` when their sizes disagree."""
    n_atoms = np.ascontiguousarray(n_atoms, dtype=np.int32)
    Z = np.ascontiguousarray(Z, dtype=np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    pbc = np.ascontiguousarray(pbc, dtype=np.uint8)
    B, N = len(n_atoms), Z.shape[0]
    if N != int(n_atoms.sum()) or pos.size != 3 * N or cell.size != 9 * B or pbc.size != 3 * B:
        raise ValueError("inconsistent batch arrays")
    return n_atoms, Z, pos, cell, pbc


def _fixed_arg(fixed, N):
    """A FixAtoms mask as the ABI takes it: uint8 [N], C-contiguous, or None."""
    if fixed is None:
        return None
    fx = np.ascontiguousarray(fixed, dtype=np.uint8)
    if fx.size != N:
        raise ValueError("fixed mask does not match the resident batch")
    return fx


class _DeviceArray:
    """A float32 (or int32) vector in device memory owned by an engine (``__cuda_array_interface__`` v2)."""

    def __init__(self, ptr, n, typestr="<f4"):
        # (read-only flag False: torch refuses read-only device arrays; consumers only read these buffers)
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


class _Handle:
    """Owns a vssr_handle*; shared plumbing for the PaiNN and Tersoff engines."""

    last_md_driver = None         # "lockstep" / "resident": the driver the last md() of this engine ran

    def __init__(self):
        self._lib = load_library()
        self._h = C.c_void_p(None)
        self.n_models = 1
        self._set_resident(np.zeros(0, np.int32))   # (no batch yet)

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.vssr_last_error(self._h)
            raise BackendError(f"vssr error {rc}: {msg.decode() if msg else '?'}")

    def close(self):
        if self._h:
            self._lib.vssr_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- resident-batch API ------------------------------------------------------------------
    def upload(self, structs):
        n_atoms, Z, pos, cell, pbc = pack_batch(structs)
        self.upload_arrays(n_atoms, Z, pos, cell, pbc)

    def _set_resident(self, n_atoms):
        """The shape of the batch the handle now holds: what ``download``, ``set_positions`` and the relaxations size arrays by."""
        self._n_cfg, self._n_atoms = len(n_atoms), int(n_atoms.sum())
        self._cfg_start = np.concatenate([[0], np.cumsum(n_atoms)]).astype(np.int64)

    def upload_arrays(self, n_atoms, Z, pos, cell, pbc):
        n_atoms, Z, pos, cell, pbc = _batch_arrays(n_atoms, Z, pos, cell, pbc)
        self._check(self._lib.vssr_batch_upload(self._h, len(n_atoms), _ptr(n_atoms, C.c_int32),
                                                _ptr(Z, C.c_int32), _ptr(pos, C.c_double),
                                                _ptr(cell, C.c_double), _ptr(pbc, C.c_uint8)))
        self._set_resident(n_atoms)

    def set_positions(self, pos):
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        if pos.size != 3 * self._n_atoms:
            raise ValueError("positions do not match the resident batch")
        self._check(self._lib.vssr_batch_set_positions(self._h, _ptr(pos, C.c_double)))

    def run(self, want=WANT_ALL):
        self._check(self._lib.vssr_batch_run(self._h, int(want)))

    def synchronize(self):
        self._check(self._lib.vssr_synchronize(self._h))

    def download(self, want=WANT_ALL):
        B, N, M = self._n_cfg, self._n_atoms, self.n_models
        res = {
            "energy": np.zeros(B, np.float32), "energy_std": np.zeros(B, np.float32),
            "forces": np.zeros((N, 3), np.float32), "forces_std": np.zeros((N, 3), np.float32),
            "energy_models": np.zeros((B, M), np.float32), "energy_atoms": np.zeros(N, np.float32),
        }
        out = Out(*[_ptr(res[k], C.c_float) for k in
                    ("energy", "energy_std", "forces", "forces_std", "energy_models", "energy_atoms")])
        self._check(self._lib.vssr_batch_download(self._h, int(want), C.byref(out)))
        res["cfg_start"] = self._cfg_start
        res["saturated"] = self.saturated()
        # the same energies without the float32 output word (vssr_batch_energy_f64): what acceptance tests and relaxation
        # drivers compare; "energy" keeps the reference's float32 type.  Only when energies were asked for (a second call with
        # three blocking copies otherwise bought nothing).
        if int(want) & WANT_ENERGY:
            e64, s64, m64 = np.zeros(B), np.zeros(B), np.zeros((B, M))
            self._check(self._lib.vssr_batch_energy_f64(self._h, _ptr(e64, C.c_double), _ptr(s64, C.c_double), _ptr(m64, C.c_double)))
            res["energy_f64"], res["energy_std_f64"], res["energy_models_f64"] = e64, s64, m64
        return res

    def embedding(self, model=None):
        """Per-atom latent features (final scalar state, the readout's input) of the resident batch after a run:
        ``[M, sum N, F]`` for ``model=None``, ``[sum N, F]`` for one ensemble member (vssr_batch_embedding)."""
        n = C.c_int64(0)
        m = -1 if model is None else int(model)
        self._check(self._lib.vssr_batch_embedding(self._h, m, None, 0, C.byref(n)))
        buf = np.zeros(n.value, np.float32)
        self._check(self._lib.vssr_batch_embedding(self._h, m, _ptr(buf, C.c_float), n.value, C.byref(n)))
        return buf.reshape((self.n_models, self._n_atoms, -1) if model is None else (self._n_atoms, -1))

    def embedding_dim(self):
        """Feature width F of the resident embedding (needs a completed run, as ``embedding``)."""
        n = C.c_int64(0)
        self._check(self._lib.vssr_batch_embedding(self._h, 0, None, 0, C.byref(n)))
        return int(n.value // max(self._n_atoms, 1))

    def saturated(self):
        """bool [B]: chains whose last evaluation left the range of the fp16-split arithmetic (a value beyond +-65504 was
        clamped) or produced a non-finite energy -- their results are finite but not the model's (vssr_batch_saturated)."""
        flags = np.zeros(self._n_cfg, np.uint8)
        n = C.c_int32(0)
        self._check(self._lib.vssr_batch_saturated(self._h, _ptr(flags, C.c_uint8), C.byref(n)))
        return flags.astype(bool)

    def stress(self):
        """``(stress [B, 6], stress_std [B, 6])`` float64, Voigt order xx yy zz yz xz xy in eV / A^3 (ASE's convention): the
        virial of the LAST evaluation of every chain, from what that evaluation left on the device (vssr_batch_stress; the run
        must have produced forces).  PaiNN: the edge gradients of the reverse pass, mean and spread over the models.  Tersoff,
        SW and EAM engines: fp64, one model, ``stress_std`` all zeros.  After a relaxation that left a partial graph (the
        chain-resident CG of ``relax_cg_f64``, a lock-step relaxation whose chains converged early) the call raises: ``run()``
        once first."""
        st, sd = np.zeros((self._n_cfg, 6)), np.zeros((self._n_cfg, 6))
        self._check(self._lib.vssr_batch_stress(self._h, _ptr(st, C.c_double), _ptr(sd, C.c_double)))
        return st, sd

    def device_results(self):
        """``(energy, energy_std)`` of the resident batch as zero-copy device arrays (objects with
        ``__cuda_array_interface__``: ``torch.as_tensor(x, device="cuda")`` wraps them).  Valid after a synchronised run."""
        e, s = C.c_void_p(None), C.c_void_p(None)
        self._check(self._lib.vssr_batch_device_results(self._h, C.byref(e), C.byref(s)))
        return _DeviceArray(e.value, self._n_cfg), _DeviceArray(s.value, self._n_cfg)

    def device_results_f64(self):
        """``(energy, energy_std)`` as zero-copy float64 device arrays (vssr_batch_device_results_f64)."""
        e, s = C.c_void_p(None), C.c_void_p(None)
        self._check(self._lib.vssr_batch_device_results_f64(self._h, C.byref(e), C.byref(s)))
        return _DeviceArray(e.value, self._n_cfg, "<f8"), _DeviceArray(s.value, self._n_cfg, "<f8")

    def device_context(self):
        """``(device ordinal, hipStream_t of the engine as int, device address of the overflow flag or None)``
        (vssr_device_context)."""
        d, st, fl = C.c_int32(0), C.c_void_p(None), C.c_void_p(None)
        self._check(self._lib.vssr_device_context(self._h, C.byref(d), C.byref(st), C.byref(fl)))
        return d.value, st.value or 0, fl.value

    def evaluate(self, structs, want=WANT_ALL):
        self.upload(structs)
        self.run(want)
        return self.download(want)

    # -- lock-step relaxation ------------------------------------------------------------------------
    def relax(self, optimizer="FIRE", **kw):
        """Dispatch on the reference's optimizer names (``mcmc/dynamics.py:119-127``: a name containing "BFGS" selects
        BFGS, everything else FIRE; BFGSLineSearch / CG / LAMMPS are not dispatched here: ``relax_bfgs_linesearch`` and ``relax_cg_f64``
        are called by name, the calculators' ``linesearch_driver`` / ``relax_batch`` choose them)."""
        name = str(optimizer)
        if "BFGSLineSearch" in name or "CG" in name or "LAMMPS" in name:
            raise BackendError(f"optimizer {optimizer!r} is not available on the device (FIRE and BFGS are)")
        return self.relax_bfgs(**kw) if "BFGS" in name else self.relax_fire(**kw)

    def relax_bfgs(self, fixed=None, max_steps=20, fmax=0.01, want=WANT_ALL, params=None, record_interval=0):
        """BFGS-relax every chain of the resident batch on the device (ASE BFGS, the reference's SrTiO3 optimizer).
        Same arguments and return value as :meth:`relax_fire`."""
        p = params or BfgsParams.default(max_steps, fmax)
        return self._relax_call(self._lib.vssr_batch_relax_bfgs, p, fixed, want, record_interval)

    def relax_fire(self, fixed=None, max_steps=20, fmax=0.01, want=WANT_ALL, params=None, record_interval=0):
        """FIRE-relax every chain of the resident batch on the device (reference optimize_slab with FIRE).
        ``fixed``: bool/uint8 [sum N], True = held fixed.  Returns dict(positions [sum N,3] float64,
        n_steps [B], converged [B]) — fetch energies/forces of the relaxed batch with download().
        ``record_interval`` k > 0 also records every chain after 0, k, 2k, ... optimizer steps (the reference's
        TrajectoryObserver, ``mcmc/dynamics.py:131-151``): key ``"traj"`` = dict(n_records [B], positions [R, sum N, 3],
        forces [R, sum N, 3] with FixAtoms applied, energies [R, B]); entries of chain b beyond n_records[b] are unused."""
        p = params or FireParams.default(max_steps, fmax)
        return self._relax_call(self._lib.vssr_batch_relax_fire, p, fixed, want, record_interval)

    def relax_bfgs_linesearch(self, fixed=None, max_steps=20, fmax=0.01, max_eval=None, want=WANT_ALL, params=None, record_interval=0):
        """BFGSLineSearch-relax every chain of the resident batch on the device (vssr_batch_relax_bfgs_linesearch: ASE's
        BFGSLineSearch restated, one lock-step evaluation per line-search trial).  Arguments as :meth:`relax_fire`, plus ``max_eval``,
        the evaluations a chain may spend (default ``20 * max_steps + 20``).  Returns the dict of :meth:`relax_fire` plus
        ``n_eval`` [B] and ``stop_reason`` [B] (``BFGSLS_STOP_REASONS``); ``converged`` is ``stop_reason == 1``.  The batch is left
        with a complete evaluation of the final positions: ``download()`` / ``results_f64()`` / ``stress()`` need no run.
        ``record_interval`` k records the points at which steps 0, k, 2k, ... open, never a line-search trial."""
        p = params or BfgsLsParams.default(max_steps, fmax, max_eval)
        ev, why = np.zeros(self._n_cfg, np.int32), np.zeros(self._n_cfg, np.int32)

        def call(h, pp, fx, want_, pos, steps, conv):
            return self._lib.vssr_batch_relax_bfgs_linesearch(h, pp, fx, want_, pos, steps, _ptr(ev, C.c_int32), _ptr(why, C.c_int32))

        out = self._relax_call(call, p, fixed, want, record_interval)
        out["n_eval"], out["stop_reason"], out["converged"] = ev, why, why == 1
        return out

    # -- molecular dynamics ---------------------------------------------------------------------------
    def _chain_ids(self, chain_id):
        if chain_id is None:
            return None
        ids = np.ascontiguousarray(chain_id, dtype=np.uint64)
        if ids.size != self._n_cfg:
            raise ValueError("chain ids do not match the resident batch")
        return ids

    def _masses(self, masses):
        m = np.ascontiguousarray(masses, dtype=np.float64)
        if m.size != self._n_atoms:
            raise ValueError("masses do not match the resident batch")
        return m

    def set_velocities(self, velocities=None):
        """Velocities [sum N, 3] in A / fs of the resident batch (``None``: zeros); they stay on the device until the next upload
        (vssr_batch_md_set_velocities)."""
        v = None
        if velocities is not None:
            v = np.ascontiguousarray(velocities, dtype=np.float64)
            if v.size != 3 * self._n_atoms:
                raise ValueError("velocities do not match the resident batch")
        self._check(self._lib.vssr_batch_md_set_velocities(self._h, _ptr(v, C.c_double)))

    def draw_velocities(self, masses, temperature, seed=0, fixed=None, chain_id=None):
        """Maxwell-Boltzmann velocities at ``temperature`` K for the resident batch, drawn on the device from (seed, chain id, atom);
        held atoms get 0, no centre-of-mass removal (vssr_batch_md_draw_velocities)."""
        m, fx, ids = self._masses(masses), _fixed_arg(fixed, self._n_atoms), self._chain_ids(chain_id)
        self._check(self._lib.vssr_batch_md_draw_velocities(self._h, _ptr(m, C.c_double), _ptr(fx, C.c_uint8), _ptr(ids, C.c_uint64),
                                                            float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def get_velocities(self):
        """The resident velocities, [sum N, 3] float64 in A / fs (vssr_batch_md_get_velocities)."""
        v = np.zeros((self._n_atoms, 3), np.float64)
        self._check(self._lib.vssr_batch_md_get_velocities(self._h, _ptr(v, C.c_double)))
        return v

    def md_driver(self, driver=None):
        """Set the handle's MD driver (``None``: leave it) and return the name of the one its last ``md`` ran, ``None`` before the
        first (vssr_batch_md_driver)."""
        code = -1 if driver is None else md_driver_code(driver)
        last = C.c_int32(0)
        self._check(self._lib.vssr_batch_md_driver(self._h, code, C.byref(last)))
        return MD_DRIVER_NAMES.get(last.value)

    def md(self, masses, steps, timestep, thermostat="nve", temperature=0.0, temperature_end=None, friction=0.0, ramp_steps=None,
           step0=0, seed=0, fixed=None, chain_id=None, thermo_interval=1, want=WANT_ALL, driver=None):
        """Integrate every chain of the resident batch for ``steps`` steps of ``timestep`` fs on the device (vssr_batch_md): velocity
        Verlet (``"nve"``) or Langevin BAOAB (``"langevin"``: ``temperature`` K running linearly to ``temperature_end`` over
        ``ramp_steps`` steps -- default: the ``steps`` of this call when an end temperature is given, else none --, ``friction`` in
        1 / fs).  The batch needs velocities (``set_velocities`` / ``draw_velocities``); ``masses`` [sum N] in amu.  ``step0`` is the
        absolute index of the first step: two calls of n steps, the second with ``step0=n``, equal one call of 2 n steps bit for bit.
        ``chain_id`` [B]: global chain ids of the random numbers (default 0 .. B-1).  ``driver``: ``"auto"`` / ``"lockstep"`` /
        ``"resident"`` (None: the handle's setting).  Returns dict(positions [sum N, 3], velocities [sum N, 3], epot / ekin
        [steps // thermo_interval + 1, B] in eV, n_done [B], stop_reason [B] (``MD_STOP_REASONS``)); ``download()`` /
        ``results_f64()`` / ``stress()`` serve the final state at once."""
        N, B = self._n_atoms, self._n_cfg
        m, fx, ids = self._masses(masses), _fixed_arg(fixed, N), self._chain_ids(chain_id)
        t_end = temperature if temperature_end is None else temperature_end
        if ramp_steps is None:
            ramp_steps = 0 if temperature_end is None else int(steps)
        p = MdParams(int(steps), md_thermostat_code(thermostat), int(thermo_interval), float(timestep), float(temperature), float(t_end),
                     float(friction), int(ramp_steps), int(step0), int(seed) & 0xFFFFFFFFFFFFFFFF)
        if driver is not None:
            self._check(self._lib.vssr_batch_md_driver(self._h, md_driver_code(driver), None))
        nrec = max(int(steps), 0) // max(int(thermo_interval), 1) + 1
        pos, thermo = np.zeros((N, 3), np.float64), np.zeros((nrec, B, 2), np.float64)
        done, why = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._check(self._lib.vssr_batch_md(self._h, C.byref(p), _ptr(m, C.c_double), _ptr(fx, C.c_uint8), _ptr(ids, C.c_uint64), int(want),
                                            _ptr(pos, C.c_double), _ptr(thermo, C.c_double), _ptr(done, C.c_int32), _ptr(why, C.c_int32)))
        self.last_relax_counts = self.relax_counts()
        self.last_md_driver = self.md_driver()
        return {"positions": pos, "velocities": self.get_velocities(), "epot": thermo[:, :, 0].copy(), "ekin": thermo[:, :, 1].copy(),
                "n_done": done, "stop_reason": why}

    def npt(self, masses, steps, timestep, fixed=None, chain_id=None, want=WANT_ALL, params=None, **kw):
        """Constant-pressure / weakly coupled MD of the resident batch on the device, in lock step (vssr_batch_md_npt; the contract is
        its header comment and tests/npt_oracle.py).  ``kw``: the keywords of ``npt_params`` -- ``thermostat`` ``"none"`` /
        ``"langevin"`` / ``"berendsen"`` (``temperature``, ``temperature_end``, ``ramp_steps``, ``friction`` 1 / fs, ``taut`` fs),
        ``barostat`` ``"none"`` / ``"berendsen"`` / ``"crescale"`` (``pressure`` eV / A^3, ``compressibility`` A^3 / eV, ``taup`` fs,
        ``mask`` three 0 / 1 per Cartesian axis, ``coupling`` ``"isotropic"`` / ``"per_axis"``), ``step0``, ``seed``,
        ``thermo_interval`` (``params``: an ``NptParams`` instead).  The batch needs velocities.  Returns dict(positions [sum N, 3],
        velocities [sum N, 3], cells [B, 3, 3], epot / ekin / volume / pressure [steps // thermo_interval + 1, B] (pressure NaN
        without a barostat), n_done [B], stop_reason [B] (``NPT_STOP_REASONS``)); ``download()`` / ``results_f64()`` / ``stress()`` /
        ``get_cell()`` serve the final state at once, and later runs keep the new cells until the next upload."""
        N, B = self._n_atoms, self._n_cfg
        p = params or npt_params(steps, timestep, **kw)
        m, fx, ids = self._masses(masses), _fixed_arg(fixed, N), self._chain_ids(chain_id)
        nrec = max(int(p.n_steps), 0) // max(int(p.thermo_interval), 1) + 1
        pos, cells, thermo = np.zeros((N, 3), np.float64), np.zeros((max(B, 1), 3, 3), np.float64), np.zeros((nrec, B, 4), np.float64)
        done, why = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._check(self._lib.vssr_batch_md_npt(self._h, C.byref(p), _ptr(m, C.c_double), _ptr(fx, C.c_uint8), _ptr(ids, C.c_uint64),
                                                int(want), _ptr(pos, C.c_double), _ptr(cells, C.c_double), _ptr(thermo, C.c_double),
                                                _ptr(done, C.c_int32), _ptr(why, C.c_int32)))
        self.last_relax_counts = self.relax_counts()
        return {"positions": pos, "velocities": self.get_velocities(), "cells": cells[:B], "epot": thermo[:, :, 0].copy(),
                "ekin": thermo[:, :, 1].copy(), "volume": thermo[:, :, 2].copy(), "pressure": thermo[:, :, 3].copy(), "n_done": done,
                "stop_reason": why}

    # -- harmonic vibrations -------------------------------------------------------------------------
    def vibrations(self, masses, vib=None, n_rep=None, delta=0.01, nfree=2, method="standard", temperature=0.0, e_min=0.0, want=WANT_ALL,
                   return_hessian=False, return_modes=False):
        """Finite-difference Hessian, modes and thermochemistry of every structure of the resident batch on the device
        (vssr_batch_vibrations).  ``masses`` [sum N] amu; ``vib`` [sum N] bool, the atoms that are displaced (None: all); ``n_rep`` [G]:
        consecutive chains that are bit-identical replicas of one structure and share its displacements (None: every chain is its
        own structure).  ``delta`` in A, ``nfree`` 2 or 4, ``method`` ``"standard"`` / ``"frederiksen"``, ``temperature`` in K; modes
        with energy <= ``e_min`` eV stay out of the sums.  Returns a dict of per-group lists / arrays: ``energies`` (list of [m], eV,
        negative = imaginary), ``energy`` / ``zpe`` / ``f_vib`` [G], ``m`` / ``n_imag`` / ``n_left_out`` / ``stop_reason`` [G]
        (``VIB_STOP_REASONS``), and with the flags ``hessian`` (list of [m, m], eV / A^2) and ``modes`` (list of [m, m], rows =
        mass-weighted unit eigenvectors).  The batch is back at its input positions, evaluated, afterwards."""
        N, B = self._n_atoms, self._n_cfg
        m = self._masses(masses)
        mask = None
        if vib is not None:
            mask = np.ascontiguousarray(np.asarray(vib).astype(bool), dtype=np.uint8).reshape(-1)
            if mask.size != N:
                raise ValueError("vib mask does not match the resident batch")
        if n_rep is None:
            reps, G = None, B
        else:
            reps = np.ascontiguousarray(n_rep, dtype=np.int32).reshape(-1)
            G = int(reps.size)
        # ld: the largest m of any chain (a group's m is that of its first chain; a bad n_rep is the library's to refuse)
        start = self._cfg_start
        ld = max([3 * (int(start[b + 1] - start[b]) if mask is None else int(np.count_nonzero(mask[start[b]:start[b + 1]]))) for b in range(B)]
                 + [1])
        p = VibParams(int(nfree), vib_method_code(method), float(delta), float(temperature), float(e_min))
        en = np.full((G, ld), np.nan)
        H = np.full((G, ld, ld), np.nan) if return_hessian else None
        V = np.full((G, ld, ld), np.nan) if return_modes else None
        th, info = np.zeros((G, 3), np.float64), np.zeros((G, 4), np.int32)
        self._check(self._lib.vssr_batch_vibrations(self._h, C.byref(p), _ptr(m, C.c_double), _ptr(mask, C.c_uint8), _ptr(reps, C.c_int32), G, ld,
                                                    int(want), _ptr(en, C.c_double), _ptr(H, C.c_double), _ptr(V, C.c_double),
                                                    _ptr(th, C.c_double), _ptr(info, C.c_int32)))
        self.last_relax_counts = self.relax_counts()
        ms = info[:, 0]
        out = {"energies": [en[g, :ms[g]].copy() for g in range(G)], "energy": th[:, 0].copy(), "zpe": th[:, 1].copy(), "f_vib": th[:, 2].copy(),
               "m": ms.copy(), "n_imag": info[:, 1].copy(), "n_left_out": info[:, 2].copy(), "stop_reason": info[:, 3].copy()}
        if return_hessian:
            out["hessian"] = [H[g, :ms[g], :ms[g]].copy() for g in range(G)]
        if return_modes:
            out["modes"] = [V[g, :ms[g], :ms[g]].copy() for g in range(G)]
        return out

    # -- nudged elastic band --------------------------------------------------------------------------
    def neb(self, n_img, fixed=None, k=0.1, climb=False, method="improvedtangent", fmax=0.05, max_steps=100, params=None, want=WANT_ALL):
        """Relax the bands of the resident batch on the device (vssr_batch_neb): band g is ``n_img[g]`` >= 3 consecutive chains that
        differ in positions only; its first and last image never move.  ``k`` spring constant in eV / A^2, ``climb`` the climbing
        image, ``method`` ``"improvedtangent"`` / ``"aseneb"``, ``fmax`` in eV / A on the NEB force, FIRE over the whole band for at
        most ``max_steps`` steps (``params``: a ``NebParams`` instead of all of these).  Returns dict(positions [sum N, 3], energies
        [B], neb_forces [sum N, 3], fmax / barrier_forward / barrier_reverse [G] (E_max - E_first, E_max - E_last), n_steps /
        stop_reason (``NEB_STOP_REASONS``) / imax [G]); ``download()`` / ``results_f64()`` / ``stress()`` / ``vibrations()`` serve the
        final state at once."""
        N, B = self._n_atoms, self._n_cfg
        fx = _fixed_arg(fixed, N)
        imgs = np.ascontiguousarray(n_img, dtype=np.int32).reshape(-1)
        G = int(imgs.size)
        p = params or NebParams.default(max_steps, method, climb, k, fmax)
        pos, e, F = np.zeros((N, 3), np.float64), np.zeros(B, np.float64), np.zeros((N, 3), np.float64)
        band, info = np.zeros((max(G, 1), 3), np.float64), np.zeros((max(G, 1), 4), np.int32)
        self._check(self._lib.vssr_batch_neb(self._h, C.byref(p), _ptr(fx, C.c_uint8), _ptr(imgs, C.c_int32), G, int(want), _ptr(pos, C.c_double),
                                             _ptr(e, C.c_double), _ptr(F, C.c_double), _ptr(band, C.c_double), _ptr(info, C.c_int32)))
        self.last_relax_counts = self.relax_counts()
        return {"positions": pos, "energies": e, "neb_forces": F, "fmax": band[:G, 0].copy(), "barrier_forward": band[:G, 1].copy(),
                "barrier_reverse": band[:G, 2].copy(), "n_steps": info[:G, 0].copy(), "stop_reason": info[:G, 1].copy(),
                "imax": info[:G, 2].copy()}

    # -- dimer method ------------------------------------------------------------------------------------
    def dimer(self, fixed=None, modes=None, dimer_id=None, seed=0, max_steps=100, max_rot_first=8, max_rot=1, delta=0.01, phi_tol=np.pi / 180.0,
              fmax=0.05, displace=0.0, params=None, want=WANT_ALL, **fire):
        """Saddle searches from the resident batch on the device (vssr_batch_dimer): dimer g is chains 2 g (the midpoint) and 2 g + 1
        (the moving end, whose uploaded positions are ignored), equal in everything but positions.  ``modes`` [sum N, 3] laid out
        like the batch (the rows of the odd chains are not read) or None: standard normals keyed by (``seed``, ``dimer_id[g]``, atom,
        component), ``dimer_id`` defaulting to g.  ``delta`` in A, ``phi_tol`` in rad, ``fmax`` in eV / A on the midpoint force (with a
        negative curvature), ``displace`` in A along the mode before the first evaluation; ``max_rot_first`` / ``max_rot`` rotations
        before the first / every later of at most ``max_steps`` FIRE translations; ``fire``: ``dt``, ``maxstep``, ``dtmax``, ``finc``,
        ``fdec``, ``astart``, ``fa``, ``nmin`` of ASE's FIRE (``params``: a ``DimerParams`` instead of all of these).  Returns
        dict(positions [sum N, 3], energies [B], modes [sum N, 3] (zero on the odd chains), fmax / curvature / e0 / f_perp [G],
        n_steps / stop_reason (``DIMER_STOP_REASONS``) / n_rot / n_eval [G]); ``download()`` / ``results_f64()`` /
        ``stress()`` / ``vibrations()`` serve the final state at once."""
        N, B = self._n_atoms, self._n_cfg
        G = B // 2
        fx = _fixed_arg(fixed, N)
        m = None
        if modes is not None:
            m = np.ascontiguousarray(modes, dtype=np.float64)
            if m.size != 3 * N:
                raise ValueError("modes do not match the resident batch ([sum N, 3] wanted)")
        ids = None
        if dimer_id is not None:
            ids = np.ascontiguousarray(dimer_id, dtype=np.uint64).reshape(-1)
            if ids.size != G:
                raise ValueError(f"{ids.size} dimer ids for {G} dimers")
        p = params or DimerParams.default(max_steps, max_rot_first, max_rot, delta, phi_tol, fmax, displace, seed, **fire)
        pos, e, mode = np.zeros((N, 3), np.float64), np.zeros(B, np.float64), np.zeros((N, 3), np.float64)
        rec, info = np.zeros((max(G, 1), 4), np.float64), np.zeros((max(G, 1), 4), np.int32)
        self._check(self._lib.vssr_batch_dimer(self._h, C.byref(p), _ptr(fx, C.c_uint8), _ptr(m, C.c_double), _ptr(ids, C.c_uint64), int(want),
                                               _ptr(pos, C.c_double), _ptr(e, C.c_double), _ptr(mode, C.c_double), _ptr(rec, C.c_double),
                                               _ptr(info, C.c_int32)))
        self.last_relax_counts = self.relax_counts()
        return {"positions": pos, "energies": e, "modes": mode, "fmax": rec[:G, 0].copy(), "curvature": rec[:G, 1].copy(),
                "e0": rec[:G, 2].copy(), "f_perp": rec[:G, 3].copy(), "n_steps": info[:G, 0].copy(), "stop_reason": info[:G, 1].copy(),
                "n_rot": info[:G, 2].copy(), "n_eval": info[:G, 3].copy()}

    # -- variable-cell relaxation ------------------------------------------------------------------------
    def relax_cell(self, fixed=None, max_steps=100, fmax=0.05, scalar_pressure=0.0, mask=None, hydrostatic_strain=False, cell_factor=0.0,
                   params=None, want=WANT_ALL, **fire):
        """Atoms and cells of the resident batch relaxed together on the device (vssr_batch_relax_cell): ASE's ``UnitCellFilter`` under
        ASE's FIRE as tests/cellrelax_oracle.py restates them (not an executed ASE).  ``fixed`` [sum N]: atoms whose fractional
        coordinates stay; ``fmax`` in eV / A over the N + 3 rows (atoms and cell); ``scalar_pressure`` in eV / A^3; ``mask``: six 0 / 1
        in Voigt order xx yy zz yz xz xy (None: all free; a slab p p f along z takes 1 1 0 0 0 1); ``hydrostatic_strain``: the cell only
        scales; ``cell_factor`` <= 0: the atom count; ``fire``: ``dt``, ``maxstep``, ``dtmax``, ``finc``, ``fdec``, ``astart``, ``fa``,
        ``nmin`` (``params``: a ``CellRelaxParams`` instead of all of these).  Every kind but pair handles with k-space.  Returns
        dict(positions [sum N, 3], cells [B, 3, 3], n_steps / stop_reason (``CELL_STOP_REASONS``) [B], fmax / energy / volume [B] as of
        the last convergence test); ``download()`` / ``results_f64()`` / ``stress()`` serve the final state at once, and later
        ``set_positions`` / ``run`` keep the relaxed cells until the next upload."""
        N, B = self._n_atoms, self._n_cfg
        fx = _fixed_arg(fixed, N)
        p = params or CellRelaxParams.default(max_steps, fmax, scalar_pressure, mask, hydrostatic_strain, cell_factor, **fire)
        pos, cells, rec = np.zeros((N, 3), np.float64), np.zeros((max(B, 1), 3, 3), np.float64), np.zeros((max(B, 1), 3), np.float64)
        steps, reason = np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
        self._check(self._lib.vssr_batch_relax_cell(self._h, C.byref(p), _ptr(fx, C.c_uint8), int(want), _ptr(pos, C.c_double),
                                                    _ptr(cells, C.c_double), _ptr(steps, C.c_int32), _ptr(reason, C.c_int32),
                                                    _ptr(rec, C.c_double)))
        self.last_relax_counts = self.relax_counts()
        return {"positions": pos, "cells": cells[:B], "n_steps": steps[:B], "stop_reason": reason[:B], "fmax": rec[:B, 0].copy(),
                "energy": rec[:B, 1].copy(), "volume": rec[:B, 2].copy()}

    def get_cell(self):
        """The cells of the resident batch as the device holds them, [B, 3, 3] (vssr_batch_get_cell)."""
        cells = np.zeros((max(self._n_cfg, 1), 3, 3), np.float64)
        self._check(self._lib.vssr_batch_get_cell(self._h, _ptr(cells, C.c_double)))
        return cells[:self._n_cfg]

    def relax_counts(self):
        """``(lock-step evaluations, dispatched chain-evaluations)`` of the last relaxation (vssr_batch_relax_counts)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.vssr_batch_relax_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_capacity(self, slots_per_atom=0, tight=-1):
        """Test hook (vssr_debug_capacity); returns the regrow count of the last relaxation."""
        n = C.c_int32(0)
        self._check(self._lib.vssr_debug_capacity(self._h, int(slots_per_atom), int(tight), C.byref(n)))
        return n.value

    def _relax_call(self, fn, p, fixed, want, record_interval=0):
        N, B = self._n_atoms, self._n_cfg
        self._check(self._lib.vssr_batch_traj_configure(self._h, int(record_interval or 0)))
        fx = _fixed_arg(fixed, N)
        pos = np.zeros((N, 3), np.float64)
        steps = np.zeros(B, np.int32)
        conv = np.zeros(B, np.uint8)
        self._check(fn(self._h, C.byref(p), _ptr(fx, C.c_uint8), int(want), _ptr(pos, C.c_double),
                       _ptr(steps, C.c_int32), _ptr(conv, C.c_uint8)))
        out = {"positions": pos, "n_steps": steps, "converged": conv.astype(bool)}
        self.last_relax_counts = self.relax_counts()
        if record_interval:
            R = C.c_int32(0)
            self._check(self._lib.vssr_batch_traj_read(self._h, 0, None, None, None, None, C.byref(R)))
            R = R.value
            n_rec = np.zeros(B, np.int32)
            tpos, tf, te = np.zeros((R, N, 3), np.float64), np.zeros((R, N, 3), np.float32), np.zeros((R, B), np.float64)
            self._check(self._lib.vssr_batch_traj_read(self._h, R, _ptr(n_rec, C.c_int32), _ptr(tpos, C.c_double),
                                                       _ptr(tf, C.c_float), _ptr(te, C.c_double), None))
            self._check(self._lib.vssr_batch_traj_configure(self._h, 0))
            out["traj"] = {"n_records": n_rec, "positions": tpos, "forces": tf, "energies": te,
                           "record_interval": int(record_interval)}
        return out

    # -- introspection -----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self._lib.vssr_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._check(self._lib.vssr_profile_reset(self._h))

    def profile_read(self):
        cap = 32
        names = (C.c_char_p * cap)()
        launches = np.zeros(cap, np.int64)
        ms = np.zeros(cap, np.float64)
        n = C.c_int32(0)
        self._check(self._lib.vssr_profile_read(self._h, cap, names, _ptr(launches, C.c_int64),
                                                _ptr(ms, C.c_double), C.byref(n)))
        return {names[k].decode(): {"launches": int(launches[k]), "total_ms": float(ms[k])}
                for k in range(n.value)}

    def stats(self):
        a, e, s = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self._lib.vssr_batch_stats(self._h, C.byref(a), C.byref(e), C.byref(s)))
        return {"atoms": a.value, "edges": e.value, "slots": s.value}

    def neighbors(self):
        n = C.c_int64(0)
        self._check(self._lib.vssr_batch_neighbors(self._h, 0, None, None, None, None, C.byref(n)))
        E = n.value
        ei = np.zeros(E, np.int32); ej = np.zeros(E, np.int32)
        eS = np.zeros((E, 3), np.int32); er = np.zeros((E, 3), np.float32)
        self._check(self._lib.vssr_batch_neighbors(self._h, E, _ptr(ei, C.c_int32), _ptr(ej, C.c_int32),
                                                   _ptr(eS, C.c_int32), _ptr(er, C.c_float), C.byref(n)))
        return ei, ej, eS, er

    def debug_read(self, name, model=0):
        n = C.c_int64(0)
        self._check(self._lib.vssr_debug_read(self._h, name.encode(), model, None, 0, C.byref(n)))
        buf = np.zeros(n.value, np.float32)
        self._check(self._lib.vssr_debug_read(self._h, name.encode(), model, _ptr(buf, C.c_float), n.value,
                                              C.byref(n)))
        return buf


class PainnEngine(_Handle):
    """PaiNN-ensemble evaluator on one GPU (one handle = one HIP stream)."""

    has_device_results = True     # vssr_batch_device_results serves fp32 PaiNN handles (sharding.ShardedEnsemble's device path)

    def __init__(self, blobs, device=0, cutoff=5.0, model_units_per_ev=23.0605, offset_per_z=None,
                 offset_const=0.0, hparams=None):
        super().__init__()
        hp = {"feat_dim": 128, "n_rbf": 20, "num_conv": 3, "n_embed": 100, "readout_hidden": 64,
              "excl_vol": True, "V_ex_power": 12, "V_ex_sigma": 1.5}
        hp.update(hparams or {})
        self._blobs = [np.ascontiguousarray(b, dtype=np.float32) for b in blobs]
        if not self._blobs:
            raise ValueError("at least one model is required")
        M = len(self._blobs)
        ptrs = (C.POINTER(C.c_float) * M)(*[_ptr(b, C.c_float) for b in self._blobs])
        off = None
        if offset_per_z is not None:
            off = np.ascontiguousarray(offset_per_z, dtype=np.float64)
            if off.size != hp["n_embed"]:
                raise ValueError("offset_per_z must have n_embed entries")
        cfg = PainnConfig(
            C.sizeof(PainnConfig), int(device), M, ptrs, self._blobs[0].size, hp["feat_dim"], hp["n_rbf"],
            hp["num_conv"], hp["n_embed"], hp["readout_hidden"], float(cutoff), int(bool(hp["excl_vol"])),
            int(hp["V_ex_power"]), float(hp["V_ex_sigma"]), float(model_units_per_ev),
            _ptr(off, C.c_double), float(offset_const))
        rc = self._lib.vssr_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_create failed ({rc}): {msg.decode() if msg else '?'}")
        self.n_models = M
        self.cutoff = float(cutoff)


class _AnalyticEngine(_Handle):
    """Shared fp64 interface of the analytic potentials (Tersoff, EAM, Stillinger-Weber, pair): types instead of atomic numbers."""

    has_device_results = False    # fp64 results: sharding uses the host result path

    def relax_f64(self, structs, fixed=None, max_steps=100, fmax=0.01, optimizer="FIRE"):
        """Relax (types, positions, cell, pbc) structures with FIRE / BFGS; returns (energy [B], e_atom [N], forces [N,3],
        positions [N,3], n_steps [B], converged [B]) with fp64 energies/forces of the relaxed structures."""
        return self.relax_arrays_f64(*pack_batch(structs), fixed=fixed, max_steps=max_steps, fmax=fmax, optimizer=optimizer)

    def relax_arrays_f64(self, n_atoms, T, pos, cell, pbc, fixed=None, max_steps=100, fmax=0.01, optimizer="FIRE"):
        """``relax_f64`` on the ABI's packed arrays (no per-structure objects)."""
        self.upload_arrays(n_atoms, T, pos, cell, pbc)
        info = self.relax(optimizer, fixed=fixed, max_steps=max_steps, fmax=fmax,
                          want=WANT_ENERGY | WANT_FORCES | WANT_PER_ATOM)
        e, ea, f = self.evaluate_arrays_f64(n_atoms, T, info["positions"], cell, pbc)
        return e, ea, f, info["positions"], info["n_steps"], info["converged"]

    last_cg_driver = None         # "lockstep" / "resident": the driver the last relax_cg_f64 / relax_cg_arrays_f64 of this engine ran

    def relax_cg_f64(self, structs, fixed=None, max_iter=100, max_eval=10000, etol=1e-5, ftol=1e-5, dmax=0.1, rerun=True,
                     driver="auto"):
        """LAMMPS ``min_style cg`` / ``minimize etol ftol max_iter max_eval`` on the device (vssr_batch_relax_cg).  Returns
        (energy [B], e_atom [N], forces [N,3], positions [N,3], n_iter [B], n_eval [B], stop_reason [B]).  ``driver``:
        ``"lockstep"`` (one batch-wide evaluation per step), ``"resident"`` (one workgroup minimises one chain from start to stop:
        chains of <= 256 atoms, any other batch runs in lock step) or ``"auto"`` (the library's rule: chain-resident for small
        Tersoff batches); same results bit for bit, ``last_cg_driver`` says which one ran."""
        cg_driver_code(driver)
        return self.relax_cg_arrays_f64(*pack_batch(structs), fixed=fixed, max_iter=max_iter, max_eval=max_eval, etol=etol, ftol=ftol,
                                        dmax=dmax, rerun=rerun, driver=driver)

    def cg_driver(self, driver=None):
        """Set the handle's CG driver (``None``: leave it) and return the name of the one its last CG relaxation ran, ``None`` before
        the first (vssr_batch_relax_cg_driver)."""
        code = -1 if driver is None else cg_driver_code(driver)
        last = C.c_int32(0)
        self._check(self._lib.vssr_batch_relax_cg_driver(self._h, code, C.byref(last)))
        return CG_DRIVER_NAMES.get(last.value)

    def results_f64(self):
        """fp64 (energy [B], e_atom [N], forces [N,3]) of the resident batch as the last evaluation or relaxation left them on the
        device (vssr_batch_results_f64: no upload, no run)."""
        e, ea, f = np.zeros(self._n_cfg), np.zeros(self._n_atoms), np.zeros((self._n_atoms, 3))
        self._check(self._lib.vssr_batch_results_f64(self._h, _ptr(e, C.c_double), _ptr(ea, C.c_double), _ptr(f, C.c_double)))
        return e, ea, f

    def relax_cg_arrays_f64(self, n_atoms, T, pos, cell, pbc, fixed=None, max_iter=100, max_eval=10000, etol=1e-5, ftol=1e-5,
                            dmax=0.1, rerun=True, driver="auto"):
        """``relax_cg_f64`` on the ABI's packed arrays: the minimisation, then the static evaluation of the minimised geometries
        (the reference's ``run_lammps_opt`` followed by ``run_lammps_energy``).  ``dmax``: LAMMPS ``min_modify dmax``.
        ``rerun=False`` returns the results the minimiser left on the device instead (no second upload, no second run).
        ``driver``: see ``relax_cg_f64``."""
        code = cg_driver_code(driver)
        self.upload_arrays(n_atoms, T, pos, cell, pbc)
        self._check(self._lib.vssr_batch_relax_cg_driver(self._h, code, None))
        N, B = self._n_atoms, self._n_cfg
        fx = _fixed_arg(fixed, N)
        p = CgParams.default(max_iter, max_eval, etol, ftol, dmax)
        out = np.zeros((N, 3), np.float64)
        it, ev, why = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._check(self._lib.vssr_batch_relax_cg(self._h, C.byref(p), _ptr(fx, C.c_uint8),
                                                  WANT_ENERGY | WANT_FORCES | WANT_PER_ATOM, _ptr(out, C.c_double),
                                                  _ptr(it, C.c_int32), _ptr(ev, C.c_int32), _ptr(why, C.c_int32)))
        self.last_relax_counts = self.relax_counts()
        self.last_cg_driver = self.cg_driver()
        e, ea, f = self.evaluate_arrays_f64(n_atoms, T, out, cell, pbc) if rerun else self.results_f64()
        return e, ea, f, out, it, ev, why

    def evaluate_f64(self, structs, want=WANT_ENERGY | WANT_FORCES | WANT_PER_ATOM):
        """structs: list of (types, positions, cell, pbc). Returns fp64 energy [B], e_atom [N], forces [N,3]."""
        return self.evaluate_arrays_f64(*pack_batch(structs), want=want)

    def evaluate_arrays_f64(self, n_atoms, T, pos, cell, pbc, want=WANT_ENERGY | WANT_FORCES | WANT_PER_ATOM):
        """``evaluate_f64`` on the ABI's packed arrays."""
        n_atoms, T, pos, cell, pbc = _batch_arrays(n_atoms, T, pos, cell, pbc)
        B, N = len(n_atoms), len(T)
        e = np.zeros(B); ea = np.zeros(N); f = np.zeros((N, 3))
        self._check(self._lib.vssr_tersoff_eval_batch(
            self._h, B, _ptr(n_atoms, C.c_int32), _ptr(T, C.c_int32), _ptr(pos, C.c_double),
            _ptr(cell, C.c_double), _ptr(pbc, C.c_uint8), int(want), None, _ptr(e, C.c_double),
            _ptr(ea, C.c_double), _ptr(f, C.c_double)))
        self._set_resident(n_atoms)
        return e, ea, f


class TersoffEngine(_AnalyticEngine):
    """Tersoff evaluator (fp64 on device)."""

    def __init__(self, params, device=0, species=None):
        """``params``: array [nt, nt, nt, 14], or the TEXT of a LAMMPS tersoff file together with ``species`` (LAMMPS type
        order) -- then the file is parsed by the library (vssr_tersoff_create_from_text)."""
        super().__init__()
        if isinstance(params, (str, bytes)):
            if not species:
                raise ValueError("species (LAMMPS type order) are required with a potential text")
            text = params if isinstance(params, bytes) else params.encode()
            arr = (C.c_char_p * len(species))(*[s.encode() for s in species])
            self.n_types = len(species)
            rc = self._lib.vssr_tersoff_create_from_text(int(device), text, len(species), arr, C.byref(self._h))
            if rc != 0:
                msg = self._lib.vssr_last_error(None)
                raise BackendError(f"vssr_tersoff_create_from_text failed ({rc}): {msg.decode() if msg else '?'}")
            return
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 4 or params.shape[3] != 14 or not (params.shape[0] == params.shape[1] == params.shape[2]):
            raise ValueError("params must be [nt, nt, nt, 14]")
        self.n_types = params.shape[0]
        rc = self._lib.vssr_tersoff_create(int(device), self.n_types, _ptr(params, C.c_double), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_tersoff_create failed ({rc}): {msg.decode() if msg else '?'}")


class SWEngine(_AnalyticEngine):
    """Stillinger-Weber (LAMMPS ``pair_style sw``) evaluator, fp64 on device.  Relaxes with FIRE / BFGS and the lock-step CG driver
    (the chain-resident minimiser on request: ``relax_cg_f64(..., driver="resident")``)."""

    def __init__(self, params, device=0, species=None):
        """``params``: array [nt, nt, nt, 11] (LAMMPS columns eps sig a lambda gamma costheta0 A B p q tol), or the TEXT of a
        ``.sw`` file together with ``species`` (LAMMPS type order) -- then the file is parsed by the library
        (vssr_sw_create_from_text)."""
        super().__init__()
        if isinstance(params, (str, bytes)):
            if not species:
                raise ValueError("species (LAMMPS type order) are required with a potential text")
            text = params if isinstance(params, bytes) else params.encode()
            arr = (C.c_char_p * len(species))(*[s.encode() for s in species])
            self.n_types = len(species)
            rc = self._lib.vssr_sw_create_from_text(int(device), text, len(species), arr, C.byref(self._h))
            if rc != 0:
                msg = self._lib.vssr_last_error(None)
                raise BackendError(f"vssr_sw_create_from_text failed ({rc}): {msg.decode() if msg else '?'}")
            return
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 4 or params.shape[3] != 11 or not (params.shape[0] == params.shape[1] == params.shape[2]):
            raise ValueError("params must be [nt, nt, nt, 11]")
        self.n_types = params.shape[0]
        rc = self._lib.vssr_sw_create(int(device), self.n_types, _ptr(params, C.c_double), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_sw_create failed ({rc}): {msg.decode() if msg else '?'}")


class VashishtaEngine(_AnalyticEngine):
    """Vashishta (LAMMPS ``pair_style vashishta``) evaluator, fp64 on device.  Relaxes with FIRE / BFGS / BFGSLineSearch and the
    lock-step CG driver; the chain-resident minimiser does not serve this kind (``relax_cg_f64(..., driver="resident")`` runs in lock
    step, same results)."""

    def __init__(self, params, device=0, species=None):
        """``params``: array [nt, nt, nt, 14] (LAMMPS columns H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta), or the TEXT
        of a ``.vashishta`` file together with ``species`` (LAMMPS type order) -- then the file is parsed by the library
        (vssr_vashishta_create_from_text)."""
        super().__init__()
        if isinstance(params, (str, bytes)):
            if not species:
                raise ValueError("species (LAMMPS type order) are required with a potential text")
            text = params if isinstance(params, bytes) else params.encode()
            arr = (C.c_char_p * len(species))(*[s.encode() for s in species])
            self.n_types = len(species)
            rc = self._lib.vssr_vashishta_create_from_text(int(device), text, len(species), arr, C.byref(self._h))
            if rc != 0:
                msg = self._lib.vssr_last_error(None)
                raise BackendError(f"vssr_vashishta_create_from_text failed ({rc}): {msg.decode() if msg else '?'}")
            return
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 4 or params.shape[3] != 14 or not (params.shape[0] == params.shape[1] == params.shape[2]):
            raise ValueError("params must be [nt, nt, nt, 14]")
        self.n_types = params.shape[0]
        rc = self._lib.vssr_vashishta_create(int(device), self.n_types, _ptr(params, C.c_double), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_vashishta_create failed ({rc}): {msg.decode() if msg else '?'}")


class PairEngine(_AnalyticEngine):
    """Pair potentials with damped-shifted-force or Ewald Coulomb (LAMMPS ``pair_style lj/cut``, ``morse``, ``buck``, ``born``,
    ``coul/dsf``, ``coul/long`` + ``kspace_style ewald``, and ``hybrid`` / ``hybrid/overlay`` of them) evaluator, fp64 on device.
    Relaxes with FIRE / BFGS and the lock-step CG driver (a handle with k-space: always lock step)."""

    def __init__(self, terms, charges=None, n_types=None, device=0, kspace=None):
        """``terms``: a ``pair.PairModel`` (then ``charges`` / ``n_types`` / ``kspace`` come from it), or a list of ``(type_a, type_b,
        style, c, rc, shift)`` with 0-based types, a style code or name of ``pair.STYLES`` and up to five coefficients in LAMMPS
        order; ``charges``: per-type charges [n_types] (needed by coul/dsf and coul/long); ``kspace``: ``(g_ewald, k_cut)``,
        ``(g_ewald, k_cut, slab)`` or a ``pair.KSpace`` -- the Ewald sum behind the coul/long terms (vssr_pair_create_kspace; with a
        slab factor other than 0 vssr_pair_create_kspace_slab: chains with pbc (1, 1, 0), the dipole-corrected sum of kspace_modify slab)."""
        super().__init__()
        from . import pair as pair_io

        if isinstance(terms, pair_io.PairModel):
            terms, charges, n_types, kspace = terms.terms, terms.charges, terms.n_types, terms.kspace
        terms = list(terms)
        if n_types is None:
            raise ValueError("n_types is required with a plain term list")
        arr = (PairTerm * max(len(terms), 1))()
        for k, (a, b, style, c, rc, shift) in enumerate(terms):
            c = [float(x) for x in c]
            if len(c) > 5:
                raise ValueError("a pair term has at most five coefficients")
            arr[k] = PairTerm(int(a), int(b), int(pair_io.STYLES.get(style, style)), (C.c_double * 5)(*(c + [0.0] * (5 - len(c)))),
                              float(rc), int(shift))
        q = None
        if charges is not None:
            q = np.ascontiguousarray(charges, dtype=np.float64)
            if q.size != int(n_types):
                raise ValueError("charges must hold one value per type")
        self.n_types = int(n_types)
        self.kspace = kspace
        if kspace is None:
            name = "vssr_pair_create"
            rc = self._lib.vssr_pair_create(int(device), self.n_types, len(terms), arr, _ptr(q, C.c_double), C.byref(self._h))
        else:
            if hasattr(kspace, "g_ewald"):
                g, kc, slab = kspace.g_ewald, kspace.k_cut, getattr(kspace, "slab", 0.0)
            else:
                g, kc, slab = (*kspace, 0.0) if len(kspace) == 2 else kspace
            if slab != 0.0:   # (also a factor <= 1.0 or NaN, which that entry point refuses)
                name = "vssr_pair_create_kspace_slab"
                rc = self._lib.vssr_pair_create_kspace_slab(int(device), self.n_types, len(terms), arr, _ptr(q, C.c_double),
                                                            C.byref(KSpace(float(g), float(kc))), float(slab), C.byref(self._h))
            else:
                name = "vssr_pair_create_kspace"
                rc = self._lib.vssr_pair_create_kspace(int(device), self.n_types, len(terms), arr, _ptr(q, C.c_double),
                                                       C.byref(KSpace(float(g), float(kc))), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"{name} failed ({rc}): {msg.decode() if msg else '?'}")


class EAMEngine(_AnalyticEngine):
    """EAM evaluator, fp64 on device.  ``funcfl``: one funcfl element (every atom has type 0, vssr_eam_create), or an
    ``eam.EamTables`` of up to 8 types -- eam/alloy, eam/fs or mixed funcfl files (type = table index, vssr_eam_create_alloy);
    tables that carry ``u`` / ``w`` make an angular-dependent potential (pair_style adp, vssr_eam_create_adp: CG relaxations of
    such an engine always run in lock step)."""

    def __init__(self, funcfl, device=0):
        super().__init__()
        if hasattr(funcfl, "z2r"):
            self._create_typed(funcfl, device)
            return
        grid = EamGrid(int(funcfl.nrho), int(funcfl.nr), float(funcfl.drho), float(funcfl.dr), float(funcfl.cutoff))
        frho, zr, rhor = (np.ascontiguousarray(a, dtype=np.float64) for a in (funcfl.frho, funcfl.zr, funcfl.rhor))
        if frho.size != funcfl.nrho or zr.size != funcfl.nr or rhor.size != funcfl.nr:
            raise ValueError("EAM tables do not match their grid")
        self.n_types = 1
        rc = self._lib.vssr_eam_create(int(device), C.byref(grid), _ptr(frho, C.c_double), _ptr(zr, C.c_double),
                                       _ptr(rhor, C.c_double), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_eam_create failed ({rc}): {msg.decode() if msg else '?'}")

    def _create_typed(self, t, device):
        n = len(t.frho)
        grid = EamGrid(int(t.nrho), int(t.nr), float(t.drho), float(t.dr), float(t.cutoff))
        frho, rhor, z2r = (np.ascontiguousarray(a, dtype=np.float64) for a in (t.frho, t.rhor, t.z2r))
        if frho.size != n * t.nrho or rhor.size != (n * n if t.fs else n) * t.nr or z2r.size != n * (n + 1) // 2 * t.nr:
            raise ValueError("EAM tables do not match their grid / element count")
        self.n_types = n
        if getattr(t, "u", None) is not None or getattr(t, "w", None) is not None:
            return self._create_adp(t, device, n, grid, frho, rhor, z2r)
        rc = self._lib.vssr_eam_create_alloy(int(device), n, 1 if t.fs else 0, C.byref(grid), _ptr(frho, C.c_double),
                                             _ptr(rhor, C.c_double), _ptr(z2r, C.c_double), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_eam_create_alloy failed ({rc}): {msg.decode() if msg else '?'}")

    def _create_adp(self, t, device, n, grid, frho, rhor, z2r):
        if t.fs:
            raise ValueError("ADP tables take alloy densities (fs=False)")
        # (a missing table goes to the library as a null pointer: it refuses)
        u, w = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (t.u, t.w))
        if any(a is not None and a.size != z2r.size for a in (u, w)):
            raise ValueError("ADP tables u / w do not match their grid / element count")
        rc = self._lib.vssr_eam_create_adp(int(device), n, C.byref(grid), _ptr(frho, C.c_double), _ptr(rhor, C.c_double),
                                           _ptr(z2r, C.c_double), _ptr(u, C.c_double), _ptr(w, C.c_double), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_eam_create_adp failed ({rc}): {msg.decode() if msg else '?'}")


class GMMEngine(_Handle):
    """Gaussian-mixture negative log-likelihood of embedding rows on one GPU (vssr_gmm_*): fp64 throughout.

    ``means [K, D]``, ``prec_chol [K, D, D]`` (full precision Cholesky factors; other covariance types are expanded by
    ``uncertainty.full_precision_cholesky``), ``weights [K]``; ``log_2pi`` is the constant of the Gaussian normaliser (the
    reference's ``GMMUncertainty`` evaluates it in float32, ``uncertainty.LOG2PI_F32``)."""

    def __init__(self, means, prec_chol, weights, device=0, log_2pi=1.8378770351409912):
        super().__init__()
        self._means = np.ascontiguousarray(means, dtype=np.float64)
        if self._means.ndim != 2:
            raise ValueError("means must be [K, D]")
        K, D = self._means.shape
        self._prec = np.ascontiguousarray(prec_chol, dtype=np.float64)
        self._weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if self._prec.shape != (K, D, D) or self._weights.shape != (K,):
            raise ValueError(f"prec_chol must be [K, D, D] and weights [K] for means of shape {(K, D)}")
        cfg = GmmConfig(C.sizeof(GmmConfig), int(device), K, D, _ptr(self._means, C.c_double), _ptr(self._prec, C.c_double),
                        _ptr(self._weights, C.c_double), float(log_2pi))
        rc = self._lib.vssr_gmm_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_gmm_create failed ({rc}): {msg.decode() if msg else '?'}")
        self.n_components, self.dim, self.device = K, D, int(device)

    def score_rows(self, x, log_prob=False):
        """NLL [n] of rows ``x [n, D]`` (any float dtype; scored in fp64); with ``log_prob=True`` also logp_k [n, K]."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {x.shape}")
        n = x.shape[0]
        nll = np.zeros(n, np.float64)
        lp = np.zeros((n, self.n_components), np.float64) if log_prob else None
        self._check(self._lib.vssr_gmm_score_rows(self._h, n, _ptr(x, C.c_double), _ptr(nll, C.c_double), _ptr(lp, C.c_double)))
        return (nll, lp) if log_prob else nll

    def score_batch(self, painn_engine, model=0, rows="atoms", order="atomic"):
        """Score the resident embedding of ``painn_engine``'s last run (ensemble member ``model``) in place on the device.
        ``rows``: "atoms" (one row per atom) or "mean" (one mean row per structure).  Returns ``(nll_rows, system)``:
        ``nll_rows`` [sum N] or [B]; ``system`` [B], the TRUE per-structure reduction named by ``order`` (None for "atomic")."""
        if rows not in GMM_ROWS:
            raise ValueError(f"rows must be one of {sorted(GMM_ROWS)}, got {rows!r}")
        if order not in GMM_ORDERS:
            raise ValueError(f"order must be one of {sorted(GMM_ORDERS)}, got {order!r}")
        B, N = painn_engine._n_cfg, painn_engine._n_atoms
        nll = np.zeros(N if rows == "atoms" else B, np.float64)
        sysv = np.zeros(B, np.float64) if order != "atomic" else None
        self._check(self._lib.vssr_gmm_score_batch(self._h, painn_engine._h, int(model), GMM_ROWS[rows], GMM_ORDERS[order],
                                                   _ptr(nll, C.c_double), _ptr(sysv, C.c_double)))
        return nll, sysv

    @classmethod
    def _adopt(cls, handle, n_components, dim, device):
        """An engine around a scoring handle the library built itself (vssr_gmm_fit_scorer)."""
        self = cls.__new__(cls)
        _Handle.__init__(self)
        self._h = handle
        self._means = self._prec = self._weights = None
        self.n_components, self.dim, self.device = int(n_components), int(dim), int(device)
        return self


def gmm_cov_shape(covariance_type, K, D):
    """sklearn's shape of covariances_ / precisions_cholesky_ for a covariance type."""
    return {"full": (K, D, D), "tied": (D, D), "diag": (K, D), "spherical": (K,)}[covariance_type]


class GMMFitEngine(_Handle):
    """Expectation-maximisation fit of a Gaussian mixture on one GPU (vssr_gmm_fit_*, ``csrc/gmm_fit.hip``): fp64 throughout,
    no floating-point atomics (a fit repeats bit for bit).

    The loop is sklearn's ``BaseMixture.fit`` (``tol`` on the change of the lower bound, ``max_iter``, ``n_init`` restarts keeping
    the best lower bound).  ``init``: "given" (``set_init``: labels, or means + weights + precisions), "kmeans" (k-means++ seeding
    and Lloyd iterations on the device) or "random_from_data".  Random draws come from Philox4x32-10 keyed by ``seed``: they
    do not reproduce numpy's or sklearn's streams.  Rows are appended from the host (``append_rows``) or taken device to device
    from a ``PainnEngine``'s resident embedding (``append_batch``).  The device is first touched by the first append or fit."""

    def __init__(self, n_components, dim, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init="given",
                 seed=0, device=0):
        super().__init__()
        if covariance_type not in GMM_COV_TYPES:
            raise ValueError(f"covariance_type must be one of {sorted(GMM_COV_TYPES)}, got {covariance_type!r}")
        if init not in GMM_INITS:
            raise ValueError(f"init must be one of {sorted(GMM_INITS)}, got {init!r}")
        cfg = GmmFitConfig(C.sizeof(GmmFitConfig), int(device), int(n_components), int(dim), GMM_COV_TYPES[covariance_type],
                           int(max_iter), int(n_init), GMM_INITS[init], float(tol), float(reg_covar), int(seed) & (2 ** 64 - 1))
        rc = self._lib.vssr_gmm_fit_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_gmm_fit_create failed ({rc}): {msg.decode() if msg else '?'}")
        self.n_components, self.dim, self.device = int(n_components), int(dim), int(device)
        self.covariance_type, self.max_iter = covariance_type, int(max_iter)
        self.n_rows = 0

    def append_rows(self, x):
        """Append rows ``x [n, D]`` (any float dtype; kept in fp64 on the device)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {x.shape}")
        self._check(self._lib.vssr_gmm_fit_append_rows(self._h, x.shape[0], _ptr(x, C.c_double)))
        self.n_rows += x.shape[0]

    def append_batch(self, painn_engine, model=0, rows="atoms"):
        """Append the resident embedding of ``painn_engine``'s last run (ensemble member ``model``), device to device:
        ``rows="atoms"`` one row per atom, ``"mean"`` one mean row per structure."""
        if rows not in GMM_ROWS:
            raise ValueError(f"rows must be one of {sorted(GMM_ROWS)}, got {rows!r}")
        self._check(self._lib.vssr_gmm_fit_append_batch(self._h, painn_engine._h, int(model), GMM_ROWS[rows]))
        self.n_rows += painn_engine._n_atoms if rows == "atoms" else painn_engine._n_cfg

    def clear(self):
        self._check(self._lib.vssr_gmm_fit_clear(self._h))
        self.n_rows = 0

    def set_init(self, means=None, weights=None, precisions=None, labels=None):
        """Starting values (each optional; a call replaces all four): ``means [K, D]``, ``weights [K]``, ``precisions`` (precision
        MATRICES in sklearn's shape for the covariance type), ``labels [N]`` in -1 .. K-1 for the resident rows."""
        K, D = self.n_components, self.dim
        conv = lambda a, shape: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
        m, w = conv(means, (K, D)), conv(weights, (K,))
        p = conv(precisions, gmm_cov_shape(self.covariance_type, K, D))
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
            if lab.shape[0] != self.n_rows:
                raise ValueError(f"{lab.shape[0]} labels for {self.n_rows} resident rows")
        self._check(self._lib.vssr_gmm_fit_set_init(self._h, _ptr(m, C.c_double), _ptr(w, C.c_double), _ptr(p, C.c_double),
                                                    _ptr(lab, C.c_int32)))

    def fit(self):
        """Run the fit; returns ``{"n_iter", "converged", "lower_bound", "best_init", "lower_bounds"}``.  A collapsed component
        raises ``ValueError`` with the reference's message."""
        trace = np.zeros(self.max_iter, np.float64)
        res = GmmFitResult(0, 0, 0, 0, 0.0, _ptr(trace, C.c_double), self.max_iter)
        rc = self._lib.vssr_gmm_fit_run(self._h, C.byref(res))
        if rc != 0:
            msg = (self._lib.vssr_last_error(self._h) or b"?").decode()
            if GMM_ILL_DEFINED in msg:
                raise ValueError(msg)
            raise BackendError(f"vssr error {rc}: {msg}")
        return {"n_iter": int(res.n_iter), "converged": bool(res.converged), "lower_bound": float(res.lower_bound),
                "best_init": int(res.best_init), "lower_bounds": trace[:res.n_lower_bounds].copy()}

    def params(self):
        """``{"weights_", "means_", "covariances_", "precisions_cholesky_"}`` in sklearn's shapes."""
        K, D = self.n_components, self.dim
        shape = gmm_cov_shape(self.covariance_type, K, D)
        w, m, cov, pc = np.zeros(K), np.zeros((K, D)), np.zeros(shape), np.zeros(shape)
        self._check(self._lib.vssr_gmm_fit_params(self._h, _ptr(w, C.c_double), _ptr(m, C.c_double), _ptr(cov, C.c_double),
                                                  _ptr(pc, C.c_double)))
        return {"weights_": w, "means_": m, "covariances_": cov, "precisions_cholesky_": pc}

    def scorer(self, log_2pi=1.8378770351409912):
        """A ``GMMEngine`` of the fitted mixture on the same GPU, built from the device arrays."""
        h = C.c_void_p(None)
        self._check(self._lib.vssr_gmm_fit_scorer(self._h, float(log_2pi), C.byref(h)))
        return GMMEngine._adopt(h, self.n_components, self.dim, self.device)


class ClusterEngine(_Handle):
    """Clustering of latent embeddings on one GPU (vssr_cluster_*, ``csrc/cluster.hip``): the PCA of the reference's
    ``perform_clustering`` (``sklearn.decomposition.PCA(n_components, whiten)``) and Ward linkage of the leading ``cluster_dims``
    projected columns without a distance matrix, fp64 throughout, no floating-point atomics (a run repeats bit for bit).

    Rows are appended from the host (``append_rows``) or device to device from a ``PainnEngine``'s last run, one mean row per
    structure (``append_resident``); several appends accumulate.  ``set_points`` skips the PCA (``get_cluster_centers``).  The tree
    comes back as scipy's ``Z``; cutting it is ``clustering.fcluster``.  The device is first touched by the first append."""

    def __init__(self, dim, n_components=32, whiten=True, cluster_dims=3, device=0):
        super().__init__()
        cfg = ClusterConfig(C.sizeof(ClusterConfig), int(device), int(dim), int(n_components), int(bool(whiten)), int(cluster_dims))
        rc = self._lib.vssr_cluster_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self._lib.vssr_last_error(None)
            raise BackendError(f"vssr_cluster_create failed ({rc}): {msg.decode() if msg else '?'}")
        self.dim, self.n_components, self.cluster_dims, self.device = int(dim), int(n_components), int(cluster_dims), int(device)
        self.n_rows = 0
        self.n_points = 0

    def append_rows(self, x):
        """Append rows ``x [n, D]`` (any float dtype; kept in fp64 on the device)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {x.shape}")
        self._check(self._lib.vssr_cluster_append_rows(self._h, x.shape[0], _ptr(x, C.c_double)))
        self.n_rows += x.shape[0]

    def append_resident(self, painn_engine, model=0):
        """Append one mean row per structure of ``painn_engine``'s last run (ensemble member ``model``), device to device."""
        self._check(self._lib.vssr_cluster_append_batch(self._h, painn_engine._h, int(model)))
        self.n_rows += painn_engine._n_cfg

    def clear(self):
        self._check(self._lib.vssr_cluster_clear(self._h))
        self.n_rows = 0
        self.n_points = 0

    def pca(self):
        """Fit the PCA on the resident rows and project them; returns ``{"n_rows", "n_sweeps", "converged"}``."""
        res = ClusterPcaResult(0, 0, 0)
        self._check(self._lib.vssr_cluster_pca(self._h, C.byref(res)))
        self.n_points = int(res.n_rows)
        return {"n_rows": int(res.n_rows), "n_sweeps": int(res.n_sweeps), "converged": bool(res.converged)}

    def pca_params(self):
        """``{"mean_", "components_", "explained_variance_", "explained_variance_ratio_"}`` in sklearn's shapes."""
        D, nc = self.dim, self.n_components
        mean, comp, ev, ratio = np.zeros(D), np.zeros((nc, D)), np.zeros(nc), np.zeros(nc)
        self._check(self._lib.vssr_cluster_pca_params(self._h, _ptr(mean, C.c_double), _ptr(comp, C.c_double), _ptr(ev, C.c_double),
                                                      _ptr(ratio, C.c_double)))
        return {"mean_": mean, "components_": comp, "explained_variance_": ev, "explained_variance_ratio_": ratio}

    def projected(self, first=0, n_rows=None):
        """Rows ``first .. first + n_rows`` of ``X_r`` as ``[n_rows, n_components]``."""
        n_rows = self.n_points - first if n_rows is None else int(n_rows)
        xr = np.zeros((max(n_rows, 0), self.n_components))
        self._check(self._lib.vssr_cluster_projected(self._h, int(first), n_rows, _ptr(xr, C.c_double)))
        return xr

    def set_points(self, points):
        """Cluster ``points [n, cluster_dims]`` directly (no PCA)."""
        p = np.ascontiguousarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.cluster_dims:
            raise ValueError(f"points must be [n, {self.cluster_dims}], got {p.shape}")
        self._check(self._lib.vssr_cluster_set_points(self._h, p.shape[0], _ptr(p, C.c_double)))
        self.n_points = p.shape[0]

    def linkage(self):
        """Ward linkage of the resident points: ``(Z [n - 1, 4], rounds)``, ``Z`` in scipy's convention."""
        Z = np.zeros((max(self.n_points - 1, 1), 4))
        rounds = C.c_int32(0)
        self._check(self._lib.vssr_cluster_linkage(self._h, _ptr(Z, C.c_double), C.byref(rounds)))
        return Z[: self.n_points - 1], int(rounds.value)
