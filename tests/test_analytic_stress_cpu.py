"""The checker of the analytic potentials' device stress (tests/strain_fd.py) pinned on the host, and the host surface of the
calculators.  No executed LAMMPS is compared anywhere: the stress is checked as the strain derivative of the project's own CPU
restatements (here tests/sw_oracle.py)."""
import inspect

import numpy as np

import cell_cases as cc
import strain_fd as sf
import sw_oracle as so
from surface_sampling_amd import calculators as calcs

PBC = np.ones(3, np.uint8)


def _sw_energy(P, T):
    return lambda X, Cl: so.sw(P, T, X, Cl, PBC)[0]


def test_sw_silicon_is_stress_free_at_a0_and_has_the_published_c11_c12():
    """Known answers of the 1985 silicon set through fd_stress: |sigma| < 1e-6 eV / A^3 at a0 = 5.430950 A, and the derivative of
    sigma with respect to an xx strain of +-1e-3 gives C11 = 151.4 and C12 = 76.4 GPa to the printed digit (README)."""
    P = so.si_params()
    T, X, Cl = so.diamond_si(so.SI_A0)
    energy = _sw_energy(P, T)
    s0 = sf.fd_stress(energy, X, Cl)
    print("sigma(a0) =", s0.sigma, "eV/A^3, unc", s0.unc, "eV")
    assert np.abs(s0.sigma).max() < 1e-6
    d = 1e-3
    sp, sm = (sf.fd_stress(energy, *sf.strained((X, Cl), sf.voigt_strain(0, e))) for e in (d, -d))
    C = (sp.sigma - sm.sigma) / (2 * d) * so.EV_A3_GPA
    print(f"C11 = {C[0]:.3f} GPa, C12 = {C[1]:.3f} / {C[2]:.3f} GPa")
    assert f"{C[0]:.1f}" == "151.4" and f"{C[1]:.1f}" == "76.4" and f"{C[2]:.1f}" == "76.4"
    assert np.abs(C[3:]).max() < 1e-3


def test_fd_stress_is_rotation_covariant():
    """fd_stress of a configuration rotated by a fixed R (positions and cell) = R sigma R^T of the unrotated one, within the two
    uncertainties."""
    P = so.si_params()
    T, X, Cl, _ = so.dense_box(n=40, box=8.4, seed=5)
    energy = _sw_energy(P, T)
    R = cc.rotation(7)
    a = sf.fd_stress(energy, X, Cl)
    b = sf.fd_stress(energy, X @ R.T, Cl @ R.T)
    want = sf.rotated_voigt(a.virial, R)
    # the uncertainty of a rotated tensor: every component mixes all six (|R| entries <= 1, shear components count twice)
    bound = b.unc + 2.0 * a.unc.sum()
    for k in range(6):
        print(f"voigt {k}: rotated {b.virial[k]:+.9e}  R sigma R^T {want[k]:+.9e}  bound {bound[k]:.2e} eV")
    assert np.abs(a.virial).max() > 1.0                      # a stressed configuration, not a trivial zero
    assert (np.abs(b.virial - want) <= bound).all()
    assert abs(a.volume - b.volume) <= 1e-9 * a.volume


def test_the_analytic_calculators_advertise_stress_and_keep_their_default_call():
    for cls in (calcs.TersoffSurfCalc, calcs.SWSurfCalc, calcs.EAMSurfCalc, calcs.LAMMPSSurfCalc):
        assert "stress" in cls.implemented_properties, cls.__name__
    assert calcs.LAMMPSRunSurfCalc is calcs.EAMSurfCalc
    assert "energies" in calcs.EAMSurfCalc.implemented_properties and "free_energy" in calcs.EAMSurfCalc.implemented_properties
    # a calculate() without ``properties`` asks for what it asked for before: no stress kernel, no new keys
    default = ("energy", "relaxed_energy", "forces", "per_atom_energies", "surface_energy")
    for cls in (calcs._AnalyticSurfCalc, calcs.TersoffSurfCalc, calcs.SWSurfCalc, calcs.EAMSurfCalc, calcs.LAMMPSSurfCalc):
        assert inspect.signature(cls.calculate).parameters["properties"].default == default, cls.__name__
