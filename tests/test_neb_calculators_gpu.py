"""``neb_batch`` of the calculators on the device: the physics anchor through ``PairSurfCalc`` (tuples, two stages), and a Cu adatom
hopping between neighbouring hollow sites of Cu(100) through ``EAMSurfCalc``."""
import os

import numpy as np
import pytest

import eam_alloy_oracle as ao
import neb_cases as nc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _atoms(struct, z):
    from surface_sampling_amd import structures

    T, X, cell, pbc = struct
    return structures.Structure(np.full(len(T), z), X, cell, np.asarray(pbc).astype(bool))


def _bound(fmax, H):
    lam = np.linalg.eigvalsh(0.5 * (H + H.T))
    return 2.0 * fmax * fmax / (2.0 * np.abs(lam).min()), lam


def test_pair_calculator_reproduces_the_anchor_through_tuples_and_two_stages():
    from surface_sampling_amd.calculators import PairSurfCalc

    calc = PairSurfCalc(commands=["pair_style lj/cut 8.0", f"pair_coeff * * {nc.ANCHOR_EPS} {nc.ANCHOR_SIGMA}"], species=["Ar"], device="cuda:0")
    a, b = (_atoms(nc.anchor_image(0.0, 0.0, z), 18) for z in (-nc.ANCHOR_ZMIN, nc.ANCHOR_ZMIN))
    held = [0, 1, 2]
    bound = nc.barrier_bound(nc.ANCHOR["fmax"], nc.anchor_saddle_hessian())
    plain, staged = calc.neb_batch([(a, b, 6), (a, b, 6)], fixed_indices=[held, held], k=0.1, fmax=nc.ANCHOR["fmax"], steps=100)[0], None
    staged = calc.neb_batch([(a, b, 6), (a, b, 7)], fixed_indices=[held, held], k=0.1, fmax=nc.ANCHOR["fmax"], steps=100, two_stage=True)
    miss = nc.ANCHOR_BARRIER - plain["barrier_forward"]
    print(f"6 images, no climbing: {plain['n_steps']} steps, misses the barrier by {miss:.4f} eV")
    assert plain["converged"] and miss > 0.1
    for r, n in zip(staged, (6, 7)):
        err = r["barrier_forward"] - nc.ANCHOR_BARRIER
        print(f"{n} images, two stages: {r['n_steps']} steps, barrier error {err:+.3e} eV (bound {bound:.3e}), imax {r['imax']}")
        assert r["converged"] and r["stop_reason"] == 1 and abs(err) <= bound and abs(r["barrier_forward"] - r["barrier_reverse"]) < 1e-9
        assert r["images"].shape == (n, 4, 3) and r["energies"].shape == (n,) and r["path"].shape == (n,) and r["path"][0] == 0.0
        assert np.all(np.diff(r["path"]) > 0) and abs(r["path"][-1] - 2 * nc.ANCHOR_ZMIN) < 0.05
        assert np.array_equal(r["images"][0], a.positions) and np.array_equal(r["images"][-1], b.positions)
        assert np.array_equal(r["images"][:, :3], np.broadcast_to(a.positions[:3], (n, 3, 3)))
        assert r["energies"][r["imax"]] - r["energies"][0] == r["barrier_forward"]
    with pytest.raises(ValueError):
        calc.neb_batch([(a, b, 2)])
    # the calculator's other entry points are as they were
    e = calc.calculate_batch([a])[0]["energy"]
    assert np.isfinite(e)


def test_eam_calculator_cu_adatom_hop_on_cu100():
    """A Cu adatom between neighbouring fourfold hollows of a 3 x 3 Cu(100) slab of three layers (bottom layer held), 7 images with the
    climbing image.  Both hollows are equivalent: forward and reverse barriers agree within 2 fmax^2 / (2 min |lambda|) with lambda from
    the device's own Hessian of the adatom at the climbing image; the barrier is positive and the middle image is the highest.  The
    barrier itself is recorded (profiles/r31/NOTES_neb.md), not pinned."""
    from surface_sampling_amd import structures
    from surface_sampling_amd.calculators import EAMSurfCalc

    a = 3.615
    pos, cell, pbc = ao.cu100_slab(3, 3, 3, a=a)
    top = pos[:, 2].max()
    sites = [np.array([1.5 * a, 1.0 * a, top + 0.45 * a]), np.array([1.0 * a, 1.5 * a, top + 0.45 * a])]
    ends = [structures.Structure(np.full(len(pos) + 1, 29), np.vstack([pos, s]), cell, np.asarray(pbc).astype(bool)) for s in sites]
    held = np.flatnonzero(pos[:, 2] < 0.5)
    ad = len(pos)
    calc = EAMSurfCalc(files=[os.path.join(GOLDEN, "Cu_u3.eam")], device="cuda:0")
    relaxed = calc.relax_batch(ends, fixed_indices=[held, held], relax_steps=400, fmax=1e-3, optimizer="FIRE")
    ends = [r[0] for r in relaxed]
    fmax = 0.01
    r = calc.neb_batch([(ends[0], ends[1], 7)], fixed_indices=[held], k=0.1, climb=True, fmax=fmax, steps=400)[0]
    saddle = ends[0].copy()
    saddle.set_positions(r["images"][r["imax"]])
    vib = calc.vibrations_batch([saddle], indices=[ad], return_hessian=True, replicas=1)[0]
    bound, lam = _bound(fmax, vib["hessian"])
    print(f"Cu adatom hop on Cu(100), Cu_u3 funcfl: forward {r['barrier_forward']:.6f} eV, reverse {r['barrier_reverse']:.6f} eV, "
          f"{r['n_steps']} steps, stop {r['stop_reason']}, fmax {r['fmax']:.4f}, imax {r['imax']}, adatom Hessian eigenvalues {lam}, "
          f"bound {bound:.3e} eV, path {r['path'][-1]:.3f} A")
    assert r["converged"] and r["imax"] == 3
    assert r["barrier_forward"] > 0.0 and r["barrier_reverse"] > 0.0
    assert abs(r["barrier_forward"] - r["barrier_reverse"]) <= bound
    assert vib["n_imag"] == 1
    assert np.array_equal(r["images"][:, held], np.broadcast_to(ends[0].positions[held], (7, len(held), 3)))
    assert np.array_equal(r["images"][0], ends[0].positions)
