#!/usr/bin/env python3
"""Device harmonic vibrations against the host path, wall time per call (one JSON line per measurement).

  (a) one 192-atom Cu(100) slab (EAM alloy tables, 8 Au atoms in the top layer = the vib atoms, m = 24) at 1 / 8 / 24 replicas;
  (b) 256 PaiNN chains of the bench batch (bench.py's chains) with 2 vib atoms each (the two topmost atoms);
  (c) the same work through the host path in the same run: one ``evaluate`` per displacement (the single structure for (a), the
      whole batch with every chain displaced in the same degree of freedom for (b)), numpy row assembly, ``numpy.linalg.eigh``.

Every timed window covers whole calls (upload included for the device path: ``vibrations`` needs the replicas resident).

    python tools/bench_vib.py [--reps 3] [--painn-chains 256] [--replicas 1,8,24]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))   # (the restatements under tests/ import the oracle's spline helpers)

KS = (-1, 1)


def host_vibrations(evaluate_forces, pos, start, vib_idx, mass, delta=0.01):
    """ASE's procedure on the host for a batch of equally masked chains: per degree of freedom two evaluations of the whole batch,
    rows, H + H^T, eigh.  ``vib_idx``: per chain the (chain-local) vib atoms, the same count everywhere."""
    import vib_oracle as vo

    B, nv = len(start) - 1, len(vib_idx[0])
    K = np.zeros((B, 3 * nv, 3 * nv))
    sel = [start[b] + np.asarray(vib_idx[b]) for b in range(B)]
    for v in range(nv):
        for c in range(3):
            F = []
            for k in KS:
                p = pos.copy()
                for b in range(B):
                    p[sel[b][v], c] = p[sel[b][v], c] + k * delta
                F.append(evaluate_forces(p))
            row = 0.5 * (F[0] - F[1]) / (2 * delta)
            for b in range(B):
                K[b, 3 * v + c] = row[sel[b]].ravel()
    out = []
    for b in range(B):
        e, _ = vo.modes(K[b] + K[b].T, mass[sel[b]])
        out.append(e)
    return out


def bench_eam(replicas, reps):
    import cg_resident_cases as rc
    import eam_alloy_oracle as ao
    from surface_sampling_amd import backend

    pos, cell, pbc = ao.cu100_slab(4, 4, 6)
    assert len(pos) == 192
    top = np.flatnonzero(pos[:, 2] > pos[:, 2].max() - 0.1)
    vib_idx = top[::4][:8]
    T = np.zeros(192, np.int32)
    T[vib_idx] = 1
    pos = pos + np.random.default_rng(0).normal(0, 0.02, pos.shape)
    mass = np.where(T == 1, 196.966569, 63.546)
    struct = (T, pos, cell, pbc)
    mask = np.zeros(192, np.uint8)
    mask[vib_idx] = 1
    eng = backend.EAMEngine(rc.eam_tables("eam_alloy"), device=0)
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    n_atoms, Tt, _, cl, pb = backend.pack_batch([struct])

    t_host, e_host = np.inf, None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        e_host = host_vibrations(lambda p: eng.evaluate_arrays_f64(n_atoms, Tt, p, cl, pb)[2], pos, [0, 192], [vib_idx], mass)[0]
        if rep:
            t_host = min(t_host, time.perf_counter() - t0)
    for n in replicas:
        best, out = np.inf, None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            eng.upload([struct] * n)
            out = eng.vibrations(np.tile(mass, n), vib=np.tile(mask, n), n_rep=[n], want=want)
            if rep:
                best = min(best, time.perf_counter() - t0)
        dev = float(np.abs(out["energies"][0] - e_host).max())
        print(json.dumps({"bench": "vib_eam_cu100_192", "vib_atoms": 8, "m": 24, "replicas": n, "reps": reps,
                          "lockstep_evaluations": int(eng.last_relax_counts[0]), "device_ms_per_call": round(1e3 * best, 3),
                          "host_ms_per_call": round(1e3 * t_host, 3), "host_over_device": round(t_host / best, 2),
                          "max_abs_energy_difference_eV": dev, "top_mode_eV": float(out["energies"][0][-1])}), flush=True)
    eng.close()


def bench_painn(n_chains, reps):
    import bench
    from surface_sampling_amd import backend, structures

    blobs, S, _ = bench.load_golden()
    slabs = bench.build_chains(S, 0, n_chains)
    packs = [structures.as_arrays(s) for s in slabs]
    mass = np.concatenate([structures.masses_of(s) for s in slabs])
    start = np.concatenate([[0], np.cumsum([len(s) for s in slabs])])
    vib_idx = [np.sort(np.argsort(-s.positions[:, 2], kind="stable")[:2]) for s in slabs]
    mask = np.zeros(len(mass), np.uint8)
    for b, ix in enumerate(vib_idx):
        mask[start[b] + ix] = 1
    eng = backend.PainnEngine(blobs, device=0)
    n_atoms, Z, pos, cell, pbc = backend.pack_batch(packs)

    def forces(p):
        eng.upload_arrays(n_atoms, Z, p, cell, pbc)
        eng.run(backend.WANT_ENERGY | backend.WANT_FORCES)
        return eng.download(backend.WANT_ENERGY | backend.WANT_FORCES)["forces"].astype(np.float64)

    t_host = t_dev = np.inf
    e_host = out = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        e_host = host_vibrations(forces, pos, start, vib_idx, mass)
        t1 = time.perf_counter()
        eng.upload(packs)
        out = eng.vibrations(mass, vib=mask, want=backend.WANT_ENERGY | backend.WANT_FORCES)
        t2 = time.perf_counter()
        if rep:
            t_host, t_dev = min(t_host, t1 - t0), min(t_dev, t2 - t1)
    # fp32 forces: compare the eigenvalues of D H D, where the noise of the near-zero modes is not magnified by a square root
    s2 = backend.VIB_ENERGY_UNIT ** 2
    dev = max(float(np.abs(np.sign(a) * a * a - np.sign(b) * b * b).max()) / s2 for a, b in zip(out["energies"], e_host))
    print(json.dumps({"bench": "vib_painn_bench_batch", "chains": n_chains, "atoms": int(len(mass)), "vib_atoms_per_chain": 2, "m": 6,
                      "reps": reps, "lockstep_evaluations": int(eng.last_relax_counts[0]), "device_ms_per_call": round(1e3 * t_dev, 3),
                      "host_ms_per_call": round(1e3 * t_host, 3), "host_over_device": round(t_host / t_dev, 2),
                      "max_abs_eigenvalue_difference": dev, "stop_reasons": sorted(set(int(r) for r in out["stop_reason"]))}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replicas", default="1,8,24")
    ap.add_argument("--painn-chains", type=int, default=256, help="0: skip the PaiNN part")
    a = ap.parse_args()
    bench_eam([int(c) for c in a.replicas.split(",") if c], a.reps)
    if a.painn_chains:
        bench_painn(a.painn_chains, a.reps)


if __name__ == "__main__":
    main()
