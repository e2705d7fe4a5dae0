"""Secondary measurement (not the BASELINE metric): Ewald sums on pair handles (ewald.hip), fp64 on one GPU, against the same model with
the damped-shifted-force Coulomb sum at the same real-space cutoff (the capability before the Ewald sum, and the yardstick).

Workload: the 8-atom rocksalt cell tiled 3 x 3 x 3 (216 atoms) under 15 A of vacuum, periodic in all three directions, every chain
rattled by its own seed, Born-Mayer-Huggins-like short-range terms (tools/bench_pair.py):
  * ewald   pair_style born/coul/long RC + kspace_style ewald A, for every A of --accuracy;
  * dsf     pair_style hybrid/overlay born RC coul/dsf 0.2 RC.
Per chain count: single-point evaluations/s of the resident batch (vssr_batch_run + synchronize) and of the whole call, and with
--relax-steps n > 0 lock-step CG relaxations/s (<= n iterations, lower half held); every Ewald line carries the DSF / Ewald ratio
of the same figure.  One JSON line per measurement.

The k-space share of an evaluation comes from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o ew -- python tools/bench_ewald.py --chains 1024 --accuracy 1e-8 --no-dsf --relax-steps 0
    python tools/bench_ewald.py --stats OUT/ew_results.db
prints the share of the k_ewald_* kernels in the total kernel time of that run, from the dispatch table of the rocpd database
rocprofv3 writes.
--slab F measures the slab handle instead (kspace_modify slab F, the same slabs with pbc 1 1 0) against the 3-D handle on the same atoms
in a fully periodic cell with c multiplied by F: the same k box, so the same reciprocal work, and the same real-space pairs (the vacuum
exceeds the cutoff).  Per (chains, accuracy): resident evaluations/s of both, the slab / 3-D ratio, the 3-D figure of --repeats
independent measurements (fresh handle each, the two handles alternating) with their spread, and the per-kernel times of one profiled run of each handle.
Usage: python tools/bench_ewald.py [--chains 256,1024,4096] [--accuracy 1e-5,1e-8] [--rc 10.0] [--reps 5] [--relax-steps 20] [--no-dsf]
                                   [--slab 3.0 [--repeats 5]]"""
import argparse, json, os, sqlite3, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BORN = ["0.2637 0.317 2.340 1.0486 -0.4993", "0.2110 0.317 2.755 6.9906 -8.6758", "0.1582 0.317 3.170 72.4022 -145.4285"]
CHARGES = ["set type 1 charge 1.0", "set type 2 charge -1.0"]


def ewald_lines(rc, accuracy):
    return [f"pair_style born/coul/long {rc}", *(f"pair_coeff {ij} {c}" for ij, c in zip(("1 1", "1 2", "2 2"), BORN)),
            f"kspace_style ewald {accuracy}", *CHARGES]


def dsf_lines(rc):
    return [f"pair_style hybrid/overlay born {rc} coul/dsf 0.2 {rc}", *(f"pair_coeff {ij} born {c}" for ij, c in zip(("1 1", "1 2", "2 2"), BORN)),
            "pair_coeff * * coul/dsf", *CHARGES]


def slab():
    import bench_pair

    T, X, C, _ = bench_pair.rocksalt_slab()
    return T, X, C, np.ones(3, np.uint8)


def batch(struct, B, sigma=0.05):
    T1, X, Cl, pbc = struct
    rng = np.random.default_rng(0)
    pos = np.concatenate([X + rng.normal(0, sigma, X.shape) for _ in range(B)])
    return (np.full(B, len(T1), np.int32), np.tile(T1, B), pos, np.tile(Cl.reshape(1, 9), (B, 1)), np.tile(pbc.reshape(1, 3), (B, 1)))


def measure(lines, struct, B, reps, relax_steps, profile=None):
    """(resident evaluations/s, whole-call evaluations/s, CG relaxations/s or None, mean CG evaluations or None); ``profile``: a dict
    that receives the handle's per-kernel counters of one more run."""
    from surface_sampling_amd import backend, pair

    eng = backend.PairEngine(pair.parse(lines, 2), device=0)
    arrays = batch(struct, B)
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    for _ in range(2):
        eng.evaluate_arrays_f64(*arrays)
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.evaluate_arrays_f64(*arrays)
    call = B * reps / (time.perf_counter() - t0)
    eng.upload_arrays(*arrays)
    eng.run(want)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.run(want)
    eng.synchronize()
    run = B * reps / (time.perf_counter() - t0)
    cg = n_eval = None
    if relax_steps > 0:
        X = struct[1]
        held = np.tile((X[:, 2] < 0.5 * (X[:, 2].min() + X[:, 2].max())).astype(np.uint8), B)
        eng.relax_cg_arrays_f64(*arrays, fixed=held, max_iter=relax_steps, rerun=False)
        t0 = time.perf_counter()
        out = eng.relax_cg_arrays_f64(*arrays, fixed=held, max_iter=relax_steps, rerun=False)
        cg, n_eval = B / (time.perf_counter() - t0), float(out[5].mean())
    if profile is not None:
        eng.profile_enable(True)
        eng.profile_reset()
        eng.run(want)
        eng.synchronize()
        profile.update({k: round(v["total_ms"], 4) for k, v in eng.profile_read().items() if v["launches"]})
        eng.profile_enable(False)
    eng.close()
    return run, call, cg, n_eval


def slab_compare(args, s):
    """The slab handle on the slabs (pbc 1 1 0) against the 3-D handle on the same atoms in the cell with c multiplied by F."""
    from surface_sampling_amd import pair

    T, X, Cl, _ = s
    F = args.slab
    tall = Cl.copy()
    tall[2] *= F
    open_z, periodic = (T, X, Cl, np.array([1, 1, 0], np.uint8)), (T, X, tall, np.ones(3, np.uint8))
    for B in [int(x) for x in args.chains.split(",") if x]:
        for A in [float(x) for x in args.accuracy.split(",") if x]:
            lines3 = ewald_lines(args.rc, A)
            k = next(n for n, ln in enumerate(lines3) if ln.startswith("kspace_style"))
            lines2 = ["boundary p p f", *lines3[:k + 1], f"kspace_modify slab {F}", *lines3[k + 1:]]
            ks = pair.parse(lines2, 2).kspace
            prof3, prof2 = {}, {}
            three, two = [], []
            for n in range(args.repeats):   # alternating, so that warm-up and clock drift fall on both sides alike
                three.append(measure(lines3, periodic, B, args.reps, 0, profile=prof3 if n == 0 else None)[0])
                two.append(measure(lines2, open_z, B, args.reps, 0, profile=prof2 if n == 0 else None)[0])
            m3, m2 = float(np.median(three)), float(np.median(two))
            print(json.dumps({"metric": f"slab Ewald sum (F {F:g}) against the 3-D sum of the same k box, rocksalt slab ({len(T)} atoms, rc {args.rc}, "
                                        f"A {A:g})", "chains": B, "g_ewald": round(ks.g_ewald, 5), "k_cut": round(ks.k_cut, 5),
                              "slab_evals_per_s_resident": [round(x, 1) for x in two], "three_d_evals_per_s_resident": [round(x, 1) for x in three],
                              "slab_median": round(m2, 1), "three_d_median": round(m3, 1), "slab_over_three_d": round(m2 / m3, 4),
                              "three_d_spread": round((max(three) - min(three)) / m3, 4), "slab_spread": round((max(two) - min(two)) / m2, 4),
                              "profile_ms_three_d": prof3, "profile_ms_slab": prof2}), flush=True)


def stats_share(path):
    """Share of the k_ewald_* kernels in the total kernel time of a rocprofv3 --kernel-trace run (its rocpd database)."""
    db = sqlite3.connect(path)
    rows = db.execute("select s.kernel_name, count(*), sum(d.end - d.start) from rocpd_kernel_dispatch d "
                      "join rocpd_info_kernel_symbol s on d.kernel_id = s.id group by s.kernel_name").fetchall()
    total = sum(r[2] for r in rows)
    ew = {("k_ewald_" + n.split("k_ewald_")[1].split("ENS_")[0]): (k, t) for n, k, t in rows if "k_ewald_" in n}
    print(json.dumps({"metric": "k-space share of the kernel time", "share": round(sum(t for _, t in ew.values()) / total, 4),
                      "ms_per_launch": {n: round(t / k / 1e6, 4) for n, (k, t) in ew.items()},
                      "all_kernels_ms": round(total / 1e6, 3), "kernels": len(rows)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="256,1024,4096")
    ap.add_argument("--accuracy", default="1e-5,1e-8")
    ap.add_argument("--rc", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--relax-steps", type=int, default=20)
    ap.add_argument("--no-dsf", action="store_true")
    ap.add_argument("--slab", type=float, default=0.0, metavar="F", help="compare the slab handle (slab factor F) with the 3-D handle of the same k box")
    ap.add_argument("--repeats", type=int, default=5, help="independent measurements per figure of --slab (run-to-run spread)")
    ap.add_argument("--stats", metavar="DB", help="print the k-space share from the rocpd database of a rocprofv3 --kernel-trace run and exit")
    args = ap.parse_args()
    if args.stats is not None:
        return stats_share(args.stats)
    from surface_sampling_amd import pair

    s = slab()
    if args.slab:
        return slab_compare(args, s)
    for B in [int(x) for x in args.chains.split(",") if x]:
        ref = None if args.no_dsf else measure(dsf_lines(args.rc), s, B, args.reps, args.relax_steps)
        if ref:
            print(json.dumps({"metric": f"coul/dsf yardstick, rocksalt slab ({len(s[0])} atoms, rc {args.rc})", "chains": B,
                              "evals_per_s_resident": round(ref[0], 1), "evals_per_s_call": round(ref[1], 1),
                              "cg_relaxations_per_s": ref[2] and round(ref[2], 1), "cg_mean_n_eval": ref[3]}), flush=True)
        for A in [float(x) for x in args.accuracy.split(",") if x]:
            lines = ewald_lines(args.rc, A)
            ks = pair.parse(lines, 2).kspace
            r = measure(lines, s, B, args.reps, args.relax_steps)
            out = {"metric": f"Ewald sum, rocksalt slab ({len(s[0])} atoms, rc {args.rc}, A {A:g})", "chains": B,
                   "g_ewald": round(ks.g_ewald, 5), "k_cut": round(ks.k_cut, 5),
                   "evals_per_s_resident": round(r[0], 1), "evals_per_s_call": round(r[1], 1),
                   "cg_relaxations_per_s": r[2] and round(r[2], 1), "cg_mean_n_eval": r[3]}
            if ref:
                out["dsf_over_ewald_resident"] = round(ref[0] / r[0], 2)
                out["dsf_over_ewald_cg"] = ref[2] and round(ref[2] / r[2], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
