"""Secondary measurement (not the BASELINE metric): what one ``stress()`` call (vssr_batch_stress) costs on the fp64 analytic
potentials next to one energy + force evaluation of the same resident batch.  Per potential one JSON line: B chains of rattled
bulk cells -- Tersoff GaN (48-atom wurtzite cells), Stillinger-Weber Si (64-atom diamond cells), EAM Cu_u3 (108-atom fcc cells).
Both times are host clocks around calls that end in a device synchronise (``run`` + ``synchronize``; ``stress`` synchronises and
copies [B, 6] doubles back itself), medians over --reps calls after --warmup calls.
Usage: python tools/bench_analytic_stress.py [--chains 1024] [--reps 30] [--warmup 5]"""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def repeat(types, pos, cell, reps):
    shifts = [i * cell[0] + j * cell[1] + k * cell[2] for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])]
    return np.tile(types, len(shifts)), np.concatenate([pos + s for s in shifts]), cell * np.asarray(reps, float)[:, None]


def cells():
    a, c, u = 3.189, 5.185, 0.377
    hexc = np.array([[a, 0, 0], [-a / 2, a * np.sqrt(3) / 2, 0], [0, 0, c]])
    frac = np.array([[1 / 3, 2 / 3, 0], [2 / 3, 1 / 3, .5], [1 / 3, 2 / 3, u], [2 / 3, 1 / 3, .5 + u]])
    gan = repeat(np.array([0, 0, 1, 1], np.int32), frac @ hexc, hexc, (2, 2, 3))
    dia = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75], [.75, .75, .25]])
    si = repeat(np.zeros(8, np.int32), dia * 5.43095, np.eye(3) * 5.43095, (2, 2, 2))
    cu = repeat(np.zeros(4, np.int32), dia[:4] * 3.615, np.eye(3) * 3.615, (3, 3, 3))
    return {"tersoff": gan, "sw": si, "eam": cu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from surface_sampling_amd import backend, eam, sw

    with open(os.path.join(GOLDEN, "GaN_tersoff_params.json")) as fh:
        gan_params = np.array(json.load(fh)["params_ijk"], dtype=np.float64)
    engines = {"tersoff": lambda: backend.TersoffEngine(gan_params, device=0),
               "sw": lambda: backend.SWEngine(sw.parse_sw(sw.builtin_text("SW_StillingerWeber_1985_Si__MO_405512056662_005"), ["Si"]), device=0),
               "eam": lambda: backend.EAMEngine(eam.read_funcfl(os.path.join(GOLDEN, "Cu_u3.eam")), device=0)}
    want = backend.WANT_ENERGY | backend.WANT_FORCES | backend.WANT_PER_ATOM
    rng = np.random.default_rng(0)
    for name, (T, X, Cl) in cells().items():
        eng = engines[name]()
        eng.upload([(T, X + rng.normal(0.0, 0.05, X.shape), Cl, np.ones(3, np.uint8)) for _ in range(args.chains)])

        def one_run():
            eng.run(want)
            eng.synchronize()

        times = {}
        for label, call in (("evaluation", one_run), ("stress", eng.stress)):
            for _ in range(args.warmup):
                call()
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                t.append(time.perf_counter() - t0)
            times[label] = (float(np.median(t)) * 1e3, float(np.min(t)) * 1e3, float(np.max(t)) * 1e3)
        st = eng.stats()
        print(json.dumps({"metric": "host time of one call ending in a device synchronise, ms (median, min, max)", "potential": name,
                          "chains": args.chains, "atoms_per_chain": len(T), "slots": st["slots"], "reps": args.reps,
                          "evaluation_ms": times["evaluation"], "stress_ms": times["stress"],
                          "stress_over_evaluation": times["stress"][0] / times["evaluation"][0]}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
