#!/usr/bin/env python3
"""Time the device Gaussian-mixture fit (csrc/gmm_fit.hip) against scikit-learn on the host: one JSON line per case.

bench_gmm_fit.py [--rows 66503,1000000] [--components 5,16] [--dim 128] [--iters 5] [--no-host]
Rows are synthetic (K separated Gaussian clusters, float32 values as a PaiNN embedding has); both sides start from the same noisy
labels and run exactly --iters EM iterations (tol = 0).  device_iter_ms: one EM iteration (a max_iter = 1 fit after warm-up, the
rows already resident, the final synchronisation included); device_fit_ms: the --iters fit; upload_ms: the host-to-device copy a
caller-row fit needs and a resident fit does not; host_fit_ms: sklearn.mixture.GaussianMixture on the same rows (the path
GMMUncertainty.fit_gmm takes without fit_device).  cov_gflop = 2 K N D^2 per iteration, the full covariance's algorithmic work.
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_gmm_fit.py --no-host ...`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from surface_sampling_amd import backend   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="66503")
    ap.add_argument("--components", default="5,16")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    D = a.dim
    for N in (int(v) for v in a.rows.split(",")):
        for K in (int(v) for v in a.components.split(",")):
            rng = np.random.default_rng(N + K)
            true = rng.integers(0, K, N)
            X = (3.0 * rng.normal(size=(K, D))[true] + rng.normal(size=(N, D))).astype(np.float32).astype(np.float64)
            labels = np.where(rng.random(N) < 0.3, rng.integers(0, K, N), true).astype(np.int32)

            def device(iters, X=X, labels=labels, K=K):
                eng = backend.GMMFitEngine(K, D, tol=0.0, max_iter=iters, init="given")
                t0 = time.perf_counter()
                eng.append_rows(X)
                t1 = time.perf_counter()
                eng.set_init(labels=labels)
                eng.fit()                                   # warm-up: allocations, code load
                t2 = time.perf_counter()
                r = eng.fit()
                t3 = time.perf_counter()
                eng.close()
                return (t1 - t0) * 1e3, (t3 - t2) * 1e3, r

            up, it_ms, _ = device(1)
            _, fit_ms, r = device(a.iters)
            out = {"rows": N, "dim": D, "components": K, "iters": a.iters, "upload_ms": round(up, 3),
                   "device_iter_ms": round(it_ms, 3), "device_fit_ms": round(fit_ms, 3), "lower_bound": r["lower_bound"],
                   "cov_gflop_per_iter": round(2.0 * K * N * D * D / 1e9, 3)}
            if not a.no_host:
                import warnings

                from sklearn.mixture import GaussianMixture

                gm = GaussianMixture(K, tol=0.0, max_iter=a.iters, reg_covar=1e-6)
                resp = np.zeros((N, K))
                resp[np.arange(N), labels] = 1.0
                gm._initialize_parameters = lambda X_, random_state, xp=None: gm._initialize(X_, resp)
                t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    gm.fit(X)
                out["host_fit_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                out["host_lower_bound"] = float(gm.lower_bound_)
                out["host_over_device"] = round(out["host_fit_ms"] / fit_ms, 1)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
