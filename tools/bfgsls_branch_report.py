"""CPU reports behind tests/bfgsls_cases.py (no GPU): what the numpy restatement of BFGSLineSearch does on every case.

    python tools/bfgsls_branch_report.py table          steps, evaluations, stop reason, smallest decision margin, the drift of a start
                                                        perturbed by 1e-12 A, and the branch counters of every case (markdown)
    python tools/bfgsls_branch_report.py search [N]     seed search for the rarer branches over N rattled clusters per kind, size and
                                                        parameter variant (default 30)

profiles/r19/NOTES_bfgs_linesearch.md keeps the output."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bfgsls_cases as bc  # noqa: E402
import bfgsls_oracle as bo  # noqa: E402
import cg_cases as cc  # noqa: E402
import oracle  # noqa: E402
from conftest import Golden  # noqa: E402

RARE = ("bisection", "skip_update", "no_update", "rho_fallback", "p_floor", "fallback_stx", "warn_rounding", "warn_xtol", "warn_stpmin",
        "error_start", "stop5")
VARIANTS = [dict(), dict(stpmax=1.0), dict(stpmax=2.0), dict(maxstep=0.02), dict(maxstep=1.0), dict(alpha=1.0), dict(alpha=70.0),
            dict(c2=0.1), dict(c1=1e-4, c2=0.9), dict(alpha=1.0, maxstep=1.0), dict(alpha=0.3, maxstep=2.0),
            dict(alpha=1.0, c2=0.05, maxstep=1.0)]


def table(golden):
    print("| case | class | atoms | held | steps | eval | stop | margin | at | drift (A) | branches |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for c in bc.all_cases(golden):
        tr = bo.Trace()
        x, e, st, ev, why, _ = bc.run_restatement(c, golden, oracle, trace=tr)
        rng = np.random.default_rng(7)
        x2, _, st2, ev2, why2, _ = bc.run_restatement(c, golden, oracle, pos=c.pos + rng.uniform(-1e-12, 1e-12, c.pos.shape))
        drift = f"{np.abs(x2 - x).max():.1e}" if (st2, ev2, why2) == (st, ev, why) else f"counts {(st2, ev2, why2)}"
        br = " ".join(f"{k}:{v}" for k, v in sorted(tr.branches.items()))
        print(f"| {c.name} | {c.klass} | {len(c.types)} | {len(c.fixed)} | {st} | {ev} | {why} | {tr.margin:.1e} | {tr.margin_at} | {drift} | {br} |")


def search(golden, n_seeds):
    found = {k: [] for k in RARE}
    for kind in ("tersoff", "pair"):
        for soft in ((0, 1) if kind == "pair" else (0,)):
            for n in (2, 3, 4, 5, 7):
                for seed in range(n_seeds):
                    t, p = cc.cluster(kind, golden, n, seed, 0.1)
                    c = bc.Case("x", kind, "exact", np.asarray(t + soft, np.int32), p, np.eye(3) * cc.BOX, np.zeros(3, np.uint8),
                                np.array([0] if n > 2 else [], np.int64), {}, None, ())
                    fn = bc.force_fn(c, golden, oracle)
                    for v in VARIANTS:
                        tr = bo.Trace()
                        _, _, st, ev, why, _ = bo.bfgs_linesearch(fn, p, fixed=c.fixed, max_steps=20, fmax=0.01, trace=tr, **v)
                        for k in RARE:
                            if k in tr.branches and len(found[k]) < 6:
                                found[k].append(f"{kind}{' soft' if soft else ''} n={n} seed={seed} {v} -> steps {st} eval {ev} stop {why} "
                                                f"margin {tr.margin:.1e} ({tr.margin_at})")
    for k, rows in found.items():
        print(f"{k}: {'NOT REACHED' if not rows else ''}")
        for r in rows:
            print("    " + r)


if __name__ == "__main__":
    oracle.build()
    oracle.set_threads(min(os.cpu_count() or 1, 8))
    mode = sys.argv[1] if len(sys.argv) > 1 else "table"
    if mode == "table":
        table(Golden())
    elif mode == "search":
        search(Golden(), int(sys.argv[2]) if len(sys.argv) > 2 else 30)
    else:
        sys.exit(__doc__)
