"""CPU reports behind tests/cg_cases.py (no GPU): what the numpy restatement of the CG minimiser does on every case.

    python tools/cg_branch_report.py table            branch counters, counts and stop reason of every case (markdown)
    python tools/cg_branch_report.py search [N]       seed search for proj_rejected / not_downhill_reset over N rattled clusters per
                                                      kind, size and parameter set (default 400)
    python tools/cg_branch_report.py noise            spread of the final energy of the noise cases over 8 starts perturbed by 1e-12 A

profiles/r18/NOTES_cg_branches.md keeps the output."""

import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import cg_cases as cc  # noqa: E402
import oracle  # noqa: E402
from cg_oracle import BRANCHES  # noqa: E402
from conftest import Golden  # noqa: E402


def table(golden):
    print("| case | atoms | held | iter | eval | stop | " + " | ".join(BRANCHES) + " |")
    print("|---|---|---|---|---|---|" + "---|" * len(BRANCHES))
    for c in cc.all_cases(golden):
        tr = Counter()
        _, e, it, ev, why, _ = cc.run_restatement(c, golden, oracle, trace=tr)
        print(f"| {c.name} | {len(c.types)} | {len(c.fixed)} | {it} | {ev} | {why} | " + " | ".join(str(tr[b]) for b in BRANCHES) + " |")


def search(golden, n_seeds):
    none = np.zeros(0, np.int64)
    cell, pbc = np.eye(3) * cc.BOX, np.zeros(3, np.uint8)
    variants = [dict(), dict(dmax=10.0), dict(dmax=1.0, etol=0.0, ftol=1e-3), dict(dmax=0.3)]
    for kind in ("tersoff", "pair"):
        found = {"proj_rejected": [], "not_downhill_reset": []}
        tried = 0
        for n in (2, 3, 4, 5, 7, 9):
            for sigma in (0.1, 0.3):
                for over in variants:
                    for seed in range(1000, 1000 + n_seeds // 8):
                        types, pos = cc.cluster(kind, golden, n, seed, sigma)
                        case = cc.Case("search", kind, "exact", types, pos, cell, pbc, none, cc._params(**over), None, ())
                        tr = Counter()
                        try:
                            _, e, it, ev, why, _ = cc.run_restatement(case, golden, oracle, trace=tr)
                        except (FloatingPointError, ZeroDivisionError):
                            continue
                        tried += 1
                        for b in found:
                            if tr[b] and why in (1, 2, 3) and np.isfinite(e):
                                found[b].append((n, seed, sigma, over, it, ev, why, tr[b]))
        print(f"{kind}: {tried} runs")
        for b, hits in found.items():
            print(f"  {b}: {len(hits)} hits; first: {hits[:5]}")


def noise(golden):
    worst = 0.0
    print("| case | stop reasons of the 9 runs | iterations | E (unperturbed) | spread of E over the 8 perturbed starts + the unperturbed one |")
    print("|---|---|---|---|---|")
    for c in cc.all_cases(golden):
        if c.klass != "noise":
            continue
        rng = np.random.default_rng(7)
        es, whys, its = [], [], []
        for k in range(9):
            pos = c.pos + (rng.uniform(-1e-12, 1e-12, c.pos.shape) if k else 0.0)
            pos[c.fixed] = c.pos[c.fixed]
            _, e, it, ev, why, _ = cc.run_restatement(c, golden, oracle, pos=pos)
            es.append(e); whys.append(why); its.append(it)
        spread = max(es) - min(es)
        worst = max(worst, spread)
        print(f"| {c.name} | {whys} | {its} | {es[0]:.15f} | {spread:.3e} |")
    print(f"largest spread {worst:.3e} eV -> bound max(10 x spread, 1e-8) = {max(10 * worst, 1e-8):.3e} eV")


if __name__ == "__main__":
    oracle.build()
    oracle.set_threads(1)
    g = Golden()
    what = sys.argv[1] if len(sys.argv) > 1 else "table"
    if what == "table":
        table(g)
    elif what == "search":
        search(g, int(sys.argv[2]) if len(sys.argv) > 2 else 400)
    else:
        noise(g)
