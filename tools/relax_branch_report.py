#!/usr/bin/env python3
"""Tables behind tests/relax_cases.py, from the numpy restatements of FIRE and BFGS alone (CPU; no device code runs):

  branches      per case: steps, converged, the branches reached with the first iteration of each, decisions that are near ties
  sensitivity   per case: the spread of 8 runs from starts perturbed by 1e-12 A and the bound max(1e-7 A, 10 x spread)
  mutation      per case and listed branch: the shift of the next iteration's positions when the other branch is forced
  capacity      the 40-atom BFGS case: m per step, the residuals of the rank decisions, the step at which the basis fills

usage: python tools/relax_branch_report.py [branches] [sensitivity] [mutation] [capacity]    (default: all four)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import relax_cases as rc  # noqa: E402


def branches():
    print("| case | atoms (held) | steps | converged | branches reached (first iteration) | near ties |\n|---|---|---|---|---|---|")
    for c in rc.all_cases():
        res, rec = rc.traced(c)
        got = sorted(rc.reached(c, rec))
        firsts = ", ".join(f"{b} ({rc.first_step_of(rec, b)})" if b not in rc.STRUCTURAL else b for b in got)
        missing = [b for b in c.branches if b not in got]
        print(f"| {c.name} | {len(c.types)} ({len(c.fixed)}) | {res[2]} | {res[3]} | {firsts}{' MISSING ' + str(missing) if missing else ''} | {rc.near_ties(c, rec) or 'none'} |")


def sensitivity():
    print("| case | spread / A | bound / A |\n|---|---|---|")
    for c in rc.all_cases():
        s, same = rc.sensitivity(c)
        print(f"| {c.name} | {s:.3e}{'' if same else ' (COUNTS DIFFER)'} | {max(rc.BOUND_FLOOR, 10 * s):.3e} |")


def mutation():
    print("| case | branch | iteration | decision flipped | shift / A | shift / bound |\n|---|---|---|---|---|---|")
    for c in rc.all_cases():
        _, rec = rc.traced(c)
        for b in c.branches:
            it, which, shift = rc.mutation_shift(c, rec, b)
            print(f"| {c.name} | {b} | {it} | {which or '-'} | {'-' if shift is None else f'{shift:.3e}'} | {'-' if shift is None else f'{shift / rc.bound(c):.1e}'} |")


def capacity():
    c = [c for c in rc.all_cases() if c.name == "bfgs:capacity_40"][0]
    _, rec = rc.traced(c)
    print(f"mmax {rc.mmax_of(c)} for max_steps {c.params['max_steps']}")
    lo = max(x for r in rec for x in r.get("residuals", ()) if x < 1e-9)
    hi = min(x for r in rec for x in r.get("residuals", ()) if x > 1e-9)
    print(f"rank decisions: largest residual of a dependent vector {lo:.2e}, smallest of a new direction {hi:.2e}")
    full = [r["it"] for r in rec if "full_basis" in r["branches"]]
    print(f"first skipped update at iteration {full[0]} (m = {rec[full[0]]['m']}), {len(full)} skipped in all")
    print("iteration: m  " + "  ".join(f"{r['it']}:{r['m']}" for r in rec if r["it"] % 8 == 0 or r["it"] in (46, 47, 50, full[0] - 1, full[0])))
    return rec


if __name__ == "__main__":
    np.set_printoptions(precision=3)
    todo = sys.argv[1:] or ["branches", "sensitivity", "mutation", "capacity"]
    for name in todo:
        print(f"\n## {name}\n")
        {"branches": branches, "sensitivity": sensitivity, "mutation": mutation, "capacity": capacity}[name]()
