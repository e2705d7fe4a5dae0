"""CPU only: how evenly BundleWalk deals the bundles of the bench chains to the 16 waves of a forward neighbor-sum workgroup.

For every chain of the bench batch: neighbor counts at the 5 A cutoff (CPU oracle), rows padded to a multiple of 4 slots with a
minimum of 8, centres sorted by padded slot count (descending), bundles of 4 consecutive centres, steps of a bundle = slots of its
longest centre / 4 (at least 2), bundles dealt to 16 waves in snake order (w, 31 - w, 32 + w, ...).  Prints, per group of chain
sizes, the step count of the slowest wave against the mean over the waves.  Usage: python profiles/r33/bundle_balance.py"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bench, oracle

oracle.build()
_, S, _ = bench.load_golden()
rows = []
for s in bench.build_chains(S, 0, 256):
    i = oracle.neighbors(s.positions, s.cell, s.pbc, 5.0)[0]
    slots = np.maximum((np.bincount(i, minlength=len(s)) + 3) // 4 * 4, 8)
    order = np.sort(slots)[::-1]
    steps = np.array([max(order[4 * b] // 4, 2) for b in range((len(s) + 3) // 4)])
    wave = np.zeros(16, np.int64)
    for b, st in enumerate(steps):
        jj, r = divmod(b, 16)
        wave[15 - r if jj & 1 else r] += st
    rows.append((len(s), len(steps), wave.max(), wave.mean(), int(np.median(steps))))
rows = np.array(rows, dtype=np.float64)
for name, sel in (("n <= 256 (NB <= 64)", rows[:, 0] <= 256), ("n >= 257 (NB >= 65)", rows[:, 0] > 256)):
    r = rows[sel]
    print(f"{name}: {len(r)} chains, atoms {int(r[:, 0].min())}..{int(r[:, 0].max())}, bundles {int(r[:, 1].min())}..{int(r[:, 1].max())}, "
          f"median bundle {int(np.median(r[:, 4]))} steps; slowest wave {int(r[:, 2].min())}..{int(r[:, 2].max())} steps, "
          f"mean wave {r[:, 3].min():.1f}..{r[:, 3].max():.1f}; slowest / mean - 1: {100 * (r[:, 2] / r[:, 3] - 1).min():.1f} .. "
          f"{100 * (r[:, 2] / r[:, 3] - 1).max():.1f} % (mean {100 * (r[:, 2] / r[:, 3] - 1).mean():.1f} %)")
all_ = 100 * (rows[:, 2] / rows[:, 3] - 1)
print(f"all 256 chains: slowest / mean - 1 = {all_.mean():.1f} % on average; idle share of a 16-wave workgroup at the end of a walk = "
      f"{100 * (1 - rows[:, 3] / rows[:, 2]).mean():.1f} %")
