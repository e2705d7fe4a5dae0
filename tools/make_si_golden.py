#!/usr/bin/env python3
"""Generate tests/golden/si111_5x5.npz from the reference's Si(111) 5x5 slab pickle (run in the build container only).

The reference's Si tutorial (tutorials/data/Si_111_5x5/Si_111_5x5_pristine_slab.pkl) holds a 100-atom slab whose first 75 atoms
form the bulk group (``bulk_index`` 75 of its lammps_config.json).  What is written is DATA only: atomic numbers, positions, cell,
pbc and the fixed mask.  No reference template or source is copied; the tests write their own run directories.

    python tools/make_si_golden.py [--reference /path/to/reference]
"""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from surface_sampling_amd import structures  # noqa: E402

BULK_INDEX = 75


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("VSSR_REFERENCE", "../reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "si111_5x5.npz"))
    args = ap.parse_args()
    src = os.path.join(args.reference, "tutorials", "data", "Si_111_5x5", "Si_111_5x5_pristine_slab.pkl")
    s = structures.read_slab_pickle(src)
    n = len(s.numbers)
    fixed = np.zeros(n, bool)
    fixed[:BULK_INDEX] = True
    if s.constraints_fixed is not None and len(s.constraints_fixed):
        if not np.array_equal(np.sort(np.asarray(s.constraints_fixed)), np.arange(BULK_INDEX)):
            print(f"note: the pickle's own constraint holds {len(s.constraints_fixed)} atoms; the mask follows bulk_index {BULK_INDEX}")
    np.savez_compressed(args.out, numbers=np.asarray(s.numbers, np.int32), positions=np.asarray(s.positions, np.float64),
                        cell=np.asarray(s.cell, np.float64), pbc=np.asarray(s.pbc, bool), fixed=fixed)
    print(f"wrote {args.out}: {n} atoms, Z = {sorted(set(np.asarray(s.numbers).tolist()))}, pbc = {np.asarray(s.pbc).tolist()}")


if __name__ == "__main__":
    main()
