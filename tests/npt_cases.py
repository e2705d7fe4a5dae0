"""Inputs that tests/test_npt_cpu.py and tests/test_npt_gpu.py share (test infrastructure): the coupling combinations, the stop cases and the
capacity case of the constant-pressure MD, each chosen with tests/npt_oracle.py under the exact pair virial on the CPU (the CPU test
rehearses them: which stop reason each chain ends with and after how many steps)."""
import numpy as np

import cellrelax_cases as cs
import cellrelax_oracle as co
import pair_cases as pc

TYPE_MASS = np.array([26.9815385, 63.546, 107.8682])          # the masses of tests/test_md_gpu.py, by type % 3

# every thermostat x barostat x coupling the entry point accepts (crescale: isotropic, with a thermostat)
COMBOS = [(t, b, c) for t in ("none", "langevin", "berendsen") for b, c in (("none", "isotropic"), ("berendsen", "isotropic"),
                                                                           ("berendsen", "per_axis"), ("crescale", "isotropic"))
          if not (b == "crescale" and t == "none")]
assert len(COMBOS) == 11

# couplings of the step-for-step runs: strong enough that ten steps move a cell by 1e-3 A and more, weak enough that no cell of the
# parity batches comes near another periodic image (the strain of a step is (dt beta / (3 taup)) (P0 - P) = (P0 - P) / 600)
COUPLING = dict(temperature=300.0, temperature_end=500.0, ramp_steps=8, friction=0.02, taut=20.0, taup=20.0, compressibility=0.1, pressure=0.01)


def masses(structs):
    return np.concatenate([TYPE_MASS[np.asarray(s[0]) % 3] for s in structs])


def start(structs):
    return np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])]).astype(np.int64)


def pair_fn(terms, structs, baro=True):
    """tests/pair_oracle.py with the exact virial as the force callback of npt_oracle.run over the batch ``structs``."""
    st = start(structs)

    def fn(pos, cells):
        E, F, S = [], [], []
        with np.errstate(all="ignore"):
            for b, s in enumerate(structs):
                e, f, sig = co.pair_virial(terms, None, s[0], pos[st[b]:st[b + 1]], cells[b], s[3])
                E.append(e); F.append(f); S.append(sig)
        return np.array(E), np.vstack(F), (np.array(S) if baro else None)
    return fn


def size_batch():
    """Chains of 1, 255, 256 and 257 atoms (the block-stride and reduction edges of the 256-thread workgroup), periodic: the single atom
    alone in a 9 A cube, the others on the jittered skewed grid of pair_cases.grid_chain."""
    one = (np.zeros(1, np.int32), np.array([[4.0, 4.5, 5.0]]), np.eye(3) * 9.0, np.ones(3, np.uint8))
    return [one] + [pc.grid_chain(n, 30 + k, [1, 1, 1], n_types=2, spacing=2.9, jitter=0.1) for k, n in enumerate((255, 256, 257))]


# ---- reason 3: the thin cell of cellrelax_cases under LJ_THIN (rc 7.9 A: a third image below a height of 3.95 A, 2 % of compression) and
# its neighbour at a = 4.25 A, under 1.5 eV / A^3: the strain of a step is (P0 - P) / 300, about 0.5 % -------------------------------
THIN = dict(n_steps=8, dt=1.0, barostat="berendsen", taup=10.0, compressibility=0.1, pressure=1.5)
THIN_CUTOFF = 7.9


def thin_case():
    thin, other, _ = cs.thin_case()
    return [thin, other]


# ---- reason 2 in the middle of a trajectory: the wall case of cellrelax_cases (a held pair 0.62 A apart rides the shrinking cell into
# the 0 - 1 term that overflows below 0.6 A, 3.3 % of compression; another image would need 5.9 %) ------------------------------------
WALL = dict(n_steps=8, dt=1.0, barostat="berendsen", taup=10.0, compressibility=0.1, pressure=1.5)


def wall_case():
    wall, held_w, terms, rc = cs.wall_case()
    other = (np.ones(8, np.int32),) + cs.thin_case()[1][1:]
    return [wall, other], np.concatenate([held_w, np.zeros(8, np.uint8)]), terms, rc


# ---- a capacity regrow in the middle of a trajectory: the 32-atom cube of cellrelax_cases at a = 4.20 A (54 neighbors within 6.5 A; the
# fifth shell, 24 more, enters below 4.11 A) compressed by the barostat ---------------------------------------------------------------------
REGROW = dict(n_steps=25, dt=1.0, thermostat="berendsen", barostat="berendsen", temperature=50.0, taut=20.0, taup=10.0, compressibility=0.1,
              pressure=0.5)
