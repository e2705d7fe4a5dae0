"""Inputs of tests/test_neb_gpu.py and their CPU rehearsal in tests/test_neb_cpu.py (test infrastructure).  Structures are
``(types, positions, cell, pbc)``; a band is a list of structures that differ in positions only, with one held mask [N] per band."""
from collections import namedtuple

import numpy as np

import cg_cases as cc
import neb_oracle as no
import pair_oracle as po

BOX = np.eye(3) * 40.0
OPEN = np.zeros(3, np.uint8)

# ---- the physics anchor: one free lj/cut atom (cg_cases.LJ_TERMS type 0: eps 1, sigma 2.6, rc 8) passes along z through a fixed
# equilateral triangle of side 4.6 A.  With R the circumradius, r(z) = sqrt(R^2 + z^2) and E(z) = 3 LJ(r): the minima sit where
# r = 2^(1/6) sigma, the saddle in the plane, and the barrier is 3 (LJ(R) + eps) whatever the cutoff shift --------------------------
ANCHOR_SIDE, ANCHOR_EPS, ANCHOR_SIGMA = 4.6, 1.0, 2.6
ANCHOR_R = ANCHOR_SIDE / np.sqrt(3.0)
ANCHOR_ZMIN = float(np.sqrt((2.0 ** (1.0 / 6.0) * ANCHOR_SIGMA) ** 2 - ANCHOR_R ** 2))
ANCHOR_BARRIER = float(3.0 * (4.0 * ANCHOR_EPS * ((ANCHOR_SIGMA / ANCHOR_R) ** 12 - (ANCHOR_SIGMA / ANCHOR_R) ** 6) + ANCHOR_EPS))
ANCHOR_BOW = 0.15
ANCHOR_CENTRE = np.array([16.0, 16.0, 16.0])
ANCHOR_HELD = np.array([1, 1, 1, 0], np.uint8)
ANCHOR = dict(k=0.1, fmax=0.01, max_steps=200)


def triangle():
    ang = np.pi / 2 + np.arange(3) * 2 * np.pi / 3
    return np.stack([ANCHOR_R * np.cos(ang), ANCHOR_R * np.sin(ang), np.zeros(3)], axis=1) + ANCHOR_CENTRE


def anchor_image(x, y, z):
    """The triangle and the free atom at (x, y, z) from its centre."""
    return np.zeros(4, np.int32), np.vstack([triangle(), ANCHOR_CENTRE + [x, y, z]]), BOX, OPEN


def anchor_band(n, bow=ANCHOR_BOW, zend=ANCHOR_ZMIN):
    """n images from z = -zend to +zend, bowed in x by bow sin(pi s)."""
    return [anchor_image(bow * np.sin(np.pi * i / (n - 1)) if 0 < i < n - 1 else 0.0, 0.0, -zend + 2.0 * zend * i / (n - 1)) for i in range(n)]


def lj_batch_fn(structs):
    """The numpy restatement of the pair_lj handle (tests/pair_oracle.py) as force callback of a whole batch."""
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])])

    def fn(pos):
        E, F = [], []
        for s, a0, a1 in zip(structs, start[:-1], start[1:]):
            e, _, f = po.pair(cc.LJ_TERMS, None, s[0], pos[a0:a1], s[2], s[3])
            E.append(e)
            F.append(f)
        return np.array(E), np.vstack(F)
    return fn


def anchor_saddle_hessian(h=1e-3):
    """3 x 3 Hessian of the free atom at the closed-form saddle (the centre of the triangle), by central differences of the forces."""
    s = anchor_image(0.0, 0.0, 0.0)
    fn = lj_batch_fn([s])
    H = np.zeros((3, 3))
    for c in range(3):
        p, m = s[1].copy(), s[1].copy()
        p[3, c] += h
        m[3, c] -= h
        H[c] = -(fn(p)[1][3] - fn(m)[1][3]) / (2 * h)
    return 0.5 * (H + H.T)


def barrier_bound(fmax, H):
    """|E(climbing image) - E(saddle)| <= 2 fmax^2 / (2 min |lambda|): a residual force g at a stationary point of a quadratic form
    leaves an energy error g^2 / (2 |lambda|) per mode; the factor 2 covers the quadratic approximation."""
    lam = np.linalg.eigvalsh(H)
    return 2.0 * fmax * fmax / (2.0 * np.abs(lam).min())


# ---- the census cases: bands on the pair_lj handle that together visit every branch of the restatement ----------------------------------
Case = namedtuple("Case", "name band held params")


def pack(cases):
    """(structures of the batch, n_img, held mask [sum N])."""
    structs = [s for c in cases for s in c.band]
    return structs, [len(c.band) for c in cases], np.concatenate([np.tile(c.held, len(c.band)) for c in cases])


def census_cases():
    out = [Case("anchor6_climb_improved", anchor_band(6), ANCHOR_HELD, dict(ANCHOR, climb=True, method="improvedtangent")),
           Case("anchor6_climb_aseneb", anchor_band(6), ANCHOR_HELD, dict(ANCHOR, climb=True, method="aseneb")),
           Case("anchor6_plain_improved", anchor_band(6), ANCHOR_HELD, dict(ANCHOR, climb=False, method="improvedtangent")),
           Case("anchor5_plain_aseneb", anchor_band(5), ANCHOR_HELD, dict(ANCHOR, climb=False, method="aseneb")),
           # three images mirror-symmetric about the plane at offsets that are exact in binary: E(i+1) == E(i-1) bit for bit
           Case("tie3", [anchor_image(0.0, 0.0, -1.25), anchor_image(0.125, 0.0625, 0.0), anchor_image(0.0, 0.0, 1.25)], ANCHOR_HELD,
                dict(ANCHOR, climb=False, method="improvedtangent", max_steps=40)),
           # nine images far off the path: forces of several eV / A on every image, so the band norm of a step passes maxstep where no
           # image's own share does
           Case("bowed9", anchor_band(9, bow=0.9), ANCHOR_HELD, dict(ANCHOR, climb=False, method="improvedtangent", max_steps=30))]
    return out


def run_case(case, force_fn=None, record=None, **over):
    structs, n_img, held = pack([case])
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])])
    fn = force_fn or lj_batch_fn(structs)
    return no.run(fn, np.vstack([s[1] for s in structs]), start, n_img, [s[2] for s in structs], [s[3] for s in structs], fixed=held,
                  record=record, **{**case.params, **over})


def census(cases=None):
    """{branch: set of case names that visit it}."""
    seen = {b: set() for b in no.BRANCHES}
    for c in cases or census_cases():
        rec = []
        run_case(c, record=rec)
        for r in rec:
            for b in r["branches"]:
                seen[b].add(c.name)
    return seen


REQUIRED = ("tangent_up", "tangent_down", "tangent_extremum_rising", "tangent_extremum_falling", "tangent_tie", "ase_below", "ase_above",
            "ase_at", "climb", "noclimb", "first", "uphill_reset", "downhill_hold", "downhill_grow", "clip_band_only", "noclip")


# ---- a band that turns non-finite after its first step ---------------------------------------------------------------------------------
# lj/cut stays finite down to 1e-25 A and the landing point of a FIRE step cannot be put on another atom to the bit, so the wall is a
# REGION: the 0 - 1 term (eps 1e308 eV, sigma 0.5 A, cutoff 0.6 A) overflows in energy or force everywhere inside its cutoff and
# is absent outside.  A held type-1 atom 2.4 A away pushes the free type-1 atom with 36 eV / A towards a held type-0 atom 0.7 A on: the
# first step is clamped to maxstep = 0.2 A and ends 0.5 A from the wall atom.  The images differ across the push, so the projection keeps it.
WALL_TERMS = [(0, 0, "lj/cut", (1.0, 2.6), 8.0, 0), (1, 1, "lj/cut", (1.0, 2.6), 8.0, 0), (0, 1, "lj/cut", (1e308, 0.5), 0.6, 0)]
WALL_HELD = np.array([1, 0, 1], np.uint8)


def wall_band():
    T = np.array([1, 1, 0], np.int32)
    return [(T, np.array([[10.0, 10.0, 10.0], [12.4, 10.0 + y, 10.0], [13.1, 10.0, 10.0]]), BOX, OPEN) for y in (-0.05, 0.0, 0.05)]


def wall_batch_fn(structs):
    """pair_oracle on WALL_TERMS as force callback of a whole batch (overflows are the point: no warnings)."""
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in structs])])

    def fn(pos):
        E, F = [], []
        with np.errstate(all="ignore"):
            for s, a0, a1 in zip(structs, start[:-1], start[1:]):
                e, _, f = po.pair(WALL_TERMS, None, s[0], pos[a0:a1], s[2], s[3])
                E.append(e)
                F.append(f)
        return np.array(E), np.vstack(F)
    return fn
