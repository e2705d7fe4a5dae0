"""A plain-Python restatement of the Tersoff energy and forces (LAMMPS pair_tersoff semantics, the loops of oracle/vssr_oracle.c)
that COUNTS which code every term runs through.

TEST INFRASTRUCTURE ONLY.  ``census`` returns the energy, the forces and a tally {(form, quantity, branch): terms}:

    form      "tile" for a centre whose neighbour row has <= 16 slots (the 16-slot LDS tile of csrc/tersoff_dev.h), "long" beyond
              (the one-thread form); a row is every neighbour inside the largest R + D of the table, d^2 <= rc^2 as the device search
    "fc_ij"   cutoff function of the pair (i, j):  "inner" r < R - D, "shell", plus the named places "R-D-", "R-D", "R-D+", "R+D-",
              "R+D" (one ulp inside, on, one ulp outside the two ends of the shell); "R+D+" are the pairs one ulp beyond the cutoff,
              which are skipped
    "fc_ik"   the same for the third atom of a term (i, j, k)
    "ex"      "lam3=0", "m=1", "m=3" (unclamped), "high" (arg > 69.0776: ex = 1e30, dex = 0), "low" (arg < -69.0776: ex = dex = 0);
              "high,m=1" / "high,m=3" / "low,m=1" / "low,m=3" split the clamps by exponent
    "bij"     the six branches of b_ij in the order of the code: ">c1", ">c2", "<c4", "<c3", "n=1", "general"
    "bij_after_high"   the b_ij branch of the pairs whose zeta holds at least one term of the high clamp: in "n=1" / "general" the
              value 1e30 itself enters E
    "margin"  ("ex",): the smallest | |arg| - 69.0776 | / 69.0776 met -- how far the input is from changing a clamp branch

Its energy is compared with ``oracle.tersoff`` on the CPU (tests/test_potential_edges_cpu.py), so the tallies describe what the C
oracle computes; parity on the device stays against the C oracle.  ``mutate``: "exp_unclamped" (exp(arg) whatever arg),
"dex_kept" (the high clamp keeps dex = ex darg) -- defects a kernel could have, for the sensitivity tests.
"""

from __future__ import annotations

import math
from collections import Counter

import numpy as np

from cell_cases import brute_neighbors

TILE_SLOTS = 16                  # TS_MAXD of csrc/tersoff_dev.h
CLAMP = 69.0776
MUTATIONS = ("exp_unclamped", "dex_kept")
FIELDS = ("m", "gamma", "lam3", "c", "d", "h", "n", "beta", "lam2", "B", "R", "D", "lam1", "A")
BIJ_BRANCHES = (">c1", ">c2", "<c4", "<c3", "n=1", "general")


def _fc(r, R, D):
    if r < R - D:
        return 1.0, 0.0
    if r > R + D:
        return 0.0, 0.0
    x = math.pi / 2 * (r - R) / D
    return 0.5 * (1.0 - math.sin(x)), -(math.pi / 4 / D) * math.cos(x)


def fc_place(r, R, D):
    lo, hi = R - D, R + D
    for name, v in (("R-D-", np.nextafter(lo, 0.0)), ("R-D", lo), ("R-D+", np.nextafter(lo, np.inf)), ("R+D-", np.nextafter(hi, 0.0)),
                    ("R+D", hi), ("R+D+", np.nextafter(hi, np.inf))):
        if r == v:
            return name
    return "inner" if r < lo else "shell" if r <= hi else "outside"


def _ex(rij, rik, p, mutate, tally, form):
    m, lam3 = p[0], p[2]
    if lam3 == 0.0:
        tally[form, "ex", "lam3=0"] += 1
        return 1.0, 0.0, "lam3=0"
    arg, darg = lam3 * (rij - rik), lam3
    kind = "m=1"
    if int(m) == 3:
        darg = 3.0 * lam3 * arg * arg
        arg = arg ** 3
        kind = "m=3"
    margin = abs(abs(arg) - CLAMP) / CLAMP
    tally["all", "margin", "ex"] = min(tally.get(("all", "margin", "ex"), np.inf), margin)
    if arg > CLAMP:
        tally[form, "ex", "high"] += 1
        tally[form, "ex", "high," + kind] += 1
        if mutate == "exp_unclamped":
            ex = math.exp(min(arg, 700.0))
            return ex, ex * darg, "high"
        return 1e30, (1e30 * darg if mutate == "dex_kept" else 0.0), "high"
    if arg < -CLAMP:
        tally[form, "ex", "low"] += 1
        tally[form, "ex", "low," + kind] += 1
        if mutate == "exp_unclamped":
            ex = math.exp(arg)
            return ex, ex * darg, "low"
        return 0.0, 0.0, "low"
    tally[form, "ex", kind] += 1
    ex = math.exp(arg)
    return ex, ex * darg, kind


def _bij(zeta, p, tally, form):
    n, beta = p[6], p[7]
    tmp = beta * zeta
    c1, c2 = (2.0 * n * 1e-16) ** (-1.0 / n), (2.0 * n * 1e-8) ** (-1.0 / n)
    c3, c4 = 1.0 / c2, 1.0 / c1
    if tmp > c1:
        tally[form, "bij", ">c1"] += 1
        return 1.0 / math.sqrt(tmp), beta * -0.5 * tmp ** -1.5, ">c1"
    if tmp > c2:
        tally[form, "bij", ">c2"] += 1
        return (1.0 - tmp ** -n / (2.0 * n)) / math.sqrt(tmp), beta * (-0.5 * tmp ** -1.5 * (1.0 - (1.0 + 1.0 / (2.0 * n)) * tmp ** -n)), ">c2"
    if tmp < c4:
        tally[form, "bij", "<c4"] += 1
        return 1.0, 0.0, "<c4"
    if tmp < c3:
        tally[form, "bij", "<c3"] += 1
        return 1.0 - tmp ** n / (2.0 * n), -0.5 * beta * tmp ** (n - 1.0), "<c3"
    branch = "n=1" if n == 1.0 else "general"
    tally[form, "bij", branch] += 1
    tn = tmp ** n
    return (1.0 + tn) ** (-1.0 / (2.0 * n)), -0.5 * (1.0 + tn) ** (-1.0 - 1.0 / (2.0 * n)) * tn / zeta, branch


def cutmax(P):
    P = np.asarray(P, float)
    return float((P[..., 10] + P[..., 11]).max())


def census(P, types, pos, cell, pbc, mutate=None):
    """Returns (E, forces [N, 3], tally)."""
    assert mutate is None or mutate in MUTATIONS
    P = np.asarray(P, float)
    types = np.asarray(types, np.int64)
    pos = np.asarray(pos, float).reshape(-1, 3)
    n = len(types)
    ei, ej, _, er = brute_neighbors(pos, cell, pbc, cutmax(P))       # d^2 <= rc^2, like the device rows
    start = np.searchsorted(ei, np.arange(n + 1))
    dist = np.sqrt((er * er).sum(axis=1))
    tally = Counter()
    E, F = 0.0, np.zeros((n, 3))
    for i in range(n):
        a, b = start[i], start[i + 1]
        form = "tile" if b - a <= TILE_SLOTS else "long"
        tally[form, "rows", "centres"] += 1
        ti = types[i]
        for e in range(a, b):
            j = ej[e]
            tj = types[j]
            pij = P[ti, tj, tj]
            r, rij = dist[e], er[e]
            R, D = pij[10], pij[11]
            tally[form, "fc_ij", fc_place(r, R, D)] += 1
            if r > R + D:
                continue
            fc, dfc = _fc(r, R, D)
            fR, fA = pij[13] * math.exp(-pij[12] * r), -pij[9] * math.exp(-pij[8] * r)
            zeta, terms, highs = 0.0, [], 0
            for e2 in range(a, b):
                if e2 == e:
                    continue
                pk = P[ti, tj, types[ej[e2]]]
                r2, rik = dist[e2], er[e2]
                tally[form, "fc_ik", fc_place(r2, pk[10], pk[11])] += 1
                if r2 > pk[10] + pk[11]:
                    continue
                cs = float(rij @ rik) / (r * r2)
                c2, d2, hc = pk[3] * pk[3], pk[4] * pk[4], pk[5] - cs
                den = d2 + hc * hc
                g, dg = pk[1] * (1.0 + c2 / d2 - c2 / den), pk[1] * (-2.0 * c2 * hc) / (den * den)
                ex, dex, path = _ex(r, r2, pk, mutate, tally, form)
                highs += path == "high"
                fck, dfck = _fc(r2, pk[10], pk[11])
                zeta += fck * g * ex
                terms.append((e2, r2, rik, cs, g, dg, ex, dex, fck, dfck))
            bij, dbij, branch = _bij(zeta, pij, tally, form)
            if highs:
                tally[form, "bij_after_high", branch] += 1
            E += 0.5 * fc * (fR + bij * fA)
            dV = 0.5 * (dfc * (fR + bij * fA) + fc * (-pij[12] * fR - pij[8] * bij * fA))
            pref = 0.5 * fc * fA * dbij
            gij = dV * rij / r
            for e2, r2, rik, cs, g, dg, ex, dex, fck, dfck in terms:
                k = ej[e2]
                dcs_j = (rik / r2 - cs * rij / r) / r
                dcs_k = (rij / r - cs * rik / r2) / r2
                gij = gij + pref * fck * (dg * dcs_j * ex + g * dex * rij / r)
                gik = pref * (dfck * rik / r2 * g * ex + fck * (dg * dcs_k * ex - g * dex * rik / r2))
                F[k] -= gik
                F[i] += gik
            F[j] -= gij
            F[i] += gij
    return E, F, tally


def by_form(tally, quantity, branch):
    return {form: tally.get((form, quantity, branch), 0) for form in ("tile", "long")}
