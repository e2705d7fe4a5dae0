"""LAMMPS ``pair_style vashishta`` potential-file parsing and the built-in named parameter sets (host side, data only).

Entries are ``e1 e2 e3  H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta`` and may span lines; ``#`` starts a comment.
e1 = centre atom i, e2 = bonded atom j, e3 = third atom k.  The two-body term and the radial factor of r_ij use entry (i, j, j);
B, C and costheta of the three-body term come from (i, j, k).  The two-body columns of an entry with j != k are read by nobody:
they only have to be finite (published files write zeros there).

``MODELS`` holds the SiC set of Vashishta, Kalia, Nakano and Rino, J. Appl. Phys. 101, 103515 (2007), written as LAMMPS writes it.
"""

from __future__ import annotations

import numpy as np

N_VASHISHTA_FIELDS = 14
FIELD_NAMES = ("H", "eta", "Zi", "Zj", "lambda1", "D", "lambda4", "W", "rc", "B", "gamma", "r0", "C", "costheta")
PAIR_FIELDS = (0, 1, 4, 5, 6, 7, 8)          # H eta lambda1 D lambda4 W rc: (i, j, j) and (j, i, i) must agree (and in Zi Zj)
TRIPLET_FIELDS = (9, 12, 13)                 # B C costheta: (i, j, k) and (i, k, j) must agree

# name -> (species in type order, .vashishta text)
MODELS = {
    "SiC_Vashishta_2007": (
        ("C", "Si"),
        "# Vashishta, Kalia, Nakano and Rino, J. Appl. Phys. 101, 103515 (2007)\n"
        "# e1 e2 e3  H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta\n"
        "C  C  C   471.74538 7 -1.201 -1.201 5.0 0.0    3.0 0.0     7.35 0.0   0.0 0.0  0.0  0.0\n"
        "Si Si Si  23.67291  7  1.201  1.201 5.0 15.575 3.0 0.0     7.35 0.0   0.0 0.0  0.0  0.0\n"
        "C  Si Si  447.09026 9 -1.201  1.201 5.0 7.7874 3.0 61.4694 7.35 9.003 1.0 2.90 5.0 -0.333333333333\n"
        "Si C  C   447.09026 9  1.201 -1.201 5.0 7.7874 3.0 61.4694 7.35 9.003 1.0 2.90 5.0 -0.333333333333\n"
        "C  C  Si  0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0 7.35 0.0 0.0 0.0 0.0 0.0\n"
        "C  Si C   0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0 7.35 0.0 0.0 0.0 0.0 0.0\n"
        "Si Si C   0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0 7.35 0.0 0.0 0.0 0.0 0.0\n"
        "Si C  Si  0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0 7.35 0.0 0.0 0.0 0.0 0.0\n"),
}


def is_builtin(name) -> bool:
    return isinstance(name, str) and name in MODELS


def builtin_text(name: str) -> str:
    return MODELS[str(name)][1]


def builtin_species(name: str) -> list[str]:
    return list(MODELS[str(name)][0])


def parse_vashishta(text: str, species: list[str]) -> np.ndarray:
    """Return params[nt, nt, nt, 14] (float64) for the given species order (LAMMPS type order).  Raises ``ValueError`` naming the
    entry / field on malformed text, missing triplets and on everything ``check_params`` refuses."""
    species = list(species)
    if not species or len(set(species)) != len(species):
        raise ValueError(f"vashishta: species must be distinct and non-empty, got {species}")
    tokens: list[str] = []
    for raw in text.splitlines():
        line = raw.split("#", 1)[0].strip()
        if line:
            tokens += line.split()
    per = 3 + N_VASHISHTA_FIELDS
    if not tokens or len(tokens) % per:
        raise ValueError(f"vashishta file: {len(tokens)} tokens, not a multiple of {per} (e1 e2 e3 + 14 numbers)")
    nt = len(species)
    idx = {s: t for t, s in enumerate(species)}
    params = np.full((nt, nt, nt, N_VASHISHTA_FIELDS), np.nan)
    seen = np.zeros((nt, nt, nt), bool)
    for o in range(0, len(tokens), per):
        e1, e2, e3 = tokens[o:o + 3]
        if e1 in idx and e2 in idx and e3 in idx:
            vals = []
            for name, x in zip(FIELD_NAMES, tokens[o + 3:o + per]):
                try:
                    vals.append(float(x))
                except ValueError:
                    raise ValueError(f"vashishta file: entry {e1} {e2} {e3}: bad number {x!r} for {name}") from None
            params[idx[e1], idx[e2], idx[e3]] = vals
            seen[idx[e1], idx[e2], idx[e3]] = True
    if not seen.all():
        a, b, c = np.argwhere(~seen)[0]
        raise ValueError(f"vashishta file lacks the entry {species[a]} {species[b]} {species[c]}")
    check_params(params, species)
    return params


def check_params(params: np.ndarray, species: list[str] | None = None) -> None:
    """The checks of ``vssr_vashishta_create`` on the host (same rules, messages name the entry and the field): non-finite numbers
    and negative B / gamma / r0 in any entry; in the entries (i, j, j): rc <= 0, eta <= 0, lambda1 <= 0 with Zi Zj != 0, lambda4 <= 0
    with D != 0, r0 > rc; (i, j, j) / (j, i, i) that differ in a two-body column; (i, j, k) / (i, k, j) that differ in B, C, costheta."""
    P = np.asarray(params, dtype=np.float64)
    if P.ndim != 4 or P.shape != (P.shape[0],) * 3 + (N_VASHISHTA_FIELDS,) or not 1 <= P.shape[0] <= 8:
        raise ValueError("vashishta params must be [nt, nt, nt, 14] with 1 <= nt <= 8 (at most 8 species)")
    nt = P.shape[0]
    sp = list(species) if species is not None else [str(t) for t in range(nt)]

    def bad(i, j, k, f, rule):
        return ValueError(f"vashishta entry {sp[i]} {sp[j]} {sp[k]}: bad {FIELD_NAMES[f]} = {float(P[i, j, k, f])!r} ({rule})")

    for i in range(nt):
        for j in range(nt):
            for k in range(nt):
                p = P[i, j, k]
                for f in range(N_VASHISHTA_FIELDS):
                    if not np.isfinite(p[f]):
                        raise bad(i, j, k, f, "must be finite")
                for f in (9, 10, 11):
                    if not p[f] >= 0:
                        raise bad(i, j, k, f, "must be >= 0")
                if j != k:
                    continue
                if not p[8] > 0:
                    raise bad(i, j, k, 8, "must be > 0")
                if not p[1] > 0:
                    raise bad(i, j, k, 1, "must be > 0")
                if p[2] * p[3] != 0.0 and not p[4] > 0:
                    raise bad(i, j, k, 4, "must be > 0 with Zi Zj != 0")
                if p[5] != 0.0 and not p[6] > 0:
                    raise bad(i, j, k, 6, "must be > 0 with D != 0")
                if p[11] > p[8]:
                    raise bad(i, j, k, 11, "must be <= rc")
    for i in range(nt):
        for j in range(i + 1, nt):
            a, b = P[i, j, j], P[j, i, i]
            for f in PAIR_FIELDS:
                if a[f] != b[f]:
                    raise ValueError(f"vashishta entries {sp[i]} {sp[j]} {sp[j]} and {sp[j]} {sp[i]} {sp[i]} differ in {FIELD_NAMES[f]}: "
                                     "the two-body term would depend on neighbor order")
            if a[2] * a[3] != b[2] * b[3]:
                raise ValueError(f"vashishta entries {sp[i]} {sp[j]} {sp[j]} and {sp[j]} {sp[i]} {sp[i]} differ in Zi Zj: "
                                 "the two-body term would depend on neighbor order")
    for f in TRIPLET_FIELDS:
        d = P[:, :, :, f] != np.swapaxes(P[:, :, :, f], 1, 2)
        if d.any():
            i, j, k = np.argwhere(d)[0]
            raise ValueError(f"vashishta entries {sp[i]} {sp[j]} {sp[k]} and {sp[i]} {sp[k]} {sp[j]} differ in {FIELD_NAMES[f]}: "
                             "the three-body term would depend on neighbor order")


def max_cutoff(params: np.ndarray) -> float:
    """The largest rc of the entries (i, j, j): the cutoff of the neighbor list."""
    P = np.asarray(params, dtype=np.float64)
    n = np.arange(P.shape[0])
    return float(P[:, n, n, 8].max())
