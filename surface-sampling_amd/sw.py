"""LAMMPS ``pair_style sw`` (Stillinger-Weber) potential-file parsing and the built-in named parameter sets (host side, data only).

Entries are ``e1 e2 e3  eps sig a lambda gamma costheta0 A B p q tol`` and may span lines; ``#`` starts a comment.  e1 = centre
atom i, e2 = bonded atom j, e3 = third atom k.  The two-body term and the radial factor of r_ij use entry (i, j, j); lambda, eps
and costheta0 of the three-body term come from (i, j, k).  ``tol`` is read and has no effect on the result.

The reference's Si(111) 5x5 run directory names the OpenKIM model ``SW_StillingerWeber_1985_Si__MO_405512056662_005`` (``pair_style
kim``); its parameters are the published 1985 silicon values (Stillinger and Weber, Phys. Rev. B 31, 5262), held in ``MODELS``.
"""

from __future__ import annotations

import numpy as np

N_SW_FIELDS = 11
FIELD_NAMES = ("eps", "sig", "a", "lambda", "gamma", "costheta0", "A", "B", "p", "q", "tol")

# name -> (species in type order, .sw text)
MODELS = {
    "SW_StillingerWeber_1985_Si__MO_405512056662_005": (
        ("Si",),
        "# Stillinger and Weber, Phys. Rev. B 31, 5262 (1985)\n"
        "Si Si Si 2.1683 2.0951 1.80 21.0 1.20 -0.3333333333333333 7.049556277 0.6022245584 4.0 0.0 0.0\n"),
}


def is_builtin(name: str) -> bool:
    return str(name) in MODELS


def builtin_text(name: str) -> str:
    return MODELS[str(name)][1]


def builtin_species(name: str) -> list[str]:
    return list(MODELS[str(name)][0])


def parse_sw(text: str, species: list[str]) -> np.ndarray:
    """Return params[nt, nt, nt, 11] (float64) for the given species order (LAMMPS type order).  Raises ``ValueError`` naming the
    entry / field on malformed text, missing triplets, bad numbers (eps, sig, a must be > 0; lambda, gamma, A, B, p, q, tol >= 0)
    and on (i, j, k) / (i, k, j) entries that differ in eps, lambda or costheta0."""
    species = list(species)
    if not species or len(set(species)) != len(species):
        raise ValueError(f"sw: species must be distinct and non-empty, got {species}")
    tokens: list[str] = []
    for raw in text.splitlines():
        line = raw.split("#", 1)[0].strip()
        if line:
            tokens += line.split()
    per = 3 + N_SW_FIELDS
    if not tokens or len(tokens) % per:
        raise ValueError(f"sw file: {len(tokens)} tokens, not a multiple of {per} (e1 e2 e3 + 11 numbers)")
    nt = len(species)
    idx = {s: t for t, s in enumerate(species)}
    params = np.full((nt, nt, nt, N_SW_FIELDS), np.nan)
    seen = np.zeros((nt, nt, nt), bool)
    for o in range(0, len(tokens), per):
        e1, e2, e3 = tokens[o:o + 3]
        if e1 in idx and e2 in idx and e3 in idx:
            vals = []
            for name, x in zip(FIELD_NAMES, tokens[o + 3:o + per]):
                try:
                    vals.append(float(x))
                except ValueError:
                    raise ValueError(f"sw file: entry {e1} {e2} {e3}: bad number {x!r} for {name}") from None
            params[idx[e1], idx[e2], idx[e3]] = vals
            seen[idx[e1], idx[e2], idx[e3]] = True
    if not seen.all():
        a, b, c = np.argwhere(~seen)[0]
        raise ValueError(f"sw file lacks the entry {species[a]} {species[b]} {species[c]}")
    check_params(params, species)
    return params


def check_params(params: np.ndarray, species: list[str] | None = None) -> None:
    """The checks of ``vssr_sw_create`` on the host (same rules, messages name the entry)."""
    P = np.asarray(params, dtype=np.float64)
    if P.ndim != 4 or P.shape != (P.shape[0],) * 3 + (N_SW_FIELDS,) or not 1 <= P.shape[0] <= 8:
        raise ValueError("sw params must be [nt, nt, nt, 11] with 1 <= nt <= 8")
    nt = P.shape[0]
    sp = list(species) if species is not None else [str(t) for t in range(nt)]
    for i in range(nt):
        for j in range(nt):
            for k in range(nt):
                for f, name in enumerate(FIELD_NAMES):
                    x = float(P[i, j, k, f])
                    pos, free = f in (0, 1, 2), f == 5
                    if not np.isfinite(x) or (pos and not x > 0) or (not pos and not free and not x >= 0):
                        rule = "must be > 0" if pos else "must be finite" if free else "must be >= 0"
                        raise ValueError(f"sw entry {sp[i]} {sp[j]} {sp[k]}: bad {name} = {x!r} ({rule})")
    for f in (0, 3, 5):
        d = P[:, :, :, f] != np.swapaxes(P[:, :, :, f], 1, 2)
        if d.any():
            i, j, k = np.argwhere(d)[0]
            raise ValueError(f"sw entries {sp[i]} {sp[j]} {sp[k]} and {sp[i]} {sp[k]} {sp[j]} differ in {FIELD_NAMES[f]}: "
                             "the three-body term would depend on neighbor order")


def max_cutoff(params: np.ndarray) -> float:
    return float((params[..., 1] * params[..., 2]).max())
