"""The LAMMPS pair commands of a template -> the term list and charges of a device pair potential (``vssr_pair_create``).

Read: ``pair_style`` (``lj/cut``, ``morse``, ``buck``, ``born``, ``coul/dsf``, and ``hybrid`` / ``hybrid/overlay`` of these),
``pair_coeff`` with LAMMPS' type wildcards, ``pair_modify shift`` / ``mix`` and ``set type N charge q``; every other command of the
template is skipped.  Units are LAMMPS ``metal``.  Whatever cannot be read raises ``ValueError`` with the offending line.
"""

from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

# style codes of include/vssr_eval.h (VSSR_PAIR_*), numbers after the type pair in a pair_coeff line, arguments in pair_style
STYLES = {"lj/cut": 1, "morse": 2, "buck": 3, "born": 4, "coul/dsf": 5}
N_COEF = {"lj/cut": 2, "morse": 3, "buck": 3, "born": 5, "coul/dsf": 0}
N_ARGS = {"lj/cut": 1, "morse": 1, "buck": 1, "born": 1, "coul/dsf": 2}
PAIR_STYLES = (*STYLES, "hybrid", "hybrid/overlay")
MAX_TYPES, MAX_TERMS = 8, 3
QQRD2E = 14.399645

Term = namedtuple("Term", "type_a type_b style c rc shift")      # 0-based types with a <= b, style code, c [5], cutoff, 0 / 1
PairModel = namedtuple("PairModel", "n_types terms charges cutoff")   # charges: [n_types] or None (no ``set type ... charge``)


def _number(tok, line, what):
    try:
        x = float(tok)
    except ValueError:
        raise ValueError(f"{line!r}: {what} {tok!r} is not a number") from None
    if not math.isfinite(x):
        raise ValueError(f"{line!r}: {what} {tok!r} is not finite")
    return x


def type_range(tok, n_types, line=""):
    """LAMMPS type field ``n``, ``*``, ``n*``, ``*n`` or ``m*n`` -> inclusive 1-based (lo, hi)."""
    try:
        if "*" not in tok:
            lo = hi = int(tok)
        else:
            a, b = tok.split("*", 1)
            lo = int(a) if a else 1
            hi = int(b) if b else n_types
    except ValueError:
        raise ValueError(f"{line!r}: bad type field {tok!r}") from None
    if lo < 1 or hi > n_types or lo > hi:
        raise ValueError(f"{line!r}: type field {tok!r} outside 1 .. {n_types}")
    return lo, hi


def _commands(lines):
    if isinstance(lines, str):
        lines = lines.splitlines()
    out, held = [], ""
    for raw in lines:
        ln = held + str(raw).split("#", 1)[0].rstrip()
        if ln.endswith("&"):
            held = ln[:-1] + " "
            continue
        held = ""
        if ln.strip():
            out.append(ln.strip())
    if held.strip():
        out.append(held.strip())
    return out


def _parse_style(tok, line):
    """``pair_style`` arguments -> (mode, {sub-style: its arguments}) with mode "single", "hybrid" or "overlay"."""
    if not tok:
        raise ValueError(f"{line!r}: pair_style without a style")
    if tok[0] not in ("hybrid", "hybrid/overlay"):
        if tok[0] not in STYLES:
            raise ValueError(f"{line!r}: pair_style {tok[0]!r} is not a pair style of this kind ({', '.join(STYLES)})")
        if len(tok) - 1 != N_ARGS[tok[0]]:
            raise ValueError(f"{line!r}: pair_style {tok[0]} takes {N_ARGS[tok[0]]} argument(s) "
                             f"({'alpha cutoff' if tok[0] == 'coul/dsf' else 'the global cutoff'})")
        return "single", {tok[0]: [_number(t, line, "argument") for t in tok[1:]]}
    subs, k = {}, 1
    while k < len(tok):
        name = tok[k]
        if name not in STYLES:
            raise ValueError(f"{line!r}: sub-style {name!r} is not a pair style of this kind ({', '.join(STYLES)}); "
                             "mixing with the many-body potentials is not provided")
        if name in subs:
            raise ValueError(f"{line!r}: sub-style {name} appears twice (numbered sub-styles are not provided)")
        args = tok[k + 1:k + 1 + N_ARGS[name]]
        if len(args) != N_ARGS[name]:
            raise ValueError(f"{line!r}: sub-style {name} takes {N_ARGS[name]} argument(s)")
        subs[name] = [_number(t, line, "argument") for t in args]
        k += 1 + N_ARGS[name]
    if not subs:
        raise ValueError(f"{line!r}: {tok[0]} without sub-styles")
    return ("hybrid" if tok[0] == "hybrid" else "overlay"), subs


def _mix_lj(ci, cj, rule):
    (ei, si), ri = ci
    (ej, sj), rj = cj
    if rule == "arithmetic":       # Lorentz-Berthelot
        return (math.sqrt(ei * ej), 0.5 * (si + sj)), 0.5 * (ri + rj)
    return (math.sqrt(ei * ej), math.sqrt(si * sj)), math.sqrt(ri * rj)


def parse(lines, n_types) -> PairModel:
    """The pair commands among ``lines`` (a text or its lines) for ``n_types`` LAMMPS atom types."""
    n_types = int(n_types)
    if not 1 <= n_types <= MAX_TYPES:
        raise ValueError(f"{n_types} atom types (1 .. {MAX_TYPES} are supported)")
    mode, subs = None, None
    coeff = {}            # (i, j) 1-based, i <= j -> {sub-style: (coefficients, cutoff)} in assignment order
    none = set()          # pairs a hybrid line switched off (pair_coeff i j none)
    shift, mix = 0, "geometric"
    charges, has_charge = np.zeros(n_types), False
    for line in _commands(lines):
        tok = line.split()
        cmd = tok[0]
        if cmd == "pair_style":
            mode, subs = _parse_style(tok[1:], line)
            coeff.clear(); none.clear()
        elif cmd == "pair_coeff":
            if mode is None:
                raise ValueError(f"{line!r}: pair_coeff before pair_style")
            if len(tok) < 3:
                raise ValueError(f"{line!r}: expected 'pair_coeff I J ...'")
            (ilo, ihi), (jlo, jhi) = type_range(tok[1], n_types, line), type_range(tok[2], n_types, line)
            rest = tok[3:]
            if mode == "single":
                name = next(iter(subs))
            else:
                if not rest:
                    raise ValueError(f"{line!r}: a {'hybrid' if mode == 'hybrid' else 'hybrid/overlay'} pair_coeff names its sub-style")
                name, rest = rest[0], rest[1:]
                if name != "none" and name not in subs:
                    raise ValueError(f"{line!r}: sub-style {name!r} is not in the pair_style line ({', '.join(subs)})")
            pairs = [(i, j) for i in range(ilo, ihi + 1) for j in range(max(jlo, i), jhi + 1)]
            if not pairs:
                raise ValueError(f"{line!r}: no type pair with I <= J")
            if name == "none":
                if rest:
                    raise ValueError(f"{line!r}: 'none' takes no coefficients")
                for p in pairs:
                    coeff.pop(p, None)
                    none.add(p)
                continue
            nc = N_COEF[name]
            if len(rest) not in ((nc,) if name == "coul/dsf" else (nc, nc + 1)):
                raise ValueError(f"{line!r}: {name} takes {nc} coefficient(s)" + ("" if name == "coul/dsf" else " and an optional cutoff"))
            c = tuple(_number(t, line, "coefficient") for t in rest[:nc])
            rc = _number(rest[nc], line, "cutoff") if len(rest) > nc else subs[name][-1]
            for p in pairs:
                none.discard(p)
                if mode == "hybrid":
                    coeff[p] = {name: (c, rc)}
                else:
                    coeff.setdefault(p, {})[name] = (c, rc)
        elif cmd == "pair_modify":
            k = 1
            while k < len(tok):
                if tok[k] == "shift" and k + 1 < len(tok) and tok[k + 1] in ("yes", "no"):
                    shift = int(tok[k + 1] == "yes")
                elif tok[k] == "mix" and k + 1 < len(tok) and tok[k + 1] in ("geometric", "arithmetic"):
                    mix = tok[k + 1]
                else:
                    raise ValueError(f"{line!r}: pair_modify {' '.join(tok[k:k + 2])!r} is not provided (shift yes|no, mix geometric|arithmetic)")
                k += 2
        elif cmd == "set" and "charge" in tok:
            if len(tok) != 5 or tok[1] != "type" or tok[3] != "charge":
                raise ValueError(f"{line!r}: charges are per type ('set type N charge q')")
            lo, hi = type_range(tok[2], n_types, line)
            charges[lo - 1:hi] = _number(tok[4], line, "charge")
            has_charge = True
    if mode is None:
        raise ValueError("no pair_style command")
    # mixing: lj/cut only, for pairs no line touched whose two types carry lj/cut (and nothing else) on their diagonal
    for i in range(1, n_types + 1):
        for j in range(i + 1, n_types + 1):
            if (i, j) in coeff or (i, j) in none:
                continue
            di, dj = coeff.get((i, i)), coeff.get((j, j))
            if di is not None and dj is not None and list(di) == ["lj/cut"] and list(dj) == ["lj/cut"]:
                coeff[(i, j)] = {"lj/cut": _mix_lj(di["lj/cut"], dj["lj/cut"], mix)}
    unset = [(i, j) for i in range(1, n_types + 1) for j in range(i, n_types + 1) if (i, j) not in coeff and (i, j) not in none]
    if unset:
        raise ValueError("All pair coeffs are not set: " + ", ".join(f"{i} {j}" for i, j in unset)
                         + " (only lj/cut mixes; morse, buck and born need explicit i j lines)")
    terms = []
    for (i, j) in sorted(coeff):
        entry = coeff[(i, j)]
        if len(entry) > MAX_TERMS:
            raise ValueError(f"type pair {i} {j} carries {len(entry)} sub-styles ({MAX_TERMS} at the most)")
        for name in subs:                      # the order of the pair_style line
            if name not in entry:
                continue
            c, rc = entry[name]
            if name == "coul/dsf":
                c = (subs[name][0],)           # alpha
            if not rc > 0:
                raise ValueError(f"type pair {i} {j}, {name}: cutoff {rc} must be > 0")
            terms.append(Term(i - 1, j - 1, STYLES[name], tuple(c) + (0.0,) * (5 - len(c)), float(rc), 0 if name == "coul/dsf" else shift))
    if not terms:
        raise ValueError("every type pair is 'none': nothing to evaluate")
    return PairModel(n_types, terms, charges if has_charge else None, max(t.rc for t in terms))
