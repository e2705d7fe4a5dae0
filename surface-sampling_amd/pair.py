"""The LAMMPS pair commands of a template -> the term list and charges of a device pair potential (``vssr_pair_create``).

Read: ``pair_style`` (``lj/cut``, ``morse``, ``buck``, ``born``, ``coul/dsf``, ``coul/long``, ``buck/coul/long``,
``born/coul/long``, ``lj/cut/coul/long``, and ``hybrid`` / ``hybrid/overlay`` of these), ``pair_coeff`` with LAMMPS' type wildcards,
``pair_modify shift`` / ``mix``, ``set type N charge q``, ``kspace_style ewald A``, ``kspace_modify gewald G``, ``boundary`` and
``kspace_modify slab F``; every other command of the template is skipped.  Units are LAMMPS ``metal``.  Whatever cannot be read raises ``ValueError`` with the offending
line.

The ``*/coul/long`` styles become their short-range term plus a ``coul/long`` term (the real-space part of the Ewald sum, cutoff
``RC_COUL``) on EVERY type pair: the reciprocal sum runs over all charges.  ``kspace_style ewald A`` sets the model's ``kspace``:
L = sqrt(-ln A), g = L / rc, k_cut = 2 g L (``kspace_modify gewald G``: g = G).  This rule depends on (A, rc) only -- LAMMPS' own
estimator also looks at the atom count and the charges, which would change g between the proposals of a semigrand MC run -- so
energies agree with LAMMPS to the accuracy asked for, not digit for digit.

``kspace_modify slab F`` (F > 1) after a ``boundary p p f`` line sets ``kspace.slab``: the Ewald sum of the cell extended to F times
its height with the dipole correction of Yeh & Berkowitz, evaluated with pbc (1, 1, 0).  Without such a boundary line LAMMPS stops
("incorrect boundaries with slab Ewald") and so does ``parse``; ``slab nozforce`` and ``slab ew2d`` are not provided.
"""

from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

# style codes of include/vssr_eval.h (VSSR_PAIR_*), numbers after the type pair in a pair_coeff line, arguments in pair_style
STYLES = {"lj/cut": 1, "morse": 2, "buck": 3, "born": 4, "coul/dsf": 5, "coul/long": 6}
N_COEF = {"lj/cut": 2, "morse": 3, "buck": 3, "born": 5, "coul/dsf": 0, "coul/long": 0}
N_ARGS = {"lj/cut": 1, "morse": 1, "buck": 1, "born": 1, "coul/dsf": 2, "coul/long": 1}
# pair_style X/coul/long RC [RC_COUL]: the short-range style X with cutoff RC plus coul/long with cutoff RC_COUL (default RC)
COMPOSITE = {"buck/coul/long": "buck", "born/coul/long": "born", "lj/cut/coul/long": "lj/cut"}
PAIR_STYLES = (*STYLES, *COMPOSITE, "hybrid", "hybrid/overlay")
MAX_TYPES, MAX_TERMS = 8, 3
QQRD2E = 14.399645

Term = namedtuple("Term", "type_a type_b style c rc shift")      # 0-based types with a <= b, style code, c [5], cutoff, 0 / 1
# charges: [n_types] or None (no ``set type ... charge``); kspace: None, or the Ewald sum behind the coul/long terms
PairModel = namedtuple("PairModel", "n_types terms charges cutoff kspace", defaults=(None,))
# relative accuracy A asked for, damping g and reciprocal cutoff (1 / A), slab factor F of kspace_modify slab (0.0: periodic in three directions)
KSpace = namedtuple("KSpace", "accuracy g_ewald k_cut slab", defaults=(0.0,))


def ewald_defaults(accuracy, rc, g_ewald=None, k_cut=None, slab=0.0) -> KSpace:
    """``kspace_style ewald A`` with the real-space cutoff ``rc``: L = sqrt(-ln A), g = L / rc, k_cut = 2 g L unless given;
    ``slab``: the factor of ``kspace_modify slab`` (0.0: none)."""
    if not (0.0 < accuracy < 1.0):
        raise ValueError(f"kspace accuracy {accuracy} must lie in (0, 1)")
    L = math.sqrt(-math.log(accuracy))
    g = L / rc if g_ewald is None else float(g_ewald)
    kc = 2.0 * g * L if k_cut is None else float(k_cut)
    if not (math.isfinite(g) and g > 0 and math.isfinite(kc) and kc > 0):
        raise ValueError(f"k-space parameters g_ewald {g}, k_cut {kc} must be finite and > 0")
    slab = float(slab)
    if slab != 0.0 and not (math.isfinite(slab) and slab > 1.0):
        raise ValueError(f"slab factor {slab} must be finite and > 1.0 (0.0: no slab correction)")
    return KSpace(float(accuracy), g, kc, slab)


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
    if tok[0] in COMPOSITE:
        if len(tok) - 1 not in (1, 2):
            raise ValueError(f"{line!r}: pair_style {tok[0]} takes the cutoff and an optional Coulomb cutoff")
        return "single", {tok[0]: [_number(t, line, "argument") for t in tok[1:]]}
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
        if name not in STYLES and name not in COMPOSITE:
            raise ValueError(f"{line!r}: sub-style {name!r} is not a pair style of this kind ({', '.join(STYLES)}); "
                             "mixing with the many-body potentials is not provided")
        if name in subs:
            raise ValueError(f"{line!r}: sub-style {name} appears twice (numbered sub-styles are not provided)")
        if name in COMPOSITE:   # one or two numbers: whatever follows up to the next sub-style
            n_args = 1 + (k + 2 < len(tok) and tok[k + 2] not in STYLES and tok[k + 2] not in COMPOSITE)
        else:
            n_args = N_ARGS[name]
        args = tok[k + 1:k + 1 + n_args]
        if len(args) != n_args:
            raise ValueError(f"{line!r}: sub-style {name} takes {n_args} argument(s)")
        subs[name] = [_number(t, line, "argument") for t in args]
        k += 1 + n_args
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
    mode, subs, style_line = None, None, None
    coeff = {}            # (i, j) 1-based, i <= j -> {sub-style: (coefficients, cutoff)} in assignment order
    none = set()          # pairs a hybrid line switched off (pair_coeff i j none)
    shift, mix = 0, "geometric"
    charges, has_charge = np.zeros(n_types), False
    accuracy, gewald, boundary, slab = None, None, None, 0.0
    for line in _commands(lines):
        tok = line.split()
        cmd = tok[0]
        if cmd == "pair_style":
            mode, subs, style_line = *_parse_style(tok[1:], line), line
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
            nc = N_COEF[COMPOSITE.get(name, name)]
            coul = name in ("coul/dsf", "coul/long")
            if len(rest) not in ((nc,) if coul else (nc, nc + 1)):
                raise ValueError(f"{line!r}: {name} takes {nc} coefficient(s)" + ("" if coul else " and an optional cutoff"))
            c = tuple(_number(t, line, "coefficient") for t in rest[:nc])
            # (the optional cutoff of a */coul/long line is that of the short-range part, as in LAMMPS)
            rc = _number(rest[nc], line, "cutoff") if len(rest) > nc else subs[name][0 if name in COMPOSITE else -1]
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
        elif cmd == "kspace_style":
            if len(tok) != 3 or tok[1] != "ewald":
                raise ValueError(f"{line!r}: only 'kspace_style ewald ACCURACY' is provided (no pppm, msm, ewald/disp, ...)")
            accuracy = _number(tok[2], line, "accuracy")
            if not 0.0 < accuracy < 1.0:
                raise ValueError(f"{line!r}: the accuracy must lie in (0, 1)")
        elif cmd == "kspace_modify":
            if len(tok) == 3 and tok[1] == "gewald":
                gewald = _number(tok[2], line, "gewald")
                if not gewald > 0:
                    raise ValueError(f"{line!r}: gewald must be > 0")
            elif len(tok) > 1 and tok[1] == "slab":
                if boundary != ["p", "p", "f"]:
                    raise ValueError(f"{line!r}: the slab correction needs a 'boundary p p f' line before it (incorrect boundaries with "
                                     "slab Ewald); without one the Ewald sum is periodic in three directions")
                if len(tok) != 3 or tok[2] in ("nozforce", "ew2d"):
                    raise ValueError(f"{line!r}: only 'kspace_modify slab F' with a number F > 1.0 is provided (no nozforce, no ew2d)")
                slab = _number(tok[2], line, "slab factor")
                if not slab > 1.0:
                    raise ValueError(f"{line!r}: bad slab parameter: the slab factor must be > 1.0")
            else:
                raise ValueError(f"{line!r}: kspace_modify {' '.join(tok[1:])!r} is not provided (gewald G)")
        elif cmd == "boundary":
            boundary = tok[1:]
            if boundary != ["p", "p", "f"] and slab:
                raise ValueError(f"{line!r}: incorrect boundaries with slab Ewald (kspace_modify slab needs 'boundary p p f')")
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
            for lj in ("lj/cut", "lj/cut/coul/long"):
                if di is not None and dj is not None and list(di) == [lj] and list(dj) == [lj]:
                    coeff[(i, j)] = {lj: _mix_lj(di[lj], dj[lj], mix)}
    unset = [(i, j) for i in range(1, n_types + 1) for j in range(i, n_types + 1) if (i, j) not in coeff and (i, j) not in none]
    if unset:
        raise ValueError("All pair coeffs are not set: " + ", ".join(f"{i} {j}" for i, j in unset)
                         + " (only lj/cut mixes; morse, buck and born need explicit i j lines)")
    # the Ewald sum: one real-space cutoff, coul/long on every type pair, kspace_style given
    long_rc = sorted({subs[n][-1] for n in subs if n in COMPOSITE or n == "coul/long"})
    if len(long_rc) > 1:
        raise ValueError(f"the coul/long sub-styles differ in their Coulomb cutoff ({', '.join(map(str, long_rc))}): one Ewald sum has one")
    if long_rc and accuracy is None:
        raise ValueError(f"{style_line!r}: pair style requires a KSpace style: a */coul/long pair_style needs 'kspace_style ewald ACCURACY'")
    if accuracy is not None and not long_rc:
        raise ValueError("kspace_style ewald without a */coul/long pair_style (KSpace style is incompatible with Pair style)")
    if long_rc and "coul/dsf" in subs:
        raise ValueError("coul/dsf next to a */coul/long style: one Coulomb sum at a time")
    if long_rc and not has_charge:
        raise ValueError("a */coul/long pair_style needs charges ('set type N charge q')")
    if "coul/long" in subs:
        bare = [(i, j) for i in range(1, n_types + 1) for j in range(i, n_types + 1) if "coul/long" not in coeff.get((i, j), {})]
        if bare and not any(n in COMPOSITE for n in subs):
            raise ValueError("coul/long must cover every type pair (pair_coeff * * coul/long): the reciprocal sum runs over all charges; "
                             "missing " + ", ".join(f"{i} {j}" for i, j in bare))
    terms = []
    for (i, j) in sorted(set(coeff) | ({(i, j) for i in range(1, n_types + 1) for j in range(i, n_types + 1)} if long_rc else set())):
        entry = coeff.get((i, j), {})
        if len(entry) - ("coul/long" in entry) + bool(long_rc) > MAX_TERMS:
            raise ValueError(f"type pair {i} {j} carries {len(entry)} sub-styles ({MAX_TERMS} at the most)")
        for name in subs:                      # the order of the pair_style line
            if name not in entry or name == "coul/long":
                continue
            c, rc = entry[name]
            if name == "coul/dsf":
                c = (subs[name][0],)           # alpha
            if not rc > 0:
                raise ValueError(f"type pair {i} {j}, {name}: cutoff {rc} must be > 0")
            terms.append(Term(i - 1, j - 1, STYLES[COMPOSITE.get(name, name)], tuple(c) + (0.0,) * (5 - len(c)), float(rc),
                              0 if name == "coul/dsf" else shift))
        if long_rc:                            # last on every pair, 'none' pairs included
            if not long_rc[0] > 0:
                raise ValueError(f"coul/long: cutoff {long_rc[0]} must be > 0")
            terms.append(Term(i - 1, j - 1, STYLES["coul/long"], (0.0,) * 5, float(long_rc[0]), 0))
    if not terms:
        raise ValueError("every type pair is 'none': nothing to evaluate")
    if slab and not long_rc:
        raise ValueError("kspace_modify slab without a */coul/long pair_style and kspace_style ewald")
    kspace = ewald_defaults(accuracy, long_rc[0], g_ewald=gewald, slab=slab) if long_rc else None
    return PairModel(n_types, terms, charges if has_charge else None, max(t.rc for t in terms), kspace)
