"""BFGSLineSearch in numpy: the contract of the device optimizer (csrc/bfgsls_dev.h, vssr_batch_relax_bfgs_linesearch).  TEST
INFRASTRUCTURE.

PROVENANCE.  Restated from ASE's ``ase/optimize/bfgslinesearch.py`` and ``ase/utils/linesearch.py`` AS REMEMBERED.  ASE cannot be
installed next to this project, so this restatement is NOT pinned by an executed ASE (tests/test_bfgsls_cpu.py compares with the real
class where ``ase.optimize`` happens to be importable, and skips elsewhere).  The interpolation routine is MINPACK-2 ``dcstep``; the
restatement CALLS ``scipy.optimize._dcsrch.dcstep``, an independent statement of it.

Like ASE it keeps the dense inverse Hessian ``H`` (the device never stores it: two-loop recursion over the accepted triples,
``two_loop`` below restates that).  Vectors run over all 3 N coordinates; entries of held atoms are zero: their force is zeroed and
they never move.  ``force_fn(pos [N, 3]) -> (E, F [N, 3])``.

Two things ASE does not have: ``max_eval``, an evaluation budget (stop reason 4 at the best point ``r + stx p`` of the interrupted
search), and the stop at a non-finite energy or force (reason 5, at ``r``).  Where ASE raises ``RuntimeError("LineSearch failed!")``
the restatement stops with reason 3 at ``r``.  Stop reasons: 1 converged, 2 max_steps, 3 line search failed, 4 max_eval, 5 non-finite.

The tracer records, per run, every branch taken (``Trace.branches``: a name -> count) and the smallest relative margin of every
comparison that decided something (``Trace.margin``): |a - b| / max(|a|, |b|, tiny).  Count parity between this restatement and the
device is meaningful only where those margins are far above round-off (class ``exact`` of tests/bfgsls_cases.py: > 1e-7)."""

import numpy as np
from scipy.optimize._dcsrch import dcstep

DEFAULTS = dict(alpha=10.0, maxstep=0.2, c1=0.23, c2=0.46, stpmax=50.0)
STPMIN, XTOL, XTRAPL, XTRAPU = 1e-8, 1e-14, 1.1, 4.0


class Trace:
    def __init__(self):
        self.branches = {}
        self.margin = np.inf
        self.margin_at = None
        self.steps = []       # per accepted step: dict(stp, phi0, dphi0, phi, dphi)  (the Wolfe tests)
        self.trials = []      # per evaluation: (kind "open" | "trial", positions)
        self.energies = []    # energy at every step-open
        self.two_loop_err = 0.0

    def hit(self, name):
        self.branches[name] = self.branches.get(name, 0) + 1

    def cmp(self, a, b, what):
        """Record the relative margin of the comparison of a with b."""
        m = abs(a - b) / max(abs(a), abs(b), 1e-300)
        if m < self.margin:
            self.margin, self.margin_at = m, what


class _NoTrace:
    steps = trials = energies = None

    def hit(self, name):
        pass

    def cmp(self, a, b, what):
        pass


def two_loop(g, hist):
    """H g for H built from H0 = I by the product-form updates of ``hist`` = [(dr, dg, rho)], with the STORED rho."""
    q = g.copy()
    a = []
    for dr, dg, rho in reversed(hist):
        ai = rho * np.dot(dr, q)
        a.append(ai)
        q -= ai * dg
    for (dr, dg, rho), ai in zip(hist, reversed(a)):
        bi = rho * np.dot(dg, q)
        q += dr * (ai - bi)
    return q


def dcstep_traced(stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax, tr):
    """MINPACK-2 dcstep written out once more, only so that the tracer sees the comparisons INSIDE it (a near tie between the cubic and
    the quadratic step flips the trial discontinuously).  Returns (case 1..4, result tuple); the result is bitwise that of
    ``scipy.optimize._dcsrch.dcstep`` (asserted on a grid by tests/test_bfgsls_cpu.py and at every call of the restatement)."""
    sgnd = np.sign(dp) * np.sign(dx)
    if fp > fx:
        case = 1
        theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt((theta / s) ** 2 - (dx / s) * (dp / s))
        if stp < stx:
            gamma *= -1
        p = (gamma - dx) + theta
        q = ((gamma - dx) + gamma) + dp
        r = p / q
        stpc = stx + r * (stp - stx)
        stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx)
        tr.cmp(abs(stpc - stx), abs(stpq - stx), "dcstep1 cubic/quadratic")
        stpf = stpc if abs(stpc - stx) <= abs(stpq - stx) else stpc + (stpq - stpc) / 2.0
        brackt = True
    elif sgnd < 0.0:
        case = 2
        theta = 3 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt((theta / s) ** 2 - (dx / s) * (dp / s))
        if stp > stx:
            gamma *= -1
        p = (gamma - dp) + theta
        q = ((gamma - dp) + gamma) + dx
        r = p / q
        stpc = stp + r * (stx - stp)
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        tr.cmp(abs(stpc - stp), abs(stpq - stp), "dcstep2 cubic/secant")
        stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
        brackt = True
    elif abs(dp) < abs(dx):
        case = 3
        theta = 3 * (fx - fp) / (stp - stx) + dx + dp
        s = max(abs(theta), abs(dx), abs(dp))
        gamma = s * np.sqrt(max(0, (theta / s) ** 2 - (dx / s) * (dp / s)))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = (gamma + (dx - dp)) + gamma
        r = p / q
        if r < 0 and gamma != 0:
            stpc = stp + r * (stx - stp)
        elif stp > stx:
            stpc = stpmax
        else:
            stpc = stpmin
        stpq = stp + (dp / (dp - dx)) * (stx - stp)
        tr.cmp(abs(stpc - stp), abs(stpq - stp), "dcstep3 cubic/secant")
        if brackt:
            stpf = stpc if abs(stpc - stp) < abs(stpq - stp) else stpq
            lim = stp + 0.66 * (sty - stp)
            tr.cmp(lim, stpf, "dcstep3 0.66 limit")
            stpf = min(lim, stpf) if stp > stx else max(lim, stpf)
        else:
            stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
            stpf = np.clip(stpf, stpmin, stpmax)
    else:
        case = 4
        if brackt:
            theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp
            s = max(abs(theta), abs(dy), abs(dp))
            gamma = s * np.sqrt((theta / s) ** 2 - (dy / s) * (dp / s))
            if stp > sty:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = ((gamma - dp) + gamma) + dy
            r = p / q
            stpf = stp + r * (sty - stp)
        elif stp > stx:
            stpf = stpmax
        else:
            stpf = stpmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    return case, (stx, fx, dx, sty, fy, dy, stpf, brackt)


class _LineSearch:
    """The scalar state machine of ase/utils/linesearch.py (MINPACK-2 dcsrch with ASE's cap on the step between two trials)."""

    def __init__(self, p, maxstep, c1, c2, stpmax, tr):
        self.p3 = p.reshape(-1, 3)
        self.maxstep, self.c1, self.c2, self.stpmax, self.tr = maxstep, c1, c2, stpmax, tr
        self.task, self.old_stp, self.no_update, self.bracket = "START", 0.0, False, False

    def determine_step(self, stp):
        dr = stp - self.old_stp
        L = float((((dr * self.p3) ** 2).sum(1) ** 0.5).max()) if len(self.p3) else 0.0
        self.tr.cmp(L, self.maxstep, "determine_step cap")
        if L >= self.maxstep:
            dr *= self.maxstep / L
            self.tr.hit("cap")
        return self.old_stp + dr

    def step(self, stp, phi, dphi):
        tr = self.tr
        if self.task == "START":
            if stp < STPMIN or stp > self.stpmax or not (dphi < 0.0):
                self.task = "ERROR"
                tr.hit("error_start")
                return stp
            tr.cmp(dphi, 0.0, "dphi < 0 at START")
            self.stage = 1
            self.finit, self.ginit, self.gtest = phi, dphi, self.c1 * dphi
            self.width = self.stpmax - STPMIN
            self.width1 = 2.0 * self.width
            self.stx = self.sty = 0.0
            self.fx = self.fy = phi
            self.gx = self.gy = dphi
            self.stmin, self.stmax = 0.0, stp + XTRAPU * stp
            self.task = "FG"
            return self.determine_step(stp)
        ftest = self.finit + stp * self.gtest
        if self.stage == 1 and phi < ftest and dphi >= 0.0:
            self.stage = 2       # (inert: ASE applies no modified-function transform)
        # the tests in dcsrch's order; a later one overrides an earlier one, CONVERGENCE last
        task = "FG"
        if self.bracket and (stp <= self.stmin or stp >= self.stmax):
            task = "WARN rounding"
        if self.bracket and self.stmax - self.stmin <= XTOL * self.stmax:
            task = "WARN xtol"
        if stp == self.stpmax and phi <= ftest and dphi <= self.gtest:
            task = "WARN stpmax"
        if stp == STPMIN and (phi > ftest or dphi >= self.gtest):
            task = "WARN stpmin"
        tr.cmp(phi, ftest, "sufficient decrease")
        tr.cmp(abs(dphi), self.c2 * (-self.ginit), "curvature")
        if phi <= ftest and abs(dphi) <= self.c2 * (-self.ginit):
            task = "CONVERGENCE"
        if task != "FG":
            self.task = task
            tr.hit("convergence" if task == "CONVERGENCE" else "warn_" + task.split()[1])
            return stp
        tr.cmp(phi, self.fx, "dcstep fp > fx")
        if not phi > self.fx and not np.sign(dphi) * np.sign(self.gx) < 0.0:
            tr.cmp(abs(dphi), abs(self.gx), "dcstep |dp| < |dx|")
        args = (self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, phi, dphi, self.bracket, self.stmin, self.stmax)
        out = dcstep(*args)              # the interpolation IS scipy's; the written-out copy only feeds the tracer
        case, mine = dcstep_traced(*args, tr)
        assert tuple(map(float, mine)) == tuple(map(float, out)), (args, mine, out)
        tr.hit(f"dcstep{case}")
        self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stpf, self.bracket = out
        stp = self.determine_step(float(stpf))
        if self.bracket:
            tr.cmp(abs(self.sty - self.stx), 0.66 * self.width1, "bisection")
            if abs(self.sty - self.stx) >= 0.66 * self.width1:
                stp = self.stx + 0.5 * (self.sty - self.stx)
                tr.hit("bisection")
            self.width1 = self.width
            self.width = abs(self.sty - self.stx)
        if self.bracket:
            self.stmin, self.stmax = min(self.stx, self.sty), max(self.stx, self.sty)
        else:
            self.stmin, self.stmax = stp + XTRAPL * (stp - self.stx), stp + XTRAPU * (stp - self.stx)
        stp = min(max(stp, STPMIN), self.stpmax)
        if self.stx == stp and stp == self.stpmax and self.stmin > self.stpmax:
            self.no_update = True
            tr.hit("no_update")
        if ((self.bracket and stp < self.stmin) or stp >= self.stmax) or (self.bracket and self.stmax - self.stmin < XTOL * self.stmax):
            stp = self.stx
            tr.hit("fallback_stx")
        self.task = "FG"
        return stp


def bfgs_linesearch(force_fn, pos, fixed=None, max_steps=20, fmax=0.01, max_eval=None, alpha=10.0, maxstep=0.2, c1=0.23, c2=0.46,
                    stpmax=50.0, trace=None, record_interval=0):
    """Returns (positions [N, 3], energy at those positions, n_steps, n_eval, stop_reason, records)
    with records = [(step, positions, energy, forces)] of the step-opens with step % record_interval == 0 (empty when 0)."""
    tr = trace if trace is not None else _NoTrace()
    pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
    nat = len(pos)
    held = np.zeros(nat, bool)
    if fixed is not None and len(fixed):
        held[np.asarray(fixed, dtype=np.int64)] = True
    if max_eval is None:
        max_eval = 20 * max_steps + 20
    neval = 0

    def evaluate(x, kind):
        nonlocal neval
        E, F = force_fn(x.reshape(-1, 3))
        F = np.array(F, dtype=np.float64).reshape(-1, 3)
        F[held] = 0.0
        neval += 1
        if tr.trials is not None:
            tr.trials.append((kind, x.reshape(-1, 3).copy()))
        return float(E), F.reshape(-1)

    def done(x, reason):
        tr.hit(f"stop{reason}")
        x = x.reshape(-1, 3).copy()
        return x, float(force_fn(x)[0]), steps, neval, reason, records   # (the closing evaluation: not one of the optimizer's)

    r = pos.reshape(-1).copy()
    H = None
    hist = []
    steps, records = 0, []
    r0 = g0 = p = None
    alpha_k, no_update, gp0, ginit0 = None, False, 0.0, 0.0
    E, F = evaluate(r, "open")
    while True:
        # ---- a step opens at r with (E, F) ----
        if not (np.isfinite(E) and np.isfinite(F).all()):
            return done(r, 5)
        e, g = E / alpha, -F / alpha
        if tr.energies is not None:
            tr.energies.append(E)
        if record_interval and steps % record_interval == 0:
            records.append((steps, r.reshape(-1, 3).copy(), E, F.reshape(-1, 3).copy()))
        fm2 = float((F.reshape(-1, 3) ** 2).sum(1).max()) if nat else 0.0
        tr.cmp(fm2, fmax * fmax, "convergence")
        if fm2 < fmax * fmax:
            return done(r, 1)
        if steps >= max_steps:
            return done(r, 2)
        if H is None:
            H = np.eye(3 * nat)
        else:
            dr, dg = r - r0, g - g0
            tr.cmp(abs(gp0), abs(ginit0), "update condition")
            if alpha_k > 0 and abs(gp0) - abs(ginit0) < 0 and not no_update:
                d = float(np.dot(dg, dr))
                with np.errstate(divide="ignore"):
                    rho = np.float64(1.0) / np.float64(d)
                if d == 0.0 or np.isinf(rho):
                    rho = 1000.0
                    tr.hit("rho_fallback")
                rho = float(rho)
                I = np.eye(3 * nat)
                A1 = I - np.outer(dr, dg) * rho
                A2 = I - np.outer(dg, dr) * rho
                H = A1 @ H @ A2 + rho * np.outer(dr, dr)
                hist.append((dr.copy(), dg.copy(), rho))
            else:
                tr.hit("skip_update")
        p = -(H @ g)
        if trace is not None:
            pl = -two_loop(g, hist)
            err = float(np.abs(pl - p).max() / max(np.abs(p).max(), 1e-300))
            tr.two_loop_err = max(tr.two_loop_err, err)
        psize, pfloor = float(np.sqrt((p ** 2).sum())), float(np.sqrt(nat * 1e-10))
        tr.cmp(psize, pfloor, "p floor")
        if psize <= pfloor:
            p = p * (pfloor / psize)
            tr.hit("p_floor")
        ls = _LineSearch(p, maxstep, c1, c2, stpmax, tr)
        stp, phi, dphi = 1.0, e, float(np.dot(g, p))
        phi0, dphi0 = phi, dphi
        r0, g0 = r, g
        while True:
            stp = ls.step(stp, phi, dphi)
            if ls.task != "FG":
                break
            if neval >= max_eval:       # the budget is spent: the best point of the interrupted search
                x = r + ls.stx * p
                return done(x, 4)
            E, F = evaluate(r + stp * p, "trial")
            if not (np.isfinite(E) and np.isfinite(F).all()):
                return done(r, 5)
            phi, dphi = E / alpha, float(np.dot(-F / alpha, p))
            ls.old_stp = stp
            if ls.no_update:
                break
        if ls.task.startswith("ERROR") or ls.task.startswith("WARN"):
            return done(r, 3)
        alpha_k, no_update, gp0, ginit0 = stp, ls.no_update, dphi, dphi0
        if tr.steps is not None:
            tr.steps.append(dict(stp=stp, phi0=phi0, dphi0=dphi0, phi=phi, dphi=dphi, no_update=ls.no_update))
        r = r + stp * p
        steps += 1
