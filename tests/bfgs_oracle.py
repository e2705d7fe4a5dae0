"""numpy restatement of ASE's BFGS (ase/optimize/bfgs.py, the optimizer of the reference's SrTiO3 configuration:
scripts/configs/sample_config_painn.json:26, dispatched at mcmc/dynamics.py:119-141) for tests: the checker of the
device relaxation.  TEST INFRASTRUCTURE.

Parity status: PINNED.  Driven by the CPU oracle (fp32 mode, like nff) it reproduces the (energy, fmax) traces stored in
the reference's notebooks (tests/test_SrTiO3_terms.ipynb:201-227: 6 + 3 + 14 points; tutorials/SrTiO3_001.ipynb:241-245:
5 points), committed as tests/golden/bfgs_traces.json -- see tests/test_bfgs.py for the tolerances.

ASE's algorithm, restated: H0 = alpha * I (alpha = 70 eV/A^2), maxstep = 0.2 A.  Every step: BFGS update of H from
(dr, df) of the previous step (skipped when max|dr| < 1e-7), eigen-decomposition H = V diag(w) V^T, step
dr = V (V^T f / |w|), rescaled so that the longest atomic displacement is at most maxstep.  Convergence: max_i |F_i| < fmax,
tested before every step; at most `max_steps` steps.  FixAtoms zeroes the forces of the held atoms and keeps their
positions; H stays block diagonal, so restricting it to the free atoms is exact.

Four optional arguments serve tests/relax_cases.py (without them nothing changes).  ``f32`` rounds the forces to float32 before use,
as the device's optimizer state does for the fp64 potentials (csrc/relax.hip::k_narrow_forces).  ``record`` is a list that receives
one dict per iteration (positions before the step, the branches taken, the margins of every decision).  ``mmax`` is the one thing
the device does that ASE does not: its factored Hessian holds at most mmax basis vectors and an update is skipped when fewer than
two are free (``m + 2 > mmax``).  The matrix here stays dense; m, the dimension of the span of all update vectors (df_i, H_i dr_i) so
far, is counted by projecting every new vector on an orthonormal basis of the earlier ones (``RANK_TOL``; the residuals are recorded
so that a test can assert that the count is never a close call).  ``mutate = (iteration, which)`` takes the OTHER branch of one
decision at one iteration (``MUTATIONS``), to show that a trajectory comparison would notice."""

import numpy as np

BRANCHES = ("first", "update", "skipped_update", "full_basis", "neg_eig", "dropped_column", "scaled", "unscaled")
# the decision whose flip leaves a branch (dropped_column has none: in the dense matrix a dependent vector adds nothing either way)
MUTATIONS = {"update": "skip", "skipped_update": "skip", "full_basis": "full", "neg_eig": "fabs", "scaled": "scale", "unscaled": "scale"}
# A new update vector whose residual against the span of the earlier ones is below RANK_TOL of its norm adds no dimension.  From the
# second update on H dr lies in that span in exact arithmetic (dr = |H|^-1 f up to a factor, and the span holds every earlier force);
# what is left of it is the rounding of r = r0 + step, at most alpha x half an ulp of a coordinate: ~1e-13 of |H dr| while the steps
# are long and up to ~1e-10 once a run has contracted to steps of 1e-4 A (``dg_noise_ratio`` of a record is the residual over that
# bound).  New directions measure 1e-5 and more.  So residuals are expected below RANK_LO or above RANK_HI, never between.
RANK_TOL, RANK_LO, RANK_HI = 1e-8, 1e-9, 1e-6


def device_mmax(max_steps):
    """Basis capacity of the device's factored Hessian: 2 max_steps + 2, lowered in steps of 2 until the eigen-decomposition's
    workspace (2 mmax (mmax | 1) + 5 mmax + 8 doubles) fits into 160 KiB - 4 KiB of LDS (csrc/relax.hip::BfgsWork::init)."""
    mmax = 2 * max_steps + 2
    while 8 * (2 * mmax * (mmax | 1) + 5 * mmax + 8) > 160 * 1024 - 4096:
        mmax -= 2
    return mmax


class _Span:
    """Orthonormal basis of the update vectors seen so far."""

    def __init__(self, n):
        self.Q = np.zeros((0, n))

    def add(self, v):
        """Relative residual of v against the span; extends the basis if it is above RANK_TOL."""
        n0 = np.linalg.norm(v)
        w = v.copy()
        for _ in range(2):
            w = w - self.Q.T @ (self.Q @ w)
        res = float(np.linalg.norm(w) / n0) if n0 > 0 else 0.0
        if res > RANK_TOL:
            self.Q = np.vstack([self.Q, w / np.linalg.norm(w)])
        return res

    @property
    def m(self):
        return len(self.Q)


def bfgs_relax(force_fn, pos, fixed=None, max_steps=20, fmax=0.01, alpha=70.0, maxstep=0.2, f32=False, record=None, mmax=None,
               mutate=None):
    """force_fn(pos) -> (energy, forces[N,3]).  Returns (pos, trace [(energy, fmax)], n_steps, converged)."""
    pos = np.array(pos, dtype=np.float64)
    n = len(pos)
    free = np.ones(n, bool)
    if fixed is not None and len(fixed):
        free[np.asarray(fixed, dtype=np.int64)] = False
    idx = np.where(free)[0]
    H = None
    r0 = f0 = None
    span = _Span(3 * len(idx)) if (mmax is not None or record is not None) else None
    trace = []
    steps, converged = 0, False
    for it in range(max_steps + 1):
        e, f = force_fn(pos)
        f = np.asarray(f, dtype=np.float64)
        if f32:
            f = f.astype(np.float32).astype(np.float64)
        f = f[idx]
        fm = float(np.sqrt((f ** 2).sum(axis=1).max())) if len(idx) else 0.0
        trace.append((float(e), fm))
        rec = None
        if record is not None:
            rec = dict(it=it, pos=pos.copy(), energy=float(e), fm=fm, branches=set(), m=span.m)
            record.append(rec)
        if fm < fmax:
            converged = True
            break
        if it == max_steps:
            break
        flip = mutate[1] if mutate is not None and mutate[0] == it else None
        r = pos[idx].reshape(-1)
        fv = f.reshape(-1)
        if H is None:
            H = np.eye(3 * len(idx)) * alpha
            if rec is not None:
                rec["branches"].add("first")
        else:
            dr = r - r0
            mx = np.abs(dr).max()
            full = mmax is not None and span.m + 2 > mmax
            if rec is not None:
                rec["max_dr"] = float(mx)
            if (mx >= 1e-7) == (flip == "skip"):
                if rec is not None:
                    rec["branches"].add("skipped_update")
            elif full != (flip == "full"):
                if rec is not None:
                    rec["branches"].add("full_basis")
            else:
                df = fv - f0
                a = np.dot(dr, df)
                dg = np.dot(H, dr)
                b = np.dot(dr, dg)
                H = H - np.outer(df, df) / a - np.outer(dg, dg) / b
                if span is not None:
                    m0 = span.m
                    res = (span.add(df), span.add(dg))
                    if rec is not None:
                        scale = np.linalg.norm(dr) * np.linalg.norm(df)
                        rec.update(a_rel=float(a / scale), b_rel=float(b / scale), residuals=res, m=span.m)
                        # the residual of H dr over what the rounding of r = r0 + step can put there at most: alpha x half an ulp
                        rec["dg_noise_ratio"] = float(res[1] * np.linalg.norm(dg) / (alpha * 2.0 ** -53 * np.linalg.norm(r)))
                        rec["branches"].add("update")
                        if span.m - m0 < 2:
                            rec["branches"].add("dropped_column")
        omega, V = np.linalg.eigh(H)
        if rec is not None:
            rec["omega_min"] = float(omega.min())
            if omega.min() < 0.0:
                rec["branches"].add("neg_eig")
        step = np.dot(V, np.dot(fv, V) / (omega if flip == "fabs" else np.fabs(omega))).reshape(-1, 3)
        longest = np.sqrt((step ** 2).sum(axis=1)).max()
        if rec is not None:
            rec["longest_rel"] = float(longest / maxstep)
            rec["branches"].add("scaled" if longest >= maxstep else "unscaled")
        if (longest >= maxstep) != (flip == "scale"):
            step *= maxstep / longest
        r0, f0 = r.copy(), fv.copy()
        pos[idx] += step
        steps += 1
    return pos, trace, steps, converged
