// bfgsls_dev.h — device side of the lock-step BFGSLineSearch optimizer (relax_bfgsls.hip): the scalar line search (MINPACK-2
// dcsrch / dcstep with ASE's step cap), the per-chain state machine and its workspace.
//
// PROVENANCE.  Restated from ASE's ase/optimize/bfgslinesearch.py and ase/utils/linesearch.py AS REMEMBERED: ASE cannot be installed
// next to this project, so the restatement is NOT pinned by an executed ASE.  The contract is the numpy restatement
// tests/bfgsls_oracle.py (dense H, as ASE holds it); its interpolation routine is scipy.optimize._dcsrch.dcstep, an independent
// statement of MINPACK-2 dcstep, and bls_dcstep below follows that routine line by line.
//
// One evaluation of the batch per launch; every chain consumes it according to its own phase:
//   BLS_OPEN   E, F at the point r a step opens at: convergence / step budget, the H update from the step just accepted, p = -H g by
//              the two-loop recursion over the stored (dr, dg, rho) triples (H itself is never stored: with H0 = I the product form
//              H <- (I - rho dr dg^T) H (I - rho dg dr^T) + rho dr dr^T holds for any rho, the 1000 fallback included), a fresh line
//              search, the move to its first trial r + stp p;
//   BLS_TRIAL  E, F at r + stp p: the line search takes (phi, dphi) and either asks for another trial, fails (positions back to r), or
//              accepts -- and the SAME evaluation then opens the next step (ASE gets that from its calculator cache).
// ASE applies no modified-function transform in stage 1; `stage` is tracked and inert.
#ifndef VSSR_BFGSLS_DEV_H
#define VSSR_BFGSLS_DEV_H
#include "cg_dev.h"

namespace vssr {

enum { BLS_OPEN = 0, BLS_TRIAL = 1 };
enum { BLS_FG = 0, BLS_CONVERGENCE = 1, BLS_WARN = 2, BLS_ERROR = 3 };
// stop reasons: 1 converged (max |F_i| < fmax), 2 max_steps, 3 line search failed (ASE raises "LineSearch failed!"), 4 max_eval,
// 5 non-finite energy or force
struct BlsParams {
    int max_steps, max_eval;
    double fmax, alpha, maxstep, c1, c2, stpmax, stpmin, xtol, xtrapl, xtrapu;
};
struct BlsState {   // per chain; every thread of the workgroup advances its own copy, thread 0 stores it
    int phase, steps, neval, reason, nhist, bracket, no_update, stage;
    double alpha_k, gp0;   // the accepted step length, g.p0 of the evaluation that accepted it
    double stp, old_stp, pmax, finit, ginit, gtest, width, width1, stx, fx, gx, sty, fy, gy, stmin, stmax;
};

// MINPACK-2 dcstep (scipy.optimize._dcsrch.dcstep, same operation order)
__device__ inline double bls_dcstep(double &stx, double &fx, double &dx, double &sty, double &fy, double &dy, double stp, double fp, double dp,
                                    int &brackt, double stpmin, double stpmax) {
    auto sign = [](double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); };
    const double sgnd = sign(dp) * sign(dx);
    double stpf;
    if (fp > fx) {   // 1: a higher function value, the minimum is bracketed
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = fmax(fmax(fabs(theta), fabs(dx)), fabs(dp));
        double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
        if (stp < stx) gamma = -gamma;
        const double p = (gamma - dx) + theta, q = ((gamma - dx) + gamma) + dp, r = p / q;
        const double stpc = stx + r * (stp - stx);
        const double stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
        stpf = fabs(stpc - stx) <= fabs(stpq - stx) ? stpc : stpc + (stpq - stpc) / 2.0;
        brackt = 1;
    } else if (sgnd < 0.0) {   // 2: lower value, derivatives of opposite sign, the minimum is bracketed
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = fmax(fmax(fabs(theta), fabs(dx)), fabs(dp));
        double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
        if (stp > stx) gamma = -gamma;
        const double p = (gamma - dp) + theta, q = ((gamma - dp) + gamma) + dx, r = p / q;
        const double stpc = stp + r * (stx - stp);
        const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
        stpf = fabs(stpc - stp) > fabs(stpq - stp) ? stpc : stpq;
        brackt = 1;
    } else if (fabs(dp) < fabs(dx)) {   // 3: lower value, same sign, the derivative shrinks
        const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
        const double s = fmax(fmax(fabs(theta), fabs(dx)), fabs(dp));
        double gamma = s * sqrt(fmax(0.0, (theta / s) * (theta / s) - (dx / s) * (dp / s)));
        if (stp > stx) gamma = -gamma;
        const double p = (gamma - dp) + theta, q = (gamma + (dx - dp)) + gamma, r = p / q;
        double stpc;
        if (r < 0.0 && gamma != 0.0) stpc = stp + r * (stx - stp);
        else stpc = stp > stx ? stpmax : stpmin;
        const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
        if (brackt) {
            stpf = fabs(stpc - stp) < fabs(stpq - stp) ? stpc : stpq;
            stpf = stp > stx ? fmin(stp + 0.66 * (sty - stp), stpf) : fmax(stp + 0.66 * (sty - stp), stpf);
        } else {
            stpf = fabs(stpc - stp) > fabs(stpq - stp) ? stpc : stpq;
            stpf = fmin(fmax(stpf, stpmin), stpmax);
        }
    } else {   // 4: lower value, same sign, the derivative does not shrink
        if (brackt) {
            const double theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp;
            const double s = fmax(fmax(fabs(theta), fabs(dy)), fabs(dp));
            double gamma = s * sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s));
            if (stp > sty) gamma = -gamma;
            const double p = (gamma - dp) + theta, q = ((gamma - dp) + gamma) + dy, r = p / q;
            stpf = stp + r * (sty - stp);
        } else
            stpf = stp > stx ? stpmax : stpmin;
    }
    if (fp > fx) { sty = stp; fy = fp; dy = dp; }
    else {
        if (sgnd < 0.0) { sty = stx; fy = fx; dy = dx; }
        stx = stp; fx = fp; dx = dp;
    }
    return stpf;
}

// ASE's cap: no trial moves an atom more than maxstep beyond the previous trial.  S.pmax = max_i |p_i| of the search direction.
__device__ inline double bls_determine_step(const BlsState &S, const BlsParams &P, double stp) {
    double dr = stp - S.old_stp;
    const double L = fabs(dr) * S.pmax;
    if (L >= P.maxstep) dr *= P.maxstep / L;
    return S.old_stp + dr;
}

// task START of a fresh line search (stp = 1 on entry)
__device__ inline int bls_ls_start(BlsState &S, const BlsParams &P, double phi, double dphi, double &stp) {
    if (stp < P.stpmin || stp > P.stpmax || !(dphi < 0.0)) return BLS_ERROR;
    S.stage = 1; S.bracket = 0;
    S.finit = phi; S.ginit = dphi; S.gtest = P.c1 * dphi;
    S.width = P.stpmax - P.stpmin; S.width1 = 2.0 * S.width;
    S.stx = S.sty = 0.0; S.fx = S.fy = phi; S.gx = S.gy = dphi;
    S.stmin = 0.0; S.stmax = stp + P.xtrapu * stp;
    stp = bls_determine_step(S, P, stp);
    return BLS_FG;
}

// (phi, dphi) of the trial at stp: the tests of dcsrch in their order (a later one overrides an earlier one, CONVERGENCE last), then the
// next trial
__device__ inline int bls_ls_next(BlsState &S, const BlsParams &P, double phi, double dphi, double &stp) {
    const double ftest = S.finit + stp * S.gtest;
    if (S.stage == 1 && phi < ftest && dphi >= 0.0) S.stage = 2;
    int task = BLS_FG;
    if (S.bracket && (stp <= S.stmin || stp >= S.stmax)) task = BLS_WARN;
    if (S.bracket && S.stmax - S.stmin <= P.xtol * S.stmax) task = BLS_WARN;
    if (stp == P.stpmax && phi <= ftest && dphi <= S.gtest) task = BLS_WARN;
    if (stp == P.stpmin && (phi > ftest || dphi >= S.gtest)) task = BLS_WARN;
    if (phi <= ftest && fabs(dphi) <= P.c2 * (-S.ginit)) task = BLS_CONVERGENCE;
    if (task != BLS_FG) return task;
    const double stpf = bls_dcstep(S.stx, S.fx, S.gx, S.sty, S.fy, S.gy, stp, phi, dphi, S.bracket, S.stmin, S.stmax);
    stp = bls_determine_step(S, P, stpf);
    if (S.bracket) {
        if (fabs(S.sty - S.stx) >= 0.66 * S.width1) stp = S.stx + 0.5 * (S.sty - S.stx);
        S.width1 = S.width;
        S.width = fabs(S.sty - S.stx);
    }
    if (S.bracket) { S.stmin = fmin(S.stx, S.sty); S.stmax = fmax(S.stx, S.sty); }
    else { S.stmin = stp + P.xtrapl * (stp - S.stx); S.stmax = stp + P.xtrapu * (stp - S.stx); }
    stp = fmin(fmax(stp, P.stpmin), P.stpmax);
    if (S.stx == stp && stp == P.stpmax && S.stmin > P.stpmax) S.no_update = 1;
    if (((S.bracket && stp < S.stmin) || stp >= S.stmax) || (S.bracket && S.stmax - S.stmin < P.xtol * S.stmax)) stp = S.stx;
    return BLS_FG;
}

// Device pointers of a relaxation (BlsWork, relax_bfgsls.hip).  Vectors run over all 3 N_b coordinates of a chain, entries of held atoms
// zero.  History: `cap` triples per chain, rows of chain b at hs / hy + 3 a0 cap (row length 3 N_b), scalars at rho / la + b cap.
struct BlsView {
    BlsState *st;
    double *r0, *g0, *p;   // [3 N]: the point the step opened at, its gradient, the search direction
    double *hs, *hy;       // dr / dg rows
    double *rho, *la;      // [B][cap]: stored rho, first-loop coefficients of the current product
    int cap;
    // trajectory observer (null ring_pos: off): records of the evaluations that OPEN a step
    int interval, nrec, B, N;
    double *ring_pos;
    float *ring_f;
    double *ring_e;
    int *ring_n;
};

// One launch of chain b's state machine on the evaluation just made; every thread of the 256-thread workgroup calls it.  FT: double
// (d_pot_f) or float (PaiNN's d_forces, widened).  Every vector loop is strided by ATOM with the same stride, so a thread only ever reads
// elements it wrote itself; the scalars all threads branch on come from the loaded state and from block reductions, which hand every
// thread the same bits: no wave can part from its workgroup in front of a barrier.
template <class FT>
__device__ __forceinline__ void bls_step_chain(int b, double *red, const int *__restrict__ cfg_start, const double *__restrict__ energy,
                                               const FT *__restrict__ forces, const uint8_t *__restrict__ fixed, const BlsParams P,
                                               double *__restrict__ pos, const BlsView V, unsigned char *__restrict__ active,
                                               int *__restrict__ running) {
    const int tid = threadIdx.x, nt = blockDim.x;
    BlsState S = V.st[b];
    __syncthreads();   // every wave holds the state before thread 0 can store the advanced one (cg_dev.h)
    if (S.reason) return;
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0, n = 3 * nat;
    double *x = pos + 3 * (size_t)a0, *r0 = V.r0 + 3 * (size_t)a0, *g0 = V.g0 + 3 * (size_t)a0, *p = V.p + 3 * (size_t)a0;
    double *hs = V.hs + 3 * (size_t)a0 * V.cap, *hy = V.hy + 3 * (size_t)a0 * V.cap, *rho = V.rho + (size_t)b * V.cap, *la = V.la + (size_t)b * V.cap;
    const FT *fg = forces + 3 * (size_t)a0;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;
    auto F = [&](int i, int c) -> double { return (fx && fx[i]) ? 0.0 : (double)fg[3 * i + c]; };
    auto G = [&](int i, int c) -> double { return -F(i, c) / P.alpha; };
    auto stop = [&](int reason) {
        if (tid == 0) { S.reason = reason; V.st[b] = S; active[b] = 0; }
    };
    auto keep_going = [&]() {
        if (tid == 0) { V.st[b] = S; *running = 1; }   // (a flag, not a count: every running chain stores the same word)
    };
    auto move_to = [&](double stp) {
        for (int i = tid; i < nat; i += nt)
            for (int c = 0; c < 3; ++c) x[3 * i + c] = r0[3 * i + c] + stp * p[3 * i + c];
    };

    // ---- what this evaluation is worth: finite?  max |F_i|^2, and F.p of a trial ----
    const double E = energy[b];
    double bad = isfinite(E) ? 0.0 : 1.0, fm2 = 0.0, gp = 0.0;
    for (int i = tid; i < nat; i += nt) {
        const double f0 = F(i, 0), f1 = F(i, 1), f2 = F(i, 2);
        if (!(isfinite(f0) && isfinite(f1) && isfinite(f2))) bad = 1.0;
        fm2 = fmax(fm2, f0 * f0 + f1 * f1 + f2 * f2);
        if (S.phase == BLS_TRIAL) gp += G(i, 0) * p[3 * i] + G(i, 1) * p[3 * i + 1] + G(i, 2) * p[3 * i + 2];
    }
    bad = block_max(bad, red);
    S.neval += 1;
    if (bad != 0.0) {   // nothing sane to follow: back to the point the step opened at (an opening evaluation is there already)
        if (S.phase == BLS_TRIAL) move_to(0.0);
        stop(5);
        return;
    }
    fm2 = block_max(fm2, red);

    if (S.phase == BLS_TRIAL) {
        const double phi = E / P.alpha, dphi = block_sum(gp, red);
        S.old_stp = S.stp;
        bool accept = S.no_update != 0;
        if (!accept) {
            double stp = S.stp;
            const int task = bls_ls_next(S, P, phi, dphi, stp);
            if (task == BLS_WARN) { move_to(0.0); stop(3); return; }
            if (task == BLS_CONVERGENCE) accept = true;
            else {
                if (S.neval >= P.max_eval) { move_to(S.stx); stop(4); return; }   // the best point of the interrupted search
                S.stp = stp;
                move_to(stp);
                keep_going();
                return;
            }
        }
        // accepted: x = r + stp p stands; this evaluation opens the next step
        S.alpha_k = S.stp; S.gp0 = dphi;
        S.steps += 1;
        S.phase = BLS_OPEN;
    }

    // ---- a step opens at x ----
    if (V.ring_pos && S.steps % V.interval == 0 && S.steps / V.interval < V.nrec) {   // the observer: before anything moves
        const int r = S.steps / V.interval;
        for (int i = tid; i < nat; i += nt)
            for (int c = 0; c < 3; ++c) {
                V.ring_pos[(size_t)r * 3 * V.N + 3 * (size_t)(a0 + i) + c] = x[3 * i + c];
                V.ring_f[(size_t)r * 3 * V.N + 3 * (size_t)(a0 + i) + c] = (float)F(i, c);
            }
        if (tid == 0) {
            V.ring_e[(size_t)r * V.B + b] = E;
            if (V.ring_n[b] < r + 1) V.ring_n[b] = r + 1;
        }
    }
    if (!(fm2 >= P.fmax * P.fmax)) { stop(1); return; }
    if (S.steps >= P.max_steps) { stop(2); return; }
    if (S.steps > 0 && S.alpha_k > 0.0 && fabs(S.gp0) - fabs(S.ginit) < 0.0 && !S.no_update && S.nhist < V.cap) {
        double *sj = hs + (size_t)S.nhist * n, *yj = hy + (size_t)S.nhist * n;
        double d = 0.0;
        for (int i = tid; i < nat; i += nt)
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * i + c;
                const double dr = x[k] - r0[k], dg = G(i, c) - g0[k];
                sj[k] = dr; yj[k] = dg;
                d += dg * dr;
            }
        d = block_sum(d, red);
        double rk = 1.0 / d;
        if (d == 0.0 || isinf(rk)) rk = 1000.0;
        if (tid == 0) rho[S.nhist] = rk;
        S.nhist += 1;
    }
    __syncthreads();   // rho of the new triple
    // p = -H g, two-loop recursion with the stored rho (q lives in p)
    for (int i = tid; i < nat; i += nt)
        for (int c = 0; c < 3; ++c) p[3 * i + c] = G(i, c);
    for (int j = S.nhist - 1; j >= 0; --j) {
        const double *sj = hs + (size_t)j * n, *yj = hy + (size_t)j * n;
        double d = 0.0;
        for (int i = tid; i < nat; i += nt)
            for (int c = 0; c < 3; ++c) d += sj[3 * i + c] * p[3 * i + c];
        const double a = rho[j] * block_sum(d, red);
        if (tid == 0) la[j] = a;
        for (int i = tid; i < nat; i += nt)
            for (int c = 0; c < 3; ++c) p[3 * i + c] -= a * yj[3 * i + c];
    }
    __syncthreads();   // la
    for (int j = 0; j < S.nhist; ++j) {
        const double *sj = hs + (size_t)j * n, *yj = hy + (size_t)j * n;
        double d = 0.0;
        for (int i = tid; i < nat; i += nt)
            for (int c = 0; c < 3; ++c) d += yj[3 * i + c] * p[3 * i + c];
        const double bt = rho[j] * block_sum(d, red);
        const double a = la[j];
        for (int i = tid; i < nat; i += nt)
            for (int c = 0; c < 3; ++c) p[3 * i + c] += sj[3 * i + c] * (a - bt);
    }
    double pp = 0.0;
    for (int i = tid; i < nat; i += nt)
        for (int c = 0; c < 3; ++c) { const double v = -p[3 * i + c]; p[3 * i + c] = v; pp += v * v; }
    const double psize = sqrt(block_sum(pp, red)), pfloor = sqrt(nat * 1e-10);
    const double pscale = psize <= pfloor ? pfloor / psize : 1.0;
    double pm2 = 0.0, gp1 = 0.0;
    for (int i = tid; i < nat; i += nt) {
        double s2 = 0.0;
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * i + c;
            const double v = psize <= pfloor ? p[k] * pscale : p[k], g = G(i, c);
            p[k] = v;
            s2 += v * v;
            gp1 += g * v;
            r0[k] = x[k];
            g0[k] = g;
        }
        pm2 = fmax(pm2, s2);
    }
    S.pmax = sqrt(block_max(pm2, red));
    const double phi = E / P.alpha, dphi = block_sum(gp1, red);
    // fresh line search
    S.old_stp = 0.0; S.no_update = 0; S.bracket = 0;
    double stp = 1.0;
    if (bls_ls_start(S, P, phi, dphi, stp) == BLS_ERROR) { stop(3); return; }
    if (S.neval >= P.max_eval) { stop(4); return; }   // (stx = 0: the point the step opened at)
    S.stp = stp;
    S.phase = BLS_TRIAL;
    move_to(stp);
    keep_going();
}

}  // namespace vssr
#endif
