// relax.hip — lock-step relaxation of all resident chains on the device: FIRE and BFGS.
//
// Counterpart of optimize_slab (reference mcmc/dynamics.py:83-170):
//   dyn = Optimizer(slab); dyn.run(steps=relax_steps, fmax=0.01)
// with Optimizer = ase.optimize.BFGS for the reference's SrTiO3 configuration (scripts/configs/sample_config_painn.json:26,
// dispatch mcmc/dynamics.py:119-127) and ase.optimize.FIRE as the default.  FixAtoms (reference mcmc/system.py:288-294)
// enters as a per-atom mask that zeroes the force.  The reference drives one structure from Python; here every chain
// carries its own optimizer state on the device and all chains step together: one energy+force evaluation of the batch
// per iteration, positions and forces never leave HBM.  A chain whose max |F_i| drops below fmax freezes (ASE's
// convergence test, evaluated before each step) and is marked inactive: the evaluation kernels skip inactive chains, so an
// iteration costs what its unconverged chains cost.
//
// FIRE (ase/optimize/fire.py; defaults dt=0.1, maxstep=0.2, dtmax=1.0, Nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)
// is restated per chain with (velocity, dt, a, Nsteps) state.
//
// BFGS (ase/optimize/bfgs.py; alpha = 70, maxstep = 0.2): H0 = alpha I; per step the rank-2 update
//   H <- H - df df^T / (dr.df) - (H dr)(H dr)^T / (dr.H dr)        (skipped when max|dr| < 1e-7)
// and the step dr = V |W|^-1 V^T f from the eigen-decomposition H = V W V^T, rescaled so that the longest atomic
// displacement is at most maxstep.  ASE holds the dense 3N x 3N matrix; here the SAME matrix is held in factored form.
// After k updates H = alpha I + Q B Q^T exactly, where the m <= 2k orthonormal columns of Q span the update vectors
// (df_i, H_i dr_i) and B is m x m: H dr costs O(N m), the eigen-decomposition is that of the m x m matrix alpha I + B
// (every direction outside span(Q) keeps the eigenvalue alpha), and
//   |H|^-1 f = (f - Q Q^T f) / alpha + Q Y |L|^-1 Y^T Q^T f ,   alpha I + B = Y L Y^T.
// No 3N x 3N storage and no large eigensolve for any number of free atoms; the m x m problem (m <= 2 relax_steps) is
// solved by cyclic Jacobi rotations in LDS, fp64.  Pinned against the reference's stored BFGS traces through
// tests/bfgs_oracle.py (dense restatement of ASE's algorithm) -- tests/test_bfgs.py.
//
// Both run in one driver frame, relax_lockstep<FireWork | BfgsWork>; its prologue and regrow also serve the frame of the other
// lock-step drivers (lockstep.h).
#include <algorithm>
#include "cg_dev.h"
#include "fire_dev.h"

namespace vssr {

// chain b has converged: freeze it and take it out of the evaluation
__device__ inline void mark_converged(int b, int *converged, unsigned char *active) {
    *converged = 1;
    active[b] = 0;
}

// ---- FIRE ---------------------------------------------------------------------------------------------------------------
struct FireState {   // per chain
    double dt, a;
    int nsteps_pos;  // steps since the last power <= 0 (ASE's Nsteps)
    int has_v;       // 0 until the first step (ASE: self.v is None)
    int steps;       // optimizer steps taken
    int converged;
};

__global__ void k_fire_init(int B, double dt0, double astart, FireState *__restrict__ st, unsigned char *__restrict__ active) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    st[b].dt = dt0; st[b].a = astart; st[b].nsteps_pos = 0; st[b].has_v = 0; st[b].steps = 0; st[b].converged = 0;
    active[b] = 1;
}

// One workgroup per chain: convergence test on the forces of the CURRENT positions, then one FIRE step.  Nothing moves
// when the neighbor capacity overflowed in the evaluation that produced `forces` (counters[2]): the host regrows the
// buffers, repeats the evaluation and launches this kernel again.
__global__ void __launch_bounds__(256)
k_fire_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const float *__restrict__ forces,
            const uint8_t *__restrict__ fixed, double fmax_tol, double maxstep, double dtmax, double finc, double fdec,
            double astart, double fa, int nmin, int max_steps, double *__restrict__ pos, double *__restrict__ vel,
            FireState *__restrict__ st, unsigned char *__restrict__ active, int *__restrict__ n_active) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (counters[2]) return;
    const int a0 = cfg_start[b], a1 = cfg_start[b + 1];
    FireState S = st[b];
    if (S.converged) return;
    // max_i |F_i| over unconstrained atoms
    double fm2 = 0.0;
    for (int i = a0 + tid; i < a1; i += blockDim.x) {
        if (fixed && fixed[i]) continue;
        double fx = forces[3 * i], fy = forces[3 * i + 1], fz = forces[3 * i + 2];
        fm2 = fmax(fm2, fx * fx + fy * fy + fz * fz);
    }
    fm2 = block_max(fm2, red);
    if (!(fm2 >= fmax_tol * fmax_tol)) {   // converged (a NaN force also stops the chain: nothing sane to follow)
        if (tid == 0) mark_converged(b, &st[b].converged, active);
        return;
    }
    if (S.steps >= max_steps) return;   // (iterations repeated after a capacity regrow never exceed relax_steps)
    double vf = 0.0, ff = 0.0, vv = 0.0;
    for (int i = a0 + tid; i < a1; i += blockDim.x) {
        const bool fx_ = fixed && fixed[i];
        for (int x = 0; x < 3; ++x) {
            double f = fx_ ? 0.0 : (double)forces[3 * i + x], v = S.has_v ? vel[3 * i + x] : 0.0;
            vf += f * v; ff += f * f; vv += v * v;
        }
    }
    vf = block_sum(vf, red);
    ff = block_sum(ff, red);
    vv = block_sum(vv, red);
    const FireKnobs K{dtmax, finc, fdec, astart, fa, maxstep, nmin};
    const FireMix M = fire_update(S, K, vf, ff, vv);
    // v <- mix(v, f) + dt f ; dr = dt v
    double dr2 = 0.0;
    for (int i = a0 + tid; i < a1; i += blockDim.x) {
        const bool fx_ = fixed && fixed[i];
        for (int x = 0; x < 3; ++x) {
            double f = fx_ ? 0.0 : (double)forces[3 * i + x];
            double v = M.mix ? vel[3 * i + x] : 0.0;
            if (M.mix) v = (1.0 - M.mix_a) * v + M.mix_s * f;
            v += S.dt * f;
            vel[3 * i + x] = v;
            dr2 += (S.dt * v) * (S.dt * v);
        }
    }
    dr2 = block_sum(dr2, red);
    const double normdr = sqrt(dr2);
    const double scale = normdr > maxstep ? maxstep / normdr : 1.0;
    for (int i = a0 + tid; i < a1; i += blockDim.x)
        for (int x = 0; x < 3; ++x) pos[3 * i + x] += scale * S.dt * vel[3 * i + x];
    if (tid == 0) {
        S.has_v = 1;
        S.steps += 1;
        st[b] = S;
        atomicAdd(n_active, 1);
    }
}

// ---- BFGS ---------------------------------------------------------------------------------------------------------------
struct BfgsState {   // per chain
    int m;           // columns of Q
    int has_prev;    // r0 / f0 hold the previous step's positions / forces
    int steps;
    int converged;
};

__global__ void k_bfgs_init(int B, BfgsState *__restrict__ st, unsigned char *__restrict__ active) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    st[b].m = 0; st[b].has_prev = 0; st[b].steps = 0; st[b].converged = 0;
    active[b] = 1;
}

// Eigen-decomposition of the symmetric m x m matrix A (LDS, row stride ld): cyclic Jacobi with the round-robin parallel
// ordering -- m / 2 disjoint rotations per round, m - 1 rounds per sweep.  On return diag(A) = eigenvalues and the columns
// of Y the eigenvectors (A_in = Y diag Y^T).  cs: 2 * (m / 2 + 1) doubles of scratch.  All threads of the block take part.
__device__ void jacobi_eigh(double *A, double *Y, int m, int ld, double *cs, double *red) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int t = tid; t < m * m; t += nt) Y[(t / m) * ld + t % m] = (t / m == t % m) ? 1.0 : 0.0;
    __syncthreads();
    if (m < 2) return;
    const int me = m + (m & 1);          // players of the tournament (a dummy player when m is odd)
    const int half = me / 2;
    for (int sweep = 0; sweep < 30; ++sweep) {
        // off-diagonal weight against the diagonal
        double off = 0.0, dg = 0.0;
        for (int t = tid; t < m * m; t += nt) {
            const int p = t / m, q = t % m;
            const double v = A[p * ld + q];
            if (p == q) dg += v * v; else off += v * v;
        }
        off = block_sum(off, red);
        dg = block_sum(dg, red);
        if (off <= 1e-30 * dg || off == 0.0) break;
        for (int r = 0; r < me - 1; ++r) {
            // rotation angles of this round's pairs
            if (tid < half) {
                int p = tid == 0 ? me - 1 : (r + tid) % (me - 1);
                int q = tid == 0 ? r : (r - tid + (me - 1)) % (me - 1);
                if (p > q) { const int t2 = p; p = q; q = t2; }
                double c = 1.0, s = 0.0;
                if (q < m) {
                    const double apq = A[p * ld + q];
                    if (apq != 0.0) {
                        const double tau = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                    }
                }
                cs[2 * tid] = c; cs[2 * tid + 1] = s;
            }
            __syncthreads();
            // columns p, q of A and of Y:  (x_p, x_q) <- (c x_p - s x_q, s x_p + c x_q) for every row
            for (int t = tid; t < half * m; t += nt) {
                const int i = t / m, k = t % m;
                int p = i == 0 ? me - 1 : (r + i) % (me - 1);
                int q = i == 0 ? r : (r - i + (me - 1)) % (me - 1);
                if (p > q) { const int t2 = p; p = q; q = t2; }
                if (q >= m) continue;
                const double c = cs[2 * i], s = cs[2 * i + 1];
                const double ap = A[k * ld + p], aq = A[k * ld + q];
                A[k * ld + p] = c * ap - s * aq; A[k * ld + q] = s * ap + c * aq;
                const double yp = Y[k * ld + p], yq = Y[k * ld + q];
                Y[k * ld + p] = c * yp - s * yq; Y[k * ld + q] = s * yp + c * yq;
            }
            __syncthreads();
            // rows p, q of A
            for (int t = tid; t < half * m; t += nt) {
                const int i = t / m, k = t % m;
                int p = i == 0 ? me - 1 : (r + i) % (me - 1);
                int q = i == 0 ? r : (r - i + (me - 1)) % (me - 1);
                if (p > q) { const int t2 = p; p = q; q = t2; }
                if (q >= m) continue;
                const double c = cs[2 * i], s = cs[2 * i + 1];
                const double ap = A[p * ld + k], aq = A[q * ld + k];
                A[p * ld + k] = c * ap - s * aq; A[q * ld + k] = s * ap + c * aq;
            }
            __syncthreads();
        }
    }
}

// One workgroup per chain.  Vectors are over ALL 3 N_b coordinates of the chain with the entries of held atoms zero (their
// force is zeroed and they never move), which is exactly ASE's block structure.  Q: [mmax][3 N_b] rows (basis vectors),
// Bm: [mmax][mmax] (row stride mmax).
__global__ void __launch_bounds__(256)
k_bfgs_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const float *__restrict__ forces,
            const uint8_t *__restrict__ fixed, double fmax_tol, double alpha, double maxstep, int mmax, int max_steps,
            double *__restrict__ pos, double *__restrict__ r0, double *__restrict__ f0, double *__restrict__ Qall,
            double *__restrict__ Ball, double *__restrict__ work /*[3 sum N] step vector*/, BfgsState *__restrict__ st,
            unsigned char *__restrict__ active, int *__restrict__ n_active) {
    extern __shared__ double lds[];
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = nt >> 6;
    if (counters[2]) return;
    const int a0 = cfg_start[b], a1 = cfg_start[b + 1];
    const int n = 3 * (a1 - a0);
    BfgsState S = st[b];
    if (S.converged) return;
    double *Q = Qall + (size_t)3 * a0 * mmax;          // rows of length n
    double *Bm = Ball + (size_t)b * mmax * mmax;
    double *x = pos + 3 * (size_t)a0, *xr0 = r0 + 3 * (size_t)a0, *xf0 = f0 + 3 * (size_t)a0, *w = work + 3 * (size_t)a0;
    const float *fg = forces + 3 * (size_t)a0;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;
    auto F = [&](int k) -> double { return (fx && fx[k / 3]) ? 0.0 : (double)fg[k]; };
    // LDS carve-up
    const int ld = mmax | 1;                             // odd row stride: no bank conflicts on column walks
    double *A = lds, *Y = A + (size_t)mmax * ld, *c1 = Y + (size_t)mmax * ld, *c2 = c1 + mmax, *cf = c2 + mmax,
           *tv = cf + mmax, *cs = tv + mmax;             // cs: mmax + 2

    // ---- convergence: max_i |F_i|^2 < fmax^2 (ase/optimize/optimize.py converged()) ----------------------------------------
    double fm2 = 0.0;
    for (int i = tid; i < a1 - a0; i += nt) {
        const double f0_ = F(3 * i), f1_ = F(3 * i + 1), f2_ = F(3 * i + 2);
        fm2 = fmax(fm2, f0_ * f0_ + f1_ * f1_ + f2_ * f2_);
    }
    fm2 = block_max(fm2, red);
    if (!(fm2 >= fmax_tol * fmax_tol)) {
        if (tid == 0) mark_converged(b, &st[b].converged, active);
        return;
    }
    if (S.steps >= max_steps) return;
    int m = S.m;
    // ---- update of H from the previous step (ase/optimize/bfgs.py update()) -------------------------------------------------
    if (S.has_prev) {
        double mx = 0.0;
        for (int k = tid; k < n; k += nt) mx = fmax(mx, fabs(x[k] - xr0[k]));
        mx = block_max(mx, red);
        if (mx >= 1e-7 && m + 2 <= mmax) {
            // a = dr.df ; c1 = Q^T dr ; xx = |x|^2 over the free coordinates
            double a = 0.0, xx = 0.0;
            for (int k = tid; k < n; k += nt) {
                a += (x[k] - xr0[k]) * (F(k) - xf0[k]);
                if (!(fx && fx[k / 3])) xx += x[k] * x[k];
            }
            a = block_sum(a, red);
            xx = block_sum(xx, red);
            // From the second update on H dr lies in span(Q) in exact arithmetic: dr is |H|^-1 f up to a factor and the span holds
            // every earlier force.  What the candidate keeps outside it is the rounding of x = xr0 + step, at most half an ulp per
            // coordinate and alpha times that in H dr: 1e-13 of |H dr| while the steps are long, 1e-10 once a run has contracted to
            // steps of 1e-4 A -- far above the relative threshold below.  Such a remainder is no column (it was taken for one: a
            // contracting chain filled its basis after 51 updates instead of 96; tests/test_relax_gpu_branches.py).  A direction
            // that H dr really adds measures 1e11 times the rounding (tests/bfgs_oracle.py, dg_noise_ratio); the floor sits 64 x
            // above it.
            const double ROUND = 64.0 * alpha * 1.1102230246251565e-16;   // 64 alpha 2^-53
            const double dg_floor = ROUND * ROUND * xx;
            for (int j = wave; j < m; j += nwaves) {   // one wave per basis vector: no block barrier per dot product
                double d = 0.0;
                for (int k = lane; k < n; k += 64) d += Q[(size_t)j * n + k] * (x[k] - xr0[k]);
                d = wave_sum_f64(d);
                if (lane == 0) c1[j] = d;
            }
            __syncthreads();
            // tv = B c1 ; dg = alpha dr + Q tv -> w ; b = dr.dg
            for (int j = tid; j < m; j += nt) {
                double d = 0.0;
                for (int i = 0; i < m; ++i) d += Bm[(size_t)j * mmax + i] * c1[i];
                tv[j] = d;
            }
            __syncthreads();
            double bb = 0.0;
            for (int k = tid; k < n; k += nt) {
                const double dr = x[k] - xr0[k];
                double g = alpha * dr;
                for (int j = 0; j < m; ++j) g += Q[(size_t)j * n + k] * tv[j];
                w[k] = g;
                bb += dr * g;
            }
            bb = block_sum(bb, red);
            // append the two update vectors to the basis: coefficients c1 (df), c2 (dg) in the extended basis.
            // Two Gram-Schmidt passes ("twice is enough"); a vector already inside span(Q) adds no column.
            for (int which = 0; which < 2; ++which) {
                double *cc = which == 0 ? c1 : c2;
                double *qn = Q + (size_t)m * n;            // candidate column
                double nrm0 = 0.0;
                for (int k = tid; k < n; k += nt) {
                    const double v = which == 0 ? F(k) - xf0[k] : w[k];
                    qn[k] = v;
                    nrm0 += v * v;
                }
                nrm0 = block_sum(nrm0, red);
                for (int j = tid; j < mmax; j += nt) cc[j] = 0.0;
                __syncthreads();
                // classical Gram-Schmidt, twice ("twice is enough"): all m projections of a pass at once (a wave per basis vector),
                // then one sweep over the candidate -- 2 x 2 barriers instead of 2 m block reductions (it was the modified form,
                // sequential in j: ~170 of the kernel's ~250 reductions at m = 42)
                for (int pass = 0; pass < 2; ++pass) {
                    for (int j = wave; j < m; j += nwaves) {
                        double d = 0.0;
                        for (int k = lane; k < n; k += 64) d += Q[(size_t)j * n + k] * qn[k];
                        d = wave_sum_f64(d);
                        if (lane == 0) tv[j] = d;
                    }
                    __syncthreads();
                    for (int k = tid; k < n; k += nt) {
                        double v = qn[k];
                        for (int j = 0; j < m; ++j) v -= tv[j] * Q[(size_t)j * n + k];
                        qn[k] = v;
                    }
                    for (int j = tid; j < m; j += nt) cc[j] += tv[j];
                    __syncthreads();
                }
                double nrm = 0.0;
                for (int k = tid; k < n; k += nt) nrm += qn[k] * qn[k];
                nrm = block_sum(nrm, red);
                if (nrm > 1e-24 * nrm0 && nrm > 0.0 && (which == 0 || nrm > dg_floor)) {
                    const double inv = 1.0 / sqrt(nrm);
                    for (int k = tid; k < n; k += nt) qn[k] *= inv;
                    if (tid == 0) cc[m] = sqrt(nrm);
                    // new row / column of B (zeros)
                    for (int j = tid; j <= m; j += nt) { Bm[(size_t)m * mmax + j] = 0.0; Bm[(size_t)j * mmax + m] = 0.0; }
                    ++m;
                }
                __syncthreads();
            }
            // B -= c1 c1^T / a + c2 c2^T / b
            for (int t = tid; t < m * m; t += nt) {
                const int i = t / m, j = t % m;
                Bm[(size_t)i * mmax + j] -= c1[i] * c1[j] / a + c2[i] * c2[j] / bb;
            }
            __syncthreads();
        }
    }
    // ---- step: dr = |H|^-1 f -------------------------------------------------------------------------------------------------
    for (int t = tid; t < m * m; t += nt) {
        const int i = t / m, j = t % m;
        A[i * ld + j] = Bm[(size_t)i * mmax + j] + (i == j ? alpha : 0.0);
    }
    __syncthreads();
    jacobi_eigh(A, Y, m, ld, cs, red);
    for (int j = wave; j < m; j += nwaves) {   // cf = Q^T f, a wave per basis vector
        double d = 0.0;
        for (int k = lane; k < n; k += 64) d += Q[(size_t)j * n + k] * F(k);
        d = wave_sum_f64(d);
        if (lane == 0) cf[j] = d;
    }
    __syncthreads();
    for (int j = tid; j < m; j += nt) {   // tv = |L|^-1 Y^T cf
        double d = 0.0;
        for (int i = 0; i < m; ++i) d += Y[i * ld + j] * cf[i];
        tv[j] = d / fabs(A[j * ld + j]);
    }
    __syncthreads();
    for (int i = tid; i < m; i += nt) {   // c1 = Y tv - cf / alpha   (coefficients of Q in the step)
        double d = 0.0;
        for (int j = 0; j < m; ++j) d += Y[i * ld + j] * tv[j];
        c1[i] = d - cf[i] / alpha;
    }
    __syncthreads();
    double mx2 = 0.0;
    for (int i = tid; i < a1 - a0; i += nt) {
        double s2 = 0.0;
        for (int xk = 0; xk < 3; ++xk) {
            const int k = 3 * i + xk;
            double d = F(k) / alpha;
            for (int j = 0; j < m; ++j) d += Q[(size_t)j * n + k] * c1[j];
            w[k] = d;
            s2 += d * d;
        }
        mx2 = fmax(mx2, s2);
    }
    mx2 = block_max(mx2, red);
    const double longest = sqrt(mx2);
    const double scale = longest >= maxstep ? maxstep / longest : 1.0;
    for (int k = tid; k < n; k += nt) {
        xr0[k] = x[k];
        xf0[k] = F(k);
        x[k] += scale * w[k];
    }
    if (tid == 0) {
        S.m = m;
        S.has_prev = 1;
        S.steps += 1;
        st[b] = S;
        atomicAdd(n_active, 1);
    }
}

__global__ void k_narrow_forces(int n3, const double *__restrict__ f64, float *__restrict__ f32) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) f32[i] = (float)f64[i];
}

template <class State>
__global__ void k_relax_report(int B, const State *__restrict__ st, int *__restrict__ steps, uint8_t *__restrict__ conv) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    steps[b] = st[b].steps;
    conv[b] = (uint8_t)st[b].converged;
}

// ---- trajectory observer ----------------------------------------------------------------------------------------------------
// Counterpart of TrajectoryObserver + dyn.attach(obs, interval=record_interval) (reference mcmc/dynamics.py:20-80,131-151): ASE
// calls the observer after the initial evaluation (nsteps = 0) and after every step whose count is a multiple of the
// interval, including the step after which the run stops.  Here: after the evaluation of an iteration and before its step
// kernel, every chain that is still running and whose own step counter is a multiple of the interval copies its positions,
// forces (FixAtoms applied, like atoms.get_forces()) and energy into record steps / interval.  The chain's counter is used,
// not the driver's iteration index: the two part after a neighbor-capacity regrow.
template <class State>
__global__ void __launch_bounds__(256)
k_traj_record(const int *__restrict__ cfg_start, const int *__restrict__ counters, const State *__restrict__ st,
              const unsigned char *__restrict__ active, int interval, int nrec, int B, int N, const uint8_t *__restrict__ fixed,
              const double *__restrict__ pos, const float *__restrict__ forces, const float *__restrict__ e32,
              const double *__restrict__ e64, double *__restrict__ ring_pos, float *__restrict__ ring_f,
              double *__restrict__ ring_e, int *__restrict__ ring_n) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (counters[2] || !active[b]) return;
    const int steps = st[b].steps;
    if (st[b].converged || steps % interval) return;
    const int r = steps / interval;
    if (r >= nrec) return;
    const int a0 = cfg_start[b], a1 = cfg_start[b + 1];
    for (int k = 3 * a0 + tid; k < 3 * a1; k += blockDim.x) {
        ring_pos[(size_t)r * 3 * N + k] = pos[k];
        ring_f[(size_t)r * 3 * N + k] = (fixed && fixed[k / 3]) ? 0.f : forces[k];
    }
    if (tid == 0) {
        ring_e[(size_t)r * B + b] = e64 ? e64[b] : (double)e32[b];
        if (ring_n[b] < r + 1) ring_n[b] = r + 1;
    }
}

// ---- the frame of a driver call (vssr_internal.h), shared by every driver's entry point ---------------------------------------
int driver_guard(vssr_handle *h, const char *func) {
    if (int rc = check_kind(h, KINDS_EVAL, func)) return rc;
    if (!h->batch_valid) return set_err(h, VSSR_E_STATE, "%s before vssr_batch_upload", func);
    return VSSR_OK;
}

// Per-relaxation buffers, the FixAtoms mask on the device (`fixed`: null without a mask), the work counters at zero.
int driver_open(vssr_handle *h, const uint8_t *fixed_host, int steps_ints_per_chain, const uint8_t *&fixed, uint32_t want) {
    const size_t B = h->n_cfg, N = h->n_atoms;
    if (h->d_fixed.ensure(N) || h->d_relax_steps.ensure(sizeof(int) * steps_ints_per_chain * B) || h->d_relax_conv.ensure(B) ||
        h->d_active.ensure(B) || h->d_counters.ensure(sizeof(int) * 4))
        return set_err(h, VSSR_E_NOMEM, "relaxation state: out of device memory");
    if (fixed_host) VSSR_HIP(h, hipMemcpyAsync(h->d_fixed.p, fixed_host, N, hipMemcpyHostToDevice, h->stream));
    fixed = fixed_host ? h->d_fixed.as<uint8_t>() : nullptr;
    h->relax_lockstep = h->relax_chain_evals = h->relax_compactions = 0;
    h->relax_regrows = 0;
    h->last_want = want | VSSR_WANT_FORCES;
    return VSSR_OK;
}

int driver_close(vssr_handle *h, bool partial) {
    h->ran = true;
    h->graph_partial = partial;
    return sync_and_check(h);
}

// Neighbor capacity overflow seen at a poll: grow (at most `cap` times per relaxation) and give the polling window back: the step
// kernels behind the overflowed evaluations moved nothing and counted nothing; chains that did step are held by their own counters.
int relax_regrow(vssr_handle *h, int cap, long long &it, int window) {
    if (int rc = grow_slot_cap(h)) return rc;
    if (++h->relax_regrows > cap) return set_err(h, VSSR_E_CAPACITY, "neighbor capacity could not be satisfied");
    it = std::max(it - window, -1LL);
    return VSSR_OK;
}

int relax_results(vssr_handle *h, bool partial, double *pos_out, std::initializer_list<int32_t *> cols) {
    if (int rc = driver_close(h, partial)) return rc;
    if (pos_out) VSSR_HIP(h, hipMemcpy(pos_out, h->d_pos.p, sizeof(double) * 3 * h->n_atoms, hipMemcpyDeviceToHost));
    const size_t k = cols.size();
    std::vector<int> rep(k * h->n_cfg);
    VSSR_HIP(h, hipMemcpy(rep.data(), h->d_relax_steps.p, sizeof(int) * rep.size(), hipMemcpyDeviceToHost));
    size_t c = 0;
    for (int32_t *col : cols) {
        if (col)
            for (int b = 0; b < h->n_cfg; ++b) col[b] = rep[k * b + c];
        ++c;
    }
    return VSSR_OK;
}

// ---- the two optimizers of the frame: a typed workspace on the handle's d_opt_state / d_opt_vec (as CgWork, cg_dev.h) that
// knows its two launches.  init sizes the buffers, hands out the pointers and resets every chain ---------------------------
struct FireWork {
    using Params = vssr_fire_params; using State = FireState;
    FireState *st;
    double *vel;   // [3 N]
    int init(vssr_handle *h, const Params &p) {
        if (h->d_opt_vec.ensure(sizeof(double) * 3 * h->n_atoms) || h->d_opt_state.ensure(sizeof(FireState) * h->n_cfg))
            return set_err(h, VSSR_E_NOMEM, "FIRE state: out of device memory");
        st = h->d_opt_state.as<FireState>(); vel = h->d_opt_vec.as<double>();
        hipLaunchKernelGGL(k_fire_init, dim3((h->n_cfg + 127) / 128), dim3(128), 0, h->stream, h->n_cfg, (double)p.dt, (double)p.astart, st,
                           h->d_active.as<unsigned char>());
        return VSSR_OK;
    }
    void step(vssr_handle *h, const Params &p, const uint8_t *fixed) const {
        hipLaunchKernelGGL(k_fire_step, dim3(h->n_cfg), dim3(256), 0, h->stream, h->d_cfg_start.as<int>(), h->d_counters.as<int>(),
                           h->d_forces.as<float>(), fixed, (double)p.fmax, (double)p.maxstep, (double)p.dtmax, (double)p.finc, (double)p.fdec,
                           (double)p.astart, (double)p.fa, p.nmin, p.max_steps, h->d_pos.as<double>(), vel, st,
                           h->d_active.as<unsigned char>(), h->d_counters.as<int>() + 3);
    }
};
struct BfgsWork {
    using Params = vssr_bfgs_params; using State = BfgsState;
    BfgsState *st;
    double *r0, *f0, *work, *Q, *B;   // [3 N] each, [mmax][3 N], [n_cfg][mmax][mmax]
    int mmax;
    size_t lds_bytes() const { return sizeof(double) * ((size_t)2 * mmax * (mmax | 1) + 5 * (size_t)mmax + 8); }
    int init(vssr_handle *h, const Params &p) {
        // At most two basis vectors per Hessian update; the rotated matrices of the eigen-decomposition (2 x mmax^2 doubles) live
        // in LDS, which holds mmax = 98 of them.  The first update takes two columns, every later one one (H dr lies in the span
        // already, see k_bfgs_step): 96 updates.  A longer relaxation keeps stepping with the Hessian of its first 96 updates (the
        // step kernel skips an update that finds fewer than two columns free): identical to ASE for 97 steps, a frozen
        // quasi-Newton method beyond (the reference's configurations use 20 steps; a chain with fewer than 33 free atoms never
        // fills the basis, m <= 3 N).  Pinned step for step by tests/test_relax_gpu_branches.py.
        const size_t nB = h->n_cfg, N = h->n_atoms;
        mmax = 2 * p.max_steps + 2;
        while (lds_bytes() > 160 * 1024 - 4096) mmax -= 2;   // (the kernel also holds 2 KB of static reduction scratch)
        if (h->d_opt_state.ensure(sizeof(BfgsState) * nB) || h->d_opt_vec.ensure(sizeof(double) * 9 * N) ||
            h->d_bfgs_q.ensure(sizeof(double) * 3 * N * mmax) || h->d_bfgs_b.ensure(sizeof(double) * nB * mmax * mmax))
            return set_err(h, VSSR_E_NOMEM, "BFGS state: out of device memory");
        VSSR_HIP(h, hipFuncSetAttribute((const void *)k_bfgs_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes()));
        st = h->d_opt_state.as<BfgsState>();
        r0 = h->d_opt_vec.as<double>(); f0 = r0 + 3 * N; work = r0 + 6 * N; Q = h->d_bfgs_q.as<double>(); B = h->d_bfgs_b.as<double>();
        hipLaunchKernelGGL(k_bfgs_init, dim3((h->n_cfg + 127) / 128), dim3(128), 0, h->stream, h->n_cfg, st, h->d_active.as<unsigned char>());
        return VSSR_OK;
    }
    void step(vssr_handle *h, const Params &p, const uint8_t *fixed) const {
        hipLaunchKernelGGL(k_bfgs_step, dim3(h->n_cfg), dim3(256), lds_bytes(), h->stream, h->d_cfg_start.as<int>(), h->d_counters.as<int>(),
                           h->d_forces.as<float>(), fixed, (double)p.fmax, (double)p.alpha, (double)p.maxstep, mmax, p.max_steps,
                           h->d_pos.as<double>(), r0, f0, Q, B, work, st, h->d_active.as<unsigned char>(), h->d_counters.as<int>() + 3);
    }
};

// ---- host driver ----------------------------------------------------------------------------------------------------------
// Iteration i: evaluate energies / forces of the chains still active, then (device side) test convergence and step.  The host
// only enqueues; every POLL iterations it reads the number of chains that took a step and the neighbor-capacity flag.  If
// the capacity overflowed, the step kernels of the affected iterations did nothing (they test the flag): the buffers are
// regrown and the loop continues from the same positions.  Iterations enqueued after every chain has converged find no
// active chain and cost only their (empty) launches.
template <class Work>
int relax_lockstep(vssr_handle *h, const typename Work::Params &p, const uint8_t *fixed_host, uint32_t want) {
    const int B = h->n_cfg, N = h->n_atoms;
    hipStream_t st = h->stream;
    const int max_steps = p.max_steps;
    const uint8_t *fixed = nullptr;
    Work w;
    if (int e = driver_open(h, fixed_host, 1, fixed, want)) return e;
    if (int e = w.init(h, p)) return e;
    int rc = VSSR_OK;
    unsigned char *active = h->d_active.as<unsigned char>();
    // The evaluation kernels skip chains whose entry of `active` is 0 -- once the mask is handed to them.  While every chain is
    // still running the mask stays away (h->active_mask = nullptr): the masked forms of the kernels cost ~0.15 ms per evaluation
    // (tile / chain tests, the per-chain instead of the streaming gradient reduction), and with the reference's settings (fmax
    // 0.01 within 20 steps) no chain ever converges.  The host learns at a poll that a chain has stopped stepping and installs
    // the mask from then on; a chain that converged inside the current poll window is evaluated a few more times at its final
    // positions, which reproduces its results bit for bit.
    h->active_mask = nullptr;
    bool masked = false;
    int *n_active_d = h->d_counters.as<int>() + 3;   // counters[3] is free for this purpose
    const int rec_iv = h->traj_interval, nrec = rec_iv > 0 ? max_steps / rec_iv + 1 : 0;
    h->traj_records = 0;
    if (nrec) {
        if (h->d_traj_pos.ensure(sizeof(double) * 3 * (size_t)N * nrec) || h->d_traj_f.ensure(sizeof(float) * 3 * (size_t)N * nrec) ||
            h->d_traj_e.ensure(sizeof(double) * (size_t)B * nrec) || h->d_traj_n.ensure(sizeof(int) * B))
            return set_err(h, VSSR_E_NOMEM, "trajectory records: out of device memory");
        VSSR_HIP(h, hipMemsetAsync(h->d_traj_n.p, 0, sizeof(int) * B, st));
        h->traj_records = nrec; h->traj_B = B; h->traj_N = N;
    }
    const bool f64 = is_analytic(h);   // Tersoff / EAM / SW / pair forces are fp64 on the device: the optimizer state works on an fp32 copy
    const int POLL = 4;
    for (long long it = 0; it <= max_steps && !rc; ++it) {
        if ((rc = evaluator(h).run(h, want | VSSR_WANT_FORCES))) break;
        ++h->relax_lockstep;
        h->relax_chain_evals += B;
        // (last iteration: every unconverged chain has taken relax_steps steps -- the kernel only tests convergence, like the
        // final check of ASE's run loop)
        const bool last = it == max_steps;
        VSSR_HIP(h, hipMemsetAsync(n_active_d, 0, sizeof(int), st));
        if (f64) {
            if (h->d_forces.ensure(sizeof(float) * 3 * N)) { rc = set_err(h, VSSR_E_NOMEM, "force buffer"); break; }
            hipLaunchKernelGGL(k_narrow_forces, dim3((3 * N + 255) / 256), dim3(256), 0, st, 3 * N, h->d_pot_f.as<double>(),
                               h->d_forces.as<float>());
        }
        const float *forces = h->d_forces.as<float>();
        if (nrec)
            hipLaunchKernelGGL(k_traj_record<typename Work::State>, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(), h->d_counters.as<int>(), w.st, active, rec_iv,
                               nrec, B, N, fixed, h->d_pos.as<double>(), forces, f64 ? nullptr : h->d_energy.as<float>(),
                               f64 ? h->d_pot_e.as<double>() : nullptr, h->d_traj_pos.as<double>(), h->d_traj_f.as<float>(),
                               h->d_traj_e.as<double>(), h->d_traj_n.as<int>());
        w.step(h, p, fixed);
        VSSR_HIP(h, hipMemcpyAsync(h->h_counters + 3, n_active_d, sizeof(int), hipMemcpyDeviceToHost, st));
        if (last || (it + 1) % POLL == 0) {
            VSSR_HIP(h, hipStreamSynchronize(st));
            // neighbor capacity overflow in one of the enqueued evaluations: grow, redo
            if (h->h_counters[2]) { rc = relax_regrow(h, h->cap_tight ? 64 : 8, it, POLL); continue; }
            if (!last && h->h_counters[3] == 0) break;   // no chain stepped in the last iteration: all converged, results final
            // (never at the final poll: the last evaluation above ran unmasked over every chain, the resident graph is complete)
            if (!last && !masked && h->h_counters[3] < B) { h->active_mask = active; masked = true; }
        }
    }
    h->active_mask = nullptr;
    if (rc) return rc;
    hipLaunchKernelGGL(k_relax_report<typename Work::State>, dim3((B + 127) / 128), dim3(128), 0, st, B, w.st, h->d_relax_steps.as<int>(),
                       h->d_relax_conv.as<uint8_t>());
    VSSR_HIP(h, hipGetLastError());
    h->ran = true;
    h->graph_partial = masked;   // (with the mask in place the last evaluation covered only the chains still running: see vssr_batch_stats)
    return VSSR_OK;
}

int relax_fire(vssr_handle *h, const vssr_fire_params &p, const uint8_t *fixed, uint32_t want) { return relax_lockstep<FireWork>(h, p, fixed, want); }
int relax_bfgs(vssr_handle *h, const vssr_bfgs_params &p, const uint8_t *fixed, uint32_t want) { return relax_lockstep<BfgsWork>(h, p, fixed, want); }

}  // namespace vssr
