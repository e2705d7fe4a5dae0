// jacobi_dev.h — the fp64 cyclic Jacobi eigen-solver of one workgroup, shared by k_clu_eigh (cluster.hip: one covariance matrix) and
// k_vib_eigh (vib.hip: one mass-weighted Hessian per workgroup).  Round-robin parallel ordering: m / 2 disjoint rotations per step,
// m - 1 steps per sweep (an odd m plays with one idle seat); a rotation is skipped once |a_pq| <= eps |src|_F / m; every sweep ends by
// mirroring the upper triangle into the lower; the solve ends with the first sweep that rotates nothing.  Every order is fixed and the
// build keeps -ffp-contract=off, so the bits depend on the matrix alone, not on where A and Vt live (global memory or LDS) nor on
// their leading dimension.
#ifndef VSSR_JACOBI_DEV_H
#define VSSR_JACOBI_DEV_H
#include <hip/hip_runtime.h>

#include <cfloat>

namespace vssr {

constexpr int EIGH_THREADS = 1024, EIGH_MAX_SWEEPS = 60;

// pair i of step r of the round-robin tournament of `me` players (me even): (p, q), p < q
__device__ __forceinline__ void rr_pair(int i, int r, int me, int &p, int &q) {
    p = i == 0 ? me - 1 : (r + i) % (me - 1);
    q = i == 0 ? r : (r - i + (me - 1)) % (me - 1);
    if (p > q) { const int t = p; p = q; q = t; }
}

// Every thread of the EIGH_THREADS-thread workgroup calls it.  A [m][ld] <- src [m][ld_src], Vt [m][ld] <- I; on return
// diag(A) = eigenvalues, ROWS of Vt = eigenvectors.  cs: 256 doubles, red: EIGH_THREADS doubles, rotated: one int, all LDS.
// sweep: sweeps run; conv: 1 when the last sweep rotated nothing.
__device__ __forceinline__ void jacobi_eigh(const double *__restrict__ src, int ld_src, double *A, double *Vt, int m, int ld, double *cs,
                                            double *red, int *rotated, int &sweep, int &conv) {
    const int tid = threadIdx.x, nt = EIGH_THREADS;
    double f2 = 0.0;
    for (int t = tid; t < m * m; t += nt) {
        const int i = t / m, j = t - i * m;
        const double v = src[(size_t)i * ld_src + j];
        A[(size_t)i * ld + j] = v;
        Vt[(size_t)i * ld + j] = i == j ? 1.0 : 0.0;
        f2 += v * v;
    }
    red[tid] = f2;
    __syncthreads();
    for (int w = nt / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double tol = DBL_EPSILON * sqrt(red[0]) / (double)m;
    const int me = m + (m & 1), half = me / 2;
    sweep = 0; conv = m < 2 ? 1 : 0;
    for (; sweep < EIGH_MAX_SWEEPS && !conv; ++sweep) {
        if (tid == 0) *rotated = 0;
        __syncthreads();
        for (int r = 0; r < me - 1; ++r) {
            if (tid < half) {
                int p, q;
                rr_pair(tid, r, me, p, q);
                double c = 1.0, s = 0.0;
                if (q < m) {
                    const double apq = A[(size_t)p * ld + q];
                    if (fabs(apq) > tol) {
                        const double tau = (A[(size_t)q * ld + q] - A[(size_t)p * ld + p]) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                        *rotated = 1;   // (same value from every writer)
                    }
                }
                cs[2 * tid] = c; cs[2 * tid + 1] = s;
            }
            __syncthreads();
            // columns p, q of A: consecutive threads take the pairs of one row (one row = a few cache lines)
            for (int t = tid; t < half * m; t += nt) {
                const int k = t / half, i = t - k * half;
                int p, q;
                rr_pair(i, r, me, p, q);
                const double c = cs[2 * i], s = cs[2 * i + 1];
                if (q >= m || s == 0.0) continue;
                const double ap = A[(size_t)k * ld + p], aq = A[(size_t)k * ld + q];
                A[(size_t)k * ld + p] = c * ap - s * aq;
                A[(size_t)k * ld + q] = s * ap + c * aq;
            }
            __syncthreads();
            // rows p, q of A and of Vt
            for (int t = tid; t < half * m; t += nt) {
                const int i = t / m, k = t - i * m;
                int p, q;
                rr_pair(i, r, me, p, q);
                const double c = cs[2 * i], s = cs[2 * i + 1];
                if (q >= m || s == 0.0) continue;
                const double ap = A[(size_t)p * ld + k], aq = A[(size_t)q * ld + k];
                A[(size_t)p * ld + k] = c * ap - s * aq;
                A[(size_t)q * ld + k] = s * ap + c * aq;
                const double vp = Vt[(size_t)p * ld + k], vq = Vt[(size_t)q * ld + k];
                Vt[(size_t)p * ld + k] = c * vp - s * vq;
                Vt[(size_t)q * ld + k] = s * vp + c * vq;
            }
            __syncthreads();
        }
        // The column and the row pass round a_pq and a_qp differently, and a rotation (an orthogonal similarity) keeps the norm of
        // an antisymmetric part: what the first sweeps round into it (eps times the entries of then, about tol) would stay above
        // tol in a_pq for good, and a matrix of low rank never ended.  The upper triangle is the matrix: mirror it.
        for (int t = tid; t < m * m; t += nt) {
            const int i = t / m, j = t - i * m;
            if (j < i) A[(size_t)i * ld + j] = A[(size_t)j * ld + i];
        }
        conv = *rotated ? 0 : 1;
        __syncthreads();
    }
}

}  // namespace vssr
#endif
