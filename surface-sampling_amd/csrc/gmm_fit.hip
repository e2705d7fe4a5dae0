// gmm_fit.hip — expectation-maximisation fit of the embedding Gaussian mixture, fp64 throughout (reference mcmc/uncertainty/gmm.py, a copy
// of sklearn.mixture.GaussianMixture whose matrix products are blocked).
//
// Rows live on the device as fp64 [N][Dp] (Dp = D padded to 16, zero columns): the layout k_gmm_logp reads.  The mixture being fitted
// lives in the handle's scoring buffers (d_gmm_P / d_gmm_c / d_gmm_kc / d_gmm_mask), so the E step IS the scoring kernel (gmm_score_f64)
// followed by k_fit_resp:  r_nk = exp(logp_nk + log w_k + NLL_n),  lower bound = mean_n(-NLL_n).
// M step (gmm.py:164-281):  n_k = sum_n r_nk + 10 eps,  mu_k = sum_n r_nk x_n / n_k  (k_fit_moments: row slabs, k_fit_means: slabs summed
// in order), then the covariances:
//   full  S_k = sum_n r_nk (x_n - mu_k)(x_n - mu_k)^T / n_k + reg I   k_fit_cov on v_mfma_f64_16x16x4_f64: a wave owns one 16-row block
//         row ib of the output and up to four column blocks jb <= ib (four independent accumulator chains); the k index of the matrix
//         product is the sample: A = r_n (x_n - mu)[16 ib ..], B = (x_n - mu)[16 jb ..], four samples per instruction.  Only blocks on or
//         below the diagonal are computed; every row slab writes partial [Dp][Dp] tiles, k_fit_cov_finish sums them in slab order,
//         divides, adds reg and mirrors.
//   tied  the same kernel with r = 1, mu = 0 gives X^T X; finish: (X^T X - sum_k n_k mu_k mu_k^T) / sum_k n_k + reg I
//   diag / spherical  vector reductions of r x^2 next to r x (k_fit_moments), gmm.py:211-247 term by term (k_fit_cov_diag)
// Precision factors (gmm.py:284-327): k_fit_chol, one workgroup per component: L = chol(S_k) (right-looking, in a global workspace that
// stays in L2: 128 x 128 doubles do not fit the 64 KB of static LDS, and one code path through generic pointers would emit FLAT
// accesses), Y = L^-1 by forward substitution (one thread per column), P_k = Y^T, log det P_k, c_k = mu_k P_k, block mask -- written
// straight into the scoring layout.  A pivot that is not positive sets flags[k]; nothing aborts on the device.
// Every reduction has a fixed order (slab partials, then sequential or tree sums): no floating-point atomics, a fit is reproducible bit
// for bit.  C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg; A / B: lane l holds A[row l & 15][k = l >> 4] and
// B[k = l >> 4][col l & 15].
#include <cfloat>
#include <cmath>

#include "vssr_internal.h"

namespace vssr {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- E step tail ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_256(double v, double *red) {   // fixed tree over the 256 threads; result in every thread
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(256)
k_fit_resp(const double *__restrict__ lp, const double *__restrict__ kc, const double *__restrict__ nll, int n, int K,
           double *__restrict__ resp, double *__restrict__ part) {
    __shared__ double red[256];
    const int row = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (row < n) {
        const double nl = nll[row];
        v = -nl;
        for (int k = 0; k < K; ++k) resp[(size_t)row * K + k] = exp((lp[(size_t)row * K + k] + kc[K + k]) + nl);
    }
    const double s = block_sum_256(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup: out[0] = scale * sum(part[0 .. m)), strided per thread, then the fixed tree
__global__ void __launch_bounds__(256)
k_fit_sum(const double *__restrict__ part, int m, double scale, double *__restrict__ out) {
    __shared__ double red[256];
    double v = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) v += part[i];
    const double s = block_sum_256(v, red);
    if (threadIdx.x == 0) out[0] = s * scale;
}

// status[0] = value[0], or NaN when a component's covariance was refused
__global__ void k_fit_status(const int *__restrict__ flags, int K, const double *__restrict__ value, double *__restrict__ status) {
    if (threadIdx.x || blockIdx.x) return;
    int bad = 0;
    for (int k = 0; k < K; ++k) bad |= flags[k];
    status[0] = bad ? NAN : value[0];
}

// ---- M step: n_k, means, second moments ----------------------------------------------------------------------------------------------
// grid (slabs, K), thread d: partial sums over the slab's rows, in row order.  resp == nullptr: one-hot responsibilities from labels.
__global__ void __launch_bounds__(256)
k_fit_moments(const double *__restrict__ X, int n, int Dp, const double *__restrict__ resp, const int *__restrict__ labels, int K,
              int rows_per_slab, int want_sq, double *__restrict__ part_s, double *__restrict__ part_q, double *__restrict__ part_n) {
    const int d = threadIdx.x, k = blockIdx.y, sl = blockIdx.x;
    if (d >= Dp) return;
    const int r0 = sl * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
    double s = 0.0, q = 0.0, cnt = 0.0;
    for (int row = r0; row < r1; ++row) {
        const double r = resp ? resp[(size_t)row * K + k] : (labels[row] == k ? 1.0 : 0.0);
        const double x = X[(size_t)row * Dp + d];
        s += r * x;
        if (want_sq) q += r * (x * x);
        cnt += r;
    }
    const size_t o = ((size_t)sl * K + k) * Dp + d;
    part_s[o] = s;
    if (want_sq) part_q[o] = q;
    if (d == 0) part_n[(size_t)sl * K + k] = cnt;
}

// grid K, thread d: slabs summed in order; n_k = sum + 10 eps, mu_k = sum_s / n_k, avg_x2 = sum_q / n_k
__global__ void __launch_bounds__(256)
k_fit_means(const double *__restrict__ part_s, const double *__restrict__ part_q, const double *__restrict__ part_n, int S, int K,
            int Dp, int want_sq, double *__restrict__ nk, double *__restrict__ means, double *__restrict__ avg_x2) {
    const int d = threadIdx.x, k = blockIdx.x;
    if (d >= Dp) return;
    double cnt = 0.0, s = 0.0, q = 0.0;
    for (int sl = 0; sl < S; ++sl) {
        cnt += part_n[(size_t)sl * K + k];
        s += part_s[((size_t)sl * K + k) * Dp + d];
        if (want_sq) q += part_q[((size_t)sl * K + k) * Dp + d];
    }
    cnt += 10.0 * DBL_EPSILON;
    means[(size_t)k * Dp + d] = s / cnt;
    if (want_sq) avg_x2[(size_t)k * Dp + d] = q / cnt;
    if (d == 0) nk[k] = cnt;
}

// one thread: w_k = n_k / n (initialisation) or n_k / sum_k n_k (M step); log w_k into the scoring constants
__global__ void k_fit_weights(const double *__restrict__ nk, int K, double n_rows, double *__restrict__ w, double *__restrict__ kc) {
    if (threadIdx.x || blockIdx.x) return;
    double tot = n_rows;
    if (!(tot > 0.0)) {
        tot = 0.0;
        for (int k = 0; k < K; ++k) tot += nk[k];
    }
    for (int k = 0; k < K; ++k) {
        const double v = nk[k] / tot;
        w[k] = v;
        kc[K + k] = log(v);
    }
}

// ---- M step: full / tied covariance on the matrix pipe -----------------------------------------------------------------------------------
// tasks of a [NB][NB] block matrix: block row ib with column blocks 4 jg .. 4 jg + 3 (<= ib)
__host__ __device__ inline int fit_cov_tasks(int NB) {
    int t = 0;
    for (int i = 0; i < NB; ++i) t += (i + 4) / 4;
    return t;
}

// grid (slabs, components, ceil(tasks / 4)), one task per wave.  resp == nullptr: r = 1; means == nullptr: mu = 0 (tied: X^T X).
// part: [slabs][components][Dp][Dp], written on and below the block diagonal.
__global__ void __launch_bounds__(256)
k_fit_cov(const double *__restrict__ X, int n, int Dp, const double *__restrict__ resp, int K, const double *__restrict__ means,
          int rows_per_slab, double *__restrict__ part) {
    __shared__ double fence[256];   // written, never read (see k_gmm_logp)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int NB = Dp >> 4;
    const int task = blockIdx.z * 4 + wave;
    int ib = -1, jg = 0;
    for (int i = 0, t = 0; i < NB; ++i) {
        const int g = (i + 4) / 4;
        if (task < t + g) { ib = i; jg = task - t; break; }
        t += g;
    }
    if (ib < 0) return;   // (no barrier below)
    const int k = blockIdx.y, Kc = gridDim.y;
    const int nj = min(4, ib + 1 - 4 * jg);
    int jb[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) jb[c] = c < nj ? 4 * jg + c : ib;   // spare chains repeat the diagonal block and are not stored
    const int g = lane >> 4, col = lane & 15;
    const double mua = means ? means[(size_t)k * Dp + 16 * ib + col] : 0.0;
    double mub[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) mub[c] = means ? means[(size_t)k * Dp + 16 * jb[c] + col] : 0.0;
    const int r0 = blockIdx.x * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
    f64x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    double xa, xb[4], rr;
    auto fetch = [&](int base) {   // sample base + g of the 4-sample step (rows past the slab: r = 0 on a clamped row)
        const int row = base + g, rc = min(row, n - 1);
        const double *xr = X + (size_t)rc * Dp + col;
        xa = xr[16 * ib];
#pragma unroll
        for (int c = 0; c < 4; ++c) xb[c] = xr[16 * jb[c]];
        rr = row < r1 ? (resp ? resp[(size_t)rc * K + k] : 1.0) : 0.0;
    };
    fetch(r0);
#pragma unroll 1
    for (int base = r0; base < r1; base += 4) {
        const double a = rr * (xa - mua);
        double b[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = xb[c] - mub[c];
        if (base + 4 < r1) fetch(base + 4);   // the next step's loads leave before the matrix block, none inside it
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {   // four independent chains: an accumulator's producer is four matrix instructions back
            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[c], acc[c], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        *(volatile __attribute__((address_space(3))) double *)(fence + tid) = acc[3][0];
        __builtin_amdgcn_sched_barrier(0);
    }
    double *out = part + ((size_t)blockIdx.x * Kc + k) * Dp * Dp;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c >= nj) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(16 * ib + g + 4 * r) * Dp + 16 * jb[c] + col] = acc[c][r];
    }
}

// grid (components, Dp), thread j: element (i, j) from the partial at (max, min), slabs in order.  tied = 0: / n_k + reg on the
// diagonal; tied = 1: (X^T X - sum_k n_k mu_k mu_k^T) / sum_k n_k + reg.  Pad rows / columns are zero.
__global__ void __launch_bounds__(256)
k_fit_cov_finish(const double *__restrict__ part, int S, int D, int Dp, int K, int tied, const double *__restrict__ nk,
                 const double *__restrict__ means, double reg, double *__restrict__ cov) {
    const int j = threadIdx.x, i = blockIdx.y, k = blockIdx.x, Kc = gridDim.x;
    if (j >= Dp) return;
    double v = 0.0;
    if (i < D && j < D) {
        const int hi = max(i, j), lo = min(i, j);
        double s = 0.0;
        for (int sl = 0; sl < S; ++sl) s += part[(((size_t)sl * Kc + k) * Dp + hi) * Dp + lo];
        if (tied) {
            double m2 = 0.0, tot = 0.0;
            for (int c = 0; c < K; ++c) {
                m2 += (nk[c] * means[(size_t)c * Dp + i]) * means[(size_t)c * Dp + j];
                tot += nk[c];
            }
            v = (s - m2) / tot;
        } else {
            v = s / nk[k];
        }
        if (i == j) v += reg;
    }
    cov[((size_t)k * Dp + i) * Dp + j] = v;
}

// grid K, thread d: avg_x2 - 2 mu mu + mu^2 + reg (gmm.py:226-229; avg_X_means is mu times the same quotient that gave mu);
// spherical: the mean over d, summed in order
__global__ void __launch_bounds__(256)
k_fit_cov_diag(const double *__restrict__ avg_x2, const double *__restrict__ means, int D, int Dp, double reg, int spherical,
               double *__restrict__ cov) {
    __shared__ double v[256];
    const int d = threadIdx.x, k = blockIdx.x;
    double s = 0.0;
    if (d < D) {
        const double mu = means[(size_t)k * Dp + d];
        s = ((avg_x2[(size_t)k * Dp + d] - 2.0 * (mu * mu)) + mu * mu) + reg;
    }
    if (!spherical) {
        if (d < Dp) cov[(size_t)k * Dp + d] = s;
        return;
    }
    v[d] = s;
    __syncthreads();
    if (d == 0) {
        double t = 0.0;
        for (int e = 0; e < D; ++e) t += v[e];
        cov[k] = t / (double)D;
    }
}

// ---- precision Cholesky factors into the scoring layout -----------------------------------------------------------------------------
// one workgroup per component.  cov_stride 0: every component factorises the same (tied) matrix.  W, Y: [K][Dp][Dp] workspaces.
__global__ void __launch_bounds__(256)
k_fit_chol(const double *cov, size_t cov_stride, double *W, double *Y, int D, int Dp, const double *means, double *P, double *c,
           double *kc, unsigned char *mask, int *flags) {
    const int t = threadIdx.x, k = blockIdx.x;
    const double *S = cov + (size_t)k * cov_stride;
    double *Wk = W + (size_t)k * Dp * Dp, *Yk = Y + (size_t)k * Dp * Dp, *Pk = P + (size_t)k * Dp * Dp;
    for (int idx = t; idx < D * D; idx += 256) {
        const int i = idx / D, j = idx - i * D;
        Wk[(size_t)i * Dp + j] = S[(size_t)i * Dp + j];
    }
    bool bad = false;
    for (int j = 0; j < D; ++j) {
        __syncthreads();
        const double d = Wk[(size_t)j * Dp + j];
        if (!(d > 0.0) || !(d < INFINITY)) { bad = true; break; }   // (uniform: every thread read the same value)
        const double l = sqrt(d);
        __syncthreads();   // everyone has the pivot before it is replaced
        if (t == 0) Wk[(size_t)j * Dp + j] = l;
        for (int i = j + 1 + t; i < D; i += 256) Wk[(size_t)i * Dp + j] /= l;
        __syncthreads();
        const int m = D - j - 1;
        for (int idx = t; idx < m * m; idx += 256) {
            const int a = idx / m, i = j + 1 + a, e = j + 1 + (idx - a * m);
            if (e <= i) Wk[(size_t)i * Dp + e] -= Wk[(size_t)i * Dp + j] * Wk[(size_t)e * Dp + j];
        }
    }
    if (bad) {   // the factors of the previous iteration stay in place; the driver stops
        if (t == 0) flags[k] = 1;
        return;
    }
    __syncthreads();
    if (t < D) {   // column t of Y = L^-1: rows t .. D-1, each thread reads only what it wrote itself
        const int j = t;
        for (int i = j; i < D; ++i) {
            double s = i == j ? 1.0 : 0.0;
            for (int m = j; m < i; ++m) s -= Wk[(size_t)i * Dp + m] * Yk[(size_t)m * Dp + j];
            Yk[(size_t)i * Dp + j] = s / Wk[(size_t)i * Dp + i];
        }
    }
    __syncthreads();
    for (int idx = t; idx < Dp * Dp; idx += 256) {   // P = Y^T, upper triangular, zero pad
        const int j = idx / Dp, i = idx - j * Dp;
        Pk[idx] = (j < D && i < D && i >= j) ? Yk[(size_t)i * Dp + j] : 0.0;
    }
    if (t < Dp) {
        double s = 0.0;
        if (t < D)
            for (int i = 0; i <= t; ++i) s += means[(size_t)k * Dp + i] * Yk[(size_t)t * Dp + i];
        c[(size_t)k * Dp + t] = s;
    }
    if (t == 0) {
        double ld = 0.0;
        for (int d = 0; d < D; ++d) ld += log(Yk[(size_t)d * Dp + d]);
        kc[k] = ld;
    }
    const int NB = Dp >> 4;
    if (t < NB * NB) mask[(size_t)k * NB * NB + t] = (t / NB) <= (t % NB) ? 1 : 0;
}

// diag / spherical: P_k = diag(1 / sqrt(s)), grid K
__global__ void __launch_bounds__(256)
k_fit_prec_diag(const double *__restrict__ cov, int spherical, int D, int Dp, const double *__restrict__ means, double *__restrict__ P,
                double *__restrict__ c, double *__restrict__ kc, unsigned char *__restrict__ mask, int *__restrict__ flags) {
    __shared__ double p[256];
    __shared__ int bad;
    const int t = threadIdx.x, k = blockIdx.x;
    if (t == 0) bad = 0;
    __syncthreads();
    double v = 1.0;
    if (t < D) {
        v = spherical ? cov[k] : cov[(size_t)k * Dp + t];
        if (!(v > 0.0) || !(v < INFINITY)) bad = 1;   // (same value from every writer)
    }
    __syncthreads();
    if (bad) {
        if (t == 0) flags[k] = 1;
        return;
    }
    p[t] = t < D ? 1.0 / sqrt(v) : 0.0;
    __syncthreads();
    double *Pk = P + (size_t)k * Dp * Dp;
    for (int idx = t; idx < Dp * Dp; idx += 256) {
        const int i = idx / Dp, j = idx - i * Dp;
        Pk[idx] = i == j ? p[i] : 0.0;
    }
    if (t < Dp) c[(size_t)k * Dp + t] = t < D ? means[(size_t)k * Dp + t] * p[t] : 0.0;
    if (t == 0) {   // summed term by term for both types, as gmm_upload sums the diagonal of an expanded factor: the scorer of a fit
        double ld = 0.0;   // and an engine built from its downloaded parameters hold the same bits
        for (int d = 0; d < D; ++d) ld += log(p[d]);
        kc[k] = ld;
    }
    const int NB = Dp >> 4;
    if (t < NB * NB) mask[(size_t)k * NB * NB + t] = (t / NB) == (t % NB) ? 1 : 0;
}

// ---- rows in, k-means -------------------------------------------------------------------------------------------------------------------
// fp32 rows [n][D] -> fp64 [n][Dp] with zero pad; flag[0] = 1 when a value is not finite
__global__ void __launch_bounds__(256)
k_fit_widen(const float *__restrict__ src, int64_t n, int D, int Dp, double *__restrict__ dst, int *__restrict__ flag) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * Dp) return;
    const int64_t row = idx / Dp;
    const int d = (int)(idx - row * Dp);
    const double v = d < D ? (double)src[row * D + d] : 0.0;
    if (!(fabs(v) < INFINITY)) flag[0] = 1;
    dst[idx] = v;
}

__global__ void __launch_bounds__(256)
k_fit_check_f64(const double *__restrict__ x, int64_t n, int *__restrict__ flag) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n && !(fabs(x[idx]) < INFINITY)) flag[0] = 1;
}

// thread per row: squared distance to centres c0 .. c1-1 (summed in column order).  fresh = 1: start from +inf, else from mind2[row].
// labels (may be null) takes the index of the nearest centre (the first on ties); part: per-workgroup sums of the minimum distances.
__global__ void __launch_bounds__(256)
k_fit_dist(const double *__restrict__ X, int n, int D, int Dp, const double *__restrict__ centers, int c0, int c1, int fresh,
           double *__restrict__ mind2, int *__restrict__ labels, double *__restrict__ part) {
    __shared__ double red[256];
    const int row = blockIdx.x * 256 + threadIdx.x;
    double best = 0.0;
    if (row < n) {
        best = fresh ? INFINITY : mind2[row];
        int arg = -1;
        const double *xr = X + (size_t)row * Dp;
        for (int cc = c0; cc < c1; ++cc) {
            const double *cr = centers + (size_t)cc * Dp;
            double s = 0.0;
            for (int d = 0; d < D; ++d) {
                const double e = xr[d] - cr[d];
                s += e * e;
            }
            if (s < best) { best = s; arg = cc; }
        }
        mind2[row] = best;
        if (labels && arg >= 0) labels[row] = arg;
    }
    const double s = block_sum_256(best, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256)
k_fit_copy_row(const double *__restrict__ X, int row, int Dp, double *__restrict__ dst) {
    if ((int)threadIdx.x < Dp) dst[threadIdx.x] = X[(size_t)row * Dp + threadIdx.x];
}

__global__ void __launch_bounds__(256)
k_fit_fill_i32(int *__restrict__ p, int n, int v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static const char *const kIllDefined =
    "Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
    "singleton or collapsed samples). Try to decrease the number of components, or increase reg_covar.";

// Philox4x32-10 (the generator of mc.py): counter (a, b, c, 0), key = seed
static void philox4x32(uint32_t c[4], uint64_t seed) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
static double fit_uniform(uint64_t seed, uint32_t restart, uint32_t draw) {   // [0, 1), 53 bits
    uint32_t c[4] = {draw, restart, 0x676d6dU, 0};
    philox4x32(c, seed);
    return (double)((((uint64_t)c[0] << 32) | c[1]) >> 11) * (1.0 / 9007199254740992.0);
}

int gmm_fit_check_config(const vssr_gmm_fit_config *cfg) {
    const int K = cfg->n_components, D = cfg->dim;
    if (K < 1 || K > 256 || D < 1 || D > 256)
        return set_err(nullptr, VSSR_E_BADARG, "GMM fit: n_components must be in 1..256 and dim in 1..256 (got %d, %d)", K, D);
    if (cfg->covariance_type < 0 || cfg->covariance_type > 3)
        return set_err(nullptr, VSSR_E_BADARG, "GMM fit: unknown covariance_type %d", cfg->covariance_type);
    if (cfg->init < 0 || cfg->init > 2) return set_err(nullptr, VSSR_E_BADARG, "GMM fit: unknown init %d", cfg->init);
    if (!(cfg->tol >= 0.0) || !std::isfinite(cfg->tol)) return set_err(nullptr, VSSR_E_BADARG, "GMM fit: tol must be finite and >= 0");
    if (!(cfg->reg_covar >= 0.0) || !std::isfinite(cfg->reg_covar))
        return set_err(nullptr, VSSR_E_BADARG, "GMM fit: reg_covar must be finite and >= 0");
    if (cfg->max_iter < 1) return set_err(nullptr, VSSR_E_BADARG, "GMM fit: max_iter must be >= 1 (got %d)", cfg->max_iter);
    if (cfg->n_init < 1) return set_err(nullptr, VSSR_E_BADARG, "GMM fit: n_init must be >= 1 (got %d)", cfg->n_init);
    return VSSR_OK;
}

// room for `extra` more rows; resident rows are kept
static int fit_reserve(vssr_handle *h, int64_t extra) {
    GmmFit *f = h->fit.get();
    const int64_t need = f->n + extra;
    if (need > (int64_t)INT32_MAX - 64) return set_err(h, VSSR_E_BADARG, "GMM fit: %lld rows exceed the supported count", (long long)need);
    if (need <= f->cap) return VSSR_OK;
    const int64_t cap = need + need / 2 + 64;
    DevBuf grown;   // sized exactly
    const size_t bytes = sizeof(double) * (size_t)cap * h->gmm_Dp;
    if (hipMalloc(&grown.p, bytes) != hipSuccess)
        return set_err(h, VSSR_E_NOMEM, "device allocation failed (GMM fit rows, %lld)", (long long)cap);
    grown.bytes = bytes;
    if (f->n) {
        VSSR_HIP(h, hipStreamSynchronize(h->stream));
        VSSR_HIP(h, hipMemcpy(grown.p, f->x(), sizeof(double) * (size_t)f->n * h->gmm_Dp, hipMemcpyDeviceToDevice));
    }
    f->rows.swap(grown);   // the old rows go with `grown`
    f->cap = cap;
    return VSSR_OK;
}

int gmm_fit_append_host(vssr_handle *h, int64_t n_rows, const double *x) {
    GmmFit *f = h->fit.get();
    const int D = h->gmm_D, Dp = h->gmm_Dp;
    int rc = fit_reserve(h, n_rows);
    if (rc) return rc;
    double *dst = f->x() + (size_t)f->n * Dp;
    if (Dp == D) {
        VSSR_HIP(h, hipMemcpy(dst, x, sizeof(double) * (size_t)n_rows * D, hipMemcpyHostToDevice));
    } else {
        VSSR_HIP(h, hipMemset(dst, 0, sizeof(double) * (size_t)n_rows * Dp));
        VSSR_HIP(h, hipMemcpy2D(dst, sizeof(double) * Dp, x, sizeof(double) * D, sizeof(double) * D, (size_t)n_rows, hipMemcpyHostToDevice));
    }
    f->n += n_rows;
    f->fitted = false;
    return VSSR_OK;
}

static int fit_flag_after(vssr_handle *h, hipStream_t st, const char *what) {
    int bad = 0;
    VSSR_HIP(h, hipStreamSynchronize(st));
    VSSR_HIP(h, hipMemcpy(&bad, h->fit->flags.p, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return set_err(h, VSSR_E_BADARG, "GMM fit: %s holds a non-finite value", what);
    return VSSR_OK;
}

int gmm_fit_append_f32(vssr_handle *h, hipStream_t st, int64_t n_rows, const float *emb_dev) {
    GmmFit *f = h->fit.get();
    const int D = h->gmm_D, Dp = h->gmm_Dp;
    int rc = fit_reserve(h, n_rows);
    if (rc) return rc;
    if (f->flags.ensure(sizeof(int) * 257)) return set_err(h, VSSR_E_NOMEM, "device allocation failed (GMM fit flags)");
    VSSR_HIP(h, hipMemsetAsync(f->flags.p, 0, sizeof(int), st));
    const int64_t tot = n_rows * Dp;
    hipLaunchKernelGGL(k_fit_widen, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, emb_dev, n_rows, D, Dp,
                       f->x() + (size_t)f->n * Dp, f->flags.as<int>());
    VSSR_HIP(h, hipGetLastError());
    rc = fit_flag_after(h, st, "the embedding");
    if (rc) return rc;
    f->n += n_rows;
    f->fitted = false;
    return VSSR_OK;
}

int gmm_fit_append_f64p(vssr_handle *h, hipStream_t st, int64_t n_rows, const double *x_dev) {
    GmmFit *f = h->fit.get();
    const int Dp = h->gmm_Dp;
    int rc = fit_reserve(h, n_rows);
    if (rc) return rc;
    if (f->flags.ensure(sizeof(int) * 257)) return set_err(h, VSSR_E_NOMEM, "device allocation failed (GMM fit flags)");
    VSSR_HIP(h, hipMemsetAsync(f->flags.p, 0, sizeof(int), st));
    const int64_t tot = n_rows * Dp;
    hipLaunchKernelGGL(k_fit_check_f64, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x_dev, tot, f->flags.as<int>());
    VSSR_HIP(h, hipGetLastError());
    VSSR_HIP(h, hipMemcpyAsync(f->x() + (size_t)f->n * Dp, x_dev, sizeof(double) * (size_t)tot, hipMemcpyDeviceToDevice, st));
    rc = fit_flag_after(h, st, "the embedding");
    if (rc) return rc;
    f->n += n_rows;
    f->fitted = false;
    return VSSR_OK;
}

// lower Cholesky factor of a symmetric [D][D] matrix (row-major), in place in the lower triangle, upper zeroed; false: not positive
static bool host_cholesky_lower(double *a, int D) {
    for (int j = 0; j < D; ++j) {
        double d = a[(size_t)j * D + j];
        for (int m = 0; m < j; ++m) d -= a[(size_t)j * D + m] * a[(size_t)j * D + m];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double l = std::sqrt(d);
        a[(size_t)j * D + j] = l;
        for (int i = j + 1; i < D; ++i) {
            double s = a[(size_t)i * D + j];
            for (int m = 0; m < j; ++m) s -= a[(size_t)i * D + m] * a[(size_t)j * D + m];
            a[(size_t)i * D + j] = s / l;
        }
        for (int i = 0; i < j; ++i) a[(size_t)i * D + j] = 0.0;
    }
    return true;
}

int gmm_fit_set_init(vssr_handle *h, const double *means, const double *weights, const double *precisions, const int32_t *labels) {
    GmmFit *f = h->fit.get();
    const int K = h->gmm_K, D = h->gmm_D;
    std::vector<double> m, w, p;
    std::vector<int> lab;
    if (means) {
        m.assign(means, means + (size_t)K * D);
        for (double v : m)
            if (!std::isfinite(v)) return set_err(h, VSSR_E_BADARG, "GMM fit: non-finite initial mean");
    }
    if (weights) {
        w.assign(weights, weights + K);
        bool any = false;
        for (int k = 0; k < K; ++k) {
            if (!std::isfinite(w[k]) || w[k] < 0) return set_err(h, VSSR_E_BADARG, "GMM fit: initial weight %d is negative or not finite", k);
            any = any || w[k] > 0;
        }
        if (!any) return set_err(h, VSSR_E_BADARG, "GMM fit: no positive initial weight");
    }
    if (precisions) {   // -> full precision Cholesky factors [K][D][D] (gmm.py:657-664: lower Cholesky of the precision matrices)
        p.assign((size_t)K * D * D, 0.0);
        const int ct = f->cov_type;
        const size_t n_in = ct == VSSR_GMM_COV_FULL ? (size_t)K * D * D : ct == VSSR_GMM_COV_TIED ? (size_t)D * D : ct == VSSR_GMM_COV_DIAG ? (size_t)K * D : (size_t)K;
        for (size_t i = 0; i < n_in; ++i)
            if (!std::isfinite(precisions[i])) return set_err(h, VSSR_E_BADARG, "GMM fit: non-finite initial precision");
        for (int k = 0; k < K; ++k) {
            double *pk = p.data() + (size_t)k * D * D;
            if (ct == VSSR_GMM_COV_FULL || ct == VSSR_GMM_COV_TIED) {
                if (ct == VSSR_GMM_COV_TIED && k > 0) {
                    memcpy(pk, p.data(), sizeof(double) * D * D);
                    continue;
                }
                memcpy(pk, precisions + (ct == VSSR_GMM_COV_FULL ? (size_t)k * D * D : 0), sizeof(double) * D * D);
                if (!host_cholesky_lower(pk, D))
                    return set_err(h, VSSR_E_BADARG, "GMM fit: the initial precision of component %d is not positive definite", k);
            } else {
                for (int d = 0; d < D; ++d) {
                    const double v = ct == VSSR_GMM_COV_DIAG ? precisions[(size_t)k * D + d] : precisions[k];
                    if (!(v > 0.0)) return set_err(h, VSSR_E_BADARG, "GMM fit: initial precision of component %d is not positive", k);
                    pk[(size_t)d * D + d] = std::sqrt(v);
                }
            }
        }
    }
    if (labels) {
        lab.assign(labels, labels + f->n);
        for (int v : lab)
            if (v < -1 || v >= K) return set_err(h, VSSR_E_BADARG, "GMM fit: label %d outside -1 .. %d", v, K - 1);
    }
    f->i_means.swap(m); f->i_weights.swap(w); f->i_prec.swap(p); f->i_labels.swap(lab);
    f->has_means = means != nullptr; f->has_weights = weights != nullptr; f->has_prec = precisions != nullptr;
    f->has_labels = labels != nullptr;
    return VSSR_OK;
}

// launch geometry of the slab kernels
struct FitGeom {
    int S_m, rps_m;        // moments: slabs, rows per slab
    int S_c, rps_c, ZT;    // covariance: slabs, rows per slab (multiple of 4), task groups
    int n_blk;             // 256-row workgroups
};
static FitGeom fit_geom(int n, int K, int Dp, int cov_components) {
    FitGeom g;
    g.n_blk = (n + 255) / 256;
    g.S_m = std::max(1, std::min(g.n_blk, 4096 / K));
    g.rps_m = (n + g.S_m - 1) / g.S_m;
    g.S_m = (n + g.rps_m - 1) / g.rps_m;
    g.ZT = (fit_cov_tasks(Dp / 16) + 3) / 4;
    const size_t tile = sizeof(double) * (size_t)cov_components * Dp * Dp;
    const int by_mem = (int)std::max<size_t>(1, ((size_t)128 << 20) / tile);
    int S = std::max(1, std::min(std::min(g.n_blk, 4096 / (cov_components * g.ZT) + 1), by_mem));
    g.rps_c = 4 * (((n + S - 1) / S + 3) / 4);
    g.S_c = (n + g.rps_c - 1) / g.rps_c;
    return g;
}

// M step from responsibilities (resp) or one-hot labels; init = true: w_k = n_k / N (gmm.py:644-647)
static int fit_m_step(vssr_handle *h, hipStream_t st, const double *resp, const int *labels, bool init) {
    GmmFit *f = h->fit.get();
    const int K = h->gmm_K, D = h->gmm_D, Dp = h->gmm_Dp, n = (int)f->n, ct = f->cov_type;
    const bool vec = ct == VSSR_GMM_COV_DIAG || ct == VSSR_GMM_COV_SPHERICAL;
    const int Kc = ct == VSSR_GMM_COV_TIED ? 1 : K;
    const FitGeom g = fit_geom(n, K, Dp, Kc);
    hipLaunchKernelGGL(k_fit_moments, dim3(g.S_m, K), dim3(256), 0, st, f->x(), n, Dp, resp, labels, K, g.rps_m, vec ? 1 : 0,
                       f->part_s.as<double>(), f->part_q.as<double>(), f->part_n.as<double>());
    hipLaunchKernelGGL(k_fit_means, dim3(K), dim3(256), 0, st, f->part_s.as<double>(), f->part_q.as<double>(), f->part_n.as<double>(),
                       g.S_m, K, Dp, vec ? 1 : 0, f->nk.as<double>(), f->means.as<double>(), f->avg_x2.as<double>());
    hipLaunchKernelGGL(k_fit_weights, dim3(1), dim3(64), 0, st, f->nk.as<double>(), K, init ? (double)n : 0.0, f->w.as<double>(),
                       h->d_gmm_kc.as<double>());
    if (vec) {
        hipLaunchKernelGGL(k_fit_cov_diag, dim3(K), dim3(256), 0, st, f->avg_x2.as<double>(), f->means.as<double>(), D, Dp, f->reg_covar,
                           ct == VSSR_GMM_COV_SPHERICAL ? 1 : 0, f->cov.as<double>());
        hipLaunchKernelGGL(k_fit_prec_diag, dim3(K), dim3(256), 0, st, f->cov.as<double>(), ct == VSSR_GMM_COV_SPHERICAL ? 1 : 0, D, Dp,
                           f->means.as<double>(), h->d_gmm_P.as<double>(), h->d_gmm_c.as<double>(), h->d_gmm_kc.as<double>(),
                           h->d_gmm_mask.as<unsigned char>(), f->flags.as<int>() + 1);
    } else {
        const bool tied = ct == VSSR_GMM_COV_TIED;
        // tied: X^T X does not change between iterations, but it is cheap next to the E step of K components and keeps one path
        hipLaunchKernelGGL(k_fit_cov, dim3(g.S_c, Kc, g.ZT), dim3(256), 0, st, f->x(), n, Dp, tied ? nullptr : resp, K,
                           tied ? nullptr : f->means.as<double>(), g.rps_c, f->part_cov.as<double>());
        hipLaunchKernelGGL(k_fit_cov_finish, dim3(Kc, Dp), dim3(256), 0, st, f->part_cov.as<double>(), g.S_c, D, Dp, K, tied ? 1 : 0,
                           f->nk.as<double>(), f->means.as<double>(), f->reg_covar, f->cov.as<double>());
        hipLaunchKernelGGL(k_fit_chol, dim3(K), dim3(256), 0, st, f->cov.as<double>(), tied ? (size_t)0 : (size_t)Dp * Dp,
                           f->chol_w.as<double>(), f->chol_y.as<double>(), D, Dp, f->means.as<double>(), h->d_gmm_P.as<double>(),
                           h->d_gmm_c.as<double>(), h->d_gmm_kc.as<double>(), h->d_gmm_mask.as<unsigned char>(), f->flags.as<int>() + 1);
    }
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

// Centred scatter of rows that are not a mixture's (cluster.hip: the covariance of a PCA): cov [Dp][Dp] = sum_n (x_n - mean)(x_n - mean)^T
// / denom[0], through the row-slab kernel with unit responsibilities and the same slab-ordered finish (no reg, pad rows / columns zero).
// mean [Dp] and denom [1] live on the device; part is the caller's workspace.
int gmm_fit_centered_cov(vssr_handle *h, hipStream_t st, const double *X, int n, int D, int Dp, const double *mean, const double *denom,
                         DevBuf &part, double *cov) {
    const FitGeom g = fit_geom(n, 1, Dp, 1);
    if (part.ensure(sizeof(double) * (size_t)g.S_c * Dp * Dp)) return set_err(h, VSSR_E_NOMEM, "device allocation failed (covariance partials)");
    hipLaunchKernelGGL(k_fit_cov, dim3(g.S_c, 1, g.ZT), dim3(256), 0, st, X, n, Dp, (const double *)nullptr, 1, mean, g.rps_c, part.as<double>());
    hipLaunchKernelGGL(k_fit_cov_finish, dim3(1, Dp), dim3(256), 0, st, part.as<double>(), g.S_c, D, Dp, 1, 0, denom, mean, 0.0, cov);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

// one-hot responsibilities of labels are only needed by the full covariance kernel: written as a dense [n][K] array
__global__ void __launch_bounds__(256)
k_fit_onehot(const int *__restrict__ labels, int n, int K, double *__restrict__ resp) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * K) return;
    const int row = (int)(idx / K), k = (int)(idx - (int64_t)row * K);
    resp[idx] = labels[row] == k ? 1.0 : 0.0;
}

static int fit_read_status(vssr_handle *h, hipStream_t st, const double *value, double *out) {
    GmmFit *f = h->fit.get();
    hipLaunchKernelGGL(k_fit_status, dim3(1), dim3(64), 0, st, f->flags.as<int>() + 1, h->gmm_K, value, f->status.as<double>() + 1);
    VSSR_HIP(h, hipGetLastError());
    VSSR_HIP(h, hipMemcpyAsync(out, f->status.as<double>() + 1, sizeof(double), hipMemcpyDeviceToHost, st));
    VSSR_HIP(h, hipStreamSynchronize(st));
    return VSSR_OK;
}

// K distinct rows in 0 .. n-1 (rejection of repeats); draws numbered from *draw
static void fit_draw_rows(const GmmFit *f, int restart, uint32_t *draw, int n, int K, std::vector<int> &rows) {
    rows.clear();
    while ((int)rows.size() < K) {
        const int r = std::min(n - 1, (int)(fit_uniform(f->seed, (uint32_t)restart, (*draw)++) * n));
        bool dup = false;
        for (int v : rows) dup = dup || v == r;
        if (!dup) rows.push_back(r);
    }
}

// k-means on the device: k-means++ seeding (D^2 sampling, one candidate per centre), then Lloyd iterations until the inertia stops
// changing (bitwise: every reduction has a fixed order) or 300 iterations; labels end up in f->labels
static int fit_kmeans(vssr_handle *h, hipStream_t st, int restart) {
    GmmFit *f = h->fit.get();
    const int K = h->gmm_K, D = h->gmm_D, Dp = h->gmm_Dp, n = (int)f->n;
    const FitGeom g = fit_geom(n, K, Dp, 1);
    double *cen = f->centers.as<double>(), *mind2 = f->centers.as<double>() + (size_t)K * Dp, *part = f->assign_part.as<double>();
    int *lab = f->labels.as<int>();
    uint32_t draw = 0;
    std::vector<double> hp(g.n_blk), hm(256);
    int first = std::min(n - 1, (int)(fit_uniform(f->seed, (uint32_t)restart, draw++) * n));
    hipLaunchKernelGGL(k_fit_copy_row, dim3(1), dim3(256), 0, st, f->x(), first, Dp, cen);
    for (int c = 1; c < K; ++c) {
        hipLaunchKernelGGL(k_fit_dist, dim3(g.n_blk), dim3(256), 0, st, f->x(), n, D, Dp, cen, c - 1, c, c == 1 ? 1 : 0, mind2, (int *)nullptr, part);
        VSSR_HIP(h, hipGetLastError());
        VSSR_HIP(h, hipMemcpyAsync(hp.data(), part, sizeof(double) * g.n_blk, hipMemcpyDeviceToHost, st));
        VSSR_HIP(h, hipStreamSynchronize(st));
        double tot = 0.0;
        for (double v : hp) tot += v;
        const double target = fit_uniform(f->seed, (uint32_t)restart, draw++) * tot;
        int blk = 0;
        double run = 0.0;
        while (blk < g.n_blk - 1 && run + hp[blk] <= target) run += hp[blk++];
        const int r0 = blk * 256, cnt = std::min(256, n - r0);
        VSSR_HIP(h, hipMemcpy(hm.data(), mind2 + r0, sizeof(double) * cnt, hipMemcpyDeviceToHost));
        int pick = 0;
        while (pick < cnt - 1 && run + hm[pick] <= target) run += hm[pick++];
        while (pick < cnt - 1 && !(hm[pick] > 0.0)) ++pick;   // (never a row that already is a centre, when another is left)
        hipLaunchKernelGGL(k_fit_copy_row, dim3(1), dim3(256), 0, st, f->x(), r0 + pick, Dp, cen + (size_t)c * Dp);
    }
    double prev = -1.0;
    for (int it = 0; it < 300; ++it) {
        hipLaunchKernelGGL(k_fit_dist, dim3(g.n_blk), dim3(256), 0, st, f->x(), n, D, Dp, cen, 0, K, 1, mind2, lab, part);
        hipLaunchKernelGGL(k_fit_sum, dim3(1), dim3(256), 0, st, part, g.n_blk, 1.0, f->status.as<double>());
        VSSR_HIP(h, hipGetLastError());
        double inertia = 0.0;
        VSSR_HIP(h, hipMemcpyAsync(&inertia, f->status.p, sizeof(double), hipMemcpyDeviceToHost, st));
        VSSR_HIP(h, hipStreamSynchronize(st));
        if (inertia == prev) break;
        prev = inertia;
        hipLaunchKernelGGL(k_fit_moments, dim3(g.S_m, K), dim3(256), 0, st, f->x(), n, Dp, (const double *)nullptr, lab, K, g.rps_m, 0,
                           f->part_s.as<double>(), f->part_q.as<double>(), f->part_n.as<double>());
        hipLaunchKernelGGL(k_fit_means, dim3(K), dim3(256), 0, st, f->part_s.as<double>(), f->part_q.as<double>(), f->part_n.as<double>(),
                           g.S_m, K, Dp, 0, f->nk.as<double>(), cen, f->avg_x2.as<double>());
        VSSR_HIP(h, hipGetLastError());
    }
    return VSSR_OK;
}

static int fit_alloc(vssr_handle *h) {
    GmmFit *f = h->fit.get();
    const int K = h->gmm_K, Dp = h->gmm_Dp, n = (int)f->n, NB = Dp / 16;
    const int Kc = f->cov_type == VSSR_GMM_COV_TIED ? 1 : K;
    const bool mat = f->cov_type == VSSR_GMM_COV_FULL || f->cov_type == VSSR_GMM_COV_TIED;
    const FitGeom g = fit_geom(n, K, Dp, Kc);
    const size_t d = sizeof(double), KD = (size_t)K * Dp, KDD = KD * Dp;
    bool bad = f->resp.ensure(d * (size_t)n * K) || f->labels.ensure(sizeof(int) * (size_t)n) || f->lbpart.ensure(d * g.n_blk) ||
               f->status.ensure(d * 4) || f->flags.ensure(sizeof(int) * 257) || f->part_s.ensure(d * g.S_m * KD) ||
               f->part_q.ensure(d * g.S_m * KD) || f->part_n.ensure(d * (size_t)g.S_m * K) || f->nk.ensure(d * K) ||
               f->means.ensure(d * KD) || f->avg_x2.ensure(d * KD) || f->w.ensure(d * K) ||
               f->cov.ensure(mat ? d * (size_t)Kc * Dp * Dp : d * KD) ||
               (mat && (f->part_cov.ensure(d * (size_t)g.S_c * Kc * Dp * Dp) || f->chol_w.ensure(d * KDD) || f->chol_y.ensure(d * KDD))) ||
               f->centers.ensure(d * (KD + (size_t)n)) || f->assign_part.ensure(d * g.n_blk) ||
               h->d_gmm_P.ensure(d * KDD) || h->d_gmm_c.ensure(d * KD) || h->d_gmm_kc.ensure(d * 2 * K) ||
               h->d_gmm_mask.ensure((size_t)K * NB * NB);
    if (!bad && f->n_init > 1)
        bad = f->b_w.ensure(d * K) || f->b_means.ensure(d * KD) || f->b_cov.ensure(mat ? d * (size_t)Kc * Dp * Dp : d * KD) ||
              f->b_P.ensure(d * KDD) || f->b_c.ensure(d * KD) || f->b_kc.ensure(d * 2 * K) || f->b_mask.ensure((size_t)K * NB * NB);
    if (bad) return set_err(h, VSSR_E_NOMEM, "device allocation failed (GMM fit workspaces: %d rows, K = %d, D = %d)", n, K, h->gmm_D);
    return VSSR_OK;
}

static int fit_copy_best(vssr_handle *h, hipStream_t st, bool save) {
    GmmFit *f = h->fit.get();
    const int K = h->gmm_K, Dp = h->gmm_Dp, NB = Dp / 16;
    const int Kc = f->cov_type == VSSR_GMM_COV_TIED ? 1 : K;
    const bool mat = f->cov_type == VSSR_GMM_COV_FULL || f->cov_type == VSSR_GMM_COV_TIED;
    const size_t d = sizeof(double), KD = (size_t)K * Dp;
    struct { DevBuf *cur, *best; size_t bytes; } items[] = {
        {&f->w, &f->b_w, d * K}, {&f->means, &f->b_means, d * KD}, {&f->cov, &f->b_cov, mat ? d * (size_t)Kc * Dp * Dp : d * KD},
        {&h->d_gmm_P, &f->b_P, d * KD * Dp}, {&h->d_gmm_c, &f->b_c, d * KD}, {&h->d_gmm_kc, &f->b_kc, d * 2 * K},
        {&h->d_gmm_mask, &f->b_mask, (size_t)K * NB * NB}};
    for (auto &it : items)
        VSSR_HIP(h, hipMemcpyAsync(save ? it.best->p : it.cur->p, save ? it.cur->p : it.best->p, it.bytes, hipMemcpyDeviceToDevice, st));
    return VSSR_OK;
}

// starting mixture of restart `restart` in the scoring buffers
static int fit_initialise(vssr_handle *h, hipStream_t st, int restart) {
    GmmFit *f = h->fit.get();
    const int K = h->gmm_K, D = h->gmm_D, Dp = h->gmm_Dp, n = (int)f->n;
    const bool all_given = f->has_means && f->has_weights && f->has_prec;
    VSSR_HIP(h, hipMemsetAsync(f->flags.p, 0, sizeof(int) * 257, st));
    VSSR_HIP(h, hipMemsetAsync(f->status.p, 0, sizeof(double) * 4, st));
    if (!all_given) {
        int *lab = f->labels.as<int>();
        if (f->has_labels) {
            VSSR_HIP(h, hipMemcpyAsync(lab, f->i_labels.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
        } else if (f->init == VSSR_GMM_INIT_KMEANS) {
            int rc = fit_kmeans(h, st, restart);
            if (rc) return rc;
        } else {   // random_from_data: K distinct rows, one component each
            std::vector<int> rows;
            uint32_t draw = 0;
            fit_draw_rows(f, restart, &draw, n, K, rows);
            std::vector<int> hl((size_t)n, -1);
            for (int k = 0; k < K; ++k) hl[rows[k]] = k;
            VSSR_HIP(h, hipMemcpy(lab, hl.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
        }
        hipLaunchKernelGGL(k_fit_onehot, dim3((unsigned)(((int64_t)n * K + 255) / 256)), dim3(256), 0, st, lab, n, K, f->resp.as<double>());
        VSSR_HIP(h, hipGetLastError());
        int rc = fit_m_step(h, st, f->resp.as<double>(), nullptr, true);
        if (rc) return rc;
        double s = 0.0;
        rc = fit_read_status(h, st, f->status.as<double>(), &s);
        if (rc) return rc;
        if (std::isnan(s) && !f->has_prec) return set_err(h, VSSR_E_STATE, "%s", kIllDefined);
    }
    if (f->has_means || f->has_weights || f->has_prec) {   // explicit values win (gmm.py:649-664); the rest comes from the device
        std::vector<double> M((size_t)K * D), W(K), P((size_t)K * D * D);
        if (!all_given) {
            VSSR_HIP(h, hipMemcpy(W.data(), f->w.p, sizeof(double) * K, hipMemcpyDeviceToHost));
            VSSR_HIP(h, hipMemcpy2D(M.data(), sizeof(double) * D, f->means.p, sizeof(double) * Dp, sizeof(double) * D, K, hipMemcpyDeviceToHost));
            if (!f->has_prec)
                for (int k = 0; k < K; ++k)
                    VSSR_HIP(h, hipMemcpy2D(P.data() + (size_t)k * D * D, sizeof(double) * D, h->d_gmm_P.as<double>() + (size_t)k * Dp * Dp,
                                            sizeof(double) * Dp, sizeof(double) * D, D, hipMemcpyDeviceToHost));
        }
        if (f->has_means) M = f->i_means;
        if (f->has_weights) W = f->i_weights;
        if (f->has_prec) P = f->i_prec;
        int rc = gmm_upload(h, M.data(), P.data(), W.data());
        if (rc) return set_err(h, rc, "GMM fit: upload of the initial parameters failed");
        VSSR_HIP(h, hipMemsetAsync(f->flags.p, 0, sizeof(int) * 257, st));
    }
    return VSSR_OK;
}

int gmm_fit_run(vssr_handle *h, vssr_gmm_fit_result *res) {
    GmmFit *f = h->fit.get();
    const int K = h->gmm_K, n = (int)f->n;
    hipStream_t st = h->stream;
    f->fitted = false;
    int rc = fit_alloc(h);
    if (rc) return rc;
    const int n_blk = (n + 255) / 256;
    double max_lb = -INFINITY;
    std::vector<double> best_trace, trace;
    int best_iter = 0, best_init = 0, best_conv = 0;
    for (int restart = 0; restart < f->n_init; ++restart) {
        rc = fit_initialise(h, st, restart);
        if (rc) return rc;
        double lb = -INFINITY;
        int conv = 0, it = 0;
        trace.clear();
        for (it = 1; it <= f->max_iter; ++it) {
            const double prev = lb;
            rc = gmm_score_f64(h, st, n, f->x());
            if (rc) return rc;
            hipLaunchKernelGGL(k_fit_resp, dim3(n_blk), dim3(256), 0, st, h->d_gmm_lp.as<double>(), h->d_gmm_kc.as<double>(),
                               h->d_gmm_nll.as<double>(), n, K, f->resp.as<double>(), f->lbpart.as<double>());
            hipLaunchKernelGGL(k_fit_sum, dim3(1), dim3(256), 0, st, f->lbpart.as<double>(), n_blk, 1.0 / (double)n, f->status.as<double>());
            VSSR_HIP(h, hipGetLastError());
            rc = fit_m_step(h, st, f->resp.as<double>(), nullptr, false);
            if (rc) return rc;
            rc = fit_read_status(h, st, f->status.as<double>(), &lb);   // the one read-back of the iteration
            if (rc) return rc;
            if (std::isnan(lb)) return set_err(h, VSSR_E_STATE, "%s", kIllDefined);
            trace.push_back(lb);
            if (std::fabs(lb - prev) < f->tol) { conv = 1; break; }
        }
        if (it > f->max_iter) it = f->max_iter;
        if (lb > max_lb || max_lb == -INFINITY) {
            max_lb = lb;
            best_trace = trace;
            best_iter = it; best_init = restart; best_conv = conv;
            if (f->n_init > 1) {
                rc = fit_copy_best(h, st, true);
                if (rc) return rc;
            }
        }
    }
    if (f->n_init > 1) {
        rc = fit_copy_best(h, st, false);
        if (rc) return rc;
    }
    VSSR_HIP(h, hipStreamSynchronize(st));
    f->fitted = true;
    if (res) {
        res->n_iter = best_iter; res->converged = best_conv; res->best_init = best_init; res->lower_bound = max_lb;
        const int m = res->lower_bounds ? std::min((int)best_trace.size(), std::max(res->lower_bounds_cap, 0)) : 0;
        for (int i = 0; i < m; ++i) res->lower_bounds[i] = best_trace[i];
        res->n_lower_bounds = m;
    }
    return VSSR_OK;
}

int gmm_fit_params(vssr_handle *h, double *weights, double *means, double *covariances, double *prec_chol) {
    GmmFit *f = h->fit.get();
    const int K = h->gmm_K, D = h->gmm_D, Dp = h->gmm_Dp, ct = f->cov_type;
    const size_t d = sizeof(double);
    if (weights) VSSR_HIP(h, hipMemcpy(weights, f->w.p, d * K, hipMemcpyDeviceToHost));
    if (means) VSSR_HIP(h, hipMemcpy2D(means, d * D, f->means.p, d * Dp, d * D, K, hipMemcpyDeviceToHost));
    const double *P = h->d_gmm_P.as<double>();
    if (ct == VSSR_GMM_COV_FULL || ct == VSSR_GMM_COV_TIED) {
        const int Kc = ct == VSSR_GMM_COV_TIED ? 1 : K;
        for (int k = 0; k < Kc; ++k) {
            if (covariances)
                VSSR_HIP(h, hipMemcpy2D(covariances + (size_t)k * D * D, d * D, f->cov.as<double>() + (size_t)k * Dp * Dp, d * Dp, d * D, D, hipMemcpyDeviceToHost));
            if (prec_chol)
                VSSR_HIP(h, hipMemcpy2D(prec_chol + (size_t)k * D * D, d * D, P + (size_t)k * Dp * Dp, d * Dp, d * D, D, hipMemcpyDeviceToHost));
        }
    } else if (ct == VSSR_GMM_COV_DIAG) {
        if (covariances) VSSR_HIP(h, hipMemcpy2D(covariances, d * D, f->cov.p, d * Dp, d * D, K, hipMemcpyDeviceToHost));
        if (prec_chol)   // the diagonals of the K factors: stride Dp + 1
            for (int k = 0; k < K; ++k)
                VSSR_HIP(h, hipMemcpy2D(prec_chol + (size_t)k * D, d, P + (size_t)k * Dp * Dp, d * (Dp + 1), d, D, hipMemcpyDeviceToHost));
    } else {
        if (covariances) VSSR_HIP(h, hipMemcpy(covariances, f->cov.p, d * K, hipMemcpyDeviceToHost));
        if (prec_chol) VSSR_HIP(h, hipMemcpy2D(prec_chol, d, P, d * (size_t)Dp * Dp, d, K, hipMemcpyDeviceToHost));
    }
    return VSSR_OK;
}

int gmm_fit_copy_scorer(vssr_handle *h, vssr_handle *g) {
    const int K = h->gmm_K, Dp = h->gmm_Dp, NB = Dp / 16;
    const size_t d = sizeof(double), KD = (size_t)K * Dp;
    if (g->d_gmm_P.ensure(d * KD * Dp) || g->d_gmm_c.ensure(d * KD) || g->d_gmm_kc.ensure(d * 2 * K) || g->d_gmm_mask.ensure((size_t)K * NB * NB))
        return set_err(nullptr, VSSR_E_NOMEM, "device allocation failed (GMM parameters)");
    VSSR_HIP(h, hipMemcpy(g->d_gmm_P.p, h->d_gmm_P.p, d * KD * Dp, hipMemcpyDeviceToDevice));
    VSSR_HIP(h, hipMemcpy(g->d_gmm_c.p, h->d_gmm_c.p, d * KD, hipMemcpyDeviceToDevice));
    VSSR_HIP(h, hipMemcpy(g->d_gmm_kc.p, h->d_gmm_kc.p, d * 2 * K, hipMemcpyDeviceToDevice));
    VSSR_HIP(h, hipMemcpy(g->d_gmm_mask.p, h->d_gmm_mask.p, (size_t)K * NB * NB, hipMemcpyDeviceToDevice));
    return VSSR_OK;
}

}  // namespace vssr
