// gmm.hip — Gaussian-mixture negative log-likelihood of embedding rows, fp64 on the matrix pipe (v_mfma_f64_16x16x4_f64).
//
// For a row x, component k (mean mu_k, precision Cholesky factor P_k, weight w_k), the reference's GMMUncertainty
// (mcmc/uncertainty/uncertainty.py:238-463) computes
//   s_k = sum_j ((x P_k)_j - c_kj)^2,  c_k = mu_k P_k          logp_k = -0.5 (D log_2pi + s_k) + log det P_k
//   NLL = -(m + log sum_k exp(logp_k + log w_k - m)),  m = max_k (logp_k + log w_k)
// k_gmm_logp: a workgroup of 4 waves owns 64 rows, each wave 16 rows whose A fragments (x, fp64) stay in registers for the whole
// kernel (Dp / 4 doubles per lane).  Each P_k is streamed through LDS in 16-column blocks; for every 16 x 16 block of P_k that is not
// exactly zero (mask built by the host at create) four MFMAs accumulate x P_k for 16 columns.  The epilogue of a column block
// subtracts c_k and adds the squares to per-lane row sums; the 16 lanes of a row group reduce them with a fixed butterfly, so every
// result is deterministic.  logp_k goes to lp [n][K]; the logsumexp of each row follows once all K components are done.
// C/D layout of the f64 MFMA (it differs from every other MFMA): col = lane & 15, row = (lane >> 4) + 4 reg.
// A / B: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15] of the 4-deep k-step.
#include <cmath>

#include "vssr_internal.h"

namespace vssr {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int GMM_ROWS = 64;   // rows per workgroup (4 waves x 16)

template <typename T, int NB>
__global__ void __launch_bounds__(256)
k_gmm_logp(const T *__restrict__ X, int n, int K, int D, double log2pi, const double *__restrict__ P,
           const double *__restrict__ c, const double *__restrict__ kc, const unsigned char *__restrict__ mask,
           double *__restrict__ lp, double *__restrict__ nll) {
    constexpr int Dp = 16 * NB, NQ = 4 * NB;
    __shared__ double Ps[Dp][16];
    __shared__ double fence[256];   // written, never read: see the fence store below
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * GMM_ROWS;
    // A fragments: row r0 + 16 wave + (lane & 15) (tail rows repeat the last row; their results are not stored), columns 4 q + (lane >> 4)
    const int arow = min(r0 + 16 * wave + (lane & 15), n - 1);
    const T *xr = X + (size_t)arow * Dp + (lane >> 4);
    double a[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] = (double)xr[4 * q];
    const int g = lane >> 4, col = lane & 15;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const double *Pk = P + (size_t)k * Dp * Dp;
        const unsigned char *mk = mask + (size_t)k * NB * NB;
        double part[4] = {0.0, 0.0, 0.0, 0.0};   // sum of squares of row g + 4 r over this lane's columns
#pragma unroll 1
        for (int jb = 0; jb < NB; ++jb) {
            __syncthreads();   // every wave has read the previous block out of Ps
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int idx = tid + 256 * i, r = idx >> 4, cc = idx & 15;
                Ps[r][cc] = Pk[(size_t)r * Dp + 16 * jb + cc];
            }
            __syncthreads();
            // four accumulator chains (one per k-step of a block): consecutive MFMAs are independent, each accumulator's producer
            // is four matrix instructions back (MFMA hazard rules)
            f64x4 acc[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) {
                if (!mk[ib * NB + jb]) continue;   // an all-zero block adds exactly 0 (uniform branch)
                double b[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) b[s] = Ps[16 * ib + 4 * s + g][col];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[4 * ib + s], b[s], acc[s], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // fence: the last MFMA's result goes to an LDS cell nobody reads.  The matrix pipe completes in order, so nothing
                // behind this store (the next block's operand loads) issues before all four MFMAs have read their sources.
                *(volatile __attribute__((address_space(3))) double *)(fence + tid) = acc[3][0];
                __builtin_amdgcn_sched_barrier(0);
            }
            const double ck = c[(size_t)k * Dp + 16 * jb + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double y = ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) - ck;
                part[r] = fma(y, y, part[r]);
            }
        }
        // the 16 lanes of a row group hold the partial sums of their columns: fixed butterfly over lane bits 0..3
#pragma unroll
        for (int m = 1; m < 16; m <<= 1)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[r] += __shfl_xor(part[r], m, 64);
        if (col < 4) {
            const int row = r0 + 16 * wave + g + 4 * col;
            const double s = col == 0 ? part[0] : col == 1 ? part[1] : col == 2 ? part[2] : part[3];
            if (row < n) lp[(size_t)row * K + k] = -0.5 * (D * log2pi + s) + kc[k];
        }
    }
    __syncthreads();   // (global writes of the workgroup are visible to the workgroup behind the barrier)
    if (tid < GMM_ROWS && r0 + tid < n) {
        const double *lr = lp + (size_t)(r0 + tid) * K;
        const double *lw = kc + K;
        double m = -INFINITY;
        for (int k = 0; k < K; ++k) m = fmax(m, lr[k] + lw[k]);
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum += exp(lr[k] + lw[k] - m);
        nll[r0 + tid] = -(m + log(sum));
    }
}

// one workgroup per structure, one thread per column: mean of the structure's rows, summed in atom order in fp64
__global__ void __launch_bounds__(256)
k_gmm_mean_rows(const float *__restrict__ emb, int D, int Dp, const int *__restrict__ start, double *__restrict__ out) {
    const int b = blockIdx.x, d = threadIdx.x;
    if (d >= Dp) return;
    const int a0 = start[b], a1 = start[b + 1];
    double s = 0.0;
    if (d < D)
        for (int i = a0; i < a1; ++i) s += (double)emb[(size_t)i * D + d];
    out[(size_t)b * Dp + d] = d < D && a1 > a0 ? s / (double)(a1 - a0) : 0.0;
}

// one workgroup per structure: sum / sum of squares / max / min of its row NLLs, strided per thread then a fixed LDS tree
__global__ void __launch_bounds__(256)
k_gmm_reduce(const double *__restrict__ nll, const int *__restrict__ start, int order, double *__restrict__ sys) {
    __shared__ double red[4][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int a0 = start[b], a1 = start[b + 1];
    double s = 0.0, s2 = 0.0, mx = -INFINITY, mn = INFINITY;
    for (int i = a0 + t; i < a1; i += 256) {
        const double v = nll[i];
        s += v;
        s2 = fma(v, v, s2);
        mx = fmax(mx, v);
        mn = fmin(mn, v);
    }
    red[0][t] = s; red[1][t] = s2; red[2][t] = mx; red[3][t] = mn;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
            red[2][t] = fmax(red[2][t], red[2][t + w]);
            red[3][t] = fmin(red[3][t], red[3][t + w]);
        }
        __syncthreads();
    }
    if (t == 0) {
        const double cnt = (double)(a1 - a0);
        double v;
        switch (order) {
            case 1: v = red[0][0]; break;
            case 2: v = red[0][0] / cnt; break;
            case 3: v = red[2][0]; break;
            case 4: v = red[3][0]; break;
            case 5: v = red[1][0] / cnt; break;
            default: v = sqrt(red[1][0] / cnt); break;
        }
        sys[b] = v;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
int gmm_upload(vssr_handle *g, const double *means, const double *prec_chol, const double *weights) {
    const int K = g->gmm_K, D = g->gmm_D, Dp = g->gmm_Dp, NB = Dp / 16;
    std::vector<double> P((size_t)K * Dp * Dp, 0.0), c((size_t)K * Dp, 0.0), kc(2 * (size_t)K);
    std::vector<unsigned char> mask((size_t)K * NB * NB, 0);
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const double *Pk = prec_chol + (size_t)k * D * D;
        double logdet = 0.0;
        for (int i = 0; i < D; ++i) {
            logdet += std::log(Pk[(size_t)i * D + i]);
            for (int j = 0; j < D; ++j) {
                const double v = Pk[(size_t)i * D + j];
                P[((size_t)k * Dp + i) * Dp + j] = v;
                if (v != 0.0) mask[((size_t)k * NB + i / 16) * NB + j / 16] = 1;
            }
        }
        for (int j = 0; j < D; ++j) {
            double s = 0.0;
            for (int i = 0; i < D; ++i) s += means[(size_t)k * D + i] * Pk[(size_t)i * D + j];
            c[(size_t)k * Dp + j] = s;
        }
        kc[k] = logdet;
        kc[K + k] = std::log(weights[k]);   // (w = 0: -inf, the component drops out of the logsumexp)
    }
    if (g->d_gmm_P.ensure(sizeof(double) * P.size()) || g->d_gmm_c.ensure(sizeof(double) * c.size()) ||
        g->d_gmm_kc.ensure(sizeof(double) * kc.size()) || g->d_gmm_mask.ensure(mask.size()))
        return set_err(nullptr, VSSR_E_NOMEM, "device allocation failed (GMM parameters)");
    if (hipMemcpy(g->d_gmm_P.p, P.data(), sizeof(double) * P.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->d_gmm_c.p, c.data(), sizeof(double) * c.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->d_gmm_kc.p, kc.data(), sizeof(double) * kc.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->d_gmm_mask.p, mask.data(), mask.size(), hipMemcpyHostToDevice) != hipSuccess)
        return set_err(nullptr, VSSR_E_DEVICE, "copy of the GMM parameters failed");
    return VSSR_OK;
}

template <typename T>
static int gmm_score_any(vssr_handle *g, hipStream_t st, int64_t n, const T *x) {
    if (n <= 0) return VSSR_OK;
    const int K = g->gmm_K;
    if (g->d_gmm_lp.ensure(sizeof(double) * (size_t)n * K) || g->d_gmm_nll.ensure(sizeof(double) * (size_t)n))
        return set_err(g, VSSR_E_NOMEM, "device allocation failed (GMM workspace of %lld rows)", (long long)n);
    const dim3 grid((unsigned)((n + GMM_ROWS - 1) / GMM_ROWS)), blk(256);
    const double *P = g->d_gmm_P.as<double>(), *c = g->d_gmm_c.as<double>(), *kc = g->d_gmm_kc.as<double>();
    const unsigned char *mask = g->d_gmm_mask.as<unsigned char>();
    double *lp = g->d_gmm_lp.as<double>(), *nll = g->d_gmm_nll.as<double>();
    const int nn = (int)n;
    switch (g->gmm_Dp / 16) {
#define GMM_CASE(NB)                                                                                                          \
    case NB:                                                                                                                  \
        hipLaunchKernelGGL((k_gmm_logp<T, NB>), grid, blk, 0, st, x, nn, K, g->gmm_D, g->gmm_log2pi, P, c, kc, mask, lp, nll); \
        break;
        GMM_CASE(1) GMM_CASE(2) GMM_CASE(3) GMM_CASE(4) GMM_CASE(5) GMM_CASE(6) GMM_CASE(7) GMM_CASE(8)
        GMM_CASE(9) GMM_CASE(10) GMM_CASE(11) GMM_CASE(12) GMM_CASE(13) GMM_CASE(14) GMM_CASE(15) GMM_CASE(16)
#undef GMM_CASE
        default: return set_err(g, VSSR_E_BADARG, "GMM dimension %d out of range", g->gmm_D);
    }
    VSSR_HIP(g, hipGetLastError());
    return VSSR_OK;
}

int gmm_score_f64(vssr_handle *g, hipStream_t st, int64_t n, const double *x_dev) { return gmm_score_any(g, st, n, x_dev); }
int gmm_score_f32(vssr_handle *g, hipStream_t st, int64_t n, const float *x_dev) { return gmm_score_any(g, st, n, x_dev); }

int gmm_mean_rows(vssr_handle *g, hipStream_t st, int B, const int *start, const float *emb) {
    if (g->d_gmm_x.ensure(sizeof(double) * (size_t)B * g->gmm_Dp))
        return set_err(g, VSSR_E_NOMEM, "device allocation failed (GMM mean rows)");
    hipLaunchKernelGGL(k_gmm_mean_rows, dim3(B), dim3(256), 0, st, emb, g->gmm_D, g->gmm_Dp, start, g->d_gmm_x.as<double>());
    VSSR_HIP(g, hipGetLastError());
    return VSSR_OK;
}

int gmm_reduce(vssr_handle *g, hipStream_t st, int B, const int *start, int order) {
    if (g->d_gmm_sys.ensure(sizeof(double) * (size_t)B))
        return set_err(g, VSSR_E_NOMEM, "device allocation failed (GMM reductions)");
    hipLaunchKernelGGL(k_gmm_reduce, dim3(B), dim3(256), 0, st, g->d_gmm_nll.as<double>(), start, order, g->d_gmm_sys.as<double>());
    VSSR_HIP(g, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
