// cluster.hip — clustering of latent embeddings on the device, fp64 throughout (reference mcmc/utils/clustering.py::perform_clustering:
// sklearn PCA(n_components, whiten=True) on one row per structure, scipy linkage(X_r[:, :3], "ward"), fcluster in the Python layer).
//
// Rows live in the handle's GmmFit as fp64 [N][Dp] (the layout and the append paths of gmm_fit.hip).
// PCA:  k_clu_colsum / k_clu_mean (row slabs, summed in slab order) -> mean;  gmm_fit_centered_cov (k_fit_cov on
//       v_mfma_f64_16x16x4_f64 with unit responsibilities, k_fit_cov_finish with the divisor N - 1) -> C;  k_clu_eigh: cyclic Jacobi with
//       the round-robin parallel ordering in ONE workgroup (D / 2 disjoint rotations per step, D - 1 steps per sweep; the matrix and
//       the eigenvectors stay in a global workspace that L2 holds: 2 x 256 x 256 doubles do not fit LDS), a rotation is skipped once
//       |a_pq| <= eps |C|_F / D, every sweep ends by mirroring the upper triangle into the lower, the solve ends with the first sweep
//       that rotates nothing;  k_clu_components: order by decreasing
//       eigenvalue, sign (largest-magnitude loading positive), explained variance and ratio;  k_clu_project: X_r and the points.
// Ward linkage without a distance matrix (the hot path).  Live clusters are (centroid [d_pad], size, id) in list order.  Per round:
//   k_ward_nn      one thread per query cluster; the candidates stream through LDS in tiles of 256 (every lane reads the same LDS
//                  address: a broadcast, no bank conflict); key = |c_i - c_j|^2 s_i s_j / (s_i + s_j) (half the squared Ward distance;
//                  both operands enter symmetrically, so thread i and thread j see the same bits for the pair); strict < over
//                  ascending j: the lowest position wins a tie
//   k_ward_mark    pair flags (lower member of a reciprocal pair / survivor) and their per-workgroup counts
//   k_ward_scan    one workgroup: exclusive scan of the counts, new live count and record count into the counters
//   k_ward_apply   survivors move to their scanned position in the other buffer; the lower member of a pair becomes the merged
//                  cluster (size-weighted mean) and writes its record (ids, height, size) at its scanned record index
// The host reads 8 bytes per round (live count, records).  Every order is fixed: no atomics, identical bits on every run.
// Afterwards the host sorts the N - 1 records by height (stable) and renumbers them to scipy's Z.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <numeric>

#include "jacobi_dev.h"
#include "vssr_internal.h"

namespace vssr {

// ---- PCA ---------------------------------------------------------------------------------------------------------------------------
// grid slabs, thread d: column sums of the slab's rows, in row order
__global__ void __launch_bounds__(256)
k_clu_colsum(const double *__restrict__ X, int n, int Dp, int rows_per_slab, double *__restrict__ part) {
    const int d = threadIdx.x, sl = blockIdx.x;
    if (d >= Dp) return;
    const int r0 = sl * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
    double s = 0.0;
    for (int row = r0; row < r1; ++row) s += X[(size_t)row * Dp + d];
    part[(size_t)sl * Dp + d] = s;
}

// one workgroup: slabs summed in order; denom[0] = n - 1
__global__ void __launch_bounds__(256)
k_clu_mean(const double *__restrict__ part, int S, int n, int Dp, double *__restrict__ mean, double *__restrict__ denom) {
    const int d = threadIdx.x;
    if (d == 0) denom[0] = (double)(n - 1);
    if (d >= Dp) return;
    double s = 0.0;
    for (int sl = 0; sl < S; ++sl) s += part[(size_t)sl * Dp + d];
    mean[d] = s / (double)n;
}

// One workgroup.  A [Dp][Dp] <- cov (rows / columns < m), Vt [Dp][Dp] <- I; on return diag(A) = eigenvalues, ROWS of Vt = eigenvectors.
// info[0] = sweeps, info[1] = 1 when the last sweep rotated nothing.  The solver itself is jacobi_dev.h's (vib.hip runs it per group).
__global__ void __launch_bounds__(EIGH_THREADS)
k_clu_eigh(const double *__restrict__ cov, double *A, double *Vt, int m, int ld, int *__restrict__ info) {
    __shared__ double cs[2 * 128];
    __shared__ double red[EIGH_THREADS];
    __shared__ int rotated;
    int sweep, conv;
    jacobi_eigh(cov, ld, A, Vt, m, ld, cs, red, &rotated, sweep, conv);
    if (threadIdx.x == 0) { info[0] = sweep; info[1] = conv; }
}

// One workgroup of 256.  Eigenvalues by decreasing value (the lower index first on ties), clamped at 0 as sklearn does; component r =
// eigenvector with its largest-magnitude entry (the first on ties) made positive.  comp [nc][Dp], comp_t [Dp][nc].
__global__ void __launch_bounds__(256)
k_clu_components(const double *__restrict__ A, const double *__restrict__ Vt, int m, int ld, int nc, double *__restrict__ comp,
                 double *__restrict__ comp_t, double *__restrict__ ev, double *__restrict__ ratio) {
    __shared__ int order[256];
    __shared__ double lam[256];
    __shared__ double total;
    const int t = threadIdx.x;
    if (t < m) lam[t] = fmax(A[(size_t)t * ld + t], 0.0);
    __syncthreads();
    if (t < m) {
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += (lam[j] > lam[t] || (lam[j] == lam[t] && j < t)) ? 1 : 0;
        order[rank] = t;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int r = 0; r < m; ++r) s += lam[order[r]];
        total = s;
    }
    __syncthreads();
    if (t < nc) {
        const int src = order[t];
        const double *v = Vt + (size_t)src * ld;
        double best = -1.0, sign = 1.0;
        for (int d = 0; d < m; ++d) {
            const double a = fabs(v[d]);
            if (a > best) { best = a; sign = v[d] < 0.0 ? -1.0 : 1.0; }
        }
        for (int d = 0; d < ld; ++d) {
            const double x = d < m ? sign * v[d] : 0.0;
            comp[(size_t)t * ld + d] = x;
            comp_t[(size_t)d * nc + t] = x;
        }
        ev[t] = lam[src];
        ratio[t] = lam[src] / total;
    }
}

// thread per (row, component): X_r = sum_d (x_d - mean_d) V_dc in column order, / max(sqrt(l_c), eps) when whitening (sklearn clips the
// scale there); the first d_clu components also land in the point array of the linkage ([n][d_pad], pad coordinates zero)
__global__ void __launch_bounds__(256)
k_clu_project(const double *__restrict__ X, int64_t n, int D, int Dp, const double *__restrict__ mean, const double *__restrict__ comp_t,
              int nc, const double *__restrict__ ev, int whiten, double *__restrict__ xr, double *__restrict__ pts, int d_clu, int d_pad) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * nc) return;
    const int64_t row = idx / nc;
    const int c = (int)(idx - row * nc);
    const double *x = X + (size_t)row * Dp;
    double s = 0.0;
    for (int d = 0; d < D; ++d) s = fma(x[d] - mean[d], comp_t[(size_t)d * nc + c], s);
    if (whiten) s /= fmax(sqrt(ev[c]), DBL_EPSILON);
    xr[idx] = s;
    if (c < d_clu) pts[(size_t)row * d_pad + c] = s;
    if (c == 0)
        for (int e = d_clu; e < d_pad; ++e) pts[(size_t)row * d_pad + e] = 0.0;
}

// ---- Ward linkage ------------------------------------------------------------------------------------------------------------------
// candidates per LDS tile: 256 up to 8 coordinates, fewer beyond (a tile of 32 coordinates stays at 16 KB)
__host__ __device__ constexpr int ward_tile(int dc) { return dc <= 8 ? 256 : dc == 16 ? 128 : 64; }

__global__ void __launch_bounds__(256)
k_ward_init(const double *__restrict__ pts, int n, int d_pad, double *__restrict__ cen, double *__restrict__ siz, int *__restrict__ cid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int e = 0; e < d_pad; ++e) cen[(size_t)i * d_pad + e] = pts[(size_t)i * d_pad + e];
    siz[i] = 1.0;
    cid[i] = i;
}

// DC = d_pad.  nn[i] = position of the nearest other live cluster (lowest position on ties)
template <int DC>
__global__ void __launch_bounds__(256)
k_ward_nn(const double *__restrict__ cen, const double *__restrict__ siz, int m, int *__restrict__ nn) {
    constexpr int WARD_TILE = ward_tile(DC);
    __shared__ double tc[WARD_TILE * DC];
    __shared__ double ts[WARD_TILE];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const int ic = min(i, m - 1);
    double q[DC];
#pragma unroll
    for (int e = 0; e < DC; ++e) q[e] = cen[(size_t)ic * DC + e];
    const double si = siz[ic];
    double best = INFINITY;
    int arg = -1;
    for (int j0 = 0; j0 < m; j0 += WARD_TILE) {
        const int cnt = min(WARD_TILE, m - j0);
        __syncthreads();
        for (int t = tid; t < cnt * DC; t += 256) tc[t] = cen[(size_t)j0 * DC + t];
        if (tid < cnt) ts[tid] = siz[j0 + tid];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            double d2 = 0.0;
#pragma unroll
            for (int e = 0; e < DC; ++e) {
                const double df = q[e] - tc[j * DC + e];
                d2 = fma(df, df, d2);
            }
            const double sj = ts[j];
            const double key = d2 * ((si * sj) / (si + sj));
            if (key < best && j0 + j != i) { best = key; arg = j0 + j; }
        }
    }
    if (i < m) nn[i] = arg;
}

// flag[i]: bit 0 = survivor (not the upper member of a reciprocal pair), bit 1 = lower member of a reciprocal pair (merges).
// blk[b] = {survivors, merges} of workgroup b
__global__ void __launch_bounds__(256)
k_ward_mark(const int *__restrict__ nn, int m, unsigned char *__restrict__ flag, int2 *__restrict__ blk) {
    __shared__ int cs[256], cm[256];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    int keep = 0, mrg = 0;
    if (i < m) {
        const int j = nn[i];
        const bool recip = j >= 0 && nn[j] == i;
        keep = (recip && j < i) ? 0 : 1;
        mrg = (recip && i < j) ? 1 : 0;
        flag[i] = (unsigned char)(keep | (mrg << 1));
    }
    cs[tid] = keep; cm[tid] = mrg;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { cs[tid] += cs[tid + w]; cm[tid] += cm[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) blk[blockIdx.x] = make_int2(cs[0], cm[0]);
}

// one workgroup: blk -> exclusive offsets (in place); counters = {new live count, records so far (in / out)}
__global__ void __launch_bounds__(256)
k_ward_scan(int2 *__restrict__ blk, int nb, int *__restrict__ counters) {
    __shared__ int2 tot[256];
    const int tid = threadIdx.x;
    const int per = (nb + 255) / 256, b0 = tid * per, b1 = min(nb, b0 + per);
    int2 s = make_int2(0, 0);
    for (int b = b0; b < b1; ++b) { s.x += blk[b].x; s.y += blk[b].y; }
    tot[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int2 run = make_int2(0, 0);
        for (int t = 0; t < 256; ++t) {
            const int2 v = tot[t];
            tot[t] = run;
            run.x += v.x; run.y += v.y;
        }
        counters[0] = run.x;
        counters[2] = counters[1];      // record base of this round
        counters[1] += run.y;
    }
    __syncthreads();
    int2 run = tot[tid];
    for (int b = b0; b < b1; ++b) {
        const int2 v = blk[b];
        blk[b] = run;
        run.x += v.x; run.y += v.y;
    }
}

// survivors -> position in the other buffer; merges: centroid = size-weighted mean, record {id_i, id_j, height, size}, id = n + record
template <int DC>
__global__ void __launch_bounds__(256)
k_ward_apply(const double *__restrict__ cen, const double *__restrict__ siz, const int *__restrict__ cid, const int *__restrict__ nn,
             const unsigned char *__restrict__ flag, const int2 *__restrict__ blk, const int *__restrict__ counters, int m, int n,
             double *__restrict__ cen2, double *__restrict__ siz2, int *__restrict__ cid2, double *__restrict__ rec) {
    __shared__ int ps[256], pm[256];
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    const int f = i < m ? flag[i] : 0;
    ps[tid] = f & 1; pm[tid] = (f >> 1) & 1;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // inclusive scan of both flags
        const int a = tid >= off ? ps[tid - off] : 0, b = tid >= off ? pm[tid - off] : 0;
        __syncthreads();
        ps[tid] += a; pm[tid] += b;
        __syncthreads();
    }
    if (!(f & 1)) return;
    const int2 base = blk[blockIdx.x];
    const int pos = base.x + ps[tid] - 1;
    if (!(f & 2)) {
#pragma unroll
        for (int e = 0; e < DC; ++e) cen2[(size_t)pos * DC + e] = cen[(size_t)i * DC + e];
        siz2[pos] = siz[i];
        cid2[pos] = cid[i];
        return;
    }
    const int j = nn[i], r = counters[2] + base.y + pm[tid] - 1;
    const double si = siz[i], sj = siz[j], st = si + sj;
    double d2 = 0.0;
#pragma unroll
    for (int e = 0; e < DC; ++e) {
        const double a = cen[(size_t)i * DC + e], b = cen[(size_t)j * DC + e];
        const double df = a - b;
        d2 = fma(df, df, d2);
        cen2[(size_t)pos * DC + e] = (si * a + sj * b) / st;
    }
    siz2[pos] = st;
    cid2[pos] = n + r;
    rec[(size_t)r * 4 + 0] = (double)cid[i];
    rec[(size_t)r * 4 + 1] = (double)cid[j];
    rec[(size_t)r * 4 + 2] = sqrt(2.0 * ((si * sj) / st)) * sqrt(d2);
    rec[(size_t)r * 4 + 3] = st;
}

template <int DC>
static void ward_round(hipStream_t st, Cluster *c, int cur, int m, int n) {
    const int nb = (m + 255) / 256;
    hipLaunchKernelGGL(k_ward_nn<DC>, dim3(nb), dim3(256), 0, st, c->cen[cur].as<double>(), c->siz[cur].as<double>(), m, c->nn.as<int>());
    hipLaunchKernelGGL(k_ward_mark, dim3(nb), dim3(256), 0, st, c->nn.as<int>(), m, c->flag.as<unsigned char>(), c->blk.as<int2>());
    hipLaunchKernelGGL(k_ward_scan, dim3(1), dim3(256), 0, st, c->blk.as<int2>(), nb, c->counters.as<int>());
    hipLaunchKernelGGL(k_ward_apply<DC>, dim3(nb), dim3(256), 0, st, c->cen[cur].as<double>(), c->siz[cur].as<double>(),
                       c->cid[cur].as<int>(), c->nn.as<int>(), c->flag.as<unsigned char>(), c->blk.as<int2>(), c->counters.as<int>(), m, n,
                       c->cen[cur ^ 1].as<double>(), c->siz[cur ^ 1].as<double>(), c->cid[cur ^ 1].as<int>(), c->rec.as<double>());
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
int cluster_pad_dims(int d) { return d <= 4 ? d : d <= 8 ? 8 : d <= 16 ? 16 : 32; }

int cluster_pca(vssr_handle *h, vssr_cluster_pca_result *res) {
    Cluster *c = h->clu.get();
    const int D = h->gmm_D, Dp = h->gmm_Dp, n = (int)h->fit->n, nc = c->n_components;
    const size_t d = sizeof(double);
    hipStream_t st = h->stream;
    c->pca_done = false;
    c->n_pts = 0;
    const int n_blk = (n + 255) / 256;
    const int S = std::max(1, std::min(n_blk, 1024));
    const int rps = (n + S - 1) / S, S2 = (n + rps - 1) / rps;
    if (c->mean.ensure(d * Dp) || c->denom.ensure(d) || c->part_sum.ensure(d * (size_t)S2 * Dp) || c->cov.ensure(d * (size_t)Dp * Dp) ||
        c->jac.ensure(d * (size_t)Dp * Dp) || c->evec.ensure(d * (size_t)Dp * Dp) || c->comp.ensure(d * (size_t)nc * Dp) ||
        c->comp_t.ensure(d * (size_t)nc * Dp) || c->ev.ensure(d * nc) || c->ratio.ensure(d * nc) || c->counters.ensure(sizeof(int) * 8) ||
        c->xr.ensure(d * (size_t)n * nc) || c->pts.ensure(d * (size_t)n * c->d_pad))
        return set_err(h, VSSR_E_NOMEM, "device allocation failed (PCA workspaces: %d rows, D = %d)", n, D);
    hipLaunchKernelGGL(k_clu_colsum, dim3(S2), dim3(256), 0, st, h->fit->x(), n, Dp, rps, c->part_sum.as<double>());
    hipLaunchKernelGGL(k_clu_mean, dim3(1), dim3(256), 0, st, c->part_sum.as<double>(), S2, n, Dp, c->mean.as<double>(), c->denom.as<double>());
    VSSR_HIP(h, hipGetLastError());
    int rc = gmm_fit_centered_cov(h, st, h->fit->x(), n, D, Dp, c->mean.as<double>(), c->denom.as<double>(), c->part_cov, c->cov.as<double>());
    if (rc) return rc;
    int *info = c->counters.as<int>() + 4;
    hipLaunchKernelGGL(k_clu_eigh, dim3(1), dim3(EIGH_THREADS), 0, st, c->cov.as<double>(), c->jac.as<double>(), c->evec.as<double>(), D, Dp, info);
    hipLaunchKernelGGL(k_clu_components, dim3(1), dim3(256), 0, st, c->jac.as<double>(), c->evec.as<double>(), D, Dp, nc, c->comp.as<double>(),
                       c->comp_t.as<double>(), c->ev.as<double>(), c->ratio.as<double>());
    const int64_t tot = (int64_t)n * nc;
    hipLaunchKernelGGL(k_clu_project, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, h->fit->x(), (int64_t)n, D, Dp, c->mean.as<double>(),
                       c->comp_t.as<double>(), nc, c->ev.as<double>(), c->whiten, c->xr.as<double>(), c->pts.as<double>(), c->d_clu, c->d_pad);
    VSSR_HIP(h, hipGetLastError());
    int hinfo[2] = {0, 0};
    VSSR_HIP(h, hipMemcpyAsync(hinfo, info, sizeof(hinfo), hipMemcpyDeviceToHost, st));
    VSSR_HIP(h, hipStreamSynchronize(st));
    c->pca_done = true;
    c->n_pts = n;
    if (res) { res->n_rows = n; res->n_sweeps = hinfo[0]; res->converged = hinfo[1]; }
    return VSSR_OK;
}

int cluster_pca_params(vssr_handle *h, double *mean, double *components, double *explained_variance, double *ratio) {
    Cluster *c = h->clu.get();
    const int D = h->gmm_D, Dp = h->gmm_Dp, nc = c->n_components;
    const size_t d = sizeof(double);
    if (mean) VSSR_HIP(h, hipMemcpy(mean, c->mean.p, d * D, hipMemcpyDeviceToHost));
    if (components) VSSR_HIP(h, hipMemcpy2D(components, d * D, c->comp.p, d * Dp, d * D, nc, hipMemcpyDeviceToHost));
    if (explained_variance) VSSR_HIP(h, hipMemcpy(explained_variance, c->ev.p, d * nc, hipMemcpyDeviceToHost));
    if (ratio) VSSR_HIP(h, hipMemcpy(ratio, c->ratio.p, d * nc, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int cluster_projected(vssr_handle *h, int64_t first, int64_t n_rows, double *xr) {
    Cluster *c = h->clu.get();
    const size_t row = sizeof(double) * c->n_components;
    VSSR_HIP(h, hipMemcpy(xr, c->xr.as<char>() + (size_t)first * row, (size_t)n_rows * row, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int cluster_set_points(vssr_handle *h, int64_t n, const double *pts) {
    Cluster *c = h->clu.get();
    const size_t d = sizeof(double);
    c->n_pts = 0;
    if (c->pts.ensure(d * (size_t)n * c->d_pad)) return set_err(h, VSSR_E_NOMEM, "device allocation failed (%lld points)", (long long)n);
    if (c->d_pad == c->d_clu) {
        VSSR_HIP(h, hipMemcpy(c->pts.p, pts, d * (size_t)n * c->d_clu, hipMemcpyHostToDevice));
    } else {
        VSSR_HIP(h, hipMemset(c->pts.p, 0, d * (size_t)n * c->d_pad));
        VSSR_HIP(h, hipMemcpy2D(c->pts.p, d * c->d_pad, pts, d * c->d_clu, d * c->d_clu, (size_t)n, hipMemcpyHostToDevice));
    }
    c->n_pts = n;
    return VSSR_OK;
}

int cluster_linkage(vssr_handle *h, double *Z, int32_t *n_rounds) {
    Cluster *c = h->clu.get();
    const int n = (int)c->n_pts, dp = c->d_pad;
    const size_t d = sizeof(double);
    hipStream_t st = h->stream;
    const int nb0 = (n + 255) / 256;
    for (int b = 0; b < 2; ++b)
        if (c->cen[b].ensure(d * (size_t)n * dp) || c->siz[b].ensure(d * (size_t)n) || c->cid[b].ensure(sizeof(int) * (size_t)n))
            return set_err(h, VSSR_E_NOMEM, "device allocation failed (linkage state, %d points)", n);
    if (c->nn.ensure(sizeof(int) * (size_t)n) || c->flag.ensure((size_t)n) || c->blk.ensure(sizeof(int2) * (size_t)nb0) ||
        c->rec.ensure(d * 4 * (size_t)n) || c->counters.ensure(sizeof(int) * 8))
        return set_err(h, VSSR_E_NOMEM, "device allocation failed (linkage workspaces, %d points)", n);
    VSSR_HIP(h, hipMemsetAsync(c->counters.p, 0, sizeof(int) * 4, st));
    hipLaunchKernelGGL(k_ward_init, dim3(nb0), dim3(256), 0, st, c->pts.as<double>(), n, dp, c->cen[0].as<double>(), c->siz[0].as<double>(),
                       c->cid[0].as<int>());
    VSSR_HIP(h, hipGetLastError());
    int m = n, cur = 0, rounds = 0;
    while (m > 1) {
        switch (dp) {
            case 1: ward_round<1>(st, c, cur, m, n); break;
            case 2: ward_round<2>(st, c, cur, m, n); break;
            case 3: ward_round<3>(st, c, cur, m, n); break;
            case 4: ward_round<4>(st, c, cur, m, n); break;
            case 8: ward_round<8>(st, c, cur, m, n); break;
            case 16: ward_round<16>(st, c, cur, m, n); break;
            default: ward_round<32>(st, c, cur, m, n); break;
        }
        VSSR_HIP(h, hipGetLastError());
        int cnt[2] = {0, 0};   // the one read-back of the round: live count, records
        VSSR_HIP(h, hipMemcpyAsync(cnt, c->counters.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
        VSSR_HIP(h, hipStreamSynchronize(st));
        ++rounds;
        if (cnt[0] >= m || cnt[0] < 1 || cnt[1] != n - cnt[0])
            return set_err(h, VSSR_E_STATE, "Ward linkage: round %d left %d of %d clusters with %d records (a non-finite point?)", rounds, cnt[0], m, cnt[1]);
        m = cnt[0];
        cur ^= 1;
    }
    if (n_rounds) *n_rounds = rounds;
    // records -> scipy's Z: stable sort by height; record r (creation order, internal id n + r) becomes row rank[r] with id n + rank[r]
    const int nr = n - 1;
    std::vector<double> rec((size_t)nr * 4);
    VSSR_HIP(h, hipMemcpy(rec.data(), c->rec.p, d * 4 * (size_t)nr, hipMemcpyDeviceToHost));
    std::vector<int> order(nr), rank(nr);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rec[(size_t)a * 4 + 2] < rec[(size_t)b * 4 + 2]; });
    for (int r = 0; r < nr; ++r) rank[order[r]] = r;
    for (int r = 0; r < nr; ++r) {
        const double *s = rec.data() + (size_t)order[r] * 4;
        int a = (int)s[0], b = (int)s[1];
        if (a >= n) a = n + rank[a - n];
        if (b >= n) b = n + rank[b - n];
        Z[(size_t)r * 4 + 0] = (double)std::min(a, b);
        Z[(size_t)r * 4 + 1] = (double)std::max(a, b);
        Z[(size_t)r * 4 + 2] = s[2];
        Z[(size_t)r * 4 + 3] = s[3];
    }
    return VSSR_OK;
}

}  // namespace vssr
