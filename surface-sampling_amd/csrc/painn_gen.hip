// painn_gen.hip — the general-width PaiNN ensemble path on gfx950: any feat_dim F that is a multiple of 16 in 16 .. 256,
// any n_rbf R in 1 .. 32, in exact fp32.
//
// Same math as painn.hip and oracle/painn_impl.inc, written for a runtime F and R:
//   node GEMMs (W1, W2, [U;V], W3, W4, W5 and their transposes in the reverse pass) -- one LDS-tiled kernel on
//     v_mfma_f32_16x16x4_f32 (exact f32 products, k-ordered f32 accumulation) with fused bias / swish / swish' / residual
//     epilogues;
//   edge kernels -- the gather pattern of painn.hip k_edge_fwd / k_edge_bwd: one workgroup per (centre, model), thread =
//     feature, ECHUNK slots staged per step with the radial functions computed on the fly; every edge quantity is accumulated
//     by the workgroup that owns the centre (no float atomics, run-to-run deterministic), rows of any length take more chunks;
//   small element-wise kernels for the update block's norms / gates and the readout.
// The reverse pass leaves dE/dr per neighbor slot in the final gbar layout of the 128 / 20 path ([M][slot_cap] float4, one
// buffer per model), so force assembly, stress, the relaxation drivers and the result downloads are shared.
#include "vssr_internal.h"

namespace vssr {

namespace {

constexpr int ECH = 16;        // slots staged per step in the edge kernels
constexpr int GT = 64;         // GEMM output tile: GT rows x GT columns per workgroup (4 waves of 16 rows)
constexpr int GK = 32;         // GEMM k-step staged in LDS
constexpr float PI_G = 3.14159265358979323846f;
constexpr float NRM_EPS = 1e-15f;

__device__ inline float sig_g(float x) { return 1.f / (1.f + expf(-x)); }
__device__ inline float swish_g(float x) { return x * sig_g(x); }
__device__ inline float dswish_g(float x) {
    const float sg = sig_g(x);
    return sg * fmaf(x, 1.f - sg, 1.f);
}

// ---- weights: one image per model, the same offsets for every model ----------------------------------------------------
struct GenLayer {
    size_t W1t, b1, W1, W2t, b2, W2, Wd, bd, UVt, UV, W3t, b3, W3, W4t, b4, W4;
};
struct GenLayout {
    size_t embed;
    GenLayer layer[MAX_LAYERS];
    size_t W5t, b5, W5, w6, b6;
    size_t len;   // floats per model image
};

GenLayout gen_layout(int F, int R, int H, int NE, int L) {
    GenLayout g{};
    const size_t F3 = 3 * (size_t)F;
    size_t o = 0;
    auto take = [&](size_t n) { const size_t r = o; o += (n + 3) & ~(size_t)3; return r; };
    g.embed = take((size_t)NE * F);
    for (int l = 0; l < L; ++l) {
        GenLayer &w = g.layer[l];
        w.W1t = take((size_t)F * F); w.b1 = take(F); w.W1 = take((size_t)F * F);
        w.W2t = take(F * F3); w.b2 = take(F3); w.W2 = take(F3 * F);
        w.Wd = take(F3 * R); w.bd = take(F3);
        w.UVt = take((size_t)F * 2 * F); w.UV = take((size_t)2 * F * F);
        w.W3t = take((size_t)2 * F * F); w.b3 = take(F); w.W3 = take((size_t)F * 2 * F);
        w.W4t = take(F * F3); w.b4 = take(F3); w.W4 = take(F3 * F);
    }
    g.W5t = take((size_t)F * H); g.b5 = take(H); g.W5 = take((size_t)H * F); g.w6 = take(H); g.b6 = take(1);
    g.len = o;
    return g;
}

// ---- node GEMM: C[r][c] = epi( bias[c] + sum_k act(A[r][k]) B[k][c] ), per model (grid.z) -----------------------------------
enum { EPI_STORE = 0, EPI_DSWISH = 1, EPI_ADD = 2 };
struct GemmP {
    int rows, K, Nc, rpa;                 // rows per model, inner dimension, output columns, rows per atom (1: s-like, 3: v-like)
    const float *A; long long lda, a_ms;  // A[m][r][k] = A[m * a_ms + r * lda + k]
    const float *B; long long ldb, b_ms;  // B[k][c]   = B[m * b_ms + k * ldb + c]  (weight image of model m)
    const float *bias;                    // [Nc] in the weight image (model stride b_ms) or null
    float *C; long long ldc, c_ms;
    const float *X; long long ldx, x_ms;  // EPI_DSWISH: C = acc * swish'(X);  EPI_ADD: C = acc + X
    int a_swish, epi;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) k_gen_gemm(GemmP p, ActiveView av) {
    __shared__ float As[GT][GK + 1];
    __shared__ float Bs[GK][GT + 4];
    __shared__ float fence[256];   // written, never read: see gemm_fence
    const int m = blockIdx.z, r0 = blockIdx.x * GT, c0 = blockIdx.y * GT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (!av.tile(r0 / p.rpa, min(r0 + GT - 1, p.rows - 1) / p.rpa)) return;
    const float *A = p.A + (size_t)m * p.a_ms;
    const float *B = p.B + (size_t)m * p.b_ms;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {   // the bias first, then the products in k order (the oracle's order of the same sum)
        const int col = c0 + 16 * t + (lane & 15);
        const float bv = (p.bias && col < p.Nc) ? p.bias[(size_t)m * p.b_ms + col] : 0.f;
        acc[t] = f32x4{bv, bv, bv, bv};
    }
    for (int k0 = 0; k0 < p.K; k0 += GK) {
        for (int idx = tid; idx < GT * GK; idx += 256) {
            const int r = idx / GK, k = idx % GK, gr = r0 + r, gk = k0 + k;
            float v = (gr < p.rows && gk < p.K) ? A[(size_t)gr * p.lda + gk] : 0.f;
            if (p.a_swish) v = swish_g(v);
            As[r][k] = v;
        }
        for (int idx = tid; idx < GK * GT; idx += 256) {
            const int k = idx / GT, c = idx % GT, gk = k0 + k, gc = c0 + c;
            Bs[k][c] = (gk < p.K && gc < p.Nc) ? B[(size_t)gk * p.ldb + gc] : 0.f;
        }
        __syncthreads();
        // MFMA source-register rule of this project (DESIGN.md "MFMA hazard rules", profiles/r01/NOTES_mfma_hazards.md): an MFMA
        // queued behind others reads its A / B registers late, and nothing protects them from a later writer.  So every operand of
        // the k-step is read from LDS first, the 32 MFMAs follow with no instruction between them (the four accumulators rotate:
        // each product's accumulator producer is four MFMAs back), and nothing that could reuse their source registers is issued
        // before a VALU has consumed the final value of every accumulator chain (gemm_fence below).
        float a[GK / 4], b[GK / 4][4];
#pragma unroll
        for (int kk = 0; kk < GK / 4; ++kk) {
            a[kk] = As[16 * wave + (lane & 15)][4 * kk + (lane >> 4)];
#pragma unroll
            for (int t = 0; t < 4; ++t) b[kk][t] = Bs[4 * kk + (lane >> 4)][16 * t + (lane & 15)];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < GK / 4; ++kk)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk][t], acc[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        // gemm_fence: the result of the group's last MFMA (it writes acc[3]) goes to an LDS cell nobody reads.  The matrix pipe
        // completes in order and waves issue in order, so every instruction behind this store -- the next k-step's loads, the
        // epilogue -- issues after all 32 MFMAs have read their sources.  (volatile: otherwise the store, and with it the
        // ordering, would be dropped.)
        *(volatile __attribute__((address_space(3))) float *)(fence + tid) = acc[3][0];
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
    }
    float *C = p.C + (size_t)m * p.c_ms;
    const float *X = p.X ? p.X + (size_t)m * p.x_ms : nullptr;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = c0 + 16 * t + (lane & 15);
        if (col >= p.Nc) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + 16 * wave + 4 * (lane >> 4) + i;
            if (row >= p.rows) continue;
            float v = acc[t][i];
            if (p.epi == EPI_DSWISH) v *= dswish_g(X[(size_t)row * p.ldx + col]);
            else if (p.epi == EPI_ADD) v += X[(size_t)row * p.ldx + col];
            C[(size_t)row * p.ldc + col] = v;
        }
    }
}

// ---- element-wise kernels: grid (ceil(N F / 256), M), thread = (atom, feature) ------------------------------------------------
__global__ void __launch_bounds__(256)
k_gen_embed(int N, int F, const int *__restrict__ Z, const float *__restrict__ Wimg, long long w_ms, size_t embed,
            float *__restrict__ s0, float *__restrict__ v0, ActiveView av) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (t >= (size_t)N * F) return;
    const int i = (int)(t / F), f = (int)(t % F);
    if (!av.atom(i)) return;
    const size_t a = (size_t)m * N + i;
    s0[a * F + f] = Wimg[(size_t)m * w_ms + embed + (size_t)Z[i] * F + f];
    v0[(a * 3 + 0) * F + f] = 0.f;
    v0[(a * 3 + 1) * F + f] = 0.f;
    v0[(a * 3 + 2) * F + f] = 0.f;
}

// norms of V v: X3[i][F + f] = sqrt(sum_x (Vv_x^2 + eps))   (UVv: [M][N][3][2F], U v in columns 0..F-1, V v in F..2F-1)
__global__ void __launch_bounds__(256)
k_gen_upd_norm(int N, int F, const float *__restrict__ UVv, float *__restrict__ X3, ActiveView av) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (t >= (size_t)N * F) return;
    const int i = (int)(t / F), f = (int)(t % F);
    if (!av.atom(i)) return;
    const size_t a = (size_t)m * N + i;
    float acc = 0.f;
    for (int x = 0; x < 3; ++x) {
        const float vv = UVv[(a * 3 + x) * 2 * F + F + f];
        acc += vv * vv + NRM_EPS;
    }
    X3[a * 2 * F + F + f] = sqrtf(acc);
}

// s_out = s_msg + a_sv <U v, V v> + a_ss ;  v_out = v_msg + a_vv U v   (q: [M][N][3F] = a_vv | a_sv | a_ss)
__global__ void __launch_bounds__(256)
k_gen_upd_out(int N, int F, const float *__restrict__ X3, const float *__restrict__ v_msg, const float *__restrict__ UVv,
              const float *__restrict__ q, float *__restrict__ s_out, float *__restrict__ v_out, ActiveView av) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (t >= (size_t)N * F) return;
    const int i = (int)(t / F), f = (int)(t % F);
    if (!av.atom(i)) return;
    const size_t a = (size_t)m * N + i;
    const float avv = q[a * 3 * F + f], asv = q[a * 3 * F + F + f], ass = q[a * 3 * F + 2 * F + f];
    float inner = 0.f;
    for (int x = 0; x < 3; ++x) {
        const float uv = UVv[(a * 3 + x) * 2 * F + f], vv = UVv[(a * 3 + x) * 2 * F + F + f];
        inner += uv * vv;
        if (v_out) v_out[(a * 3 + x) * F + f] = v_msg[(a * 3 + x) * F + f] + avv * uv;
    }
    s_out[a * F + f] = X3[a * 2 * F + f] + asv * inner + ass;
}

// update block reverse, part 1: qbar = [sum_x vbar U v | sbar <U v, V v> | sbar], UVbar = [vbar a_vv + sbar a_sv V v | sbar a_sv U v]
__global__ void __launch_bounds__(256)
k_gen_upd_bwd1(int N, int F, const float *__restrict__ UVv, const float *__restrict__ q, const float *__restrict__ sbar,
               const float *__restrict__ vbar, float *__restrict__ qbar, float *__restrict__ UVbar, ActiveView av) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (t >= (size_t)N * F) return;
    const int i = (int)(t / F), f = (int)(t % F);
    if (!av.atom(i)) return;
    const size_t a = (size_t)m * N + i;
    const float avv = q[a * 3 * F + f], asv = q[a * 3 * F + F + f];
    const float sb = sbar[a * F + f];
    float abar_vv = 0.f, inner = 0.f;
    for (int x = 0; x < 3; ++x) {
        const size_t r = (a * 3 + x) * 2 * F;
        const float uv = UVv[r + f], vv = UVv[r + F + f], vb = vbar[(a * 3 + x) * F + f];
        abar_vv += vb * uv;
        inner += uv * vv;
        UVbar[r + f] = vb * avv + sb * asv * vv;
        UVbar[r + F + f] = sb * asv * uv;
    }
    qbar[a * 3 * F + f] = abar_vv;
    qbar[a * 3 * F + F + f] = sb * inner;
    qbar[a * 3 * F + 2 * F + f] = sb;
}

// part 2 (after tmp2 = (W4^T qbar * swish'(h3)) W3): s1bar = sbar + tmp2[:F];  V v-bar += nbar V v / |V v|
__global__ void __launch_bounds__(256)
k_gen_upd_bwd2(int N, int F, const float *__restrict__ UVv, const float *__restrict__ X3, const float *__restrict__ tmp2,
               const float *__restrict__ sbar, float *__restrict__ s1bar, float *__restrict__ UVbar, ActiveView av) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (t >= (size_t)N * F) return;
    const int i = (int)(t / F), f = (int)(t % F);
    if (!av.atom(i)) return;
    const size_t a = (size_t)m * N + i;
    s1bar[a * F + f] = sbar[a * F + f] + tmp2[a * 2 * F + f];
    const float nb = tmp2[a * 2 * F + F + f], nn = X3[a * 2 * F + F + f];
    for (int x = 0; x < 3; ++x) {
        const size_t r = (a * 3 + x) * 2 * F;
        UVbar[r + F + f] += nb * UVv[r + F + f] / nn;
    }
}

// readout tail: e_i = b6 + sum_o w6[o] swish(h5[o]) (+ excluded volume); with forces, h5 is replaced by w6 swish'(h5) in place
__global__ void __launch_bounds__(256)
k_gen_readout(int N, int H, const float *__restrict__ Wimg, long long w_ms, size_t w6_off, size_t b6_off, float *__restrict__ h5,
              const float *__restrict__ e_excl, float *__restrict__ e_atom, int want_bar, ActiveView av) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
    if (i >= N || !av.atom(i)) return;
    const float *w6 = Wimg + (size_t)m * w_ms + w6_off;
    float *h = h5 + ((size_t)m * N + i) * H;
    float e = Wimg[(size_t)m * w_ms + b6_off];
    for (int o = 0; o < H; ++o) {
        const float x = h[o];
        e += w6[o] * swish_g(x);
        if (want_bar) h[o] = w6[o] * dswish_g(x);
    }
    if (e_excl) e += e_excl[i];
    e_atom[(size_t)m * N + i] = e;
}

// ---- edge kernels ----------------------------------------------------------------------------------------------------------
// RP: radial functions + the envelope column, padded (R + 1 <= RP); the filter weights of a feature live in registers
template <int RP>
struct GenChunk {
    float rho[ECH][RP];
    float drho[ECH][RP];
    float u[ECH][4];   // unit vector centre -> neighbor, [3] = distance
    float rep[ECH];    // (sigma / d)^p
    int j[ECH];
    float fc[ECH], dfc[ECH];
};

template <int RP, bool DERIV>
__device__ inline void gen_stage(GenChunk<RP> &S, const float4 *__restrict__ edge, int e0, int ne, int R, float rc, float excl_sigma,
                                 int excl_power) {
    const int tid = threadIdx.x;
    if (tid < ECH) {
        int j = -1;
        float d = 1.f, fc = 0.f, dfc = 0.f, ux = 0.f, uy = 0.f, uz = 0.f, rep = 0.f;
        if (tid < ne) {
            const float4 ed = edge[e0 + tid];
            j = __float_as_int(ed.w);
            if (j >= 0) {
                d = sqrtf(fmaf(ed.z, ed.z, fmaf(ed.y, ed.y, ed.x * ed.x)));
                const float inv = 1.f / d;
                ux = ed.x * inv; uy = ed.y * inv; uz = ed.z * inv;
                if (d < rc) {
                    fc = 0.5f * (cosf(PI_G * d / rc) + 1.f);
                    dfc = -0.5f * PI_G / rc * sinf(PI_G * d / rc);
                }
                rep = powf(excl_sigma / d, (float)excl_power);
            }
        }
        S.j[tid] = j;
        S.u[tid][0] = ux; S.u[tid][1] = uy; S.u[tid][2] = uz; S.u[tid][3] = d;
        S.fc[tid] = fc; S.dfc[tid] = dfc; S.rep[tid] = rep;
    }
    __syncthreads();
    for (int p = tid; p < ECH * RP; p += blockDim.x) {
        const int e = p / RP, k = p % RP;
        float r = 0.f, dr = 0.f;
        if (S.j[e] >= 0) {
            if (k < R) {
                const float d = S.u[e][3], a = (float)(k + 1) * PI_G / rc;
                float sn, cs;
                sincosf(a * d, &sn, &cs);
                const float rb = sn / d;
                r = rb * S.fc[e];
                if (DERIV) dr = fmaf(a * cs / d - sn / (d * d), S.fc[e], rb * S.dfc[e]);
            } else if (k == R) {
                r = S.fc[e];
                dr = S.dfc[e];
            }
        }
        S.rho[e][k] = r;
        if (DERIV) S.drho[e][k] = dr;
    }
    __syncthreads();
}

// filter weights of feature f in the three sections: w[s][k] = Wd[sF + f][k] (k < R), bd[sF + f] (k = R), 0 beyond
template <int RP>
__device__ inline void gen_filter(const float *__restrict__ Wd, const float *__restrict__ bd, int F, int R, int f, float (&w)[3][RP]) {
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int k = 0; k < RP; ++k)
            w[s][k] = f >= F ? 0.f : k < R ? Wd[(size_t)(s * F + f) * R + k] : k == R ? bd[s * F + f] : 0.f;
}

// message block, forward: one workgroup per (centre i, model), thread = feature.
// s_msg_i = s_i + sum_e phi_j[b] w_e[b] (written into columns 0..F-1 of X3, row stride 2F);
// v_msg_i = v_i + sum_e (phi_j[c] w_e[c] u_e + phi_j[a] w_e[a] v_j).  Layer 0 (first = 1) also writes the excluded-volume
// energy of the centre (model 0).
template <int RP>
__global__ void __launch_bounds__(256)
k_gen_edge_fwd(int N, int F, int R, const float *__restrict__ Wimg, long long w_ms, size_t wd_off, size_t bd_off, GraphView G,
               const int *__restrict__ counters, float rc, float excl_sigma, int excl_power, int first, const float *__restrict__ s_in,
               const float *__restrict__ v_in, const float *__restrict__ phi, float *__restrict__ X3, float *__restrict__ v_msg,
               float *__restrict__ e_excl) {
    __shared__ GenChunk<RP> S;
    if (counters[2] || !G.act.atom(blockIdx.x)) return;
    const int i = blockIdx.x, m = blockIdx.y, f = threadIdx.x;
    const int F3 = 3 * F;
    float w[3][RP];
    gen_filter<RP>(Wimg + (size_t)m * w_ms + wd_off, Wimg + (size_t)m * w_ms + bd_off, F, R, f, w);
    const size_t mN = (size_t)m * N;
    float acc_s = 0.f, ax = 0.f, ay = 0.f, az = 0.f, ex = 0.f;
    const int e_begin = G.row_start[i], e_end = G.row_start[i + 1];
    for (int e0 = e_begin; e0 < e_end; e0 += ECH) {
        const int ne = min(ECH, e_end - e0);
        gen_stage<RP, false>(S, G.edge, e0, ne, R, rc, excl_sigma, excl_power);
        if (f == 0)
            for (int e = 0; e < ne; ++e) ex += S.rep[e];
        if (f < F) {
            for (int e = 0; e < ne; ++e) {
                const int j = S.j[e];
                if (j < 0) continue;
                float wA = 0.f, wB = 0.f, wC = 0.f;
#pragma unroll
                for (int k = 0; k < RP; ++k) {
                    const float r = S.rho[e][k];
                    wA = fmaf(w[0][k], r, wA);
                    wB = fmaf(w[1][k], r, wB);
                    wC = fmaf(w[2][k], r, wC);
                }
                const float *pj = phi + (mN + j) * F3;
                const float *vj = v_in + (mN + j) * 3 * F;
                acc_s = fmaf(pj[F + f], wB, acc_s);
                const float mc = pj[2 * F + f] * wC, ma = pj[f] * wA;
                ax = fmaf(ma, vj[f], fmaf(mc, S.u[e][0], ax));
                ay = fmaf(ma, vj[F + f], fmaf(mc, S.u[e][1], ay));
                az = fmaf(ma, vj[2 * F + f], fmaf(mc, S.u[e][2], az));
            }
        }
        __syncthreads();
    }
    if (f >= F) return;
    const size_t a = mN + i;
    X3[a * 2 * F + f] = s_in[a * F + f] + acc_s;
    v_msg[(a * 3 + 0) * F + f] = v_in[(a * 3 + 0) * F + f] + ax;
    v_msg[(a * 3 + 1) * F + f] = v_in[(a * 3 + 1) * F + f] + ay;
    v_msg[(a * 3 + 2) * F + f] = v_in[(a * 3 + 2) * F + f] + az;
    if (first && m == 0 && f == 0) e_excl[i] = ex;
}

// message block, reverse: one workgroup per (atom c, model), c in its role as SOURCE of the edges (n -> c) of its row.
// Gathers the output adjoints of the neighbors n, accumulates phibar_c and vbar_c without scatter and writes (accumulate = 0)
// or adds dE/dr for the edge (n -> c) at the slot (c, n).  The per-edge sums over the features run as wave sums in a fixed order.
template <int RP>
__global__ void __launch_bounds__(256)
k_gen_edge_bwd(int N, int F, int R, const float *__restrict__ Wimg, long long w_ms, size_t wd_off, size_t bd_off, GraphView G,
               const int *__restrict__ counters, float rc, int excl_vol, float excl_sigma, int excl_power, int accumulate, int layer0,
               const float *__restrict__ v_in, const float *__restrict__ phi, const float *__restrict__ s1bar,
               const float *__restrict__ v1bar, float *__restrict__ phibar, float *__restrict__ vbar_in, float4 *__restrict__ gbar,
               long long gbar_stride) {
    __shared__ GenChunk<RP> S;
    __shared__ float wred[ECH][4][4];
    if (counters[2] || !G.act.atom(blockIdx.x)) return;
    const int c = blockIdx.x, m = blockIdx.y, f = threadIdx.x, wave = f >> 6, lane = f & 63, nw = blockDim.x >> 6;
    const int F3 = 3 * F;
    const bool on = f < F;
    float w[3][RP];
    gen_filter<RP>(Wimg + (size_t)m * w_ms + wd_off, Wimg + (size_t)m * w_ms + bd_off, F, R, f, w);
    const size_t mN = (size_t)m * N, ac = mN + c;
    const float pc_a = on ? phi[ac * F3 + f] : 0.f, pc_b = on ? phi[ac * F3 + F + f] : 0.f, pc_c = on ? phi[ac * F3 + 2 * F + f] : 0.f;
    const float vc0 = on ? v_in[(ac * 3 + 0) * F + f] : 0.f, vc1 = on ? v_in[(ac * 3 + 1) * F + f] : 0.f,
                vc2 = on ? v_in[(ac * 3 + 2) * F + f] : 0.f;
    float accb = 0.f, accc = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
    float4 *gb = gbar + (size_t)m * gbar_stride;
    const int e_begin = G.row_start[c], e_end = G.row_start[c + 1];
    for (int e0 = e_begin; e0 < e_end; e0 += ECH) {
        const int ne = min(ECH, e_end - e0);
        gen_stage<RP, true>(S, G.edge, e0, ne, R, rc, excl_sigma, excl_power);
        for (int e = 0; e < ne; ++e) {
            const int n = S.j[e];   // (uniform across the workgroup)
            if (n < 0) continue;
            float dpart = 0.f, r0 = 0.f, r1 = 0.f, r2 = 0.f;
            if (on) {
                float wA = 0.f, wB = 0.f, wC = 0.f, dA = 0.f, dB = 0.f, dC = 0.f;
#pragma unroll
                for (int k = 0; k < RP; ++k) {
                    const float r = S.rho[e][k], dr = S.drho[e][k];
                    wA = fmaf(w[0][k], r, wA); dA = fmaf(w[0][k], dr, dA);
                    wB = fmaf(w[1][k], r, wB); dB = fmaf(w[1][k], dr, dB);
                    wC = fmaf(w[2][k], r, wC); dC = fmaf(w[2][k], dr, dC);
                }
                const size_t an = mN + n;
                const float sbn = s1bar[an * F + f];
                const float vb0 = v1bar[(an * 3 + 0) * F + f], vb1 = v1bar[(an * 3 + 1) * F + f], vb2 = v1bar[(an * 3 + 2) * F + f];
                const float u0 = -S.u[e][0], u1 = -S.u[e][1], u2 = -S.u[e][2];   // unit vector of (n -> c)
                const float p = fmaf(vb2, u2, fmaf(vb1, u1, vb0 * u0));
                const float qd = fmaf(vb2, vc2, fmaf(vb1, vc1, vb0 * vc0));
                accb = fmaf(wB, sbn, accb);
                accc = fmaf(wC, p, accc);
                ax = fmaf(wA, vb0, ax);
                ay = fmaf(wA, vb1, ay);
                az = fmaf(wA, vb2, az);
                dpart = fmaf(pc_a * qd, dA, fmaf(pc_b * sbn, dB, pc_c * p * dC));
                const float mc = pc_c * wC;
                r0 = mc * vb0; r1 = mc * vb1; r2 = mc * vb2;
            }
            dpart = wave_sum_f32(dpart);
            r0 = wave_sum_f32(r0);
            r1 = wave_sum_f32(r1);
            r2 = wave_sum_f32(r2);
            if (lane == 0) {
                wred[e][0][wave] = dpart; wred[e][1][wave] = r0; wred[e][2][wave] = r1; wred[e][3][wave] = r2;
            }
        }
        __syncthreads();
        if (f < ne && S.j[f] >= 0) {
            float tot[4];
            for (int q = 0; q < 4; ++q) {
                float s = 0.f;
                for (int k = 0; k < nw; ++k) s += wred[f][q][k];
                tot[q] = s;
            }
            const float d = S.u[f][3];
            const float u0 = -S.u[f][0], u1 = -S.u[f][1], u2 = -S.u[f][2];
            float db = tot[0];
            if (layer0 && excl_vol) db -= (float)excl_power * S.rep[f] / d;
            const float dot = fmaf(tot[3], u2, fmaf(tot[2], u1, tot[1] * u0));
            float g0 = fmaf(db, u0, (tot[1] - dot * u0) / d);
            float g1 = fmaf(db, u1, (tot[2] - dot * u1) / d);
            float g2 = fmaf(db, u2, (tot[3] - dot * u2) / d);
            if (accumulate) {
                const float4 old = gb[e0 + f];
                g0 += old.x; g1 += old.y; g2 += old.z;
            }
            gb[e0 + f] = make_float4(g0, g1, g2, 0.f);
        }
        __syncthreads();
    }
    if (!on || !phibar) return;
    phibar[ac * F3 + f] = fmaf(vc2, az, fmaf(vc1, ay, vc0 * ax));
    phibar[ac * F3 + F + f] = accb;
    phibar[ac * F3 + 2 * F + f] = accc;
    vbar_in[(ac * 3 + 0) * F + f] = fmaf(pc_a, ax, v1bar[(ac * 3 + 0) * F + f]);
    vbar_in[(ac * 3 + 1) * F + f] = fmaf(pc_a, ay, v1bar[(ac * 3 + 1) * F + f]);
    vbar_in[(ac * 3 + 2) * F + f] = fmaf(pc_a, az, v1bar[(ac * 3 + 2) * F + f]);
}

// activations of the general path, per model: offsets (floats) inside one arena [M][per_model]... laid out buffer by buffer
struct GenState {
    float *s_in[MAX_LAYERS + 1], *v_in[MAX_LAYERS], *h1[MAX_LAYERS], *phi[MAX_LAYERS], *X3[MAX_LAYERS], *v_msg[MAX_LAYERS],
        *UVv[MAX_LAYERS], *h3[MAX_LAYERS], *q[MAX_LAYERS];
    float *h5, *e_atom;
    float *sbar, *vbar, *s1bar, *v1bar, *qbar, *T, *tmp2, *UVbar, *phibar;
};

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------
int painn_gen_upload(vssr_handle *h, const vssr_painn_config *cfg) {
    const int M = cfg->n_models, L = cfg->num_conv, R = cfg->n_rbf, H = cfg->readout_hidden, NE = cfg->n_embed, F = cfg->feat_dim;
    const size_t F3 = 3 * (size_t)F;
    const size_t per_layer = (size_t)F * F + F + F3 * F + F3 + F3 * R + F3 + 2 * (size_t)F * F + (size_t)F * 2 * F + F + F3 * F + F3;
    const size_t blob_len = (size_t)NE * F + L * per_layer + (size_t)H * F + H + H + 1;
    if (cfg->weights_len != blob_len)
        return set_err(h, VSSR_E_BADARG, "weights_len %llu does not match the layout (%zu floats)",
                       (unsigned long long)cfg->weights_len, blob_len);
    const GenLayout g = gen_layout(F, R, H, NE, L);
    std::vector<float> img(g.len * M, 0.f);
    auto T = [](const float *src, int rows, int cols, float *dst) {   // dst[c][r] = src[r][c]
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) dst[(size_t)c * rows + r] = src[(size_t)r * cols + c];
    };
    for (int m = 0; m < M; ++m) {
        const float *b = cfg->weights[m];
        for (size_t t = 0; t < blob_len; ++t)
            if (!std::isfinite(b[t])) return set_err(h, VSSR_E_BADARG, "model %d: non-finite weight", m);
        float *d = img.data() + (size_t)m * g.len;
        size_t o = 0;
        auto take = [&](size_t n) { const float *r = b + o; o += n; return r; };
        memcpy(d + g.embed, take((size_t)NE * F), sizeof(float) * NE * F);
        for (int l = 0; l < L; ++l) {
            const GenLayer &w = g.layer[l];
            const float *W1 = take((size_t)F * F), *b1 = take(F), *W2 = take(F3 * F), *b2 = take(F3), *Wd = take(F3 * R),
                        *bd = take(F3), *U = take((size_t)F * F), *V = take((size_t)F * F), *W3 = take((size_t)F * 2 * F),
                        *b3 = take(F), *W4 = take(F3 * F), *b4 = take(F3);
            memcpy(d + w.W1, W1, sizeof(float) * F * F); T(W1, F, F, d + w.W1t); memcpy(d + w.b1, b1, sizeof(float) * F);
            memcpy(d + w.W2, W2, sizeof(float) * F3 * F); T(W2, (int)F3, F, d + w.W2t); memcpy(d + w.b2, b2, sizeof(float) * F3);
            memcpy(d + w.Wd, Wd, sizeof(float) * F3 * R); memcpy(d + w.bd, bd, sizeof(float) * F3);
            memcpy(d + w.UV, U, sizeof(float) * F * F);            // [U; V]: [2F][F]
            memcpy(d + w.UV + (size_t)F * F, V, sizeof(float) * F * F);
            for (int k = 0; k < F; ++k)                            // [U^T | V^T]: [F][2F]
                for (int o2 = 0; o2 < F; ++o2) {
                    d[w.UVt + (size_t)k * 2 * F + o2] = U[(size_t)o2 * F + k];
                    d[w.UVt + (size_t)k * 2 * F + F + o2] = V[(size_t)o2 * F + k];
                }
            memcpy(d + w.W3, W3, sizeof(float) * F * 2 * F); T(W3, F, 2 * F, d + w.W3t); memcpy(d + w.b3, b3, sizeof(float) * F);
            memcpy(d + w.W4, W4, sizeof(float) * F3 * F); T(W4, (int)F3, F, d + w.W4t); memcpy(d + w.b4, b4, sizeof(float) * F3);
        }
        const float *W5 = take((size_t)H * F), *b5 = take(H), *w6 = take(H), *b6 = take(1);
        memcpy(d + g.W5, W5, sizeof(float) * H * F); T(W5, H, F, d + g.W5t);
        memcpy(d + g.b5, b5, sizeof(float) * H); memcpy(d + g.w6, w6, sizeof(float) * H); d[g.b6] = b6[0];
    }
    if (h->weights.ensure(img.size() * sizeof(float))) return set_err(h, VSSR_E_NOMEM, "weights: out of device memory");
    VSSR_HIP(h, hipMemcpy(h->weights.p, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    return VSSR_OK;
}

template <int RP>
static void launch_edge_fwd(dim3 grid, dim3 blk, hipStream_t st, int N, int F, int R, const float *W, long long w_ms, const GenLayer &gl,
                            const GraphView &G, const int *counters, const vssr_handle *h, int first, const float *s_in, const float *v_in,
                            const float *phi, float *X3, float *v_msg, float *e_excl) {
    hipLaunchKernelGGL(k_gen_edge_fwd<RP>, grid, blk, 0, st, N, F, R, W, w_ms, gl.Wd, gl.bd, G, counters, h->cutoff, h->excl_sigma,
                       h->excl_power, first, s_in, v_in, phi, X3, v_msg, e_excl);
}
template <int RP>
static void launch_edge_bwd(dim3 grid, dim3 blk, hipStream_t st, int N, int F, int R, const float *W, long long w_ms, const GenLayer &gl,
                            const GraphView &G, const int *counters, const vssr_handle *h, int accumulate, int layer0, const float *v_in,
                            const float *phi, const float *s1bar, const float *v1bar, float *phibar, float *vbar_in, float4 *gbar,
                            long long gbar_stride) {
    hipLaunchKernelGGL(k_gen_edge_bwd<RP>, grid, blk, 0, st, N, F, R, W, w_ms, gl.Wd, gl.bd, G, counters, h->cutoff, h->excl_vol,
                       h->excl_sigma, h->excl_power, accumulate, layer0, v_in, phi, s1bar, v1bar, phibar, vbar_in, gbar, gbar_stride);
}

int painn_gen_run(vssr_handle *h, uint32_t want) {
    const int N = h->n_atoms, M = h->n_models, L = h->num_conv, H = h->readout_hidden, F = h->feat_dim, R = h->n_rbf, NE = h->n_embed;
    const size_t F3 = 3 * (size_t)F;
    hipStream_t st = h->stream;
    h->h_sat_valid = false;
    h->l0_used = false;
    int rc = build_neighbors(h, (double)h->cutoff);
    if (rc) return rc;
    rc = painn_alloc_results(h);
    if (rc) return rc;
    // activation arena: per model and atom 23 F per layer + F (final state) + H (readout) + 1 (energy) + 24 F (reverse scratch)
    const size_t nS = (size_t)M * N * F;
    const size_t floats = (size_t)L * 23 * nS + nS + (size_t)M * N * H + (size_t)M * N + 24 * nS;
    if (h->d_state.ensure(floats * sizeof(float)))
        return set_err(h, VSSR_E_NOMEM, "activation arena (%zu MB): out of device memory", floats * 4 >> 20);
    if (h->d_excl.ensure(sizeof(float) * (size_t)N + 16) || h->d_gbar.ensure(sizeof(float4) * (size_t)M * (size_t)h->slot_cap))
        return set_err(h, VSSR_E_NOMEM, "edge-gradient buffer: out of device memory");
    GenState S{};
    {
        float *p = h->d_state.as<float>();
        auto take = [&](size_t n) { float *r = p; p += n; return r; };
        for (int l = 0; l <= L; ++l) S.s_in[l] = take(nS);
        for (int l = 0; l < L; ++l) {
            S.v_in[l] = take(3 * nS); S.h1[l] = take(nS); S.phi[l] = take(3 * nS); S.X3[l] = take(2 * nS);
            S.v_msg[l] = take(3 * nS); S.UVv[l] = take(6 * nS); S.h3[l] = take(nS); S.q[l] = take(3 * nS);
        }
        S.h5 = take((size_t)M * N * H); S.e_atom = take((size_t)M * N);
        S.sbar = take(nS); S.vbar = take(3 * nS); S.s1bar = take(nS); S.v1bar = take(3 * nS); S.qbar = take(3 * nS);
        S.T = take(nS); S.tmp2 = take(2 * nS); S.UVbar = take(6 * nS); S.phibar = take(3 * nS);
    }
    // what the shared download / finalize code reads
    StateView &sv = h->sv;
    sv.n_atoms = N;
    sv.n_models = M;
    for (int l = 0; l <= MAX_LAYERS; ++l) sv.s_in[l] = l <= L ? S.s_in[l] : nullptr;
    sv.e_atom = S.e_atom;
    sv.e_excl = h->d_excl.as<float>();
    sv.gbar = h->d_gbar.as<float4>();

    const GraphView G = graph_view(h);
    const ActiveView &av = G.act;
    const int *counters = h->d_counters.as<int>();
    const GenLayout gl = gen_layout(F, R, H, NE, L);
    const float *W = h->weights.as<float>();
    const long long w_ms = (long long)gl.len;
    Profiler &P = h->prof;
    const long long sN = (long long)N * F;   // model strides of the s-like / v-like buffers
    const dim3 g_elem((unsigned)(((size_t)N * F + 255) / 256), M), g_edge(N, M), blk_edge(((F + 63) / 64) * 64);

    auto gemm = [&](int rows, int rpa, int K, int Nc, const float *A, long long lda, long long a_ms, int a_swish, size_t b_off, long long ldb,
                    long long bias_off, float *C, long long ldc, long long c_ms, int epi, const float *X, long long ldx, long long x_ms) {
        GemmP p;
        p.rows = rows; p.K = K; p.Nc = Nc; p.rpa = rpa;
        p.A = A; p.lda = lda; p.a_ms = a_ms;
        p.B = W + b_off; p.ldb = ldb; p.b_ms = w_ms;
        p.bias = bias_off >= 0 ? W + bias_off : nullptr;
        p.C = C; p.ldc = ldc; p.c_ms = c_ms;
        p.X = X; p.ldx = ldx; p.x_ms = x_ms;
        p.a_swish = a_swish; p.epi = epi;
        const dim3 grid((unsigned)((rows + GT - 1) / GT), (unsigned)((Nc + GT - 1) / GT), M);
        hipLaunchKernelGGL(k_gen_gemm, grid, dim3(256), 0, st, p, av);
    };
    const int RP = R <= 8 ? 9 : R <= 16 ? 17 : R <= 24 ? 25 : 33;   // R + 1 <= RP
#define GEN_EDGE(FN, ...)                                                                 \
    switch (RP) {                                                                         \
        case 9: FN<9>(__VA_ARGS__); break;                                                \
        case 17: FN<17>(__VA_ARGS__); break;                                              \
        case 25: FN<25>(__VA_ARGS__); break;                                              \
        default: FN<33>(__VA_ARGS__); break;                                              \
    }

    P.begin(KC_EMBED, st);
    hipLaunchKernelGGL(k_gen_embed, g_elem, dim3(256), 0, st, N, F, h->d_Z.as<int>(), W, w_ms, gl.embed, S.s_in[0], S.v_in[0], av);
    P.end(st);
    for (int l = 0; l < L; ++l) {
        const GenLayer &w = gl.layer[l];
        P.begin(KC_MSG_MLP, st);   // h1 = W1 s + b1 ; phi = W2 swish(h1) + b2
        gemm(N, 1, F, F, S.s_in[l], F, sN, 0, w.W1t, F, (long long)w.b1, S.h1[l], F, sN, EPI_STORE, nullptr, 0, 0);
        gemm(N, 1, F, (int)F3, S.h1[l], F, sN, 1, w.W2t, (long long)F3, (long long)w.b2, S.phi[l], (long long)F3, 3 * sN, EPI_STORE,
             nullptr, 0, 0);
        P.end(st);
        P.begin(KC_EDGE_FWD, st);
        GEN_EDGE(launch_edge_fwd, g_edge, blk_edge, st, N, F, R, W, w_ms, w, G, counters, h, (int)(l == 0), S.s_in[l], S.v_in[l], S.phi[l],
                 S.X3[l], S.v_msg[l], h->d_excl.as<float>());
        P.end(st);
        P.begin(KC_UPDATE_FWD, st);   // [U v | V v] ; |V v| ; h3 = W3 [s; |V v|] + b3 ; q = W4 swish(h3) + b4 ; gates
        gemm(3 * N, 3, F, 2 * F, S.v_msg[l], F, 3 * sN, 0, w.UVt, 2 * F, -1, S.UVv[l], 2 * F, 6 * sN, EPI_STORE, nullptr, 0, 0);
        hipLaunchKernelGGL(k_gen_upd_norm, g_elem, dim3(256), 0, st, N, F, S.UVv[l], S.X3[l], av);
        gemm(N, 1, 2 * F, F, S.X3[l], 2 * F, 2 * sN, 0, w.W3t, F, (long long)w.b3, S.h3[l], F, sN, EPI_STORE, nullptr, 0, 0);
        gemm(N, 1, F, (int)F3, S.h3[l], F, sN, 1, w.W4t, (long long)F3, (long long)w.b4, S.q[l], (long long)F3, 3 * sN, EPI_STORE,
             nullptr, 0, 0);
        hipLaunchKernelGGL(k_gen_upd_out, g_elem, dim3(256), 0, st, N, F, S.X3[l], S.v_msg[l], S.UVv[l], S.q[l], S.s_in[l + 1],
                           l + 1 < L ? S.v_in[l + 1] : (float *)nullptr, av);
        P.end(st);
    }
    const bool want_forces = (want & VSSR_WANT_FORCES) != 0;
    P.begin(KC_READOUT, st);   // h5 = W5 s + b5 ; e = w6 . swish(h5) + b6 (+ excluded volume)
    gemm(N, 1, F, H, S.s_in[L], F, sN, 0, gl.W5t, H, (long long)gl.b5, S.h5, H, (long long)N * H, EPI_STORE, nullptr, 0, 0);
    hipLaunchKernelGGL(k_gen_readout, dim3((N + 255) / 256, M), dim3(256), 0, st, N, H, W, w_ms, gl.w6, gl.b6, S.h5,
                       h->excl_vol ? (const float *)h->d_excl.as<float>() : (const float *)nullptr, S.e_atom, (int)want_forces, av);
    P.end(st);

    if (want_forces) {
        P.begin(KC_UPDATE_BWD, st);   // sbar = W5^T (w6 swish'(h5)) ; vbar = 0
        gemm(N, 1, H, F, S.h5, H, (long long)N * H, 0, gl.W5, F, -1, S.sbar, F, sN, EPI_STORE, nullptr, 0, 0);
        VSSR_HIP(h, hipMemsetAsync(S.vbar, 0, sizeof(float) * 3 * nS, st));
        P.end(st);
        for (int l = L - 1; l >= 0; --l) {
            const GenLayer &w = gl.layer[l];
            P.begin(KC_UPDATE_BWD, st);
            hipLaunchKernelGGL(k_gen_upd_bwd1, g_elem, dim3(256), 0, st, N, F, S.UVv[l], S.q[l], S.sbar, S.vbar, S.qbar, S.UVbar, av);
            // T = (W4^T qbar) * swish'(h3) ; tmp2 = W3^T T ([s part | norm part])
            gemm(N, 1, (int)F3, F, S.qbar, (long long)F3, 3 * sN, 0, w.W4, F, -1, S.T, F, sN, EPI_DSWISH, S.h3[l], F, sN);
            gemm(N, 1, F, 2 * F, S.T, F, sN, 0, w.W3, 2 * F, -1, S.tmp2, 2 * F, 2 * sN, EPI_STORE, nullptr, 0, 0);
            hipLaunchKernelGGL(k_gen_upd_bwd2, g_elem, dim3(256), 0, st, N, F, S.UVv[l], S.X3[l], S.tmp2, S.sbar, S.s1bar, S.UVbar, av);
            // v1bar = vbar + [U v-bar | V v-bar] [U; V]
            gemm(3 * N, 3, 2 * F, F, S.UVbar, 2 * F, 6 * sN, 0, w.UV, F, -1, S.v1bar, F, 3 * sN, EPI_ADD, S.vbar, F, 3 * sN);
            P.end(st);
            P.begin(KC_EDGE_BWD, st);   // phibar, vbar (adjoint of v_in[l]) and the edge gradients
            GEN_EDGE(launch_edge_bwd, g_edge, blk_edge, st, N, F, R, W, w_ms, w, G, counters, h, (int)(l != L - 1), (int)(l == 0), S.v_in[l],
                     S.phi[l], S.s1bar, S.v1bar, l > 0 ? S.phibar : (float *)nullptr, S.vbar, sv.gbar, (long long)h->slot_cap);
            P.end(st);
            if (l > 0) {   // sbar (adjoint of s_in[l]) = s1bar + W1^T ((W2^T phibar) * swish'(h1))
                P.begin(KC_MSG_MLP_BWD, st);
                gemm(N, 1, (int)F3, F, S.phibar, (long long)F3, 3 * sN, 0, w.W2, F, -1, S.T, F, sN, EPI_DSWISH, S.h1[l], F, sN);
                gemm(N, 1, F, F, S.T, F, sN, 0, w.W1, F, -1, S.sbar, F, sN, EPI_ADD, S.s1bar, F, sN);
                P.end(st);
            }
        }
    }
#undef GEN_EDGE
    P.begin(KC_FINALIZE, st);
    painn_finalize(h, G, want);
    P.end(st);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
