// ewald.hip — the reciprocal-space part of an Ewald sum (LAMMPS kspace_style ewald with pair_style */coul/long, units metal) for pair
// handles created by vssr_pair_create_kspace, fp64, batched over independent chains.  pair_run launches these after the site kernel,
// whose coul/long terms are the real-space part qqrd2e q_a q_b erfc(g r) / r.
//
//   E_k    = sum_{k != 0, |k| <= k_cut} u(k) |S(k)|^2,  u(k) = qqrd2e (2 pi / V) exp(-k^2 / 4 g^2) / k^2,  S(k) = sum_j q_j exp(i k.r_j)
//   E_self = -qqrd2e g / sqrt(pi) sum q_i^2,            E_bg = -qqrd2e pi Q^2 / (2 g^2 V)   (neutralising background, Q = sum q_i)
//   F_i    = q_i sum_k 2 u(k) k [sin(k.r_i) Re S(k) - cos(k.r_i) Im S(k)]
//   e_i    = q_i sum_k u(k) Re(exp(-i k.r_i) S(k)) - qqrd2e g q_i^2 / sqrt(pi) - qqrd2e pi q_i Q / (2 g^2 V)      (pe/atom of LAMMPS ewald)
//
// Three kernels over the half box of ewald_dev.h, no atomics, every sum in an order fixed by the chain's own cell and atom order, so a
// chain's bits depend neither on the rest of the batch nor on the run:
//   k_ewald_sk      one workgroup per (chain, 256 k cells), one cell per thread.  Atoms in tiles; per tile the phase factors
//                   exp(2 pi i m s_a), m = 0 .. m_a, of the three axes go to LDS (sincospi of the exact argument, no recurrence),
//                   a thread sums q_j e_x[h] e_y[k] e_z[l] over the tile and writes 2 u(k) S(k) (zeros outside the half sphere).
//   k_ewald_atoms   one wave per (chain, 64 atoms), one atom per lane.  The chain's 2 u S is staged through LDS 256 cells at a time; a
//                   lane walks the cells in order, takes the phase at the start of every l row from sincospi and steps along the row
//                   with exp(2 pi i s_z) (at most 126 complex products: ~1e-14 relative), and adds e_i and F_i to its own entries of
//                   d_pot_ea / d_pot_f (read-add-store; analytic_end reduces afterwards).
//   k_ewald_virial  one workgroup per chain: dE_k / d eps_ab = sum_k u |S|^2 [2 k_a k_b (1 / k^2 + 1 / 4 g^2) - delta_ab] and
//                   dE_bg / d eps_ab = -E_bg delta_ab, divided by V and added to what k_slot_stress stored.
//
// A slab handle (vssr_pair_create_kspace_slab: kspace_modify slab F under boundary p p f; Yeh & Berkowitz 1999, Ballenegger, Arnold &
// Cerda 2009 for Q != 0) runs the <true> instantiations of the same kernels.  All of the above is taken on the extended cell
// (a, b, F c) of ewald_geom, V = V' = F |det cell| included, and with n = a x b / |a x b|, z_i = r_i . n (the open axis is never
// wrapped), L' = F |c . n|, Q = sum q, M = sum q z, R2 = sum q z^2:
//   E_slab = qqrd2e (2 pi / V') (M^2 - Q R2 - Q^2 L'^2 / 12)
//   e_i   += qqrd2e (2 pi / V') q_i (z_i M - (R2 + Q z_i^2) / 2 - Q L'^2 / 12),      F_i += -qqrd2e (4 pi / V') q_i (M - Q z_i) n
//   dE_slab / d eps = E_slab (-1, -1, +1, 0, 0, 0)   (n along z: vssr_batch_upload refuses any other slab cell)
// The thread of k_ewald_sk that holds the cell (0, 0, 0) sums Q already; it sums M and R2 beside it, over the tiles in atom order,
// and stores the three behind the chain's k cells.  k_ewald_virial divides a slab chain's sums by the real volume V' / F.
#include "ewald_dev.h"
#include "pair_dev.h"
#include "virial_dev.h"

namespace vssr {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// idx -> (h, k, l) of the half box
__device__ __forceinline__ void ew_decode(int idx, const int m[3], int &h, int &k, int &l) {
    const int nl = 2 * m[2] + 1, nk = 2 * m[1] + 1;
    l = idx % nl - m[2];
    const int row = idx / nl;
    k = row % nk - m[1];
    h = row / nk;
}

// unit normal of the slab and the extended length along it, from the third reciprocal row: r[2] = a x b / det.  For a left-handed
// cell (det < 0) this n is -a x b / |a x b|; E_slab, e_i, F_i and the virial do not change under n -> -n (z_i and M change sign
// together, M^2, z_i M, z_i^2, R2 and (M - Q z_i) n do not), so the sign is left as it comes.
__device__ __forceinline__ void slab_axis(const EwaldGeom &G, double n[3], double &len) {
    const double inv = sqrt(G.r[2][0] * G.r[2][0] + G.r[2][1] * G.r[2][1] + G.r[2][2] * G.r[2][2]);
    for (int x = 0; x < 3; ++x) n[x] = G.r[2][x] / inv;
    len = 1.0 / inv;
}

template <bool SLAB>
__device__ __forceinline__ void sk_chain(int b, int c0, const EwaldParams &P, const int *__restrict__ cfg_start, const int *__restrict__ type,
                                         const double *__restrict__ cell, const double *__restrict__ wpos, int stride,
                                         double2 *__restrict__ S, double2 *tab, double *qs, double *zs) {
    EwaldGeom G;
    ewald_geom(cell + 9 * (size_t)b, P.k_cut, 0.0, G, SLAB ? P.slab : 0.0);
    // (uniform.  The second never holds while vssr_batch_upload is the only writer of d_cell and ew_stride: it sized the stride from
    // bounds >= these.  Should it ever hold, nothing is written here and k_ewald_atoms / k_ewald_virial store NaN: no silent result)
    if (c0 >= G.cells || G.cells > stride) return;
    const int tid = threadIdx.x, idx = c0 + tid;
    const bool valid = idx < G.cells;
    int h = 0, k = 0, l = 0;
    if (valid) ew_decode(idx, G.m, h, k, l);
    const int ne = G.m[0] + G.m[1] + G.m[2] + 3, offy = G.m[0] + 1, offz = offy + G.m[1] + 1;
    const int TA = min(EW_TILE_MAX, EW_TAB / ne);
    const int ak = k < 0 ? -k : k, al = l < 0 ? -l : l;
    double sre = 0.0, sim = 0.0;
    const bool origin = valid && h == 0 && k == 0 && l == 0;
    double nz[3] = {0.0, 0.0, 0.0}, zlen = 0.0, mom1 = 0.0, mom2 = 0.0;
    if (SLAB) slab_axis(G, nz, zlen);
    for (int a0 = cfg_start[b], a1 = cfg_start[b + 1]; a0 < a1; a0 += TA) {
        const int na = min(TA, a1 - a0);
        __syncthreads();
        for (int t = tid; t < ne * TA; t += EW_KBLOCK) {
            const int row = t / TA, a = t % TA;
            if (a >= na) continue;
            const int axis = row >= offz ? 2 : row >= offy ? 1 : 0, m = row - (axis == 2 ? offz : axis == 1 ? offy : 0);
            const double *x = wpos + 3 * (size_t)(a0 + a);
            // (selects, not G.r[axis]: a dynamically indexed array would live in scratch)
            const double r0 = axis == 2 ? G.r[2][0] : axis == 1 ? G.r[1][0] : G.r[0][0], r1 = axis == 2 ? G.r[2][1] : axis == 1 ? G.r[1][1] : G.r[0][1],
                         r2 = axis == 2 ? G.r[2][2] : axis == 1 ? G.r[1][2] : G.r[0][2];
            const double s = x[0] * r0 + x[1] * r1 + x[2] * r2;
            double sn, cs;
            sincospi(2.0 * (m * s), &sn, &cs);
            tab[t] = make_double2(cs, sn);
        }
        if (tid < na) qs[tid] = P.q[type[a0 + tid]];
        if (SLAB && tid < na) {
            const double *x = wpos + 3 * (size_t)(a0 + tid);
            zs[tid] = x[0] * nz[0] + x[1] * nz[1] + x[2] * nz[2];
        }
        __syncthreads();
        if (valid)
            for (int a = 0; a < na; ++a) {
                const double2 ex = tab[h * TA + a];
                double2 ey = tab[(offy + ak) * TA + a], ez = tab[(offz + al) * TA + a];
                if (k < 0) ey.y = -ey.y;
                if (l < 0) ez.y = -ez.y;
                const double2 p = cmul(cmul(ex, ey), ez);
                sre += qs[a] * p.x;
                sim += qs[a] * p.y;
            }
        if (SLAB && origin)
            for (int a = 0; a < na; ++a) {
                mom1 += qs[a] * zs[a];
                mom2 += qs[a] * (zs[a] * zs[a]);
            }
    }
    if (!valid) return;
    double2 *Sb = S + (size_t)b * (stride + EW_EXTRA);
    const double kx = h * G.b[0][0] + k * G.b[1][0] + l * G.b[2][0], ky = h * G.b[0][1] + k * G.b[1][1] + l * G.b[2][1],
                 kz = h * G.b[0][2] + k * G.b[1][2] + l * G.b[2][2];
    const double k2 = kx * kx + ky * ky + kz * kz;
    const bool half = h > 0 || (h == 0 && (k > 0 || (k == 0 && l > 0)));
    double2 out = make_double2(0.0, 0.0);
    if (half && k2 <= P.k_cut * P.k_cut) {
        const double u2 = 2.0 * PAIR_QQRD2E * (EW_2PI / G.vol) * exp(-k2 / (4.0 * P.g * P.g)) / k2;
        out = make_double2(u2 * sre, u2 * sim);
    }
    Sb[idx] = out;
    if (origin) {   // S(0) = Q, the chain's total charge (phases are exactly 1); a slab handle: M and R2 beside it
        Sb[stride] = make_double2(sre, mom1);
        if (SLAB) Sb[stride + 1] = make_double2(mom2, 0.0);
    }
}

template <bool SLAB>
__global__ void __launch_bounds__(EW_KBLOCK)
k_ewald_sk(PotView V, EwaldParams P, int stride, double2 *__restrict__ S) {
    __shared__ double2 tab[EW_TAB];
    __shared__ double qs[EW_TILE_MAX];
    __shared__ double zs[SLAB ? EW_TILE_MAX : 1];
    if (V.counters[2]) return;   // (uniform)
    const int b = blockIdx.x;
    if (!V.act.chain(b)) return;
    sk_chain<SLAB>(b, blockIdx.y * EW_KBLOCK, P, V.cfg_start, V.type, V.cell, V.wpos, stride, S, tab, qs, zs);
}

template <bool SLAB>
__device__ __forceinline__ void atoms_chain(int b, int tile, const EwaldParams &P, const int *__restrict__ cfg_start,
                                            const int *__restrict__ type, const double *__restrict__ cell,
                                            const double *__restrict__ wpos, int stride, const double2 *__restrict__ S,
                                            double *__restrict__ e_atom, double *__restrict__ forces, double2 *sh) {
    const int a1 = cfg_start[b + 1], i0 = cfg_start[b] + tile * EW_ATOMS;
    if (i0 >= a1) return;   // (uniform)
    EwaldGeom G;
    ewald_geom(cell + 9 * (size_t)b, P.k_cut, 0.0, G, SLAB ? P.slab : 0.0);
    const int tid = threadIdx.x, i = i0 + tid, cells = (int)G.cells;
    const bool mine = i < a1;
    if (G.cells > stride) {   // (uniform; never: see sk_chain) the chain has no S(k): its results must not pass for numbers
        if (mine) {
            e_atom[i] = __longlong_as_double(0x7ff8000000000000LL);
            for (int x = 0; x < 3; ++x) forces[3 * (size_t)i + x] = __longlong_as_double(0x7ff8000000000000LL);
        }
        return;
    }
    double s[3] = {0.0, 0.0, 0.0}, qi = 0.0;
    if (mine) {
        const double *x = wpos + 3 * (size_t)i;
        for (int a = 0; a < 3; ++a) s[a] = x[0] * G.r[a][0] + x[1] * G.r[a][1] + x[2] * G.r[a][2];
        qi = P.q[type[i]];
    }
    double sn, cs;
    sincospi(2.0 * s[2], &sn, &cs);
    const double2 ez1 = make_double2(cs, sn);
    const double2 *Sb = S + (size_t)b * (stride + EW_EXTRA);
    int h = 0, k = -G.m[1], l = -G.m[2];
    double2 ph = make_double2(1.0, 0.0);
    double e = 0.0, fh = 0.0, fk = 0.0, fl = 0.0;
#pragma unroll 1
    for (int c0 = 0; c0 < cells; c0 += EW_KBLOCK) {
        __syncthreads();
        for (int t = tid; t < EW_KBLOCK; t += EW_ATOMS) sh[t] = c0 + t < cells ? Sb[c0 + t] : make_double2(0.0, 0.0);
        __syncthreads();
        const int n = min(EW_KBLOCK, cells - c0);
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
            if (l == -G.m[2]) {   // (uniform) a new l row: the phase from its exact argument
                sincospi(2.0 * (h * s[0] + k * s[1] - G.m[2] * s[2]), &sn, &cs);
                ph = make_double2(cs, sn);
            }
            const double2 w = sh[j];
            if (w.x != 0.0 || w.y != 0.0) {   // (uniform)
                const double t = ph.y * w.x - ph.x * w.y;
                e += ph.x * w.x + ph.y * w.y;
                fh += h * t; fk += k * t; fl += l * t;
            }
            ph = cmul(ph, ez1);
            if (++l > G.m[2]) {
                l = -G.m[2];
                if (++k > G.m[1]) { k = -G.m[1]; ++h; }
            }
        }
    }
    if (!mine) return;
    const double Q = Sb[stride].x;
    e_atom[i] += qi * e - PAIR_QQRD2E * P.g * qi * qi / EW_SQRTPI - PAIR_QQRD2E * (0.5 * EW_2PI) * qi * Q / (2.0 * P.g * P.g * G.vol);
    for (int x = 0; x < 3; ++x) forces[3 * (size_t)i + x] += 2.0 * qi * (fh * G.b[0][x] + fk * G.b[1][x] + fl * G.b[2][x]);
    if (SLAB) {   // the dipole correction from the chain's moments
        double nz[3], zlen;
        slab_axis(G, nz, zlen);
        const double *x = wpos + 3 * (size_t)i;
        const double z = x[0] * nz[0] + x[1] * nz[1] + x[2] * nz[2];
        const double M = Sb[stride].y, R2 = Sb[stride + 1].x, c = PAIR_QQRD2E * (EW_2PI / G.vol);
        e_atom[i] += c * qi * (z * M - 0.5 * (R2 + Q * (z * z)) - Q * (zlen * zlen) / 12.0);
        const double fz = -2.0 * c * qi * (M - Q * z);
        for (int a = 0; a < 3; ++a) forces[3 * (size_t)i + a] += fz * nz[a];
    }
}

template <bool SLAB>
__global__ void __launch_bounds__(EW_ATOMS)
k_ewald_atoms(PotView V, EwaldParams P, int stride, const double2 *__restrict__ S, double *__restrict__ e_atom, double *__restrict__ forces) {
    __shared__ double2 sh[EW_KBLOCK];
    if (V.counters[2]) return;   // (uniform)
    const int b = blockIdx.x;
    if (!V.act.chain(b)) return;
    atoms_chain<SLAB>(b, blockIdx.y, P, V.cfg_start, V.type, V.cell, V.wpos, stride, S, e_atom, forces, sh);
}

template <bool SLAB>
__global__ void __launch_bounds__(VIR_THREADS)
k_ewald_virial(PotView V, EwaldParams P, int stride, const double2 *__restrict__ S, double *__restrict__ stress) {
    __shared__ double red[6][VIR_THREADS];
    if (V.counters[2]) return;   // (uniform)
    const int b = blockIdx.x, tid = threadIdx.x;
    EwaldGeom G;
    ewald_geom(V.cell + 9 * (size_t)b, P.k_cut, 0.0, G, SLAB ? P.slab : 0.0);
    const double2 *Sb = S + (size_t)b * (stride + EW_EXTRA);
    double w[6] = {0, 0, 0, 0, 0, 0};
    const bool lost = G.cells > stride;   // (never: see sk_chain) then the stress is NaN
    const int cells = lost ? 0 : (int)G.cells;
    for (int idx = tid; idx < cells; idx += VIR_THREADS) {
        const double2 s = Sb[idx];
        if (s.x == 0.0 && s.y == 0.0) continue;
        int h, k, l;
        ew_decode(idx, G.m, h, k, l);
        const double kx = h * G.b[0][0] + k * G.b[1][0] + l * G.b[2][0], ky = h * G.b[0][1] + k * G.b[1][1] + l * G.b[2][1],
                     kz = h * G.b[0][2] + k * G.b[1][2] + l * G.b[2][2];
        const double k2 = kx * kx + ky * ky + kz * kz;
        const double u2 = 2.0 * PAIR_QQRD2E * (EW_2PI / G.vol) * exp(-k2 / (4.0 * P.g * P.g)) / k2;
        const double ek = (s.x * s.x + s.y * s.y) / u2;   // 2 u |S|^2: this vector and its mirror image
        const double c = 2.0 * (1.0 / k2 + 1.0 / (4.0 * P.g * P.g));
        w[0] += ek * (c * kx * kx - 1.0);
        w[1] += ek * (c * ky * ky - 1.0);
        w[2] += ek * (c * kz * kz - 1.0);
        w[3] += ek * c * ky * kz;
        w[4] += ek * c * kx * kz;
        w[5] += ek * c * kx * ky;
    }
    for (int k = 0; k < 6; ++k) red[k][tid] = w[k];
    __syncthreads();
    for (int s = VIR_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 6; ++k) red[k][tid] += red[k][tid + s];
        __syncthreads();
    }
    if (tid < 6) {
        const double Q = Sb[stride].x;
        const double ebg = -PAIR_QQRD2E * (0.5 * EW_2PI) * Q * Q / (2.0 * P.g * P.g * G.vol);
        double sum = red[tid][0] - (tid < 3 ? ebg : 0.0), vol = G.vol;
        if (SLAB) {   // dE_slab / d eps = E_slab (-1, -1, +1, 0, 0, 0); the stress is per real volume V' / F
            double nz[3], zlen;
            slab_axis(G, nz, zlen);
            const double M = Sb[stride].y, R2 = Sb[stride + 1].x;
            const double eslab = PAIR_QQRD2E * (EW_2PI / G.vol) * (M * M - Q * R2 - Q * Q * (zlen * zlen) / 12.0);
            if (tid < 3) sum += tid == 2 ? eslab : -eslab;
            vol = G.vol / P.slab;
        }
        stress[6 * (size_t)b + tid] += lost ? __longlong_as_double(0x7ff8000000000000LL) : sum / vol;
    }
}

static EwaldParams ewald_params(const vssr_handle *h) {
    EwaldParams P;
    P.g = h->ew_g;
    P.k_cut = h->ew_kcut;
    P.slab = h->ew_slab;
    for (int t = 0; t < 8; ++t) P.q[t] = h->ew_q[t];
    return P;
}

static void launch_sk(vssr_handle *h, const PotView &V, const EwaldParams &P) {
    const int blocks = (h->ew_stride + EW_KBLOCK - 1) / EW_KBLOCK;
    const auto kern = h->ew_slab > 0 ? k_ewald_sk<true> : k_ewald_sk<false>;   // (a slab handle: the dipole moments beside S(0))
    hipLaunchKernelGGL(kern, dim3(V.n_cfg, blocks), dim3(EW_KBLOCK), 0, h->stream, V, P, h->ew_stride, h->d_ew_S.as<double2>());
}

// after the site kernel of pair_run: e_i and F_i of the reciprocal, self and background terms (a slab handle: and the dipole
// correction) on top of what it stored
void ewald_run(vssr_handle *h, const PotView &V) {
    const EwaldParams P = ewald_params(h);
    launch_sk(h, V, P);
    const auto kern = h->ew_slab > 0 ? k_ewald_atoms<true> : k_ewald_atoms<false>;
    hipLaunchKernelGGL(kern, dim3(V.n_cfg, (h->max_cfg_atoms + EW_ATOMS - 1) / EW_ATOMS), dim3(EW_ATOMS), 0, h->stream, V, P,
                       h->ew_stride, h->d_ew_S.as<double2>(), h->d_pot_ea.as<double>(), h->d_pot_f.as<double>());
}

// after slot_stress: the reciprocal and background virials on top of d_stress (S(k) rebuilt from the resident positions)
int ewald_stress(vssr_handle *h) {
    const PotView V = pot_view(h);
    const EwaldParams P = ewald_params(h);
    launch_sk(h, V, P);
    const auto kern = h->ew_slab > 0 ? k_ewald_virial<true> : k_ewald_virial<false>;
    hipLaunchKernelGGL(kern, dim3(V.n_cfg), dim3(VIR_THREADS), 0, h->stream, V, P, h->ew_stride, h->d_ew_S.as<double2>(),
                       h->d_stress.as<double>());
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
