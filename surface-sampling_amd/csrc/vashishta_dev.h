// vashishta_dev.h — device bodies of the Vashishta kernels (vashishta.hip): the pair term, the radial factor of the three-body term,
// the site tile (long pair row + short three-body row compacted into LDS) and its long form, the gather.  Semantics: LAMMPS
// pair_style vashishta, units metal (see vashishta.hip).
#ifndef VSSR_VASHISHTA_DEV_H
#define VSSR_VASHISHTA_DEV_H
#include "pair_dev.h"

namespace vssr {

// One entry (i, j, k) as the kernels read it (128 bytes), derived on the host at vssr_vashishta_create from the file's columns
// (H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta):
//   two-body term and radial factor, read from entry (i, j, j): H, eta, zz = qqr2e Zi Zj, il1 = 1 / lambda1, D, il4 = 1 / lambda4,
//     W, rc, vrc = V(rc), dvrc = V'(rc), gamma, r0   (il1 / il4 = 0 where the term is absent: zz == 0 / D == 0)
//   three-body term, read from entry (i, j, k): B, C, c0 = costheta
struct VashPairP { double H, eta, zz, il1, D, il4, W, rc, vrc, dvrc, gamma, r0; };
struct VashTri { double B, C, c0; };
struct VashP {
    VashPairP two;
    VashTri tri;
    double pad;
};

constexpr int VA_MAXD = 16, VA_CENTRES = PAIR_CENTRES, VA_LANES = PAIR_LANES;   // short slots per centre in LDS; the launch shape of k_pair_site
constexpr int VA_MAXT = 8;   // species

// r^-eta from ir = 1 / r.  Published sets have integer eta (7, 9): then by squaring, else pow().  ONE function for every caller,
// host (V(rc), V'(rc) at create) and device.
__host__ __device__ __forceinline__ double vash_rpow(double r, double ir, double eta) {
    const int n = (int)eta;
    if ((double)n != eta || n < 1 || n > 64) return pow(r, -eta);
    double acc = 1.0, b = ir;
    for (int k = n; k; k >>= 1) {
        if (k & 1) acc *= b;
        b *= b;
    }
    return acc;
}
// V(r) = H / r^eta + zz / r exp(-r / lambda1) - D / r^4 exp(-r / lambda4) - W / r^6 and V'(r)
__host__ __device__ __forceinline__ void vash_v(const VashPairP &p, double r, double &v, double &dv) {
    const double ir = 1.0 / r, i2 = ir * ir, i4 = i2 * i2, i6 = i4 * i2;
    const double hr = p.H * vash_rpow(r, ir, p.eta);
    v = hr - p.W * i6;
    dv = (-p.eta * hr + 6.0 * p.W * i6) * ir;
    if (p.zz != 0.0) {
        const double c = p.zz * ir * exp(-r * p.il1);
        v += c;
        dv -= c * (ir + p.il1);
    }
    if (p.D != 0.0) {
        const double d = p.D * i4 * exp(-r * p.il4);
        v -= d;
        dv += d * (4.0 * ir + p.il4);
    }
}
// phi2(r) = V(r) - V(rc) - (r - rc) V'(rc) and its derivative at r < rc (the caller has tested the cutoff).  ONE expression for the
// energy launch, the gradient launch and both forms of the site kernel.
__device__ __forceinline__ void vash_pair(const VashPairP &p, double r, double &e, double &de) {
    double v, dv;
    vash_v(p, r, v, dv);
    e = v - p.vrc - (r - p.rc) * p.dvrc;
    de = dv - p.dvrc;
}
// Radial factor of the three-body term with entry (i, j, j): f = exp(gamma / (r - r0)) for r < r0, else 0; and d ln f / dr.  ONE
// expression each for the tile form (f read from LDS) and the long form (f recomputed): the same bits either way.
__device__ __forceinline__ double vash_f(const VashPairP &p, double r) {
    if (!(r < p.r0)) return 0.0;
    return exp(p.gamma * (1.0 / (r - p.r0)));
}
__device__ __forceinline__ double vash_dlf(const VashPairP &p, double r) {
    const double x = 1.0 / (r - p.r0);
    return -p.gamma * x * x;
}

// Sums of short slot n over the other short slots m of its centre, h(dc) = dc^2 / (1 + C dc^2), dc = cs - c0_nm:
//   T = sum_m B_nm f_m h,   S = sum_m B_nm f_m h' (u_m - cs u_n),   h' = 2 dc / (1 + C dc^2)^2.
// With them phi3 summed over the pairs {n, m} is f_n T and its gradient with respect to r_n is f_n (S / r_n + dlf_n T u_n)
// (the sw_term / sw_finish structure with the extra 1 / (1 + C dc^2)).
struct VashAcc { double T, sx, sy, sz; };
__device__ __forceinline__ void vash_term(VashAcc &a, double ux, double uy, double uz, double vx, double vy, double vz, double fm,
                                          const VashTri &t) {
    const double cs = ux * vx + uy * vy + uz * vz;
    const double dc = cs - t.c0, q = 1.0 / (1.0 + t.C * dc * dc), w = t.B * fm;
    a.T += w * dc * dc * q;
    const double g = 2.0 * w * dc * q * q;
    a.sx += g * (vx - cs * ux);
    a.sy += g * (vy - cs * uy);
    a.sz += g * (vz - cs * uz);
}
// Short slot n complete: e3 = f_n T (twice the slot's part of the centre's three-body energy) and G3_n = dE3_i / d r_n.  pe/atom of
// LAMMPS (ev_tally3, thirds): the centre takes e3 / 6 (its third, split over the two slots of every pair), the neighbor e3 / 3.
__device__ __forceinline__ void vash_finish(const VashAcc &a, double ux, double uy, double uz, double r, double f, double dlf, double &e3,
                                            double &gx, double &gy, double &gz) {
    e3 = f * a.T;
    const double pa = f / r, su = f * dlf * a.T;
    gx = pa * a.sx + su * ux;
    gy = pa * a.sy + su * uy;
    gz = pa * a.sz + su * uz;
}

struct VashShared {   // the short rows: 46 080 bytes
    double ux[VA_MAXD][VA_CENTRES], uy[VA_MAXD][VA_CENTRES], uz[VA_MAXD][VA_CENTRES], r[VA_MAXD][VA_CENTRES], f[VA_MAXD][VA_CENTRES];
    int idx[VA_MAXD][VA_CENTRES];           // slot of the short entry within the centre's row
    signed char tp[VA_MAXD][VA_CENTRES];
};
// The tables, in the dynamic LDS of the launch, sized by the species in use: {B, C, costheta} of every entry (i, j, k), then the pair /
// radial columns of every entry (i, j, j).  2 species: 576 B, 3: 1 512 B (3 workgroups per CU with the short rows); 8: 18 432 B (2).
struct VashTables {
    VashTri *tri;
    VashPairP *two;
    static size_t bytes(int nt) { return sizeof(VashTri) * nt * nt * nt + sizeof(VashPairP) * nt * nt; }
    __device__ static VashTables in(unsigned char *lds, int nt) {
        return {reinterpret_cast<VashTri *>(lds), reinterpret_cast<VashPairP *>(lds + sizeof(VashTri) * nt * nt * nt)};
    }
};

// d_gbar of a Vashishta handle: ej3 [slots] | G [slots][3] | per atom: number of short slots, then the first VA_MAXD of them (ints).
// A plain evaluation writes ej3 and G at short slots only (r < r0max), 32 of the 32 bytes allocated per slot; the gradient launch
// of vssr_batch_stress writes G of every slot.
constexpr int VA_ATOM_INTS = VA_MAXD + 2;
struct VashSlots {
    double *ej3, *gslot;
    int *sidx;
    static size_t doubles(const vssr_handle *h) { return 4 * (size_t)h->slot_cap + (size_t)(VA_ATOM_INTS / 2) * (size_t)h->n_atoms; }
    static VashSlots of(const vssr_handle *h) {
        double *p = h->d_gbar.as<double>();
        return {p, p + h->slot_cap, reinterpret_cast<int *>(p + 4 * (size_t)h->slot_cap)};
    }
};

// One tile of VA_CENTRES centres, VA_LANES lanes each: thread tid serves centre i = (tile's first atom) + (tid >> 2) with lane
// q = tid & 3; `mine`: the centre exists and is evaluated; tb: the tables' place in LDS (filled here).  Every thread of the workgroup
// calls this (two barriers inside).
//   Phase 1: the lanes stride the row four slots at a time.  Every slot with r < rc(i, j) adds the centre's half pair energy and its
//   full pair force (GRAD: its half pair gradient goes to gslot unless the slot is short).  Slots with r < r0max are appended, in slot
//   order (a ballot over the quad gives each lane its place), to the centre's short row in LDS.
//   Phase 2: lane q takes the short entries q, q + 4, ... and computes G3_n = dE3_i / d r_n in one walk over the other short entries.
//   A centre with more than VA_MAXD short slots takes the long form: the same lanes recompute every short neighbor's values from
//   global memory with the same expressions, in the same order.
// Every ej3 / G slot, e_atom and force is written by exactly one lane.
template <bool GRAD>
__device__ __forceinline__ void vash_site_tile(VashShared &sh, const VashTables tb, int i, bool mine, int nt, double r0max,
                                               const VashP *__restrict__ P, const int *__restrict__ type, const int *__restrict__ atom_cfg,
                                               const double *__restrict__ cell, const double *__restrict__ wpos,
                                               const int *__restrict__ row_start, const float4 *__restrict__ edge,
                                               const int *__restrict__ edge_S, double *__restrict__ e_atom, double *__restrict__ forces,
                                               double *__restrict__ ej3, double *__restrict__ gslot, int *__restrict__ sidx) {
    const int tid = threadIdx.x, cb = tid >> 2, q = tid & (VA_LANES - 1);
    for (int t = tid; t < nt * nt * nt; t += VA_CENTRES * VA_LANES) tb.tri[t] = P[t].tri;
    for (int t = tid; t < nt * nt; t += VA_CENTRES * VA_LANES) tb.two[t] = P[(t * nt) + (t % nt)].two;   // entry (a, b, b), t = a nt + b
    __syncthreads();
    int e0 = 0, deg = 0, ti = 0;
    const double *C = cell;
    if (mine) {
        e0 = row_start[i];
        deg = row_start[i + 1] - e0;
        ti = type[i];
        C = cell + 9 * atom_cfg[i];
    }
    double es = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
    int cnt = 0;   // short slots of the centre so far: the same number in the four lanes of the quad
    const int quad_shift = (tid & 63) & ~(VA_LANES - 1);
    // ---- phase 1: the pair row; the short row -> LDS ---------------------------------------------------------------------------
#pragma unroll 1
    for (int base = 0; base < deg; base += VA_LANES) {   // (deg is the same in the four lanes of a quad: they leave together)
        const int n = base + q;
        bool is_short = false;
        double u[3] = {0.0, 0.0, 0.0}, r = 1.0, f = 0.0;
        int tn = 0;
        if (n < deg) {
            const int j = __float_as_int(edge[e0 + n].w);
            if (j >= 0) {   // (else a padding slot: k_slot_stress skips it as well)
                double rv[3];
                edge_vec(wpos, C, i, j, edge_S[e0 + n], rv);
                r = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
                tn = type[j];
                const VashPairP &p = tb.two[ti * nt + tn];
                double e = 0.0, de = 0.0;
                if (r < p.rc) vash_pair(p, r, e, de);
                const double w = de / r;
                is_short = r < r0max;
                if (GRAD) {
                    if (!is_short) {
                        double *g = gslot + 3 * (size_t)(e0 + n);
                        g[0] = 0.5 * w * rv[0]; g[1] = 0.5 * w * rv[1]; g[2] = 0.5 * w * rv[2];
                    }
                } else {
                    es += 0.5 * e;
                    fx += w * rv[0]; fy += w * rv[1]; fz += w * rv[2];
                }
                if (is_short) {
                    const double inv = 1.0 / r;
                    u[0] = rv[0] * inv; u[1] = rv[1] * inv; u[2] = rv[2] * inv;
                    f = vash_f(p, r);
                }
            }
        }
        const unsigned bits = (unsigned)(__ballot(is_short) >> quad_shift) & 0xFu;
        const int at = cnt + __popc(bits & ((1u << q) - 1u));
        if (is_short && at < VA_MAXD) {
            sh.ux[at][cb] = u[0]; sh.uy[at][cb] = u[1]; sh.uz[at][cb] = u[2];
            sh.r[at][cb] = r; sh.f[at][cb] = f;
            sh.idx[at][cb] = n; sh.tp[at][cb] = (signed char)tn;
        }
        cnt += __popc(bits);
    }
    __syncthreads();
    // ---- phase 2: the three-body term on the short row ----------------------------------------------------------------------------
    if (mine && cnt <= VA_MAXD) {
#pragma unroll 1
        for (int s = q; s < cnt; s += VA_LANES) {
            const double ux = sh.ux[s][cb], uy = sh.uy[s][cb], uz = sh.uz[s][cb], r = sh.r[s][cb], f = sh.f[s][cb];
            const int tn = sh.tp[s][cb], n = sh.idx[s][cb];
            const VashPairP &p = tb.two[ti * nt + tn];
            double e3 = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
            if (f != 0.0) {
                VashAcc a = {0.0, 0.0, 0.0, 0.0};
                const int t0 = (ti * nt + tn) * nt;
#pragma unroll 1
                for (int m = 0; m < cnt; ++m) {
                    const double fm = sh.f[m][cb];
                    if (m == s || fm == 0.0) continue;
                    vash_term(a, ux, uy, uz, sh.ux[m][cb], sh.uy[m][cb], sh.uz[m][cb], fm, tb.tri[t0 + sh.tp[m][cb]]);
                }
                vash_finish(a, ux, uy, uz, r, f, vash_dlf(p, r), e3, gx, gy, gz);
            }
            double *g = gslot + 3 * (size_t)(e0 + n);
            if (GRAD) {
                double e = 0.0, de = 0.0;
                if (r < p.rc) vash_pair(p, r, e, de);
                g[0] = 0.5 * de * ux + gx; g[1] = 0.5 * de * uy + gy; g[2] = 0.5 * de * uz + gz;
            } else {
                ej3[e0 + n] = e3 * (1.0 / 3.0);
                g[0] = gx; g[1] = gy; g[2] = gz;
                sidx[(size_t)VA_ATOM_INTS * i + 1 + s] = n;
                es += e3 * (1.0 / 6.0);
                fx += gx; fy += gy; fz += gz;
            }
        }
    } else if (mine) {   // more short slots than the tile holds: every short neighbor's values recomputed from global memory
#pragma unroll 1
        for (int n = q; n < deg; n += VA_LANES) {
            const int j = __float_as_int(edge[e0 + n].w);
            if (j < 0) continue;
            double rv[3];
            edge_vec(wpos, C, i, j, edge_S[e0 + n], rv);
            const double r = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
            if (!(r < r0max)) continue;
            const double inv = 1.0 / r, ux = rv[0] * inv, uy = rv[1] * inv, uz = rv[2] * inv;
            const int tn = type[j];
            const VashPairP &p = tb.two[ti * nt + tn];
            const double f = vash_f(p, r);
            double e3 = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
            if (f != 0.0) {
                VashAcc a = {0.0, 0.0, 0.0, 0.0};
                const int t0 = (ti * nt + tn) * nt;
#pragma unroll 1
                for (int m = 0; m < deg; ++m) {
                    const int jm = __float_as_int(edge[e0 + m].w);
                    if (m == n || jm < 0) continue;
                    double v[3];
                    edge_vec(wpos, C, i, jm, edge_S[e0 + m], v);
                    const double rm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                    if (!(rm < r0max)) continue;
                    const int tm = type[jm];
                    const double fm = vash_f(tb.two[ti * nt + tm], rm);
                    if (fm == 0.0) continue;
                    const double invm = 1.0 / rm;
                    vash_term(a, ux, uy, uz, v[0] * invm, v[1] * invm, v[2] * invm, fm, tb.tri[t0 + tm]);
                }
                vash_finish(a, ux, uy, uz, r, f, vash_dlf(p, r), e3, gx, gy, gz);
            }
            double *g = gslot + 3 * (size_t)(e0 + n);
            if (GRAD) {
                double e = 0.0, de = 0.0;
                if (r < p.rc) vash_pair(p, r, e, de);
                g[0] = 0.5 * de * ux + gx; g[1] = 0.5 * de * uy + gy; g[2] = 0.5 * de * uz + gz;
            } else {
                ej3[e0 + n] = e3 * (1.0 / 3.0);
                g[0] = gx; g[1] = gy; g[2] = gz;
                es += e3 * (1.0 / 6.0);
                fx += gx; fy += gy; fz += gz;
            }
        }
    }
    if (GRAD) return;
    // (every lane of the wave arrives here: lanes without a centre carry zeros into the quad sums)
    es = quad_sum_f64(es);
    fx = quad_sum_f64(fx);
    fy = quad_sum_f64(fy);
    fz = quad_sum_f64(fz);
    if (mine && q == 0) {
        e_atom[i] = es;
        forces[3 * i] = fx; forces[3 * i + 1] = fy; forces[3 * i + 2] = fz;
        sidx[(size_t)VA_ATOM_INTS * i] = cnt;
    }
}

// Atom c: the neighbor shares of the three-body terms centred on its short neighbors, and minus their gradients, over the reverse
// slots of its own short slots, added to what the site kernel left in e_atom / forces.  A centre with more than VA_MAXD short slots
// finds them by the site kernel's own test (r < r0max on the same fp64 edge vector).
__device__ __forceinline__ void vash_gather_atom(int c, double r0max, const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                                                 const double *__restrict__ wpos, const int *__restrict__ row_start,
                                                 const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                                                 const int *__restrict__ rev, const double *__restrict__ ej3,
                                                 const double *__restrict__ gslot, const int *__restrict__ sidx,
                                                 double *__restrict__ e_atom, double *__restrict__ forces) {
    const int e0 = row_start[c], cnt = sidx[(size_t)VA_ATOM_INTS * c];
    if (cnt == 0) return;
    double ea = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0;
    if (cnt <= VA_MAXD) {
        for (int s = 0; s < cnt; ++s) {
            const int r = rev[e0 + sidx[(size_t)VA_ATOM_INTS * c + 1 + s]];
            if (r < 0) continue;
            ea += ej3[r];
            f0 -= gslot[3 * (size_t)r]; f1 -= gslot[3 * (size_t)r + 1]; f2 -= gslot[3 * (size_t)r + 2];
        }
    } else {
        const double *C = cell + 9 * atom_cfg[c];
        for (int e = e0; e < row_start[c + 1]; ++e) {
            const int j = __float_as_int(edge[e].w), r = rev[e];
            if (j < 0 || r < 0) continue;
            double rv[3];
            edge_vec(wpos, C, c, j, edge_S[e], rv);
            if (!(sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]) < r0max)) continue;
            ea += ej3[r];
            f0 -= gslot[3 * (size_t)r]; f1 -= gslot[3 * (size_t)r + 1]; f2 -= gslot[3 * (size_t)r + 2];
        }
    }
    e_atom[c] += ea;
    forces[3 * c] += f0; forces[3 * c + 1] += f1; forces[3 * c + 2] += f2;
}

}  // namespace vssr
#endif
