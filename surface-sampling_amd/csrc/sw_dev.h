// sw_dev.h — device bodies of the Stillinger-Weber kernels (sw.hip): per-slot radial factors, the site tile and its long-row form,
// the gather.  Semantics: LAMMPS pair_style sw, units metal (see sw.hip).
#ifndef VSSR_SW_DEV_H
#define VSSR_SW_DEV_H
#include "pot_dev.h"

namespace vssr {

// One entry (i, j, k) as the kernels read it, derived on the host at vssr_sw_create from the file's columns
// (eps sig a lambda gamma costheta0 A B p q tol):
//   cut = a sig, c5 = A eps B sig^p, c6 = A eps sig^q, gs = gamma sig   (two-body term and radial factor: entry (i, j, j))
//   le = lambda eps, c0 = costheta0                                      (three-body term: entry (i, j, k))
struct SwP { double cut, sig, gs, c5, c6, p, q, le, c0, pad0, pad1; };

constexpr int SW_MAXD = 16, SW_CENTRES = 64, SW_LANES = 4, SW_MAXP = 512;   // slots per row in LDS; centres / workgroup; lanes / centre; 8^3 entries
constexpr int SW_OWN = SW_MAXD / SW_LANES;                                     // slots a lane owns in the tile form

// Radial factor of the three-body term for a slot at distance r with entry (i, j, j): ef = exp(gamma sig / (r - a sig)), 0 outside.
// ONE expression for both forms of the site kernel (a neighbor's ef is read from LDS in the tile form, recomputed in the long-row
// form): the same bits either way.
__device__ __forceinline__ double sw_ef(const SwP &p, double r) {
    if (!(r < p.cut)) return 0.0;
    return exp(p.gs * (1.0 / (r - p.cut)));
}
// Everything the slot's own lane needs: ef, d ln ef / dr, the two-body term phi2 = (c5 r^-p - c6 r^-q) exp(sig / (r - a sig)) and
// its derivative (LAMMPS PairSW::twobody).
__device__ __forceinline__ void sw_radial(const SwP &p, double r, double &ef, double &dlf, double &e2, double &de2) {
    ef = 0.0; dlf = 0.0; e2 = 0.0; de2 = 0.0;
    if (!(r < p.cut)) return;
    const double x = 1.0 / (r - p.cut);
    ef = exp(p.gs * x);
    dlf = -p.gs * x * x;
    const double rp = pow(r, -p.p), rq = pow(r, -p.q), es = exp(p.sig * x);
    const double v = p.c5 * rp - p.c6 * rq;
    e2 = v * es;
    de2 = ((-p.p * p.c5 * rp + p.q * p.c6 * rq) / r - v * p.sig * x * x) * es;
}

// Sums of slot n over the other slots m of its centre: T = sum_m le_nm ef_m dc^2, S = sum_m 2 le_nm ef_m dc (u_m - cs u_n), dc = cs - c0_nm.
// With them phi3 summed over the pairs {n, m} is ef_n T and its gradient with respect to r_n is ef_n (S / r_n + dlf_n T u_n).
struct SwAcc { double T, sx, sy, sz; };
__device__ __forceinline__ void sw_term(SwAcc &a, double ux, double uy, double uz, double vx, double vy, double vz, double efm, double le,
                                        double c0) {
    const double cs = ux * vx + uy * vy + uz * vz;
    const double dc = cs - c0, w = le * efm;
    a.T += w * dc * dc;
    const double g = 2.0 * w * dc;
    a.sx += g * (vx - cs * ux);
    a.sy += g * (vy - cs * uy);
    a.sz += g * (vz - cs * uz);
}
// Slot n complete: energy shares and G_n = dE / d r_n.  eo: the centre's share (1/4 of the directed two-body half, 1/6 of every
// three-body term the slot takes part in: the centre's third split over the two slots), ej: the neighbor's share (1/4 of the directed
// half, 1/3 of every three-body term).  pe/atom of LAMMPS: pair terms half / half, three-body terms in thirds (ev_tally3).
__device__ __forceinline__ void sw_finish(const SwAcc &a, double ux, double uy, double uz, double r, double ef, double dlf, double e2,
                                          double de2, double &eo, double &ej, double &gx, double &gy, double &gz) {
    const double e3 = ef * a.T;
    eo = 0.25 * e2 + e3 * (1.0 / 6.0);
    ej = 0.25 * e2 + e3 * (1.0 / 3.0);
    const double pa = ef / r, su = 0.5 * de2 + ef * dlf * a.T;
    gx = pa * a.sx + su * ux;
    gy = pa * a.sy + su * uy;
    gz = pa * a.sz + su * uz;
}

struct SwShared {
    double ux[SW_MAXD][SW_CENTRES], uy[SW_MAXD][SW_CENTRES], uz[SW_MAXD][SW_CENTRES], ef[SW_MAXD][SW_CENTRES];
    signed char tp[SW_MAXD][SW_CENTRES];
    double2 lc[SW_MAXP];   // {lambda eps, costheta0} of every entry (i, j, k)
};

// One tile of SW_CENTRES centres, SW_LANES lanes each: thread tid serves centre i = (tile's first atom) + (tid >> 2) with lane
// q = tid & 3, which owns the slots n = q, q + 4, ... of the centre.  Rows of <= SW_MAXD slots: the neighborhood (unit vectors, ef,
// types) is staged in LDS, the own slots' radial values stay in registers; longer rows: the same lanes recompute every neighbor's
// values from global memory (the long-row form, same arithmetic).  Every G_slot, eo, ej is written by exactly one lane.
__device__ __forceinline__ void sw_site_tile(SwShared &sh, int i, bool mine, int nt, const SwP *__restrict__ P,
                                             const int *__restrict__ type, const int *__restrict__ atom_cfg,
                                             const double *__restrict__ cell, const double *__restrict__ wpos,
                                             const int *__restrict__ row_start, const float4 *__restrict__ edge,
                                             const int *__restrict__ edge_S, double *__restrict__ eo_out, double *__restrict__ ej_out,
                                             double *__restrict__ gslot) {
    const int tid = threadIdx.x, cb = tid >> 2, q = tid & 3;
    for (int t = tid; t < nt * nt * nt; t += SW_CENTRES * SW_LANES) sh.lc[t] = make_double2(P[t].le, P[t].c0);
    int e0 = 0, deg = 0, ti = 0;
    if (mine) {
        e0 = row_start[i];
        deg = row_start[i + 1] - e0;
        ti = type[i];
    }
    const bool tile = mine && deg <= SW_MAXD;
    const double *C = mine ? cell + 9 * atom_cfg[i] : cell;
    // ---- own slots: geometry and radial values; the neighborhood -> LDS (tile form) -----------------------------------------
    double o_ux[SW_OWN], o_uy[SW_OWN], o_uz[SW_OWN], o_r[SW_OWN], o_ef[SW_OWN], o_dlf[SW_OWN], o_e2[SW_OWN], o_de2[SW_OWN];
    int o_tp[SW_OWN];
#pragma unroll
    for (int k = 0; k < SW_OWN; ++k) {
        const int n = q + SW_LANES * k;
        double u[3] = {0.0, 0.0, 0.0}, r = 1.0, ef = 0.0, dlf = 0.0, e2 = 0.0, de2 = 0.0;
        int tp = -1;
        if (tile && n < deg) {
            const int j = __float_as_int(edge[e0 + n].w);
            if (j >= 0) {
                edge_vec(wpos, C, i, j, edge_S[e0 + n], u);
                r = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
                const double inv = 1.0 / r;
                u[0] *= inv; u[1] *= inv; u[2] *= inv;
                tp = type[j];
                sw_radial(P[(ti * nt + tp) * nt + tp], r, ef, dlf, e2, de2);
            }
            sh.ux[n][cb] = u[0]; sh.uy[n][cb] = u[1]; sh.uz[n][cb] = u[2];
            sh.ef[n][cb] = ef; sh.tp[n][cb] = (signed char)tp;
        }
        o_ux[k] = u[0]; o_uy[k] = u[1]; o_uz[k] = u[2]; o_r[k] = r; o_ef[k] = ef; o_dlf[k] = dlf; o_e2[k] = e2; o_de2[k] = de2;
        o_tp[k] = tp;
    }
    __syncthreads();
    if (tile) {
#pragma unroll
        for (int k = 0; k < SW_OWN; ++k) {
            const int n = q + SW_LANES * k;
            if (n >= deg) break;
            double eo = 0.0, ej = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
            if (o_ef[k] != 0.0) {
                SwAcc a = {0.0, 0.0, 0.0, 0.0};
                const int base = (ti * nt + o_tp[k]) * nt;
#pragma unroll 1
                for (int m = 0; m < deg; ++m) {
                    const double efm = sh.ef[m][cb];
                    if (m == n || efm == 0.0) continue;
                    const double2 lc = sh.lc[base + sh.tp[m][cb]];
                    sw_term(a, o_ux[k], o_uy[k], o_uz[k], sh.ux[m][cb], sh.uy[m][cb], sh.uz[m][cb], efm, lc.x, lc.y);
                }
                sw_finish(a, o_ux[k], o_uy[k], o_uz[k], o_r[k], o_ef[k], o_dlf[k], o_e2[k], o_de2[k], eo, ej, gx, gy, gz);
            }
            eo_out[e0 + n] = eo; ej_out[e0 + n] = ej;
            gslot[3 * (e0 + n)] = gx; gslot[3 * (e0 + n) + 1] = gy; gslot[3 * (e0 + n) + 2] = gz;
        }
    } else if (mine) {   // long row: every neighbor's vector and ef recomputed from global memory
#pragma unroll 1
        for (int n = q; n < deg; n += SW_LANES) {
            double eo = 0.0, ej = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
            const int j = __float_as_int(edge[e0 + n].w);
            if (j >= 0) {
                double u[3], ef, dlf, e2, de2;
                edge_vec(wpos, C, i, j, edge_S[e0 + n], u);
                const double r = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), inv = 1.0 / r;
                u[0] *= inv; u[1] *= inv; u[2] *= inv;
                const int tn = type[j];
                sw_radial(P[(ti * nt + tn) * nt + tn], r, ef, dlf, e2, de2);
                if (ef != 0.0) {
                    SwAcc a = {0.0, 0.0, 0.0, 0.0};
                    const int base = (ti * nt + tn) * nt;
#pragma unroll 1
                    for (int m = 0; m < deg; ++m) {
                        const int jm = __float_as_int(edge[e0 + m].w);
                        if (m == n || jm < 0) continue;
                        double v[3];
                        edge_vec(wpos, C, i, jm, edge_S[e0 + m], v);
                        const double rm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), invm = 1.0 / rm;
                        const int tm = type[jm];
                        const double efm = sw_ef(P[(ti * nt + tm) * nt + tm], rm);
                        if (efm == 0.0) continue;
                        const double2 lc = sh.lc[base + tm];
                        sw_term(a, u[0], u[1], u[2], v[0] * invm, v[1] * invm, v[2] * invm, efm, lc.x, lc.y);
                    }
                    sw_finish(a, u[0], u[1], u[2], r, ef, dlf, e2, de2, eo, ej, gx, gy, gz);
                }
            }
            eo_out[e0 + n] = eo; ej_out[e0 + n] = ej;
            gslot[3 * (e0 + n)] = gx; gslot[3 * (e0 + n) + 1] = gy; gslot[3 * (e0 + n) + 2] = gz;
        }
    }
}

// Atom c: pe/atom = its own shares of its slots + the neighbor shares of the reverse slots; force = sum (G[slot] - G[rev[slot]]).
__device__ __forceinline__ void sw_gather_atom(int c, const int *__restrict__ row_start, const int *__restrict__ rev,
                                               const double *__restrict__ eo, const double *__restrict__ ej,
                                               const double *__restrict__ gslot, double *__restrict__ e_atom,
                                               double *__restrict__ forces) {
    double ea = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0;
    for (int e = row_start[c]; e < row_start[c + 1]; ++e) {
        const int r = rev[e];
        if (r < 0) continue;
        ea += eo[e] + ej[r];
        f0 += gslot[3 * e] - gslot[3 * r];
        f1 += gslot[3 * e + 1] - gslot[3 * r + 1];
        f2 += gslot[3 * e + 2] - gslot[3 * r + 2];
    }
    e_atom[c] = ea;
    forces[3 * c] = f0; forces[3 * c + 1] = f1; forces[3 * c + 2] = f2;
}

// d_gbar of a Stillinger-Weber handle between the site kernel, the gather and the virial kernel: eo [slots] | ej [slots] | G [slots][3]
// (sw.hip and the chain-resident minimiser, chain_min.hip)
struct SwSlots {
    double *eo, *ej, *gslot;
    static size_t doubles(const vssr_handle *h) { return 5 * (size_t)h->slot_cap; }
    static SwSlots of(const vssr_handle *h) {
        double *eo = h->d_gbar.as<double>();
        return {eo, eo + h->slot_cap, eo + 2 * h->slot_cap};
    }
};

}  // namespace vssr
#endif
