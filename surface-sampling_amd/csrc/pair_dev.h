// pair_dev.h — device bodies of the pair-potential kernel (pair.hip): the term table, one term's energy and derivative, the
// 4-lane combine, the site tile.  Semantics: LAMMPS pair_style lj/cut, morse, buck, born and coul/dsf, units metal (see pair.hip).
#ifndef VSSR_PAIR_DEV_H
#define VSSR_PAIR_DEV_H
#include "pot_dev.h"

namespace vssr {

constexpr int PAIR_MAX_TYPES = 8, PAIR_MAX_TERMS = 3;
constexpr int PAIR_CENTRES = 64, PAIR_LANES = 4;   // centres / workgroup; lanes / centre (the launch shape of k_sw_site)
constexpr double PAIR_QQRD2E = 14.399645;          // LAMMPS qqrd2e, units metal
constexpr double PAIR_2_SQRTPI = 1.12837916709551257390;   // 2 / sqrt(pi)

// One term of an ordered type pair as the kernel reads it (64 bytes), derived on the host at vssr_pair_create.  style: VSSR_PAIR_*
// (0 = no term: ends the pair's list).  c[] by style:
//   lj/cut    eps, sig
//   morse     D0, alpha, r0
//   buck      A, 1 / rho, C
//   born      A, 1 / rho, sig, C, D
//   coul/dsf  alpha, erfc(alpha rc) / rc, B = erfc(alpha rc) / rc^2 + 2 alpha / sqrt(pi) exp(-alpha^2 rc^2) / rc, qqrd2e q_a q_b
//   coul/long g, -, -, qqrd2e q_a q_b   (qqrd2e q_a q_b erfc(g r) / r: the real-space part of the Ewald sum of ewald.hip)
// eshift: E(rc) of the four non-Coulomb styles under pair_modify shift yes, else 0.
struct PairTerm {
    double c[5], rc, eshift;
    int style, pad;
};
// The handle's table (pot_params): terms of every ordered pair [a][b][k] with the compiled strides, then the coul/dsf self energy
// of every type, -(erfc(alpha rc) / (2 rc) + alpha / sqrt(pi)) qqrd2e q_a^2 (0 for a type without a coul/dsf term).
struct PairTable {
    PairTerm term[PAIR_MAX_TYPES * PAIR_MAX_TYPES * PAIR_MAX_TERMS];
    double self_e[PAIR_MAX_TYPES];
};

// E(r) and dE/dr of one term at r < rc (the caller has tested the cutoff).  ONE expression for the energy and for the gradient
// launch, so both see the same bits.
__device__ __forceinline__ void pair_term(const PairTerm &t, double r, double &e, double &de) {
    const double ir = 1.0 / r;
    switch (t.style) {
    case VSSR_PAIR_LJ_CUT: {
        const double s = t.c[1] * ir, s2 = s * s, s6 = s2 * s2 * s2;
        e = 4.0 * t.c[0] * s6 * (s6 - 1.0);
        de = -24.0 * t.c[0] * s6 * (2.0 * s6 - 1.0) * ir;
        break;
    }
    case VSSR_PAIR_MORSE: {
        const double x = exp(-t.c[1] * (r - t.c[2]));
        e = t.c[0] * (x * x - 2.0 * x);
        de = -2.0 * t.c[1] * t.c[0] * (x * x - x);
        break;
    }
    case VSSR_PAIR_BUCK: {
        const double x = t.c[0] * exp(-r * t.c[1]), i2 = ir * ir, i6 = i2 * i2 * i2;
        e = x - t.c[2] * i6;
        de = -x * t.c[1] + 6.0 * t.c[2] * i6 * ir;
        break;
    }
    case VSSR_PAIR_BORN: {
        const double x = t.c[0] * exp((t.c[2] - r) * t.c[1]), i2 = ir * ir, i6 = i2 * i2 * i2, i8 = i6 * i2;
        e = x - t.c[3] * i6 + t.c[4] * i8;
        de = -x * t.c[1] + 6.0 * t.c[3] * i6 * ir - 8.0 * t.c[4] * i8 * ir;
        break;
    }
    case VSSR_PAIR_COUL_LONG: {   // the real-space part of an Ewald sum: no shift (c: g, -, -, qqrd2e q_a q_b)
        const double a = t.c[0], ec = erfc(a * r) * ir;
        e = t.c[3] * ec;
        de = t.c[3] * (-ec * ir - PAIR_2_SQRTPI * a * exp(-a * a * r * r) * ir);
        break;
    }
    default: {   // VSSR_PAIR_COUL_DSF
        const double a = t.c[0], ec = erfc(a * r) * ir;
        e = t.c[3] * (ec - t.c[1] + t.c[2] * (r - t.rc));
        de = t.c[3] * (-ec * ir - PAIR_2_SQRTPI * a * exp(-a * a * r * r) * ir + t.c[2]);
        break;
    }
    }
    e -= t.eshift;
}

// Sum over the four lanes of a centre (one DPP quad), the same bits in every lane: (x_q + x_q^1) + (x_q^2 + x_q^3), and fp64
// addition commutes.  Two 32-bit moves per step; every lane of the wave takes part (lanes without a centre carry zeros).
__device__ __forceinline__ double quad_xchg_f64(double x, bool far) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    if (far) {
        lo = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
        hi = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true);
    } else {
        lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
        hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true);
    }
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double quad_sum_f64(double x) {
    x += quad_xchg_f64(x, false);
    x += quad_xchg_f64(x, true);
    return x;
}

// One tile of PAIR_CENTRES centres, PAIR_LANES lanes each: thread tid serves centre i = (tile's first atom) + (tid >> 2), `mine`: the
// centre exists and is evaluated.  Every thread of the workgroup calls this (one barrier inside).  sh: the term table in LDS,
// PAIR_MAX_TYPES^2 x PAIR_MAX_TERMS entries.  GRAD: write the per-slot gradients G_n = 1/2 E'(r_n) u_n into gslot and nothing else.
template <bool GRAD>
__device__ __forceinline__ void pair_site_tile(PairTerm *sh, int i, bool mine, int nt, const PairTable *__restrict__ P,
                                               const int *__restrict__ type, const int *__restrict__ atom_cfg,
                                               const double *__restrict__ cell, const double *__restrict__ wpos,
                                               const int *__restrict__ row_start, const float4 *__restrict__ edge,
                                               const int *__restrict__ edge_S, double *__restrict__ e_atom, double *__restrict__ forces,
                                               double *__restrict__ gslot) {
    const int tid = threadIdx.x, q = tid & (PAIR_LANES - 1);
    // the terms of the nt x nt pairs in use, packed [a][b][k]; 16-byte pieces
    {
        constexpr int PIECES = sizeof(PairTerm) / sizeof(uint4);
        const uint4 *src = reinterpret_cast<const uint4 *>(P->term);
        uint4 *dst = reinterpret_cast<uint4 *>(sh);
        for (int t = tid; t < nt * nt * PAIR_MAX_TERMS * PIECES; t += PAIR_CENTRES * PAIR_LANES) {
            const int term = t / PIECES, piece = t % PIECES;
            const int k = term % PAIR_MAX_TERMS, ab = term / PAIR_MAX_TERMS, a = ab / nt, b = ab % nt;
            dst[t] = src[((a * PAIR_MAX_TYPES + b) * PAIR_MAX_TERMS + k) * PIECES + piece];
        }
    }
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
#pragma unroll 1
    for (int n = q; n < deg; n += PAIR_LANES) {
        const int j = __float_as_int(edge[e0 + n].w);
        if (j < 0) continue;   // padding slot (k_slot_stress skips it as well)
        double rv[3];
        edge_vec(wpos, C, i, j, edge_S[e0 + n], rv);
        const double r = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
        const PairTerm *T = sh + (ti * nt + type[j]) * PAIR_MAX_TERMS;
        double e = 0.0, de = 0.0;
#pragma unroll 1
        for (int k = 0; k < PAIR_MAX_TERMS; ++k) {
            if (T[k].style == VSSR_PAIR_NONE) break;
            if (!(r < T[k].rc)) continue;
            double ek, dek;
            pair_term(T[k], r, ek, dek);
            e += ek;
            de += dek;
        }
        const double w = de / r;
        if (GRAD) {
            double *g = gslot + 3 * (size_t)(e0 + n);
            g[0] = 0.5 * w * rv[0]; g[1] = 0.5 * w * rv[1]; g[2] = 0.5 * w * rv[2];
        } else {
            es += e;
            fx += w * rv[0]; fy += w * rv[1]; fz += w * rv[2];
        }
    }
    if (GRAD) return;
    // (every lane of the wave arrives here: lanes without a centre carry zeros into the quad sums)
    es = quad_sum_f64(es);
    fx = quad_sum_f64(fx);
    fy = quad_sum_f64(fy);
    fz = quad_sum_f64(fz);
    if (mine && q == 0) {
        e_atom[i] = 0.5 * es + P->self_e[ti];
        forces[3 * i] = fx; forces[3 * i + 1] = fy; forces[3 * i + 2] = fz;
    }
}

}  // namespace vssr
#endif
