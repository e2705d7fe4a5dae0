// pair_dev.h — device bodies of the pair-potential kernel (pair.hip): the term table, one term's energy and derivative, the
// 4-lane combine.  Semantics: LAMMPS pair_style lj/cut, morse, buck, born and coul/dsf, units metal (see pair.hip).
#ifndef VSSR_PAIR_DEV_H
#define VSSR_PAIR_DEV_H
#include "tersoff_dev.h"   // edge_vec, tersoff_chain_energy

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

}  // namespace vssr
#endif
