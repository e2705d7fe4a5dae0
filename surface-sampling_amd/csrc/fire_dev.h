// fire_dev.h -- ASE's FIRE update (ase/optimize/fire.py), once: the dt / a / Nsteps bookkeeping with the mixing coefficients, the
// step length from three sums, the knobs and their check.  Serves k_fire_step (relax.hip: per chain, with its own reduction of the
// step length), k_neb_step (neb.hip: over a band), k_dimer_advance (dimer.hip: the translation) and k_cell_step (relax_cell.hip: over
// atoms and strain).  G is the force the step follows.
#ifndef VSSR_FIRE_DEV_H
#define VSSR_FIRE_DEV_H
#include <cmath>
#include "vssr_internal.h"

namespace vssr {

struct FireKnobs {
    double dtmax, finc, fdec, astart, fa, maxstep;
    int nmin;
};
// v' = c1 v + (mix_s + dt) G; without mix (the first step, or a power v.G <= 0) v' = dt G
struct FireMix {
    bool mix;
    double mix_a, mix_s, c1;
};

// S: a state with dt, a, nsteps_pos (ASE's Nsteps) and has_v (0 until the first step); vG, GG, vv: v.G, G.G, v.v
template <class State>
__device__ __forceinline__ FireMix fire_update(State &S, const FireKnobs &K, double vG, double GG, double vv) {
    FireMix M = {false, 0.0, 0.0, 0.0};
    if (S.has_v) {
        if (vG > 0.0) {
            M.mix = true;
            M.mix_a = S.a;
            M.mix_s = S.a * sqrt(vv / GG);   // v = (1 - a) v + a G |v| / |G|
            M.c1 = 1.0 - M.mix_a;
            if (S.nsteps_pos > K.nmin) { S.dt = fmin(S.dt * K.finc, K.dtmax); S.a *= K.fa; }
            S.nsteps_pos += 1;
        } else {
            S.a = K.astart; S.dt *= K.fdec; S.nsteps_pos = 0;
        }
    }
    return M;
}

// The scale that keeps the step dt v' within maxstep: |dt v'| follows from the three sums, which saves a second reduction pass
__device__ __forceinline__ double fire_step_scale(double dt, const FireMix &M, const FireKnobs &K, double vG, double GG, double vv) {
    const double c2 = M.mix_s + dt;
    const double nv2 = (M.c1 * M.c1) * vv + (2.0 * M.c1 * c2) * vG + (c2 * c2) * GG;
    const double normdr = dt * sqrt(nv2);
    return normdr > K.maxstep ? K.maxstep / normdr : 1.0;
}

// the knobs of an entry point's parameters, checked in this order; func: the entry point's name for the message
inline int fire_check(vssr_handle *h, const char *func, double dt, const FireKnobs &K) {
    auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!positive(dt)) return set_err(h, VSSR_E_BADARG, "%s: dt %g (finite and > 0 wanted)", func, dt);
    if (!positive(K.maxstep)) return set_err(h, VSSR_E_BADARG, "%s: maxstep %g A (finite and > 0 wanted)", func, K.maxstep);
    if (!positive(K.dtmax)) return set_err(h, VSSR_E_BADARG, "%s: dtmax %g (finite and > 0 wanted)", func, K.dtmax);
    if (!(std::isfinite(K.finc) && K.finc >= 1.0)) return set_err(h, VSSR_E_BADARG, "%s: finc %g (finite and >= 1 wanted)", func, K.finc);
    if (!(K.fdec > 0.0 && K.fdec < 1.0)) return set_err(h, VSSR_E_BADARG, "%s: fdec %g outside (0, 1)", func, K.fdec);
    if (!(K.fa > 0.0 && K.fa < 1.0)) return set_err(h, VSSR_E_BADARG, "%s: fa %g outside (0, 1)", func, K.fa);
    if (!(K.astart > 0.0 && K.astart <= 1.0)) return set_err(h, VSSR_E_BADARG, "%s: astart %g outside (0, 1]", func, K.astart);
    if (K.nmin < 0) return set_err(h, VSSR_E_BADARG, "%s: nmin %d < 0", func, K.nmin);
    return VSSR_OK;
}

}  // namespace vssr
#endif
