// dimer.hip — the dimer method over the resident batch, on every handle kind that evaluates: a saddle search from ONE structure by
// min-mode following (Henkelman & Jonsson, J. Chem. Phys. 111, 7010 (1999)) with the one-gradient rotation of Heyden, Bell & Keil,
// J. Chem. Phys. 123, 224101 (2005), the force extrapolation of Kaestner & Sherwood, J. Chem. Phys. 128, 014106 (2008), and ASE's FIRE
// step as neb.hip restates it for the translation.  Restated from the three papers; NOT ASE's MinModeTranslate and not pinned by any
// executed library: the contract is the header comment of vssr_batch_dimer and the numpy restatement tests/dimer_oracle.py.
// A DIMER is two consecutive chains: 2 g holds the midpoint x0, 2 g + 1 the moving end x0 + delta N.  The driver frame is lockstep.h's:
// one batch-wide evaluation per visit, ONE launch behind it (k_dimer_advance, one 256-thread workgroup per dimer, which owns both
// chains: no slot exchange, no second launch; state advances nowhere else, so an evaluation repeated after a regrow moves nothing twice).
// A visit finds the dimer in one of two phases: behind an evaluation E (x0, x0 + delta N) or behind an evaluation R (x0,
// x0 + delta N*).  It closes the rotation in flight, runs the rotation test, and either opens the next trial rotation (-> R) or runs
// the step test and the FIRE translation (-> E).  Every vector loop is strided by ATOM with the same stride, so a thread only ever
// reads elements it wrote itself; the scalars all threads branch on come from the loaded state and from block reductions (fixed
// order, the same bits in every thread).  The passes over the 3 n components are kept in the plain form of the restatement -- a dot
// product per reduction -- instead of being fused: the kernel streams a few short arrays and is launch-bound next to any evaluation.
// Dimers that stopped leave the evaluation through d_active, as in relax_lockstep; one last unmasked evaluation restores the complete
// graph where the mask was installed, a dimer went back to where its step opened, or a dimer stopped after rotating (chain 2 g + 1
// then moves from the last trial end to x0 + delta N).
// Out of scope: conjugate-gradient or L-BFGS rotation directions, L-BFGS translation, a central-difference dimer, taking the idle
// midpoint out of evaluation R, a cap on the distance travelled, removal of rotation and translation, deduplication of saddles.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "arena.h"
#include "fire_dev.h"
#include "lockstep.h"
#include "md_dev.h"
#include "neb_dev.h"

namespace vssr {

enum { MD_TAG_DIMER = 2 };              // the Philox draw tag of a starting mode: no MD draw uses it (md_dev.h: 0 and 1)
enum { DIMER_PH_E = 0, DIMER_PH_R = 1 };

struct DimerState {   // per dimer
    double dt, a;              // FIRE
    double C, phi1, b1, e0;    // curvature; the trial angle and slope of the rotation in flight; E0 of the last evaluation E
    int nsteps_pos;            // steps since the last power <= 0 (ASE's Nsteps)
    int has_v;                 // 0 until the first translation
    int steps, reason, phase, rot, n_rot, n_eval;
};
struct DimerParams {
    int max_steps, max_rot_first, max_rot;
    double delta, phi_tol, fmax;
    FireKnobs fire;
};
struct DimerView {
    DimerState *st;                 // [G]
    // [3 N] each, laid out like the batch; a dimer uses the rows of its chain 2 g, the rows of the odd chains stay zero
    double *N, *Nopen, *xopen;      // the mode; the mode and midpoint the step in flight opened at
    double *F0, *F1, *theta, *vel;  // forces kept across evaluation R, the rotation direction, the FIRE velocity
    double *rec;                    // [G][4]
    int *info;                      // [G][4]
};

// Starting modes nobody handed in: standard normals of the free atoms of every dimer's chain 2 g, staged where mode_in would be.
__global__ void __launch_bounds__(256)
k_dimer_draw(const int *__restrict__ cfg_start, const uint8_t *__restrict__ fixed, const unsigned long long *__restrict__ dimer_id,
             uint32_t seed_lo, uint32_t seed_hi, double *__restrict__ staged) {
    const int g = blockIdx.x;
    const int a0 = cfg_start[2 * g], nat = cfg_start[2 * g + 1] - a0;
    uint32_t q0, q1;
    md_chain_key(seed_lo, seed_hi, dimer_id[g], q0, q1);
    for (int i = threadIdx.x; i < nat; i += blockDim.x) {
        double z[3] = {0.0, 0.0, 0.0};
        if (!(fixed && fixed[a0 + i])) md_normal3(q0, q1, 0, i, MD_TAG_DIMER, z);
        for (int k = 0; k < 3; ++k) staged[3 * (size_t)(a0 + i) + k] = z[k];
    }
}

// The starting mode (staged in V.theta: mode_in or k_dimer_draw's normals), held rows zeroed, normalised over the free atoms;
// x0 += displace N; the moving end; the state.
__global__ void __launch_bounds__(256)
k_dimer_init(const int *__restrict__ cfg_start, const uint8_t *__restrict__ fixed, double displace, double delta, double dt0, double astart,
             double *__restrict__ pos, DimerView V, unsigned char *__restrict__ active) {
    __shared__ double red[16];
    const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int a0 = cfg_start[2 * g], nat = cfg_start[2 * g + 1] - a0, a1 = cfg_start[2 * g + 1];
    double *x0 = pos + 3 * (size_t)a0, *x1 = pos + 3 * (size_t)a1;
    double *N = V.N + 3 * (size_t)a0, *No = V.Nopen + 3 * (size_t)a0, *xo = V.xopen + 3 * (size_t)a0;
    const double *staged = V.theta + 3 * (size_t)a0;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;
    double nn = 0.0;
    for (int i = tid; i < nat; i += nt) {
        const bool held = fx && fx[i];
        for (int k = 0; k < 3; ++k) {
            const double z = held ? 0.0 : staged[3 * i + k];
            N[3 * i + k] = z;
            nn += z * z;
        }
    }
    nn = block_sum(nn, red);
    const double norm = sqrt(nn);
    for (int i = tid; i < nat; i += nt)
        for (int k = 0; k < 3; ++k) {
            const int t = 3 * i + k;
            const double n = N[t] / norm;
            const double x = x0[t] + displace * n;
            N[t] = n; No[t] = n;
            x0[t] = x; xo[t] = x;
            x1[t] = x + delta * n;
        }
    if (tid == 0) {
        DimerState S = {dt0, astart, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, DIMER_PH_E, 0, 0, 0};
        V.st[g] = S;
        active[2 * g] = 1; active[2 * g + 1] = 1;
    }
}

// Behind an evaluation of the batch: one visit of dimer g's state machine.  FT: double (d_pot_f) or float (PaiNN's forces, widened).
// stopped: [0] dimers stopped, [1] of those that need the closing evaluation (went back, or stopped after rotating).
template <class FT>
__global__ void __launch_bounds__(256)
k_dimer_advance(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
                const FT *__restrict__ forces, const uint8_t *__restrict__ fixed, DimerParams P, double *__restrict__ pos, DimerView V,
                unsigned char *__restrict__ active, int *__restrict__ stopped) {
    __shared__ double red[16];
    if (counters[2]) return;   // the evaluation overflowed the neighbor capacity: the host regrows and repeats it; nothing moves
    const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    DimerState S = V.st[g];
    __syncthreads();   // every wave holds the state before thread 0 can store the advanced one (cg_dev.h)
    if (S.reason) return;
    const int b0 = 2 * g, b1 = 2 * g + 1;
    const int a0 = cfg_start[b0], nat = cfg_start[b0 + 1] - a0, a1 = cfg_start[b1];
    double *x0 = pos + 3 * (size_t)a0, *x1 = pos + 3 * (size_t)a1;
    const FT *fa = forces + 3 * (size_t)a0, *fb = forces + 3 * (size_t)a1;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;
    double *N = V.N + 3 * (size_t)a0, *No = V.Nopen + 3 * (size_t)a0, *xo = V.xopen + 3 * (size_t)a0;
    double *F0 = V.F0 + 3 * (size_t)a0, *F1 = V.F1 + 3 * (size_t)a0, *Th = V.theta + 3 * (size_t)a0, *v = V.vel + 3 * (size_t)a0;
    const double delta = P.delta;
    S.n_eval += 1;

    auto stop = [&](int reason, int refresh) {
        if (tid == 0) {
            S.reason = reason;
            V.st[g] = S;
            active[b0] = 0; active[b1] = 0;
            int *info = V.info + 4 * g;
            info[0] = S.steps; info[1] = reason; info[2] = S.n_rot; info[3] = S.n_eval;
            atomicAdd(stopped, 1);
            if (refresh) atomicAdd(stopped + 1, 1);
        }
    };

    // the finiteness test stands at the head of every visit, E or R, over both chains
    double bad = (isfinite(energy[b0]) && isfinite(energy[b1])) ? 0.0 : 1.0;
    for (int t = tid; t < 3 * nat; t += nt)
        if (!(isfinite((double)fa[t]) && isfinite((double)fb[t]))) bad = 1.0;
    bad = block_max(bad, red);
    if (bad != 0.0) {   // nothing sane to follow: back to the x0 and N the step opened at; that step is not counted
        for (int i = tid; i < nat; i += nt)
            for (int k = 0; k < 3; ++k) {
                const int t = 3 * i + k;
                N[t] = No[t];
                x0[t] = xo[t];
                x1[t] = xo[t] + delta * No[t];
            }
        if (S.steps > 0) S.steps -= 1;
        stop(3, 1);
        return;
    }

    if (S.phase == DIMER_PH_E) {   // 1. evaluation E: F0, F1, E0, the curvature
        double d0 = 0.0, d1 = 0.0;
        for (int i = tid; i < nat; i += nt) {
            const bool held = fx && fx[i];
            for (int k = 0; k < 3; ++k) {
                const int t = 3 * i + k;
                const double f0 = held ? 0.0 : (double)fa[t], f1 = held ? 0.0 : (double)fb[t];
                F0[t] = f0; F1[t] = f1;
                d0 += f0 * N[t]; d1 += f1 * N[t];
            }
        }
        d0 = block_sum(d0, red);
        d1 = block_sum(d1, red);
        S.C = (d0 - d1) / delta;
        S.e0 = energy[b0];
        S.rot = 0;
    } else {   // 3. evaluation R: close the rotation in flight
        const double c1 = cos(S.phi1), s1 = sin(S.phi1);
        double d0 = 0.0, d1 = 0.0;
        for (int i = tid; i < nat; i += nt) {
            const bool held = fx && fx[i];
            for (int k = 0; k < 3; ++k) {
                const int t = 3 * i + k;
                const double ns = N[t] * c1 + Th[t] * s1;
                const double f1s = held ? 0.0 : (double)fb[t];
                d0 += F0[t] * ns; d1 += f1s * ns;
            }
        }
        d0 = block_sum(d0, red);
        d1 = block_sum(d1, red);
        const double C = S.C, C1 = (d0 - d1) / delta;
        const double A1 = (C - C1 + S.b1 * sin(2.0 * S.phi1)) / (1.0 - cos(2.0 * S.phi1));
        const double A0 = 2.0 * (C - A1);
        double phim = 0.5 * atan(S.b1 / A1);
        double Cm = 0.5 * A0 + A1 * cos(2.0 * phim) + S.b1 * sin(2.0 * phim);
        if (Cm > C) {
            phim += 0.5 * M_PI;
            Cm = 0.5 * A0 + A1 * cos(2.0 * phim) + S.b1 * sin(2.0 * phim);
        }
        const double k1 = sin(S.phi1 - phim) / sin(S.phi1), k2 = sin(phim) / sin(S.phi1);
        const double k3 = 1.0 - cos(phim) - sin(phim) * tan(0.5 * S.phi1);
        const double cm = cos(phim), sm = sin(phim);
        double nn = 0.0;
        for (int i = tid; i < nat; i += nt) {
            const bool held = fx && fx[i];
            for (int k = 0; k < 3; ++k) {
                const int t = 3 * i + k;
                const double f1s = held ? 0.0 : (double)fb[t];
                F1[t] = k1 * F1[t] + k2 * f1s + k3 * F0[t];
                const double n = N[t] * cm + Th[t] * sm;
                N[t] = n;
                nn += n * n;
            }
        }
        nn = block_sum(nn, red);
        const double norm = sqrt(nn);
        for (int i = tid; i < nat; i += nt)
            for (int k = 0; k < 3; ++k) N[3 * i + k] = N[3 * i + k] / norm;
        S.C = Cm;
        S.rot += 1;
        S.n_rot += 1;
    }

    // 2. the rotation test
    double fdn = 0.0;
    for (int i = tid; i < nat; i += nt)
        for (int k = 0; k < 3; ++k) {
            const int t = 3 * i + k;
            fdn += (2.0 * (F1[t] - F0[t])) * N[t];
        }
    fdn = block_sum(fdn, red);
    double ff = 0.0;
    for (int i = tid; i < nat; i += nt)
        for (int k = 0; k < 3; ++k) {
            const int t = 3 * i + k;
            const double fp = 2.0 * (F1[t] - F0[t]) - fdn * N[t];
            ff += fp * fp;
        }
    ff = block_sum(ff, red);
    const double f = sqrt(ff);
    const double b1r = -f / (2.0 * delta);
    const double phi1 = 0.5 * atan(f / (2.0 * delta * fabs(S.C)));
    const int limit = S.steps == 0 ? P.max_rot_first : P.max_rot;
    if (tid == 0) V.rec[4 * g + 3] = f;
    if (S.rot < limit && f > 0.0 && phi1 >= P.phi_tol) {   // open the trial rotation
        const double c1 = cos(phi1), s1 = sin(phi1);
        for (int i = tid; i < nat; i += nt)
            for (int k = 0; k < 3; ++k) {
                const int t = 3 * i + k;
                const double th = (2.0 * (F1[t] - F0[t]) - fdn * N[t]) / f;
                Th[t] = th;
                x1[t] = x0[t] + delta * (N[t] * c1 + th * s1);
            }
        S.phi1 = phi1; S.b1 = b1r; S.phase = DIMER_PH_R;
        if (tid == 0) V.st[g] = S;
        return;
    }

    // 4. the step test, on F0 of the last evaluation E
    S.phase = DIMER_PH_E;
    double fm2 = 0.0, f0n = 0.0;
    for (int i = tid; i < nat; i += nt) {
        double g2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const int t = 3 * i + k;
            g2 += F0[t] * F0[t];
            f0n += F0[t] * N[t];
        }
        fm2 = fmax(fm2, g2);
    }
    fm2 = block_max(fm2, red);
    f0n = block_sum(f0n, red);
    if (tid == 0) { V.rec[4 * g] = sqrt(fm2); V.rec[4 * g + 1] = S.C; V.rec[4 * g + 2] = S.e0; }
    const bool done = fm2 < P.fmax * P.fmax && S.C < 0.0;
    if (done || S.steps >= P.max_steps) {
        // chain 2 g + 1 stands at the end of the last evaluation: behind a rotation that is not x0 + delta N
        if (S.rot > 0)
            for (int i = tid; i < nat; i += nt)
                for (int k = 0; k < 3; ++k) x1[3 * i + k] = x0[3 * i + k] + delta * N[3 * i + k];
        stop(done ? 1 : 2, S.rot > 0);
        return;
    }

    // 5. the translation: one ASE FIRE step on G, v' = c1 v + c2 G
    const bool saddle = S.C < 0.0;
    const double gn = saddle ? 2.0 * f0n : f0n;   // G = F0 - (2 F0.N) N below a negative curvature, -(F0.N) N otherwise
    double vG = 0.0, GG = 0.0, vv = 0.0;
    for (int i = tid; i < nat; i += nt)
        for (int k = 0; k < 3; ++k) {
            const int t = 3 * i + k;
            const double G = saddle ? F0[t] - gn * N[t] : (-gn) * N[t];
            const double vk = v[t];
            vG += vk * G; GG += G * G; vv += vk * vk;
        }
    vG = block_sum(vG, red);
    GG = block_sum(GG, red);
    vv = block_sum(vv, red);
    const FireMix M = fire_update(S, P.fire, vG, GG, vv);
    const double scale = fire_step_scale(S.dt, M, P.fire, vG, GG, vv);
    for (int i = tid; i < nat; i += nt) {
        const bool held = fx && fx[i];
        for (int k = 0; k < 3; ++k) {
            const int t = 3 * i + k;
            xo[t] = x0[t];
            No[t] = N[t];
            if (!held) {
                const double G = saddle ? F0[t] - gn * N[t] : (-gn) * N[t];
                double vk = M.mix ? (1.0 - M.mix_a) * v[t] + M.mix_s * G : 0.0;
                vk += S.dt * G;
                v[t] = vk;
                x0[t] += scale * (S.dt * vk);
            }
            x1[t] = x0[t] + delta * N[t];
        }
    }
    if (tid == 0) {
        S.has_v = 1;
        S.steps += 1;
        V.st[g] = S;
    }
}

// The call's workspace, all of it in the handle's d_dimer
struct DimerWork {
    DimerView V;
    DimerParams P;
    const uint8_t *fixed;        // the mask on the device (null: all free)
    NebChain *ch;                // [B]: a dimer as a group of two chains, for k_neb_compare
    unsigned long long *ids;     // [G]
    int *flags;                  // [0] dimers stopped, [1] of those that need the closing evaluation, [2] chain mismatch
    int ng;
};

static void dimer_launch(vssr_handle *h, const DimerWork &W) {
    hipStream_t st = h->stream;
    h->prof.begin(KC_DIMER, st);
    with_forces(h, [&](const double *energy, auto *forces) {
        hipLaunchKernelGGL(k_dimer_advance<force_type<decltype(forces)>>, dim3(W.ng), dim3(256), 0, st, h->d_cfg_start.as<int>(),
                           h->d_counters.as<int>(), energy, forces, W.fixed, W.P, h->d_pos.as<double>(), W.V,
                           h->d_active.as<unsigned char>(), W.flags);
    });
    h->prof.end(st);
}

static int dimer_lockstep(vssr_handle *h, const DimerWork &W, uint32_t want) {
    // evaluations a dimer can consume: one E per step and the last test, and every rotation it is allowed
    LockstepPlan plan{8, (long long)W.P.max_steps + 1 + W.P.max_rot_first + (long long)W.P.max_steps * W.P.max_rot, LOCKSTEP_MASK_AT_STOP};
    plan.stopped = W.flags; plan.groups = W.ng;
    bool finished;
    if (int rc = lockstep_run(h, plan, want, finished, [&] { dimer_launch(h, W); })) return rc;
    if (!finished) return set_err(h, VSSR_E_DEVICE, "vssr_batch_dimer: the dimer loop did not finish");
    return VSSR_OK;
}

}  // namespace vssr

using namespace vssr;

extern "C" int vssr_batch_dimer(vssr_handle *h, const vssr_dimer_params *p, const uint8_t *fixed, const double *mode_in, const uint64_t *dimer_id,
                                uint32_t want, double *pos_out, double *energy, double *mode_out, double *dimer, int32_t *info) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!p) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: null parameters");
    const int B = h->n_cfg, N = h->n_atoms, ng = B / 2;
    if (B < 2 || B % 2) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: %d chains (an even number wanted: a dimer is two chains)", B);
    if (p->max_steps < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: max_steps %d < 0", (int)p->max_steps);
    if (p->max_rot_first < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: max_rot_first %d < 0", (int)p->max_rot_first);
    if (p->max_rot < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: max_rot %d < 0", (int)p->max_rot);
    // (a negative nmin has always been reported ahead of delta and fmax here: it keeps its place; fire_check finds it in order otherwise)
    if (p->nmin < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: nmin %d < 0", (int)p->nmin);
    auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!positive(p->delta)) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: delta %g A (finite and > 0 wanted)", p->delta);
    if (!positive(p->fmax)) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: fmax %g eV/A (finite and > 0 wanted)", p->fmax);
    const FireKnobs fire{p->dtmax, p->finc, p->fdec, p->astart, p->fa, p->maxstep, p->nmin};
    if (int rc = fire_check(h, __func__, p->dt, fire)) return rc;
    if (!(p->phi_tol > 0.0 && p->phi_tol <= 0.25 * M_PI))
        return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: phi_tol %g rad outside (0, pi / 4]", p->phi_tol);
    if (!std::isfinite(p->displace)) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: displace %g A is not finite", p->displace);
    std::vector<NebChain> ch(B);
    for (int g = 0; g < ng; ++g) {
        const int f = 2 * g, b = f + 1, f0 = h->h_cfg_start[f], b0 = h->h_cfg_start[b], nat = h->h_n_atoms[f];
        if (h->h_n_atoms[b] != nat)
            return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: chains %d and %d are no dimer (atom counts)", f, b);
        int n_free = 0;
        double nn = 0.0;
        for (int i = 0; i < nat; ++i) {
            const bool held = fixed && fixed[f0 + i] != 0;
            if (fixed && (fixed[b0 + i] != 0) != held)
                return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: chains %d and %d are no dimer (fixed mask)", f, b);
            if (held) continue;
            ++n_free;
            if (mode_in)
                for (int k = 0; k < 3; ++k) nn += mode_in[3 * (size_t)(f0 + i) + k] * mode_in[3 * (size_t)(f0 + i) + k];
        }
        if (!n_free) return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: dimer %d has no free atom to carry a mode", g);
        if (mode_in && !(std::isfinite(nn) && nn > 0.0))
            return set_err(h, VSSR_E_BADARG, "vssr_batch_dimer: mode_in of dimer %d has squared length %g over its free atoms (finite and > 0 wanted)", g, nn);
        ch[f] = {f, 0, 2, g};
        ch[b] = {f, 1, 2, g};
    }

    VSSR_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    VSSR_HIP(h, hipStreamSynchronize(st));
    const size_t n3 = 3 * (size_t)N;
    DimerWork W;
    size_t dbl_bytes = 0;   // the doubles at the head of d_dimer, cleared in one piece
    auto layout = [&](Arena &a) {
        a.place(W.V.N, n3); a.place(W.V.Nopen, n3); a.place(W.V.xopen, n3); a.place(W.V.F0, n3); a.place(W.V.F1, n3);
        a.place(W.V.theta, n3); a.place(W.V.vel, n3); a.place(W.V.rec, 4 * (size_t)ng);
        dbl_bytes = a.offset();
        a.place(W.ids, (size_t)ng); a.place(W.V.st, (size_t)ng);
        a.place(W.ch, (size_t)B); a.place(W.V.info, 4 * (size_t)ng); a.place(W.flags, 4);
    };
    if (h->d_dimer.ensure(arena_size(layout))) return set_err(h, VSSR_E_NOMEM, "dimer workspace: out of device memory");
    arena_carve(h->d_dimer.p, layout);
    W.ng = ng;
    W.P = {p->max_steps, p->max_rot_first, p->max_rot, p->delta, p->phi_tol, p->fmax, fire};
    std::vector<unsigned long long> ids(ng);
    for (int g = 0; g < ng; ++g) ids[g] = dimer_id ? (unsigned long long)dimer_id[g] : (unsigned long long)g;
    VSSR_HIP(h, hipMemcpyAsync(W.ids, ids.data(), sizeof(unsigned long long) * ng, hipMemcpyHostToDevice, st));
    if (int rc = neb_compare_groups(h, ch, W.ch, W.flags,
                                    "vssr_batch_dimer: the two chains of a dimer differ in more than positions (species, cell or pbc; the comparison is bitwise)"))
        return rc;

    W.fixed = nullptr;
    if (int rc = driver_open(h, fixed, 2, W.fixed, want)) return rc;
    VSSR_HIP(h, hipMemsetAsync(W.V.N, 0, dbl_bytes, st));
    VSSR_HIP(h, hipMemsetAsync(W.V.info, 0, sizeof(int) * 4 * (size_t)ng, st));
    if (mode_in) {
        VSSR_HIP(h, hipMemcpyAsync(W.V.theta, mode_in, sizeof(double) * n3, hipMemcpyHostToDevice, st));
    } else {
        hipLaunchKernelGGL(k_dimer_draw, dim3(ng), dim3(256), 0, st, h->d_cfg_start.as<int>(), W.fixed, W.ids,
                           (uint32_t)(p->seed & 0xFFFFFFFFull), (uint32_t)(p->seed >> 32), W.V.theta);
    }
    hipLaunchKernelGGL(k_dimer_init, dim3(ng), dim3(256), 0, st, h->d_cfg_start.as<int>(), W.fixed, (double)p->displace, (double)p->delta,
                       (double)p->dt, (double)p->astart, h->d_pos.as<double>(), W.V, h->d_active.as<unsigned char>());
    VSSR_HIP(h, hipGetLastError());
    if (int rc = dimer_lockstep(h, W, want)) return rc;
    if (int rc = driver_close(h, false)) return rc;

    if (pos_out) VSSR_HIP(h, hipMemcpy(pos_out, h->d_pos.p, sizeof(double) * n3, hipMemcpyDeviceToHost));
    if (energy) VSSR_HIP(h, hipMemcpy(energy, chain_energy64(h), sizeof(double) * (size_t)B, hipMemcpyDeviceToHost));
    if (mode_out) VSSR_HIP(h, hipMemcpy(mode_out, W.V.N, sizeof(double) * n3, hipMemcpyDeviceToHost));
    if (dimer) VSSR_HIP(h, hipMemcpy(dimer, W.V.rec, sizeof(double) * 4 * (size_t)ng, hipMemcpyDeviceToHost));
    if (info) VSSR_HIP(h, hipMemcpy(info, W.V.info, sizeof(int) * 4 * (size_t)ng, hipMemcpyDeviceToHost));
    return VSSR_OK;
}
