// neb.hip — nudged elastic band over the resident batch, on every handle kind that evaluates: the improved-tangent NEB (Henkelman &
// Jonsson, J. Chem. Phys. 113, 9978 (2000)), ASE's `aseneb` variant, the climbing image (Henkelman, Uberuaga & Jonsson, J. Chem. Phys.
// 113, 9901 (2000)) and ASE's FIRE over the concatenated interior images of a band.  Restated from the papers and from ASE's neb.py /
// fire.py as remembered, NOT pinned by an executed ASE; the contract is the numpy restatement tests/neb_oracle.py.
// A BAND is n_img consecutive chains (its images).  The driver frame is lockstep.h's: one batch-wide evaluation per step, two
// launches behind it (one workgroup per chain each; state advances only in k_neb_step, so an evaluation repeated after a regrow
// moves nothing twice).
//   k_neb_project  an interior image reads its two neighbours' positions and the band's energies, forms t1, t2 and the tangent, writes
//                  G [3 N] and its partial sums (v.G, G.G, v.v, max |G_atom|^2, non-finite flag, zero-tangent flag) to its own slot;
//                  an end image writes zeros and its non-finite flag.
//   k_neb_step     every image reduces the slots of its band in image order (one thread, fixed order), so all images of a band hold
//                  the same band scalars without a third launch or a grid sync; every image carries its own copy of the band's FIRE
//                  state (nothing another workgroup writes is read in the same launch) and moves its own v and x.  The first
//                  interior image writes the band's outputs and counts the band as stopped.
// The FIRE update is fire_dev.h's, with the step length from the three sums.  Chains of a stopped band leave the evaluation through d_active, as in relax_lockstep; one last unmasked
// evaluation restores the complete graph where the mask was installed or a band went back to the positions its step opened at.
// Out of scope: other optimizers over the band, IDPP interpolation, free-end / string / eb / spline variants, per-spring constants,
// dynamic relaxation, a full minimum-image search, removal of rotation and translation, taking the end images out of the evaluation.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "arena.h"
#include "cg_dev.h"
#include "fire_dev.h"
#include "lockstep.h"
#include "neb_dev.h"

namespace vssr {

constexpr int NEB_SLOT = 8;   // doubles per image: v.G, G.G, v.v, max |G_atom|^2, non-finite, zero tangent, 2 spare

struct NebState {   // per chain: every image carries its band's state
    double dt, a;
    int nsteps_pos;  // steps since the last power <= 0 (ASE's Nsteps)
    int has_v;       // 0 until the first step
    int steps, reason, imax, pad;
};
struct NebParams {
    int max_steps, method, climb;
    double k, fmax;
    FireKnobs fire;
};
struct NebView {
    NebState *st;            // [B]
    const NebChain *ch;      // [B]
    double *vel, *xprev;     // [3 N] each: FIRE velocity; the positions the step in flight opened at
    double *G;               // [3 N] NEB force
    double *slot;            // [B][NEB_SLOT]
    double *band;            // [G][3]
    int *binfo;              // [G][4]
};

__global__ void k_neb_init(int B, double dt0, double astart, NebState *__restrict__ st, unsigned char *__restrict__ active) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    NebState S = {dt0, astart, 0, 0, 0, 0, 0, 0};
    st[b] = S;
    active[b] = 1;
}

// d = xb - xa of one atom, whole lattice vectors taken off along the periodic axes (I: rows of the transposed inverse cell)
__device__ __forceinline__ void neb_disp(const double *__restrict__ xa, const double *__restrict__ xb, const double *C, const double *I,
                                         const unsigned char *pb, double d[3]) {
    d[0] = xb[0] - xa[0]; d[1] = xb[1] - xa[1]; d[2] = xb[2] - xa[2];
    const double e0 = d[0], e1 = d[1], e2 = d[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!pb[a]) continue;
        const double n = rint(I[3 * a] * e0 + I[3 * a + 1] * e1 + I[3 * a + 2] * e2);
        if (n != 0.0) { d[0] -= n * C[3 * a]; d[1] -= n * C[3 * a + 1]; d[2] -= n * C[3 * a + 2]; }
    }
}

// Behind an evaluation of the batch: G and the partial sums of image b.  FT: double (d_pot_f) or float (PaiNN's forces, widened).
template <class FT>
__global__ void __launch_bounds__(256)
k_neb_project(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
              const FT *__restrict__ forces, const uint8_t *__restrict__ fixed, const double *__restrict__ cell,
              const double *__restrict__ invcell, const unsigned char *__restrict__ pbc, NebParams P, const double *__restrict__ pos,
              NebView V) {
    __shared__ double red[16];
    if (counters[2]) return;   // the evaluation overflowed the neighbor capacity: the host regrows and repeats it
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    if (V.st[b].reason) return;   // (this kernel stores no state)
    const NebChain c = V.ch[b];
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0;
    const FT *fg = forces + 3 * (size_t)a0;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;
    double *slot = V.slot + (size_t)NEB_SLOT * b;

    double bad = isfinite(energy[b]) ? 0.0 : 1.0;
    for (int t = tid; t < 3 * nat; t += nt)
        if (!isfinite((double)fg[t])) bad = 1.0;
    bad = block_max(bad, red);
    const bool interior = c.idx > 0 && c.idx < c.nimg - 1;
    if (!interior || bad != 0.0) {
        if (tid == 0) { slot[0] = 0.0; slot[1] = 0.0; slot[2] = 0.0; slot[3] = 0.0; slot[4] = bad; slot[5] = 0.0; }
        return;
    }
    const double Em = energy[b - 1], E0 = energy[b], Ep = energy[b + 1];
    int imax = 1;
    {
        double emax = energy[c.first + 1];
        for (int j = 2; j < c.nimg - 1; ++j) {
            const double e = energy[c.first + j];
            if (e > emax) { emax = e; imax = j; }
        }
    }
    const double *C = cell + 9 * (size_t)b, *I = invcell + 9 * (size_t)b;
    const unsigned char *pb = pbc + 3 * b;
    const double *x0 = pos + 3 * (size_t)a0;
    const double *xm = pos + 3 * (size_t)cfg_start[b - 1], *xp = pos + 3 * (size_t)cfg_start[b + 1];
    double *G = V.G + 3 * (size_t)a0;
    const double *v = V.vel + 3 * (size_t)a0;
    const bool climbing = P.climb && c.idx == imax;

    // the tangent t = al t2 + be t1 (before normalisation)
    double al, be;
    if (P.method == VSSR_NEB_IMPROVED_TANGENT) {
        if (Ep > E0 && E0 > Em) { al = 1.0; be = 0.0; }
        else if (Ep < E0 && E0 < Em) { al = 0.0; be = 1.0; }
        else {
            const double dp = fabs(Ep - E0), dm = fabs(Em - E0);
            const double dmax = fmax(dp, dm), dmin = fmin(dp, dm);
            if (Ep > Em) { al = dmax; be = dmin; } else { al = dmin; be = dmax; }
        }
    } else {
        al = c.idx <= imax ? 1.0 : 0.0;
        be = c.idx >= imax ? 1.0 : 0.0;
    }
    // pass 1: |t1|^2, |t2|^2, t.t, F.t, (k t1 - k t2).t with the raw tangent
    double s11 = 0.0, s22 = 0.0, tt = 0.0, ft = 0.0, st_ = 0.0;
    for (int i = tid; i < nat; i += nt) {
        double t1[3], t2[3];
        neb_disp(xm + 3 * i, x0 + 3 * i, C, I, pb, t1);
        neb_disp(x0 + 3 * i, xp + 3 * i, C, I, pb, t2);
        const bool held = fx && fx[i];
        for (int k = 0; k < 3; ++k) {
            const double t = al * t2[k] + be * t1[k];
            const double f = held ? 0.0 : (double)fg[3 * i + k];
            s11 += t1[k] * t1[k]; s22 += t2[k] * t2[k]; tt += t * t; ft += f * t;
            st_ += (P.k * t1[k] - P.k * t2[k]) * t;
        }
    }
    s11 = block_sum(s11, red);
    s22 = block_sum(s22, red);
    tt = block_sum(tt, red);
    // two coincident images: the tangent has no length, G = F there; the band stops (reason 4) unless it has converged as it stands
    const bool zt = !(tt > 0.0);
    double tn = 1.0, cf;
    if (zt) {
        cf = 0.0;
    } else if (P.method == VSSR_NEB_IMPROVED_TANGENT) {
        tn = sqrt(tt);
        double fpar = 0.0;   // F.(t / |t|), summed over the normalised tangent as the restatement does
        for (int i = tid; i < nat; i += nt) {
            if (fx && fx[i]) continue;
            double t1[3], t2[3];
            neb_disp(xm + 3 * i, x0 + 3 * i, C, I, pb, t1);
            neb_disp(x0 + 3 * i, xp + 3 * i, C, I, pb, t2);
            for (int k = 0; k < 3; ++k) fpar += (double)fg[3 * i + k] * ((al * t2[k] + be * t1[k]) / tn);
        }
        fpar = block_sum(fpar, red);
        cf = climbing ? -2.0 * fpar : -fpar + P.k * (sqrt(s22) - sqrt(s11));
    } else {
        ft = block_sum(ft, red);
        st_ = block_sum(st_, red);
        cf = climbing ? -2.0 * (ft / tt) : -(ft / tt) - st_ / tt;
    }
    double vG = 0.0, GG = 0.0, vv = 0.0, g2max = 0.0;
    for (int i = tid; i < nat; i += nt) {
        double t1[3], t2[3];
        neb_disp(xm + 3 * i, x0 + 3 * i, C, I, pb, t1);
        neb_disp(x0 + 3 * i, xp + 3 * i, C, I, pb, t2);
        const bool held = fx && fx[i];
        double g2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const double t = (al * t2[k] + be * t1[k]) / tn;
            const double g = held ? 0.0 : (double)fg[3 * i + k] + cf * t;
            const double vk = v[3 * i + k];
            G[3 * i + k] = g;
            vG += vk * g; GG += g * g; vv += vk * vk; g2 += g * g;
        }
        g2max = fmax(g2max, g2);
    }
    vG = block_sum(vG, red);
    GG = block_sum(GG, red);
    vv = block_sum(vv, red);
    g2max = block_max(g2max, red);
    const double gbad = isfinite(GG) ? 0.0 : 1.0;   // (a non-finite neighbour energy or position difference)
    if (tid == 0) { slot[0] = vG; slot[1] = GG; slot[2] = vv; slot[3] = g2max; slot[4] = gbad; slot[5] = zt ? 1.0 : 0.0; }
}

// Behind k_neb_project: the test and the FIRE step of the band, by every image for itself.  stopped: [0] bands stopped, [1] of those
// that went back to the positions their step opened at.
__global__ void __launch_bounds__(256)
k_neb_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
           const uint8_t *__restrict__ fixed, NebParams P, double *__restrict__ pos, NebView V, unsigned char *__restrict__ active,
           int *__restrict__ stopped) {
    __shared__ double sh[8];
    __shared__ int shi[2];
    if (counters[2]) return;   // nothing moves behind an overflowed evaluation
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    NebState S = V.st[b];
    __syncthreads();   // every wave holds the state before thread 0 can store the advanced one (cg_dev.h)
    if (S.reason) return;
    const NebChain c = V.ch[b];
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0;
    const bool interior = c.idx > 0 && c.idx < c.nimg - 1;
    const bool writer = c.idx == 1;   // the first interior image speaks for the band
    double *x = pos + 3 * (size_t)a0, *xp = V.xprev + 3 * (size_t)a0, *v = V.vel + 3 * (size_t)a0;
    const double *G = V.G + 3 * (size_t)a0;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;

    if (tid == 0) {   // the band's scalars, in image order: the same bits in every image of the band
        double vG = 0.0, GG = 0.0, vv = 0.0, fm2 = 0.0, bad = 0.0, zt = 0.0;
        for (int j = 0; j < c.nimg; ++j) {
            const double *s = V.slot + (size_t)NEB_SLOT * (c.first + j);
            if (s[4] != 0.0) bad = 1.0;
            if (j == 0 || j == c.nimg - 1) continue;
            vG += s[0]; GG += s[1]; vv += s[2]; fm2 = fmax(fm2, s[3]);
            if (s[5] != 0.0) zt = 1.0;
        }
        int imax = 1;
        double emax = energy[c.first + 1];
        for (int j = 2; j < c.nimg - 1; ++j) {
            const double e = energy[c.first + j];
            if (e > emax) { emax = e; imax = j; }
        }
        sh[0] = vG; sh[1] = GG; sh[2] = vv; sh[3] = fm2; sh[4] = bad; sh[5] = zt;
        sh[6] = emax - energy[c.first]; sh[7] = emax - energy[c.first + c.nimg - 1];
        shi[0] = imax;
    }
    __syncthreads();
    const double vG = sh[0], GG = sh[1], vv = sh[2], fm2 = sh[3];
    const bool bad = sh[4] != 0.0, zt = sh[5] != 0.0;

    auto stop = [&](int reason, int went_back) {
        if (tid == 0) {
            S.reason = reason;
            V.st[b] = S;
            active[b] = 0;
            if (writer) { atomicAdd(stopped, 1); if (went_back) atomicAdd(stopped + 1, 1); }
        }
    };
    if (bad) {   // nothing sane to follow: back to the positions the step opened at (an evaluation with no step taken is there already)
        const int back = S.has_v;
        if (back) {
            if (interior)
                for (int t = tid; t < 3 * nat; t += nt) x[t] = xp[t];
            S.steps -= 1;
        }
        stop(3, back);
        return;
    }
    if (tid == 0 && writer) {
        V.band[3 * c.band] = sqrt(fm2); V.band[3 * c.band + 1] = sh[6]; V.band[3 * c.band + 2] = sh[7];
    }
    S.imax = shi[0];
    if (fm2 < P.fmax * P.fmax) { stop(1, 0); return; }
    if (zt) { stop(4, 0); return; }
    if (S.steps >= P.max_steps) { stop(2, 0); return; }
    // ASE FIRE on the band: v' = c1 v + c2 G
    const FireMix M = fire_update(S, P.fire, vG, GG, vv);
    const double scale = fire_step_scale(S.dt, M, P.fire, vG, GG, vv);
    if (interior)
        for (int i = tid; i < nat; i += nt) {
            const bool held = fx && fx[i];
            for (int k = 0; k < 3; ++k) {
                const int t = 3 * i + k;
                xp[t] = x[t];
                if (held) continue;
                double vk = M.mix ? (1.0 - M.mix_a) * v[t] + M.mix_s * G[t] : 0.0;
                vk += S.dt * G[t];
                v[t] = vk;
                x[t] += scale * (S.dt * vk);
            }
        }
    if (tid == 0) {
        S.has_v = 1;
        S.steps += 1;
        V.st[b] = S;
    }
}

__global__ void k_neb_report(int nb, const int *__restrict__ gfirst, const NebState *__restrict__ st, int *__restrict__ info) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nb) return;
    const NebState S = st[gfirst[g] + 1];
    info[4 * g] = S.steps; info[4 * g + 1] = S.reason; info[4 * g + 2] = S.imax; info[4 * g + 3] = 0;
}

// The call's workspace: FIRE state and vectors on the handle's optimizer buffers (as FireWork), G / slots / band records in d_neb
struct NebWork {
    NebView V;
    NebParams P;
    const uint8_t *fixed;   // the mask on the device (null: all free)
    NebChain *ch;
    int *gfirst, *flags;    // flags: [0] bands stopped, [1] of those that went back, [2] image mismatch
    int nb;
};

static void neb_launch(vssr_handle *h, const NebWork &W) {
    hipStream_t st = h->stream;
    const int B = h->n_cfg;
    h->prof.begin(KC_NEB_PROJECT, st);
    with_forces(h, [&](const double *energy, auto *forces) {
        hipLaunchKernelGGL(k_neb_project<force_type<decltype(forces)>>, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(),
                           h->d_counters.as<int>(), energy, forces, W.fixed, h->d_cell.as<double>(), h->d_invcell.as<double>(),
                           h->d_pbc.as<unsigned char>(), W.P, h->d_pos.as<double>(), W.V);
    });
    h->prof.end(st);
    h->prof.begin(KC_NEB_STEP, st);
    hipLaunchKernelGGL(k_neb_step, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(), h->d_counters.as<int>(), chain_energy64(h), W.fixed,
                       W.P, h->d_pos.as<double>(), W.V, h->d_active.as<unsigned char>(), W.flags);
    h->prof.end(st);
}

static int neb_lockstep(vssr_handle *h, const NebWork &W, uint32_t want) {
    // evaluations a band needs: one per step and the last test.  A band that went back to the positions its step opened at asks
    // for the closing evaluation.
    LockstepPlan plan{8, (long long)W.P.max_steps + 1, LOCKSTEP_MASK_AT_STOP};
    plan.stopped = W.flags; plan.groups = W.nb;
    bool finished;
    if (int rc = lockstep_run(h, plan, want, finished, [&] { neb_launch(h, W); })) return rc;
    if (!finished) return set_err(h, VSSR_E_DEVICE, "vssr_batch_neb: the band loop did not finish");
    return VSSR_OK;
}

}  // namespace vssr

using namespace vssr;

extern "C" int vssr_batch_neb(vssr_handle *h, const vssr_neb_params *p, const uint8_t *fixed, const int32_t *n_img, int32_t n_bands,
                              uint32_t want, double *pos_out, double *energy, double *neb_force, double *band, int32_t *info) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!p) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: null parameters");
    if (!n_img) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: null n_img");
    if (n_bands < 1) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: n_bands %d < 1", (int)n_bands);
    if (p->method != VSSR_NEB_IMPROVED_TANGENT && p->method != VSSR_NEB_ASENEB)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: method %d is neither VSSR_NEB_IMPROVED_TANGENT (0) nor VSSR_NEB_ASENEB (1)", (int)p->method);
    if (p->climb != 0 && p->climb != 1) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: climb %d is neither 0 nor 1", (int)p->climb);
    if (p->max_steps < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: max_steps %d < 0", (int)p->max_steps);
    auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (!positive(p->k)) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: spring constant k %g eV/A^2 (finite and > 0 wanted)", p->k);
    if (!positive(p->fmax)) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: fmax %g eV/A (finite and > 0 wanted)", p->fmax);
    const FireKnobs fire{p->dtmax, p->finc, p->fdec, p->astart, p->fa, p->maxstep, p->nmin};
    if (int rc = fire_check(h, __func__, p->dt, fire)) return rc;
    const int B = h->n_cfg, N = h->n_atoms, nb = n_bands;
    {
        long long sum = 0;
        for (int g = 0; g < nb; ++g) {
            if (n_img[g] < 3) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: band %d has %d images (>= 3 wanted)", g, (int)n_img[g]);
            sum += n_img[g];
            if (sum > B) break;
        }
        if (sum != B) return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: n_img does not sum to the %d chains of the batch", B);
    }
    std::vector<NebChain> ch(B);
    std::vector<int> gfirst(nb);
    for (int g = 0, b = 0; g < nb; ++g) {
        gfirst[g] = b;
        const int f = b, f0 = h->h_cfg_start[f], nat = h->h_n_atoms[f];
        for (int k = 0; k < n_img[g]; ++k, ++b) {
            if (h->h_n_atoms[b] != nat)
                return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: chain %d is no image of the band of chain %d (atom counts)", b, f);
            if (fixed)
                for (int i = 0; i < nat; ++i)
                    if ((fixed[h->h_cfg_start[b] + i] != 0) != (fixed[f0 + i] != 0))
                        return set_err(h, VSSR_E_BADARG, "vssr_batch_neb: chain %d is no image of the band of chain %d (fixed mask)", b, f);
            ch[b] = {f, k, (int)n_img[g], g};
        }
    }

    VSSR_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    VSSR_HIP(h, hipStreamSynchronize(st));
    const size_t n3 = 3 * (size_t)N;
    NebWork W;
    size_t dbl_bytes = 0;   // the doubles at the head of d_neb, cleared in one piece
    auto layout = [&](Arena &a) {
        a.place(W.V.G, n3); a.place(W.V.slot, (size_t)NEB_SLOT * B); a.place(W.V.band, 3 * (size_t)nb);
        dbl_bytes = a.offset();
        a.place(W.ch, (size_t)B); a.place(W.V.binfo, 4 * (size_t)nb); a.place(W.gfirst, (size_t)nb); a.place(W.flags, 4);
    };
    if (h->d_neb.ensure(arena_size(layout)) || h->d_opt_state.ensure(sizeof(NebState) * (size_t)B) ||
        h->d_opt_vec.ensure(sizeof(double) * 2 * n3))
        return set_err(h, VSSR_E_NOMEM, "nudged elastic band workspace: out of device memory");
    arena_carve(h->d_neb.p, layout);
    W.V.ch = W.ch;
    W.V.st = h->d_opt_state.as<NebState>();
    W.V.vel = h->d_opt_vec.as<double>(); W.V.xprev = W.V.vel + n3;
    W.nb = nb;
    W.P = {p->max_steps, p->method, p->climb, p->k, p->fmax, fire};
    VSSR_HIP(h, hipMemcpyAsync(W.gfirst, gfirst.data(), sizeof(int) * nb, hipMemcpyHostToDevice, st));
    if (int rc = neb_compare_groups(h, ch, W.ch, W.flags,
                                    "vssr_batch_neb: the images of a band differ in more than positions (species, cell or pbc; the comparison is bitwise)"))
        return rc;

    W.fixed = nullptr;
    if (int rc = driver_open(h, fixed, 2, W.fixed, want)) return rc;
    VSSR_HIP(h, hipMemsetAsync(W.V.vel, 0, sizeof(double) * 2 * n3, st));
    VSSR_HIP(h, hipMemsetAsync(W.V.G, 0, dbl_bytes, st));
    hipLaunchKernelGGL(k_neb_init, dim3((B + 127) / 128), dim3(128), 0, st, B, (double)p->dt, (double)p->astart, W.V.st,
                       h->d_active.as<unsigned char>());
    VSSR_HIP(h, hipGetLastError());
    if (int rc = neb_lockstep(h, W, want)) return rc;
    hipLaunchKernelGGL(k_neb_report, dim3((nb + 127) / 128), dim3(128), 0, st, nb, W.gfirst, W.V.st, W.V.binfo);
    VSSR_HIP(h, hipGetLastError());
    if (int rc = driver_close(h, false)) return rc;

    if (pos_out) VSSR_HIP(h, hipMemcpy(pos_out, h->d_pos.p, sizeof(double) * n3, hipMemcpyDeviceToHost));
    if (energy) VSSR_HIP(h, hipMemcpy(energy, chain_energy64(h), sizeof(double) * (size_t)B, hipMemcpyDeviceToHost));
    if (neb_force) VSSR_HIP(h, hipMemcpy(neb_force, W.V.G, sizeof(double) * n3, hipMemcpyDeviceToHost));
    if (band) VSSR_HIP(h, hipMemcpy(band, W.V.band, sizeof(double) * 3 * (size_t)nb, hipMemcpyDeviceToHost));
    if (info) VSSR_HIP(h, hipMemcpy(info, W.V.binfo, sizeof(int) * 4 * (size_t)nb, hipMemcpyDeviceToHost));
    return VSSR_OK;
}
