// md_npt.hip -- constant-pressure and weakly-coupled molecular dynamics of the resident batch (vssr_batch_md_npt): the Berendsen
// thermostat and barostat (isotropic or per axis, ASE's NVTBerendsen / NPTBerendsen / Inhomogeneous_NPTBerendsen) and stochastic cell
// rescaling (Bernetti & Bussi, J. Chem. Phys. 153, 114107 (2020), isotropic, Euler form) around the velocity-Verlet / Langevin BAOAB
// step of md_dev.h.  Restated from ASE and from the paper as remembered, NOT pinned by an executed library: the contract is the header
// comment of vssr_batch_md_npt and the numpy restatement tests/npt_oracle.py.
//
// Lock step only (the driver frame is lockstep.h's): one batch-wide evaluation per time step, with a barostat the kind's stress kernels
// behind it (as relax_cell.hip: nothing else consumes a stress on the device), then ONE launch, k_npt_step: one 256-thread workgroup
// per chain closes the step in flight, records, rescales velocities, cell and positions, opens the next step and writes the chain's
// d_pos, d_cell, d_invcell and d_nimg (cell_dev.h: the formulas of vssr_batch_upload).  The neighbor list is rebuilt at every
// evaluation, so the evaluation kernels never learn that the cell changed; what the host sized from the uploaded cells stays valid
// because a step is only taken if its new cell needs no more periodic images along any axis than the chain had when the call began.
// With a barostat the evaluation is never masked (LOCKSTEP_MASK_NEVER: the stress kernels are not written for a masked batch);
// without one no stress kernel is launched at all and the plan is md_lockstep's.  Reductions are block_sum / block_max in a fixed
// order, no floating-point atomics: a chain gives the same bits alone and inside any batch.  The atom update is md_step_chain's,
// expression for expression (with no thermostat or Langevin and no barostat the call leaves the bits of vssr_batch_md).
// Out of scope: the chain-resident driver (vssr_batch_md_driver does not apply here), full-tensor (shear) cell coupling, anisotropic
// stochastic cell rescaling, Nose-Hoover / MTK chains, pair handles with k-space under a barostat, centre-of-mass removal.
#include <cmath>
#include <vector>
#include "arena.h"
#include "cell_dev.h"
#include "lockstep.h"
#include "md_dev.h"

namespace vssr {

enum { NPT_TAG_CRESCALE = 3 };   // draw tag of the cell noise (md_dev.h: MD uses 0 and 1, the dimer 2)

struct NptParams {
    int n_steps, thermostat, barostat, coupling, thermo_interval, B;   // B: chains of the batch (row stride of the thermo records)
    int mask[3];
    double dt, t0, t1, c1, c2, taut, taup, p0, beta, cutoff;
    long long ramp_steps, step0;
    uint32_t seed_lo, seed_hi;
};
struct NptState {   // per chain
    int steps, reason, open, pad;   // open: a step is in flight (positions moved, the closing half kick is due)
    int nimg0[3], pad2;             // image counts when the call began: no step may exceed them
    double cell_prev[9];            // the cell the step in flight opened at
};
struct NptView {
    NptState *st;
    double *vel;                 // [3 N], the handle's resident velocities
    double *r_prev, *v_prev;     // [3 N] each: the state the step in flight opened at
    const double *mass;          // [N] amu
    const unsigned long long *chain_id;   // [B]
    double *thermo;              // [n_steps / thermo_interval + 1][B][4]
    int *info;                   // [B][2]: steps completed, stop reason
};

__device__ __forceinline__ double npt_det3(const double *m) {   // (the expression of virial_dev.h's volume)
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// every chain at step 0 of this call; held atoms carry no velocity, whatever the caller set
__global__ void __launch_bounds__(256)
k_npt_init(const int *__restrict__ cfg_start, const uint8_t *__restrict__ fixed, const double *__restrict__ cell,
           const int *__restrict__ nimg, NptView V, unsigned char *__restrict__ active) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int a0 = cfg_start[b], a1 = cfg_start[b + 1];
    if (fixed)
        for (int i = a0 + tid; i < a1; i += blockDim.x)
            if (fixed[i]) { V.vel[3 * (size_t)i] = 0.0; V.vel[3 * (size_t)i + 1] = 0.0; V.vel[3 * (size_t)i + 2] = 0.0; }
    if (tid == 0) {
        NptState S = {};
        for (int k = 0; k < 3; ++k) S.nimg0[k] = nimg[3 * (size_t)b + k];
        for (int k = 0; k < 9; ++k) S.cell_prev[k] = cell[9 * (size_t)b + k];
        V.st[b] = S;
        V.info[2 * b] = 0; V.info[2 * b + 1] = 0;
        active[b] = 1;
    }
}

// Behind an evaluation of the batch (and, with a barostat, its stress): one visit of chain b, the numbered steps of the header
// comment.  FT: double (d_pot_f) or float (PaiNN's forces, widened).  stress: [B][6] Voigt (PaiNN: the ensemble mean), null without
// a barostat.  Every vector loop is strided by ATOM with the same stride, so a thread only ever reads elements it wrote itself; the
// scalars all threads branch on come from the loaded state and from block reductions, which hand every thread the same bits.
// stopped: [0] chains that stopped, [1] of those with reason 2 (they need the closing evaluation).
template <class FT>
__global__ void __launch_bounds__(256)
k_npt_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
           const FT *__restrict__ forces, const double *__restrict__ stress, const uint8_t *__restrict__ fixed,
           const uint8_t *__restrict__ pbc_all, NptParams P, double *__restrict__ pos, double *__restrict__ cell,
           double *__restrict__ invcell, int *__restrict__ nimg, NptView V, unsigned char *__restrict__ active,
           int *__restrict__ stopped) {
    __shared__ double red[16];
    if (counters[2]) return;   // the evaluation overflowed the neighbor capacity: nothing moves, the host regrows and repeats it
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    NptState S = V.st[b];
    double C[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) C[k] = cell[9 * (size_t)b + k];
    __syncthreads();   // every wave holds the state and the cell before thread 0 can store the advanced ones (cg_dev.h)
    if (S.reason) return;
    const bool baro = P.barostat != VSSR_NPT_BAROSTAT_NONE;
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0;
    double *x = pos + 3 * (size_t)a0, *v = V.vel + 3 * (size_t)a0, *xp = V.r_prev + 3 * (size_t)a0, *vp = V.v_prev + 3 * (size_t)a0;
    const double *m = V.mass + a0;
    const FT *fg = forces + 3 * (size_t)a0;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;
    const uint8_t pbc[3] = {pbc_all[3 * b], pbc_all[3 * b + 1], pbc_all[3 * b + 2]};
    const double *sg = baro ? stress + 6 * (size_t)b : nullptr;

    auto write_cell = [&](const double *Cw, const double *inv, const int *ni) {   // thread 0
#pragma unroll
        for (int k = 0; k < 9; ++k) { cell[9 * (size_t)b + k] = Cw[k]; invcell[9 * (size_t)b + k] = inv[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) nimg[3 * (size_t)b + k] = ni[k];
    };
    auto store = [&](int stop, int refresh) {   // thread 0: the advanced state; stop: the chain is switched off
        V.st[b] = S;
        V.info[2 * b] = S.steps; V.info[2 * b + 1] = S.reason;
        if (stop) {
            active[b] = 0;
            atomicAdd(stopped, 1);
            if (refresh) atomicAdd(stopped + 1, 1);
        }
    };

    // 1. finite?
    const double E = energy[b];
    double bad = isfinite(E) ? 0.0 : 1.0;
    for (int i = tid; i < nat; i += nt) {
        const double f0 = (double)fg[3 * i], f1 = (double)fg[3 * i + 1], f2 = (double)fg[3 * i + 2];
        if (!(isfinite(f0) && isfinite(f1) && isfinite(f2))) bad = 1.0;
    }
    if (baro && tid < 6 && !isfinite(sg[tid])) bad = 1.0;
    bad = block_max(bad, red);
    if (bad != 0.0) {   // back to the last completed step: positions, velocities and cell (an evaluation with no step in flight is there already)
        if (S.open) {
            for (int i = tid; i < nat; i += nt)
                for (int c = 0; c < 3; ++c) { x[3 * i + c] = xp[3 * i + c]; v[3 * i + c] = vp[3 * i + c]; }
            if (baro && tid == 0) {
                double inv[9];
                int ni[3];
                bool ok;
                cell_setup(S.cell_prev, pbc, P.cutoff, inv, ni, ok);
                write_cell(S.cell_prev, inv, ni);
            }
        }
        if (tid == 0) { S.open = 0; S.reason = 2; store(1, 1); }
        return;
    }
    const double hdt = 0.5 * P.dt;
    // 2. close the step in flight
    if (S.open) {
        for (int i = tid; i < nat; i += nt) {
            if (fx && fx[i]) continue;
            for (int c = 0; c < 3; ++c) v[3 * i + c] += hdt * (((double)fg[3 * i + c] / m[i]) * MD_ACC);
        }
        S.steps += 1; S.open = 0;
    }
    // one pass over the atoms: sum m v^2 (the expression of md_step_chain), the diagonal of sum m v v^T, the free atoms
    const bool record = S.steps % P.thermo_interval == 0;
    const bool berendsen_t = P.thermostat == VSSR_NPT_THERMOSTAT_BERENDSEN;
    double k = 0.0, kd[3] = {0.0, 0.0, 0.0}, nfree = 0.0;
    for (int i = tid; i < nat; i += nt) {
        const double v0 = v[3 * i], v1 = v[3 * i + 1], v2 = v[3 * i + 2];
        k += m[i] * (v0 * v0 + v1 * v1 + v2 * v2);
        kd[0] += m[i] * (v0 * v0); kd[1] += m[i] * (v1 * v1); kd[2] += m[i] * (v2 * v2);
        if (!(fx && fx[i])) nfree += 1.0;
    }
    if (record || berendsen_t) k = block_sum(k, red);
    if (berendsen_t) nfree = block_sum(nfree, red);
    if (baro) {
        kd[0] = block_sum(kd[0], red); kd[1] = block_sum(kd[1], red); kd[2] = block_sum(kd[2], red);
    }
    const double ekin = 0.5 * k / MD_ACC;
    const double vol = fabs(npt_det3(C));
    // 3. thermo record
    if (record && tid == 0) {
        double *rec = V.thermo + 4 * ((size_t)(S.steps / P.thermo_interval) * P.B + b);
        rec[0] = E; rec[1] = ekin; rec[2] = vol;
        rec[3] = baro ? ((-sg[0] + (kd[0] / MD_ACC) / vol) + (-sg[1] + (kd[1] / MD_ACC) / vol) + (-sg[2] + (kd[2] / MD_ACC) / vol)) / 3.0
                      : __longlong_as_double(0x7FF8000000000000LL);   // no stress was evaluated
    }
    // 4. finished
    if (S.steps == P.n_steps) {
        if (tid == 0) { S.reason = 1; store(1, 0); }
        return;
    }
    // 5. open step n
    const long long n = P.step0 + S.steps;
    uint32_t q0 = 0, q1 = 0;
    double kT = 0.0;
    if (P.thermostat != VSSR_NPT_THERMOSTAT_NONE) {
        const double T = n < P.ramp_steps ? P.t0 + (P.t1 - P.t0) * ((double)n / (double)P.ramp_steps) : P.t1;
        kT = MD_KB * T;
    }
    if (P.thermostat == VSSR_NPT_THERMOSTAT_LANGEVIN || P.barostat == VSSR_NPT_BAROSTAT_CRESCALE)
        md_chain_key(P.seed_lo, P.seed_hi, V.chain_id[b], q0, q1);
    // 5a. Berendsen thermostat: lambda
    double lam = 1.0;
    if (berendsen_t && ekin != 0.0 && nfree != 0.0) {
        const double kTkin = 2.0 * ekin / (3.0 * nfree);
        const double arg = 1.0 + (P.dt / P.taut) * (kT / kTkin - 1.0);
        lam = arg > 0.0 ? sqrt(arg) : 0.0;
        lam = fmin(fmax(lam, 0.9), 1.1);
    }
    // 5b. barostat: mu per Cartesian axis, the velocity divisor of the stochastic rescaling
    double mu[3] = {1.0, 1.0, 1.0}, vdiv = 1.0;
    double Cn[9], inv[9];
    int ni[3];
    if (baro) {
        const double l2 = lam * lam;
        const double Pi[3] = {-sg[0] + ((l2 * kd[0]) / MD_ACC) / vol, -sg[1] + ((l2 * kd[1]) / MD_ACC) / vol, -sg[2] + ((l2 * kd[2]) / MD_ACC) / vol};
        if (P.barostat == VSSR_NPT_BAROSTAT_CRESCALE) {
            const double Pint = (Pi[0] + Pi[1] + Pi[2]) / 3.0;
            double xi, unused;
            md_normal2(q0, q1, n, 0, NPT_TAG_CRESCALE, 0, xi, unused);
            const double deps = -(P.beta / P.taup) * (P.p0 - Pint) * P.dt + sqrt((((2.0 * kT) * P.beta) * P.dt) / (vol * P.taup)) * xi;
            const double s = exp(deps / 3.0);
            mu[0] = mu[1] = mu[2] = s; vdiv = s;
        } else {
            const double g = (P.dt * P.beta) / (3.0 * P.taup);
            if (P.coupling == VSSR_NPT_COUPLING_PER_AXIS) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (P.mask[c]) mu[c] = 1.0 - g * (P.p0 - Pi[c]);
            } else {
                double sum = 0.0;
                int cnt = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (P.mask[c]) { sum += Pi[c]; ++cnt; }
                const double s = 1.0 - g * (P.p0 - sum / (double)cnt);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (P.mask[c]) mu[c] = s;
            }
        }
        // 5c. the new cell C D: finite, det keeps its sign, no more images along any periodic axis than the call began with
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Cn[3 * r + c] = C[3 * r + c] * mu[c];
        const double d0 = npt_det3(C), d1 = npt_det3(Cn);
        bool sane = isfinite(d1) && ((d0 > 0.0 && d1 > 0.0) || (d0 < 0.0 && d1 < 0.0));
#pragma unroll
        for (int c = 0; c < 9; ++c) sane = sane && isfinite(Cn[c]);
        if (sane) {
            bool ok;
            cell_setup(Cn, pbc, P.cutoff, inv, ni, ok);
            sane = ok;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (pbc[c] && (ni[c] < 1 || ni[c] > S.nimg0[c])) sane = false;
        }
        if (!sane) {   // the step is not taken: the chain stays at the state this evaluation saw, which is complete
            if (tid == 0) { S.reason = 3; store(1, 0); }
            return;
        }
    }
    // 5d. integrate with the forces of this evaluation (positions and velocities saved first)
    const bool langevin = P.thermostat == VSSR_NPT_THERMOSTAT_LANGEVIN;
    for (int i = tid; i < nat; i += nt) {
        double xs[3], vs[3];
        for (int c = 0; c < 3; ++c) {
            xp[3 * i + c] = x[3 * i + c]; vp[3 * i + c] = v[3 * i + c];
            xs[c] = x[3 * i + c] * mu[c];
            vs[c] = (v[3 * i + c] * lam) / vdiv;
        }
        if (fx && fx[i]) {   // held atoms ride the cell
            for (int c = 0; c < 3; ++c) x[3 * i + c] = xs[c];
            continue;
        }
        if (langevin) {
            double z[3];
            md_normal3(q0, q1, n, i, MD_TAG_LANGEVIN, z);
            const double sigma = sqrt(P.c2 * kT * MD_ACC / m[i]);
            for (int c = 0; c < 3; ++c) {
                double vv = vs[c] + hdt * (((double)fg[3 * i + c] / m[i]) * MD_ACC);
                double xx = xs[c] + hdt * vv;
                vv = P.c1 * vv + sigma * z[c];
                xx += hdt * vv;
                v[3 * i + c] = vv; x[3 * i + c] = xx;
            }
        } else {
            for (int c = 0; c < 3; ++c) {
                const double vv = vs[c] + hdt * (((double)fg[3 * i + c] / m[i]) * MD_ACC);
                v[3 * i + c] = vv;
                x[3 * i + c] = xs[c] + P.dt * vv;
            }
        }
    }
    if (tid == 0) {
        if (baro) {
#pragma unroll
            for (int c = 0; c < 9; ++c) S.cell_prev[c] = C[c];
            write_cell(Cn, inv, ni);
        }
        S.open = 1;
        store(0, 0);
    }
}

struct NptWork {
    NptView V;
    NptParams P;
    const uint8_t *fixed;   // the mask on the device (null: all free)
    int *stopped;           // [2]: chains that stopped, of those with reason 2
    int nrec;
};

static int npt_lockstep(vssr_handle *h, const NptWork &W, uint32_t want) {
    const int B = h->n_cfg;
    const bool baro = W.P.barostat != VSSR_NPT_BAROSTAT_NONE;
    // evaluations a chain needs: the initial state and one per step (md_lockstep).  The stress kernels are not written for a masked batch.
    LockstepPlan plan{8, (long long)W.P.n_steps + 1, baro ? LOCKSTEP_MASK_NEVER : LOCKSTEP_MASK_AT_STOP};
    plan.stopped = W.stopped; plan.groups = B;
    int launch_rc = VSSR_OK;
    bool finished;
    int rc = lockstep_run(h, plan, want, finished,
        [&] {
            if (launch_rc || (baro && (launch_rc = evaluator(h).stress(h)))) return;   // (seen at the next poll)
            with_forces(h, [&](const double *energy, auto *forces) {
                hipLaunchKernelGGL(k_npt_step<force_type<decltype(forces)>>, dim3(B), dim3(256), 0, h->stream, h->d_cfg_start.as<int>(),
                                   h->d_counters.as<int>(), energy, forces, baro ? h->d_stress.as<double>() : nullptr, W.fixed,
                                   h->d_pbc.as<uint8_t>(), W.P, h->d_pos.as<double>(), h->d_cell.as<double>(), h->d_invcell.as<double>(),
                                   h->d_nimg.as<int>(), W.V, h->d_active.as<unsigned char>(), W.stopped);
            });
        },
        [&](bool) { return launch_rc; });
    return rc ? rc : launch_rc;
}

// A barostat moves lattice vectors along the Cartesian axes of its mask.  An open axis k is served where lattice vector k lies along
// one Cartesian axis m, the other two have no component along m (the rule of vssr_batch_relax_cell) and m is masked out: the vacuum
// direction then stays out of the rescaling exactly.  (From the resident cells: an earlier call may have changed them.)
static int npt_open_axes_ok(vssr_handle *h, const vssr_npt_params *p) {
    const int B = h->n_cfg;
    std::vector<double> cell((size_t)9 * B);
    std::vector<uint8_t> pbc((size_t)3 * B);
    VSSR_HIP(h, hipMemcpy(cell.data(), h->d_cell.p, sizeof(double) * cell.size(), hipMemcpyDeviceToHost));
    VSSR_HIP(h, hipMemcpy(pbc.data(), h->d_pbc.p, pbc.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 3; ++k) {
            if (pbc[3 * b + k]) continue;
            if (p->barostat == VSSR_NPT_BAROSTAT_CRESCALE)
                return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: stochastic cell rescaling is isotropic, but chain %d is open along axis %d", b, k);
            const double *c = cell.data() + 9 * (size_t)b;
            int m = -1, nz = 0;
            for (int x = 0; x < 3; ++x)
                if (c[3 * k + x] != 0.0) { m = x; ++nz; }
            if (nz != 1)
                return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: chain %d is open along axis %d, whose lattice vector (%g %g %g) does not lie "
                               "along one Cartesian axis", b, k, c[3 * k], c[3 * k + 1], c[3 * k + 2]);
            for (int r = 0; r < 3; ++r)
                if (r != k && c[3 * r + m] != 0.0)
                    return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: chain %d is open along axis %d (Cartesian %d), but lattice vector %d has "
                                   "the component %g along it", b, k, m, r, c[3 * r + m]);
            if (p->mask[m])
                return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: chain %d is open along axis %d (Cartesian %d), but mask[%d] couples that "
                               "direction to the barostat", b, k, m, m);
        }
    return VSSR_OK;
}

}  // namespace vssr

using namespace vssr;

extern "C" int vssr_batch_md_npt(vssr_handle *h, const vssr_npt_params *p, const double *mass, const uint8_t *fixed, const uint64_t *chain_id,
                                 uint32_t want, double *pos_out, double *cell_out, double *thermo, int32_t *n_done, int32_t *stop_reason) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!p) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: null parameters");
    const bool thermo_on = p->thermostat != VSSR_NPT_THERMOSTAT_NONE, baro = p->barostat != VSSR_NPT_BAROSTAT_NONE;
    if (p->thermostat < VSSR_NPT_THERMOSTAT_NONE || p->thermostat > VSSR_NPT_THERMOSTAT_BERENDSEN)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: thermostat %d is none of VSSR_NPT_THERMOSTAT_NONE (0), _LANGEVIN (1), _BERENDSEN (2)", (int)p->thermostat);
    if (p->barostat < VSSR_NPT_BAROSTAT_NONE || p->barostat > VSSR_NPT_BAROSTAT_CRESCALE)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: barostat %d is none of VSSR_NPT_BAROSTAT_NONE (0), _BERENDSEN (1), _CRESCALE (2)", (int)p->barostat);
    if (p->coupling != VSSR_NPT_COUPLING_ISOTROPIC && p->coupling != VSSR_NPT_COUPLING_PER_AXIS)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: coupling %d is neither VSSR_NPT_COUPLING_ISOTROPIC (0) nor _PER_AXIS (1)", (int)p->coupling);
    if (baro && !evaluator(h).stress) return set_err(h, VSSR_E_STATE, "vssr_batch_md_npt: this handle serves no stress");
    if (baro && h->ew_on)
        return set_err(h, VSSR_E_STATE, "vssr_batch_md_npt: a pair handle with k-space is not served: the S(k) stride (ew_stride = %d reciprocal "
                       "cells per chain) was sized from the uploaded cells and a changed cell may exceed it", h->ew_stride);
    if (p->n_steps < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: n_steps %d < 0", (int)p->n_steps);
    if (p->thermo_interval < 1) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: thermo_interval %d < 1", (int)p->thermo_interval);
    {
        const double vals[8] = {p->dt, p->temperature, p->temperature_end, p->friction, p->taut, p->taup, p->pressure, p->compressibility};
        static const char *const names[8] = {"dt", "temperature", "temperature_end", "friction", "taut", "taup", "pressure", "compressibility"};
        for (int k = 0; k < 8; ++k)
            if (!std::isfinite(vals[k])) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: %s %g is not finite", names[k], vals[k]);
    }
    if (!(p->dt > 0.0)) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: dt %g fs (> 0 wanted)", p->dt);
    if (thermo_on) {
        if (!(p->temperature >= 0.0 && p->temperature_end >= 0.0))
            return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: temperatures %g K, %g K (>= 0 wanted)", p->temperature, p->temperature_end);
        if (p->ramp_steps < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: ramp_steps %lld < 0", (long long)p->ramp_steps);
    }
    if (p->thermostat == VSSR_NPT_THERMOSTAT_LANGEVIN && !(p->friction > 0.0))
        return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: Langevin friction %g 1/fs (> 0 wanted)", p->friction);
    if (p->thermostat == VSSR_NPT_THERMOSTAT_BERENDSEN && !(p->taut > 0.0))
        return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: Berendsen taut %g fs (> 0 wanted)", p->taut);
    for (int k = 0; k < 3; ++k)
        if (p->mask[k] != 0 && p->mask[k] != 1) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: mask[%d] = %d (0 or 1 wanted)", k, (int)p->mask[k]);
    if (baro) {
        if (!(p->taup > 0.0)) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: barostat taup %g fs (> 0 wanted)", p->taup);
        if (!(p->compressibility > 0.0))
            return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: compressibility %g A^3/eV (> 0 wanted)", p->compressibility);
        const int n_mask = p->mask[0] + p->mask[1] + p->mask[2];
        if (n_mask == 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: a barostat with an empty mask");
        if (p->barostat == VSSR_NPT_BAROSTAT_CRESCALE) {
            if (!thermo_on) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: stochastic cell rescaling needs a thermostat (its noise has a temperature)");
            if (p->coupling != VSSR_NPT_COUPLING_ISOTROPIC) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: stochastic cell rescaling is isotropic only (coupling PER_AXIS)");
            if (n_mask != 3) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_npt: stochastic cell rescaling is isotropic only (mask %d %d %d)", (int)p->mask[0], (int)p->mask[1], (int)p->mask[2]);
        }
    }
    if (int rc = md_masses_ok(h, __func__, mass)) return rc;
    if (!h->md_vel_valid)
        return set_err(h, VSSR_E_STATE, "vssr_batch_md_npt: the resident batch has no velocities (vssr_batch_md_set_velocities / _draw_velocities)");
    VSSR_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    VSSR_HIP(h, hipStreamSynchronize(st));
    if (baro)
        if (int rc = npt_open_axes_ok(h, p)) return rc;

    const size_t B = h->n_cfg, N = h->n_atoms, n3 = 3 * N;
    NptWork W;
    W.nrec = p->n_steps / p->thermo_interval + 1;
    double *d_mass;
    unsigned long long *d_ids;
    auto layout = [&](Arena &a) {
        a.place(W.V.r_prev, n3); a.place(W.V.v_prev, n3); a.place(d_mass, N); a.place(W.V.thermo, 4 * B * (size_t)W.nrec);
        a.place(d_ids, B); a.place(W.V.st, B); a.place(W.V.info, 2 * B); a.place(W.stopped, 4);
    };
    if (h->d_npt.ensure(arena_size(layout)) || (baro && h->d_stress.ensure(sizeof(double) * 12 * B)))
        return set_err(h, VSSR_E_NOMEM, "constant-pressure MD workspace: out of device memory");
    arena_carve(h->d_npt.p, layout);
    W.V.vel = h->d_md_vel.as<double>(); W.V.mass = d_mass; W.V.chain_id = d_ids;
    const bool langevin = p->thermostat == VSSR_NPT_THERMOSTAT_LANGEVIN;
    const double c1 = langevin ? std::exp(-p->friction * p->dt) : 1.0;
    W.P = {p->n_steps, p->thermostat, p->barostat, p->coupling, p->thermo_interval, (int)B, {p->mask[0], p->mask[1], p->mask[2]},
           p->dt, p->temperature, p->temperature_end, c1, 1.0 - c1 * c1, p->taut, p->taup, p->pressure, p->compressibility,
           evaluator(h).cutoff(h), thermo_on ? (long long)p->ramp_steps : 0LL, (long long)p->step0, (uint32_t)p->seed, (uint32_t)(p->seed >> 32)};

    W.fixed = nullptr;
    if (int rc = driver_open(h, fixed, 2, W.fixed, want)) return rc;
    if (baro) h->ran = false;   // (until the loop has left a complete evaluation: a failure in between leaves moved cells behind)
    std::vector<unsigned long long> ids(B);
    for (size_t b = 0; b < B; ++b) ids[b] = chain_id ? (unsigned long long)chain_id[b] : (unsigned long long)b;
    VSSR_HIP(h, hipMemcpyAsync(d_ids, ids.data(), sizeof(unsigned long long) * B, hipMemcpyHostToDevice, st));
    VSSR_HIP(h, hipMemcpyAsync(d_mass, mass, sizeof(double) * N, hipMemcpyHostToDevice, st));
    VSSR_HIP(h, hipMemsetAsync(W.stopped, 0, 16, st));
    VSSR_HIP(h, hipMemsetAsync(W.V.thermo, 0xFF, sizeof(double) * 4 * B * (size_t)W.nrec, st));   // records a chain never reaches read as NaN
    hipLaunchKernelGGL(k_npt_init, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(), W.fixed, h->d_cell.as<double>(), h->d_nimg.as<int>(),
                       W.V, h->d_active.as<unsigned char>());
    VSSR_HIP(h, hipGetLastError());
    VSSR_HIP(h, hipStreamSynchronize(st));   // (ids leaves scope with the call, mass is the caller's)
    if (int rc = npt_lockstep(h, W, want)) return rc;
    if (int rc = driver_close(h, false)) return rc;

    if (pos_out) VSSR_HIP(h, hipMemcpy(pos_out, h->d_pos.p, sizeof(double) * n3, hipMemcpyDeviceToHost));
    if (cell_out) VSSR_HIP(h, hipMemcpy(cell_out, h->d_cell.p, sizeof(double) * 9 * B, hipMemcpyDeviceToHost));
    if (thermo) VSSR_HIP(h, hipMemcpy(thermo, W.V.thermo, sizeof(double) * 4 * B * (size_t)W.nrec, hipMemcpyDeviceToHost));
    if (n_done || stop_reason) {
        std::vector<int> info(2 * B);
        VSSR_HIP(h, hipMemcpy(info.data(), W.V.info, sizeof(int) * info.size(), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) {
            if (n_done) n_done[b] = info[2 * b];
            if (stop_reason) stop_reason[b] = info[2 * b + 1];
        }
    }
    return VSSR_OK;
}
