// relax_cell.hip -- variable-cell relaxation of the resident batch on the device, on every handle kind that evaluates and serves a
// stress (all but pair handles with k-space): ASE's UnitCellFilter (ase/filters.py) under ASE's FIRE (ase/optimize/fire.py), batched over
// the chains, in fp64.  Restated from ASE as remembered; ASE is not installed where this was written, so this is NOT pinned by an
// executed ASE: the contract is the header comment of vssr_batch_relax_cell and the numpy restatement tests/cellrelax_oracle.py, whose
// row force tests/test_cellrelax_cpu.py checks to be the exact negative gradient of the enthalpy E + p V.
//
// Row vectors; cell rows are lattice vectors.  Per chain, fixed when the call starts: the cell C0 and c = cell_factor (default: the
// atom count).  State: s [N][3] and the deformation gradient F [3][3], from s = x and F = I; the physical state is x = s F^T,
// C = C0 F^T.  The optimizer sees N + 3 rows: s and c F.  The driver frame is lockstep.h's: one batch-wide evaluation per visit, the
// kind's stress kernels behind it (nothing else consumes a stress on the device), then ONE launch, k_cell_step: one 256-thread
// workgroup per chain forms the row forces, runs ASE's convergence test over all N + 3 rows and one FIRE step (fire_dev.h) over the
// 3 N + 9 numbers, and writes the chain's d_pos, d_cell, d_invcell and d_nimg (cell_dev.h: the formulas of vssr_batch_upload).  The
// neighbor list is rebuilt at every evaluation, so the evaluation kernels never learn that the cell changed.
// What the host sized from the uploaded cells stays valid because a step is only taken if its new cell needs no more periodic images
// along any axis than the upload gave that chain (h->max_images, the 64-bit hit masks); otherwise, or with det F <= 0 or a non-finite
// cell, the chain stops with reason 4 where it stands.  Pair handles with k-space are refused: ew_stride sizes d_ew_S from the
// uploaded cells.  The evaluation is never masked (LOCKSTEP_MASK_NEVER: the stress kernels are not written for a masked batch); chains
// that stopped simply stop moving.  Reductions are block_sum / block_max in a fixed order, no floating-point atomics: a chain gives the
// same bits alone and inside any batch.
// Out of scope: constant_volume, ExpCellFilter / FrechetCellFilter, other optimizers over the filter, trajectory rings, k-space handles.
// (Cells that move under a barostat at finite temperature: md_npt.hip.)
#include <cmath>
#include <vector>

#include "arena.h"
#include "cell_dev.h"
#include "cg_dev.h"
#include "fire_dev.h"
#include "lockstep.h"

namespace vssr {

struct CellState {   // per chain
    double dt, a;               // FIRE
    double cfac;                // c
    double C0[9], F[9], Fopen[9], vF[9];   // the starting cell; F; F where the step in flight opened; the velocity of the rows c F
    int nimg0[3];               // image counts of the upload: no step may exceed them
    int nsteps_pos, has_v;      // steps since the last power <= 0 (ASE's Nsteps); 0 until the first step
    int steps, reason;
};
struct CellParams {
    int max_steps, hydrostatic;
    double fmax, pressure, cutoff;
    double mask[9];             // 3 x 3 of 0 / 1
    FireKnobs fire;
};
struct CellView {
    CellState *st;              // [B]
    double *s, *sopen, *vel;    // [3 N] each, laid out like the batch: s, s where the step in flight opened, the velocity of the atom rows
    double *rec;                // [B][3]: largest row force at the last test, E, V
    int *info;                  // [B][2]: steps, stop reason
};

__device__ __forceinline__ double det3(const double *m) {   // (the expression of virial_dev.h's volume)
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// C = C0 F^T
__device__ __forceinline__ void deformed_cell(const double *C0, const double *F, double *C) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) C[3 * r + k] = C0[3 * r] * F[3 * k] + C0[3 * r + 1] * F[3 * k + 1] + C0[3 * r + 2] * F[3 * k + 2];
}
// x = s F^T over the chain's atoms; the cell, its inverse and the image counts by thread 0
__device__ __forceinline__ void write_geometry(int b, int a0, int nat, const double *__restrict__ s, const double *F, const double *C,
                                               const double *inv, const int *ni, double *__restrict__ pos, double *__restrict__ cell,
                                               double *__restrict__ invcell, int *__restrict__ nimg) {
    for (int i = threadIdx.x; i < nat; i += blockDim.x) {
        const double *si = s + 3 * (size_t)(a0 + i);
        double *xi = pos + 3 * (size_t)(a0 + i);
#pragma unroll
        for (int k = 0; k < 3; ++k) xi[k] = si[0] * F[3 * k] + si[1] * F[3 * k + 1] + si[2] * F[3 * k + 2];
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { cell[9 * (size_t)b + k] = C[k]; invcell[9 * (size_t)b + k] = inv[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) nimg[3 * (size_t)b + k] = ni[k];
    }
}

__global__ void __launch_bounds__(256)
k_cell_init(const int *__restrict__ cfg_start, double dt0, double astart, double cell_factor, const double *__restrict__ pos,
            const double *__restrict__ cell, const int *__restrict__ nimg, CellView V) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int a0 = cfg_start[b], a1 = cfg_start[b + 1];
    for (int t = 3 * a0 + tid; t < 3 * a1; t += blockDim.x) {
        V.s[t] = pos[t]; V.sopen[t] = pos[t]; V.vel[t] = 0.0;
    }
    if (tid == 0) {
        CellState S;
        S.dt = dt0; S.a = astart;
        S.cfac = cell_factor > 0.0 ? cell_factor : (double)(a1 - a0);
        for (int k = 0; k < 9; ++k) {
            S.C0[k] = cell[9 * (size_t)b + k];
            S.F[k] = S.Fopen[k] = (k % 4 == 0) ? 1.0 : 0.0;
            S.vF[k] = 0.0;
        }
        for (int k = 0; k < 3; ++k) S.nimg0[k] = nimg[3 * (size_t)b + k];
        S.nsteps_pos = 0; S.has_v = 0; S.steps = 0; S.reason = 0;
        V.st[b] = S;
        V.info[2 * b] = 0; V.info[2 * b + 1] = 0;
        V.rec[3 * b] = V.rec[3 * b + 1] = V.rec[3 * b + 2] = 0.0;
    }
}

// Behind an evaluation of the batch and its stress: one visit of chain b.  FT: double (d_pot_f) or float (PaiNN's forces, widened).
// stress: [B][6] Voigt (PaiNN: the ensemble mean).  stopped: [0] chains stopped, [1] of those that need the closing evaluation.
template <class FT>
__global__ void __launch_bounds__(256)
k_cell_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
            const FT *__restrict__ forces, const double *__restrict__ stress, const uint8_t *__restrict__ fixed,
            const uint8_t *__restrict__ pbc_all, CellParams P, double *__restrict__ pos, double *__restrict__ cell,
            double *__restrict__ invcell, int *__restrict__ nimg, CellView V, int *__restrict__ stopped) {
    __shared__ double red[16];
    if (counters[2]) return;   // the evaluation overflowed the neighbor capacity: the host regrows and repeats it; nothing moves twice
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const CellState *G = V.st + b;
    const int reason0 = G->reason;
    double dt = G->dt, a = G->a;
    const double cfac = G->cfac;
    double C0[9], F[9], Fo[9], vF[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { C0[k] = G->C0[k]; F[k] = G->F[k]; Fo[k] = G->Fopen[k]; vF[k] = G->vF[k]; }
    const int n0[3] = {G->nimg0[0], G->nimg0[1], G->nimg0[2]};
    int nsteps_pos = G->nsteps_pos, has_v = G->has_v, steps = G->steps;
    __syncthreads();   // every wave holds the state before thread 0 can store the advanced one (cg_dev.h)
    if (reason0) return;
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0;
    const FT *f = forces + 3 * (size_t)a0;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;
    const uint8_t pbc[3] = {pbc_all[3 * b], pbc_all[3 * b + 1], pbc_all[3 * b + 2]};
    double *s = V.s, *so = V.sopen, *v = V.vel;   // (indexed by the batch's atom number)

    auto stop = [&](int reason, int refresh) {
        if (tid == 0) {
            CellState *W = V.st + b;
            W->reason = reason; W->steps = steps;
#pragma unroll
            for (int k = 0; k < 9; ++k) W->F[k] = F[k];
            V.info[2 * b] = steps; V.info[2 * b + 1] = reason;
            atomicAdd(stopped, 1);
            if (refresh) atomicAdd(stopped + 1, 1);
        }
    };

    // a non-finite energy, force or stress: back to where the step opened; that step is not counted
    double bad = isfinite(energy[b]) ? 0.0 : 1.0;
    for (int t = tid; t < 3 * nat; t += nt)
        if (!isfinite((double)f[t])) bad = 1.0;
    if (tid < 6 && !isfinite(stress[6 * (size_t)b + tid])) bad = 1.0;
    bad = block_max(bad, red);
    if (bad != 0.0) {
        for (int t = 3 * a0 + tid; t < 3 * (a0 + nat); t += nt) s[t] = so[t];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = Fo[k];
        double C[9], inv[9];
        int ni[3];
        bool ok;
        deformed_cell(C0, F, C);
        cell_setup(C, pbc, P.cutoff, inv, ni, ok);
        write_geometry(b, a0, nat, s, F, C, inv, ni, pos, cell, invcell, nimg);
        if (steps > 0) steps -= 1;
        stop(3, 1);
        return;
    }

    // the row forces: atoms g_i = f_i F (held rows zero); cell W = -V (sigma + p I) F^-T, hydrostatic, mask, / c
    double C[9];
    deformed_cell(C0, F, C);
    const double vol = fabs(det3(C));
    const double detF = det3(F);
    const double Finv[9] = {(F[4] * F[8] - F[5] * F[7]) / detF, (F[2] * F[7] - F[1] * F[8]) / detF, (F[1] * F[5] - F[2] * F[4]) / detF,
                            (F[5] * F[6] - F[3] * F[8]) / detF, (F[0] * F[8] - F[2] * F[6]) / detF, (F[2] * F[3] - F[0] * F[5]) / detF,
                            (F[3] * F[7] - F[4] * F[6]) / detF, (F[1] * F[6] - F[0] * F[7]) / detF, (F[0] * F[4] - F[1] * F[3]) / detF};
    const double *sg = stress + 6 * (size_t)b;
    const double A[9] = {sg[0] + P.pressure, sg[5], sg[4], sg[5], sg[1] + P.pressure, sg[3], sg[4], sg[3], sg[2] + P.pressure};
    double Gc[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            Gc[3 * r + k] = -vol * (A[3 * r] * Finv[3 * k] + A[3 * r + 1] * Finv[3 * k + 1] + A[3 * r + 2] * Finv[3 * k + 2]);
    if (P.hydrostatic) {
        const double tr = (Gc[0] + Gc[4] + Gc[8]) / 3.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) Gc[k] = (k % 4 == 0) ? tr : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Gc[k] = (Gc[k] * P.mask[k]) / cfac;

    auto row = [&](int i, double g[3]) {   // g_i = f_i F
        const bool held = fx && fx[i];
        const double f0 = held ? 0.0 : (double)f[3 * i], f1 = held ? 0.0 : (double)f[3 * i + 1], f2 = held ? 0.0 : (double)f[3 * i + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = f0 * F[k] + f1 * F[3 + k] + f2 * F[6 + k];
    };

    // convergence over all N + 3 rows, tested when the step opens
    double fm2 = 0.0, vG = 0.0, GG = 0.0, vv = 0.0;
    for (int i = tid; i < nat; i += nt) {
        double g[3];
        row(i, g);
        fm2 = fmax(fm2, g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double vk = v[3 * (size_t)(a0 + i) + k];
            vG += vk * g[k]; GG += g[k] * g[k]; vv += vk * vk;
        }
    }
    fm2 = block_max(fm2, red);
#pragma unroll
    for (int r = 0; r < 3; ++r) fm2 = fmax(fm2, Gc[3 * r] * Gc[3 * r] + Gc[3 * r + 1] * Gc[3 * r + 1] + Gc[3 * r + 2] * Gc[3 * r + 2]);
    if (tid == 0) { V.rec[3 * b] = sqrt(fm2); V.rec[3 * b + 1] = energy[b]; V.rec[3 * b + 2] = vol; }
    if (fm2 < P.fmax * P.fmax) { stop(1, 0); return; }
    if (steps >= P.max_steps) { stop(2, 0); return; }

    // one FIRE step over the 3 N + 9 numbers
    vG = block_sum(vG, red);
    GG = block_sum(GG, red);
    vv = block_sum(vv, red);
#pragma unroll
    for (int k = 0; k < 9; ++k) { vG += vF[k] * Gc[k]; GG += Gc[k] * Gc[k]; vv += vF[k] * vF[k]; }
    struct { double dt, a; int nsteps_pos, has_v; } S = {dt, a, nsteps_pos, has_v};
    const FireMix M = fire_update(S, P.fire, vG, GG, vv);
    const double scale = fire_step_scale(S.dt, M, P.fire, vG, GG, vv);
    double Fn[9], vFn[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        double vk = M.mix ? (1.0 - M.mix_a) * vF[k] + M.mix_s * Gc[k] : 0.0;
        vk += S.dt * Gc[k];
        vFn[k] = vk;
        Fn[k] = F[k] + (scale * (S.dt * vk)) / cfac;
    }
    // the new cell: finite, det F > 0, and no more images along any periodic axis than the upload gave this chain
    double Cn[9], inv[9];
    int ni[3];
    bool ok;
    deformed_cell(C0, Fn, Cn);
    bool sane = det3(Fn) > 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) sane = sane && isfinite(Cn[k]);
    if (sane) {
        cell_setup(Cn, pbc, P.cutoff, inv, ni, ok);
        sane = ok;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (pbc[k] && (ni[k] < 1 || ni[k] > n0[k])) sane = false;
    }
    if (!sane) { stop(4, 1); return; }   // the step is not taken: the chain stays at the state this evaluation saw

    for (int i = tid; i < nat; i += nt) {
        double g[3];
        row(i, g);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t t = 3 * (size_t)(a0 + i) + k;
            double vk = M.mix ? (1.0 - M.mix_a) * v[t] + M.mix_s * g[k] : 0.0;
            vk += S.dt * g[k];
            v[t] = vk;
            so[t] = s[t];
            s[t] += scale * (S.dt * vk);
        }
    }
    // (a thread reads back only the rows it wrote itself: the same stride)
    write_geometry(b, a0, nat, s, Fn, Cn, inv, ni, pos, cell, invcell, nimg);
    if (tid == 0) {
        CellState *W = V.st + b;
        W->dt = S.dt; W->a = S.a; W->nsteps_pos = S.nsteps_pos; W->has_v = 1; W->steps = steps + 1;
#pragma unroll
        for (int k = 0; k < 9; ++k) { W->Fopen[k] = F[k]; W->F[k] = Fn[k]; W->vF[k] = vFn[k]; }
    }
}

struct CellWork {
    CellView V;
    CellParams P;
    const uint8_t *fixed;   // the mask on the device (null: all free)
    int *flags;             // [0] chains stopped, [1] of those that need the closing evaluation
};

static int cell_lockstep(vssr_handle *h, const CellWork &W, uint32_t want) {
    const int B = h->n_cfg;
    hipStream_t st = h->stream;
    // every chain tests once per evaluation and takes at most max_steps steps
    LockstepPlan plan{8, (long long)W.P.max_steps + 1, LOCKSTEP_MASK_NEVER};
    plan.stopped = W.flags; plan.groups = B;
    int launch_rc = VSSR_OK;
    bool finished;
    int rc = lockstep_run(h, plan, want, finished,
        [&] {
            if (launch_rc || (launch_rc = evaluator(h).stress(h))) return;   // (seen at the next poll)
            with_forces(h, [&](const double *energy, auto *forces) {
                hipLaunchKernelGGL(k_cell_step<force_type<decltype(forces)>>, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(),
                                   h->d_counters.as<int>(), energy, forces, h->d_stress.as<double>(), W.fixed, h->d_pbc.as<uint8_t>(), W.P,
                                   h->d_pos.as<double>(), h->d_cell.as<double>(), h->d_invcell.as<double>(), h->d_nimg.as<int>(), W.V,
                                   W.flags);
            });
        },
        [&](bool) { return launch_rc; });
    if (rc) return rc;
    if (launch_rc) return launch_rc;
    if (!finished) return set_err(h, VSSR_E_DEVICE, "vssr_batch_relax_cell: the relaxation loop did not finish");
    return VSSR_OK;
}

}  // namespace vssr

using namespace vssr;

extern "C" int vssr_batch_get_cell(vssr_handle *h, double *cell) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->batch_valid) return set_err(h, VSSR_E_STATE, "vssr_batch_get_cell before vssr_batch_upload");
    if (!cell) return set_err(h, VSSR_E_BADARG, "vssr_batch_get_cell: null output");
    VSSR_HIP(h, hipSetDevice(h->device));
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    VSSR_HIP(h, hipMemcpy(cell, h->d_cell.p, sizeof(double) * 9 * (size_t)h->n_cfg, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

extern "C" int vssr_batch_relax_cell(vssr_handle *h, const vssr_cell_relax_params *p, const uint8_t *fixed, uint32_t want, double *pos_out,
                                     double *cell_out, int32_t *n_steps, int32_t *stop_reason, double *result) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!evaluator(h).stress) return set_err(h, VSSR_E_STATE, "vssr_batch_relax_cell: this handle serves no stress");
    if (h->ew_on)
        return set_err(h, VSSR_E_STATE, "vssr_batch_relax_cell: a pair handle with k-space is not served: the S(k) stride (ew_stride = %d reciprocal "
                       "cells per chain) was sized from the uploaded cells and a changed cell may exceed it", h->ew_stride);
    if (!p) return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: null parameters");
    if (p->max_steps < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: max_steps %d < 0", (int)p->max_steps);
    if (!(std::isfinite(p->fmax) && p->fmax > 0.0)) return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: fmax %g eV/A (finite and > 0 wanted)", p->fmax);
    if (!std::isfinite(p->scalar_pressure))
        return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: scalar_pressure %g eV/A^3 is not finite", p->scalar_pressure);
    if (!std::isfinite(p->cell_factor)) return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: cell_factor %g is not finite", p->cell_factor);
    for (int k = 0; k < 6; ++k)
        if (p->mask[k] != 0 && p->mask[k] != 1)
            return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: mask[%d] = %d (0 or 1 wanted)", k, (int)p->mask[k]);
    const FireKnobs fire{p->dtmax, p->finc, p->fdec, p->astart, p->fa, p->maxstep, p->nmin};
    if (int rc = fire_check(h, __func__, p->dt, fire)) return rc;
    const int B = h->n_cfg, N = h->n_atoms;
    VSSR_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    VSSR_HIP(h, hipStreamSynchronize(st));
    // An open axis k: lattice vector k along one Cartesian axis m, no component along m in the other two, and no strain component that
    // involves m freed -- the vacuum direction then stays out of F exactly.  (From the resident cells: an earlier call may have changed them.)
    {
        std::vector<double> cell((size_t)9 * B);
        std::vector<uint8_t> pbc((size_t)3 * B);
        VSSR_HIP(h, hipMemcpy(cell.data(), h->d_cell.p, sizeof(double) * cell.size(), hipMemcpyDeviceToHost));
        VSSR_HIP(h, hipMemcpy(pbc.data(), h->d_pbc.p, pbc.size(), hipMemcpyDeviceToHost));
        static const int voigt33[3][3] = {{0, 5, 4}, {5, 1, 3}, {4, 3, 2}};
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 3; ++k) {
                if (pbc[3 * b + k]) continue;
                const double *c = cell.data() + 9 * (size_t)b;
                int m = -1, nz = 0;
                for (int x = 0; x < 3; ++x)
                    if (c[3 * k + x] != 0.0) { m = x; ++nz; }
                if (nz != 1)
                    return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: chain %d is open along axis %d, whose lattice vector (%g %g %g) does not lie "
                                   "along one Cartesian axis", b, k, c[3 * k], c[3 * k + 1], c[3 * k + 2]);
                for (int r = 0; r < 3; ++r)
                    if (r != k && c[3 * r + m] != 0.0)
                        return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: chain %d is open along axis %d (Cartesian %d), but lattice vector %d has "
                                       "the component %g along it", b, k, m, r, c[3 * r + m]);
                for (int x = 0; x < 3; ++x)
                    if (p->mask[voigt33[m][x]])
                        return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cell: chain %d is open along axis %d (Cartesian %d), but mask[%d] frees a "
                                       "strain component that involves it", b, k, m, voigt33[m][x]);
            }
    }

    const size_t n3 = 3 * (size_t)N;
    CellWork W;
    auto layout = [&](Arena &a) {
        a.place(W.V.s, n3); a.place(W.V.sopen, n3); a.place(W.V.vel, n3); a.place(W.V.rec, 3 * (size_t)B);
        a.place(W.V.st, (size_t)B); a.place(W.V.info, 2 * (size_t)B); a.place(W.flags, 2);
    };
    if (h->d_cellrelax.ensure(arena_size(layout)) || h->d_stress.ensure(sizeof(double) * 12 * (size_t)B))
        return set_err(h, VSSR_E_NOMEM, "cell relaxation workspace: out of device memory");
    arena_carve(h->d_cellrelax.p, layout);
    W.P.max_steps = p->max_steps; W.P.hydrostatic = p->hydrostatic_strain != 0;
    W.P.fmax = p->fmax; W.P.pressure = p->scalar_pressure; W.P.cutoff = evaluator(h).cutoff(h);
    static const int voigt_of[9] = {0, 5, 4, 5, 1, 3, 4, 3, 2};
    for (int k = 0; k < 9; ++k) W.P.mask[k] = (double)p->mask[voigt_of[k]];
    W.P.fire = fire;

    W.fixed = nullptr;
    if (int rc = driver_open(h, fixed, 2, W.fixed, want)) return rc;
    h->ran = false;   // (until the loop has left a complete evaluation: a failure in between leaves moved cells behind)
    VSSR_HIP(h, hipMemsetAsync(W.flags, 0, sizeof(int) * 2, st));
    hipLaunchKernelGGL(k_cell_init, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(), (double)p->dt, (double)p->astart, (double)p->cell_factor,
                       h->d_pos.as<double>(), h->d_cell.as<double>(), h->d_nimg.as<int>(), W.V);
    VSSR_HIP(h, hipGetLastError());
    if (int rc = cell_lockstep(h, W, want)) return rc;
    if (int rc = driver_close(h, false)) return rc;

    if (pos_out) VSSR_HIP(h, hipMemcpy(pos_out, h->d_pos.p, sizeof(double) * n3, hipMemcpyDeviceToHost));
    if (cell_out) VSSR_HIP(h, hipMemcpy(cell_out, h->d_cell.p, sizeof(double) * 9 * (size_t)B, hipMemcpyDeviceToHost));
    if (result) VSSR_HIP(h, hipMemcpy(result, W.V.rec, sizeof(double) * 3 * (size_t)B, hipMemcpyDeviceToHost));
    if (n_steps || stop_reason) {
        std::vector<int> info(2 * (size_t)B);
        VSSR_HIP(h, hipMemcpy(info.data(), W.V.info, sizeof(int) * info.size(), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) {
            if (n_steps) n_steps[b] = info[2 * b];
            if (stop_reason) stop_reason[b] = info[2 * b + 1];
        }
    }
    return VSSR_OK;
}
