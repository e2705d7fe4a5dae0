// relax_cg.hip — lock-step LAMMPS-style conjugate gradients on the fp64 potentials (the reference's `optimizer: "LAMMPS"`): the driver
// that steps every chain's state machine (cg_dev.h) once per batch-wide evaluation in the frame of lockstep.h, and the Compactor
// that shrinks the resident batch to the chains still running.
#include <algorithm>
#include "arena.h"
#include "cg_dev.h"
#include "lockstep.h"

namespace vssr {

// ---- LAMMPS min_style cg: the state machine lives in cg_dev.h (cg_step_chain) --------------------------------------------
__global__ void k_cg_init(int B, CgState *__restrict__ st, unsigned char *__restrict__ active) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    CgState S = {};
    S.phase = PH_START;
    st[b] = S;
    active[b] = 1;
}

__global__ void __launch_bounds__(256)
k_cg_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
          const double *__restrict__ forces, const uint8_t *__restrict__ fixed, int max_iter, int max_eval, double etol,
          double ftol, double dmax, double *__restrict__ pos, double *__restrict__ x0all, double *__restrict__ hall,
          double *__restrict__ gall, CgState *__restrict__ st, unsigned char *__restrict__ active, int *__restrict__ n_active) {
    __shared__ double red[256];
    if (counters[2]) return;
    cg_step_chain(blockIdx.x, red, cfg_start, energy, forces, fixed, max_iter, max_eval, etol, ftol, dmax, pos, x0all, hall, gall, st, active,
                  n_active);
}

// ---- live-chain compaction of the resident batch (fp64 analytic potentials) ---------------------------------------------------
// The CG minimiser stops every chain by its own criteria; with the activity mask alone a finished chain still costs its share of
// every later launch (grids are sized for the whole batch, its workgroups leave at once).  At a poll with at most 3/4 of the
// resident chains still running the batch is PHYSICALLY compacted: the live chains' inputs (positions, types, cells) and optimizer
// state are gathered into a smaller resident batch, the finished chains' final positions / states are parked in full-size
// arrays, and every kernel of the path (neighbor build, potential, CG step) runs unchanged on the smaller batch -- a chain's
// results do not depend on its batch, so the trajectories are the same bit for bit (tests/test_cg.py).  The original batch is
// restored before the final static evaluation.
struct CmpView {   // device pointers of one layout of the per-chain / per-atom arrays
    int *cfg_start, *Z, *atom_cfg, *nimg;
    double *pos, *cell, *inv, *x0, *hh, *gg;
    uint8_t *pbc, *fixed;
    CgState *st;
};

__global__ void __launch_bounds__(1024)
k_cmp_plan(int B, const int *__restrict__ cfg_start, const unsigned char *__restrict__ active, const int *__restrict__ live,
           int *__restrict__ live_new, int *__restrict__ src, int *__restrict__ start_new, int *__restrict__ totals) {
    __shared__ int sc[1024], sa[1024];
    const int t = threadIdx.x, per = (B + 1023) / 1024, c0 = min(B, t * per), c1 = min(B, c0 + per);
    int nc = 0, na = 0;
    for (int c = c0; c < c1; ++c)
        if (active[c]) { nc += 1; na += cfg_start[c + 1] - cfg_start[c]; }
    sc[t] = nc; sa[t] = na;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive scans
        const int vc = t >= d ? sc[t - d] : 0, va = t >= d ? sa[t - d] : 0;
        __syncthreads();
        sc[t] += vc; sa[t] += va;
        __syncthreads();
    }
    int oc = sc[t] - nc, oa = sa[t] - na;
    for (int c = c0; c < c1; ++c)
        if (active[c]) {
            live_new[oc] = live ? live[c] : c;
            src[oc] = c;
            start_new[oc] = oa;
            oc += 1;
            oa += cfg_start[c + 1] - cfg_start[c];
        }
    if (t == 1023) { start_new[sc[t]] = sa[t]; totals[0] = sc[t]; totals[1] = sa[t]; }
}

// chains of the CURRENT batch whose results are final (active == nullptr: all of them): positions and optimizer state to their
// places in the ORIGINAL batch
__global__ void __launch_bounds__(128)
k_cmp_flush(const int *__restrict__ cfg_start, const unsigned char *__restrict__ active, const int *__restrict__ live,
            const int *__restrict__ start0, const double *__restrict__ pos, const CgState *__restrict__ st,
            double *__restrict__ final_pos, CgState *__restrict__ final_st) {
    const int c = blockIdx.x;
    if (active && active[c]) return;
    const int o = live ? live[c] : c, a0 = cfg_start[c], n = 3 * (cfg_start[c + 1] - a0);
    const size_t d0 = 3 * (size_t)start0[o], s0 = 3 * (size_t)a0;
    for (int k = threadIdx.x; k < n; k += blockDim.x) final_pos[d0 + k] = pos[s0 + k];
    if (threadIdx.x == 0) final_st[o] = st[c];
}

__global__ void __launch_bounds__(128)
k_cmp_gather(const int *__restrict__ src, const int *__restrict__ start_new, CmpView from, CmpView to, unsigned char *__restrict__ active_new) {
    const int nc = blockIdx.x, c = src[nc], a0 = from.cfg_start[c], na = from.cfg_start[c + 1] - a0, b0 = start_new[nc];
    for (int k = threadIdx.x; k < 3 * na; k += blockDim.x) {
        to.pos[3 * (size_t)b0 + k] = from.pos[3 * (size_t)a0 + k];
        to.x0[3 * (size_t)b0 + k] = from.x0[3 * (size_t)a0 + k];
        to.hh[3 * (size_t)b0 + k] = from.hh[3 * (size_t)a0 + k];
        to.gg[3 * (size_t)b0 + k] = from.gg[3 * (size_t)a0 + k];
    }
    for (int k = threadIdx.x; k < na; k += blockDim.x) {
        to.Z[b0 + k] = from.Z[a0 + k];
        to.atom_cfg[b0 + k] = nc;
        if (from.fixed) to.fixed[b0 + k] = from.fixed[a0 + k];
    }
    if (threadIdx.x < 9) { to.cell[9 * (size_t)nc + threadIdx.x] = from.cell[9 * (size_t)c + threadIdx.x]; to.inv[9 * (size_t)nc + threadIdx.x] = from.inv[9 * (size_t)c + threadIdx.x]; }
    if (threadIdx.x < 3) { to.nimg[3 * nc + threadIdx.x] = from.nimg[3 * c + threadIdx.x]; to.pbc[3 * nc + threadIdx.x] = from.pbc[3 * c + threadIdx.x]; }
    if (threadIdx.x == 0) { to.st[nc] = from.st[c]; active_new[nc] = 1; }
}

// the gathered arrays back over the resident ones, one launch (13 small device-to-device copies cost more than the evaluation of a
// small batch); live / start_new travel along
__global__ void __launch_bounds__(256)
k_cmp_copyback(int Bn, int Nn, CmpView to, CmpView from, int *__restrict__ live, const int *__restrict__ live_new,
               const int *__restrict__ start_new) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t k = t; k < 3 * (size_t)Nn; k += step) { to.pos[k] = from.pos[k]; to.x0[k] = from.x0[k]; to.hh[k] = from.hh[k]; to.gg[k] = from.gg[k]; }
    for (size_t k = t; k < (size_t)Nn; k += step) { to.Z[k] = from.Z[k]; to.atom_cfg[k] = from.atom_cfg[k]; if (from.fixed && to.fixed) to.fixed[k] = from.fixed[k]; }
    for (size_t k = t; k < 9 * (size_t)Bn; k += step) { to.cell[k] = from.cell[k]; to.inv[k] = from.inv[k]; }
    for (size_t k = t; k < 3 * (size_t)Bn; k += step) { to.nimg[k] = from.nimg[k]; to.pbc[k] = from.pbc[k]; }
    for (size_t k = t; k < (size_t)Bn; k += step) { to.st[k] = from.st[k]; live[k] = live_new[k]; }
    for (size_t k = t; k <= (size_t)Bn; k += step) to.cfg_start[k] = start_new[k];
}

__global__ void k_cg_report(int B, const CgState *__restrict__ st, int *__restrict__ out /*[B][3]*/) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[3 * b] = st[b].niter; out[3 * b + 1] = st[b].neval; out[3 * b + 2] = st[b].reason;
}

// The field list of a CmpView, once: fn(member, elements, role) per array of a layout with B chains / N atoms.  The arena's layout,
// the save of the uploaded batch and its restore walk this list; element sizes come from the members' types.
enum CmpRole { CMP_INPUT, CMP_RESULT, CMP_WORK };   // uploaded inputs < what a relaxation leaves (positions, state) < optimizer vectors
template <class Fn>
static void for_each_field(size_t B, size_t N, Fn fn) {
    fn(&CmpView::cfg_start, B + 1, CMP_INPUT); fn(&CmpView::Z, N, CMP_INPUT); fn(&CmpView::atom_cfg, N, CMP_INPUT);
    fn(&CmpView::nimg, 3 * B, CMP_INPUT); fn(&CmpView::pos, 3 * N, CMP_RESULT); fn(&CmpView::cell, 9 * B, CMP_INPUT);
    fn(&CmpView::inv, 9 * B, CMP_INPUT); fn(&CmpView::x0, 3 * N, CMP_WORK); fn(&CmpView::hh, 3 * N, CMP_WORK); fn(&CmpView::gg, 3 * N, CMP_WORK);
    fn(&CmpView::pbc, 3 * B, CMP_INPUT); fn(&CmpView::fixed, N, CMP_INPUT); fn(&CmpView::st, B, CMP_RESULT);
}

struct Compactor {
    vssr_handle *h;
    const CgWork W;
    const uint8_t *fixed;   // the FixAtoms mask and the activity mask of the relaxation
    unsigned char *active;
    const int B, N;     // the uploaded batch
    int B_cur, N_cur;   // the resident batch the kernels see
    // VSSR_RELAX_COMPACT, read per call: 0 switches the compaction off (A/B runs, the equality test), n > 1: smallest resident batch, atoms
    const int knob = getenv("VSSR_RELAX_COMPACT") ? atoi(getenv("VSSR_RELAX_COMPACT")) : 1;
    bool compacted = false;
    const CmpView cur{h->d_cfg_start.as<int>(), h->d_Z.as<int>(), h->d_atom_cfg.as<int>(), h->d_nimg.as<int>(), h->d_pos.as<double>(),
                      h->d_cell.as<double>(), h->d_invcell.as<double>(), W.x0, W.hh, W.gg, h->d_pbc.as<uint8_t>(),
                      const_cast<uint8_t *>(fixed), W.st};   // the resident arrays
    // arena (h->d_cmp): [orig | maps | tmp].  orig: the uploaded inputs and the parked final positions / states of the chains that have
    // left the resident batch (no optimizer vectors); tmp: the gather target
    CmpView orig{}, tmp{};
    int *live = nullptr, *live_new = nullptr, *src = nullptr, *start_new = nullptr, *totals = nullptr;

    // at most 3/4 of the resident chains are still running: continue on a compacted batch.  Only where the kernels are
    // throughput-bound: below ~one round of workgroups (256 CUs x 3 x 64 centres = 49 k atoms) a launch costs the same
    // whatever the live share, and the compaction (four launches + a host read) would only add to it (measured, 256
    // chains x 48 atoms: -3 %; profiles/r05/NOTES_tersoff.md)
    bool due(int n_live) const { return knob != 0 && N_cur >= (knob > 1 ? knob : 65536) && (long long)n_live * 4 <= (long long)B_cur * 3; }
    int carve() {   // every block on 256-byte lines of its own, the last one included
        auto layout = [&](Arena &a) {
            for_each_field(B, N, [&](auto m, size_t n, CmpRole role) { if (role != CMP_WORK) a.place(orig.*m, n); });
            a.place(live, B); a.place(live_new, B); a.place(src, B); a.place(start_new, (size_t)B + 1); a.place(totals, 4);
            for_each_field(B, N, [&](auto m, size_t n, CmpRole) { a.place(tmp.*m, n); });
            a.align(256);
        };
        if (h->d_cmp.ensure(arena_size(layout, 256))) return -1;
        arena_carve(h->d_cmp.p, layout, 256);
        return 0;
    }
    int copy_fields(const CmpView &to, const CmpView &from, CmpRole upto) {   // the arrays of roles <= upto, at the uploaded batch's sizes
        hipError_t e = hipSuccess;
        for_each_field(B, N, [&](auto m, size_t n, CmpRole role) {
            if (role <= upto && to.*m && from.*m && e == hipSuccess)
                e = hipMemcpyAsync(to.*m, from.*m, n * sizeof(*(to.*m)), hipMemcpyDeviceToDevice, h->stream);
        });
        return e == hipSuccess ? VSSR_OK : set_err(h, VSSR_E_DEVICE, "live-chain compaction: copy failed: %s", hipGetErrorString(e));
    }
    int compact() {
        hipStream_t st = h->stream;
        if (!compacted) {   // first time: keep the original batch
            if (carve()) return set_err(h, VSSR_E_NOMEM, "compaction arena: out of device memory");
            if (int rc = copy_fields(orig, cur, CMP_INPUT)) return rc;
        }
        const int *lv = compacted ? live : nullptr;
        hipLaunchKernelGGL(k_cmp_plan, dim3(1), dim3(1024), 0, st, B_cur, cur.cfg_start, active, lv, live_new, src, start_new, totals);
        hipLaunchKernelGGL(k_cmp_flush, dim3(B_cur), dim3(128), 0, st, cur.cfg_start, active, lv, orig.cfg_start, cur.pos, cur.st, orig.pos, orig.st);
        int tot[2] = {0, 0};
        VSSR_HIP(h, hipMemcpyAsync(tot, totals, sizeof(tot), hipMemcpyDeviceToHost, st));
        VSSR_HIP(h, hipStreamSynchronize(st));
        const int Bn = tot[0], Nn = tot[1];
        if (Bn <= 0 || Bn > B_cur || Nn <= 0 || Nn > N_cur) return set_err(h, VSSR_E_STATE, "live-chain compaction: inconsistent plan");
        hipLaunchKernelGGL(k_cmp_gather, dim3(Bn), dim3(128), 0, st, src, start_new, cur, tmp, active);
        // (the gather reads the resident arrays and writes the arena; one more launch copies the arena over the resident arrays)
        CmpView from = tmp;
        if (!fixed) from.fixed = nullptr;
        const int blocks = (int)std::min<size_t>(1024, (3 * (size_t)Nn + 255) / 256);
        hipLaunchKernelGGL(k_cmp_copyback, dim3(blocks), dim3(256), 0, st, Bn, Nn, cur, from, live, live_new, start_new);
        compacted = true;
        h->n_cfg = B_cur = Bn; h->n_atoms = N_cur = Nn;
        ++h->relax_compactions;
        return VSSR_OK;
    }
    int restore() {   // park what is still resident, then bring the original batch back (positions = the final ones)
        if (!compacted) return VSSR_OK;
        hipLaunchKernelGGL(k_cmp_flush, dim3(B_cur), dim3(128), 0, h->stream, cur.cfg_start, (const unsigned char *)nullptr, live, orig.cfg_start,
                           cur.pos, cur.st, orig.pos, orig.st);
        compacted = false;
        h->n_cfg = B_cur = B; h->n_atoms = N_cur = N;
        return copy_fields(cur, orig, CMP_RESULT);
    }
    int abandon(int rc) {   // error path: a compacted batch is not handed back half-way, the caller uploads again
        if (compacted) { h->n_cfg = B; h->n_atoms = N; h->batch_valid = false; }
        return rc;
    }
};

int relax_cg(vssr_handle *h, const vssr_cg_params *cp, const uint8_t *fixed_host, uint32_t want) {
    hipStream_t st = h->stream;
    if (!is_analytic(h))
        return set_err(h, VSSR_E_STATE, "conjugate gradients need an fp64 potential (Tersoff / EAM / SW handle); use BFGS or FIRE");
    const uint8_t *fixed = nullptr;
    CgWork W;
    if (int e = driver_open(h, fixed_host, 3, fixed, want)) return e;
    if (int e = CgWork::ensure(h, W)) return e;
    unsigned char *active = h->d_active.as<unsigned char>();
    hipLaunchKernelGGL(k_cg_init, dim3((h->n_cfg + 127) / 128), dim3(128), 0, st, h->n_cfg, W.st, active);
    Compactor C{h, W, fixed, active, h->n_cfg, h->n_atoms, h->n_cfg, h->n_atoms};
    // every launch is one evaluation; max_eval is tested between line searches, and a line search ends after at most ~60
    // halvings of alpha (fp64), so the launch budget is max_eval plus one line search plus setup / reset evaluations.  The step
    // kernel counts the chains still running into counters[3]; finished chains were switched off at different times, so the closing
    // evaluation always runs.
    LockstepPlan plan{8, (long long)cp->max_eval + 72, LOCKSTEP_MASK_FROM_START};
    plan.always_close = true;
    bool finished;
    int rc = lockstep_run(
        h, plan, want, finished,
        [&] {
            hipLaunchKernelGGL(k_cg_step, dim3(C.B_cur), dim3(256), 0, st, h->d_cfg_start.as<int>(), h->d_counters.as<int>(),
                               h->d_pot_e.as<double>(), h->d_pot_f.as<double>(), fixed, cp->max_iter, cp->max_eval, cp->etol, cp->ftol,
                               cp->dmax, h->d_pos.as<double>(), W.x0, W.hh, W.gg, W.st, active, h->d_counters.as<int>() + 3);
        },
        [&](bool closing) -> int {   // the uploaded batch again before the closing evaluation; at a poll, a smaller resident batch where due
            if (closing) return C.restore();
            return C.due(h->h_counters[3]) ? C.compact() : (int)VSSR_OK;
        });
    if (rc) return C.abandon(rc);   // (nothing to abandon once restore has run)
    hipLaunchKernelGGL(k_cg_report, dim3((C.B + 127) / 128), dim3(128), 0, st, C.B, W.st, h->d_relax_steps.as<int>());
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
