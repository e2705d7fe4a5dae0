// relax_bfgsls.hip — lock-step BFGSLineSearch on every handle kind (the reference's `optimizer: "BFGSLineSearch"`, mcmc/dynamics.py:119-127
// -> ase.optimize.BFGSLineSearch): the driver that steps every chain's state machine (bfgsls_dev.h) once per batch-wide evaluation, with
// the frame of lockstep.h.  Evaluation-counted like relax_cg: a trial of a line search costs one lock-step evaluation, and
// the evaluation that ends a line search opens the next step.  Not pinned by an executed ASE: see the header of bfgsls_dev.h.
// Out of scope here: live-chain compaction (relax_cg.hip's Compactor) and a chain-resident form (chain_min.hip); finished chains are
// skipped through the activity mask only.
#include <algorithm>
#include "bfgsls_dev.h"
#include "lockstep.h"

namespace vssr {

__global__ void k_bls_init(int B, BlsState *__restrict__ st, unsigned char *__restrict__ active) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    BlsState S = {};
    S.phase = BLS_OPEN;
    st[b] = S;
    active[b] = 1;
}

template <class FT>
__global__ void __launch_bounds__(256)
k_bls_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
           const FT *__restrict__ forces, const uint8_t *__restrict__ fixed, BlsParams P, double *__restrict__ pos, BlsView V,
           unsigned char *__restrict__ active, int *__restrict__ running) {
    __shared__ double red[16];
    if (counters[2]) return;   // the evaluation overflowed the neighbor capacity: nothing moves, the host regrows and repeats it
    bls_step_chain<FT>(blockIdx.x, red, cfg_start, energy, forces, fixed, P, pos, V, active, running);
}

__global__ void k_bls_report(int B, const BlsState *__restrict__ st, int *__restrict__ out /*[B][3]*/) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[3 * b] = st[b].steps; out[3 * b + 1] = st[b].neval; out[3 * b + 2] = st[b].reason;
}

// The optimizer's workspace on the handle's optimizer buffers (as BfgsWork, relax.hip): state, three vectors, the update history
// (max_steps triples per chain in HBM: 2 x 3 N x max_steps doubles) and, when armed, the trajectory rings of relax_lockstep.
static int bls_workspace(vssr_handle *h, int max_steps, BlsView &V) {
    const size_t B = h->n_cfg, N = h->n_atoms, cap = (size_t)std::max(max_steps, 1);
    if (h->d_opt_state.ensure(sizeof(BlsState) * B) || h->d_opt_vec.ensure(sizeof(double) * 9 * N) ||
        h->d_bfgs_q.ensure(sizeof(double) * 6 * N * cap) || h->d_bfgs_b.ensure(sizeof(double) * 2 * B * cap))
        return set_err(h, VSSR_E_NOMEM, "BFGSLineSearch state: out of device memory");
    V = {};
    V.st = h->d_opt_state.as<BlsState>();
    V.r0 = h->d_opt_vec.as<double>(); V.g0 = V.r0 + 3 * N; V.p = V.r0 + 6 * N;
    V.hs = h->d_bfgs_q.as<double>(); V.hy = V.hs + 3 * N * cap;
    V.rho = h->d_bfgs_b.as<double>(); V.la = V.rho + B * cap;
    V.cap = (int)cap;
    const int iv = h->traj_interval, nrec = iv > 0 ? max_steps / iv + 1 : 0;
    h->traj_records = 0;
    if (nrec) {
        if (h->d_traj_pos.ensure(sizeof(double) * 3 * N * nrec) || h->d_traj_f.ensure(sizeof(float) * 3 * N * nrec) ||
            h->d_traj_e.ensure(sizeof(double) * B * nrec) || h->d_traj_n.ensure(sizeof(int) * B))
            return set_err(h, VSSR_E_NOMEM, "trajectory records: out of device memory");
        VSSR_HIP(h, hipMemsetAsync(h->d_traj_n.p, 0, sizeof(int) * B, h->stream));
        h->traj_records = nrec; h->traj_B = (int)B; h->traj_N = (int)N;
        V.interval = iv; V.nrec = nrec; V.B = (int)B; V.N = (int)N;
        V.ring_pos = h->d_traj_pos.as<double>(); V.ring_f = h->d_traj_f.as<float>(); V.ring_e = h->d_traj_e.as<double>();
        V.ring_n = h->d_traj_n.as<int>();
    }
    return VSSR_OK;
}

int relax_bfgsls(vssr_handle *h, const vssr_bfgsls_params *bp, const uint8_t *fixed_host, uint32_t want) {
    hipStream_t st = h->stream;
    const int B = h->n_cfg;
    const uint8_t *fixed = nullptr;
    BlsView V;
    if (int e = driver_open(h, fixed_host, 3, fixed, want)) return e;
    if (int e = bls_workspace(h, bp->max_steps, V)) return e;
    // ASE's defaults for what the ABI does not expose: stpmin, xtol, xtrapl, xtrapu
    const BlsParams P{bp->max_steps, bp->max_eval, bp->fmax, bp->alpha, bp->maxstep, bp->c1, bp->c2, bp->stpmax, 1e-8, 1e-14, 1.1, 4.0};
    unsigned char *active = h->d_active.as<unsigned char>();
    hipLaunchKernelGGL(k_bls_init, dim3((B + 127) / 128), dim3(128), 0, st, B, V.st, active);
    // every launch is one evaluation for every chain still running (counted into counters[3]), and a chain stops once it has spent
    // max_eval of them; finished chains leave the evaluation at once, so the closing evaluation always runs
    LockstepPlan plan{4, (long long)bp->max_eval + 2, LOCKSTEP_MASK_FROM_START};
    plan.always_close = true;
    bool finished;
    int rc = lockstep_run(h, plan, want, finished, [&] {
        // fp64 energies and forces of the potential; PaiNN: the fp64 ensemble mean and fp32 forces, widened
        with_forces(h, [&](const double *energy, auto *forces) {
            hipLaunchKernelGGL(k_bls_step<force_type<decltype(forces)>>, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(),
                               h->d_counters.as<int>(), energy, forces, fixed, P, h->d_pos.as<double>(), V, active,
                               h->d_counters.as<int>() + 3);
        });
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_bls_report, dim3((B + 127) / 128), dim3(128), 0, st, B, V.st, h->d_relax_steps.as<int>());
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
