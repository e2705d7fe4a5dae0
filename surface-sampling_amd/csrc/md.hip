// md.hip — molecular dynamics of every chain of the resident batch, on every handle kind that relaxes: velocity Verlet (NVE) and
// Langevin BAOAB.  The lock-step driver: one batch-wide evaluation per time step, one k_md_step launch behind it (one workgroup per
// chain, the integrator of md_dev.h); positions, velocities and forces never leave HBM.  The driver frame is lockstep.h's (every
// random number is keyed by the chain's own step counter, so an evaluation repeated after a regrow retraces nothing twice).  The
// analytic kinds integrate their fp64 forces (d_pot_f), PaiNN its fp32 forces widened and the fp64
// ensemble-mean energy.  The chain-resident driver (k_md_chain, chain_min.hip) runs the same md_step_chain; the entry points below
// choose between the two.
// Variable cells and the Berendsen / stochastic-cell-rescaling couplings are md_npt.hip's (vssr_batch_md_npt, lock step only).
// Out of scope: constraints other than FixAtoms, centre-of-mass removal (slabs hold their bottom layers), neighbor-list reuse with a
// skin, live-chain compaction.
#include <algorithm>
#include <cmath>
#include <vector>
#include "arena.h"
#include "lockstep.h"
#include "md_dev.h"

namespace vssr {

__global__ void k_md_init(int B, MdState *__restrict__ st, unsigned char *__restrict__ active) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    MdState S = {};
    st[b] = S;
    active[b] = 1;
}

// held atoms carry no velocity, whatever the caller set
__global__ void k_md_hold(int N, const uint8_t *__restrict__ fixed, double *__restrict__ vel) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || !fixed[i]) return;
    vel[3 * i] = 0.0; vel[3 * i + 1] = 0.0; vel[3 * i + 2] = 0.0;
}

template <class FT>
__global__ void __launch_bounds__(256)
k_md_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
          const FT *__restrict__ forces, const uint8_t *__restrict__ fixed, MdParams P, double *__restrict__ pos, MdView V,
          unsigned char *__restrict__ active, int *__restrict__ stopped) {
    __shared__ double red[16];
    if (counters[2]) return;   // the evaluation overflowed the neighbor capacity: nothing moves, the host regrows and repeats it
    md_step_chain<FT>(blockIdx.x, red, cfg_start, energy, forces, fixed, P, pos, V, active, stopped);
}

__global__ void k_md_report(int B, const MdState *__restrict__ st, int *__restrict__ out /*[B][2]*/) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[2 * b] = st[b].steps; out[2 * b + 1] = st[b].reason;
}

// Maxwell-Boltzmann velocities: v = sqrt(kB T MD_ACC / m) xi per component, held atoms 0 (md_dev.h: draw tag MD_TAG_MAXWELL, n = 0)
__global__ void k_md_draw(int N, const int *__restrict__ atom_cfg, const int *__restrict__ cfg_start, const double *__restrict__ mass,
                          const uint8_t *__restrict__ fixed, const unsigned long long *__restrict__ chain_id, double temperature,
                          uint32_t seed_lo, uint32_t seed_hi, double *__restrict__ vel) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double z[3] = {0.0, 0.0, 0.0};
    double sigma = 0.0;
    if (!(fixed && fixed[i])) {
        const int b = atom_cfg[i];
        uint32_t q0, q1;
        md_chain_key(seed_lo, seed_hi, chain_id[b], q0, q1);
        md_normal3(q0, q1, 0, i - cfg_start[b], MD_TAG_MAXWELL, z);
        sigma = sqrt(MD_KB * temperature * MD_ACC / mass[i]);
    }
    for (int c = 0; c < 3; ++c) vel[3 * i + c] = sigma * z[c];
}

// d_md_aux: [stop counters (16 bytes) | chain ids [B] | thermo records [nrec][B][2]]
struct MdAux {
    int *stopped;
    unsigned long long *ids;
    double *thermo;
};

// d_md_aux carved for nrec thermo records (0: a caller that draws velocities ahead of the run, which knows no count yet and needs the
// ids only), chain ids on the device (null: 0 .. B-1)
static int md_upload_ids(vssr_handle *h, const uint64_t *chain_id, size_t nrec, MdAux &X) {
    const size_t B = h->n_cfg;
    auto layout = [&](Arena &a) { a.place(X.stopped, 4); a.place(X.ids, B); a.place(X.thermo, 2 * B * nrec); };
    if (h->d_md_aux.ensure(arena_size(layout))) return set_err(h, VSSR_E_NOMEM, "molecular dynamics state: out of device memory");
    arena_carve(h->d_md_aux.p, layout);
    std::vector<unsigned long long> ids(B);
    for (size_t b = 0; b < B; ++b) ids[b] = chain_id ? (unsigned long long)chain_id[b] : (unsigned long long)b;
    VSSR_HIP(h, hipMemcpyAsync(X.ids, ids.data(), sizeof(unsigned long long) * B, hipMemcpyHostToDevice, h->stream));
    VSSR_HIP(h, hipStreamSynchronize(h->stream));   // (ids leaves scope)
    return VSSR_OK;
}

int md_begin(vssr_handle *h, const vssr_md_params *p, const double *mass, const uint8_t *fixed_host, const uint64_t *chain_id, uint32_t want,
             MdWork &W) {
    hipStream_t st = h->stream;
    const size_t B = h->n_cfg, N = h->n_atoms;
    W.fixed = nullptr;
    if (int e = driver_open(h, fixed_host, 2, W.fixed, want)) return e;
    W.nrec = p->n_steps / p->thermo_interval + 1;
    const size_t thermo_bytes = sizeof(double) * 2 * B * (size_t)W.nrec;
    if (h->d_opt_state.ensure(sizeof(MdState) * B) || h->d_opt_vec.ensure(sizeof(double) * 7 * N))
        return set_err(h, VSSR_E_NOMEM, "molecular dynamics state: out of device memory");
    MdAux X;
    if (int e = md_upload_ids(h, chain_id, (size_t)W.nrec, X)) return e;
    W.stopped = X.stopped;
    double *w = h->d_opt_vec.as<double>();
    W.V = {h->d_opt_state.as<MdState>(), h->d_md_vel.as<double>(), w, w + 3 * N, w + 6 * N, X.ids, X.thermo};
    VSSR_HIP(h, hipMemsetAsync(W.stopped, 0, 16, st));
    VSSR_HIP(h, hipMemsetAsync(W.V.thermo, 0xFF, thermo_bytes, st));   // records a chain never reaches read as NaN
    VSSR_HIP(h, hipMemcpyAsync(w + 6 * N, mass, sizeof(double) * N, hipMemcpyHostToDevice, st));   // (pageable source: copied before the call returns)
    hipLaunchKernelGGL(k_md_init, dim3((h->n_cfg + 127) / 128), dim3(128), 0, st, h->n_cfg, W.V.st, h->d_active.as<unsigned char>());
    if (W.fixed) hipLaunchKernelGGL(k_md_hold, dim3((h->n_atoms + 255) / 256), dim3(256), 0, st, h->n_atoms, W.fixed, W.V.vel);
    const bool langevin = p->thermostat == VSSR_MD_LANGEVIN;
    const double c1 = langevin ? std::exp(-p->friction * p->dt) : 1.0;
    W.P = {p->n_steps, p->thermostat, p->thermo_interval, (int)B, p->dt, p->temperature, p->temperature_end, c1, 1.0 - c1 * c1,
           langevin ? (long long)p->ramp_steps : 0LL, (long long)p->step0, (uint32_t)p->seed, (uint32_t)(p->seed >> 32)};
    return VSSR_OK;
}

int md_end(vssr_handle *h, const MdWork &W, double *thermo_out) {
    const int B = h->n_cfg;
    hipLaunchKernelGGL(k_md_report, dim3((B + 127) / 128), dim3(128), 0, h->stream, B, W.V.st, h->d_relax_steps.as<int>());
    VSSR_HIP(h, hipGetLastError());
    if (thermo_out)
        VSSR_HIP(h, hipMemcpyAsync(thermo_out, W.V.thermo, sizeof(double) * 2 * (size_t)B * (size_t)W.nrec, hipMemcpyDeviceToHost, h->stream));
    return VSSR_OK;
}

int md_lockstep(vssr_handle *h, const MdWork &W, uint32_t want) {
    const int B = h->n_cfg;
    // evaluations a chain needs: the initial state and one per step.  Only a non-finite chain stops early: it went back to its last
    // completed step, which asks for the closing evaluation.  (A loop the budget ended is no error here.)
    LockstepPlan plan{8, (long long)W.P.n_steps + 1, LOCKSTEP_MASK_AT_STOP};
    plan.stopped = W.stopped; plan.groups = B;
    bool finished;
    return lockstep_run(h, plan, want, finished, [&] {
        with_forces(h, [&](const double *energy, auto *forces) {
            hipLaunchKernelGGL(k_md_step<force_type<decltype(forces)>>, dim3(B), dim3(256), 0, h->stream, h->d_cfg_start.as<int>(),
                               h->d_counters.as<int>(), energy, forces, W.fixed, W.P, h->d_pos.as<double>(), W.V,
                               h->d_active.as<unsigned char>(), W.stopped);
        });
    });
}

int md_masses_ok(vssr_handle *h, const char *func, const double *mass) {
    if (!mass) return set_err(h, VSSR_E_BADARG, "%s: null masses", func);
    for (int i = 0; i < h->n_atoms; ++i)
        if (!(std::isfinite(mass[i]) && mass[i] > 0.0)) return set_err(h, VSSR_E_BADARG, "%s: mass of atom %d is %g (finite and > 0 wanted)", func, i, mass[i]);
    return VSSR_OK;
}

}  // namespace vssr

using namespace vssr;

extern "C" {

int vssr_batch_md_set_velocities(vssr_handle *h, const double *vel) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->batch_valid) return set_err(h, VSSR_E_STATE, "vssr_batch_md_set_velocities before vssr_batch_upload");
    const size_t n3 = 3 * (size_t)h->n_atoms;
    if (vel)
        for (size_t t = 0; t < n3; ++t)
            if (!std::isfinite(vel[t])) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_set_velocities: non-finite velocity");
    VSSR_HIP(h, hipSetDevice(h->device));
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    h->md_vel_valid = false;
    if (h->d_md_vel.ensure(sizeof(double) * n3)) return set_err(h, VSSR_E_NOMEM, "velocities: out of device memory");
    if (vel) VSSR_HIP(h, hipMemcpy(h->d_md_vel.p, vel, sizeof(double) * n3, hipMemcpyHostToDevice));
    else VSSR_HIP(h, hipMemset(h->d_md_vel.p, 0, sizeof(double) * n3));
    h->md_vel_valid = true;
    return VSSR_OK;
}

int vssr_batch_md_draw_velocities(vssr_handle *h, const double *mass, const uint8_t *fixed, const uint64_t *chain_id, double temperature,
                                  uint64_t seed) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->batch_valid) return set_err(h, VSSR_E_STATE, "vssr_batch_md_draw_velocities before vssr_batch_upload");
    if (int rc = md_masses_ok(h, __func__, mass)) return rc;
    if (!(std::isfinite(temperature) && temperature >= 0.0))
        return set_err(h, VSSR_E_BADARG, "vssr_batch_md_draw_velocities: temperature %g K (finite and >= 0 wanted)", temperature);
    VSSR_HIP(h, hipSetDevice(h->device));
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    const int N = h->n_atoms;
    h->md_vel_valid = false;
    if (h->d_md_vel.ensure(sizeof(double) * 3 * (size_t)N) || h->d_opt_vec.ensure(sizeof(double) * 7 * (size_t)N) || h->d_fixed.ensure((size_t)N))
        return set_err(h, VSSR_E_NOMEM, "velocities: out of device memory");
    MdAux X;
    if (int rc = md_upload_ids(h, chain_id, 0, X)) return rc;
    double *d_mass = h->d_opt_vec.as<double>() + 6 * (size_t)N;   // (where md_begin puts the masses)
    VSSR_HIP(h, hipMemcpy(d_mass, mass, sizeof(double) * (size_t)N, hipMemcpyHostToDevice));
    if (fixed) VSSR_HIP(h, hipMemcpy(h->d_fixed.p, fixed, (size_t)N, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_md_draw, dim3((N + 255) / 256), dim3(256), 0, h->stream, N, h->d_atom_cfg.as<int>(), h->d_cfg_start.as<int>(), d_mass,
                       fixed ? h->d_fixed.as<uint8_t>() : nullptr,
                       X.ids, temperature, (uint32_t)seed, (uint32_t)(seed >> 32), h->d_md_vel.as<double>());
    VSSR_HIP(h, hipGetLastError());
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    h->md_vel_valid = true;
    return VSSR_OK;
}

int vssr_batch_md_get_velocities(vssr_handle *h, double *vel) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->batch_valid || !h->md_vel_valid)
        return set_err(h, VSSR_E_STATE, "vssr_batch_md_get_velocities: the resident batch has no velocities (vssr_batch_md_set_velocities / _draw_velocities)");
    if (!vel) return set_err(h, VSSR_E_BADARG, "vssr_batch_md_get_velocities: null output");
    VSSR_HIP(h, hipSetDevice(h->device));
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    VSSR_HIP(h, hipMemcpy(vel, h->d_md_vel.p, sizeof(double) * 3 * (size_t)h->n_atoms, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int vssr_batch_md(vssr_handle *h, const vssr_md_params *p, const double *mass, const uint8_t *fixed, const uint64_t *chain_id, uint32_t want,
                  double *pos_out, double *thermo, int32_t *n_done, int32_t *stop_reason) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!p) return set_err(h, VSSR_E_BADARG, "vssr_batch_md: null parameters");
    if (p->n_steps < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_md: n_steps %d < 0", (int)p->n_steps);
    if (p->thermo_interval < 1) return set_err(h, VSSR_E_BADARG, "vssr_batch_md: thermo_interval %d < 1", (int)p->thermo_interval);
    if (!(std::isfinite(p->dt) && p->dt > 0.0)) return set_err(h, VSSR_E_BADARG, "vssr_batch_md: dt %g fs (finite and > 0 wanted)", p->dt);
    if (p->thermostat != VSSR_MD_NVE && p->thermostat != VSSR_MD_LANGEVIN)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_md: thermostat %d is neither VSSR_MD_NVE (0) nor VSSR_MD_LANGEVIN (1)", (int)p->thermostat);
    if (p->thermostat == VSSR_MD_LANGEVIN) {
        if (!(std::isfinite(p->friction) && p->friction > 0.0))
            return set_err(h, VSSR_E_BADARG, "vssr_batch_md: Langevin friction %g 1/fs (finite and > 0 wanted)", p->friction);
        if (!(std::isfinite(p->temperature) && p->temperature >= 0.0) || !(std::isfinite(p->temperature_end) && p->temperature_end >= 0.0))
            return set_err(h, VSSR_E_BADARG, "vssr_batch_md: Langevin temperatures %g K, %g K (finite and >= 0 wanted)", p->temperature, p->temperature_end);
        if (p->ramp_steps < 0) return set_err(h, VSSR_E_BADARG, "vssr_batch_md: ramp_steps %lld < 0", (long long)p->ramp_steps);
    }
    if (int rc = md_masses_ok(h, __func__, mass)) return rc;
    if (!h->md_vel_valid)
        return set_err(h, VSSR_E_STATE, "vssr_batch_md: the resident batch has no velocities (vssr_batch_md_set_velocities / _draw_velocities)");
    VSSR_HIP(h, hipSetDevice(h->device));
    // one workgroup integrates one chain for the whole call (k_md_chain, chain_min.hip: where the handle's driver setting asks for it
    // and the kernel applies); else the lock-step driver above.  Same results bit for bit.
    const bool resident = chain_md_supported(h);
    MdWork W;
    if (int rc = md_begin(h, p, mass, fixed, chain_id, want, W)) return rc;
    if (int rc = resident ? chain_md(h, W) : md_lockstep(h, W, want)) return rc;
    if (int rc = md_end(h, W, thermo)) return rc;
    h->md_last_driver = resident ? VSSR_MD_DRIVER_RESIDENT : VSSR_MD_DRIVER_LOCKSTEP;
    // (the lock-step driver leaves the batch-wide graph of its last evaluation, the chain-resident one numbers its rows per chain:
    // introspection wants one plain run first)
    return relax_results(h, resident, pos_out, {n_done, stop_reason});
}

int vssr_batch_md_driver(vssr_handle *h, int32_t driver, int32_t *last_used) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (driver > VSSR_MD_DRIVER_RESIDENT)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_md_driver: driver %d is none of 0 (automatic), 1 (lock-step), 2 (chain-resident)", (int)driver);
    if (driver >= 0) h->md_driver = driver;
    if (last_used) *last_used = h->md_last_driver;
    return VSSR_OK;
}

}  // extern "C"
