/*
 * vssr_eval.h — C ABI of the MI355X (gfx950) energy/force evaluation backend for VSSR-MC.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * has no FFI today: its ASE calculators call into nff/torch and LAMMPS.  Each entry point below
 * names the reference interface it replaces (paths relative to the reference repo):
 *
 *   vssr_create / vssr_destroy      <- EnsembleNFFSurface.__init__ + load_model x3
 *                                      (mcmc/calculators/calculators.py:366-377,
 *                                       scripts/sample_surface.py:164-175)
 *   vssr_eval / vssr_eval_batch     <- EnsembleNFFSurface.calculate -> EnsembleNFF.calculate
 *                                      (mcmc/calculators/calculators.py:468-489, :484) including
 *                                      AtomsBatch.update_nbr_list (mcmc/dynamics.py:129,
 *                                      mcmc/utils/misc.py:34-42)
 *   vssr_batch_upload / _run / _download / _set_positions
 *                                   <- the same call split into its H2D / compute / D2H parts so
 *                                      a relaxation loop (mcmc/dynamics.py:133-143) can keep the
 *                                      batch resident in HBM between force calls
 *   vssr_tersoff_create / vssr_tersoff_eval_batch
 *                                   <- LAMMMPSCalc.run_lammps_calc / run_lammps_energy with
 *                                      pair_style tersoff (mcmc/calculators/calculators.py:507-640)
 *   vssr_sw_create / vssr_sw_eval_batch
 *                                   <- the same with pair_style sw, or pair_style kim with the
 *                                      Stillinger-Weber Si model (tutorials/Si_111_5x5)
 *   vssr_pair_create / vssr_pair_eval_batch
 *                                   <- the same with pair_style lj/cut, morse, buck, born, coul/dsf
 *                                      and hybrid / hybrid/overlay of them
 *   vssr_gmm_create / vssr_gmm_score_rows / vssr_gmm_score_batch
 *                                   <- GMMUncertainty.estimate_log_prob / negative_log_likelihood
 *                                      (mcmc/uncertainty/uncertainty.py:238-463)
 *   vssr_gmm_fit_*                  <- gmm.GaussianMixture.fit / GMMUncertainty.fit_gmm (EM on the device)
 *
 * Conventions
 *   - All arrays are caller-allocated and borrowed only for the duration of the call.
 *   - Positions are double [N][3] (Angstrom), cell is double[9] with rows = lattice vectors,
 *     pbc is uint8[3].  Results are float32 (fp32 state and fp32-level arithmetic, like the reference: matrix products
 *     run as exact-split fp16 pieces with fp32 accumulation).
 *   - A batch is a list of independent configurations (Markov chains), concatenated:
 *     n_atoms[B], then Z / pos / forces concatenated in chain order.
 *   - Status codes: 0 ok, <0 error (see VSSR_E_*); vssr_last_error() gives the message.
 *     Non-finite energies are returned, not raised (the +-1000 clamp is the caller's job,
 *     mcmc/dynamics.py:159-168).
 *   - A handle is not re-entrant; distinct handles are independent (one per GPU / stream) and may be driven from
 *     different host threads at the same time (mc.ConcurrentChains does).
 *     Calls are synchronous unless stated.
 *
 * Weight blob layout (float32, little endian), F=feat_dim, R=n_rbf, H=readout_hidden:
 *   embed [n_embed][F]
 *   for l in 0..num_conv-1:
 *     msg.W1 [F][F], msg.b1 [F], msg.W2 [3F][F], msg.b2 [3F], msg.Wd [3F][R], msg.bd [3F],
 *     upd.U [F][F], upd.V [F][F], upd.W3 [F][2F], upd.b3 [F], upd.W4 [3F][F], upd.b4 [3F]
 *   readout.W5 [H][F], readout.b5 [H], readout.w6 [H], readout.b6 [1]
 * (torch Linear layout W[out][in]; nff state-dict keys in surface-sampling_amd/checkpoint.py).
 */
#ifndef VSSR_EVAL_H
#define VSSR_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSSR_ABI_VERSION 1

enum {
    VSSR_OK = 0,
    VSSR_E_BADARG = -1,
    VSSR_E_DEVICE = -2,   /* HIP runtime error */
    VSSR_E_CAPACITY = -3, /* neighbor capacity exceeded even after regrow / LDS limits */
    VSSR_E_NOMEM = -4,
    VSSR_E_STATE = -5     /* call sequence error (e.g. run before upload) */
};

/* `want` bitmask */
enum {
    VSSR_WANT_ENERGY = 1u,
    VSSR_WANT_FORCES = 2u,
    VSSR_WANT_STD = 4u,       /* ensemble std of energy / forces */
    VSSR_WANT_PER_MODEL = 8u, /* per-model energies */
    VSSR_WANT_PER_ATOM = 16u  /* per-atom energies (Tersoff: pe/atom) */
};

typedef struct vssr_handle vssr_handle;

typedef struct {
    uint32_t struct_size; /* sizeof(vssr_painn_config), for forward compatibility */
    int32_t device;       /* HIP device ordinal */
    /* ensemble */
    int32_t n_models;
    const float *const *weights; /* n_models blobs in the layout above */
    uint64_t weights_len;        /* floats per blob */
    /* PaiNN hyper-parameters (params.json of the reference checkpoints) */
    int32_t feat_dim;       /* 128; any multiple of 16 in 16 .. 256 is accepted */
    int32_t n_rbf;          /* 20; 1 .. 32.  (128, 20) runs the specialised path, every other shape the general-width fp32
                               path (painn_gen.hip); the environment variable VSSR_PAINN_PATH=general sends (128, 20) there too */
    int32_t num_conv;       /* 3 */
    int32_t n_embed;        /* rows of the embedding table, 100 */
    int32_t readout_hidden; /* 64 */
    float cutoff;           /* 5.0 A */
    int32_t excl_vol;       /* 1 -> add sum_e (excl_sigma/d_e)^excl_power */
    int32_t excl_power;     /* 12 */
    float excl_sigma;       /* 1.5 A */
    /* EnsembleNFF unit handling: E_eV = E_model / model_units_per_ev + offset */
    double model_units_per_ev;  /* 23.0605 for kcal/mol models */
    const double *offset_per_z; /* [n_embed] eV per atom of species Z, or NULL */
    double offset_const;        /* eV per structure (applied only when offset_per_z != NULL) */
} vssr_painn_config;

typedef struct {
    float *energy;        /* [B]            ensemble mean, eV (incl. offset)            */
    float *energy_std;    /* [B]            population std over models (WANT_STD)       */
    float *forces;        /* [sum N][3]     -mean gradient, eV/A (WANT_FORCES)          */
    float *forces_std;    /* [sum N][3]     (WANT_FORCES|WANT_STD)                      */
    float *energy_models; /* [B][n_models]  (WANT_PER_MODEL)                            */
    float *energy_atoms;  /* [sum N]        per-atom energies where defined (PER_ATOM)  */
} vssr_out;

/* ---- PaiNN ensemble ------------------------------------------------------------------- */
int vssr_abi_version(void);
/* Environment variables -- test / measurement hooks, none is needed in production (eleven; the knobs of experiments that were
 * measured and dropped are gone with their code: profiles/EXPERIMENTS.md).  Read once by vssr_create:
 *   VSSR_EDGE_IMPL=gather    every chain takes the gather neighbor kernels (reference path of the parity tests)
 *   VSSR_L0_FACTORISE=0      layer 0 runs the generic kernels instead of the species factorisation
 *   VSSR_EDGE_FS16_MAX=n, VSSR_EDGE_FS8_MAX=n   largest chain (atoms) served by the single-pass 16- / 8-feature-slice kernels
 *                            (tests: lower = force the path of larger chains onto small structures)
 *   VSSR_EDGE_FWD_2PASS=0|8|16, VSSR_EDGE_BWD_MPASS=0|1|2, VSSR_EDGE_SUB_CHUNK=n
 *                            large chains (forward: > 405 atoms, reverse: > 557): 16-feature slices in several passes over sub-ranges of
 *                            the chain's neighbors (the default) instead of the narrower single-pass kernels (FWD_2PASS=0 /
 *                            BWD_MPASS=0); 8: the forward multi-pass form on 8-feature slices; BWD_MPASS=2 + SUB_CHUNK=n (tests):
 *                            every chain takes the multi-pass forms, ranges of n atoms
 *   VSSR_UPD_SAVE=1          update blocks store their forward intermediates for the reverse pass (measured: no gain; kept because
 *                            the parity tests use it as an independent second path through the reverse update kernel)
 *   VSSR_DEBUG_KEEP=1        materialise buffers that only vssr_debug_read consumes (the last block's vector output)
 * Read by every vssr_batch_relax_cg call:
 *   VSSR_CG_FUSED=0|1        0: always the lock-step driver (one batch-wide evaluation per launch sequence), whatever the kind of
 *                            handle and its vssr_batch_relax_cg_driver setting; 1: a Tersoff handle takes the chain-resident minimiser
 *                            (one workgroup relaxes one chain from start to stop, csrc/chain_min.hip) whenever it applies (chains of
 *                            <= 256 atoms), SW / EAM / pair handles are not affected; unset: the handle's setting decides
 *                            (vssr_batch_relax_cg_driver; its default takes the chain-resident minimiser for Tersoff batches of
 *                            <= 3 072 chains of <= 64 atoms).  Same results bit for bit either way
 *   VSSR_RELAX_COMPACT=0     no live-chain compaction of the resident batch (default on for resident batches of >= 65 536 atoms: once
 *                            at most 3/4 of the chains are still minimising, the batch continues as a smaller one; same trajectories
 *                            bit for bit); n > 1: compact batches of >= n atoms (tests: 2 = always) */
int vssr_create(const vssr_painn_config *cfg, vssr_handle **out);
void vssr_destroy(vssr_handle *h);
const char *vssr_last_error(const vssr_handle *h); /* h may be NULL: last create() error of the calling thread */

/* One configuration (what one ASE calculate() call is). */
int vssr_eval(vssr_handle *h, int32_t n_atoms, const int32_t *Z, const double *pos,
              const double cell[9], const uint8_t pbc[3], uint32_t want, vssr_out *out);

/* B independent configurations in one lock-step evaluation (upload + run + download). */
int vssr_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *Z,
                    const double *pos, const double *cell /*[B][9]*/, const uint8_t *pbc /*[B][3]*/,
                    uint32_t want, vssr_out *out);

/* The same, split: keep the batch resident in HBM across a relaxation loop. */
int vssr_batch_upload(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *Z,
                      const double *pos, const double *cell, const uint8_t *pbc);
int vssr_batch_set_positions(vssr_handle *h, const double *pos /*[sum N][3]*/);
int vssr_batch_run(vssr_handle *h, uint32_t want); /* asynchronous on the handle's stream */
int vssr_batch_download(vssr_handle *h, uint32_t want, vssr_out *out); /* synchronises */
int vssr_synchronize(vssr_handle *h);

/* ---- lock-step relaxation of the resident batch (reference optimize_slab, mcmc/dynamics.py:83-170) ---- */
typedef struct {
    int32_t max_steps; /* relax_steps (reference default 20) */
    float fmax;        /* convergence: max_i |F_i| < fmax (reference: 0.01 eV/A) */
    /* ASE FIRE parameters (ase/optimize/fire.py defaults: 0.1, 0.2, 1.0, 1.1, 0.5, 0.1, 0.99, 5) */
    float dt, maxstep, dtmax, finc, fdec, astart, fa;
    int32_t nmin;
} vssr_fire_params;
/* FIRE-relaxes every chain of the resident batch in lock step (forces and positions stay in HBM).
 * fixed: [sum N] 1 = atom held by FixAtoms (force zeroed), NULL = all free.  Afterwards the batch holds the
 * relaxed positions and the results of the last evaluation: fetch them with vssr_batch_download;
 * pos_out [sum N][3], n_steps [B], converged [B] may each be NULL. */
int vssr_batch_relax_fire(vssr_handle *h, const vssr_fire_params *params, const uint8_t *fixed, uint32_t want,
                          double *pos_out, int32_t *n_steps, uint8_t *converged);

/* ASE BFGS (ase/optimize/bfgs.py: alpha = 70 eV/A^2, maxstep = 0.2 A) -- the optimizer of the reference's SrTiO3
 * configuration (scripts/configs/sample_config_painn.json:26 "optimizer": "BFGS", dispatched at mcmc/dynamics.py:119-141).
 * Same contract as vssr_batch_relax_fire.  The per-chain Hessian is kept in factored form H = alpha I + Q B Q^T; its
 * on-chip workspace holds 98 basis vectors, two for the first update and one for each later one: 96 updates.  Identical to ASE
 * for the first 97 steps, later steps keep that Hessian (csrc/relax.hip; tests/test_relax_gpu_branches.py follows it step for step). */
typedef struct {
    int32_t max_steps; /* relax_steps (reference: 20) */
    float fmax;        /* 0.01 eV/A */
    float alpha;       /* initial Hessian, 70 eV/A^2 */
    float maxstep;     /* longest atomic displacement per step, 0.2 A */
} vssr_bfgs_params;
int vssr_batch_relax_bfgs(vssr_handle *h, const vssr_bfgs_params *params, const uint8_t *fixed, uint32_t want,
                          double *pos_out, int32_t *n_steps, uint8_t *converged);

/* Trajectory recording during vssr_batch_relax_fire / _bfgs -- the reference's TrajectoryObserver attached with
 * `dyn.attach(obs, interval=record_interval)` (mcmc/dynamics.py:20-80,131-151; optimize_slab(save_traj=True, record_interval=5)).
 * record_interval > 0 arms it for the following relaxations of this handle (0 = off, the default): every chain records its
 * positions, forces (FixAtoms applied) and energy after 0, k, 2k, ... optimizer steps, like ASE calls the observer.
 * vssr_batch_traj_read: max_records (may be NULL) = relax_steps / k + 1 of the last relaxation; with buffers of
 * cap_records >= max_records: n_records [B] = valid records of every chain, pos [R][sum N][3], forces [R][sum N][3],
 * energy [R][B] (record-major; entries of a chain beyond its n_records are undefined).  Any pointer may be NULL. */
int vssr_batch_traj_configure(vssr_handle *h, int32_t record_interval);
int vssr_batch_traj_read(vssr_handle *h, int32_t cap_records, int32_t *n_records, double *pos, float *forces, double *energy,
                         int32_t *max_records);

/* LAMMPS `min_style cg` + `minimize etol ftol maxiter maxeval` for the analytic (fp64) potentials -- the reference relaxes
 * GaN with it ("optimizer": "LAMMPS": mcmc/dynamics.py:107-116 -> LAMMMPSCalc.run_lammps_opt, mcmc/calculators/calculators.py:600-619,
 * template tutorials/data/GaN_0001/GaN_0001_lammps_opt_template.txt: `fix 2 bulk setforce 0 0 0`, `min_style cg`,
 * `minimize 1e-5 1e-5 {relax_steps} 10000`).  Polak-Ribiere conjugate gradients with LAMMPS' quadratic line search
 * (dmax 0.1 A per coordinate and line search), restated from LAMMPS min_cg.cpp / min_linesearch.cpp; the analytic
 * (Tersoff, EAM, SW, pair) handles only (fp64 energies drive the line search).  stop_reason [B] (may be NULL): 1 energy tolerance, 2 force tolerance,
 * 3 maxiter, 4 maxeval, 5 search direction not downhill, 6 zero force, 7 zero quadratic step, 8 zero alpha. */
typedef struct {
    int32_t max_iter;  /* relax_steps (reference GaN: 100) */
    int32_t max_eval;  /* 10000; >= 0, tested once per iteration behind the line search (0: stop after the first one, as LAMMPS) */
    double etol, ftol; /* 1e-5, 1e-5 */
    double dmax;       /* 0.1 */
} vssr_cg_params;
/* Two drivers, same results bit for bit (csrc/chain_min.hip, csrc/relax_cg.hip; VSSR_CG_FUSED / VSSR_RELAX_COMPACT above).  The
 * chain-resident one minimises every chain with ONE workgroup from the first evaluation to the stop criterion (no lock step: the GaN
 * chains of the reference stop after 21 .. 159 evaluations each); it serves Tersoff, Stillinger-Weber, EAM (funcfl, alloy, fs) and
 * pair handles whose largest chain has <= 256 atoms.  The lock-step one evaluates the whole batch per step, with the resident batch
 * compacted to the chains still minimising once it is large enough for that to pay.  Which one runs: vssr_batch_relax_cg_driver
 * below.  The automatic choice takes the chain-resident driver for Tersoff batches of <= 3 072 chains of <= 64 atoms (the measured
 * regime) and the lock-step driver for everything else; VSSR_CG_FUSED=0 forces lock step, VSSR_CG_FUSED=1 chain-resident on Tersoff.
 * State of the handle afterwards: positions, energies, per-atom energies and forces are those of the minimised geometries with
 * either driver.  The resident neighbor GRAPH differs: the lock-step driver leaves the batch-wide graph of the final evaluation
 * (vssr_batch_stats / vssr_batch_neighbors work at once), the chain-resident driver numbers its rows per chain and leaves no
 * batch-wide graph -- those two calls return VSSR_E_STATE until one vssr_batch_run has been made. */
int vssr_batch_relax_cg(vssr_handle *h, const vssr_cg_params *params, const uint8_t *fixed, uint32_t want,
                        double *pos_out, int32_t *n_iter, int32_t *n_eval, int32_t *stop_reason);
/* The driver of vssr_batch_relax_cg for this handle.  AUTO (the default): the rule above.  LOCKSTEP / RESIDENT force one; RESIDENT
 * applies where the chain-resident kernel does (Tersoff / SW / EAM / pair handle, largest chain of the resident batch <= 256 atoms),
 * any other batch runs in lock step without an error.  VSSR_CG_FUSED, when set, goes first as described above.
 * driver >= 0: set the handle's choice for later vssr_batch_relax_cg calls; driver < 0: leave it.
 * last_used (may be NULL): the driver the last vssr_batch_relax_cg of this handle ran (0 = none yet, 1 lock-step, 2 chain-resident).
 * VSSR_E_BADARG: a driver value above 2, or a PaiNN handle (it has no CG). */
enum { VSSR_CG_DRIVER_AUTO = 0, VSSR_CG_DRIVER_LOCKSTEP = 1, VSSR_CG_DRIVER_RESIDENT = 2 };
int vssr_batch_relax_cg_driver(vssr_handle *h, int32_t driver, int32_t *last_used);

/* ASE BFGSLineSearch (ase/optimize/bfgslinesearch.py + ase/utils/linesearch.py: alpha = 10, maxstep = 0.2, c1 = 0.23, c2 = 0.46,
 * stpmax = 50; fixed inside: stpmin 1e-8, xtol 1e-14, xtrapl 1.1, xtrapu 4.0) in lock step on every handle kind that relaxes: PaiNN
 * (fp64 ensemble-mean energy, fp32 forces widened), Tersoff, SW, EAM and pair (fp64 throughout).  A trial of a line search costs one
 * batch-wide evaluation; the evaluation that ends a line search opens the next step (csrc/bfgsls_dev.h, csrc/relax_bfgsls.hip).
 * PROVENANCE: restated from the two ASE files as remembered and NOT pinned by an executed ASE (it cannot be installed next to this
 * project); the contract is the numpy restatement tests/bfgsls_oracle.py, whose interpolation is scipy's MINPACK-2 dcstep.
 * Parameters are doubles so that the restatement sees the same values.  max_eval: evaluations a chain may spend (>= 1; the Python
 * default is 20 max_steps + 20).  n_steps / n_eval / stop_reason [B], pos_out [sum N][3] may each be NULL.  stop_reason: 1 converged
 * (max_i |F_i| < fmax, tested when a step opens), 2 max_steps, 3 the line search failed (where ASE raises "LineSearch failed!";
 * positions back at the point the step opened at), 4 max_eval spent (positions at the best point of the interrupted search),
 * 5 non-finite energy or force (positions back at the point the step opened at).  One chain's failure is never an error of the call.
 * Afterwards the batch holds the final positions and a complete evaluation of them over all chains (download, vssr_batch_stress,
 * vssr_batch_results_f64, vssr_batch_stats work at once).  With vssr_batch_traj_configure armed a chain records at the evaluations that
 * open a step (steps % interval == 0), never at a line-search trial.  No live-chain compaction, no chain-resident form.
 * VSSR_E_BADARG (with a message): max_steps < 0, max_eval < 1, fmax / alpha / maxstep <= 0, c1 or c2 outside (0, 1), stpmax < 1. */
typedef struct { int32_t max_steps, max_eval; double fmax, alpha, maxstep, c1, c2, stpmax; } vssr_bfgsls_params;
int vssr_batch_relax_bfgs_linesearch(vssr_handle *h, const vssr_bfgsls_params *p, const uint8_t *fixed, uint32_t want,
                                     double *pos_out, int32_t *n_steps, int32_t *n_eval, int32_t *stop_reason);

/* ---- molecular dynamics of the resident batch (csrc/md_dev.h, csrc/md.hip, k_md_chain in csrc/chain_min.hip) ----
 * Velocity Verlet (VSSR_MD_NVE) and Langevin BAOAB (VSSR_MD_LANGEVIN; Leimkuhler & Matthews 2013) on every handle kind that relaxes:
 * PaiNN (fp64 ensemble-mean energy, fp32 forces widened), Tersoff, SW, EAM / ADP, Vashishta and pair handles with and without k-space.
 * All integrator arithmetic is fp64.  Units: A, eV, fs, amu, K; velocities in A / fs, friction in 1 / fs; kB = 8.617333262e-5 eV / K,
 * 1 eV / amu = (1.602176634e-19 / 1.66053906660e-27) 1e-10 A^2 / fs^2.  The numpy restatement is tests/md_oracle.py.
 * One step n = step0 + (steps completed in this call), with a = F / m in A / fs^2:
 *   NVE       v += (dt/2) a;  r += dt v;                                                              [evaluate]  v += (dt/2) a
 *   Langevin  v += (dt/2) a;  r += (dt/2) v;  v = c1 v + sqrt((1 - c1^2) kB T_n / m) xi;  r += (dt/2) v;  [evaluate]  v += (dt/2) a
 * c1 = exp(-friction dt); T_n runs linearly from `temperature` at n = 0 to `temperature_end` at n = ramp_steps and stays there
 * (ramp_steps = 0: temperature_end throughout).  xi: standard normals from Philox4x32-10 keyed by (seed, chain id) and counted by
 * (n, atom index within the chain, draw tag) -- the bit layout is written out in csrc/md_dev.h -- so a chain's trajectory depends on
 * neither its place in a batch nor the batch around it, and a repeated evaluation (capacity regrow) draws nothing twice.
 * Atoms under `fixed` (1 = held, NULL = all free) have v = 0, draw no noise and never move.  No centre-of-mass removal.
 * Velocities are resident on the handle between calls: vssr_batch_md_set_velocities (NULL = zeros) or _draw_velocities
 * (Maxwell-Boltzmann, v = sqrt(kB T / m) xi per component under its own draw tag, held atoms 0) put them there, vssr_batch_upload voids
 * them, _get_velocities reads them.  vssr_batch_md and _get_velocities without velocities: VSSR_E_STATE.
 * vssr_batch_md: mass [sum N] amu; chain_id [B] global chain ids (NULL = 0 .. B-1); thermo (may be NULL)
 * [n_steps / thermo_interval + 1][B][2] = (E_pot, E_kin = 1/2 sum m v^2) in eV after 0, k, 2k, ... steps of this call (record 0 is the
 * state the call found; records a chain did not reach are NaN); n_done [B] steps completed; stop_reason [B]: 1 all n_steps taken,
 * 2 a non-finite energy or force (positions and velocities are those of the last completed step).  One chain's blow-up is never an
 * error of the call.  pos_out, thermo, n_done, stop_reason may each be NULL.
 * RESUMABLE: two calls of n steps, the second with step0 = n, leave what one call of 2 n steps leaves, bit for bit (that is how
 * callers take frames; there are no trajectory rings for MD).  Afterwards the batch holds the final positions and a complete
 * evaluation of them over all chains: download and vssr_batch_results_f64 work at once with either driver; vssr_batch_stress,
 * vssr_batch_stats and vssr_batch_neighbors at once after the lock-step driver, after one vssr_batch_run behind the chain-resident one
 * (it numbers its rows per chain and leaves no batch-wide graph, as the chain-resident CG).
 * VSSR_E_BADARG (with a message, before anything moves; the handle stays usable): p or mass NULL, n_steps < 0, thermo_interval < 1,
 * dt not finite or <= 0, a mass not finite or <= 0, an unknown thermostat; Langevin: friction <= 0, a negative temperature,
 * ramp_steps < 0.  _draw_velocities: mass NULL or bad, a negative temperature.  _set_velocities: a non-finite velocity.
 * Two drivers, same results bit for bit (vssr_batch_md_driver, as vssr_batch_relax_cg_driver): LOCKSTEP evaluates the whole batch once
 * per step (every kind); RESIDENT integrates every chain with ONE workgroup for the whole call (k_md_chain, csrc/chain_min.hip: Tersoff, SW, EAM
 * funcfl / alloy / fs and pair handles without k-space whose largest chain has <= 256 atoms; any other batch runs in lock step
 * without an error); AUTO (the default) takes the chain-resident kernel for Tersoff batches of <= 256 chains of <= 64 atoms (the measured
 * regime, profiles/r29/NOTES_md.md) and the lock-step driver for everything else.  driver >= 0 sets the handle's choice, < 0 leaves it;
 * last_used (may be NULL): the driver the last vssr_batch_md ran (0 none yet, 1 lock-step, 2 chain-resident).  VSSR_E_BADARG: a value
 * above 2. */
enum { VSSR_MD_NVE = 0, VSSR_MD_LANGEVIN = 1 };
enum { VSSR_MD_DRIVER_AUTO = 0, VSSR_MD_DRIVER_LOCKSTEP = 1, VSSR_MD_DRIVER_RESIDENT = 2 };
typedef struct {
    int32_t n_steps, thermostat, thermo_interval;   /* thermo_interval >= 1 */
    double dt;                                      /* fs */
    double temperature, temperature_end, friction;  /* K, K, 1/fs (Langevin) */
    int64_t ramp_steps, step0;
    uint64_t seed;
} vssr_md_params;
int vssr_batch_md_set_velocities(vssr_handle *h, const double *vel /*[sum N][3], NULL = zeros*/);
int vssr_batch_md_draw_velocities(vssr_handle *h, const double *mass, const uint8_t *fixed, const uint64_t *chain_id,
                                  double temperature, uint64_t seed);
int vssr_batch_md_get_velocities(vssr_handle *h, double *vel);
int vssr_batch_md(vssr_handle *h, const vssr_md_params *p, const double *mass /*[sum N] amu*/, const uint8_t *fixed /*or NULL*/,
                  const uint64_t *chain_id /*[B], NULL = 0..B-1*/, uint32_t want, double *pos_out,
                  double *thermo /*[n_steps / thermo_interval + 1][B][2]*/, int32_t *n_done, int32_t *stop_reason);
int vssr_batch_md_driver(vssr_handle *h, int32_t driver, int32_t *last_used);

/* ---- constant-pressure and weakly-coupled MD of the resident batch (csrc/md_npt.hip) ----
 * The step of vssr_batch_md with a Berendsen thermostat, a Berendsen barostat (isotropic or per axis) or stochastic cell rescaling
 * around it, on every handle kind vssr_batch_md serves.  LOCK STEP ONLY: one evaluation per time step, with a barostat the kind's
 * stress kernels behind it, then one kernel launch; vssr_batch_md_driver(RESIDENT) does not apply to this entry point.
 * CONTRACT: restated from ASE (NVTBerendsen, NPTBerendsen, Inhomogeneous_NPTBerendsen) and from Bernetti & Bussi, J. Chem. Phys. 153,
 * 114107 (2020) as remembered -- not pinned by an executed library.  The contract is this comment and the numpy restatement
 * tests/npt_oracle.py.  Units as vssr_batch_md (A, eV, fs, amu, K, its kB and its eV / amu); pressure in eV / A^3, compressibility
 * beta in A^3 / eV.  All arithmetic is fp64.  Row vectors; cell rows are lattice vectors.
 * Per chain, behind one evaluation (E, f, and with a barostat the virial stress sigma in the sign and volume convention of
 * vssr_batch_stress; PaiNN: the ensemble mean), with n = step0 + (steps completed in this call):
 *  1. a non-finite E, force or (with a barostat) stress component: positions, velocities AND cell (with its inverse and image
 *     counts) go back to the last completed step; stop reason 2.
 *  2. a step in flight is closed: v += (dt/2) a, exactly as vssr_batch_md.
 *  3. every thermo_interval steps a record (E_pot, E_kin, V, P): E_kin = 1/2 sum m v^2, V = |det C|, P = tr Pi / 3 with the pressure
 *     tensor Pi = -sigma + (1/V) sum m v v^T (held atoms have v = 0).  Without a barostat no stress is evaluated and P is NaN.
 *  4. after n_steps: stop reason 1.
 *  5. step n is opened, in this order:
 *     a. thermostat.  T_n: the linear ramp of vssr_batch_md (any thermostat but NONE).  NONE and LANGEVIN do nothing here (LANGEVIN
 *        takes the BAOAB step in d).  BERENDSEN: kT_kin = 2 E_kin / (3 N_free), lambda = sqrt(1 + (dt / taut)(kB T_n / kT_kin - 1))
 *        (0 where the argument is negative), clamped to [0.9, 1.1]; lambda = 1 if E_kin = 0 or no atom is free; v <- lambda v, and
 *        the kinetic part of Pi used in b is scaled by lambda^2.
 *     b. barostat, with Pi_kk the diagonal of Pi, P0 = pressure and mask[3] of 0 / 1 per Cartesian axis.  NONE: nothing (and no
 *        stress kernel runs at all).  BERENDSEN, ISOTROPIC: P = mean of Pi_kk over the masked axes, mu = 1 - (dt beta / (3 taup))
 *        (P0 - P) on the masked axes (mask 1 1 1: NPTBerendsen).  BERENDSEN, PER_AXIS: mu_k = 1 - (dt beta / (3 taup))(P0 - Pi_kk)
 *        per masked axis (mask 1 1 1, orthorhombic cell: Inhomogeneous_NPTBerendsen).  Both: D = diag(mu_k), 1 on unmasked axes;
 *        C <- C D, x <- x D for EVERY atom (held atoms ride the cell, as in vssr_batch_relax_cell), v unchanged.
 *        CRESCALE (isotropic only): d eps = -(beta / taup)(P0 - tr Pi / 3) dt + sqrt(2 kB T_n beta dt / (V taup)) xi,
 *        mu = exp(d eps / 3), C <- mu C, x <- mu x, v <- v / mu.  xi: one standard normal of the chain's Philox stream (key from
 *        (seed, chain id), counter (n, atom 0), draw tag 3, first normal of pair 0: csrc/md_dev.h; MD draws use tags 0 and 1, the dimer
 *        2).  For an ideal gas this Euler form has the stationary density p(V) ~ V^N exp(-P0 V / kB T).
 *     c. cell check, before anything of a and b is written: the new cell must be finite, its determinant keep its sign, and it must
 *        need no more periodic images along any axis (floor(cutoff / height) + 1) than the chain had when the call began; otherwise
 *        the chain stops with reason 3 at the state it was evaluated at (the step is not taken).
 *     d. integrate with the forces of this evaluation: v += (dt/2) a; x += dt v, or the Langevin BAOAB update of vssr_batch_md.
 *        ONE evaluation per step: forces are NOT recomputed after the rescaling (a stated choice of this contract).
 * thermo (may be NULL): [n_steps / thermo_interval + 1][B][4]; records a chain did not reach are NaN.  n_done [B] steps completed;
 * stop_reason [B]: 1 all n_steps taken, 2 non-finite, 3 the cell check.  One chain's stop is never an error of the call.  pos_out
 * [sum N][3], cell_out [B][9], thermo, n_done, stop_reason may each be NULL.  fixed, chain_id, mass, want as vssr_batch_md.
 * RESUMABLE: two calls of n steps, the second with step0 = n, leave what one call of 2 n steps leaves, bit for bit (positions,
 * velocities, cells, records), as long as no chain meets the image-count limit of 5c, which the second call takes from the cells the
 * first one left.  BATCH-INDEPENDENT: a chain gives the same bits alone and inside any batch.  AFTERWARDS the batch holds a complete
 * evaluation of the final state: download, vssr_batch_results_f64, vssr_batch_stress, vssr_batch_get_cell and vssr_batch_stats work at
 * once, and later runs use the new cells until the next vssr_batch_upload.
 * VSSR_E_STATE (before anything moves): no velocities; any barostat on a pair handle with k-space (as vssr_batch_relax_cell;
 * thermostat-only calls are served there).  VSSR_E_BADARG (with a message, before anything moves; the handle stays usable): p or
 * mass NULL, a non-finite parameter, n_steps < 0, thermo_interval < 1, dt <= 0, an unknown thermostat / barostat / coupling, a bad
 * mass; with a thermostat a negative temperature or ramp_steps < 0; LANGEVIN friction <= 0; BERENDSEN thermostat taut <= 0; a mask
 * entry other than 0 / 1; with a barostat taup <= 0, compressibility <= 0, an empty mask; CRESCALE with thermostat NONE, with
 * PER_AXIS, with a mask other than 1 1 1, or on a chain with an open axis; a Berendsen barostat on a chain with an open axis k
 * unless lattice vector k lies along one Cartesian axis m, the other two lattice vectors have no component along m (the rule of
 * vssr_batch_relax_cell) and mask[m] = 0 (a slab p p f along z with mask 1 1 0 is the supported surface case). */
enum { VSSR_NPT_THERMOSTAT_NONE = 0, VSSR_NPT_THERMOSTAT_LANGEVIN = 1, VSSR_NPT_THERMOSTAT_BERENDSEN = 2 };
enum { VSSR_NPT_BAROSTAT_NONE = 0, VSSR_NPT_BAROSTAT_BERENDSEN = 1, VSSR_NPT_BAROSTAT_CRESCALE = 2 };
enum { VSSR_NPT_COUPLING_ISOTROPIC = 0, VSSR_NPT_COUPLING_PER_AXIS = 1 };
typedef struct {
    int32_t n_steps, thermostat, barostat, coupling, thermo_interval;   /* thermo_interval >= 1 */
    int32_t mask[3];                                /* 0 / 1 per Cartesian axis x y z (barostat) */
    double dt;                                      /* fs */
    double temperature, temperature_end, friction;  /* K, K, 1/fs (Langevin) */
    double taut, taup;                              /* fs: Berendsen thermostat; barostat */
    double pressure, compressibility;               /* eV / A^3, A^3 / eV */
    int64_t ramp_steps, step0;
    uint64_t seed;
} vssr_npt_params;
int vssr_batch_md_npt(vssr_handle *h, const vssr_npt_params *p, const double *mass /*[sum N] amu*/, const uint8_t *fixed /*or NULL*/,
                      const uint64_t *chain_id /*[B], NULL = 0..B-1*/, uint32_t want, double *pos_out /*[sum N][3]*/,
                      double *cell_out /*[B][9]*/, double *thermo /*[n_steps / thermo_interval + 1][B][4]*/, int32_t *n_done,
                      int32_t *stop_reason);

/* ---- harmonic vibrations of the resident batch (csrc/vib.hip, csrc/jacobi_dev.h) ----
 * Finite-difference Hessian, modes, zero-point energy and vibrational Helmholtz energy of every structure of the resident batch, on
 * every handle kind that evaluates (PaiNN: fp32 ensemble-mean forces widened to fp64; Tersoff, SW, EAM / ADP, Vashishta and pair
 * handles with and without k-space: their fp64 forces).  What ASE's Vibrations (+ HarmonicThermo.get_helmholtz_energy minus the
 * potential energy) does with 6 n serial evaluations and a host eigh; restated from ASE as remembered, NOT pinned by an executed ASE.
 * The numpy restatement is tests/vib_oracle.py.
 * GROUPS AND REPLICAS.  A group is one structure, resident as n_rep[g] >= 1 identical consecutive chains (n_rep NULL: every chain is
 * its own group, n_groups = B).  Its m = 3 (vib atoms) degrees of freedom are numbered by (vib atom in chain order, x / y / z); the
 * replica of rank k works through the degrees of freedom r = k (mod n_rep[g]), replicas beyond m stay idle, so one structure's
 * displacements fill the batch.  Replicas must agree bit for bit in atom count, species, cell, pbc, masses, vib mask and positions.
 * Every displacement is one lock-step evaluation of the whole batch: nfree (largest share of a replica) + 1 evaluations, the last
 * at x0 over all chains, so download, vssr_batch_results_f64, vssr_batch_stress and vssr_batch_stats work at once afterwards and the
 * positions equal the input bit for bit (a displaced coordinate is x0 + k delta, k = -1, +1 or -2, -1, +1, +2, from a saved copy).
 * ROWS.  With F(s) the forces at displacement s delta of degree of freedom r, restricted to the vib atoms and flattened:
 *   nfree = 2: row = 0.5 (F(-1) - F(+1));  nfree = 4: row = (-F(-2) + 8 F(-1) - 8 F(+1) + F(+2)) / 12;  row /= 2 delta;
 * VSSR_VIB_FREDERIKSEN: before use, the force on the displaced atom is replaced by itself minus the sum of the forces over all atoms
 * of the chain (vib or not, in atom order).  Then H <- H + H^T: `hessian` [G][ld][ld] in eV / A^2.
 * MODES.  A = D H D, D = diag(mass^-1/2) per component; fp64 cyclic Jacobi, one workgroup per group; eigenvalues w2 ascending;
 * energies[k] = sign(w2) s sqrt(|w2|) eV with s = hbar 1e10 / sqrt(e amu) = 0.0646541513... (CODATA 2018: hbar = 1.054571817e-34,
 * e = 1.602176634e-19, amu = 1.66053906660e-27); a negative entry is an imaginary mode.  modes [G][ld][ld]: row k is the unit
 * eigenvector of A (mass-weighted, ASE's modes[k]), signed so that its largest-magnitude entry (the first on ties) is positive.
 * Entries beyond a group's m in the padded outputs are left untouched.
 * THERMO.  thermo[g] = (E_pot(x0), zpe, f_vib); over the modes with energy > e_min (imaginary ones are never in):
 *   zpe = 1/2 sum e_k;  f_vib = sum [e_k / 2 + kT log1p(-exp(-e_k / kT))], kB = 8.617333262e-5 eV / K;  T = 0: f_vib = zpe.
 * info[g] = (m, modes with w2 < 0, modes left out of the sums, stop reason): 1 done; 2 a non-finite energy or force was met at some
 * displacement (the group's energies, hessian, modes, zpe and f_vib are NaN, other groups are unaffected); 3 the Jacobi hit its sweep
 * limit (outputs are what it had).  One group's failure is never an error of the call.  A group with m = 0 has empty outputs.
 * There is no FixAtoms mask: forces are the raw forces, and a caller who wants ASE-with-FixAtoms behaviour leaves held atoms out of
 * `vib`.  The same call twice gives the same bits.  energies, hessian, modes, thermo, info may each be NULL.
 * VSSR_E_BADARG (with a message, before anything moves; the handle stays usable): p or mass NULL, nfree not 2 or 4, an unknown
 * method, delta not finite or <= 0, a mass not finite or <= 0, a negative or non-finite temperature or e_min, n_rep not summing to B
 * or holding a value < 1, n_groups != B with n_rep NULL, replicas that differ, a group with m > 256 (85 vib atoms), ld < max m.
 * VSSR_E_STATE before vssr_batch_upload.
 * Out of scope: a chain-resident driver, infrared intensities, more than 256 degrees of freedom per structure, projection of
 * rotations / translations, live-chain compaction. */
enum { VSSR_VIB_STANDARD = 0, VSSR_VIB_FREDERIKSEN = 1 };
typedef struct {
    int32_t nfree;        /* 2 (central) or 4 (five-point) */
    int32_t method;       /* VSSR_VIB_* */
    double delta;         /* A; ASE default 0.01 */
    double temperature;   /* K, >= 0 */
    double e_min;         /* eV, >= 0: modes with energy <= e_min (imaginary ones included) stay out of zpe / f_vib */
} vssr_vib_params;
int vssr_batch_vibrations(vssr_handle *h, const vssr_vib_params *p, const double *mass /*[sum N] amu*/,
                          const uint8_t *vib /*[sum N] 1 = atom is displaced and its force rows are read; NULL = all*/,
                          const int32_t *n_rep /*[G], sum = B: consecutive chains that are replicas of one structure; NULL: G = B*/,
                          int32_t n_groups, int32_t ld, uint32_t want,
                          double *energies /*[G][ld]*/, double *hessian /*[G][ld][ld]*/, double *modes /*[G][ld][ld]*/,
                          double *thermo /*[G][3]*/, int32_t *info /*[G][4]*/);

/* ---- nudged elastic band over the resident batch (csrc/neb.hip) ----
 * Minimum-energy paths between minima: the improved-tangent NEB (Henkelman & Jonsson, J. Chem. Phys. 113, 9978 (2000)), ASE's
 * `aseneb` variant and the climbing image (Henkelman, Uberuaga & Jonsson, J. Chem. Phys. 113, 9901 (2000)), relaxed by ASE's FIRE over
 * the whole band, on every handle kind that evaluates.  Restated from the papers and from ASE's neb.py / fire.py as remembered, NOT
 * pinned by an executed ASE: the contract is the numpy restatement tests/neb_oracle.py.  Everything is fp64 (PaiNN: fp32 ensemble-mean
 * forces widened, the fp64 ensemble-mean energy; the analytic kinds: their fp64 forces, never narrowed).
 * BANDS.  Band g is n_img[g] >= 3 consecutive chains of the resident batch (its images); bands may differ in length and
 * sum n_img = B.  The images of a band must agree bit for bit in atom count, species, cell, pbc and fixed mask; only positions differ.
 * The first and the last image never move, not by a bit; neither does an atom under `fixed` (1 = held, NULL = all free).
 * DISPLACEMENTS.  d(i) = x(i+1) - x(i) per atom, taken to the nearest image along the periodic axes: with s = d cell^-1 the whole
 * lattice vectors rint(s_a) (fp64, ties to even) are subtracted from d for every periodic axis a (s - rint(s) transformed back, without
 * rounding d where nothing wraps).  This is the minimum image while every atom moves less than half the smallest periodic cell height
 * between neighbouring images; there is no full minimum-image search over skewed cells.  |d| = sqrt(sum over all atoms and components).
 * NEB FORCE of interior image i from F (the raw forces, held atoms zeroed first), the energies E of the band, t1 = d(i-1), t2 = d(i);
 * imax = the first interior image of maximal energy:
 *   VSSR_NEB_IMPROVED_TANGENT  t = t2 if E(i+1) > E(i) > E(i-1); t = t1 if E(i+1) < E(i) < E(i-1); else with dmax / dmin the larger /
 *     smaller of |E(i+1) - E(i)|, |E(i-1) - E(i)|: t = t2 dmax + t1 dmin if E(i+1) > E(i-1), else t = t2 dmin + t1 dmax.  t <- t / |t|,
 *     fpar = F.t.  Climbing image (climb = 1 and i = imax): G = F - 2 fpar t; any other: G = F - fpar t + k (|t2| - |t1|) t.
 *   VSSR_NEB_ASENEB  t = t2 for i < imax, t1 for i > imax, t1 + t2 at imax (not normalised); m = t.t, fpar = F.t.
 *     Climbing image: G = F - 2 (fpar / m) t; any other: G = F - (fpar / m) t - ((k t1 - k t2).t / m) t.
 * G of a held atom is then set to zero (the tangent runs over all atoms).  An image whose tangent has zero length (two coincident
 * images) has G = F, and the band stops with reason 4 unless it has converged as it stands.
 * OPTIMIZER.  ASE FIRE (dt, maxstep, dtmax, nmin, finc, fdec, astart, fa as vssr_fire_params) on the concatenated interior images of a
 * band: v.G, G.G, v.v and the maxstep norm |dt v| run over the whole band, (dt, a, Nsteps) are per band.  |dt v| of the new velocity
 * v' = c1 v + c2 G is formed from the three sums (c1^2 v.v + 2 c1 c2 v.G + c2^2 G.G; all terms >= 0 where c1 != 0).
 * A STEP OPENS WITH THE TEST, on G of the evaluation of the current positions: 1. a non-finite energy or force in any image of the
 * band: the band goes back to the positions the step opened at and stops, reason 3 (that step is not counted); 2. max over
 * interior images and atoms of |G_atom| < fmax: converged, reason 1; 3. a zero tangent: reason 4; 4. steps == max_steps: reason 2;
 * 5. else the FIRE step.  One band's stop is never an error of the call; the other bands are unaffected.
 * OUTPUTS (each may be NULL).  pos_out [sum N][3]; energy [B]; neb_force [sum N][3] = G at the last test (zero on end images);
 * band [G][3] = (fmax at the last test, E(imax) - E(first), E(imax) - E(last)); info [G][4] = (steps taken, stop reason, imax as image
 * index within the band, 0).  neb_force, band and imax of a band that stopped with reason 3 are unspecified.
 * Afterwards the batch holds the final positions and a complete evaluation of them over all chains: download,
 * vssr_batch_results_f64, vssr_batch_stress, vssr_batch_stats and vssr_batch_vibrations work at once.  The same call twice gives the
 * same bits, and a band gives the same bits alone and inside a larger batch (fixed-order reductions, no floating-point atomics).
 * VSSR_E_BADARG (with a message, before anything moves; the handle stays usable): p or n_img NULL, n_bands < 1, an n_img entry < 3,
 * n_img not summing to B, an unknown method, climb not 0 or 1, max_steps < 0, k / fmax / dt / maxstep / dtmax not finite and > 0,
 * finc < 1, fdec or fa outside (0, 1), astart outside (0, 1], nmin < 0, images of a band that differ in anything but positions.
 * VSSR_E_STATE before vssr_batch_upload.
 * Out of scope: other optimizers over the band, IDPP interpolation, free-end / string / `eb` / spline variants, per-spring constants,
 * dynamic relaxation, a full minimum-image search, removal of rotation and translation, taking the fixed end images out of the
 * lock-step evaluation. */
enum { VSSR_NEB_IMPROVED_TANGENT = 0, VSSR_NEB_ASENEB = 1 };
typedef struct {
    int32_t max_steps;   /* FIRE steps of a band */
    int32_t method;      /* VSSR_NEB_* */
    int32_t climb;       /* 0 / 1: climbing image from the first step */
    double  k;           /* spring constant, eV / A^2 (ASE default 0.1) */
    double  fmax;        /* convergence: largest |NEB force| of an atom over the band's interior images */
    double  dt, maxstep, dtmax, finc, fdec, astart, fa;   /* ASE FIRE: 0.1 0.2 1.0 1.1 0.5 0.1 0.99 */
    int32_t nmin;        /* 5 */
} vssr_neb_params;
int vssr_batch_neb(vssr_handle *h, const vssr_neb_params *p, const uint8_t *fixed /*[sum N] or NULL*/,
                   const int32_t *n_img /*[G], each >= 3, sum = B*/, int32_t n_bands, uint32_t want,
                   double *pos_out /*[sum N][3]*/, double *energy /*[B]*/, double *neb_force /*[sum N][3]*/,
                   double *band /*[G][3]: fmax at the last test, E_max - E_first, E_max - E_last*/,
                   int32_t *info /*[G][4]: steps taken, stop reason, imax (image index within the band), 0*/);

/* ---- dimer method over the resident batch (csrc/dimer.hip) ----
 * Saddle search from ONE structure by min-mode following: the dimer of Henkelman & Jonsson, J. Chem. Phys. 111, 7010 (1999), with the
 * one-gradient rotation of Heyden, Bell & Keil, J. Chem. Phys. 123, 224101 (2005) and the force extrapolation of Kaestner & Sherwood,
 * J. Chem. Phys. 128, 014106 (2008), translated by ASE's FIRE as vssr_batch_neb restates it, on every handle kind that evaluates.
 * Restated from the three papers; it is NOT ASE's MinModeTranslate and is not pinned by any executed library: the contract is the
 * numpy restatement tests/dimer_oracle.py.  Everything is fp64 (PaiNN: fp32 ensemble-mean forces widened, the fp64 ensemble-mean
 * energy; the analytic kinds: their fp64 forces, never narrowed).
 * DIMERS.  The batch holds B = 2 G chains; dimer g is chain 2 g (the midpoint x0) and chain 2 g + 1 (the moving end x1 = x0 + delta N).
 * The two chains must agree bit for bit in atom count, species, cell, pbc and fixed mask.  The uploaded positions of chain 2 g + 1 are
 * ignored and overwritten.  mode_in / mode_out are laid out like the batch; their rows of the odd chains are not read and are zero
 * on output.  An atom under `fixed` (1 = held, NULL = all free) never moves in chain 2 g, and chain 2 g + 1 holds it where chain 2 g does.
 * MODE.  N is a unit vector over the 3 n components of the dimer's free atoms, zero on held atoms.  From mode_in: held rows are
 * zeroed, then N <- N / sqrt(N.N).  With mode_in NULL: component c of atom i is a standard normal of the Philox generator of
 * vssr_batch_md (csrc/md_dev.h: chain key from (seed, dimer_id[g]), draw index n = 0, atom i, tag 2 -- MD draws use tags 0 and 1),
 * then the same; dimer_id NULL means dimer_id[g] = g.  Then x0 <- x0 + displace N, once, before the first evaluation.
 * Forces below are the raw forces with held atoms zeroed; sums run over all atoms and components of the dimer.
 * ONE CYCLE.
 *  1. Evaluation E: chain 2 g at x0, chain 2 g + 1 at x0 + delta N give E0, F0, F1.  C = (F0.N - F1.N) / delta.  The rotation
 *     counter of this step is 0.
 *  2. Rotation test: Fd = 2 (F1 - F0), Fp = Fd - (Fd.N) N, f = |Fp|, b1 = -f / (2 delta), phi1 = atan(f / (2 delta |C|)) / 2 (IEEE
 *     division: C = 0 gives pi / 4).  A rotation is made only if the counter is below its limit (max_rot_first before the first
 *     translation, max_rot before every later one), f > 0 and phi1 >= phi_tol; otherwise go to 4.
 *  3. Trial rotation: T = Fp / f, N* = N cos phi1 + T sin phi1 (not renormalised).  Evaluation R: chain 2 g + 1 at x0 + delta N*;
 *     chain 2 g is evaluated again at x0, its result is ignored and F0, E0 of evaluation E are kept.  With F1* of evaluation R:
 *     C1 = (F0.N* - F1*.N*) / delta, a1 = (C - C1 + b1 sin 2 phi1) / (1 - cos 2 phi1), a0 = 2 (C - a1), phim = atan(b1 / a1) / 2 (IEEE
 *     division), Cm = a0 / 2 + a1 cos 2 phim + b1 sin 2 phim; if Cm > C: phim += pi / 2 and Cm is formed again.  The end force of the
 *     rotated dimer is extrapolated, no evaluation is spent on it:
 *     F1 <- [sin(phi1 - phim) / sin phi1] F1 + [sin phim / sin phi1] F1* + [1 - cos phim - sin phim tan(phi1 / 2)] F0.
 *     N <- N cos phim + T sin phim, divided by its norm; C <- Cm; counter + 1; back to 2 with the extrapolated F1.
 *  4. Step test, on F0 of the last evaluation E, in this order: a non-finite energy or force in either chain, at E or at R: x0 and N
 *     go back to the values the step opened at (those of the input after `displace` before the first translation), chain 2 g + 1 to
 *     x0 + delta N, the dimer stops with reason 3 and that step is not counted; max over atoms of |F0_atom| < fmax and C < 0:
 *     reason 1; steps == max_steps: reason 2; otherwise translate.  (The finiteness test stands at the head of every visit.)
 *  5. Translation: G = F0 - 2 (F0.N) N if C < 0, else G = -(F0.N) N.  One ASE FIRE step on G (dt, maxstep, dtmax, nmin, finc, fdec,
 *     astart, fa and the rule of vssr_batch_neb, the maxstep clamp on |dt v'| formed from the three sums v.v, v.G, G.G); its state
 *     (v, dt, a, Nsteps) belongs to the dimer.  steps + 1; evaluation E of the next step at the new x0 with the current N.
 * OUTPUTS (each may be NULL).  pos_out [sum N][3]; energy [B]; mode_out [sum N][3]; dimer [G][4] = (largest |F0_atom| at the last
 * step test, curvature C, E0, f = |Fp| at the last rotation test); info [G][4] = (translation steps, stop reason, rotations made,
 * lock-step evaluations the dimer consumed: its E and R evaluations, the one that showed a non-finite value included; the closing
 * evaluation of the call is not counted).  dimer [g] of a dimer that stopped with reason 3 is that of its last complete step test.
 * Afterwards chain 2 g holds x0 and chain 2 g + 1 holds x0 + delta N of the final state, and a complete evaluation of all chains is
 * resident: download, vssr_batch_results_f64, vssr_batch_stress, vssr_batch_stats and vssr_batch_vibrations work at once.  One
 * dimer's stop is never an error of the call.  The same call twice gives the same bits, and a dimer gives the same bits alone and
 * inside a larger batch (fixed-order reductions, no floating-point atomics); dimer_id, not the place in the batch, decides a drawn mode.
 * VSSR_E_BADARG (with a message, before anything moves; the handle stays usable): p NULL, an odd number of chains, max_steps /
 * max_rot_first / max_rot / nmin < 0, delta / fmax / dt / maxstep / dtmax not finite and > 0, finc < 1, fdec or fa outside (0, 1),
 * astart outside (0, 1], phi_tol outside (0, pi / 4], a non-finite displace, a mode_in of zero or non-finite length over a dimer's
 * free atoms (with mode_in NULL: a dimer without a free atom), the two chains of a dimer differing in anything but positions.
 * VSSR_E_STATE before vssr_batch_upload.
 * Out of scope: conjugate-gradient or L-BFGS rotation directions, L-BFGS translation, a central-difference dimer, taking the idle
 * midpoint out of evaluation R, a cap on the distance travelled, removal of rotation and translation, deduplication of the saddles
 * found. */
typedef struct {
    int32_t max_steps;       /* translation steps of a dimer */
    int32_t max_rot_first;   /* rotations allowed before the first translation (>= 0) */
    int32_t max_rot;         /* rotations allowed before every later translation (>= 0) */
    int32_t nmin;            /* FIRE */
    double  delta;           /* dimer half-length, A: x1 = x0 + delta N */
    double  phi_tol;         /* rad: a rotation whose trial angle is below this is not made */
    double  fmax;            /* eV / A: convergence on the largest |F0| of an atom, with C < 0 */
    double  displace;        /* A: x0 <- x0 + displace N before the first evaluation (0: none) */
    double  dt, maxstep, dtmax, finc, fdec, astart, fa;   /* ASE FIRE, as vssr_neb_params */
    uint64_t seed;           /* starting modes when mode_in is NULL */
} vssr_dimer_params;
int vssr_batch_dimer(vssr_handle *h, const vssr_dimer_params *p, const uint8_t *fixed /*[sum N] or NULL*/,
                     const double *mode_in /*[sum N][3] or NULL*/, const uint64_t *dimer_id /*[G] or NULL: g*/, uint32_t want,
                     double *pos_out /*[sum N][3]*/, double *energy /*[B]*/, double *mode_out /*[sum N][3]*/,
                     double *dimer /*[G][4]: fmax at the last test, curvature C, E0, largest |F_perp| seen at the last rotation test*/,
                     int32_t *info /*[G][4]: translation steps, stop reason, rotations made, lock-step evaluations the dimer took part in*/);

/* ---- variable-cell relaxation of the resident batch (csrc/relax_cell.hip) ------------------------------------------------------
 * Atoms and cell of every chain relaxed together on the device, in lock step: ASE's UnitCellFilter (ase/filters.py) under ASE's FIRE
 * (ase/optimize/fire.py), in fp64.  SERVED: every handle kind that evaluates (PaiNN, Tersoff, SW, EAM / ADP, Vashishta, pair) except
 * pair handles with k-space, which are refused with VSSR_E_STATE (the message names ew_stride: the S(k) array was sized from the
 * uploaded cells).  CONTRACT: restated from ASE as remembered -- ASE was not installed where this was written, so it is not pinned by
 * an executed ASE.  The contract is this comment and the numpy restatement tests/cellrelax_oracle.py, whose row force is checked
 * to be the exact negative gradient of the enthalpy E + p V (tests/test_cellrelax_cpu.py).
 * COORDINATES (row vectors; cell rows are lattice vectors).  Per chain, fixed when the call starts: the cell C0 and c = cell_factor
 * (<= 0: the chain's atom count, as ASE).  State: s [N][3] and the deformation gradient F [3][3], from s = x and F = I.  Physical
 * state: x = s F^T, C = C0 F^T.  The optimizer sees N + 3 rows: s, then c F.  After an evaluation and its stress (sigma: the 3 x 3 of
 * vssr_batch_stress, ASE's sign; PaiNN: the ensemble mean), with V = |det C| and p = scalar_pressure, the row forces are formed in
 * this order:
 *  1. atoms: g_i = f_i F; rows of atoms under `fixed` are zero (they still ride the cell through x = s F^T);
 *  2. cell: W = -V (sigma + p I) F^-T;
 *  3. hydrostatic_strain: W <- (tr W / 3) I;
 *  4. W <- W o mask, the 3 x 3 of 0 / 1 built from the Voigt-6 mask (xx yy zz yz xz xy);
 *  5. the three cell rows are W / c.
 * Convergence is ASE's over all N + 3 rows, max_row |row| < fmax, tested when a step opens.  The step is ASE FIRE (dt, maxstep,
 * dtmax, nmin, finc, fdec, astart, fa) over the 3 N + 9 numbers; maxstep bounds the norm of the WHOLE step (|dt v'| formed from the
 * three sums v.v, v.G, G.G, as vssr_batch_neb); the cell rows move F by (step of c F) / c.
 * STOPS (stop_reason; one chain's stop is never an error of the call): 1 converged; 2 max_steps reached; 3 a non-finite energy,
 * force or stress: the chain goes back to the state its step opened at and that step is not counted; 4 the step's new cell would need
 * more periodic images along an axis than vssr_batch_upload gave that chain (floor(cutoff / height) + 1; fewer are fine), or has
 * det F <= 0, or is not finite: the step is not taken and the chain stays at the state it was evaluated at.
 * OUTPUTS (each may be NULL): pos_out [sum N][3], cell_out [B][9], n_steps [B], stop_reason [B], result [B][3] = (largest row force
 * at the last test, E, V at that test).  Afterwards the batch holds the final cells and positions and a complete evaluation of
 * them over all chains: download, vssr_batch_results_f64, vssr_batch_stress and vssr_batch_stats work at once, and a later
 * vssr_batch_set_positions / vssr_batch_run uses the relaxed cells until the next vssr_batch_upload.  The same call twice gives the
 * same bits, and a chain gives the same bits alone and inside any batch (fixed-order reductions, no floating-point atomics).
 * VSSR_E_BADARG (with a message, before anything moves; the handle stays usable): p NULL, max_steps < 0, fmax not finite and > 0, a
 * non-finite scalar_pressure or cell_factor, a mask entry other than 0 or 1, dt / maxstep / dtmax not finite and > 0, finc < 1, fdec
 * or fa outside (0, 1), astart outside (0, 1], nmin < 0; a chain with an open axis k unless lattice vector k lies along one
 * Cartesian axis, the other two lattice vectors have no component along that axis and the mask frees no strain component that
 * involves it (a slab p p f along z with mask 1 1 0 0 0 1 is the supported surface case).  VSSR_E_STATE before vssr_batch_upload
 * and for a pair handle with k-space.
 * Out of scope: constant_volume, ExpCellFilter / FrechetCellFilter, other optimizers over the filter, trajectory rings, k-space
 * handles. */
typedef struct {
    int32_t max_steps;
    int32_t nmin;                 /* FIRE */
    int32_t hydrostatic_strain;   /* 0 / 1 */
    int32_t mask[6];              /* 0 / 1 per strain component, Voigt order xx yy zz yz xz xy */
    double  fmax;                 /* eV / A over all N + 3 rows */
    double  scalar_pressure;      /* eV / A^3 */
    double  cell_factor;          /* <= 0: the chain's atom count */
    double  dt, maxstep, dtmax, finc, fdec, astart, fa;   /* ASE FIRE, as vssr_neb_params */
} vssr_cell_relax_params;
int vssr_batch_relax_cell(vssr_handle *h, const vssr_cell_relax_params *p, const uint8_t *fixed /*[sum N] or NULL*/, uint32_t want,
                          double *pos_out /*[sum N][3]*/, double *cell_out /*[B][9]*/, int32_t *n_steps /*[B]*/, int32_t *stop_reason /*[B]*/,
                          double *result /*[B][3]: fmax at the last test, E, V*/);
/* The cells of the resident batch as the device holds them, [B][9] (synchronises): those of vssr_batch_upload bit for bit, or what
 * vssr_batch_relax_cell left.  VSSR_E_STATE before vssr_batch_upload. */
int vssr_batch_get_cell(vssr_handle *h, double *cell /*[B][9]*/);

/* ---- introspection used by tests and bench (no effect on results) ---------------------- */
/* Per-kernel timing with HIP events on the handle's own stream.  enable=1 starts recording;
 * vssr_profile_read synchronises and returns, for each kernel class, the number of launches and
 * the summed duration since the last reset.  names[i] points to a static string. */
int vssr_profile_enable(vssr_handle *h, int enable);
int vssr_profile_reset(vssr_handle *h);
int vssr_profile_read(vssr_handle *h, int32_t cap, const char **names, int64_t *launches,
                      double *total_ms, int32_t *n_out);
/* Workload counters of the resident batch after a run: atoms, directed edges (unpadded),
 * padded edge slots.  After vssr_batch_relax_fire / _bfgs the resident graph and activations cover only the chains that
 * were still running in the last iteration: vssr_batch_stats, vssr_batch_neighbors and vssr_debug_read then return
 * VSSR_E_STATE until the batch has been run once more (vssr_batch_run); results (download) are complete at all times. */
int vssr_batch_stats(vssr_handle *h, int64_t *n_atoms, int64_t *n_edges, int64_t *n_slots);
/* Neighbor multigraph of the resident batch (after a run): for every directed edge its centre i,
 * neighbor j (global atom indices) and image shift S.  Returns the edge count through n_edges;
 * arrays may be NULL to query the size. */
int vssr_batch_neighbors(vssr_handle *h, int64_t cap, int32_t *ei, int32_t *ej, int32_t *eS,
                         float *er, int64_t *n_edges);
/* Device addresses of the per-chain results of the resident batch (energy [B], energy_std [B], fp32, valid after a
 * synchronised run): lets the multi-GPU result gather (RCCL all_gather of per-chain scalars) read
 * them in place instead of through the host.  The pointers stay valid until the next vssr_batch_upload. */
int vssr_batch_device_results(vssr_handle *h, const float **energy, const float **energy_std);
/* The same values as doubles (the device holds the ensemble mean / spread in fp64 before narrowing them to the float32 result
 * word): what the result gather of sharding.py moves between GPUs. */
int vssr_batch_device_results_f64(vssr_handle *h, const double **energy, const double **energy_std);
/* Energies of the LAST evaluation of the resident batch without the float32 output word (synchronises).  The reference's
 * results["energy"] is a float32 tensor (EnsembleNFF.calculate, mcmc/calculators/calculators.py:484) and vssr_out keeps that
 * type; but the per-chain sum over atoms, the unit conversion, the stoichiometric offset and the mean / population spread over
 * the models are formed in fp64 on the device, and at |E| ~ 2 ... 9 keV the spacing of float32 (1.2e-4 ... 4.9e-4 eV) is as
 * large as the whole arithmetic error of the evaluation.  energy [B], energy_std [B], energy_models [B][n_models]; any pointer
 * may be NULL.  Tersoff / EAM handles: energy = energy_models = the fp64 energy, energy_std = 0.  The Metropolis test of the
 * batched MC loop (mc.py) and relax_batch's returned energy take these values. */
int vssr_batch_energy_f64(vssr_handle *h, double *energy, double *energy_std, double *energy_models);
/* fp64 results of the LAST evaluation of the resident batch of an analytic (Tersoff / EAM / SW / pair) handle exactly as the device
 * holds them (synchronises; no upload, no run): energy [B], energy_atoms [sum N], forces [sum N][3]; any pointer may be NULL.
 * After vssr_batch_relax_fire / _bfgs / _cg: what the driver left, i.e. the static results of the relaxed geometries.  VSSR_E_STATE
 * before any run, for a PaiNN handle, and for forces after a run that was asked for energies only. */
int vssr_batch_results_f64(vssr_handle *h, double *energy, double *energy_atoms, double *forces);
/* Latent-space embedding: the per-atom scalar features after the last update block, [sum N][feat_dim] fp32 per model --
 * what nff's Painn returns as results["embedding"] with requires_embedding=True and the reference's clustering /
 * uncertainty helpers read (get_embeddings_single, mcmc/calculators/calculators.py:67-93; scripts/clustering.py:239).
 * model >= 0: that ensemble member; model = -1: all members, model-major [M][sum N][feat_dim].  Valid after a run of the
 * resident batch; dst may be NULL to query the size through n_out. */
int vssr_batch_embedding(vssr_handle *h, int32_t model, float *dst, int64_t cap, int64_t *n_out);
/* Range guard of the PaiNN path.  The dense contractions run as exact 2-way fp16 splits: an
 * activation or adjoint beyond +-65504 cannot be represented and is clamped -- the results stay finite but are no longer
 * the model's (seen with weights scaled far outside the trained regime).  The kernels track the largest magnitude they
 * split; flags [B] (may be NULL) receives 1 for every chain whose LAST evaluation clamped a value or produced a non-finite
 * energy, n_flagged (may be NULL) their count.  The reference has no counterpart (fp32 torch arithmetic overflows at 3e38);
 * callers treat a flagged chain like the out-of-bounds energies of mcmc/dynamics.py:159-168.  Tersoff / EAM: always 0. */
int vssr_batch_saturated(vssr_handle *h, uint8_t *flags, int32_t *n_flagged);
/* Virial stress of every chain of the resident batch from its LAST evaluation (which must have produced forces): the
 * "stress" property that nff's EnsembleNFF / the reference's EnsembleNFFSurface list in implemented_properties
 * (mcmc/calculators/calculators.py:369) and ASE's Atoms.get_stress() asks a calculator for.  Nothing is re-evaluated: the
 * reverse pass leaves dE/d r for every directed edge on the device, and sigma_ab = (1/V) sum_edges (dE/d r_a) r_b.
 * stress, stress_std (may be NULL): [B][6] fp64, Voigt order xx yy zz yz xz xy, eV / A^3, ASE's sign convention; ensemble
 * mean and population standard deviation over the models.  V = |det cell| (also for slabs with a vacuum axis, as ASE).
 * Tersoff, EAM (funcfl, eam/alloy, eam/fs, mixed) and Stillinger-Weber handles are served the same way, in fp64: the "stress" the
 * reference's LAMMPSRun fills from pxx .. pxy (mcmc/calculators/lammpsrun.py:456-465).  Tersoff / SW: from the per-slot gradients
 * dE_i / d r_ij of the last evaluation; EAM: the pair derivative of every edge is recomputed from the F'(rho) it left.  One model:
 * stress_std is all zeros.  The kernels run only inside this call; an evaluation that is not asked for stress costs nothing extra.
 * VSSR_E_STATE: before any run, for a handle of another kind, after a run that was not asked for forces, or after a relaxation that
 * left a partial graph -- a lock-step relaxation during which chains converged early, and the chain-resident CG minimiser
 * (vssr_batch_relax_cg on chains of <= 256 atoms, any analytic kind), which leaves no batch-wide gradients: run the batch once
 * (vssr_batch_run), then ask.  After a lock-step relaxation that ended with its batch-wide evaluation the stress is that of the
 * relaxed geometry. */
int vssr_batch_stress(vssr_handle *h, double *stress, double *stress_std);
/* The handle's HIP device ordinal, its stream (hipStream_t: every kernel of the handle is enqueued there) and the device
 * address of the neighbor-capacity overflow flag of the last run (int32, non-zero = the run's results are void and
 * vssr_synchronize will repeat it with grown buffers; NULL before the first run).  For consumers that order their own device
 * work behind an evaluation with events instead of a host synchronisation (the multi-GPU result gather, sharding.py). */
int vssr_device_context(vssr_handle *h, int32_t *device, void **stream, const int32_t **overflow_flag);
/* Test hook for the capacity-regrow paths: initial neighbor capacity in slots per atom (<= 0: unchanged), tight != 0:
 * regrow to the exact need only (every later growth of the edge count overflows again), tight < 0: unchanged;
 * n_regrows (may be NULL) receives the number of regrows of the last relaxation. */
int vssr_debug_capacity(vssr_handle *h, int32_t slots_per_atom, int32_t tight, int32_t *n_regrows);
/* Work counters of the LAST relaxation of this handle (vssr_batch_relax_fire / _bfgs / _cg): lockstep_evaluations = evaluations of
 * the batch the driver launched (the final static evaluation included); chain_evaluations = chain-evaluations those launches
 * dispatched (a launch over all B chains counts B even when converged chains leave their kernels at once).  Together with the
 * per-chain counts the relaxation returns (n_steps / n_eval) they give the lock-step waste: dispatched / needed. */
int vssr_batch_relax_counts(vssr_handle *h, int64_t *lockstep_evaluations, int64_t *chain_evaluations);
/* Copy a named device intermediate of model m (fp32) to host; for parity debugging.
 * Names: "phi<l>", "s_msg<l>", "v_msg<l>", "s_upd<l>", "v_upd<l>", "sbar_msg<l>", "vbar_msg<l>",
 * "e_atom".  Layouts: s [N][F], v [N][3][F], phi [N][3F]. */
int vssr_debug_read(vssr_handle *h, const char *name, int32_t model, float *dst, int64_t cap,
                    int64_t *n_out);

/* ---- EAM (Cu(100) toy config, BASELINE configs[0]) ------------------------------------------------------ */
/* One-element funcfl tables of LAMMPS `pair_style eam` (reference: LAMMPSRunSurfCalc + mcmc/potentials/Cu_u3.eam,
 * mcmc/calculators/calculators.py:755-811, tests/test_Cu.py:41): frho[nrho] embedding energy F(rho) in eV on the grid
 * rho = k drho; zr[nr] effective charge Z(r) and rhor[nr] density rho(r) on r = k dr; pair term
 * phi(r) = 27.2 * 0.529 * Z(r)^2 / r.  Evaluate with vssr_tersoff_eval_batch / vssr_eam_eval_batch (all types 0). */
typedef struct {
    int32_t nrho, nr;
    double drho, dr, cutoff;
} vssr_eam_grid;
int vssr_eam_create(int32_t device, const vssr_eam_grid *grid, const double *frho, const double *zr, const double *rhor,
                    vssr_handle **out);
/* Several elements (LAMMPS pair_style eam/alloy, eam/fs, or funcfl files mixed per type, brought to one common grid by the
 * caller): n_elem in 1 .. 8 tables on one grid.  frho [n_elem][nrho] embedding energies F_t(rho); rhor [n_elem][nr] (fs = 0:
 * the density an atom of type t contributes) or [n_elem][n_elem][nr] (fs != 0: entry [a][b] = the density an atom of type a
 * contributes at a site of type b); z2r [n_elem (n_elem + 1) / 2][nr] r * phi in eV A of the pairs (0,0), (1,0), (1,1), (2,0), ...
 * (setfl order).  Cutoff: grid->cutoff.  Same splines, linear continuation of F and pe/atom split as vssr_eam_create; evaluate
 * with vssr_eam_eval_batch, type[i] = the atom's table index (VSSR_E_BADARG outside [0, n_elem)).  The input is checked before
 * any device is touched: VSSR_E_BADARG for a bad grid, n_elem outside 1 .. 8 or a non-finite table entry. */
int vssr_eam_create_alloy(int32_t device, int32_t n_elem, int32_t fs, const vssr_eam_grid *grid, const double *frho,
                          const double *rhor, const double *z2r, vssr_handle **out);
/* Angular-dependent potential (LAMMPS pair_style adp; Mishin, Mehl, Papaconstantopoulos 2005): the eam/alloy tables of
 * vssr_eam_create_alloy (fs = 0) plus a dipole function u and a quadrupole function w per element pair, [n_elem (n_elem + 1) / 2][nr]
 * each in the pair order of z2r, on the r grid, NOT scaled by r:
 *   E = sum_i [F(rho_i) + 1/2 mu_i.mu_i + 1/2 lambda_i:lambda_i - (tr lambda_i)^2 / 6] + 1/2 sum_{i != j} phi(r_ij),
 *   mu_i = sum_j u(r_ij) r_ij,  lambda_i = sum_j w(r_ij) r_ij (x) r_ij;  pe/atom of i = the bracket + half of its pair energies.
 * Same splines for u and w as for the other tables.  VSSR_E_BADARG, before any device is touched: null u or w, a non-finite
 * entry, and everything vssr_eam_create_alloy refuses.  Evaluate with vssr_eam_eval_batch; every vssr_batch_* entry point serves
 * the handle as it serves an eam/alloy one (stress, FIRE, BFGS, BFGSLineSearch, CG), except that a CG relaxation always runs in
 * lock step (VSSR_CG_DRIVER_RESIDENT is accepted, last_used reports VSSR_CG_DRIVER_LOCKSTEP). */
int vssr_eam_create_adp(int32_t device, int32_t n_elem, const vssr_eam_grid *grid, const double *frho, const double *rhor,
                        const double *z2r, const double *u, const double *w, vssr_handle **out);
/* same signature and meaning as vssr_tersoff_eval_batch (fp64 energies / per-atom energies / forces) */
int vssr_eam_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                        const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                        double *energy_atoms_f64, double *forces_f64);

/* ---- Tersoff (GaN config) ---------------------------------------------------------------- */
/* params: n_types^3 entries ordered [i][j][k], 14 doubles each, LAMMPS column order
 * (m gamma lambda3 c d costheta0 n beta lambda2 B R D lambda1 A). */
int vssr_tersoff_create(int32_t device, int32_t n_types, const double *params, vssr_handle **out);
/* The same from the text of a LAMMPS tersoff potential file and the species in LAMMPS type order -- what the reference
 * passes to LAMMPS as `pair_coeff * * <file> Ga N` (mcmc/calculators/calculators.py:559-568).
 * Entries `e1 e2 e3 m gamma lambda3 c d costheta0 n beta lambda2 B R D lambda1 A` may span lines, `#` starts a comment;
 * every triplet of the given species must be present. */
int vssr_tersoff_create_from_text(int32_t device, const char *param_text, int32_t n_species, const char *const *species,
                                  vssr_handle **out);
/* type[i] in [0,n_types).  Fills out->energy (total, eV), out->energy_atoms (WANT_PER_ATOM),
 * out->forces (WANT_FORCES).  fp64 arithmetic on the device; results narrowed to fp32 in
 * vssr_out, and returned exactly through the optional double arrays. */
int vssr_tersoff_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms,
                            const int32_t *type, const double *pos, const double *cell,
                            const uint8_t *pbc, uint32_t want, vssr_out *out,
                            double *energy_f64 /*[B] or NULL*/, double *energy_atoms_f64,
                            double *forces_f64);

/* ---- Stillinger-Weber (pair_style sw; the Si(111) 5x5 config's KIM model SW_StillingerWeber_1985_Si__MO_405512056662_005) --- */
/* params: n_types^3 entries ordered [i][j][k], 11 doubles each, LAMMPS column order
 * (eps sig a lambda gamma costheta0 A B p q tol); tol is read and has no effect.  Refused with VSSR_E_BADARG: non-finite numbers,
 * eps / sig / a <= 0, negative lambda / gamma / A / B / p / q / tol, and entries (i,j,k), (i,k,j) that differ in eps, lambda or
 * costheta0 (LAMMPS' energy would then depend on the order of its neighbor list).  Cutoff: the largest a * sig.
 * pe/atom as LAMMPS: pair terms half / half, three-body terms in thirds between the three atoms. */
int vssr_sw_create(int32_t device, int32_t n_types, const double *params, vssr_handle **out);
/* The same from the text of a LAMMPS .sw file and the species in LAMMPS type order: entries
 * `e1 e2 e3 eps sig a lambda gamma costheta0 A B p q tol` may span lines, `#` starts a comment; every triplet of the given species
 * must be present.  The input is checked before any device is touched. */
int vssr_sw_create_from_text(int32_t device, const char *param_text, int32_t n_species, const char *const *species,
                             vssr_handle **out);
/* same signature and meaning as vssr_tersoff_eval_batch (fp64 energies / per-atom energies / forces) */
int vssr_sw_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                       const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                       double *energy_atoms_f64, double *forces_f64);

/* ---- Vashishta (pair_style vashishta: SiC, SiO2, InP, GaAs, Al2O3) ------------------------------------------------------------ */
/* Handle kind 9.  LAMMPS units metal, qqr2e = 14.399645, fp64 throughout.  params: n_types^3 entries ordered [i][j][k] (i = centre),
 * 14 doubles each, LAMMPS column order (H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta):
 *   V(r)    = H / r^eta + qqr2e Zi Zj / r exp(-r / lambda1) - D / r^4 exp(-r / lambda4) - W / r^6
 *   phi2(r) = V(r) - V(rc) - (r - rc) V'(rc)                        r < rc, entry (i, j, j): energy and force vanish at rc
 *   phi3    = B f_ij(r_ij) f_ik(r_ik) dc^2 / (1 + C dc^2),  dc = cos theta_jik - costheta        B, C, costheta: entry (i, j, k)
 *   f_ij(r) = exp(gamma / (r - r0)) for r < r0, else 0              gamma, r0: entry (i, j, j)
 * E = sum over pairs phi2 + sum over centres i and unordered neighbor pairs {j, k} phi3; every directed slot i -> j carries half of
 * phi2 with entry (i, j, j).  pe/atom as LAMMPS: pair terms half / half, three-body terms in thirds between the three atoms.
 * Refused with VSSR_E_BADARG, by entry and field, before any device is touched: non-finite numbers and negative B / gamma / r0 in
 * any entry; in the entries (i, j, j), whose two-body and radial columns are the ones read: rc <= 0, eta <= 0, lambda1 <= 0 with
 * Zi Zj != 0, lambda4 <= 0 with D != 0, r0 > rc; entries (i, j, j), (j, i, i) that differ in H, eta, Zi Zj, lambda1, D, lambda4, W or rc
 * and entries (i, j, k), (i, k, j) that differ in B, C or costheta (LAMMPS' energy would then depend on the order of its neighbor
 * list); n_types outside 1 .. 8.  gamma and r0 of (i, j, j) and (j, i, i) may differ.  The two-body columns of an entry with j != k are
 * read by nobody and only have to be finite (published files write zeros there).  Cutoff of the neighbor list: the largest rc.
 * Relaxations: FIRE, BFGS, BFGSLineSearch and the lock-step CG serve these handles; the chain-resident CG minimiser does not
 * (VSSR_CG_DRIVER_RESIDENT runs in lock step, same results, as for ADP and k-space handles). */
int vssr_vashishta_create(int32_t device, int32_t n_types, const double *params, vssr_handle **out);
/* The same from the text of a LAMMPS .vashishta file and the species in LAMMPS type order: entries
 * `e1 e2 e3 H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta` may span lines, `#` starts a comment; every triplet of the
 * given species must be present, entries of other elements are skipped.  The input is checked before any device is touched. */
int vssr_vashishta_create_from_text(int32_t device, const char *param_text, int32_t n_species, const char *const *species,
                                    vssr_handle **out);
/* same signature and meaning as vssr_tersoff_eval_batch (fp64 energies / per-atom energies / forces) */
int vssr_vashishta_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                              const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                              double *energy_atoms_f64, double *forces_f64);

/* ---- Pair potentials with damped-shifted-force Coulomb (pair_style lj/cut, morse, buck, born, coul/dsf; hybrid and
 * hybrid/overlay of these) ------------------------------------------------------------------------------------------------------- */
/* LAMMPS units metal: eV, A, charges in e, qqrd2e = 14.399645.  E(r) for r < rc, coefficients in LAMMPS order:
 *   VSSR_PAIR_LJ_CUT    4 eps [(sig/r)^12 - (sig/r)^6]                         c = eps sig
 *   VSSR_PAIR_MORSE     D0 [exp(-2 alpha (r - r0)) - 2 exp(-alpha (r - r0))]   c = D0 alpha r0
 *   VSSR_PAIR_BUCK      A exp(-r/rho) - C/r^6                                  c = A rho C
 *   VSSR_PAIR_BORN      A exp((sig - r)/rho) - C/r^6 + D/r^8                   c = A rho sig C D
 *   VSSR_PAIR_COUL_DSF  qqrd2e q_a q_b [erfc(alpha r)/r - erfc(alpha rc)/rc + B (r - rc)]      c = alpha
 *                       B = erfc(alpha rc)/rc^2 + 2 alpha/sqrt(pi) exp(-alpha^2 rc^2)/rc  (energy and force vanish at rc)
 * shift != 0 (pair_modify shift yes) subtracts E(rc) from the four non-Coulomb styles; coul/dsf ignores it.  Every atom whose type
 * has a coul/dsf term gets the self energy -(erfc(alpha rc)/(2 rc) + alpha/sqrt(pi)) qqrd2e q_i^2 in its pe/atom; pair energies
 * are split half / half. */
enum { VSSR_PAIR_NONE = 0, VSSR_PAIR_LJ_CUT = 1, VSSR_PAIR_MORSE = 2, VSSR_PAIR_BUCK = 3, VSSR_PAIR_BORN = 4, VSSR_PAIR_COUL_DSF = 5,
       VSSR_PAIR_COUL_LONG = 6 /* qqrd2e q_a q_b erfc(g r)/r, the real-space part of an Ewald sum: vssr_pair_create_kspace only */ };
typedef struct vssr_pair_term {
    int32_t type_a, type_b, style;
    double c[5], rc;
    int32_t shift;
} vssr_pair_term;
/* Handle kind 8.  terms: n_terms entries; a term on (a, b) serves (b, a) as well (give each unordered pair's term once), and the
 * terms of a pair add up.  charge: [n_types] per-type charges, or NULL.  Refused with VSSR_E_BADARG before any device is touched:
 * n_types outside 1 .. 8, a type outside [0, n_types), an unknown style, more than 3 terms on a pair, a non-finite coefficient,
 * rc <= 0, lj/cut sig <= 0, buck / born rho <= 0, coul/dsf alpha < 0, coul/dsf without charges or with a non-finite charge, and
 * coul/dsf terms that differ in alpha or rc (the self energy of a type would not be defined).  Cutoff of the neighbor list: the
 * largest rc.  vssr_batch_upload refuses with VSSR_E_CAPACITY a periodic cell so thin for that cutoff that an axis would need more
 * than 100 images on either side (the neighbor search's limit); nothing is truncated. */
int vssr_pair_create(int32_t device, int32_t n_types, int32_t n_terms, const vssr_pair_term *terms, const double *charge,
                     vssr_handle **out);
/* A pair handle whose Coulomb term is an Ewald sum (LAMMPS pair_style coul/long, buck/coul/long, born/coul/long, lj/cut/coul/long
 * with kspace_style ewald): the terms of vssr_pair_create plus VSSR_PAIR_COUL_LONG terms (c is ignored: the damping is ks->g_ewald;
 * rc is the real-space cutoff) and the k-space parameters.  For a chain with cell volume V, charges q_i and total charge Q:
 *   E = E_real + E_k + E_self + E_bg
 *   E_real = sum over pairs with r < rc of qqrd2e q_a q_b erfc(g r) / r                        (no shift, as LAMMPS coul/long)
 *   E_k    = sum over k != 0, |k| <= k_cut of u(k) |S(k)|^2,  u(k) = qqrd2e (2 pi / V) exp(-k^2 / 4 g^2) / k^2,
 *            S(k) = sum_j q_j exp(i k.r_j),  k = h b1 + k b2 + l b3 over the reciprocal vectors of the chain's own cell
 *   E_self = -qqrd2e g / sqrt(pi) sum q_i^2,   E_bg = -qqrd2e pi Q^2 / (2 g^2 V)  (neutralising background: charged cells are served)
 * pe/atom as LAMMPS ewald: q_i sum_k u(k) Re(exp(-i k.r_i) S(k)) - qqrd2e g q_i^2 / sqrt(pi) - qqrd2e pi q_i Q / (2 g^2 V) on top of
 * the half / half pair split.  The k set is a function of (g_ewald, k_cut) and the chain's cell only (a sphere in reciprocal space,
 * any cell shape) -- not LAMMPS' accuracy estimator, which depends on the atom count and the charges; energies agree with LAMMPS to
 * the accuracy asked for, not digit for digit.  vssr_batch_stress adds the reciprocal and background virials.
 * Refused with VSSR_E_BADARG before any device is touched, besides what vssr_pair_create refuses: ks NULL, charge NULL, g_ewald or
 * k_cut not finite and positive, VSSR_PAIR_COUL_LONG terms that do not cover every type pair or that differ in rc, and a
 * VSSR_PAIR_COUL_LONG term next to a VSSR_PAIR_COUL_DSF term.  vssr_pair_create itself refuses a VSSR_PAIR_COUL_LONG term.
 * vssr_batch_upload refuses a chain with a non-periodic axis (VSSR_E_BADARG: a 3-D Ewald sum needs three periodic axes; slabs are
 * served by vssr_pair_create_kspace_slab below) and, with VSSR_E_CAPACITY, a chain whose k sphere needs a per-axis index floor(k_cut |a_i| / 2 pi) above 63 or a half
 * box (m1 + 1)(2 m2 + 1)(2 m3 + 1) of more than 65 536 cells; nothing is ever truncated.
 * Relaxations: FIRE, BFGS, BFGSLineSearch and the lock-step CG serve these handles; the chain-resident CG minimiser does not
 * (VSSR_CG_DRIVER_RESIDENT runs in lock step, same results, as for chains of more than 256 atoms).  Entry points that hand out
 * per-slot gradients (the gradient buffers of vssr_debug_read) carry the real-space part only. */
typedef struct vssr_kspace {
    double g_ewald, k_cut;   /* 1 / A */
} vssr_kspace;
int vssr_pair_create_kspace(int32_t device, int32_t n_types, int32_t n_terms, const vssr_pair_term *terms, const double *charge,
                            const vssr_kspace *ks, vssr_handle **out);
/* The same handle for slabs: LAMMPS kspace_style ewald + kspace_modify slab F under boundary p p f (Yeh & Berkowitz 1999; Ballenegger,
 * Arnold & Cerda 2009 for cells with net charge; restated from the papers, no LAMMPS was executed).  Chains have pbc 1 1 0, cell rows
 * a, b in the xy plane and c along z.  With the extended cell (a, b, F c) of volume V' = F V:
 *   E_real   over the in-plane images only (the neighbor list of pbc 1 1 0)
 *   E_k, E_self, E_bg and their pe/atom and forces: the formulas above in the extended cell (V' for V, its reciprocal vectors; the
 *            capacity limits below are taken on it too)
 *   E_slab = qqrd2e (2 pi / V') (M^2 - Q R2 - Q^2 L'^2 / 12),   Q = sum q, M = sum q z, R2 = sum q z^2, z_i = r_i . n (never wrapped),
 *            n = a x b / |a x b|, L' = F |c . n|
 *   e_i   += qqrd2e (2 pi / V') q_i (z_i M - (R2 + Q z_i^2) / 2 - Q L'^2 / 12)              (sums to E_slab)
 *   F_i   += -qqrd2e (4 pi / V') q_i (M - Q z_i) n
 * E_slab does not change under a common shift along z, for Q != 0 either.  vssr_batch_stress includes the slab virial
 * dE_slab / d eps = E_slab (-1, -1, +1, 0, 0, 0) (Voigt xx yy zz yz xz xy) and divides by the real V = |det cell|, not by V'.
 * Q, M and R2 are summed in atom order without atomics: a chain's bits depend neither on its batch nor on the run.
 * Refused with VSSR_E_BADARG at creation: what vssr_pair_create_kspace refuses, and a slab_factor that is not finite or is <= 1.0.
 * vssr_batch_upload on such a handle refuses with VSSR_E_BADARG a chain whose pbc is not exactly 1 1 0 (the message names the pbc), a
 * cell whose a or b has a z component or whose c has an x or y component beyond 1e-12 |c| (in-plane skew of a and b is fine), and a
 * chain whose atoms span more than |c| along z (the vacuum of the extended cell is then not guaranteed; positions that a relaxation
 * or an MD run moves later are NOT re-checked); with VSSR_E_CAPACITY a chain whose extended cell exceeds the limits above (the
 * message names the extended length F |c|).  vssr_pair_create_kspace handles keep their refusal of a non-periodic axis. */
int vssr_pair_create_kspace_slab(int32_t device, int32_t n_types, int32_t n_terms, const vssr_pair_term *terms, const double *charge,
                                 const vssr_kspace *ks, double slab_factor, vssr_handle **out);
/* same signature and meaning as vssr_tersoff_eval_batch (fp64 energies / per-atom energies / forces) */
int vssr_pair_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                         const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                         double *energy_atoms_f64, double *forces_f64);

/* ---- Gaussian-mixture uncertainty of PaiNN latent embeddings (reference mcmc.uncertainty.GMMUncertainty,
 *      mcmc/uncertainty/uncertainty.py:238-463; scripts/clustering.py --clustering_metric gmm) ---------------------------------- */
/* For a row x (fp64), component k with mean mu_k, precision Cholesky factor P_k ([D][D]) and weight w_k:
 *   s_k(x)  = sum_j ((x P_k)_j - (mu_k P_k)_j)^2
 *   logp_k  = -0.5 (D log_2pi + s_k) + sum_d log P_k[d][d]
 *   NLL(x)  = -(m + log sum_k exp(logp_k + log w_k - m)),  m = max_k (logp_k + log w_k)
 * All arithmetic is fp64 (v_mfma_f64_16x16x4_f64 for x P_k).  log_2pi is an input: GMMUncertainty evaluates it in float32
 * (1.8378770351409912), sklearn / gmm.py in fp64 (1.8378770664093453).  Covariance types other than "full" are expanded to
 * per-component full P_k by the caller. */
typedef struct {
    uint32_t struct_size; /* sizeof(vssr_gmm_config) */
    int32_t device;       /* HIP device ordinal */
    int32_t n_components; /* K, 1 .. 256 */
    int32_t dim;          /* D, 1 .. 256 */
    const double *means;     /* [K][D] */
    const double *prec_chol; /* [K][D][D], row-major: P_k[i][j] multiplies x_i into column j */
    const double *weights;   /* [K] */
    double log_2pi;
} vssr_gmm_config;
/* Handle kind 5 (freed by vssr_destroy).  Refused with VSSR_E_BADARG before any device is touched: K or D out of range, null
 * arrays, non-finite numbers, a non-positive diagonal entry of any P_k, a negative weight or no positive one.  The 16 x 16 blocks of
 * every P_k that are exactly zero are found here and skipped by the kernel (they add exactly 0: sklearn's factors are triangular).
 * Every entry point other than vssr_gmm_*, vssr_destroy and vssr_last_error refuses a GMM handle. */
int vssr_gmm_create(const vssr_gmm_config *cfg, vssr_handle **out);
/* Score n_rows caller rows x [n_rows][D] (fp64): nll [n_rows]; log_prob [n_rows][K] (logp_k, unweighted) may be NULL. */
int vssr_gmm_score_rows(vssr_handle *g, int64_t n_rows, const double *x, double *nll, double *log_prob);
/* Score the resident embedding of a PaiNN handle (the features vssr_batch_embedding returns) of ensemble member `model`, read in
 * place on the device.  rows: 0 = every atom (nll_rows [sum N]), 1 = one mean row per structure (nll_rows [B], summed in fp64 in
 * atom order).  order: 0 atomic, 1 system_sum, 2 system_mean, 3 system_max, 4 system_min, 5 system_mean_squared,
 * 6 system_root_mean_squared; for order >= 1, system [B] receives the true per-structure reduction of the row NLLs (rows = 1: the
 * structure's own NLL).  Deterministic: one workgroup reduces one structure in a fixed order.  Either output may be NULL.
 * Runs on the PaiNN handle's stream and synchronises.  VSSR_E_STATE as vssr_batch_embedding (no PaiNN run, or a partial graph
 * after a relaxation); VSSR_E_BADARG when D != feat_dim or the handles live on different devices. */
int vssr_gmm_score_batch(vssr_handle *g, vssr_handle *painn, int32_t model, int32_t rows, int32_t order, double *nll_rows,
                         double *system);

/* ---- Fitting the Gaussian mixture on the device (fp64 EM; reference mcmc.uncertainty.gmm.GaussianMixture, a copy of sklearn's with a
 *      blocked matrix product; GMMUncertainty.fit_gmm, mcmc/uncertainty/uncertainty.py:295-315) ------------------------------------ */
/* Rows x_n [D] (fp64, resident on the device as [N][Dp], Dp = 16 ceil(D / 16), zero pad columns).  One EM iteration:
 *   E:  logp_nk and NLL_n as vssr_gmm_score_rows with the fp64 constant log 2 pi;  r_nk = exp(logp_nk + log w_k + NLL_n);
 *       lower bound = mean_n(-NLL_n), reduced in a fixed order (per-workgroup partials, then one tree)
 *   M:  n_k = sum_n r_nk + 10 eps;  mu_k = sum_n r_nk x_n / n_k;  w_k = n_k / sum_k n_k
 *       full:       S_k = sum_n r_nk (x_n - mu_k)(x_n - mu_k)^T / n_k + reg_covar I   (centred form, v_mfma_f64_16x16x4_f64, row slabs
 *                   summed in slab order)
 *       tied:       S = (X^T X - sum_k n_k mu_k mu_k^T) / sum_k n_k + reg_covar I
 *       diag:       s_kd = sum_n r_nk x_nd^2 / n_k - 2 mu_kd mu_kd + mu_kd^2 + reg_covar;   spherical: mean_d s_kd
 *       P_k = (chol(S_k)^-1)^T (diag / spherical: 1 / sqrt(s)), log det P_k, c_k = mu_k P_k, written into the scoring layout
 *   stop when |lower bound - previous| < tol, or after max_iter iterations; n_init restarts keep the best final lower bound.
 * No floating-point atomics: two runs of the same fit on the same rows give the same bits. */
enum { VSSR_GMM_COV_FULL = 0, VSSR_GMM_COV_TIED = 1, VSSR_GMM_COV_DIAG = 2, VSSR_GMM_COV_SPHERICAL = 3 };
/* GIVEN: the start comes from vssr_gmm_fit_set_init (all of means / weights / precisions, or labels, or both: explicit values win as in
 * sklearn's _initialize).  KMEANS: Lloyd iterations on the device from K distinct rows drawn with Philox4x32-10 keyed by `seed`;
 * RANDOM_FROM_DATA: K distinct rows drawn the same way get responsibility 1 for one component each.  The draws do not reproduce numpy's
 * streams.  Explicit values from set_init override what either produces.
 * KMEANS in full: the first centre is row min(N - 1, floor(u N)); every later one is drawn by D^2 sampling over the running minimum
 * squared distances (one candidate per centre; the cumulative walk runs over the sums of 256-row blocks, then inside the block, and
 * passes over a row at distance zero while another is left).  Lloyd rounds assign every row to its nearest centre (the first on ties)
 * and move each centre to the mean of its members, until the inertia repeats or for 300 rounds.  A cluster that ends without members is
 * not relocated: its sum is divided by 10 eps like any other, so its centre is the origin, and its component starts with n_k = 10 eps
 * (weight 10 eps / N), mean 0 and covariance reg_covar I (an ill-defined covariance when reg_covar = 0). */
enum { VSSR_GMM_INIT_GIVEN = 0, VSSR_GMM_INIT_KMEANS = 1, VSSR_GMM_INIT_RANDOM_FROM_DATA = 2 };
typedef struct {
    uint32_t struct_size;    /* sizeof(vssr_gmm_fit_config) */
    int32_t device;          /* HIP device ordinal; the device is first touched by the first append / run */
    int32_t n_components;    /* K, 1 .. 256 */
    int32_t dim;             /* D, 1 .. 256 */
    int32_t covariance_type; /* VSSR_GMM_COV_* */
    int32_t max_iter;        /* >= 1 */
    int32_t n_init;          /* >= 1 */
    int32_t init;            /* VSSR_GMM_INIT_* */
    double tol;              /* >= 0 */
    double reg_covar;        /* >= 0 */
    uint64_t seed;
} vssr_gmm_fit_config;
typedef struct {
    int32_t n_iter;          /* iterations of the best restart */
    int32_t converged;       /* 1 = that restart stopped on tol */
    int32_t best_init;       /* index of the best restart */
    int32_t n_lower_bounds;  /* entries written to lower_bounds (min(n_iter, lower_bounds_cap)) */
    double lower_bound;      /* lower bound of the last iteration of the best restart */
    double *lower_bounds;    /* caller buffer [lower_bounds_cap] for that restart's trace; may be NULL */
    int32_t lower_bounds_cap;
} vssr_gmm_fit_result;
/* Handle kind 6 (freed by vssr_destroy); every entry point other than vssr_gmm_fit_*, vssr_destroy and vssr_last_error refuses it.
 * Refused with VSSR_E_BADARG without touching a device: K or D outside 1 .. 256, an unknown covariance type or init, tol < 0,
 * reg_covar < 0, max_iter < 1, n_init < 1, non-finite tol / reg_covar. */
int vssr_gmm_fit_create(const vssr_gmm_fit_config *cfg, vssr_handle **out);
/* Append caller rows x [n_rows][D] (fp64) to the resident set.  VSSR_E_BADARG (before a device is touched) for a null pointer,
 * n_rows < 1 or a non-finite entry; VSSR_E_DEVICE when no device is available. */
int vssr_gmm_fit_append_rows(vssr_handle *h, int64_t n_rows, const double *x);
/* Append the resident embedding of a PaiNN handle's last run (ensemble member `model`), device to device, widened to fp64.
 * rows: 0 = one row per atom, 1 = one mean row per structure.  Errors as vssr_gmm_score_batch: VSSR_E_STATE without a completed run
 * (or with a partial graph), VSSR_E_BADARG when D != feat_dim, the devices differ, or a row is not finite. */
int vssr_gmm_fit_append_batch(vssr_handle *h, vssr_handle *painn, int32_t model, int32_t rows);
/* Drop the resident rows and the labels given to set_init (explicit parameters are kept). */
int vssr_gmm_fit_clear(vssr_handle *h);
/* Starting values; every pointer may be NULL (= not given; a call replaces all four).  means [K][D]; weights [K] (finite, >= 0, one positive; that
 * they sum to 1 is the caller's check); precisions in sklearn's shape for the
 * covariance type (full [K][D][D], tied [D][D], diag [K][D], spherical [K]) -- PRECISION matrices, factorised here with a lower
 * Cholesky as gmm.py:657-664 does; labels [N] in -1 .. K-1 for the N rows resident at the time of the call (one-hot
 * responsibilities, -1 = no component; what sklearn does with its k-means result).  VSSR_E_BADARG for non-finite values, a precision
 * that is not positive definite, or a label out of range. */
int vssr_gmm_fit_set_init(vssr_handle *h, const double *means, const double *weights, const double *precisions,
                          const int32_t *labels);
/* Run the fit (sklearn's BaseMixture.fit loop).  VSSR_E_BADARG (no device touched) when N < 2, K > N, or the start is
 * incomplete (INIT_GIVEN without labels and without all three parameter arrays; labels of another length).  VSSR_E_STATE with the
 * reference's "ill-defined empirical covariance" text when a covariance has a non-positive pivot (flag set by the kernel, no device
 * assert).  One 8-byte read-back per iteration. */
int vssr_gmm_fit_run(vssr_handle *h, vssr_gmm_fit_result *res);
/* Fitted parameters in sklearn's shapes for the handle's covariance type: weights [K], means [K][D], covariances and prec_chol
 * (full [K][D][D], tied [D][D], diag [K][D], spherical [K]).  Any may be NULL.  VSSR_E_STATE before a successful run. */
int vssr_gmm_fit_params(vssr_handle *h, double *weights, double *means, double *covariances, double *prec_chol);
/* A scoring handle (kind 5) of the fitted mixture on the same device, built from the device arrays (no host copy); log_2pi as in
 * vssr_gmm_config.  VSSR_E_STATE before a successful run. */
int vssr_gmm_fit_scorer(vssr_handle *h, double log_2pi, vssr_handle **gmm);

/* ---- Clustering latent embeddings on the device (reference mcmc/utils/clustering.py: perform_clustering :21-85,
 *      get_cluster_centers :160-188; scripts/clustering.py) ------------------------------------------------------------------------- */
/* Rows x_n [D] (fp64, resident as [N][Dp] like the rows of the mixture fit).  All arithmetic fp64, fixed summation orders, no
 * floating-point atomics: two runs on the same rows give the same bits.
 *   PCA (clustering.py:50-51, sklearn PCA(n_components, whiten).fit(X).transform(X)):  mean_ = column means;  C = sum_n (x_n - mean)
 *       (x_n - mean)^T / (N - 1) on v_mfma_f64_16x16x4_f64 (the row-slab kernel of the mixture fit, unit responsibilities);  C = V diag(l)
 *       V^T by cyclic Jacobi rotations in one workgroup (round-robin ordering);  components_ = the n_components eigenvectors of the
 *       largest l, each with its largest-magnitude entry positive (the first one on ties; sklearn's svd_flip on V^T);
 *       explained_variance_ = l;  ratio = l / sum of all l;  X_r = (X - mean) components_^T, divided by sqrt(l) when whitening.
 *   Ward linkage (clustering.py:60, :174, scipy linkage(P, "ward")) of points P [N][cluster_dims] without a distance matrix: clusters are
 *       (centroid, size); d(A, B) = sqrt(2 |A| |B| / (|A| + |B|)) |c_A - c_B|.  Per round every live cluster finds its nearest live
 *       cluster (the lowest position in the live list wins a tie), all reciprocal pairs merge (centroid = size-weighted mean), the live
 *       list is compacted in order.  Ward is reducible, so the tree equals that of one global minimum at a time.  The N - 1 merge
 *       records are then sorted by height (stable) and renumbered to scipy's Z: row r creates cluster N + r, the smaller id first.
 * optimal_ordering=True of the reference (a reordering of children for the dendrogram plot) is not built. */
typedef struct {
    uint32_t struct_size;  /* sizeof(vssr_cluster_config) */
    int32_t device;        /* HIP device ordinal; the device is first touched by the first append / set_points */
    int32_t dim;           /* D, 1 .. 256 */
    int32_t n_components;  /* 1 .. D (and <= N when vssr_cluster_pca runs) */
    int32_t whiten;        /* 0 / 1 */
    int32_t cluster_dims;  /* 1 .. 32: leading columns of X_r that are clustered (the reference: 3), or the width of set_points */
} vssr_cluster_config;
typedef struct {
    int64_t n_rows;        /* rows the PCA was fitted on */
    int32_t n_sweeps;      /* Jacobi sweeps */
    int32_t converged;     /* 1 = every off-diagonal entry fell below eps |C|_F / D before the sweep limit */
} vssr_cluster_pca_result;
/* Handle kind 7 (freed by vssr_destroy); every entry point other than vssr_cluster_*, vssr_destroy and vssr_last_error refuses it, and
 * the vssr_cluster_* calls refuse every other kind.  Refused with VSSR_E_BADARG without touching a device: dim outside 1 .. 256,
 * n_components outside 1 .. dim, cluster_dims outside 1 .. 32, whiten other than 0 / 1, a negative device. */
int vssr_cluster_create(const vssr_cluster_config *cfg, vssr_handle **out);
/* Append caller rows x [n_rows][D] (fp64); several appends accumulate.  VSSR_E_BADARG (before a device is touched) for a null
 * pointer, n_rows < 1 or a non-finite entry. */
int vssr_cluster_append_rows(vssr_handle *h, int64_t n_rows, const double *x);
/* Append one mean row per structure of a PaiNN handle's last run (ensemble member `model`), device to device -- the reference's
 * get_embeddings_single(flatten=True, flatten_axis=0).  Errors as vssr_gmm_fit_append_batch. */
int vssr_cluster_append_batch(vssr_handle *h, vssr_handle *painn, int32_t model);
/* Drop the resident rows, the PCA and the points. */
int vssr_cluster_clear(vssr_handle *h);
/* Fit the PCA on the resident rows and project them; the first cluster_dims columns of X_r become the points of the linkage.
 * VSSR_E_BADARG (no device touched) when N < 2, n_components > N or cluster_dims > n_components.  result may be NULL. */
int vssr_cluster_pca(vssr_handle *h, vssr_cluster_pca_result *result);
/* mean_ [D], components_ [n_components][D], explained_variance_ and explained_variance_ratio_ [n_components]; any may be NULL.
 * VSSR_E_STATE before vssr_cluster_pca. */
int vssr_cluster_pca_params(vssr_handle *h, double *mean, double *components, double *explained_variance, double *ratio);
/* Rows first .. first + n_rows - 1 of X_r into xr [n_rows][n_components].  VSSR_E_STATE before vssr_cluster_pca, VSSR_E_BADARG for a
 * range outside the fitted rows. */
int vssr_cluster_projected(vssr_handle *h, int64_t first, int64_t n_rows, double *xr);
/* Skip the PCA: cluster caller points p [n][cluster_dims] (clustering.py:174, get_cluster_centers).  Replaces the resident points.
 * VSSR_E_BADARG (before a device is touched) for a null pointer, n < 2 or a non-finite entry. */
int vssr_cluster_set_points(vssr_handle *h, int64_t n, const double *p);
/* Ward linkage of the resident points: Z [N - 1][4] in scipy's convention (ids as doubles, height, size); n_rounds (may be NULL)
 * receives the rounds taken (at most N - 1: every round merges at least one pair, duplicated points included).  One 8-byte read-back
 * per round.  VSSR_E_STATE without points. */
int vssr_cluster_linkage(vssr_handle *h, double *Z, int32_t *n_rounds);

#ifdef __cplusplus
}
#endif
#endif /* VSSR_EVAL_H */
