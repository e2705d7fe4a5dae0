// md_dev.h — device side of molecular dynamics on the resident batch (md.hip): velocity Verlet (NVE) and Langevin BAOAB
// (Leimkuhler & Matthews, J. Chem. Phys. 138, 174102 (2013)), the per-chain state, the random numbers.  md_step_chain is the only place
// the integrator arithmetic lives; the numpy restatement is tests/md_oracle.py.
//
// UNITS.  A, eV, fs, amu, K; velocities in A / fs, friction in 1 / fs.  kB = 8.617333262e-5 eV / K.  An acceleration is
// (F / m) * MD_ACC with MD_ACC the value of 1 eV / amu in A^2 / fs^2, formed below from the CODATA 2018 values of e and amu; a kinetic
// energy is 0.5 * sum(m v^2) / MD_ACC.  Everything is fp64 (fp32 forces are widened on read) and the build keeps -ffp-contract=off.
//
// ONE CALL of md_step_chain stands right behind an evaluation (E, F) of the chain's current positions r:
//   1. a non-finite E or force component: r, v back to the last completed step, stop reason 2, chain switched off;
//   2. a step in flight is closed:           v += (dt / 2) (F / m) MD_ACC;  steps += 1
//   3. steps % thermo_interval == 0:         record steps / thermo_interval = (E, 0.5 sum m v^2 / MD_ACC)
//   4. steps == n_steps:                     stop reason 1, chain switched off
//   5. the next step n = step0 + steps is opened (r, v saved first):
//        NVE       v += (dt / 2) a;  r += dt v
//        Langevin  v += (dt / 2) a;  r += (dt / 2) v;  v = c1 v + sqrt(c2 kB T_n MD_ACC / m) xi;  r += (dt / 2) v
//      with a = (F / m) MD_ACC, c1 = exp(-friction dt), c2 = 1 - c1 c1 (both formed on the host), and
//      T_n = temperature + (temperature_end - temperature) * (n / ramp_steps) for n < ramp_steps, temperature_end from there on.
// Atoms under the FixAtoms mask keep v = 0, draw no noise and never move.  Nothing here depends on the host's iteration count: an
// evaluation repeated after a neighbor-capacity regrow finds the state it left.
//
// RANDOM NUMBERS.  Philox4x32-10 (the function of mc.philox4x32).  The step index and the chain id are 64-bit and the atom index 32-bit:
// together they do not fit the 128-bit counter, so the chain id goes into the key, in two stages:
//   chain key   (q0, q1) = words 0, 1 of Philox(counter = (chain_id & 0xFFFFFFFF, chain_id >> 32, 0x4D44, 0), key = (seed & 0xFFFFFFFF, seed >> 32))
//   draw        w[0..3]  = Philox(counter = (n & 0xFFFFFFFF, n >> 32, atom index within the chain, (tag << 8) | pair), key = (q0, q1))
// tag: MD_TAG_MAXWELL = 0 (the Maxwell-Boltzmann draw, n = 0), MD_TAG_LANGEVIN = 1.  One draw gives two 53-bit uniforms in (0, 1],
//   u1 = (((w0 << 21) | (w1 >> 11)) + 1) 2^-53,  u2 likewise from (w2, w3),
// and Box-Muller two standard normals z0 = R cospi(2 u2), z1 = R sinpi(2 u2), R = sqrt(-2 log u1) (log, sqrt, sincospi).  pair 0
// serves the x and y components of the atom, pair 1 the z component (its z1 is not used).
#ifndef VSSR_MD_DEV_H
#define VSSR_MD_DEV_H
#include "cg_dev.h"

namespace vssr {

constexpr double MD_KB = 8.617333262e-5;                                     // eV / K
constexpr double MD_ACC = 1.602176634e-19 / 1.66053906660e-27 * 1e-10;       // (eV / amu) in A^2 / fs^2
enum { MD_TAG_MAXWELL = 0, MD_TAG_LANGEVIN = 1 };
// stop reasons: 1 all n_steps taken, 2 non-finite energy or force (positions and velocities of the last completed step)

struct MdParams {
    int n_steps, thermostat, thermo_interval, B;   // B: chains of the batch (row stride of the thermo records)
    double dt, t0, t1, c1, c2;
    long long ramp_steps, step0;
    uint32_t seed_lo, seed_hi;
};
struct MdState {   // per chain
    int steps, reason, open, pad;   // open: a step is in flight (positions moved, the closing half kick is due)
};
struct MdView {
    MdState *st;
    double *vel;                 // [3 N], resident on the handle between calls
    double *r_prev, *v_prev;     // [3 N] each: the state the step in flight opened at
    const double *mass;          // [N] amu
    const unsigned long long *chain_id;   // [B]
    double *thermo;              // [n_steps / thermo_interval + 1][B][2]
};

__device__ __forceinline__ void md_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
__device__ __forceinline__ void md_chain_key(uint32_t seed_lo, uint32_t seed_hi, unsigned long long chain, uint32_t &q0, uint32_t &q1) {
    uint32_t w[4];
    md_philox((uint32_t)chain, (uint32_t)(chain >> 32), 0x4D44u, 0u, seed_lo, seed_hi, w);
    q0 = w[0]; q1 = w[1];
}
// two standard normals of draw (n, atom, tag, pair) under the chain key
__device__ __forceinline__ void md_normal2(uint32_t q0, uint32_t q1, long long n, int atom, int tag, int pair, double &z0, double &z1) {
    uint32_t w[4];
    md_philox((uint32_t)(unsigned long long)n, (uint32_t)((unsigned long long)n >> 32), (uint32_t)atom, ((uint32_t)tag << 8) | (uint32_t)pair, q0, q1, w);
    const double u1 = ((double)(((unsigned long long)w[0] << 21) | (w[1] >> 11)) + 1.0) * 0x1p-53;
    const double u2 = ((double)(((unsigned long long)w[2] << 21) | (w[3] >> 11)) + 1.0) * 0x1p-53;
    const double R = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    z0 = R * c; z1 = R * s;
}
__device__ __forceinline__ void md_normal3(uint32_t q0, uint32_t q1, long long n, int atom, int tag, double z[3]) {
    double unused;
    md_normal2(q0, q1, n, atom, tag, 0, z[0], z[1]);
    md_normal2(q0, q1, n, atom, tag, 1, z[2], unused);
}

// One call of chain b's integrator on the evaluation just made; every thread of the 256-thread workgroup calls it.  FT: double
// (d_pot_f) or float (PaiNN's d_forces, widened).  Every vector loop is strided by ATOM with the same stride, so a thread only ever
// reads elements it wrote itself; the scalars all threads branch on come from the loaded state and from block reductions, which hand
// every thread the same bits (bfgsls_dev.h).  red: >= 16 doubles of LDS.  stopped: [0] chains that stopped, [1] of those with reason 2.
template <class FT>
__device__ __forceinline__ void md_step_chain(int b, double *red, const int *__restrict__ cfg_start, const double *__restrict__ energy,
                                              const FT *__restrict__ forces, const uint8_t *__restrict__ fixed, const MdParams &P,
                                              double *__restrict__ pos, const MdView &V, unsigned char *__restrict__ active,
                                              int *__restrict__ stopped) {
    const int tid = threadIdx.x, nt = blockDim.x;
    MdState S = V.st[b];
    __syncthreads();   // every wave holds the state before thread 0 can store the advanced one (cg_dev.h)
    if (S.reason) return;
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0;
    double *x = pos + 3 * (size_t)a0, *v = V.vel + 3 * (size_t)a0, *xp = V.r_prev + 3 * (size_t)a0, *vp = V.v_prev + 3 * (size_t)a0;
    const double *m = V.mass + a0;
    const FT *fg = forces + 3 * (size_t)a0;
    const uint8_t *fx = fixed ? fixed + a0 : nullptr;

    // 1. finite?
    const double E = energy[b];
    double bad = isfinite(E) ? 0.0 : 1.0;
    for (int i = tid; i < nat; i += nt) {
        const double f0 = (double)fg[3 * i], f1 = (double)fg[3 * i + 1], f2 = (double)fg[3 * i + 2];
        if (!(isfinite(f0) && isfinite(f1) && isfinite(f2))) bad = 1.0;
    }
    bad = block_max(bad, red);
    if (bad != 0.0) {   // nothing sane to follow: back to the last completed step (an evaluation with no step in flight is there already)
        if (S.open)
            for (int i = tid; i < nat; i += nt)
                for (int c = 0; c < 3; ++c) { x[3 * i + c] = xp[3 * i + c]; v[3 * i + c] = vp[3 * i + c]; }
        if (tid == 0) {
            S.open = 0; S.reason = 2;
            V.st[b] = S; active[b] = 0;
            atomicAdd(stopped, 1); atomicAdd(stopped + 1, 1);
        }
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
    // 3. thermo record
    if (S.steps % P.thermo_interval == 0) {
        double k = 0.0;
        for (int i = tid; i < nat; i += nt) k += m[i] * (v[3 * i] * v[3 * i] + v[3 * i + 1] * v[3 * i + 1] + v[3 * i + 2] * v[3 * i + 2]);
        k = block_sum(k, red);
        if (tid == 0) {
            double *rec = V.thermo + 2 * ((size_t)(S.steps / P.thermo_interval) * P.B + b);
            rec[0] = E; rec[1] = 0.5 * k / MD_ACC;
        }
    }
    // 4. finished
    if (S.steps == P.n_steps) {
        if (tid == 0) { S.reason = 1; V.st[b] = S; active[b] = 0; atomicAdd(stopped, 1); }
        return;
    }
    // 5. open step n
    const long long n = P.step0 + S.steps;
    uint32_t q0 = 0, q1 = 0;
    double kT = 0.0;
    if (P.thermostat == VSSR_MD_LANGEVIN) {
        md_chain_key(P.seed_lo, P.seed_hi, V.chain_id[b], q0, q1);
        const double T = n < P.ramp_steps ? P.t0 + (P.t1 - P.t0) * ((double)n / (double)P.ramp_steps) : P.t1;
        kT = MD_KB * T;
    }
    for (int i = tid; i < nat; i += nt) {
        for (int c = 0; c < 3; ++c) { xp[3 * i + c] = x[3 * i + c]; vp[3 * i + c] = v[3 * i + c]; }
        if (fx && fx[i]) continue;
        if (P.thermostat == VSSR_MD_LANGEVIN) {
            double z[3];
            md_normal3(q0, q1, n, i, MD_TAG_LANGEVIN, z);
            const double sigma = sqrt(P.c2 * kT * MD_ACC / m[i]);
            for (int c = 0; c < 3; ++c) {
                double vv = v[3 * i + c] + hdt * (((double)fg[3 * i + c] / m[i]) * MD_ACC);
                double xx = x[3 * i + c] + hdt * vv;
                vv = P.c1 * vv + sigma * z[c];
                xx += hdt * vv;
                v[3 * i + c] = vv; x[3 * i + c] = xx;
            }
        } else {
            for (int c = 0; c < 3; ++c) {
                const double vv = v[3 * i + c] + hdt * (((double)fg[3 * i + c] / m[i]) * MD_ACC);
                v[3 * i + c] = vv;
                x[3 * i + c] += P.dt * vv;
            }
        }
    }
    if (tid == 0) { S.open = 1; V.st[b] = S; }
}

// ---- host side, shared by the two drivers (md.hip; the chain-resident one is in chain_min.hip) ------------------------------
// The integrator's workspace: state and the pre-step copies on the handle's optimizer buffers (as FireWork / BfgsWork / CgWork), the
// masses behind them; the stop counters, chain ids and thermo records in d_md_aux; the velocities in d_md_vel, which no relaxation
// touches.
struct MdWork {
    MdView V;
    MdParams P;
    const uint8_t *fixed;   // the mask on the device (null: all free)
    int *stopped;           // [2]: chains that stopped, of those with reason 2
    int nrec;
};
// driver_open, the workspace, masses / chain ids / mask on the device, every chain at step 0 of this call, held atoms at v = 0
int md_begin(vssr_handle *h, const vssr_md_params *p, const double *mass, const uint8_t *fixed_host, const uint64_t *chain_id, uint32_t want,
             MdWork &W);
// d_relax_steps [B][2] = (steps completed, stop reason); the thermo records into thermo_out (may be null; stream-ordered copy)
int md_end(vssr_handle *h, const MdWork &W, double *thermo_out);
int md_lockstep(vssr_handle *h, const MdWork &W, uint32_t want);
// VSSR_E_BADARG (message under `func`) unless mass is [n_atoms] finite values > 0 (md.hip; md_npt.hip asks the same)
int md_masses_ok(vssr_handle *h, const char *func, const double *mass);
// chain_min.hip: the same integration with one workgroup per chain.  chain_md_supported: this call takes it (the kernel applies AND
// the handle's md_driver asks for it)
bool chain_md_supported(const vssr_handle *h);
int chain_md(vssr_handle *h, const MdWork &W);

}  // namespace vssr
#endif
