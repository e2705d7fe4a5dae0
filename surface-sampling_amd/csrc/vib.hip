// vib.hip — harmonic vibrations of the structures of the resident batch by finite differences, on every handle kind that evaluates:
// the Hessian rows of ASE's Vibrations.read (central or five-point differences of the forces, optional Frederiksen correction),
// H <- H + H^T, the modes of D H D with D = diag(mass^-1/2), zero-point energy and vibrational Helmholtz energy.  Restated from ASE as
// remembered; the contract is the numpy restatement tests/vib_oracle.py.
// A GROUP is one structure, resident as n_rep identical consecutive chains (replicas).  Its m = 3 (vib atoms) degrees of freedom are
// numbered by (vib atom in chain order, x / y / z); the replica of rank k works through the degrees of freedom r = k, k + n_rep, ...,
// so that one structure's displacements fill the batch.  The driver frame is lockstep.h's: one batch-wide evaluation per displacement,
// one k_vib_step launch behind it (one workgroup per chain; what a chain does next follows from its own state, so an evaluation
// repeated after a regrow writes no row twice and skips none).  A displaced coordinate is x0 + k delta in one fp64 operation from a saved
// copy of x0, and goes back by copying the saved value.  nfree (largest share of a replica) + 1 evaluations; the last is at x0 over
// all chains.  Rows of a group are written by different workgroups to disjoint rows: no atomics on results, the same bits every run.
// Then, per group: k_vib_sym (H + H^T and D H D), k_vib_eigh (the cyclic Jacobi of jacobi_dev.h, from LDS where two m x m matrices fit
// beside its own arrays: m <= 96), k_vib_modes (ascending order, energies, signed modes, thermochemistry).
// Forces are the raw forces: there is no FixAtoms mask here, a caller who wants ASE-with-FixAtoms behaviour leaves held atoms out of vib.
// Out of scope: a chain-resident driver, infrared intensities, more than 256 degrees of freedom per structure, projection of
// rotations / translations, live-chain compaction.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "arena.h"
#include "jacobi_dev.h"
#include "lockstep.h"
#include "md_dev.h"

namespace vssr {

constexpr int VIB_MAX_DOF = 256;   // rows the one-workgroup Jacobi takes
constexpr double VIB_HBAR = 1.054571817e-34;   // J s (CODATA 2018); e and amu as in md_dev.h

struct VibChain { int group, rank, nrep, m; };
struct VibState { int j, s, reason, pad; };   // j: degrees of freedom of this chain completed; s: displacement in place; reason 1 done, 2 non-finite
struct VibView {
    VibState *st;              // [B]
    const VibChain *ch;        // [B]
    const int *vib_start;      // [B + 1] into vib_list
    const int *vib_list;       // chain-local indices of the vib atoms, chain order
    double *x0;                // [3 N] the positions the call found
    double *Fs;                // [nfree][3 N] forces at the displacements of the degree of freedom in work
    double *K;                 // [G][ld][ld] rows before H + H^T
    int *gbad;                 // [G] 1: a replica of the group met a non-finite energy or force
    size_t n3;                 // 3 N
    int ld, nfree, method;
    double delta;
};

// the displacement s (0 .. nfree - 1) in units of delta: -1, +1 / -2, -1, +1, +2
__device__ __forceinline__ double vib_k(int nfree, int s) {
    return nfree == 2 ? (s == 0 ? -1.0 : 1.0) : (s == 0 ? -2.0 : s == 1 ? -1.0 : s == 2 ? 1.0 : 2.0);
}

// Replicas: chain b of rank > 0 against the first chain of its group, bit for bit (species, cell, pbc, positions; atom counts, masses
// and masks were compared on the host).  flag[0] = 1 on any difference.
__global__ void __launch_bounds__(256)
k_vib_compare(const VibChain *__restrict__ ch, const int *__restrict__ cfg_start, const int *__restrict__ Z,
              const unsigned long long *__restrict__ cell, const unsigned char *__restrict__ pbc,
              const unsigned long long *__restrict__ pos, int *__restrict__ flag) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const VibChain c = ch[b];
    if (c.rank == 0) return;
    const int f = b - c.rank;
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0, f0 = cfg_start[f];
    bool diff = false;
    for (int i = tid; i < nat; i += 256) diff |= Z[a0 + i] != Z[f0 + i];
    for (int t = tid; t < 3 * nat; t += 256) diff |= pos[3 * (size_t)a0 + t] != pos[3 * (size_t)f0 + t];
    if (tid < 9) diff |= cell[9 * (size_t)b + tid] != cell[9 * (size_t)f + tid];
    if (tid < 3) diff |= pbc[3 * b + tid] != pbc[3 * f + tid];
    if (diff) flag[0] = 1;   // (same value from every writer)
}

// x0 saved, every chain at its first displacement (rank < m) or finished at once (idle replica, empty mask)
__global__ void __launch_bounds__(256)
k_vib_place(const int *__restrict__ cfg_start, double *__restrict__ pos, VibView V, int *__restrict__ stopped) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0;
    double *x = pos + 3 * (size_t)a0, *x0 = V.x0 + 3 * (size_t)a0;
    for (int t = tid; t < 3 * nat; t += 256) x0[t] = x[t];
    __syncthreads();
    if (tid) return;
    const VibChain c = V.ch[b];
    VibState S = {0, 0, 0, 0};
    if (c.rank < c.m) {
        const int dof = 3 * V.vib_list[V.vib_start[b] + c.rank / 3] + c.rank % 3;
        x[dof] = x0[dof] + vib_k(V.nfree, 0) * V.delta;
    } else {
        S.reason = 1;
        atomicAdd(stopped, 1);
    }
    V.st[b] = S;
}

// Behind an evaluation of the batch: chain b reads the forces of its displacement in place, writes the Hessian row when the
// degree of freedom is complete, and places its next displacement (or goes back to x0 and stops).  FT: double (d_pot_f) or float
// (PaiNN's ensemble-mean forces, widened).
template <class FT>
__global__ void __launch_bounds__(256)
k_vib_step(const int *__restrict__ cfg_start, const int *__restrict__ counters, const double *__restrict__ energy,
           const FT *__restrict__ forces, double *__restrict__ pos, VibView V, int *__restrict__ stopped) {
    __shared__ double red[16];
    if (counters[2]) return;   // the evaluation overflowed the neighbor capacity: nothing moves, the host regrows and repeats it
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    VibState S = V.st[b];
    __syncthreads();   // every wave holds the state before thread 0 can store the advanced one (cg_dev.h)
    if (S.reason) return;
    const VibChain c = V.ch[b];
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0;
    double *x = pos + 3 * (size_t)a0;
    const double *x0 = V.x0 + 3 * (size_t)a0;
    const FT *fg = forces + 3 * (size_t)a0;
    const int *vl = V.vib_list + V.vib_start[b];
    const int r = c.rank + S.j * c.nrep;
    const int da = vl[r / 3], dof = 3 * da + r % 3;

    double bad = isfinite(energy[b]) ? 0.0 : 1.0;
    for (int t = tid; t < 3 * nat; t += nt)
        if (!isfinite((double)fg[t])) bad = 1.0;
    bad = block_max(bad, red);
    if (bad != 0.0) {   // the group's results are void; this chain goes home, its sibling replicas finish their rows
        if (tid == 0) {
            x[dof] = x0[dof];
            S.reason = 2;
            V.st[b] = S;
            V.gbad[c.group] = 1;   // (same value from every writer)
            atomicAdd(stopped, 1);
        }
        return;
    }
    double *F = V.Fs + (size_t)S.s * V.n3 + 3 * (size_t)a0;
    for (int t = tid; t < 3 * nat; t += nt) F[t] = (double)fg[t];
    __syncthreads();
    if (V.method == VSSR_VIB_FREDERIKSEN && tid < 3) {   // force on the displaced atom minus the sum over all atoms, in atom order
        double sum = 0.0;
        for (int i = 0; i < nat; ++i) sum += F[3 * i + tid];
        F[3 * da + tid] = F[3 * da + tid] - sum;
    }
    __syncthreads();
    if (S.s == V.nfree - 1) {
        double *row = V.K + ((size_t)c.group * V.ld + r) * V.ld;
        const double *F0 = V.Fs + 3 * (size_t)a0, *F1 = F0 + V.n3, *F2 = F1 + V.n3, *F3 = F2 + V.n3;
        for (int cc = tid; cc < c.m; cc += nt) {
            const int k = 3 * vl[cc / 3] + cc % 3;
            double v;
            if (V.nfree == 2) v = 0.5 * (F0[k] - F1[k]);
            else v = (-F0[k] + 8.0 * F1[k] - 8.0 * F2[k] + F3[k]) / 12.0;
            row[cc] = v / (2.0 * V.delta);
        }
        S.j += 1; S.s = 0;
    } else {
        S.s += 1;
    }
    if (tid == 0) {
        x[dof] = x0[dof];
        const int rn = c.rank + S.j * c.nrep;
        if (rn < c.m) {
            const int nd = 3 * vl[rn / 3] + rn % 3;
            x[nd] = x0[nd] + vib_k(V.nfree, S.s) * V.delta;
        } else {
            S.reason = 1;
            atomicAdd(stopped, 1);
        }
        V.st[b] = S;
    }
}

// Per group: Hs = K + K^T (the output Hessian, eV / A^2), A = D Hs D.  A void group reads NaN.
__global__ void __launch_bounds__(256)
k_vib_sym(const int *__restrict__ gm, const int *__restrict__ gfirst, const int *__restrict__ cfg_start, const int *__restrict__ vib_start,
          const int *__restrict__ vib_list, const double *__restrict__ mass, const int *__restrict__ gbad, int ld,
          const double *__restrict__ K, double *__restrict__ Hs, double *__restrict__ A) {
    __shared__ double dinv[VIB_MAX_DOF];
    const int g = blockIdx.x, tid = threadIdx.x, m = gm[g];
    const int b = gfirst[g];
    const int *vl = vib_list + vib_start[b];
    for (int t = tid; t < m; t += 256) dinv[t] = 1.0 / sqrt(mass[cfg_start[b] + vl[t / 3]]);
    __syncthreads();
    const size_t off = (size_t)g * ld * ld;
    const bool bad = gbad[g] != 0;
    for (int t = tid; t < m * m; t += 256) {
        const int i = t / m, j = t - i * m;
        const double h = bad ? __longlong_as_double(0x7FF8000000000000LL) : K[off + (size_t)i * ld + j] + K[off + (size_t)j * ld + i];
        Hs[off + (size_t)i * ld + j] = h;
        A[off + (size_t)i * ld + j] = (dinv[i] * h) * dinv[j];
    }
}

// One workgroup per group.  w2 [G][ld] <- eigenvalues (unordered), Vt [G][ld][ld] rows <- eigenvectors; jinfo [G][2] = (sweeps, converged).
// A group whose two matrices fit the dynamic LDS (lds_doubles) is solved there; the arithmetic is the same either way.
__global__ void __launch_bounds__(EIGH_THREADS)
k_vib_eigh(const int *__restrict__ gm, const int *__restrict__ gbad, int ld, int lds_doubles, const double *__restrict__ A, double *W,
           double *Vt, double *__restrict__ w2, int *__restrict__ jinfo) {
    extern __shared__ double mats[];
    __shared__ double cs[2 * 128];
    __shared__ double red[EIGH_THREADS];
    __shared__ int rotated;
    const int g = blockIdx.x, tid = threadIdx.x, m = gm[g];
    if (m == 0 || gbad[g]) {
        if (tid == 0) { jinfo[2 * g] = 0; jinfo[2 * g + 1] = 1; }
        return;
    }
    const size_t off = (size_t)g * ld * ld;
    const int ll = m | 1;
    const bool in_lds = 2 * m * ll <= lds_doubles;
    double *a = in_lds ? mats : W + off, *v = in_lds ? mats + (size_t)m * ll : Vt + off;
    const int la = in_lds ? ll : ld;
    int sweep, conv;
    jacobi_eigh(A + off, ld, a, v, m, la, cs, red, &rotated, sweep, conv);
    for (int t = tid; t < m; t += EIGH_THREADS) w2[(size_t)g * ld + t] = a[(size_t)t * la + t];
    if (in_lds)
        for (int t = tid; t < m * m; t += EIGH_THREADS) {
            const int i = t / m, j = t - i * m;
            Vt[off + (size_t)i * ld + j] = v[(size_t)i * ll + j];
        }
    if (tid == 0) { jinfo[2 * g] = sweep; jinfo[2 * g + 1] = conv; }
}

// One workgroup of 256 per group.  Eigenvalues ascending (the lower index first on ties); energies[k] = sign(w2) s sqrt(|w2|) eV;
// mode k = its eigenvector with the largest-magnitude entry (the first on ties) made positive; thermo = (E_pot(x0), zpe, f_vib) over
// the modes with energy > e_min; info = (m, modes with w2 < 0, modes left out, stop reason).
__global__ void __launch_bounds__(256)
k_vib_modes(const int *__restrict__ gm, const int *__restrict__ gfirst, const int *__restrict__ gbad, const int *__restrict__ jinfo, int ld,
            const double *__restrict__ w2, const double *__restrict__ Vt, const double *__restrict__ e_pot, double s_unit, double kT,
            double e_min, double *__restrict__ energies, double *__restrict__ modes, double *__restrict__ thermo, int *__restrict__ info) {
    __shared__ double lam[VIB_MAX_DOF], en[VIB_MAX_DOF];
    __shared__ int order[VIB_MAX_DOF];
    const int g = blockIdx.x, tid = threadIdx.x, m = gm[g];
    const size_t off = (size_t)g * ld * ld;
    const double e0 = e_pot[gfirst[g]];
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    if (gbad[g]) {
        for (int t = tid; t < m; t += 256) energies[(size_t)g * ld + t] = nan;
        for (int t = tid; t < m * m; t += 256) modes[off + (size_t)(t / m) * ld + t % m] = nan;
        if (tid == 0) {
            thermo[3 * g] = e0; thermo[3 * g + 1] = nan; thermo[3 * g + 2] = nan;
            info[4 * g] = m; info[4 * g + 1] = 0; info[4 * g + 2] = 0; info[4 * g + 3] = 2;
        }
        return;
    }
    if (tid < m) { lam[tid] = w2[(size_t)g * ld + tid]; order[tid] = tid; }
    __syncthreads();
    int at = 0;
    if (tid < m) {
        const double l = lam[tid];
        for (int j = 0; j < m; ++j) at += (lam[j] < l || (lam[j] == l && j < tid)) ? 1 : 0;
    }
    __syncthreads();
    if (tid < m) order[at] = tid;
    __syncthreads();
    if (tid < m) {
        const int src = order[tid];
        const double w = lam[src];
        const double e = (w < 0.0 ? -1.0 : 1.0) * s_unit * sqrt(fabs(w));
        en[tid] = e;
        energies[(size_t)g * ld + tid] = e;
        const double *v = Vt + off + (size_t)src * ld;
        double big = -1.0, sign = 1.0;
        for (int j = 0; j < m; ++j)
            if (fabs(v[j]) > big) { big = fabs(v[j]); sign = v[j] < 0.0 ? -1.0 : 1.0; }
        double *out = modes + off + (size_t)tid * ld;
        for (int j = 0; j < m; ++j) out[j] = sign * v[j];
    }
    __syncthreads();
    if (tid == 0) {
        int n_imag = 0, n_out = 0;
        double esum = 0.0, f = 0.0;
        for (int k = 0; k < m; ++k) {
            const double e = en[k];
            if (lam[order[k]] < 0.0) ++n_imag;
            if (e > e_min) {
                esum += e;
                if (kT > 0.0) f += 0.5 * e + kT * log1p(-exp(-e / kT));
            } else {
                ++n_out;
            }
        }
        const double zpe = 0.5 * esum;
        thermo[3 * g] = e0; thermo[3 * g + 1] = zpe; thermo[3 * g + 2] = kT > 0.0 ? f : zpe;
        info[4 * g] = m; info[4 * g + 1] = n_imag; info[4 * g + 2] = n_out; info[4 * g + 3] = jinfo[2 * g + 1] ? 1 : 3;
    }
}

// The call's workspace: one arena on the handle (d_vib), doubles first
struct VibWork {
    VibView V;
    double *mass, *Hs, *A, *W, *Vt, *w2, *en, *modes, *thermo;
    VibChain *ch;
    int *vib_start, *vib_list, *gm, *gfirst, *jinfo, *info, *flags;   // flags: [0] chains stopped, [1] replica mismatch
    int G, ld, max_share;
};

static int vib_lockstep(vssr_handle *h, const VibWork &W, uint32_t want) {
    hipStream_t st = h->stream;
    const int B = h->n_cfg;
    const long long need = (long long)W.V.nfree * W.max_share;   // evaluations at displaced positions
    int stopped = 0;   // (chains with nothing to displace stopped in k_vib_place)
    VSSR_HIP(h, hipMemcpyAsync(&stopped, W.flags, sizeof(int), hipMemcpyDeviceToHost, st));
    VSSR_HIP(h, hipStreamSynchronize(st));
    // The longest chain stops behind evaluation `need`: every iteration polls from there on, so the loop ends with that evaluation.
    // The budget leaves room for the windows 64 regrows give back.  Every chain ends back at x0, where the closing evaluation
    // leaves the batch complete; no chain ever leaves the evaluation.
    LockstepPlan plan{8, 0, LOCKSTEP_MASK_NEVER};
    plan.max_launch = need + 64LL * (plan.poll + 1) + 1;
    plan.stopped = W.flags; plan.stop_ints = 1; plan.groups = B;
    plan.always_close = true;
    plan.poll_all_from = need;
    plan.finished_at_start = stopped == B;
    bool finished;
    int rc = lockstep_run(h, plan, want, finished, [&] {
        with_forces(h, [&](const double *energy, auto *forces) {
            hipLaunchKernelGGL(k_vib_step<force_type<decltype(forces)>>, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(),
                               h->d_counters.as<int>(), energy, forces, h->d_pos.as<double>(), W.V, W.flags);
        });
    });
    if (rc) return rc;
    if (!finished) return set_err(h, VSSR_E_DEVICE, "vssr_batch_vibrations: the displacement loop did not finish");
    return VSSR_OK;
}

}  // namespace vssr

using namespace vssr;

extern "C" int vssr_batch_vibrations(vssr_handle *h, const vssr_vib_params *p, const double *mass, const uint8_t *vib, const int32_t *n_rep,
                                     int32_t n_groups, int32_t ld, uint32_t want, double *energies, double *hessian, double *modes,
                                     double *thermo, int32_t *info) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!p) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: null parameters");
    if (!mass) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: null masses");
    if (p->nfree != 2 && p->nfree != 4) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: nfree %d is neither 2 nor 4", (int)p->nfree);
    if (p->method != VSSR_VIB_STANDARD && p->method != VSSR_VIB_FREDERIKSEN)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: method %d is neither VSSR_VIB_STANDARD (0) nor VSSR_VIB_FREDERIKSEN (1)", (int)p->method);
    if (!(std::isfinite(p->delta) && p->delta > 0.0)) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: delta %g A (finite and > 0 wanted)", p->delta);
    if (!(std::isfinite(p->temperature) && p->temperature >= 0.0))
        return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: temperature %g K (finite and >= 0 wanted)", p->temperature);
    if (!(std::isfinite(p->e_min) && p->e_min >= 0.0)) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: e_min %g eV (finite and >= 0 wanted)", p->e_min);
    const int B = h->n_cfg, N = h->n_atoms;
    for (int i = 0; i < N; ++i)
        if (!(std::isfinite(mass[i]) && mass[i] > 0.0))
            return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: mass of atom %d is %g (finite and > 0 wanted)", i, mass[i]);
    if (!n_rep && n_groups != B) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: %d groups for %d chains without n_rep", (int)n_groups, B);
    if (n_groups < 1) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: %d groups", (int)n_groups);
    const int G = n_groups;
    std::vector<VibChain> ch(B);
    std::vector<int> gfirst(G), gm(G), vib_start(B + 1, 0), vib_list;
    {
        long long sum = 0;
        for (int g = 0; g < G; ++g) {
            const int nr = n_rep ? n_rep[g] : 1;
            if (nr < 1) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: group %d has %d replicas (>= 1 wanted)", g, nr);
            sum += nr;
            if (sum > B) break;
        }
        if (sum != B) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: the replica counts do not sum to the %d chains of the batch", B);
    }
    int max_m = 0, max_share = 0;
    for (int g = 0, b = 0; g < G; ++g) {
        const int nr = n_rep ? n_rep[g] : 1;
        gfirst[g] = b;
        const int f0 = h->h_cfg_start[b], nat = h->h_n_atoms[b];
        int nv = 0;
        for (int i = 0; i < nat; ++i) nv += (!vib || vib[f0 + i]) ? 1 : 0;
        const int m = 3 * nv;
        if (m > VIB_MAX_DOF)
            return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: group %d has %d degrees of freedom (at most %d: 85 vib atoms)", g, m, VIB_MAX_DOF);
        gm[g] = m;
        max_m = std::max(max_m, m);
        if (m) max_share = std::max(max_share, (m + nr - 1) / nr);
        for (int k = 0; k < nr; ++k, ++b) {
            const int a0 = h->h_cfg_start[b];
            if (h->h_n_atoms[b] != nat) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: chain %d is no replica of chain %d (atom counts)", b, gfirst[g]);
            if (std::memcmp(mass + a0, mass + f0, sizeof(double) * nat))
                return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: chain %d is no replica of chain %d (masses)", b, gfirst[g]);
            for (int i = 0; i < nat; ++i) {
                const bool on = !vib || vib[a0 + i];
                if (on != (!vib || vib[f0 + i])) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: chain %d is no replica of chain %d (vib mask)", b, gfirst[g]);
                if (on) vib_list.push_back(i);
            }
            vib_start[b + 1] = (int)vib_list.size();
            ch[b] = {g, k, nr, m};
        }
    }
    if (ld < max_m) return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: ld %d < %d degrees of freedom", (int)ld, max_m);
    const size_t ldd = (size_t)std::max<int>(ld, 1), mat = (size_t)G * ldd * ldd, n3 = 3 * (size_t)N;

    VSSR_HIP(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    VSSR_HIP(h, hipStreamSynchronize(st));
    VibWork W;
    auto layout = [&](Arena &a) {
        const size_t nB = B, nG = G;
        a.place(W.V.x0, n3); a.place(W.V.Fs, 4 * n3); a.place(W.mass, (size_t)N);
        a.place(W.V.K, mat); a.place(W.Hs, mat); a.place(W.A, mat); a.place(W.W, mat); a.place(W.Vt, mat);
        a.place(W.w2, nG * ldd); a.place(W.en, nG * ldd); a.place(W.thermo, 3 * nG);
        a.place(W.ch, nB); a.place(W.V.st, nB);
        a.place(W.vib_start, nB + 1); a.place(W.vib_list, vib_list.size() + 1);
        a.place(W.gm, nG); a.place(W.gfirst, nG); a.place(W.V.gbad, nG); a.place(W.jinfo, 2 * nG); a.place(W.info, 4 * nG);
        a.place(W.flags, 4);
    };
    if (h->d_vib.ensure(arena_size(layout))) return set_err(h, VSSR_E_NOMEM, "vibrations workspace: out of device memory");
    arena_carve(h->d_vib.p, layout);
    W.modes = W.V.K;   // (an alias: the rows are consumed by k_vib_sym before k_vib_modes writes the modes)
    W.V.ch = W.ch; W.V.vib_start = W.vib_start; W.V.vib_list = W.vib_list;
    W.V.n3 = n3; W.V.ld = (int)ldd; W.V.nfree = p->nfree; W.V.method = p->method; W.V.delta = p->delta;
    W.G = G; W.ld = (int)ldd; W.max_share = max_share;
    VSSR_HIP(h, hipMemcpyAsync(W.mass, mass, sizeof(double) * N, hipMemcpyHostToDevice, st));
    VSSR_HIP(h, hipMemcpyAsync(W.ch, ch.data(), sizeof(VibChain) * B, hipMemcpyHostToDevice, st));
    VSSR_HIP(h, hipMemcpyAsync(W.vib_start, vib_start.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice, st));
    if (!vib_list.empty()) VSSR_HIP(h, hipMemcpyAsync(W.vib_list, vib_list.data(), sizeof(int) * vib_list.size(), hipMemcpyHostToDevice, st));
    VSSR_HIP(h, hipMemcpyAsync(W.gm, gm.data(), sizeof(int) * G, hipMemcpyHostToDevice, st));
    VSSR_HIP(h, hipMemcpyAsync(W.gfirst, gfirst.data(), sizeof(int) * G, hipMemcpyHostToDevice, st));
    VSSR_HIP(h, hipMemsetAsync(W.V.gbad, 0, sizeof(int) * G, st));
    VSSR_HIP(h, hipMemsetAsync(W.flags, 0, sizeof(int) * 4, st));
    VSSR_HIP(h, hipMemsetAsync(W.V.K, 0, sizeof(double) * mat, st));
    int mismatch = 0;
    if (G != B) {
        hipLaunchKernelGGL(k_vib_compare, dim3(B), dim3(256), 0, st, W.ch, h->d_cfg_start.as<int>(), h->d_Z.as<int>(),
                           h->d_cell.as<unsigned long long>(), h->d_pbc.as<unsigned char>(), h->d_pos.as<unsigned long long>(), W.flags + 1);
        VSSR_HIP(h, hipGetLastError());
        VSSR_HIP(h, hipMemcpyAsync(&mismatch, W.flags + 1, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    VSSR_HIP(h, hipStreamSynchronize(st));   // (the host vectors leave scope with the call; nothing has moved yet)
    if (mismatch)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_vibrations: the replicas of a group differ (species, cell, pbc or positions; the comparison is bitwise)");

    const uint8_t *unused = nullptr;
    if (int rc = driver_open(h, nullptr, 2, unused, want)) return rc;
    hipLaunchKernelGGL(k_vib_place, dim3(B), dim3(256), 0, st, h->d_cfg_start.as<int>(), h->d_pos.as<double>(), W.V, W.flags);
    VSSR_HIP(h, hipGetLastError());
    if (int rc = vib_lockstep(h, W, want)) return rc;
    if (int rc = driver_close(h, false)) return rc;

    hipLaunchKernelGGL(k_vib_sym, dim3(G), dim3(256), 0, st, W.gm, W.gfirst, h->d_cfg_start.as<int>(), W.vib_start, W.vib_list, W.mass,
                       W.V.gbad, W.ld, W.V.K, W.Hs, W.A);
    // two m x (m | 1) matrices in LDS beside the solver's 10 KB: m <= 96 of the 160 KB of a gfx950 workgroup
    const int lds_m = std::min(max_m, 96);
    const int lds_doubles = 2 * lds_m * (lds_m | 1);
    if (lds_doubles * sizeof(double) > 48 * 1024)
        VSSR_HIP(h, hipFuncSetAttribute((const void *)k_vib_eigh, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_doubles * sizeof(double))));
    hipLaunchKernelGGL(k_vib_eigh, dim3(G), dim3(EIGH_THREADS), lds_doubles * sizeof(double), st, W.gm, W.V.gbad, W.ld, lds_doubles, W.A, W.W, W.Vt,
                       W.w2, W.jinfo);
    const double s_unit = VIB_HBAR * 1e10 / std::sqrt(1.602176634e-19 * 1.66053906660e-27);
    hipLaunchKernelGGL(k_vib_modes, dim3(G), dim3(256), 0, st, W.gm, W.gfirst, W.V.gbad, W.jinfo, W.ld, W.w2, W.Vt,
                       chain_energy64(h), s_unit, MD_KB * p->temperature, p->e_min, W.en,
                       W.modes, W.thermo, W.info);
    VSSR_HIP(h, hipGetLastError());
    VSSR_HIP(h, hipStreamSynchronize(st));

    // padded outputs: entries beyond a group's m are left as the caller had them
    std::vector<double> buf;
    auto fetch_mats = [&](const double *dev, double *out) -> int {
        buf.resize(mat);
        VSSR_HIP(h, hipMemcpy(buf.data(), dev, sizeof(double) * mat, hipMemcpyDeviceToHost));
        for (int g = 0; g < G; ++g)
            for (int i = 0; i < gm[g]; ++i)
                std::memcpy(out + ((size_t)g * ld + i) * ld, buf.data() + ((size_t)g * ldd + i) * ldd, sizeof(double) * gm[g]);
        return VSSR_OK;
    };
    if (hessian)
        if (int rc = fetch_mats(W.Hs, hessian)) return rc;
    if (modes)
        if (int rc = fetch_mats(W.modes, modes)) return rc;
    if (energies) {
        buf.resize((size_t)G * ldd);
        VSSR_HIP(h, hipMemcpy(buf.data(), W.en, sizeof(double) * G * ldd, hipMemcpyDeviceToHost));
        for (int g = 0; g < G; ++g) std::memcpy(energies + (size_t)g * ld, buf.data() + (size_t)g * ldd, sizeof(double) * gm[g]);
    }
    if (thermo) VSSR_HIP(h, hipMemcpy(thermo, W.thermo, sizeof(double) * 3 * G, hipMemcpyDeviceToHost));
    if (info) VSSR_HIP(h, hipMemcpy(info, W.info, sizeof(int) * 4 * G, hipMemcpyDeviceToHost));
    return VSSR_OK;
}
