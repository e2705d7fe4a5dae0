// pair.hip — pair potentials with damped-shifted-force Coulomb on gfx950 (fp64), batched over independent configurations.
//
// Semantics of LAMMPS pair_style lj/cut, morse, buck, born and coul/dsf (units metal, qqrd2e = 14.399645), alone or combined as
// pair_style hybrid / hybrid/overlay: every ordered type pair (a, b) carries up to PAIR_MAX_TERMS terms, each with its own cutoff,
//   lj/cut    4 eps [(sig/r)^12 - (sig/r)^6]                      morse  D0 [exp(-2 alpha (r - r0)) - 2 exp(-alpha (r - r0))]
//   buck      A exp(-r/rho) - C/r^6                                born   A exp((sig - r)/rho) - C/r^6 + D/r^8
//   coul/dsf  qqrd2e q_a q_b [erfc(alpha r)/r - erfc(alpha rc)/rc + B (r - rc)],  B = erfc(alpha rc)/rc^2 + 2 alpha/sqrt(pi) exp(-alpha^2 rc^2)/rc
// (Fennell & Gezelter 2006: energy and force both vanish at rc), minus E(rc) for the first four under pair_modify shift yes.  pe/atom
// splits every pair half / half; the coul/dsf self term -(erfc(alpha rc)/(2 rc) + alpha/sqrt(pi)) qqrd2e q_i^2 goes to atom i.
//
// A pair potential needs no reverse gather: the edge list holds i -> j and j -> i, so centre i takes half of every pair energy and
// its own full force F_i = sum_n E'(r_n) u_n from its own row.  One site kernel in the launch shape of k_sw_site (64 centres x 4
// lanes per workgroup): the lanes stride the centre's slots -- rows of any length take the same loop, a 12 A cutoff on an 8 A cell
// gives rows of several hundred slots -- and a fixed-order sum over the DPP quad finishes the centre.  No atomics; a centre's
// numbers depend on its own row only, so a chain's results do not depend on what else is in the batch.  The term table (at most
// 8 x 8 x 3 entries of 64 bytes) sits in LDS: lanes of a wave read the entries of different type pairs, 16 dwords apart, so four
// distinct pairs already cover the 64 banks; with the 9 pairs of a three-type oxide that is a 2- or 3-way conflict on a read that
// is followed by an inlined fp64 exp or erfc (a hundred and more fp64 VALU instructions per slot), not worth a transposed table.
// vssr_batch_stress launches the same kernel once more with GRAD = true: it writes the per-slot gradients G_n = dE_i / d r_n =
// 1/2 E'(r_n) u_n into d_gbar for slot_stress (tersoff.hip) and nothing else, so an evaluation that is not asked for stress
// stores no per-slot data at all.
#include "pair_dev.h"

namespace vssr {

template <bool GRAD>
__global__ void __launch_bounds__(PAIR_CENTRES * PAIR_LANES)
k_pair_site(int N, int nt, const PairTable *__restrict__ P, const int *__restrict__ type, const int *__restrict__ atom_cfg,
            const double *__restrict__ cell, const double *__restrict__ wpos, const int *__restrict__ row_start,
            const float4 *__restrict__ edge, const int *__restrict__ edge_S, const int *__restrict__ counters,
            double *__restrict__ e_atom, double *__restrict__ forces, double *__restrict__ gslot, ActiveView av) {
    __shared__ PairTerm sh[PAIR_MAX_TYPES * PAIR_MAX_TYPES * PAIR_MAX_TERMS];
    if (counters[2]) return;   // (uniform)
    const int tid = threadIdx.x, q = tid & (PAIR_LANES - 1);
    // the terms of the nt x nt pairs in use, packed [a][b][k]; 16-byte pieces
    {
        constexpr int PIECES = sizeof(PairTerm) / sizeof(uint4);
        const uint4 *src = reinterpret_cast<const uint4 *>(P->term);
        uint4 *dst = reinterpret_cast<uint4 *>(sh);
        for (int t = tid; t < nt * nt * PAIR_MAX_TERMS * PIECES; t += PAIR_CENTRES * PAIR_LANES) {
            const int term = t / PIECES, piece = t % PIECES;
            const int k = term % PAIR_MAX_TERMS, ab = term / PAIR_MAX_TERMS, a = ab / nt, b = ab % nt;
            dst[t] = src[((a * PAIR_MAX_TYPES + b) * PAIR_MAX_TERMS + k) * PIECES + piece];
        }
    }
    __syncthreads();
    const int i = blockIdx.x * PAIR_CENTRES + (tid >> 2);
    const bool mine = i < N && av.atom(i);
    int e0 = 0, deg = 0, ti = 0;
    const double *C = cell;
    if (mine) {
        e0 = row_start[i];
        deg = row_start[i + 1] - e0;
        ti = type[i];
        C = cell + 9 * atom_cfg[i];
    }
    double es = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
#pragma unroll 1
    for (int n = q; n < deg; n += PAIR_LANES) {
        const int j = __float_as_int(edge[e0 + n].w);
        if (j < 0) continue;   // padding slot (k_slot_stress skips it as well)
        double rv[3];
        edge_vec(wpos, C, i, j, edge_S[e0 + n], rv);
        const double r = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
        const PairTerm *T = sh + (ti * nt + type[j]) * PAIR_MAX_TERMS;
        double e = 0.0, de = 0.0;
#pragma unroll 1
        for (int k = 0; k < PAIR_MAX_TERMS; ++k) {
            if (T[k].style == VSSR_PAIR_NONE) break;
            if (!(r < T[k].rc)) continue;
            double ek, dek;
            pair_term(T[k], r, ek, dek);
            e += ek;
            de += dek;
        }
        const double w = de / r;
        if (GRAD) {
            double *g = gslot + 3 * (size_t)(e0 + n);
            g[0] = 0.5 * w * rv[0]; g[1] = 0.5 * w * rv[1]; g[2] = 0.5 * w * rv[2];
        } else {
            es += e;
            fx += w * rv[0]; fy += w * rv[1]; fz += w * rv[2];
        }
    }
    if (GRAD) return;
    // (every lane of the wave arrives here: lanes without a centre carry zeros into the quad sums)
    es = quad_sum_f64(es);
    fx = quad_sum_f64(fx);
    fy = quad_sum_f64(fy);
    fz = quad_sum_f64(fz);
    if (mine && q == 0) {
        e_atom[i] = 0.5 * es + P->self_e[ti];
        forces[3 * i] = fx; forces[3 * i + 1] = fy; forces[3 * i + 2] = fz;
    }
}

__global__ void __launch_bounds__(256)
k_pair_energy(const int *__restrict__ cfg_start, const double *__restrict__ e_atom, double *__restrict__ energy,
              const unsigned char *__restrict__ active) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    if (active && !active[b]) return;
    tersoff_chain_energy(b, red, cfg_start, e_atom, energy);
}

template <bool GRAD>
static void launch_site(vssr_handle *h, double *gslot) {
    const int N = h->n_atoms;
    const ActiveView av{h->active_mask, h->d_atom_cfg.as<int>()};
    hipLaunchKernelGGL(k_pair_site<GRAD>, dim3((N + PAIR_CENTRES - 1) / PAIR_CENTRES), dim3(PAIR_CENTRES * PAIR_LANES), 0, h->stream, N,
                       h->n_types, h->pot_params.as<PairTable>(), h->d_Z.as<int>(), h->d_atom_cfg.as<int>(), h->d_cell.as<double>(),
                       h->d_wpos.as<double>(), h->d_row_start.as<int>(), h->d_edge.as<float4>(), h->d_edge_S.as<int>(),
                       h->d_counters.as<int>(), h->d_pot_ea.as<double>(), h->d_pot_f.as<double>(), gslot, av);
}

// vssr_batch_stress: the gradient launch over the resident rows of the last run, then the virial kernel Tersoff and SW use
int pair_stress(vssr_handle *h) {
    if (h->d_gbar.ensure(sizeof(double) * 3 * (size_t)h->slot_cap)) return set_err(h, VSSR_E_NOMEM, "pair gradients: out of device memory");
    launch_site<true>(h, h->d_gbar.as<double>());
    VSSR_HIP(h, hipGetLastError());
    return slot_stress(h, h->d_gbar.as<double>());
}

int pair_run(vssr_handle *h, uint32_t want) {
    (void)want;
    const int N = h->n_atoms;
    hipStream_t st = h->stream;
    int rc = build_neighbors(h, h->pot_cutoff);
    if (rc) return rc;
    if (h->d_pot_e.ensure(sizeof(double) * h->n_cfg) || h->d_pot_ea.ensure(sizeof(double) * N) || h->d_pot_f.ensure(sizeof(double) * 3 * N))
        return set_err(h, VSSR_E_NOMEM, "pair buffers: out of device memory");
    h->prof.begin(KC_ANALYTIC, st);
    launch_site<false>(h, nullptr);
    hipLaunchKernelGGL(k_pair_energy, dim3(h->n_cfg), dim3(256), 0, st, h->d_cfg_start.as<int>(), h->d_pot_ea.as<double>(),
                       h->d_pot_e.as<double>(), h->active_mask);
    h->prof.end(st);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
