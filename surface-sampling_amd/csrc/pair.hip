// pair.hip — pair potentials with damped-shifted-force Coulomb on gfx950 (fp64), batched over independent configurations.
//
// Semantics of LAMMPS pair_style lj/cut, morse, buck, born and coul/dsf (units metal, qqrd2e = 14.399645), alone or combined as
// pair_style hybrid / hybrid/overlay: every ordered type pair (a, b) carries up to PAIR_MAX_TERMS terms, each with its own cutoff,
//   lj/cut    4 eps [(sig/r)^12 - (sig/r)^6]                      morse  D0 [exp(-2 alpha (r - r0)) - 2 exp(-alpha (r - r0))]
//   buck      A exp(-r/rho) - C/r^6                                born   A exp((sig - r)/rho) - C/r^6 + D/r^8
//   coul/dsf  qqrd2e q_a q_b [erfc(alpha r)/r - erfc(alpha rc)/rc + B (r - rc)],  B = erfc(alpha rc)/rc^2 + 2 alpha/sqrt(pi) exp(-alpha^2 rc^2)/rc
//   coul/long qqrd2e q_a q_b erfc(g r)/r, no shift: the real-space part of the Ewald sum of a handle with k-space (ewald.hip runs
//             behind the site kernel and adds the reciprocal, self and background terms to the same per-atom results)
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
// 1/2 E'(r_n) u_n into d_gbar for slot_stress (pot_common.hip) and nothing else, so an evaluation that is not asked for stress
// stores no per-slot data at all.
#include "pair_dev.h"

namespace vssr {

template <bool GRAD>
__global__ void __launch_bounds__(PAIR_CENTRES * PAIR_LANES)
k_pair_site(PotView V, const PairTable *__restrict__ P, double *__restrict__ e_atom, double *__restrict__ forces, double *__restrict__ gslot) {
    __shared__ PairTerm sh[PAIR_MAX_TYPES * PAIR_MAX_TYPES * PAIR_MAX_TERMS];
    if (V.counters[2]) return;   // (uniform)
    const int i = blockIdx.x * PAIR_CENTRES + (threadIdx.x >> 2);
    pair_site_tile<GRAD>(sh, i, i < V.n_atoms && V.act.atom(i), V.n_types, P, V.type, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge,
                         V.edge_S, e_atom, forces, gslot);
}

template <bool GRAD>
static void launch_site(vssr_handle *h, const PotView &V, double *gslot) {
    hipLaunchKernelGGL(k_pair_site<GRAD>, dim3((V.n_atoms + PAIR_CENTRES - 1) / PAIR_CENTRES), dim3(PAIR_CENTRES * PAIR_LANES), 0, h->stream,
                       V, h->pot_params.as<PairTable>(), h->d_pot_ea.as<double>(), h->d_pot_f.as<double>(), gslot);
}

// vssr_batch_stress: the gradient launch over the resident rows of the last run, then the virial kernel Tersoff and SW use
int pair_stress(vssr_handle *h) {
    if (h->d_gbar.ensure(sizeof(double) * 3 * (size_t)h->slot_cap)) return set_err(h, VSSR_E_NOMEM, "pair gradients: out of device memory");
    launch_site<true>(h, pot_view(h), h->d_gbar.as<double>());
    VSSR_HIP(h, hipGetLastError());
    if (int rc = slot_stress(h, h->d_gbar.as<double>())) return rc;
    return h->ew_on ? ewald_stress(h) : VSSR_OK;
}

int pair_run(vssr_handle *h, uint32_t want) {
    (void)want;
    int rc = analytic_begin(h, h->pot_cutoff, nullptr, "pair");
    if (rc) return rc;
    const PotView V = pot_view(h);
    launch_site<false>(h, V, nullptr);
    if (h->ew_on) ewald_run(h, V);
    return analytic_end(h, V);
}

}  // namespace vssr
