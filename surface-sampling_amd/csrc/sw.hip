// sw.hip — Stillinger-Weber energy / per-atom energy / forces on gfx950 (fp64), batched over independent configurations.
//
// Semantics of LAMMPS pair_style sw (units metal).  Entry (i, j, k) of the parameter file:
//   phi2(r_ij) = A eps [B (sig/r)^p - (sig/r)^q] exp(sig / (r - a sig))            r < a sig, entry (i, j, j)
//   phi3(j, i, k) = lambda eps (cos theta_jik - costheta0)^2 exp(gamma sig / (r_ij - a sig))_(i,j,j) exp(gamma sig / (r_ik - a sig))_(i,k,k)
//                  lambda, eps, costheta0 of entry (i, j, k)
//   E = sum over pairs phi2 + sum over centres i and unordered neighbor pairs {j, k} phi3.
// Each directed slot i -> j carries half of phi2 with entry (i, j, j) (the same value LAMMPS takes once per pair whenever the
// entries (i, j, j) and (j, i, i) agree in their two-body columns, as in every published set); pe/atom splits pair terms half / half
// and three-body terms in thirds between i, j and k (ev_tally3).  vssr_sw_create refuses sets whose (i, j, k) and (i, k, j) entries
// differ in eps, lambda or costheta0: there the LAMMPS energy depends on the order of its neighbor list.
//
// The energy of centre i depends only on its slot vectors r_ij, and the three-body term factorises into per-slot radial factors ef
// and a function of the angle.  So a lane computes G_n = dE_i / d r_n of its slot n completely in one walk over the centre's other
// slots (ef and the unit vectors of all slots staged in LDS, no exp() in that walk); forces and pe/atom are then gathered per atom
// over its own and its reverse slots (k_sw_gather) -- no atomics, and a chain's results do not depend on what else is in the batch.
// Layout and launch shape follow k_tersoff_site4 (64 centres x 4 lanes per workgroup); rows longer than SW_MAXD slots take the
// long-row form inside the same launch (sw_dev.h).
#include "sw_dev.h"

namespace vssr {

__global__ void __launch_bounds__(SW_CENTRES * SW_LANES)
k_sw_site(PotView V, const SwP *__restrict__ P, double *__restrict__ eo, double *__restrict__ ej, double *__restrict__ gslot) {
    __shared__ SwShared sh;
    if (V.counters[2]) return;   // (uniform)
    const int i = blockIdx.x * SW_CENTRES + (threadIdx.x >> 2);
    sw_site_tile(sh, i, i < V.n_atoms && V.act.atom(i), V.n_types, P, V.type, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, eo,
                 ej, gslot);
}

__global__ void k_sw_gather(PotView V, const double *__restrict__ eo, const double *__restrict__ ej, const double *__restrict__ gslot,
                            double *__restrict__ e_atom, double *__restrict__ forces) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (!V.runs(c)) return;
    sw_gather_atom(c, V.row_start, V.rev, eo, ej, gslot, e_atom, forces);
}

int sw_stress(vssr_handle *h) { return slot_stress(h, SwSlots::of(h).gslot); }

int sw_run(vssr_handle *h, uint32_t want) {
    (void)want;
    int rc = analytic_begin(h, h->pot_cutoff, SwSlots::doubles, "sw");
    if (rc) return rc;
    const PotView V = pot_view(h);
    const SwSlots S = SwSlots::of(h);
    const int N = V.n_atoms;
    hipLaunchKernelGGL(k_sw_site, dim3((N + SW_CENTRES - 1) / SW_CENTRES), dim3(SW_CENTRES * SW_LANES), 0, h->stream, V,
                       h->pot_params.as<SwP>(), S.eo, S.ej, S.gslot);
    hipLaunchKernelGGL(k_sw_gather, dim3((N + 63) / 64), dim3(64), 0, h->stream, V, S.eo, S.ej, S.gslot, h->d_pot_ea.as<double>(),
                       h->d_pot_f.as<double>());
    return analytic_end(h, V);
}

}  // namespace vssr
