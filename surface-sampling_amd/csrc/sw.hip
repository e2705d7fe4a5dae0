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
k_sw_site(int N, int nt, const SwP *__restrict__ P, const int *__restrict__ type, const int *__restrict__ atom_cfg,
          const double *__restrict__ cell, const double *__restrict__ wpos, const int *__restrict__ row_start,
          const float4 *__restrict__ edge, const int *__restrict__ edge_S, const int *__restrict__ counters,
          double *__restrict__ eo, double *__restrict__ ej, double *__restrict__ gslot, ActiveView av) {
    __shared__ SwShared sh;
    if (counters[2]) return;   // (uniform)
    const int i = blockIdx.x * SW_CENTRES + (threadIdx.x >> 2);
    sw_site_tile(sh, i, i < N && av.atom(i), nt, P, type, atom_cfg, cell, wpos, row_start, edge, edge_S, eo, ej, gslot);
}

__global__ void k_sw_gather(int N, const int *__restrict__ row_start, const int *__restrict__ rev, const int *__restrict__ counters,
                            const double *__restrict__ eo, const double *__restrict__ ej, const double *__restrict__ gslot,
                            double *__restrict__ e_atom, double *__restrict__ forces, ActiveView av) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N || counters[2] || !av.atom(c)) return;
    sw_gather_atom(c, row_start, rev, eo, ej, gslot, e_atom, forces);
}

__global__ void __launch_bounds__(256)
k_sw_energy(const int *__restrict__ cfg_start, const double *__restrict__ e_atom, double *__restrict__ energy,
            const unsigned char *__restrict__ active) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    if (active && !active[b]) return;
    tersoff_chain_energy(b, red, cfg_start, e_atom, energy);
}

int sw_stress(vssr_handle *h) { return slot_stress(h, h->d_gbar.as<double>() + 2 * h->slot_cap); }   // eo | ej | G (sw_run)

int sw_run(vssr_handle *h, uint32_t want) {
    (void)want;
    const int N = h->n_atoms;
    hipStream_t st = h->stream;
    int rc = build_neighbors(h, h->pot_cutoff);
    if (rc) return rc;
    if (h->d_pot_e.ensure(sizeof(double) * h->n_cfg) || h->d_pot_ea.ensure(sizeof(double) * N) ||
        h->d_pot_f.ensure(sizeof(double) * 3 * N) || h->d_gbar.ensure(sizeof(double) * 5 * (size_t)h->slot_cap))
        return set_err(h, VSSR_E_NOMEM, "sw buffers: out of device memory");
    double *eo = h->d_gbar.as<double>();
    double *ej = eo + h->slot_cap;
    double *gslot = ej + h->slot_cap;
    h->prof.begin(KC_ANALYTIC, st);
    const ActiveView av{h->active_mask, h->d_atom_cfg.as<int>()};
    hipLaunchKernelGGL(k_sw_site, dim3((N + SW_CENTRES - 1) / SW_CENTRES), dim3(SW_CENTRES * SW_LANES), 0, st, N, h->n_types,
                       h->pot_params.as<SwP>(), h->d_Z.as<int>(), h->d_atom_cfg.as<int>(), h->d_cell.as<double>(),
                       h->d_wpos.as<double>(), h->d_row_start.as<int>(), h->d_edge.as<float4>(), h->d_edge_S.as<int>(),
                       h->d_counters.as<int>(), eo, ej, gslot, av);
    hipLaunchKernelGGL(k_sw_gather, dim3((N + 63) / 64), dim3(64), 0, st, N, h->d_row_start.as<int>(), h->d_rev.as<int>(),
                       h->d_counters.as<int>(), eo, ej, gslot, h->d_pot_ea.as<double>(), h->d_pot_f.as<double>(), av);
    hipLaunchKernelGGL(k_sw_energy, dim3(h->n_cfg), dim3(256), 0, st, h->d_cfg_start.as<int>(), h->d_pot_ea.as<double>(),
                       h->d_pot_e.as<double>(), h->active_mask);
    h->prof.end(st);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
