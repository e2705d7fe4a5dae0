// vashishta.hip — Vashishta energy / per-atom energy / forces on gfx950 (fp64), batched over independent configurations.
//
// Semantics of LAMMPS pair_style vashishta (units metal, qqr2e = 14.399645).  Entry (i, j, k) of the parameter file
// (H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta):
//   V(r)    = H / r^eta + qqr2e Zi Zj / r exp(-r / lambda1) - D / r^4 exp(-r / lambda4) - W / r^6
//   phi2(r) = V(r) - V(rc) - (r - rc) V'(rc)                              r < rc, entry (i, j, j): energy and force vanish at rc
//   phi3(j, i, k) = B f_ij(r_ij) f_ik(r_ik) dc^2 / (1 + C dc^2),  dc = cos theta_jik - costheta        B, C, costheta of entry (i, j, k)
//   f_ij(r) = exp(gamma / (r - r0)) for r < r0, else 0                    gamma, r0 of entry (i, j, j)
//   E = sum over pairs phi2 + sum over centres i and unordered neighbor pairs {j, k} phi3.
// Each directed slot i -> j carries half of phi2 with entry (i, j, j); vssr_vashishta_create refuses sets whose (i, j, j) and (j, i, i)
// entries differ in a two-body column and whose (i, j, k) and (i, k, j) entries differ in B, C or costheta (there the LAMMPS energy
// depends on the order of its neighbor list).  pe/atom splits pair terms half / half and three-body terms in thirds (ev_tally3).
//
// The two ranges differ by an order of magnitude: the pair term reaches to rc (7.35 A in SiC: 150 .. 200 slots per row), the three-body
// term to r0 (2.9 A: about 4 slots).  So the site kernel is the pair kernel's row walk (k_pair_site: 64 centres x 4 lanes, rows of any
// length, the centre's half pair energy and full pair force from its own row, nothing stored per slot) that also compacts the few
// slots below r0max -- the largest r0 of the table, so a slot and its reverse are short together -- into a 16-entry row in LDS, and
// then the Stillinger-Weber tile on that short row (sw_dev.h: G3_n = dE3_i / d r_n in one walk over the other short slots, no exp()
// in it).  The three-body parts that belong to the neighbors travel through per-slot scratch at the short slots only and are
// gathered per atom over the reverse slots (k_vashishta_gather) -- no atomics, and a chain's results do not depend on what else is
// in the batch.  Centres with more than 16 short slots take the long form inside the same launch (vashishta_dev.h).
// vssr_batch_stress launches the site kernel once more with GRAD = true: it writes the complete per-slot gradients (half pair
// gradient + three-body gradient) for slot_stress and nothing else.
// LDS: 46 080 B of short rows per workgroup plus the tables of the species in use in the launch's dynamic LDS (VashTables: 576 B for
// two species, 18 432 B for eight), so the usual two- and three-species sets run three workgroups per CU, as the registers allow.
#include "vashishta_dev.h"

namespace vssr {

template <bool GRAD>
__global__ void __launch_bounds__(VA_CENTRES * VA_LANES)
k_vashishta_site(PotView V, const VashP *__restrict__ P, double r0max, double *__restrict__ e_atom, double *__restrict__ forces,
                 double *__restrict__ ej3, double *__restrict__ gslot, int *__restrict__ sidx) {
    __shared__ VashShared sh;
    extern __shared__ __align__(16) unsigned char va_tables[];   // VashTables::bytes(n_types)
    if (V.counters[2]) return;   // (uniform)
    const int i = blockIdx.x * VA_CENTRES + (threadIdx.x >> 2);
    vash_site_tile<GRAD>(sh, VashTables::in(va_tables, V.n_types), i, i < V.n_atoms && V.act.atom(i), V.n_types, r0max, P, V.type,
                         V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, e_atom, forces, ej3, gslot, sidx);
}

__global__ void k_vashishta_gather(PotView V, double r0max, const double *__restrict__ ej3, const double *__restrict__ gslot,
                                   const int *__restrict__ sidx, double *__restrict__ e_atom, double *__restrict__ forces) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (!V.runs(c)) return;
    vash_gather_atom(c, r0max, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, V.rev, ej3, gslot, sidx, e_atom, forces);
}

template <bool GRAD>
static void launch_site(vssr_handle *h, const PotView &V, const VashSlots &S) {
    hipLaunchKernelGGL(k_vashishta_site<GRAD>, dim3((V.n_atoms + VA_CENTRES - 1) / VA_CENTRES), dim3(VA_CENTRES * VA_LANES),
                       VashTables::bytes(V.n_types), h->stream, V, h->pot_params.as<VashP>(), h->vash_r0max, h->d_pot_ea.as<double>(),
                       h->d_pot_f.as<double>(), S.ej3, S.gslot, S.sidx);
}

// vssr_batch_stress: the gradient launch over the resident rows of the last run, then the virial kernel Tersoff, SW and pair use
int vashishta_stress(vssr_handle *h) {
    if (h->d_gbar.ensure(sizeof(double) * VashSlots::doubles(h))) return set_err(h, VSSR_E_NOMEM, "vashishta gradients: out of device memory");
    const VashSlots S = VashSlots::of(h);
    launch_site<true>(h, pot_view(h), S);
    VSSR_HIP(h, hipGetLastError());
    return slot_stress(h, S.gslot);
}

int vashishta_run(vssr_handle *h, uint32_t want) {
    (void)want;
    int rc = analytic_begin(h, h->pot_cutoff, VashSlots::doubles, "vashishta");
    if (rc) return rc;
    const PotView V = pot_view(h);
    const VashSlots S = VashSlots::of(h);
    launch_site<false>(h, V, S);
    hipLaunchKernelGGL(k_vashishta_gather, dim3((V.n_atoms + 63) / 64), dim3(64), 0, h->stream, V, h->vash_r0max, S.ej3, S.gslot, S.sidx,
                       h->d_pot_ea.as<double>(), h->d_pot_f.as<double>());
    return analytic_end(h, V);
}

}  // namespace vssr
