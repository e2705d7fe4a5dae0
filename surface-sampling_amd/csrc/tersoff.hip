// tersoff.hip — Tersoff energy / per-atom energy / forces on gfx950 (fp64), batched over
// independent configurations.
//
// Replaces LAMMMPSCalc.run_lammps_calc with `pair_style tersoff` (reference
// mcmc/calculators/calculators.py:507-640; potential mcmc/potentials/GaN.tersoff; template
// tutorials/data/GaN_0001/GaN_0001_lammps_energy_template.txt).  Semantics follow LAMMPS
// pair_tersoff: entry (i,j,k); two-body terms and fc(r_ij) from (i,j,j),
// three-body terms and fc(r_ik) from (i,j,k); b_ij with the LAMMPS asymptotic branches;
// pe/atom splits every directed pair term half/half between i and j.
//
// The site energy E_i depends only on the vectors r_ij from i to its neighbors, so a centre is self-contained:
// G_slot = dE_i/d r_ij is written for its own slots, and the force on atom c is gathered as
// sum_{slots of c} (G[slot] - G[rev[slot]]) — no atomics, deterministic.
//
// k_tersoff_site4 (rows of <= TS_MAXD slots, <= 4 species: every row of the GaN workloads): FOUR lanes per centre.  The
// neighborhood (unit vectors, distances, types) is written to LDS once, the parameter entries sit in LDS next to it, and
// every loop of the three-body sums runs from LDS -- the first form of this kernel (k_tersoff_site, one thread per centre,
// kept for longer rows / more species) chased edge -> type -> parameters -> position through global memory for every (j, k)
// and accumulated dE/dr_ik with global read-modify-writes: 882 us per evaluation of 4 096 x 48 atoms, all of it latency
// (profiles/r04/NOTES_tersoff.md).  A lane owns the slots n = q, q + 4, ... of its centre in both passes:
//   pass 1 (slot n as j): zeta_n over all k, b_ij, the pair energy, pref_n = 1/2 fc fA db/dzeta -> LDS, and the slot's own part of
//                          G_n = dV/dr_n rhat_n + pref_n sum_m dzeta_nm/dr_n  (sums collected in the zeta walk, scaled afterwards)
//   pass 2 (slot n as k): G_n += sum_m pref_m dzeta_mn/dr_n
// so every G is produced by one lane (stored by pass 1, completed by pass 2), without atomics.
#include "tersoff_dev.h"

namespace vssr {

__global__ void __launch_bounds__(64)
k_tersoff_site(PotView V, const TersP *__restrict__ P, double *__restrict__ eps /*[slots]*/, double *__restrict__ gslot /*[slots][3]*/,
               int longer_than) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!V.runs(i)) return;
    tersoff_site_atom(i, V.n_types, P, V.type, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, eps, gslot, longer_than);
}

__global__ void __launch_bounds__(TS_CENTRES * TS_LANES)
k_tersoff_site4(PotView V, const TersP *__restrict__ P, double *__restrict__ eps /*[slots]*/, double *__restrict__ gslot /*[slots][3]*/) {
    __shared__ TersShared sh;
    if (V.counters[2]) return;   // (uniform)
    const int i = blockIdx.x * TS_CENTRES + (threadIdx.x >> 2);
    tersoff_derive_params(sh, V.n_types, P);
    tersoff_site4_tile(sh, i, i < V.n_atoms && V.act.atom(i), V.n_types, V.type, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S,
                       eps, gslot);
}

__global__ void k_tersoff_gather(PotView V, const double *__restrict__ eps, const double *__restrict__ gslot, double *__restrict__ e_atom,
                                 double *__restrict__ forces) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (!V.runs(c)) return;
    tersoff_gather_atom(c, V.row_start, V.rev, eps, gslot, e_atom, forces);
}

int tersoff_stress(vssr_handle *h) { return slot_stress(h, slots_of(h).gslot); }

int tersoff_run(vssr_handle *h, uint32_t want) {
    (void)want;
    int rc = analytic_begin(h, h->pot_cutoff, TersoffSlots::doubles, "tersoff");
    if (rc) return rc;
    const PotView V = pot_view(h);
    const TersoffSlots S = slots_of(h);
    const TersP *P = h->pot_params.as<TersP>();
    const int N = V.n_atoms;
    hipStream_t st = h->stream;
    dim3 blk(64), grd((N + 63) / 64);
    // rows of <= TS_MAXD slots: four lanes per centre from LDS; longer rows (and potentials of more than 4 species): one thread per
    // centre.
    const bool fast = h->n_types * h->n_types * h->n_types <= TS_MAXP;
    if (fast)
        hipLaunchKernelGGL(k_tersoff_site4, dim3((N + TS_CENTRES - 1) / TS_CENTRES), dim3(TS_CENTRES * TS_LANES), 0, st, V, P, S.eps, S.gslot);
    hipLaunchKernelGGL(k_tersoff_site, grd, blk, 0, st, V, P, S.eps, S.gslot, fast ? TS_MAXD : -1);
    hipLaunchKernelGGL(k_tersoff_gather, grd, blk, 0, st, V, S.eps, S.gslot, h->d_pot_ea.as<double>(), h->d_pot_f.as<double>());
    return analytic_end(h, V);
}

}  // namespace vssr
