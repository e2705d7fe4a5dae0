// adp.hip — angular-dependent potential (LAMMPS pair_style adp) energy / per-atom energy / forces / stress on gfx950 (fp64),
// batched over independent configurations.  An EAM handle with eam_adp set (vssr_eam_create_adp) runs these kernels in place of
// those of eam.hip; the formulas, the table layout and the per-atom row are in adp_dev.h.
// Launch shape of eam.hip: one thread owns one centre and walks its CSR row.  Pass 1 sums rho, mu and lambda of the centre and
// evaluates F, F' (one 12-double row per atom in d_gbar); pass 2 gathers the rows of the neighbours and sums pe/atom and the
// force -- every pair is seen from both ends, so there is no scatter and no atomics, and every sum runs in row order.
#include "adp_dev.h"

namespace vssr {

static AdpTyped adp_tables(const vssr_handle *h) { return AdpTyped{eam_tables(h)}; }

__global__ void k_adp_density(PotView V, vssr_eam_grid g, AdpTyped A, double *__restrict__ rows) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!V.runs(i)) return;
    adp_density_atom(i, g, A, V.type, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, rows);
}

__global__ void k_adp_force(PotView V, vssr_eam_grid g, AdpTyped A, const double *__restrict__ rows, double *__restrict__ e_atom,
                            double *__restrict__ forces) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!V.runs(i)) return;
    adp_force_atom(i, g, A, V.type, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, rows, e_atom, forces);
}

__global__ void __launch_bounds__(VIR_THREADS)
k_adp_stress(PotView V, vssr_eam_grid g, AdpTyped A, const double *__restrict__ rows, double *__restrict__ stress,
             double *__restrict__ stress_std) {
    __shared__ double red[6][VIR_THREADS];
    if (V.counters[2]) return;   // (uniform)
    adp_stress_chain(blockIdx.x, red, g, A, V.type, V.cfg_start, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, rows, stress, stress_std);
}

int adp_stress(vssr_handle *h) {
    if (h->d_stress.ensure(sizeof(double) * 12 * (size_t)h->n_cfg)) return set_err(h, VSSR_E_NOMEM, "out of device memory (stress)");
    double *out = h->d_stress.as<double>();
    hipLaunchKernelGGL(k_adp_stress, dim3(h->n_cfg), dim3(VIR_THREADS), 0, h->stream, pot_view(h), h->eam_grid, adp_tables(h),
                       AdpAtoms::of(h), out, out + 6 * (size_t)h->n_cfg);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

int adp_run(vssr_handle *h, uint32_t want) {
    (void)want;
    int rc = analytic_begin(h, h->eam_grid.cutoff, AdpAtoms::doubles, "ADP");
    if (rc) return rc;
    const PotView V = pot_view(h);
    const AdpTyped A = adp_tables(h);
    double *rows = AdpAtoms::of(h);
    dim3 blk(64), grd((V.n_atoms + 63) / 64);
    hipLaunchKernelGGL(k_adp_density, grd, blk, 0, h->stream, V, h->eam_grid, A, rows);
    hipLaunchKernelGGL(k_adp_force, grd, blk, 0, h->stream, V, h->eam_grid, A, rows, h->d_pot_ea.as<double>(), h->d_pot_f.as<double>());
    return analytic_end(h, V);
}

}  // namespace vssr
