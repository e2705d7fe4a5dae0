// eam.hip — embedded-atom energy / per-atom energy / forces on gfx950 (fp64), batched over independent configurations.
//
// Replaces the `lmp` subprocess behind LAMMPSRunSurfCalc with `pair_style eam` + a funcfl file (reference
// mcmc/calculators/calculators.py:755-811, mcmc/calculators/lammpsrun.py:309-469; potential mcmc/potentials/Cu_u3.eam;
// BASELINE configs[0], tests/test_Cu.py).  Semantics follow LAMMPS pair_eam for one funcfl element:
//   E = sum_i F(rho_i) + 1/2 sum_{i != j} phi(r_ij),  rho_i = sum_j rho(r_ij),  phi(r) = z2r(r) / r,
//   z2r = 27.2 * 0.529 * Z(r)^2 (Hartree * Bohr -> eV * A), all three functions as LAMMPS' cubic splines over the file's
//   grids (coefficients built at vssr_eam_create, see build_spline), rho beyond the table extrapolated linearly,
//   pe/atom = F(rho_i) + 1/2 sum_j phi.
// One thread owns one centre and walks its CSR row (padded multigraph of nbr.hip, cutoff = the file's cutoff):
// pass 1 densities and F'(rho_i); pass 2 energies and the force sum_slots [(F'_i + F'_j) rho'(r) + phi'(r)] r_hat --
// every pair is seen from both ends, so there is no scatter and no atomics.  Several elements (pair_style eam/alloy, eam/fs,
// funcfl files mixed per type) run the same bodies with the type look-ups switched on (eam_dev.h).
#include "eam_dev.h"

namespace vssr {

template <bool TYPED>
__global__ void k_eam_density(PotView V, vssr_eam_grid g, EamTyped T, double *__restrict__ e_embed, double *__restrict__ fp) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!V.runs(i)) return;
    eam_density_atom<TYPED>(i, g, T, V.type, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, e_embed, fp);
}

template <bool TYPED>
__global__ void k_eam_force(PotView V, vssr_eam_grid g, EamTyped T, const double *__restrict__ e_embed, const double *__restrict__ fp,
                            double *__restrict__ e_atom, double *__restrict__ forces) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!V.runs(i)) return;
    eam_force_atom<TYPED>(i, g, T, V.type, V.atom_cfg, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, e_embed, fp, e_atom, forces);
}

template <bool TYPED>
__global__ void __launch_bounds__(VIR_THREADS)
k_eam_stress(PotView V, vssr_eam_grid g, EamTyped T, const double *__restrict__ fp, double *__restrict__ stress,
             double *__restrict__ stress_std) {
    __shared__ double red[6][VIR_THREADS];
    if (V.counters[2]) return;   // (uniform)
    eam_stress_chain<TYPED>(blockIdx.x, red, g, T, V.type, V.cfg_start, V.cell, V.wpos, V.row_start, V.edge, V.edge_S, fp, stress,
                            stress_std);
}

// LAMMPS PairEAM::interpolate(): rows 1..n, [6] = f_m, [5] = finite-difference slope, [4], [3] = cubic through (f, slope) of
// m and m + 1, [2..0] = the derivative's coefficients / delta.  Row 0 is unused.
void eam_build_spline(const double *f, int n, double delta, double *spl /*[n + 1][7]*/) {
    auto S = [&](int m, int k) -> double & { return spl[7 * (size_t)m + k]; };
    for (int k = 0; k < 7; ++k) S(0, k) = 0.0;
    for (int m = 1; m <= n; ++m) S(m, 6) = f[m - 1];
    S(1, 5) = S(2, 6) - S(1, 6);
    S(2, 5) = 0.5 * (S(3, 6) - S(1, 6));
    S(n - 1, 5) = 0.5 * (S(n, 6) - S(n - 2, 6));
    S(n, 5) = S(n, 6) - S(n - 1, 6);
    for (int m = 3; m <= n - 2; ++m) S(m, 5) = ((S(m - 2, 6) - S(m + 2, 6)) + 8.0 * (S(m + 1, 6) - S(m - 1, 6))) / 12.0;
    for (int m = 1; m <= n - 1; ++m) {
        S(m, 4) = 3.0 * (S(m + 1, 6) - S(m, 6)) - 2.0 * S(m, 5) - S(m + 1, 5);
        S(m, 3) = S(m, 5) + S(m + 1, 5) - 2.0 * (S(m + 1, 6) - S(m, 6));
    }
    S(n, 4) = 0.0;
    S(n, 3) = 0.0;
    for (int m = 1; m <= n; ++m) {
        S(m, 2) = S(m, 5) / delta;
        S(m, 1) = 2.0 * S(m, 4) / delta;
        S(m, 0) = 3.0 * S(m, 3) / delta;
    }
}

int eam_stress(vssr_handle *h) {
    if (h->eam_adp) return adp_stress(h);
    if (h->d_stress.ensure(sizeof(double) * 12 * (size_t)h->n_cfg)) return set_err(h, VSSR_E_NOMEM, "out of device memory (stress)");
    double *out = h->d_stress.as<double>();
    hipLaunchKernelGGL(h->eam_nel > 0 ? k_eam_stress<true> : k_eam_stress<false>, dim3(h->n_cfg), dim3(VIR_THREADS), 0, h->stream,
                       pot_view(h), h->eam_grid, eam_tables(h), EamAtoms::of(h).fp, out, out + 6 * (size_t)h->n_cfg);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

int eam_run(vssr_handle *h, uint32_t want) {
    if (h->eam_adp) return adp_run(h, want);
    int rc = analytic_begin(h, h->eam_grid.cutoff, EamAtoms::doubles, "EAM");
    if (rc) return rc;
    const PotView V = pot_view(h);
    const EamAtoms S = EamAtoms::of(h);
    const EamTyped T = eam_tables(h);
    const bool typed = h->eam_nel > 0;   // (a funcfl handle never takes the typed kernels: 2.6 .. 3.4 % slower on pure Cu, profiles/r10/NOTES_eam_alloy.md)
    dim3 blk(64), grd((V.n_atoms + 63) / 64);
    hipLaunchKernelGGL(typed ? k_eam_density<true> : k_eam_density<false>, grd, blk, 0, h->stream, V, h->eam_grid, T, S.e_embed, S.fp);
    hipLaunchKernelGGL(typed ? k_eam_force<true> : k_eam_force<false>, grd, blk, 0, h->stream, V, h->eam_grid, T, S.e_embed, S.fp,
                       h->d_pot_ea.as<double>(), h->d_pot_f.as<double>());
    return analytic_end(h, V);
}

}  // namespace vssr
