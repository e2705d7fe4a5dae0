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
// every pair is seen from both ends, so there is no scatter and no atomics.
#include "virial_dev.h"

namespace vssr {

// spline row m (1-based like LAMMPS): [0..2] derivative coefficients, [3..6] value coefficients
__device__ inline void eam_eval(const double *__restrict__ spl, int n, double x, double rd, bool clamp_lo, double &val,
                                double &der) {
    double p = x * rd + 1.0;
    int m = (int)p;
    m = clamp_lo ? max(1, min(m, n - 1)) : min(m, n - 1);
    p -= m;
    p = fmin(p, 1.0);
    const double *c = spl + 7 * (size_t)m;
    val = ((c[3] * p + c[4]) * p + c[5]) * p + c[6];
    der = (c[0] * p + c[1]) * p + c[2];
}

__device__ inline void eam_edge(const double *__restrict__ wpos, const double *C, int i, int j, int packedS, double r[3]) {
    int s0 = (packedS & 255) - 128, s1 = ((packedS >> 8) & 255) - 128, s2 = ((packedS >> 16) & 255) - 128;
    for (int x = 0; x < 3; ++x)
        r[x] = wpos[3 * j + x] - wpos[3 * i + x] + s0 * C[x] + s1 * C[3 + x] + s2 * C[6 + x];
}

__global__ void k_eam_density(int N, vssr_eam_grid g, const double *__restrict__ frho, const double *__restrict__ rhor,
                              const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                              const double *__restrict__ wpos, const int *__restrict__ row_start,
                              const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                              const int *__restrict__ counters, double *__restrict__ e_embed, double *__restrict__ fp,
                              ActiveView av) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || counters[2] || !av.atom(i)) return;
    const double *C = cell + 9 * atom_cfg[i];
    double rho = 0.0;
    for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
        const int j = __float_as_int(edge[e].w);
        if (j < 0) continue;
        double r[3];
        eam_edge(wpos, C, i, j, edge_S[e], r);
        const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (d >= g.cutoff) continue;
        double v, dv;
        eam_eval(rhor, g.nr, d, 1.0 / g.dr, false, v, dv);
        rho += v;
    }
    double F, dF;
    eam_eval(frho, g.nrho, rho, 1.0 / g.drho, true, F, dF);
    const double rhomax = (g.nrho - 1) * g.drho;
    if (rho > rhomax) F += dF * (rho - rhomax);   // linear continuation beyond the table (pair_eam.cpp)
    e_embed[i] = F;
    fp[i] = dF;
}

__global__ void k_eam_force(int N, vssr_eam_grid g, const double *__restrict__ rhor, const double *__restrict__ z2r,
                            const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                            const double *__restrict__ wpos, const int *__restrict__ row_start,
                            const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                            const int *__restrict__ counters, const double *__restrict__ e_embed,
                            const double *__restrict__ fp, double *__restrict__ e_atom, double *__restrict__ forces,
                            ActiveView av) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || counters[2] || !av.atom(i)) return;
    const double *C = cell + 9 * atom_cfg[i];
    const double fpi = fp[i];
    double ea = e_embed[i], f0 = 0.0, f1 = 0.0, f2 = 0.0;
    for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
        const int j = __float_as_int(edge[e].w);
        if (j < 0) continue;
        double r[3];
        eam_edge(wpos, C, i, j, edge_S[e], r);
        const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (d >= g.cutoff) continue;
        double rh, drh, z, dz;
        eam_eval(rhor, g.nr, d, 1.0 / g.dr, false, rh, drh);
        eam_eval(z2r, g.nr, d, 1.0 / g.dr, false, z, dz);
        const double recip = 1.0 / d;
        const double phi = z * recip;
        const double phip = dz * recip - phi * recip;
        const double psip = (fpi + fp[j]) * drh + phip;     // dE / d r of this pair, seen from centre i
        ea += 0.5 * phi;
        const double s = psip * recip;                      // force on i = + psip * r_hat (r points from i to j)
        f0 += s * r[0]; f1 += s * r[1]; f2 += s * r[2];
    }
    e_atom[i] = ea;
    forces[3 * i] = f0; forces[3 * i + 1] = f1; forces[3 * i + 2] = f2;
}

__global__ void __launch_bounds__(256)
k_eam_energy(const int *__restrict__ cfg_start, const double *__restrict__ e_atom, double *__restrict__ energy,
             const unsigned char *__restrict__ active) {
    __shared__ double red[256];
    int b = blockIdx.x, tid = threadIdx.x;
    if (active && !active[b]) return;
    double acc = 0.0;
    for (int i = cfg_start[b] + tid; i < cfg_start[b + 1]; i += blockDim.x) acc += e_atom[i];
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) energy[b] = red[0];
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

// ---- several elements (pair_style eam/alloy, eam/fs, funcfl files mixed per type) ----------------------------------------------
// Tables (vssr_eam_create_alloy): F_t [n][nrho + 1][7] | rho [n or n * n][nr + 1][7] | r phi [n (n + 1) / 2][nr + 1][7].
// rho index of the density an atom of type a contributes at a site of type b: a (alloy) or a * n + b (fs); r phi of the pair
// (a, b) at max(a,b) (max(a,b) + 1) / 2 + min(a,b).  The element of a neighbour comes from the resident type array.
struct EamTyped {
    const double *frho, *rhor, *z2r;
    int n, fs;
    size_t sF, sR;   // doubles per F row set / per r-table
    __device__ const double *rho_tab(int from, int at) const { return rhor + sR * (size_t)(fs ? from * n + at : from); }
    __device__ const double *z2r_tab(int a, int b) const {
        const int hi = max(a, b), lo = min(a, b);
        return z2r + sR * (size_t)(hi * (hi + 1) / 2 + lo);
    }
};

__global__ void k_eam_density_typed(int N, vssr_eam_grid g, EamTyped T, const int *__restrict__ type,
                                    const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                                    const double *__restrict__ wpos, const int *__restrict__ row_start,
                                    const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                                    const int *__restrict__ counters, double *__restrict__ e_embed, double *__restrict__ fp,
                                    ActiveView av) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || counters[2] || !av.atom(i)) return;
    const double *C = cell + 9 * atom_cfg[i];
    const int ti = type[i];
    double rho = 0.0;
    for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
        const int j = __float_as_int(edge[e].w);
        if (j < 0) continue;
        double r[3];
        eam_edge(wpos, C, i, j, edge_S[e], r);
        const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (d >= g.cutoff) continue;
        double v, dv;
        eam_eval(T.rho_tab(type[j], ti), g.nr, d, 1.0 / g.dr, false, v, dv);
        rho += v;
    }
    double F, dF;
    eam_eval(T.frho + T.sF * ti, g.nrho, rho, 1.0 / g.drho, true, F, dF);
    const double rhomax = (g.nrho - 1) * g.drho;
    if (rho > rhomax) F += dF * (rho - rhomax);
    e_embed[i] = F;
    fp[i] = dF;
}

__global__ void k_eam_force_typed(int N, vssr_eam_grid g, EamTyped T, const int *__restrict__ type,
                                  const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                                  const double *__restrict__ wpos, const int *__restrict__ row_start,
                                  const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                                  const int *__restrict__ counters, const double *__restrict__ e_embed,
                                  const double *__restrict__ fp, double *__restrict__ e_atom, double *__restrict__ forces,
                                  ActiveView av) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || counters[2] || !av.atom(i)) return;
    const double *C = cell + 9 * atom_cfg[i];
    const int ti = type[i];
    const double fpi = fp[i];
    double ea = e_embed[i], f0 = 0.0, f1 = 0.0, f2 = 0.0;
    for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
        const int j = __float_as_int(edge[e].w);
        if (j < 0) continue;
        double r[3];
        eam_edge(wpos, C, i, j, edge_S[e], r);
        const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (d >= g.cutoff) continue;
        const int tj = type[j];
        double rh, drh_ji, z, dz;
        eam_eval(T.rho_tab(tj, ti), g.nr, d, 1.0 / g.dr, false, rh, drh_ji);   // rho of j at i
        eam_eval(T.z2r_tab(ti, tj), g.nr, d, 1.0 / g.dr, false, z, dz);
        double dE;
        if (ti == tj) {   // one density table serves both directions
            dE = (fpi + fp[j]) * drh_ji;
        } else {
            double rh2, drh_ij;
            eam_eval(T.rho_tab(ti, tj), g.nr, d, 1.0 / g.dr, false, rh2, drh_ij);   // rho of i at j
            dE = fpi * drh_ji + fp[j] * drh_ij;
        }
        const double recip = 1.0 / d;
        const double phi = z * recip;
        const double phip = dz * recip - phi * recip;
        const double psip = dE + phip;
        ea += 0.5 * phi;
        const double s = psip * recip;
        f0 += s * r[0]; f1 += s * r[1]; f2 += s * r[2];
    }
    e_atom[i] = ea;
    forces[3 * i] = f0; forces[3 * i + 1] = f1; forces[3 * i + 2] = f2;
}

// ---- virial stress (vssr_batch_stress) ---------------------------------------------------------------------------------------
// There are no per-slot gradients to read: every directed edge recomputes psip = dE / d r of its pair exactly as the force kernels do,
// from the F'(rho) of the last run (fp: the linear continuation of F beyond the table is inside it), and W_ab = 1/2 sum over the
// directed edges of psip r_a r_b / d -- every pair is seen from both ends.  Lane layout and reduction: virial_dev.h.
__global__ void __launch_bounds__(VIR_THREADS)
k_eam_stress(vssr_eam_grid g, const double *__restrict__ rhor, const double *__restrict__ z2r, const int *__restrict__ cfg_start,
             const double *__restrict__ cell, const double *__restrict__ wpos, const int *__restrict__ row_start,
             const float4 *__restrict__ edge, const int *__restrict__ edge_S, const int *__restrict__ counters,
             const double *__restrict__ fp, double *__restrict__ stress, double *__restrict__ stress_std) {
    __shared__ double red[6][VIR_THREADS];
    const int b = blockIdx.x, q = threadIdx.x % VIR_LANES;
    if (counters[2]) return;   // (uniform)
    const double *C = cell + 9 * (size_t)b;
    double w[6] = {0, 0, 0, 0, 0, 0};
    for (int i = cfg_start[b] + threadIdx.x / VIR_LANES; i < cfg_start[b + 1]; i += VIR_THREADS / VIR_LANES) {
        const double fpi = fp[i];
        for (int e = row_start[i] + q; e < row_start[i + 1]; e += VIR_LANES) {
            const int j = __float_as_int(edge[e].w);
            if (j < 0) continue;
            double r[3];
            eam_edge(wpos, C, i, j, edge_S[e], r);
            const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            if (d >= g.cutoff) continue;
            double rh, drh, z, dz;
            eam_eval(rhor, g.nr, d, 1.0 / g.dr, false, rh, drh);
            eam_eval(z2r, g.nr, d, 1.0 / g.dr, false, z, dz);
            const double recip = 1.0 / d;
            const double phi = z * recip;
            const double phip = dz * recip - phi * recip;
            const double psip = (fpi + fp[j]) * drh + phip;
            const double s = psip * recip;
            virial_add(w, s * r[0], s * r[1], s * r[2], r[0], r[1], r[2]);
        }
    }
    virial_reduce_store(red, w, 0.5, b, cell, stress, stress_std);
}

__global__ void __launch_bounds__(VIR_THREADS)
k_eam_stress_typed(vssr_eam_grid g, EamTyped T, const int *__restrict__ type, const int *__restrict__ cfg_start,
                   const double *__restrict__ cell, const double *__restrict__ wpos, const int *__restrict__ row_start,
                   const float4 *__restrict__ edge, const int *__restrict__ edge_S, const int *__restrict__ counters,
                   const double *__restrict__ fp, double *__restrict__ stress, double *__restrict__ stress_std) {
    __shared__ double red[6][VIR_THREADS];
    const int b = blockIdx.x, q = threadIdx.x % VIR_LANES;
    if (counters[2]) return;   // (uniform)
    const double *C = cell + 9 * (size_t)b;
    double w[6] = {0, 0, 0, 0, 0, 0};
    for (int i = cfg_start[b] + threadIdx.x / VIR_LANES; i < cfg_start[b + 1]; i += VIR_THREADS / VIR_LANES) {
        const int ti = type[i];
        const double fpi = fp[i];
        for (int e = row_start[i] + q; e < row_start[i + 1]; e += VIR_LANES) {
            const int j = __float_as_int(edge[e].w);
            if (j < 0) continue;
            double r[3];
            eam_edge(wpos, C, i, j, edge_S[e], r);
            const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            if (d >= g.cutoff) continue;
            const int tj = type[j];
            double rh, drh_ji, z, dz;
            eam_eval(T.rho_tab(tj, ti), g.nr, d, 1.0 / g.dr, false, rh, drh_ji);   // rho of j at i
            eam_eval(T.z2r_tab(ti, tj), g.nr, d, 1.0 / g.dr, false, z, dz);
            double dE;
            if (ti == tj) {
                dE = (fpi + fp[j]) * drh_ji;
            } else {
                double rh2, drh_ij;
                eam_eval(T.rho_tab(ti, tj), g.nr, d, 1.0 / g.dr, false, rh2, drh_ij);   // rho of i at j
                dE = fpi * drh_ji + fp[j] * drh_ij;
            }
            const double recip = 1.0 / d;
            const double phi = z * recip;
            const double phip = dz * recip - phi * recip;
            const double psip = dE + phip;
            const double s = psip * recip;
            virial_add(w, s * r[0], s * r[1], s * r[2], r[0], r[1], r[2]);
        }
    }
    virial_reduce_store(red, w, 0.5, b, cell, stress, stress_std);
}

// the typed tables of a handle of several elements (layout: see EamTyped)
static EamTyped eam_typed_view(const vssr_handle *h) {
    const int n = h->eam_nel;
    const double *frho = h->pot_params.as<double>();
    return EamTyped{frho, frho + 7 * (size_t)(h->eam_grid.nrho + 1) * n,
                    frho + 7 * (size_t)(h->eam_grid.nrho + 1) * n + 7 * (size_t)(h->eam_grid.nr + 1) * (h->eam_fs ? n * n : n),
                    n, h->eam_fs, 7 * (size_t)(h->eam_grid.nrho + 1), 7 * (size_t)(h->eam_grid.nr + 1)};
}

int eam_stress(vssr_handle *h) {
    if (h->d_stress.ensure(sizeof(double) * 12 * (size_t)h->n_cfg)) return set_err(h, VSSR_E_NOMEM, "out of device memory (stress)");
    double *out = h->d_stress.as<double>(), *out_std = out + 6 * (size_t)h->n_cfg;
    const double *fp = h->d_gbar.as<double>() + h->n_atoms;   // e_embed | fp (eam_run)
    if (h->eam_nel > 0) {
        hipLaunchKernelGGL(k_eam_stress_typed, dim3(h->n_cfg), dim3(VIR_THREADS), 0, h->stream, h->eam_grid, eam_typed_view(h),
                           h->d_Z.as<int>(), h->d_cfg_start.as<int>(), h->d_cell.as<double>(), h->d_wpos.as<double>(),
                           h->d_row_start.as<int>(), h->d_edge.as<float4>(), h->d_edge_S.as<int>(), h->d_counters.as<int>(), fp, out,
                           out_std);
    } else {
        const double *rhor = h->pot_params.as<double>() + 7 * (size_t)(h->eam_grid.nrho + 1);
        const double *z2r = rhor + 7 * (size_t)(h->eam_grid.nr + 1);
        hipLaunchKernelGGL(k_eam_stress, dim3(h->n_cfg), dim3(VIR_THREADS), 0, h->stream, h->eam_grid, rhor, z2r, h->d_cfg_start.as<int>(),
                           h->d_cell.as<double>(), h->d_wpos.as<double>(), h->d_row_start.as<int>(), h->d_edge.as<float4>(),
                           h->d_edge_S.as<int>(), h->d_counters.as<int>(), fp, out, out_std);
    }
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

int eam_run(vssr_handle *h, uint32_t want) {
    (void)want;
    const int N = h->n_atoms;
    hipStream_t st = h->stream;
    int rc = build_neighbors(h, h->eam_grid.cutoff);
    if (rc) return rc;
    if (h->d_pot_e.ensure(sizeof(double) * h->n_cfg) || h->d_pot_ea.ensure(sizeof(double) * N) ||
        h->d_pot_f.ensure(sizeof(double) * 3 * N) || h->d_gbar.ensure(sizeof(double) * 2 * (size_t)N))
        return set_err(h, VSSR_E_NOMEM, "EAM buffers: out of device memory");
    double *e_embed = h->d_gbar.as<double>(), *fp = e_embed + N;
    const double *frho = h->pot_params.as<double>();
    const double *rhor = frho + 7 * (size_t)(h->eam_grid.nrho + 1);
    const double *z2r = rhor + 7 * (size_t)(h->eam_grid.nr + 1);
    h->prof.begin(KC_ANALYTIC, st);
    dim3 blk(64), grd((N + 63) / 64);
    const ActiveView av{h->active_mask, h->d_atom_cfg.as<int>()};
    if (h->eam_nel > 0) {
        const EamTyped T = eam_typed_view(h);
        hipLaunchKernelGGL(k_eam_density_typed, grd, blk, 0, st, N, h->eam_grid, T, h->d_Z.as<int>(), h->d_atom_cfg.as<int>(),
                           h->d_cell.as<double>(), h->d_wpos.as<double>(), h->d_row_start.as<int>(), h->d_edge.as<float4>(),
                           h->d_edge_S.as<int>(), h->d_counters.as<int>(), e_embed, fp, av);
        hipLaunchKernelGGL(k_eam_force_typed, grd, blk, 0, st, N, h->eam_grid, T, h->d_Z.as<int>(), h->d_atom_cfg.as<int>(),
                           h->d_cell.as<double>(), h->d_wpos.as<double>(), h->d_row_start.as<int>(), h->d_edge.as<float4>(),
                           h->d_edge_S.as<int>(), h->d_counters.as<int>(), e_embed, fp, h->d_pot_ea.as<double>(),
                           h->d_pot_f.as<double>(), av);
        hipLaunchKernelGGL(k_eam_energy, dim3(h->n_cfg), dim3(256), 0, st, h->d_cfg_start.as<int>(),
                           h->d_pot_ea.as<double>(), h->d_pot_e.as<double>(), h->active_mask);
        h->prof.end(st);
        VSSR_HIP(h, hipGetLastError());
        return VSSR_OK;
    }
    hipLaunchKernelGGL(k_eam_density, grd, blk, 0, st, N, h->eam_grid, frho, rhor, h->d_atom_cfg.as<int>(),
                       h->d_cell.as<double>(), h->d_wpos.as<double>(), h->d_row_start.as<int>(), h->d_edge.as<float4>(),
                       h->d_edge_S.as<int>(), h->d_counters.as<int>(), e_embed, fp, av);
    hipLaunchKernelGGL(k_eam_force, grd, blk, 0, st, N, h->eam_grid, rhor, z2r, h->d_atom_cfg.as<int>(),
                       h->d_cell.as<double>(), h->d_wpos.as<double>(), h->d_row_start.as<int>(), h->d_edge.as<float4>(),
                       h->d_edge_S.as<int>(), h->d_counters.as<int>(), e_embed, fp, h->d_pot_ea.as<double>(),
                       h->d_pot_f.as<double>(), av);
    hipLaunchKernelGGL(k_eam_energy, dim3(h->n_cfg), dim3(256), 0, st, h->d_cfg_start.as<int>(),
                       h->d_pot_ea.as<double>(), h->d_pot_e.as<double>(), h->active_mask);
    h->prof.end(st);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
