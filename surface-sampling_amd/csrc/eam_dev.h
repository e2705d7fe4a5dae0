// eam_dev.h — device bodies of the embedded-atom kernels (eam.hip): spline evaluation, the table view, and one body each for the
// density, force and stress kernels.  TYPED = false is the single funcfl element: no type look-ups, table 0 everywhere, one density
// table for both directions of a pair; TYPED = true reads the resident type array (eam/alloy, eam/fs, mixed funcfl).
#ifndef VSSR_EAM_DEV_H
#define VSSR_EAM_DEV_H
#include "pot_dev.h"
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

// Tables (vssr_eam_create_alloy): F_t [n][nrho + 1][7] | rho [n or n * n][nr + 1][7] | r phi [n (n + 1) / 2][nr + 1][7]; the funcfl
// handle's frho | rhor | z2r is this layout with n = 1, fs = 0.
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

// pass 1, centre i: rho_i, then F(rho_i) and F'(rho_i)
template <bool TYPED>
__device__ __forceinline__ void eam_density_atom(int i, const vssr_eam_grid &g, const EamTyped &T, const int *__restrict__ type,
                                                 const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                                                 const double *__restrict__ wpos, const int *__restrict__ row_start,
                                                 const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                                                 double *__restrict__ e_embed, double *__restrict__ fp) {
    const double *C = cell + 9 * atom_cfg[i];
    const int ti = TYPED ? type[i] : 0;
    double rho = 0.0;
    for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
        const int j = __float_as_int(edge[e].w);
        if (j < 0) continue;
        double r[3];
        edge_vec(wpos, C, i, j, edge_S[e], r);
        const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (d >= g.cutoff) continue;
        double v, dv;
        eam_eval(T.rho_tab(TYPED ? type[j] : 0, ti), g.nr, d, 1.0 / g.dr, false, v, dv);
        rho += v;
    }
    double F, dF;
    eam_eval(T.frho + T.sF * ti, g.nrho, rho, 1.0 / g.drho, true, F, dF);
    const double rhomax = (g.nrho - 1) * g.drho;
    if (rho > rhomax) F += dF * (rho - rhomax);   // linear continuation beyond the table (pair_eam.cpp)
    e_embed[i] = F;
    fp[i] = dF;
}

// One directed edge i -> j at distance d < cutoff (fp: F' of every atom): phi(d), and the return value psip / d with psip = dE / d r of the pair seen from
// centre i (the force on i is + psip r_hat, r pointing from i to j).  ONE expression for the force and the stress kernels.
template <bool TYPED>
__device__ __forceinline__ double eam_pair(const vssr_eam_grid &g, const EamTyped &T, int ti, int tj, double d, double fpi,
                                           const double *__restrict__ fp, int j, double &phi) {
    double rh, drh_ji, z, dz;
    eam_eval(T.rho_tab(tj, ti), g.nr, d, 1.0 / g.dr, false, rh, drh_ji);   // rho of j at i
    eam_eval(T.z2r_tab(ti, tj), g.nr, d, 1.0 / g.dr, false, z, dz);
    double dE;
    if (!TYPED || ti == tj) {   // one density table serves both directions
        dE = (fpi + fp[j]) * drh_ji;
    } else {
        double rh2, drh_ij;
        eam_eval(T.rho_tab(ti, tj), g.nr, d, 1.0 / g.dr, false, rh2, drh_ij);   // rho of i at j
        dE = fpi * drh_ji + fp[j] * drh_ij;
    }
    const double recip = 1.0 / d;
    phi = z * recip;
    const double phip = dz * recip - phi * recip;
    const double psip = dE + phip;
    return psip * recip;
}

// pass 2, centre i: pe/atom = F(rho_i) + 1/2 sum phi, force = sum psip r_hat
template <bool TYPED>
__device__ __forceinline__ void eam_force_atom(int i, const vssr_eam_grid &g, const EamTyped &T, const int *__restrict__ type,
                                               const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                                               const double *__restrict__ wpos, const int *__restrict__ row_start,
                                               const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                                               const double *__restrict__ e_embed, const double *__restrict__ fp,
                                               double *__restrict__ e_atom, double *__restrict__ forces) {
    const double *C = cell + 9 * atom_cfg[i];
    const int ti = TYPED ? type[i] : 0;
    const double fpi = fp[i];
    double ea = e_embed[i], f0 = 0.0, f1 = 0.0, f2 = 0.0;
    for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
        const int j = __float_as_int(edge[e].w);
        if (j < 0) continue;
        double r[3];
        edge_vec(wpos, C, i, j, edge_S[e], r);
        const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (d >= g.cutoff) continue;
        double phi;
        const double s = eam_pair<TYPED>(g, T, ti, TYPED ? type[j] : 0, d, fpi, fp, j, phi);
        ea += 0.5 * phi;
        f0 += s * r[0]; f1 += s * r[1]; f2 += s * r[2];
    }
    e_atom[i] = ea;
    forces[3 * i] = f0; forces[3 * i + 1] = f1; forces[3 * i + 2] = f2;
}

// Virial stress of chain b.  There are no per-slot gradients to read: every directed edge recomputes psip of its pair exactly as the
// force kernel does, from the F'(rho) of the last run (fp: the linear continuation of F beyond the table is inside it), and
// W_ab = 1/2 sum over the directed edges of psip r_a r_b / d -- every pair is seen from both ends.  Lane layout and reduction: virial_dev.h.
template <bool TYPED>
__device__ __forceinline__ void eam_stress_chain(int b, double (*red)[VIR_THREADS], const vssr_eam_grid &g, const EamTyped &T,
                                                 const int *__restrict__ type, const int *__restrict__ cfg_start,
                                                 const double *__restrict__ cell, const double *__restrict__ wpos,
                                                 const int *__restrict__ row_start, const float4 *__restrict__ edge,
                                                 const int *__restrict__ edge_S, const double *__restrict__ fp,
                                                 double *__restrict__ stress, double *__restrict__ stress_std) {
    const int q = threadIdx.x % VIR_LANES;
    const double *C = cell + 9 * (size_t)b;
    double w[6] = {0, 0, 0, 0, 0, 0};
    for (int i = cfg_start[b] + threadIdx.x / VIR_LANES; i < cfg_start[b + 1]; i += VIR_THREADS / VIR_LANES) {
        const int ti = TYPED ? type[i] : 0;
        const double fpi = fp[i];
        for (int e = row_start[i] + q; e < row_start[i + 1]; e += VIR_LANES) {
            const int j = __float_as_int(edge[e].w);
            if (j < 0) continue;
            double r[3];
            edge_vec(wpos, C, i, j, edge_S[e], r);
            const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            if (d >= g.cutoff) continue;
            double phi;
            const double s = eam_pair<TYPED>(g, T, ti, TYPED ? type[j] : 0, d, fpi, fp, j, phi);
            virial_add(w, s * r[0], s * r[1], s * r[2], r[0], r[1], r[2]);
        }
    }
    virial_reduce_store(red, w, 0.5, b, cell, stress, stress_std);
}

// the tables of a handle (layout: see EamTyped); a funcfl handle (eam_nel == 0) is one element
inline EamTyped eam_tables(const vssr_handle *h) {
    const int n = h->eam_nel > 0 ? h->eam_nel : 1;
    const size_t sF = 7 * (size_t)(h->eam_grid.nrho + 1), sR = 7 * (size_t)(h->eam_grid.nr + 1);
    const double *frho = h->pot_params.as<double>(), *rhor = frho + sF * n;
    return EamTyped{frho, rhor, rhor + sR * (h->eam_fs ? n * n : n), n, h->eam_fs, sF, sR};
}

// d_gbar of an EAM handle between the two passes and the virial kernel: F(rho) [atoms] | F'(rho) [atoms]
// (eam.hip and the chain-resident minimiser, chain_min.hip)
struct EamAtoms {
    double *e_embed, *fp;
    static size_t doubles(const vssr_handle *h) { return 2 * (size_t)h->n_atoms; }
    static EamAtoms of(const vssr_handle *h) {
        double *e_embed = h->d_gbar.as<double>();
        return {e_embed, e_embed + h->n_atoms};
    }
};

}  // namespace vssr
#endif
