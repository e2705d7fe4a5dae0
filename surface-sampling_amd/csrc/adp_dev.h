// adp_dev.h — device bodies of the angular-dependent potential kernels (adp.hip): the table view, the per-atom row, and one body
// each for the density, force and stress kernels.  ADP (Mishin, Mehl, Papaconstantopoulos 2005; LAMMPS pair_style adp) is
// eam/alloy plus a dipole and a quadrupole term per atom:
//   E = sum_i [ F(rho_i) + 1/2 mu_i.mu_i + 1/2 lambda_i:lambda_i - nu_i^2 / 6 ] + 1/2 sum_{i != j} phi(r_ij),
//   mu_i = sum_j u(r) r,  lambda_i = sum_j w(r) r (x) r,  nu_i = tr lambda_i,  r = x_j - x_i over the slots of the row.
// F, rho and r phi are the typed tables of eam_dev.h (always the typed bodies, alloy densities); u and w are two more r-tables per
// element pair on the same grid and spline, NOT scaled by r.
#ifndef VSSR_ADP_DEV_H
#define VSSR_ADP_DEV_H
#include "eam_dev.h"

namespace vssr {

// Tables (vssr_eam_create_adp): the EamTyped layout with fs = 0, followed by u [n (n + 1) / 2][nr + 1][7] | w [same], in the pair
// order of r phi.
struct AdpTyped {
    EamTyped T;
    __device__ const double *u_tab(int a, int b) const { return T.z2r_tab(a, b) + T.sR * (size_t)(T.n * (T.n + 1) / 2); }
    __device__ const double *w_tab(int a, int b) const { return T.z2r_tab(a, b) + T.sR * (size_t)(T.n * (T.n + 1)); }
};

// d_gbar of an ADP handle between the two passes and the virial kernel: one row of ADP_ROW doubles per atom,
// F | F' | mu x y z | lambda xx yy zz yz xz xy | 0 -- eleven values padded to twelve, so a row is six aligned 16-byte words.
constexpr int ADP_ROW = 12;

struct AdpRow {
    double v[ADP_ROW];
    __device__ __forceinline__ double F() const { return v[0]; }
    __device__ __forceinline__ const double *mu() const { return v + 2; }
    __device__ __forceinline__ const double *lam() const { return v + 5; }
    __device__ __forceinline__ double nu() const { return (v[5] + v[6]) + v[7]; }
};

__device__ __forceinline__ void adp_load_row(const double *__restrict__ rows, int i, AdpRow &R) {
    const double2 *p = reinterpret_cast<const double2 *>(rows) + (ADP_ROW / 2) * (size_t)i;
#pragma unroll
    for (int k = 0; k < ADP_ROW / 2; ++k) {
        const double2 x = p[k];
        R.v[2 * k] = x.x;
        R.v[2 * k + 1] = x.y;
    }
}

// pass 1, centre i: rho_i, mu_i, lambda_i in row order, then F(rho_i) and F'(rho_i); writes the atom's row
__device__ __forceinline__ void adp_density_atom(int i, const vssr_eam_grid &g, const AdpTyped &A, const int *__restrict__ type,
                                                 const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                                                 const double *__restrict__ wpos, const int *__restrict__ row_start,
                                                 const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                                                 double *__restrict__ rows) {
    const double *C = cell + 9 * atom_cfg[i];
    const int ti = type[i];
    const double rd = 1.0 / g.dr;
    double rho = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, lxx = 0.0, lyy = 0.0, lzz = 0.0, lyz = 0.0, lxz = 0.0, lxy = 0.0;
    for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
        const int j = __float_as_int(edge[e].w);
        if (j < 0) continue;
        double r[3];
        edge_vec(wpos, C, i, j, edge_S[e], r);
        const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (d >= g.cutoff) continue;
        const int tj = type[j];
        double v, dv, u, w;
        eam_eval(A.T.rho_tab(tj, ti), g.nr, d, rd, false, v, dv);
        eam_eval(A.u_tab(ti, tj), g.nr, d, rd, false, u, dv);
        eam_eval(A.w_tab(ti, tj), g.nr, d, rd, false, w, dv);
        rho += v;
        m0 += u * r[0]; m1 += u * r[1]; m2 += u * r[2];
        lxx += w * r[0] * r[0]; lyy += w * r[1] * r[1]; lzz += w * r[2] * r[2];
        lyz += w * r[1] * r[2]; lxz += w * r[0] * r[2]; lxy += w * r[0] * r[1];
    }
    double F, dF;
    eam_eval(A.T.frho + A.T.sF * ti, g.nrho, rho, 1.0 / g.drho, true, F, dF);
    const double rhomax = (g.nrho - 1) * g.drho;
    if (rho > rhomax) F += dF * (rho - rhomax);   // linear continuation beyond the table, as eam_density_atom
    double2 *p = reinterpret_cast<double2 *>(rows) + (ADP_ROW / 2) * (size_t)i;
    p[0] = make_double2(F, dF);
    p[1] = make_double2(m0, m1);
    p[2] = make_double2(m2, lxx);
    p[3] = make_double2(lyy, lzz);
    p[4] = make_double2(lyz, lxz);
    p[5] = make_double2(lxy, 0.0);
}

// One directed edge i -> j (r = x_j - x_i, |r| = d < cutoff), Ri / Rj the rows of the two atoms: phi(d), and G = dE / d r of the
// pair seen from centre i (the force on i is + G).  The EAM part is eam_pair's psip r_hat; the angular part is not central:
//   u (mu_i - mu_j) + u' ((mu_i - mu_j).r) r_hat + w' (r^T L r) r_hat + 2 w L r - (nu_i + nu_j) / 3 (w' d^2 r_hat + 2 w r),
// L = lambda_i + lambda_j.  ONE expression for the force and the stress kernels.
__device__ __forceinline__ void adp_pair(const vssr_eam_grid &g, const AdpTyped &A, int ti, int tj, double d, const double r[3],
                                         const AdpRow &Ri, const AdpRow &Rj, double &phi, double G[3]) {
    const double s = eam_pair<true>(g, A.T, ti, tj, d, Ri.v[1], &Rj.v[1], 0, phi);
    double u, du, w, dw;
    eam_eval(A.u_tab(ti, tj), g.nr, d, 1.0 / g.dr, false, u, du);
    eam_eval(A.w_tab(ti, tj), g.nr, d, 1.0 / g.dr, false, w, dw);
    const double *mi = Ri.mu(), *mj = Rj.mu(), *li = Ri.lam(), *lj = Rj.lam();
    const double dm0 = mi[0] - mj[0], dm1 = mi[1] - mj[1], dm2 = mi[2] - mj[2];
    const double Lxx = li[0] + lj[0], Lyy = li[1] + lj[1], Lzz = li[2] + lj[2];
    const double Lyz = li[3] + lj[3], Lxz = li[4] + lj[4], Lxy = li[5] + lj[5];
    const double nu = Ri.nu() + Rj.nu();
    const double Lr0 = Lxx * r[0] + Lxy * r[1] + Lxz * r[2];
    const double Lr1 = Lxy * r[0] + Lyy * r[1] + Lyz * r[2];
    const double Lr2 = Lxz * r[0] + Lyz * r[1] + Lzz * r[2];
    const double dmr = dm0 * r[0] + dm1 * r[1] + dm2 * r[2];
    const double rLr = r[0] * Lr0 + r[1] * Lr1 + r[2] * Lr2;
    const double third = 1.0 / 3.0;
    // the coefficient of r: the EAM term, the three r_hat terms over d, and the trace term's 2 w r
    const double c = s + (du * dmr + dw * rLr - third * nu * dw * (d * d)) / d - 2.0 * third * nu * w;
    G[0] = c * r[0] + u * dm0 + 2.0 * w * Lr0;
    G[1] = c * r[1] + u * dm1 + 2.0 * w * Lr1;
    G[2] = c * r[2] + u * dm2 + 2.0 * w * Lr2;
}

// pass 2, centre i: pe/atom = F + 1/2 mu^2 + 1/2 lambda:lambda - nu^2 / 6 + 1/2 sum phi, force = sum G
__device__ __forceinline__ void adp_force_atom(int i, const vssr_eam_grid &g, const AdpTyped &A, const int *__restrict__ type,
                                               const int *__restrict__ atom_cfg, const double *__restrict__ cell,
                                               const double *__restrict__ wpos, const int *__restrict__ row_start,
                                               const float4 *__restrict__ edge, const int *__restrict__ edge_S,
                                               const double *__restrict__ rows, double *__restrict__ e_atom,
                                               double *__restrict__ forces) {
    const double *C = cell + 9 * atom_cfg[i];
    const int ti = type[i];
    AdpRow Ri;
    adp_load_row(rows, i, Ri);
    const double *m = Ri.mu(), *l = Ri.lam();
    const double nu = Ri.nu();
    double ea = Ri.F() + 0.5 * (m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) + 0.5 * (l[0] * l[0] + l[1] * l[1] + l[2] * l[2]) +
                (l[3] * l[3] + l[4] * l[4] + l[5] * l[5]) - nu * nu / 6.0;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    for (int e = row_start[i]; e < row_start[i + 1]; ++e) {
        const int j = __float_as_int(edge[e].w);
        if (j < 0) continue;
        double r[3];
        edge_vec(wpos, C, i, j, edge_S[e], r);
        const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (d >= g.cutoff) continue;
        AdpRow Rj;
        adp_load_row(rows, j, Rj);
        double phi, G[3];
        adp_pair(g, A, ti, type[j], d, r, Ri, Rj, phi, G);
        ea += 0.5 * phi;
        f0 += G[0]; f1 += G[1]; f2 += G[2];
    }
    e_atom[i] = ea;
    forces[3 * i] = f0; forces[3 * i + 1] = f1; forces[3 * i + 2] = f2;
}

// Virial stress of chain b: every directed edge recomputes G of its pair exactly as the force kernel does, from the rows of the last
// run, and W_ab = 1/2 sum over the directed edges of sym(G (x) r) -- every pair is seen from both ends (an atom and its own image:
// the edges r and -r).  Lane layout and reduction: virial_dev.h.
__device__ __forceinline__ void adp_stress_chain(int b, double (*red)[VIR_THREADS], const vssr_eam_grid &g, const AdpTyped &A,
                                                 const int *__restrict__ type, const int *__restrict__ cfg_start,
                                                 const double *__restrict__ cell, const double *__restrict__ wpos,
                                                 const int *__restrict__ row_start, const float4 *__restrict__ edge,
                                                 const int *__restrict__ edge_S, const double *__restrict__ rows,
                                                 double *__restrict__ stress, double *__restrict__ stress_std) {
    const int q = threadIdx.x % VIR_LANES;
    const double *C = cell + 9 * (size_t)b;
    double w[6] = {0, 0, 0, 0, 0, 0};
    for (int i = cfg_start[b] + threadIdx.x / VIR_LANES; i < cfg_start[b + 1]; i += VIR_THREADS / VIR_LANES) {
        const int ti = type[i];
        AdpRow Ri;
        adp_load_row(rows, i, Ri);
        for (int e = row_start[i] + q; e < row_start[i + 1]; e += VIR_LANES) {
            const int j = __float_as_int(edge[e].w);
            if (j < 0) continue;
            double r[3];
            edge_vec(wpos, C, i, j, edge_S[e], r);
            const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            if (d >= g.cutoff) continue;
            AdpRow Rj;
            adp_load_row(rows, j, Rj);
            double phi, G[3];
            adp_pair(g, A, ti, type[j], d, r, Ri, Rj, phi, G);
            virial_add(w, G[0], G[1], G[2], r[0], r[1], r[2]);
        }
    }
    virial_reduce_store(red, w, 0.5, b, cell, stress, stress_std);
}

// the rows of a handle in d_gbar
struct AdpAtoms {
    static size_t doubles(const vssr_handle *h) { return ADP_ROW * (size_t)h->n_atoms; }
    static double *of(const vssr_handle *h) { return h->d_gbar.as<double>(); }
};

}  // namespace vssr
#endif
