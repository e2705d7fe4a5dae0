// ewald_dev.h — what the reciprocal-space kernels of a pair handle with k-space share (ewald.hip), and what the host needs of it
// (api_batch.hip sizes the S(k) array and refuses a chain over capacity with the same arithmetic the kernels run).
//
// The k set of a chain is a function of (g, k_cut) and the chain's own cell only: every k = h b1 + k b2 + l b3 with 0 < |k| <= k_cut.
// The kernels walk the half box h = 0 .. mx, k = -my .. my, l = -mz .. mz in the order idx = (h (2 my + 1) + k + my) (2 mz + 1) + l + mz,
// m_a = floor(k_cut |a_a| / 2 pi): h = k . a_1 / 2 pi, so |h| <= |k| |a_1| / 2 pi and no vector of the sphere lies outside the box.  A
// cell of the box outside the sphere or outside the half space (h > 0, or h = 0 and k > 0, or h = k = 0 and l > 0) carries zeros.
// Nothing per chain is stored between evaluations: bounds, reciprocal vectors and the cell count are rebuilt from d_cell by every
// workgroup, so a live-chain compaction (relax_cg.hip) has nothing of this to move.
//
// A slab handle (vssr_pair_create_kspace_slab, slab factor F > 1, chains with pbc 1 1 0): everything above is taken on the extended
// cell (a, b, F c) -- volume V' = F V, reciprocal vectors, bounds, cell count -- and ewald.hip adds the dipole correction of
// Yeh & Berkowitz from the moments Q = sum q, M = sum q z, R2 = sum q z^2 with z = r . n, n = a x b / |a x b|.
#ifndef VSSR_EWALD_DEV_H
#define VSSR_EWALD_DEV_H
#include "pot_dev.h"

namespace vssr {

constexpr int EW_MAX_INDEX = 63;        // largest per-axis index m_a (vssr_batch_upload refuses a chain beyond it: VSSR_E_CAPACITY)
constexpr int EW_MAX_CELLS = 65536;     // largest half box (mx + 1)(2 my + 1)(2 mz + 1) of a chain (same refusal)
constexpr int EW_KBLOCK = 256;          // k cells per workgroup of the structure-factor kernel; cells staged per round by the atom kernel
constexpr int EW_TAB = 736;             // phase-factor entries in LDS: with the 64 charges of a tile 12 288 B, the table of k_pair_site
constexpr int EW_TILE_MAX = 64;         // atoms per tile at the most: tile = min(64, EW_TAB / (mx + my + mz + 3)) >= 3
constexpr int EW_ATOMS = 64;            // atoms per workgroup of the atom kernel (one wave, one atom per lane)
constexpr double EW_2PI = 6.28318530717958647692;
constexpr double EW_SQRTPI = 1.77245385090551602730;

constexpr int EW_EXTRA = 2;             // double2 entries of a chain behind its k cells in the S(k) array: (Q, M) and (R2, 0)

struct EwaldParams {   // by value to every kernel
    double g, k_cut;
    double slab;       // slab factor F of the extended cell (a, b, F c); 0: a sum periodic in three directions
    double q[8];       // per-type charges (PAIR_MAX_TYPES)
};

struct EwaldGeom {
    double b[3][3];    // reciprocal vectors, 2 pi included: b[a] . a_c = 2 pi delta_ac
    double r[3][3];    // b / 2 pi: fractional coordinate s_a = x . r[a]
    double vol;        // |det cell| (a slab handle: of the extended cell, V' = F V)
    int m[3];          // per-axis bounds
    long long cells;   // (mx + 1)(2 my + 1)(2 mz + 1)
};

// slack: 0 on the device; the host adds 1e-9 to k_cut |a| / 2 pi before the floor, so its bounds are never below the device's.
// slab: 0, or the factor F of a slab handle: the geometry of the extended cell (a, b, F c).
__host__ __device__ inline void ewald_geom(const double *C, double k_cut, double slack, EwaldGeom &G, double slab = 0.0) {
    double ext[3] = {C[6], C[7], C[8]};
    if (slab > 0.0)
        for (int x = 0; x < 3; ++x) ext[x] *= slab;
    const double *a = C, *b = C + 3, *c = ext;
    const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
    const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double det = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2];
    for (int x = 0; x < 3; ++x) {
        G.r[0][x] = bc[x] / det; G.r[1][x] = ca[x] / det; G.r[2][x] = ab[x] / det;
        for (int k = 0; k < 3; ++k) G.b[k][x] = EW_2PI * G.r[k][x];
    }
    G.vol = det < 0 ? -det : det;
    for (int k = 0; k < 3; ++k) {
        const double *v = k == 2 ? ext : C + 3 * k;
        const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double x = k_cut * len / EW_2PI + slack;
        G.m[k] = x < 1e6 ? (int)x : 1000000;   // (x >= 0: the conversion is the floor)
    }
    G.cells = (long long)(G.m[0] + 1) * (2 * G.m[1] + 1) * (2 * G.m[2] + 1);
}

}  // namespace vssr
#endif
