// cell_dev.h -- what a cell needs before the neighbor search can use it: the inverse by the adjugate and, per periodic axis, the image
// count floor(cutoff / height) + 1.  One definition for vssr_batch_upload (host) and for the driver kernel that changes a chain's
// cell between two evaluations (relax_cell.hip), so both write the same numbers (the library is built with -ffp-contract=off).
// ok = false: periodic along some axis, but |det cell| < 1e-12 (inv and nimg stay zero).
#ifndef VSSR_CELL_DEV_H
#define VSSR_CELL_DEV_H
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace vssr {

__host__ __device__ inline void cell_setup(const double *cell, const uint8_t *pbc, double cutoff, double inv[9], int nimg[3], bool &ok) {
    const double *a = cell, *b = cell + 3, *c = cell + 6;
    double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
    double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    double vol = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2];
    ok = true;
    for (int x = 0; x < 9; ++x) inv[x] = 0.0;
    nimg[0] = nimg[1] = nimg[2] = 0;
    if (!(pbc[0] || pbc[1] || pbc[2])) return;
    if (fabs(vol) < 1e-12) { ok = false; return; }
    for (int x = 0; x < 3; ++x) { inv[x] = bc[x] / vol; inv[3 + x] = ca[x] / vol; inv[6 + x] = ab[x] / vol; }
    double hgt[3] = {fabs(vol) / sqrt(bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2]),
                     fabs(vol) / sqrt(ca[0] * ca[0] + ca[1] * ca[1] + ca[2] * ca[2]),
                     fabs(vol) / sqrt(ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2])};
    for (int k = 0; k < 3; ++k)
        if (pbc[k]) nimg[k] = (int)floor(cutoff / hgt[k]) + 1;
}

}  // namespace vssr
#endif
