// virial_dev.h — device bodies of the virial-stress kernels of the fp64 analytic potentials (k_slot_stress in pot_common.hip for the
// Tersoff, Stillinger-Weber and pair handles, k_eam_stress in eam.hip): the lane layout and the reduction they share.
//
// Under a homogeneous strain every edge vector becomes (1 + eps) r, so W_ab = dE / d eps_ab is a sum over the chain's slots of
// (dE / d r)_a r_b; sigma = sym(W) / |det cell| (ASE's sign: tensile positive; the volume of the cell also for slabs), Voigt order
// xx yy zz yz xz xy, eV / A^3 -- the contract of the PaiNN k_stress (painn.hip).  One workgroup of 256 threads per chain: four lanes
// share a centre (its slots n = q, q + 4, ...), 64 centres per pass; six symmetrised fp64 partial sums per lane, then a binary tree
// in LDS.  No atomics: the order of every sum is fixed by the chain's own layout, so two calls return the same bits and a chain's
// result does not depend on what else is in the batch.
#ifndef VSSR_VIRIAL_DEV_H
#define VSSR_VIRIAL_DEV_H
#include "vssr_internal.h"

namespace vssr {

constexpr int VIR_THREADS = 256, VIR_LANES = 4;

// w += sym(g (x) r): xx yy zz yz xz xy
__device__ __forceinline__ void virial_add(double w[6], double gx, double gy, double gz, double rx, double ry, double rz) {
    w[0] += gx * rx;
    w[1] += gy * ry;
    w[2] += gz * rz;
    w[3] += 0.5 * (gy * rz + gz * ry);
    w[4] += 0.5 * (gx * rz + gz * rx);
    w[5] += 0.5 * (gx * ry + gy * rx);
}

// Every thread of the workgroup calls this with its partial sums: stress[b] = scale * (sum over the lanes) / |det cell_b|, and zeros
// for the spread over models (one model).  red: 6 x VIR_THREADS doubles.
__device__ __forceinline__ void virial_reduce_store(double (*red)[VIR_THREADS], const double w[6], double scale, int b,
                                                    const double *__restrict__ cell, double *__restrict__ stress,
                                                    double *__restrict__ stress_std) {
    const int tid = threadIdx.x;
    for (int k = 0; k < 6; ++k) red[k][tid] = w[k];
    __syncthreads();
    for (int s = VIR_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 6; ++k) red[k][tid] += red[k][tid + s];
        __syncthreads();
    }
    if (tid < 6) {
        const double *c = cell + 9 * (size_t)b;
        const double vol = fabs(c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]));
        stress[6 * (size_t)b + tid] = scale * red[tid][0] / vol;
        stress_std[6 * (size_t)b + tid] = 0.0;
    }
}

}  // namespace vssr
#endif
