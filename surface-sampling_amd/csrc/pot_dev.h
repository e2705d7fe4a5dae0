// pot_dev.h — what the fp64 analytic potentials (tersoff.hip, sw.hip, pair.hip, eam.hip) share: the view of the resident batch their
// kernels take, the edge vector, the chain-energy reduction, and the host steps around a run (pot_common.hip).
//
// Every kernel takes a PotView by value plus its own arguments (parameter table, scratch, outputs), unpacks the view and calls a
// __device__ body with __restrict__ pointer parameters: the compiler honours __restrict__ on parameters, not on struct members, so
// the arithmetic stays in those bodies (tersoff_dev.h, sw_dev.h, pair_dev.h, eam_dev.h) and a kernel is "unpack, call".
#ifndef VSSR_POT_DEV_H
#define VSSR_POT_DEV_H
#include "vssr_internal.h"

namespace vssr {

struct PotView {   // read-only view of the resident batch and its neighbor rows (padded CSR by centre, nbr.hip)
    int n_atoms, n_cfg, n_types;
    const int *type;         // [n_atoms] species index
    const int *atom_cfg;     // [n_atoms] chain of each atom
    const int *cfg_start;    // [n_cfg + 1]
    const double *cell;      // [n_cfg][9]
    const double *wpos;      // [n_atoms][3] wrapped positions
    const int *row_start;    // [n_atoms + 1]
    const float4 *edge;      // [slots] .w = bitcast(j), j < 0: padding slot
    const int *edge_S;       // [slots] packed image shifts
    const int *rev;          // [slots] slot of the reverse edge
    const int *counters;     // [2]: the neighbor build overflowed, nothing below it is valid
    ActiveView act;          // chains switched off by the relaxation driver
    // centre i of a one-thread-per-atom kernel is evaluated
    __device__ __forceinline__ bool runs(int i) const { return i < n_atoms && !counters[2] && act.atom(i); }
};
PotView pot_view(const vssr_handle *h);   // the only place that spells out the handle's buffers for these kernels

// Around the kernels of a potential's run.  analytic_begin: neighbor build, the result buffers d_pot_e / _ea / _f, `scratch(h)`
// doubles of d_gbar (nullptr: none; asked after the build, which may have grown slot_cap), then the profiler bracket opens;
// what: the potential's name in the out-of-memory message.  analytic_end: chain energies from d_pot_ea, bracket closes.
int analytic_begin(vssr_handle *h, double cutoff, size_t (*scratch)(const vssr_handle *), const char *what);
int analytic_end(vssr_handle *h, const PotView &V);
// vssr_batch_stress of the potentials that keep per-slot gradients G = dE_i / d r_ij (Tersoff, SW, pair): the virial kernel over gslot
int slot_stress(vssr_handle *h, const double *gslot);

__device__ inline void edge_vec(const double *__restrict__ wpos, const double *C, int i, int j, int packedS,
                                double r[3]) {
    int s0 = (packedS & 255) - 128, s1 = ((packedS >> 8) & 255) - 128, s2 = ((packedS >> 16) & 255) - 128;
    for (int x = 0; x < 3; ++x)
        r[x] = wpos[3 * j + x] - wpos[3 * i + x] + s0 * C[x] + s1 * C[3 + x] + s2 * C[6 + x];
}

// energy of chain b: 256 threads (strided partial sums, binary tree in LDS); red: 256 doubles
__device__ __forceinline__ void chain_energy(int b, double *red, const int *__restrict__ cfg_start, const double *__restrict__ e_atom,
                                             double *__restrict__ energy) {
    const int tid = threadIdx.x;
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

}  // namespace vssr
#endif
