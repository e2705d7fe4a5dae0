// pot_common.hip — the host and device code every fp64 analytic potential runs (declared in pot_dev.h): the batch view, the steps in
// front of and behind a potential's own kernels, the chain-energy kernel, and the virial kernel of the potentials that keep per-slot
// gradients (Tersoff, Stillinger-Weber, pair).
#include "pot_dev.h"
#include "virial_dev.h"

namespace vssr {

PotView pot_view(const vssr_handle *h) {
    return PotView{h->n_atoms, h->n_cfg, h->n_types, h->d_Z.as<int>(), h->d_atom_cfg.as<int>(), h->d_cfg_start.as<int>(),
                   h->d_cell.as<double>(), h->d_wpos.as<double>(), h->d_row_start.as<int>(), h->d_edge.as<float4>(),
                   h->d_edge_S.as<int>(), h->d_rev.as<int>(), h->d_counters.as<int>(),
                   ActiveView{h->active_mask, h->d_atom_cfg.as<int>()}};
}

__global__ void __launch_bounds__(256) k_chain_energy(PotView V, const double *__restrict__ e_atom, double *__restrict__ energy) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    if (!V.act.chain(b)) return;
    chain_energy(b, red, V.cfg_start, e_atom, energy);
}

// W_ab of chain b = sum over the chain's slots of G_a r_b, G_slot = dE_i / d r_ij as the last evaluation left it (every slot of a row is
// written, padding slots as zeros), r rebuilt in fp64 as the site kernels build it (virial_dev.h)
__device__ __forceinline__ void slot_stress_chain(int b, double (*red)[VIR_THREADS], const int *__restrict__ cfg_start,
                                                  const int *__restrict__ row_start, const float4 *__restrict__ edge,
                                                  const int *__restrict__ edge_S, const double *__restrict__ cell,
                                                  const double *__restrict__ wpos, const double *__restrict__ gslot,
                                                  double *__restrict__ stress, double *__restrict__ stress_std) {
    const int q = threadIdx.x % VIR_LANES;
    const double *C = cell + 9 * (size_t)b;
    double w[6] = {0, 0, 0, 0, 0, 0};
    for (int i = cfg_start[b] + threadIdx.x / VIR_LANES; i < cfg_start[b + 1]; i += VIR_THREADS / VIR_LANES)
        for (int e = row_start[i] + q; e < row_start[i + 1]; e += VIR_LANES) {
            const int j = __float_as_int(edge[e].w);
            if (j < 0) continue;   // padding slot
            double r[3];
            edge_vec(wpos, C, i, j, edge_S[e], r);
            virial_add(w, gslot[3 * (size_t)e], gslot[3 * (size_t)e + 1], gslot[3 * (size_t)e + 2], r[0], r[1], r[2]);
        }
    virial_reduce_store(red, w, 1.0, b, cell, stress, stress_std);
}

__global__ void __launch_bounds__(VIR_THREADS)
k_slot_stress(PotView V, const double *__restrict__ gslot, double *__restrict__ stress, double *__restrict__ stress_std) {
    __shared__ double red[6][VIR_THREADS];
    if (V.counters[2]) return;   // (uniform)
    slot_stress_chain(blockIdx.x, red, V.cfg_start, V.row_start, V.edge, V.edge_S, V.cell, V.wpos, gslot, stress, stress_std);
}

int slot_stress(vssr_handle *h, const double *gslot) {
    if (h->d_stress.ensure(sizeof(double) * 12 * (size_t)h->n_cfg)) return set_err(h, VSSR_E_NOMEM, "out of device memory (stress)");
    double *out = h->d_stress.as<double>();
    hipLaunchKernelGGL(k_slot_stress, dim3(h->n_cfg), dim3(VIR_THREADS), 0, h->stream, pot_view(h), gslot, out, out + 6 * (size_t)h->n_cfg);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

int analytic_begin(vssr_handle *h, double cutoff, size_t (*scratch)(const vssr_handle *), const char *what) {
    int rc = build_neighbors(h, cutoff);
    if (rc) return rc;
    const size_t N = h->n_atoms;
    if (h->d_pot_e.ensure(sizeof(double) * h->n_cfg) || h->d_pot_ea.ensure(sizeof(double) * N) || h->d_pot_f.ensure(sizeof(double) * 3 * N) ||
        (scratch && h->d_gbar.ensure(sizeof(double) * scratch(h))))
        return set_err(h, VSSR_E_NOMEM, "%s buffers: out of device memory", what);
    h->prof.begin(KC_ANALYTIC, h->stream);
    return VSSR_OK;
}

int analytic_end(vssr_handle *h, const PotView &V) {
    hipLaunchKernelGGL(k_chain_energy, dim3(h->n_cfg), dim3(256), 0, h->stream, V, h->d_pot_ea.as<double>(), h->d_pot_e.as<double>());
    h->prof.end(h->stream);
    VSSR_HIP(h, hipGetLastError());
    return VSSR_OK;
}

}  // namespace vssr
