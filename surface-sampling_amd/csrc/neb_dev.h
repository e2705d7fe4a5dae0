// neb_dev.h -- what neb.hip and dimer.hip share: the chain table of a group of chains that may differ in positions only (the images
// of a band, the two chains of a dimer) and the bitwise comparison of such chains on the device.
#ifndef VSSR_NEB_DEV_H
#define VSSR_NEB_DEV_H
#include "vssr_internal.h"

namespace vssr {

struct NebChain { int first, idx, nimg, band; };   // first chain of the band, image index within it, images, band

// Images: chain b of index > 0 against the first chain of its band, bit for bit (species, cell, pbc; atom counts and masks were
// compared on the host).  flag[0] = 1 on any difference.
static __global__ void __launch_bounds__(256)
k_neb_compare(const NebChain *__restrict__ ch, const int *__restrict__ cfg_start, const int *__restrict__ Z,
              const unsigned long long *__restrict__ cell, const unsigned char *__restrict__ pbc, int *__restrict__ flag) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const NebChain c = ch[b];
    if (c.idx == 0) return;
    const int f = c.first;
    const int a0 = cfg_start[b], nat = cfg_start[b + 1] - a0, f0 = cfg_start[f];
    bool diff = false;
    for (int i = tid; i < nat; i += 256) diff |= Z[a0 + i] != Z[f0 + i];
    if (tid < 9) diff |= cell[9 * (size_t)b + tid] != cell[9 * (size_t)f + tid];
    if (tid < 3) diff |= pbc[3 * b + tid] != pbc[3 * f + tid];
    if (diff) flag[0] = 1;   // (same value from every writer)
}

}  // namespace vssr
#endif
