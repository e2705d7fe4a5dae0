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

// The host side of it: the chain table to ch_d, the call's four flags cleared, the comparison into flags[2]; VSSR_E_BADARG with the
// caller's text where a group's chains differ.  Synchronises: host arrays the caller queued for upload before may leave scope after.
static int neb_compare_groups(vssr_handle *h, const std::vector<NebChain> &ch, NebChain *ch_d, int *flags, const char *differ_text) {
    hipStream_t st = h->stream;
    const int B = h->n_cfg;
    VSSR_HIP(h, hipMemcpyAsync(ch_d, ch.data(), sizeof(NebChain) * B, hipMemcpyHostToDevice, st));
    VSSR_HIP(h, hipMemsetAsync(flags, 0, sizeof(int) * 4, st));
    int mismatch = 0;
    hipLaunchKernelGGL(k_neb_compare, dim3(B), dim3(256), 0, st, ch_d, h->d_cfg_start.as<int>(), h->d_Z.as<int>(),
                       h->d_cell.as<unsigned long long>(), h->d_pbc.as<unsigned char>(), flags + 2);
    VSSR_HIP(h, hipGetLastError());
    VSSR_HIP(h, hipMemcpyAsync(&mismatch, flags + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    VSSR_HIP(h, hipStreamSynchronize(st));   // (nothing has moved yet)
    return mismatch ? set_err(h, VSSR_E_BADARG, "%s", differ_text) : (int)VSSR_OK;
}

}  // namespace vssr
#endif
