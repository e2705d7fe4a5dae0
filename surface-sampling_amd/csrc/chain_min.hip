// chain_min.hip — the chain-resident minimiser: ONE workgroup runs the whole LAMMPS-style CG relaxation of ONE chain.
//
// Replaces, for chains of <= 256 atoms on the fp64 potentials, the lock-step driver of relax_cg.hip (reference: `optimizer: "LAMMPS"`,
// LAMMMPSCalc.run_lammps_opt, mcmc/calculators/calculators.py:600-619 -> `min_style cg` / `minimize 1e-5 1e-5 {relax_steps} 10000`,
// tutorials/data/GaN_0001/GaN_0001_lammps_opt_template.txt; one relaxation per MC proposal, mcmc/system.py:450-470).
//
// Why: the GaN chains of BASELINE configs[1] have 48 atoms and stop after 21 .. 159 evaluations each (median 55).  In lock step
// every evaluation is ~12 dependent launches over the whole batch, each ~10 us of dispatch + drain whatever its size, and the
// batch runs until its slowest chain is done: 131 .. 161 lock-step evaluations per proposal, 2.2 .. 2.7 x the chain-evaluations
// the chains need (profiles/r05/NOTES_tersoff.md).  A 48-atom chain is a workgroup-sized problem: here a 256-thread workgroup
// owns a chain from its first evaluation to its stop criterion -- wrap, neighbor rows, site terms, force gather, energy,
// CG state machine -- with barriers instead of launches between the phases, and leaves when ITS chain is done; the hardware
// workgroup scheduler hands the CU to the next chain.  No lock step, no host polls, one launch per relaxation.
//
// One kernel template, k_cg_chain<Site>: the common phases are written once, a site policy per kind of handle -- TersoffSite, SwSite,
// EamSite<TYPED>, PairSite -- supplies the LDS struct, the scratch pointers in d_gbar and the per-evaluation phases of its potential,
// so an instantiation carries only its own LDS (gfx950 cross-compile, tools/kernel_regs.sh: Tersoff 55 304 B, SW 45 064 B, pair
// 15 368 B, EAM 3 080 B; two workgroups per CU at amdgpu_waves_per_eu(2, 2); profiles/r15/NOTES_chain_resident_kinds.md).  Which
// relaxations take this driver: chain_min_supported below (the handle's vssr_batch_relax_cg_driver setting, VSSR_CG_FUSED, the
// automatic rule for Tersoff).
//
// Same bits: every phase is the device function the lock-step kernels run (nbr_dev.h, tersoff_dev.h, sw_dev.h, eam_dev.h, pair_dev.h,
// cg_dev.h) with the same lane-to-work mapping (16 lanes per centre in the neighbor search, 4 lanes per centre in the site tiles, one
// thread per centre in the EAM passes and the gathers, 256-thread reductions), so rows, energies, forces, iteration / evaluation counts
// and stop reasons equal the lock-step driver's bit for bit (tests/test_cg.py::test_chain_resident_minimiser_equals_the_lock_step_driver,
// tests/test_cg_resident_kinds_gpu.py).  Only the slot numbering differs: a chain owns the fixed slot range
// [cfg_start[b], cfg_start[b + 1]) x cap_per_atom instead of a place in a batch-wide scan.
//
// The evaluation phase is the device function template cm_evaluate<Site>; a second kernel template, k_md_chain<Site>, puts the
// molecular-dynamics integrator of md_dev.h behind it instead of the CG state machine (further down; host side: chain_md).
#include <algorithm>
#include "arena.h"
#include "cg_dev.h"
#include "md_dev.h"
#include "nbr_dev.h"
#ifdef CM_PHASE_TIMING   // sub-phases of the site tile: slots 10 .. 12 of g_cm_phase
#include <hip/hip_runtime.h>
extern __device__ unsigned long long g_cm_phase[16];
#define TS_MARK_INIT unsigned long long ts_t = wall_clock64();
#define TS_MARK(k) { __syncthreads(); const unsigned long long ts_n = wall_clock64(); if (threadIdx.x == 0 && blockIdx.x == 0) g_cm_phase[10 + (k)] += ts_n - ts_t; ts_t = wall_clock64(); }
#endif
#include "tersoff_dev.h"
#include "sw_dev.h"
#include "eam_dev.h"
#include "pair_dev.h"

#include <vector>

#ifdef CM_PHASE_TIMING   // debug build only (tools/gpu_cm_phase.py): 100 MHz wall-clock ticks per phase, workgroup 0
__device__ unsigned long long g_cm_phase[16];
#define CMP_INIT unsigned long long cmp_t = wall_clock64();
#define CMP(k) { __syncthreads(); const unsigned long long cmp_n = wall_clock64(); if (threadIdx.x == 0 && blockIdx.x == 0) g_cm_phase[k] += cmp_n - cmp_t; cmp_t = wall_clock64(); }
extern "C" int vssr_debug_cm_phases(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cm_phase), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_cm_phase), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#else
#define CMP_INIT
#define CMP(k)
#endif

namespace vssr {

// What every instantiation of the kernel reads, in device memory (CmArgs<Site> below adds the site policy's own block).
struct CmCommon {
    // resident batch
    int n_types;
    const int *type, *atom_cfg, *cfg_start, *nimg;
    const double *cell, *invcell;
    const uint8_t *pbc, *fixed;
    double *pos;
    // graph scratch (chain b: rows row_start[b + i], slots [cfg_start[b] * cap_per_atom, ...))
    double *wpos;
    int *wrap, *deg, *row_start, *edge_S, *rev;
    float4 *edge;
    unsigned long long *hits;
    int hits_stride, cap_per_atom;
    double rc2;
    // potential results
    double *e_atom, *forces, *energy;
    // CG
    int max_iter, max_eval;
    double etol, ftol, dmax;
    double *x0, *hh, *gg;
    CgState *st;
    unsigned char *active;
    int *flags;   // [0]: a chain ran out of slot capacity (host regrows, relaunches); [1]: sink of the state machine's live counter
    int *n_evals; // [B] evaluations this workgroup made for its chain (work counters)
    long long max_launch;
};
template <class Site>
struct CmArgs {
    CmCommon c;
    typename Site::Params p;
};

constexpr int CM_THREADS = 256, CM_MAX_ATOMS = 256, CM_LPC = 16;

// ---- site policies: what differs between the kinds -------------------------------------------------------------------------
// A policy names its LDS struct (Shared: an instantiation carries only its own), its block of arguments (Params: parameter table
// and the scratch pointers in d_gbar), whether its phases read the reverse-slot table (REV), and two functions every thread of the
// workgroup calls in uniform control flow:
//   prepare(sh, A, P)                   once per launch, in front of the first barrier
//   sites(sh, A, P, a0, a1, rs)         rows rs of the atoms [a0, a1) -> e_atom, forces; ends behind a barrier
// Every phase inside is the device function the batch-wide kernel of the kind calls, with that kernel's lane-to-work mapping:
// thread tid serves centre tile0 + (tid >> 2) with lane tid & 3 in the site tiles, one thread per centre elsewhere.

struct TersoffSite {   // tersoff.hip: k_tersoff_site4 tiles, k_tersoff_site for the longer rows, k_tersoff_gather
    using Shared = TersShared;
    static constexpr bool REV = true;
    struct Params {
        int fast;
        const TersP *P;
        double *eps, *gslot;   // TersoffSlots
    };
    static __device__ __forceinline__ void prepare(Shared &sh, const CmCommon &A, const Params &P) {
        if (P.fast) tersoff_derive_params(sh, A.n_types, P.P);
    }
    static __device__ __forceinline__ void sites(Shared &sh, const CmCommon &A, const Params &P, int a0, int a1, const int *rs) {
        const int tid = threadIdx.x;
        CMP_INIT
        if (P.fast) {
            for (int t0 = a0; t0 < a1; t0 += TS_CENTRES) {
                const int i = t0 + (tid >> 2);
                tersoff_site4_tile(sh, i, i < a1, A.n_types, A.type, A.atom_cfg, A.cell, A.wpos, rs, A.edge, A.edge_S, P.eps, P.gslot);
                __syncthreads();
            }
        }
        CMP(5)
        for (int i = a0 + tid; i < a1; i += CM_THREADS)
            tersoff_site_atom(i, A.n_types, P.P, A.type, A.atom_cfg, A.cell, A.wpos, rs, A.edge, A.edge_S, P.eps, P.gslot, P.fast ? TS_MAXD : -1);
        __syncthreads();
        CMP(6)
        for (int i = a0 + tid; i < a1; i += CM_THREADS) tersoff_gather_atom(i, rs, A.rev, P.eps, P.gslot, A.e_atom, A.forces);
        __syncthreads();
        CMP(7)
    }
};

struct SwSite {   // sw.hip: k_sw_site tiles (the long-row form is inside the body), k_sw_gather
    using Shared = SwShared;
    static constexpr bool REV = true;
    struct Params {
        const SwP *P;
        double *eo, *ej, *gslot;   // SwSlots
    };
    static __device__ __forceinline__ void prepare(Shared &, const CmCommon &, const Params &) {}
    static __device__ __forceinline__ void sites(Shared &sh, const CmCommon &A, const Params &P, int a0, int a1, const int *rs) {
        const int tid = threadIdx.x;
        CMP_INIT
        static_assert(SW_CENTRES * SW_LANES == CM_THREADS, "the site tile is the workgroup");
        for (int t0 = a0; t0 < a1; t0 += SW_CENTRES) {
            const int i = t0 + (tid >> 2);
            sw_site_tile(sh, i, i < a1, A.n_types, P.P, A.type, A.atom_cfg, A.cell, A.wpos, rs, A.edge, A.edge_S, P.eo, P.ej, P.gslot);
            __syncthreads();   // (the next tile overwrites the staged neighborhood; behind the last tile: every G, eo, ej is written)
        }
        CMP(5)
        for (int i = a0 + tid; i < a1; i += CM_THREADS) sw_gather_atom(i, rs, A.rev, P.eo, P.ej, P.gslot, A.e_atom, A.forces);
        __syncthreads();
        CMP(7)
    }
};

template <bool TYPED>
struct EamSite {   // eam.hip: k_eam_density, k_eam_force, one thread per centre
    struct Shared {};
    static constexpr bool REV = false;   // every pair is seen from both ends: no gather over reverse slots
    struct Params {
        vssr_eam_grid g;
        EamTyped T;
        double *e_embed, *fp;   // EamAtoms
    };
    static __device__ __forceinline__ void prepare(Shared &, const CmCommon &, const Params &) {}
    static __device__ __forceinline__ void sites(Shared &, const CmCommon &A, const Params &P, int a0, int a1, const int *rs) {
        const int tid = threadIdx.x;
        CMP_INIT
        for (int i = a0 + tid; i < a1; i += CM_THREADS)
            eam_density_atom<TYPED>(i, P.g, P.T, A.type, A.atom_cfg, A.cell, A.wpos, rs, A.edge, A.edge_S, P.e_embed, P.fp);
        __syncthreads();   // (pass 2 reads F'(rho_j) of the chain's other atoms)
        CMP(5)
        for (int i = a0 + tid; i < a1; i += CM_THREADS)
            eam_force_atom<TYPED>(i, P.g, P.T, A.type, A.atom_cfg, A.cell, A.wpos, rs, A.edge, A.edge_S, P.e_embed, P.fp, A.e_atom, A.forces);
        __syncthreads();
        CMP(7)
    }
};

struct PairSite {   // pair.hip: k_pair_site<false> tiles; the body writes e_atom and the forces itself
    struct Shared { PairTerm term[PAIR_MAX_TYPES * PAIR_MAX_TYPES * PAIR_MAX_TERMS]; };
    static constexpr bool REV = false;
    struct Params { const PairTable *P; };
    static __device__ __forceinline__ void prepare(Shared &, const CmCommon &, const Params &) {}
    static __device__ __forceinline__ void sites(Shared &sh, const CmCommon &A, const Params &P, int a0, int a1, const int *rs) {
        const int tid = threadIdx.x;
        CMP_INIT
        static_assert(PAIR_CENTRES * PAIR_LANES == CM_THREADS, "the site tile is the workgroup");
        for (int t0 = a0; t0 < a1; t0 += PAIR_CENTRES) {
            const int i = t0 + (tid >> 2);
            pair_site_tile<false>(sh.term, i, i < a1, A.n_types, P.P, A.type, A.atom_cfg, A.cell, A.wpos, rs, A.edge, A.edge_S, A.e_atom,
                                  A.forces, nullptr);
            __syncthreads();   // (the next tile stages the term table again)
        }
        CMP(5)
    }
};

// One energy + force evaluation of chain b at its current positions, every thread of the workgroup in uniform control flow; false: the
// slot capacity of the chain's pool is exceeded (nothing downstream of the row scan ran).  Shared by the minimiser (k_cg_chain) and the
// integrator (k_md_chain) below.  scan: CM_THREADS ints, red: 256 doubles, s_over: one int of LDS, zero at the first call.
template <class Site>
__device__ __forceinline__ bool cm_evaluate(typename Site::Shared &sh, double *red, int *scan, int *s_over, const CmCommon &A,
                                            const typename Site::Params &SP, int b, int a0, int n, long long slot0, long long slot1, int *rs) {
    const int tid = threadIdx.x, a1 = a0 + n;
    CMP_INIT
    for (int i = a0 + tid; i < a1; i += CM_THREADS) wrap_atom(i, A.pos, A.atom_cfg, A.cell, A.invcell, A.pbc, A.wpos, A.wrap);
    __syncthreads();
    CMP(0)
    for (int base = a0; base < a1; base += CM_THREADS / CM_LPC) {   // 16 lanes per centre, 16 centres per pass
        const int i = base + tid / CM_LPC;
        if (i < a1)
            nbr_row<false, CM_LPC>(i, A.wpos, A.atom_cfg, A.cfg_start, A.cell, A.invcell, A.nimg, A.rc2, A.deg, rs, A.edge, A.edge_S, slot1,
                                   A.hits, A.hits_stride, nullptr);
    }
    __syncthreads();
    CMP(1)
    {   // rows of the chain: exclusive scan of the padded degrees (n <= 256: one atom per thread)
        const int pd = tid < n ? max((A.deg[a0 + tid] + 3) & ~3, 8) : 0;
        scan[tid] = pd;
        __syncthreads();
        for (int d = 1; d < CM_THREADS; d <<= 1) {
            const int v = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        if (tid < n) rs[a0 + tid] = (int)(slot0 + scan[tid] - pd);
        if (tid == CM_THREADS - 1) {
            rs[a1] = (int)(slot0 + scan[tid]);
            if (slot0 + scan[tid] > slot1) *s_over = 1;
        }
        __syncthreads();
        if (*s_over) return false;
    }
    CMP(2)
    for (int base = a0; base < a1; base += CM_THREADS / CM_LPC) {
        const int i = base + tid / CM_LPC;
        if (i < a1)
            nbr_row<true, CM_LPC>(i, A.wpos, A.atom_cfg, A.cfg_start, A.cell, A.invcell, A.nimg, A.rc2, A.deg, rs, A.edge, A.edge_S, slot1,
                                  A.hits, A.hits_stride, nullptr);
    }
    __syncthreads();
    CMP(3)
    if (Site::REV) {
        for (int base = a0; base < a1; base += CM_THREADS / CM_LPC) {
            const int i = base + tid / CM_LPC;
            if (i < a1) rev_row<CM_LPC>(i, rs, A.edge, A.edge_S, A.rev);
        }
        __syncthreads();
    }
    CMP(4)
    Site::sites(sh, A, SP, a0, a1, rs);
    {
        CMP_INIT
        chain_energy(b, red, A.cfg_start, A.e_atom, A.energy);
        __syncthreads();
        CMP(8)
    }
    return true;
}

template <class Site>
__global__ void __launch_bounds__(CM_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_cg_chain(const CmArgs<Site> *__restrict__ Ap) {
    const CmCommon &A = Ap->c;   // (arguments in memory: ~45 pointers and scalars live across every phase would otherwise sit in -- and spill from -- scalar registers)
    const typename Site::Params &SP = Ap->p;
    __shared__ typename Site::Shared sh;
    __shared__ double red[256];
    __shared__ int scan[CM_THREADS];
    __shared__ int s_over;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int a0 = A.cfg_start[b], n = A.cfg_start[b + 1] - a0;
    const long long slot0 = (long long)a0 * A.cap_per_atom, slot1 = slot0 + (long long)n * A.cap_per_atom;
    int *rs = A.row_start + b;   // rs[i], rs[i + 1] for the global atom index i of this chain: n + 1 entries of its own
    Site::prepare(sh, A, SP);
    if (tid == 0) s_over = 0;
    __syncthreads();
    int evals = 0;

    // one energy + force evaluation of the chain at its current positions; false: slot capacity exceeded (nothing was stepped)
    auto evaluate = [&]() -> bool {
        if (!cm_evaluate<Site>(sh, red, scan, &s_over, A, SP, b, a0, n, slot0, slot1, rs)) return false;
        evals += 1;
        return true;
    };

    // Every stop of the state machine happens right behind an evaluation of the positions the chain is left at (cg_dev.h: no branch
    // moves atoms and stops), so the results of the LAST evaluation are the static results of the final geometry -- what the
    // lock-step driver obtains with one more batch-wide evaluation after its loop.
    for (long long it = 0;; ++it) {
        if (!evaluate()) {   // (state untouched: the host enlarges the slot pools and launches again)
            if (tid == 0) { atomicOr(A.flags, 1); A.n_evals[b] += evals; }
            return;
        }
        if (it >= A.max_launch) break;   // launch budget of the lock-step driver exhausted (max_eval + 72 evaluations)
        {
            CMP_INIT
            cg_step_chain(b, red, A.cfg_start, A.energy, A.forces, A.fixed, A.max_iter, A.max_eval, A.etol, A.ftol, A.dmax, A.pos, A.x0, A.hh, A.gg,
                          A.st, A.active, A.flags + 1);
            __syncthreads();
            CMP(9)
        }
        if (A.st[b].reason) break;   // (uniform: written by thread 0 in front of the barrier)
    }
    if (tid == 0) A.n_evals[b] += evals;
}

// ---- the chain-resident integrator: ONE workgroup runs the whole molecular-dynamics call of ONE chain ------------------------
// MD is the minimiser's argument with thousands of evaluations per call instead of 55: the evaluation phase above, then the integrator
// of md_dev.h -- the function the lock-step driver launches as k_md_step (md.hip) -- with a barrier instead of ~12 launches in between.
// Same bits as that driver: positions, velocities, thermo records, step counts, stop reasons, the final static results
// (tests/test_md_gpu.py).  CmCommon is taken as it is (its CG fields stay unused) so that k_cg_chain's argument block keeps its layout.
struct CmMd {
    MdParams P;
    MdView V;
    int *stopped;
};
template <class Site>
struct CmMdArgs {
    CmCommon c;
    typename Site::Params p;
    CmMd m;
};

template <class Site>
__global__ void __launch_bounds__(CM_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_md_chain(const CmMdArgs<Site> *__restrict__ Ap) {
    const CmCommon &A = Ap->c;
    const typename Site::Params &SP = Ap->p;
    const CmMd &M = Ap->m;
    __shared__ typename Site::Shared sh;
    __shared__ double red[256];
    __shared__ int scan[CM_THREADS];
    __shared__ int s_over;
    const int b = blockIdx.x, tid = threadIdx.x;
    // A launch after a capacity regrow finds the chains where they stopped: reason 1 -- the results of the final positions are in
    // place; reason 2 -- the chain went back to its last completed step, the static evaluation of that state is (still) due.
    int done = M.V.st[b].reason;   // (uniform: nothing has written it in this launch)
    if (done == 1) return;
    const int a0 = A.cfg_start[b], n = A.cfg_start[b + 1] - a0;
    const long long slot0 = (long long)a0 * A.cap_per_atom, slot1 = slot0 + (long long)n * A.cap_per_atom;
    int *rs = A.row_start + b;
    Site::prepare(sh, A, SP);
    if (tid == 0) s_over = 0;
    __syncthreads();
    int evals = 0;
    // A step closes right behind the evaluation of the positions it moved to, and the chain stops there (md_dev.h): the results of the
    // LAST evaluation are the static results of the final state, as in k_cg_chain.
    for (;;) {
        if (!cm_evaluate<Site>(sh, red, scan, &s_over, A, SP, b, a0, n, slot0, slot1, rs)) {   // (state untouched: the host enlarges the pools)
            if (tid == 0) { atomicOr(A.flags, 1); A.n_evals[b] += evals; }
            return;
        }
        evals += 1;
        if (done) break;
        md_step_chain<double>(b, red, A.cfg_start, A.energy, A.forces, A.fixed, M.P, A.pos, M.V, A.active, M.stopped);
        __syncthreads();
        done = M.V.st[b].reason;   // (uniform: written by thread 0 in front of the barrier)
        if (done == 1) break;
    }
    if (tid == 0) A.n_evals[b] += evals;
}

__global__ void k_cm_init(int B, CgState *__restrict__ st, unsigned char *__restrict__ active, int *__restrict__ n_evals) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    CgState S = {};
    S.phase = PH_START;
    st[b] = S;
    active[b] = 1;
    n_evals[b] = 0;
}
__global__ void k_cm_report(int B, const CgState *__restrict__ st, int *__restrict__ out /*[B][3]*/) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    out[3 * b] = st[b].niter; out[3 * b + 1] = st[b].neval; out[3 * b + 2] = st[b].reason;
}

template <class Site>
static hipError_t cm_launch(hipStream_t st, int B, void *d_args, const CmCommon &c, const typename Site::Params &p, const CmMd *md) {
    static_assert(sizeof(CmArgs<Site>) <= 1024 && sizeof(CmMdArgs<Site>) <= 1024, "argument block");
    if (md) {   // the integrator
        const CmMdArgs<Site> A{c, p, *md};
        if (hipError_t e = hipMemcpyAsync(d_args, &A, sizeof(A), hipMemcpyHostToDevice, st)) return e;   // (pageable source: copied before the call returns)
        hipLaunchKernelGGL(k_md_chain<Site>, dim3(B), dim3(CM_THREADS), 0, st, static_cast<const CmMdArgs<Site> *>(d_args));
        return hipGetLastError();
    }
    const CmArgs<Site> A{c, p};
    if (hipError_t e = hipMemcpyAsync(d_args, &A, sizeof(A), hipMemcpyHostToDevice, st)) return e;   // (pageable source: copied before the call returns)
    hipLaunchKernelGGL(k_cg_chain<Site>, dim3(B), dim3(CM_THREADS), 0, st, static_cast<const CmArgs<Site> *>(d_args));
    return hipGetLastError();
}

// The kind's scratch in d_gbar (sized for the slot_cap / atom count of this attempt), its argument block, its instantiation of the
// minimiser (md == nullptr) or of the integrator.
static int cm_launch_kind(vssr_handle *h, void *d_args, const CmCommon &c, const CmMd *md = nullptr) {
    const int B = h->n_cfg;
    hipStream_t st = h->stream;
    size_t scratch = 0;   // doubles
    switch (h->kind) {
    case Kind::TERSOFF: scratch = TersoffSlots::doubles(h); break;
    case Kind::SW: scratch = SwSlots::doubles(h); break;
    case Kind::EAM: scratch = EamAtoms::doubles(h); break;
    default: break;   // pair: the site tile writes e_atom and the forces itself
    }
    if (scratch && h->d_gbar.ensure(sizeof(double) * scratch)) return set_err(h, VSSR_E_NOMEM, "chain-resident minimiser: out of device memory");
    h->prof.begin(KC_ANALYTIC, st);
    hipError_t e = hipSuccess;
    switch (h->kind) {
    case Kind::TERSOFF: {
        const TersoffSlots S = slots_of(h);
        const int fast = (h->n_types * h->n_types * h->n_types <= TS_MAXP) ? 1 : 0;
        e = cm_launch<TersoffSite>(st, B, d_args, c, {fast, h->pot_params.as<TersP>(), S.eps, S.gslot}, md);
        break;
    }
    case Kind::SW: {
        const SwSlots S = SwSlots::of(h);
        e = cm_launch<SwSite>(st, B, d_args, c, {h->pot_params.as<SwP>(), S.eo, S.ej, S.gslot}, md);
        break;
    }
    case Kind::EAM: {
        const EamAtoms S = EamAtoms::of(h);
        if (h->eam_nel > 0)   // as eam_run chooses: a funcfl handle keeps the untyped bodies
            e = cm_launch<EamSite<true>>(st, B, d_args, c, {h->eam_grid, eam_tables(h), S.e_embed, S.fp}, md);
        else
            e = cm_launch<EamSite<false>>(st, B, d_args, c, {h->eam_grid, eam_tables(h), S.e_embed, S.fp}, md);
        break;
    }
    case Kind::PAIR: e = cm_launch<PairSite>(st, B, d_args, c, {h->pot_params.as<PairTable>()}, md); break;
    default: h->prof.end(st); return set_err(h, VSSR_E_STATE, "chain-resident minimiser: no kernel for this kind of handle");
    }
    h->prof.end(st);
    VSSR_HIP(h, e);
    return VSSR_OK;
}

// Can the chain-resident kernel serve this handle's resident batch at all?
static bool cm_capable(const vssr_handle *h) {
    const bool kind = h->kind == Kind::TERSOFF || h->kind == Kind::SW || h->kind == Kind::EAM || h->kind == Kind::PAIR;
    // (a pair handle with k-space: the reciprocal sum is not part of the chain-resident kernel, those relaxations run in lock step;
    // likewise an ADP handle: the kernel has no site tile for the dipole / quadrupole rows)
    return kind && !h->ew_on && !h->eam_adp && h->max_cfg_atoms <= CM_MAX_ATOMS;
}

// Which driver.  The handle's choice (vssr_batch_relax_cg_driver) forces one of them, the chain-resident one only where the kernel
// applies; VSSR_CG_FUSED keeps the meaning it had when the kernel served Tersoff alone: 0 = always the lock-step driver (every
// kind), non-zero = the chain-resident kernel for a Tersoff handle whenever it applies (no effect on the other kinds).
// AUTO: the chain-resident kernel wins while the batch is small enough for launch latency and lock-step waste to dominate
// (same-box A/B, GaN 48-atom chains, MC proposals/s, profiles/r05/NOTES_tersoff.md: 256 chains 20.9 k vs 15.9 k, 1 024: 45.0 k vs
// 36.9 k, 4 096: 51.5 k vs 52 .. 56 k, 16 384: 63 k vs 70 .. 75 k): two 4-wave workgroups per CU cannot hide the fp64 latency chains
// of the site terms as well as the batch-wide kernels do at 12 waves per CU once every CU has work for many rounds.
bool chain_min_supported(const vssr_handle *h) {
    if (!cm_capable(h)) return false;
    const char *e = getenv("VSSR_CG_FUSED");   // (read per call)
    if (e && atoi(e) == 0) return false;
    if (e && h->kind == Kind::TERSOFF) return true;
    if (h->cg_driver == VSSR_CG_DRIVER_LOCKSTEP) return false;
    if (h->cg_driver == VSSR_CG_DRIVER_RESIDENT) return true;
    // the automatic choice covers the regime that was measured: Tersoff chains of <= 64 atoms (one site tile per workgroup).  A
    // 200-atom chain runs its 64-centre site tiles one after another inside one workgroup, and the SW, EAM and pair instantiations
    // win or lose by batch size and kind (profiles/r15/NOTES_chain_resident_kinds.md): those take the lock-step kernels unless the
    // handle asks for the chain-resident one (advisor r5)
    return h->kind == Kind::TERSOFF && h->n_cfg <= 3072 && h->max_cfg_atoms <= 64;
}

// The resident batch, the graph scratch and the result arrays of one launch attempt (slot pools of `cap` slots per atom).
static CmCommon cm_batch_args(const vssr_handle *h, const uint8_t *fixed, unsigned long long *hits_buf, int hits_stride, int cap, double rc,
                              int *flags, int *n_evals) {
    CmCommon A{};
    A.n_types = h->n_types;
    A.type = h->d_Z.as<int>(); A.atom_cfg = h->d_atom_cfg.as<int>(); A.cfg_start = h->d_cfg_start.as<int>(); A.nimg = h->d_nimg.as<int>();
    A.cell = h->d_cell.as<double>(); A.invcell = h->d_invcell.as<double>();
    A.pbc = h->d_pbc.as<uint8_t>(); A.fixed = fixed;
    A.pos = h->d_pos.as<double>();
    A.wpos = h->d_wpos.as<double>(); A.wrap = h->d_wrap.as<int>(); A.deg = h->d_deg.as<int>(); A.row_start = h->d_row_start.as<int>();
    A.edge_S = h->d_edge_S.as<int>(); A.rev = h->d_rev.as<int>(); A.edge = h->d_edge.as<float4>();
    A.hits = hits_buf; A.hits_stride = hits_stride; A.cap_per_atom = cap; A.rc2 = rc * rc;
    A.e_atom = h->d_pot_ea.as<double>(); A.forces = h->d_pot_f.as<double>(); A.energy = h->d_pot_e.as<double>();
    A.active = h->d_active.as<unsigned char>(); A.flags = flags; A.n_evals = n_evals;
    return A;
}

// One chain-resident call, the part the minimiser and the integrator share: the graph scratch and result buffers, d_cm carved into
// [arguments (1 KB) | flags [8] | evaluations [B]], then launch attempts with slot pools of `cap` slots per atom until no chain
// overflowed its pool, and the evaluations the chains spent.  `who` names the driver in the out-of-memory message; reset(n_evals)
// enqueues what clears the evaluation counts ahead of the first attempt, fill(A) sets the driver's own fields of an attempt's CmCommon
// (md != null: the integrator, which has none), report() enqueues what the driver reads out of its state behind the last attempt.
template <class Reset, class Fill, class Report>
static int cm_run(vssr_handle *h, const char *who, const uint8_t *fixed, const CmMd *md, Reset reset, Fill fill, Report report) {
    const int B = h->n_cfg, N = h->n_atoms;
    hipStream_t st = h->stream;
    char *d_args = nullptr;
    int *flags = nullptr, *n_evals = nullptr;
    auto layout = [&](Arena &a) { a.place(d_args, 1024); a.place(flags, 8); a.place(n_evals, (size_t)B); };
    if (h->d_cm.ensure(arena_size(layout)) || h->d_wpos.ensure(sizeof(double) * 3 * (size_t)N) ||
        h->d_wrap.ensure(sizeof(int) * 3 * (size_t)N) || h->d_deg.ensure(sizeof(int) * (size_t)N) ||
        h->d_row_start.ensure(sizeof(int) * ((size_t)N + B + 1)) || h->d_pot_e.ensure(sizeof(double) * (size_t)B) ||
        h->d_pot_ea.ensure(sizeof(double) * (size_t)N) || h->d_pot_f.ensure(sizeof(double) * 3 * (size_t)N))
        return set_err(h, VSSR_E_NOMEM, "chain-resident %s: out of device memory", who);
    arena_carve(h->d_cm.p, layout);
    VSSR_HIP(h, reset(n_evals));
    const double rc = evaluator(h).cutoff(h);   // (EAM: the file's cutoff, as eam_run; the others: the table's largest)
    // slots per atom of the per-chain pools: the handle's capacity, or what an earlier chain-resident call had to grow to.  The
    // grown value stays with THIS driver family (cm_cap_per_atom): the batch-wide runs size their buffers from cap_per_atom and repair
    // an overflow exactly, they must not inherit up to 64x from a pool that doubles (advisor r5)
    int cap = std::max(h->cap_per_atom, h->cm_cap_per_atom);
    for (int attempt = 0;; ++attempt) {
        // slot pools: every chain owns n_atoms x cap slots
        const long long slots = (long long)N * cap + 64;
        if (slots > 2147483000LL) return set_err(h, VSSR_E_CAPACITY, "neighbor list exceeds 2^31 slots");
        if (h->slot_cap < slots) h->slot_cap = slots;
        if (h->d_edge.ensure(sizeof(float4) * h->slot_cap) || h->d_edge_S.ensure(sizeof(int) * h->slot_cap) ||
            h->d_rev.ensure(sizeof(int) * h->slot_cap))
            return set_err(h, VSSR_E_NOMEM, "neighbor buffers: out of device memory");
        unsigned long long *hits_buf = nullptr;
        const int hits_stride = (h->max_cfg_atoms + 63) & ~63;
        if (h->max_images <= 64 && (size_t)N * hits_stride * 8 <= ((size_t)1 << 30) && !h->d_hits.ensure((size_t)N * hits_stride * 8))
            hits_buf = h->d_hits.as<unsigned long long>();
        VSSR_HIP(h, hipMemsetAsync(flags, 0, sizeof(int) * 8, st));
        CmCommon A = cm_batch_args(h, fixed, hits_buf, hits_stride, cap, rc, flags, n_evals);
        fill(A);
        if (int e = cm_launch_kind(h, d_args, A, md)) return e;
        ++h->relax_lockstep;
        int over = 0;
        VSSR_HIP(h, hipMemcpyAsync(&over, flags, sizeof(int), hipMemcpyDeviceToHost, st));
        VSSR_HIP(h, hipStreamSynchronize(st));
        if (!over) break;
        // a chain needed more slots per atom than its pool holds: chains that were stopped kept their state (nothing is stepped on
        // an overflowed evaluation) and continue in the next launch, from their own counters, with larger pools
        // (ten doublings: a pair cutoff over several images of a small cell gives rows of several hundred slots, 2^31 slots bound the rest)
        if (attempt >= 10) return set_err(h, VSSR_E_CAPACITY, "neighbor capacity could not be satisfied");
        cap *= 2;
        ++h->relax_regrows;
    }
    h->cm_cap_per_atom = cap;
    report();
    std::vector<int> ne(B);
    VSSR_HIP(h, hipMemcpyAsync(ne.data(), n_evals, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    VSSR_HIP(h, hipStreamSynchronize(st));
    long long tot = 0;
    for (int b = 0; b < B; ++b) tot += ne[b];
    h->relax_chain_evals = tot;
    h->active_mask = nullptr;
    h->h_counters[2] = 0;      // (no batch-wide neighbor build ran: nothing for vssr_synchronize to repair)
    return VSSR_OK;
}

// Same contract as relax_cg (relax_cg.hip): afterwards the batch holds the minimised positions, d_pot_e / _ea / _f the static results of
// those geometries, d_relax_steps [B][3] = (iterations, evaluations, stop reason) per chain.  (The rows are numbered per chain: the
// entry point closes the call with graph_partial set, the batch-wide introspection calls want one plain run first.)
int chain_min_cg(vssr_handle *h, const vssr_cg_params *cp, const uint8_t *fixed_host, uint32_t want) {
    const int B = h->n_cfg;
    hipStream_t st = h->stream;
    const uint8_t *fixed = nullptr;
    CgWork W;
    if (int e = driver_open(h, fixed_host, 3, fixed, want)) return e;
    if (int e = CgWork::ensure(h, W)) return e;
    return cm_run(
        h, "minimiser", fixed, nullptr,
        [&](int *n_evals) {
            hipLaunchKernelGGL(k_cm_init, dim3((B + 127) / 128), dim3(128), 0, st, B, W.st, h->d_active.as<unsigned char>(), n_evals);
            return hipSuccess;
        },
        [&](CmCommon &A) {
            A.max_iter = cp->max_iter; A.max_eval = cp->max_eval; A.etol = cp->etol; A.ftol = cp->ftol; A.dmax = cp->dmax;
            A.x0 = W.x0; A.hh = W.hh; A.gg = W.gg;
            A.st = W.st;
            A.max_launch = (long long)cp->max_eval + 72;   // the lock-step driver's launch budget (relax_cg.hip), per chain here
        },
        [&] { hipLaunchKernelGGL(k_cm_report, dim3((B + 127) / 128), dim3(128), 0, st, B, W.st, h->d_relax_steps.as<int>()); });
}

// ---- the integrator's host side ---------------------------------------------------------------------------------------------------
// RESIDENT applies where the kernel does.  AUTO covers the regime that was measured (Langevin MD of the relaxed 48-atom GaN Tersoff
// chains, chain-steps/s, lock-step against chain-resident alternating in one run, profiles/r29/NOTES_md.md: the chain-resident kernel
// wins at 256 chains and loses from 1 024 chains on, for the reason given at chain_min_supported): Tersoff batches of <= 256 chains of
// <= 64 atoms take the chain-resident kernel, everything else the lock-step driver.
bool chain_md_supported(const vssr_handle *h) {
    if (!cm_capable(h) || h->md_driver == VSSR_MD_DRIVER_LOCKSTEP) return false;
    if (h->md_driver == VSSR_MD_DRIVER_RESIDENT) return true;
    return h->kind == Kind::TERSOFF && h->n_cfg <= 256 && h->max_cfg_atoms <= 64;
}

// Same contract as md_lockstep (md.hip): afterwards the batch holds the final positions, d_md_vel the velocities, d_pot_e / _ea / _f the
// static results of the final state of every chain, the workspace the step counts, stop reasons and thermo records.
int chain_md(vssr_handle *h, const MdWork &W) {
    const CmMd M{W.P, W.V, W.stopped};
    return cm_run(
        h, "integrator", W.fixed, &M,
        [&](int *n_evals) { return hipMemsetAsync(n_evals, 0, sizeof(int) * (size_t)h->n_cfg, h->stream); }, [](CmCommon &) {}, [] {});
}

}  // namespace vssr
