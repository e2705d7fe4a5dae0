// vssr_internal.h — shared declarations of the gfx950 evaluation backend (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/vssr_eval.h"

namespace vssr {

constexpr int F = 128;        // feat_dim (compiled value)
constexpr int F3 = 3 * F;
constexpr int MAX_LAYERS = 4;
constexpr int MAX_MODELS = 8;
constexpr int RB_MAX = 24;    // n_rbf + 1 (envelope/bias column) padded to a multiple of 4
constexpr int NODE_TILE = 8;  // atoms per workgroup in the node kernels
constexpr int L0_MAX_SPECIES = 8;  // layer-0 species factorisation is used when the batch has at most this many species

// ---- device-side views -------------------------------------------------------------------
struct LayerW {
    const float *W1, *W1t, *b1;  // [F][F], transposed [F][F]
    const float *W2, *W2t, *b2;  // [3F][F], transposed [F][3F]
    const float *Wd, *bd;        // [3F][R], [3F]
    const float *U, *Ut, *V, *Vt;  // [F][F]
    const float *W3, *W3t, *b3;  // [F][2F], transposed [2F][F]
    const float *W4, *W4t, *b4;  // [3F][F], transposed [F][3F]
    // W1, W2, U, V, W3, W4 (forward) and W1^T, W2^T, W4^T, W3^T, [U;V]^T (reverse) as 2-way fp16 pieces in
    // v_mfma_f32_16x16x32_f16 B-fragment order (pack_mfma_tiles16), 16-column tiles
    const uint4 *qW1, *qW2, *qU, *qV, *qW3, *qW4, *qW1t, *qW2t, *qW4t, *qW3t, *qUVt;
    const uint4 *wd16;           // radial-filter weights, 2-way fp16 split in MFMA A-operand order: [3F rows][4 quarters][operand 1, 2] (build_wd16)
};
struct ModelW {
    const float *embed;  // [n_embed][F]
    LayerW layer[MAX_LAYERS];
    const float *W5, *W5t, *b5, *w6, *b6;  // [H][F], [F][H], [H], [H], [1]
    const uint4 *qW5, *qW5t;               // readout matrices as fp16 pieces in MFMA fragment order (painn_node_mfma.hip)
};

// Chains that take part in an evaluation.  During a lock-step relaxation converged chains are switched off: every kernel
// tests its chain (or the chains of its atom tile) and leaves at once, so an iteration costs what the unconverged chains cost;
// the results of a switched-off chain stay those of its last evaluation.  mask == nullptr: all chains.
struct ActiveView {
    const unsigned char *mask;   // [n_cfg] 1 = evaluate
    const int *atom_cfg;         // [n_atoms]
    unsigned *sat = nullptr;     // [n_cfg] raised by the node kernels when an activation left the fp16-split range (mfma16.h SatTrack)
    __device__ __forceinline__ bool chain(int c) const { return !mask || mask[c]; }
    __device__ __forceinline__ bool atom(int i) const { return !mask || mask[atom_cfg[i]]; }
    // any active chain among atoms [a0, a1]?  (chains are contiguous atom ranges)
    __device__ __forceinline__ bool tile(int a0, int a1) const {
        if (!mask) return true;
        for (int c = atom_cfg[a0], c1 = atom_cfg[a1]; c <= c1; ++c)
            if (mask[c]) return true;
        return false;
    }
};

struct GraphView {  // neighbor multigraph of the resident batch (padded CSR by centre)
    int n_atoms;             // total atoms in the batch
    int n_cfg;
    const int *atom_cfg;     // [n_atoms] configuration (chain) of each atom
    const int *cfg_start;    // [n_cfg+1]
    const int *row_start;    // [n_atoms+1] first slot of each centre (slot counts are multiples of 4)
    const int *deg;          // [n_atoms] real degree (unpadded)
    const float4 *edge;      // [slots] {r_x, r_y, r_z, bitcast(j)} ; j < 0 marks a pad slot
    const int *rev;          // [slots] slot of the reverse edge (j -> i, -S)
    // per-slot geometry tables, computed once per evaluation and shared by every layer / model / feature slice
    const float4 *erec;      // [slots] {u_x, u_y, u_z, bitcast(j local to its chain)} ; pads: u = 0, j = 0 (same condition as rho, else null)
    const float *rho;        // [slots][4][6]  radial basis * envelope, [kq][ks] = rho_{kq+4ks}: only for the layer-0 kernel of batches with > 4 species (else null)
    const uint4 *rho16;      // operand-ready 2-way fp16 split of rho + the slot's scalars, quad-interleaved: [slot / 4][unit 0, 1][quarter][slot % 4] x 16 B (nbr.hip f16_unit, write_f16_record)
    const uint4 *drho16;     // same for d rho / d d
    const unsigned char *zslot;   // [slots] species index (zmap) of the neighbor, 255 for pads / unmapped
    const float2 *dist2;     // [slots] {1 / edge length (pads: -1), excluded-volume dE/dd = -p (sigma/d)^p / d (pads: 0)}
    const int4 *bundle;      // [n_atoms] per chain: centres sorted by padded degree (descending): {centre (chain-local), first slot, padded slot count, 0}
    const unsigned char *chain_class;   // [n_cfg] EDGE_BCLASS_*: which reverse neighbor kernels serve the chain (layers >= 1); a chain
                                        // gathers in the reverse pass exactly when it gathers in the forward pass
    ActiveView act;          // chains switched off by the relaxation driver
};

// Wave-wide integer prefix sum and float sum on the DPP network / the gfx950 row swaps (no LDS permutes: a __shfl is a ds_bpermute,
// ~100 cycles, and a scan / butterfly is six of them in a dependent chain).  Fixed orders, independent of what else runs.
#if defined(__HIPCC__)
__device__ __forceinline__ int wave_incl_scan_i32(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);    // row_shr:1 (lanes without a source add 0)
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);    // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);    // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);    // row_shr:8   -> inclusive inside every 16-lane row
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);   // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);   // row_bcast:31 into rows 2 and 3
    return x;
}
__device__ __forceinline__ float xrow_sum_f32(float x) {   // sum over the four 16-lane rows (lanes l, l^16, l^32, l^48), result in every lane
    const unsigned u = __float_as_uint(x);
    const auto r32 = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const float y = __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
    const unsigned v = __float_as_uint(y);
    const auto r16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
}
__device__ __forceinline__ float wave_sum_f32(float x) {   // result in every lane
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x124, 0xF, 0xF, true));   // row_ror:4
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x128, 0xF, 0xF, true));   // row_ror:8
    const unsigned u = __float_as_uint(x);
    const auto r32 = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const float y = __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
    const unsigned v = __float_as_uint(y);
    const auto r16 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
}
#endif

// Radial basis of one slot for one table quarter kq (radial indices n = kq + 1 + 4 ks, ks = 0..4, then the envelope):
//   r[ks] = sin(n pi d / rc) / d * fc(d),  dr[ks] = d r[ks] / d d,  r[5] = fc,  dr[5] = fc'   
// ONE definition for the kernel that writes the per-slot tables (k_edge_geom, nbr.hip) and for the kernel that rebuilds the fp32
// values instead of reading them (k_l0_bwd, painn_l0.hip): both see bit-identical numbers (no contraction, same operation order).
// ed: {r_x, r_y, r_z, bitcast(j)}, j < 0 marks a pad slot (everything zero, inv = 0).
#if defined(__HIPCC__)
__device__ __forceinline__ void radial_quarter(const float4 &ed, int kq, float rc, float (&r)[6], float (&dr)[6], float &inv, bool &valid) {
    const float alpha = 3.14159265358979323846f / rc;
    valid = __float_as_int(ed.w) >= 0;
    const float d2 = fmaf(ed.z, ed.z, fmaf(ed.y, ed.y, ed.x * ed.x));
    const float d = valid ? sqrtf(d2) : 1.f;
    inv = valid ? 1.f / d : 0.f;
    float s1, c1;
    sincosf(alpha * d, &s1, &c1);
    const bool inside = valid && d < rc;
    const float fc = inside ? 0.5f * (c1 + 1.f) : 0.f;
    const float dfc = inside ? -0.5f * alpha * s1 : 0.f;
    const float s2 = 2.f * s1 * c1, c2 = fmaf(c1, c1, -s1 * s1);
    const float s3 = fmaf(s2, c1, c2 * s1), c3 = fmaf(c2, c1, -s2 * s1);
    const float s4 = 2.f * s2 * c2, c4 = fmaf(c2, c2, -s2 * s2);
    float sn = kq == 0 ? s1 : kq == 1 ? s2 : kq == 2 ? s3 : s4;
    float cn = kq == 0 ? c1 : kq == 1 ? c2 : kq == 2 ? c3 : c4;
    float nf = (float)(kq + 1);
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
        const float rb = sn * inv;
        r[ks] = rb * fc;
        dr[ks] = fmaf(nf * alpha * cn * inv - rb * inv, fc, rb * dfc);
        const float sn2 = fmaf(sn, c4, cn * s4), cn2 = fmaf(cn, c4, -sn * s4);
        sn = sn2; cn = cn2; nf += 4.f;
    }
    r[5] = fc;      // envelope (bias column) replicated in every quarter
    dr[5] = dfc;
}
#endif

struct StateView {  // activations of all models: index [m][atom][...]
    int n_atoms;
    int n_models;
    // forward
    float *s_in[MAX_LAYERS + 1];  // [M][N][F]   state entering layer l (l = L: final)
    float *v_in[MAX_LAYERS + 1];  // [M][N][3][F]
    float *phi[MAX_LAYERS];       // [M][N][3F]
    float *s_msg[MAX_LAYERS];     // after message block l
    float *v_msg[MAX_LAYERS];
    float *e_atom;                // [M][N]
    const float *e_excl;          // [N] excluded-volume part (geometry only: written by k_edge_geom, nbr.hip)
    // reverse
    float *sbar;                  // [M][N][F]     adjoint of s_in[l+1] / s_in[l]
    float *vbar;                  // [M][N][3][F]
    float *sbar_msg;              // adjoint of s_msg[l] (the fused reverse kernels alternate between sbar_msg and sbar)
    float *sbar_msg_l0;           // the buffer that holds the adjoint of s_msg[0] after a reverse pass
    float *vbar_msg;
    float *phibar;                // [M][N][3F]
    float4 *gbar;                 // [M][slots] dE/d r for the edge (j -> i) stored at slot (i, j)
};

// ---- host-side helpers ----------------------------------------------------------------------
struct DevBuf {   // owns its device allocation
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t need) {  // grow-only; contents are NOT preserved
        if (need <= bytes) return 0;
        release();
        size_t want = need + need / 4 + 256;
        if (hipMalloc(&p, want) != hipSuccess) return -1;
        bytes = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// The handle's stream and its pinned counters: created by open_device, released with the handle.  Both convert to the raw
// pointer, so call sites read as they would with one.
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream &) = delete;
    OwnedStream &operator=(const OwnedStream &) = delete;
    ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
struct PinnedInts {
    int *p = nullptr;
    PinnedInts() = default;
    PinnedInts(const PinnedInts &) = delete;
    PinnedInts &operator=(const PinnedInts &) = delete;
    ~PinnedInts() { if (p) (void)hipHostFree(p); }
    operator int *() const { return p; }
};

enum KernelClass {
    KC_NBR = 0,
    KC_EMBED,
    KC_MSG_MLP,
    KC_EDGE_FWD,
    KC_UPDATE_FWD,
    KC_READOUT,
    KC_UPDATE_BWD,
    KC_EDGE_BWD,
    KC_MSG_MLP_BWD,
    KC_FINALIZE,
    KC_ANALYTIC,   // the fp64 analytic potentials (reported as "tersoff")
    KC_L0_FWD,
    KC_L0_BWD,
    KC_NEB_PROJECT,   // nudged elastic band (neb.hip): the tangent / projection kernel
    KC_NEB_STEP,      // and the band-wide FIRE step
    KC_DIMER,         // dimer method (dimer.hip): the per-dimer state machine behind every evaluation
    KC_COUNT
};
extern const char *const kKernelClassNames[KC_COUNT];

struct Profiler {
    bool enabled = false;
    struct Rec { int kc; hipEvent_t a, b; };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    int64_t launches[KC_COUNT] = {0};
    double total_ms[KC_COUNT] = {0};
    hipEvent_t get_event();
    void begin(int kc, hipStream_t s);
    void end(hipStream_t s);
    void collect();  // stream must be synchronised
    void reset();
    Profiler() = default;
    Profiler(const Profiler &) = delete;
    Profiler &operator=(const Profiler &) = delete;
    ~Profiler();     // stream must be synchronised; no HIP call when no event was ever created
};

// State of a Gaussian-mixture fit (Kind::GMM_FIT, gmm_fit.hip).  The mixture being fitted lives in the handle's scoring layout
// (gmm_K / gmm_D / gmm_Dp / d_gmm_P / d_gmm_c / d_gmm_kc / d_gmm_mask): the E step is gmm_score_f64 on the resident rows.
struct GmmFit {
    int cov_type = 0;   // VSSR_GMM_COV_*
    int init = 0;       // VSSR_GMM_INIT_*
    int max_iter = 100, n_init = 1;
    double tol = 1e-3, reg_covar = 1e-6;
    uint64_t seed = 0;
    bool device_ready = false, fitted = false;
    int64_t n = 0, cap = 0;        // resident rows / capacity of rows
    DevBuf rows;                   // [cap][Dp] fp64, zero pad columns (sized exactly and grown with its contents: fit_reserve, gmm_fit.hip)
    double *x() const { return rows.as<double>(); }
    // explicit initial values (vssr_gmm_fit_set_init), host side
    std::vector<double> i_means, i_weights, i_prec;
    std::vector<int> i_labels;
    bool has_means = false, has_weights = false, has_prec = false, has_labels = false;
    DevBuf resp, labels, lbpart, status, flags;
    DevBuf part_s, part_q, part_n, nk, means, avg_x2, w, cov, part_cov, chol_w, chol_y, centers, assign_part;
    DevBuf b_w, b_means, b_cov, b_P, b_c, b_kc, b_mask;   // best restart so far (n_init > 1)
};

// State of a latent-space clustering (Kind::CLUSTER, cluster.hip).  The rows live in the handle's GmmFit (x / n / cap: the append paths
// of the mixture fit serve both kinds); everything below is the PCA and the Ward linkage.
struct Cluster {
    int n_components = 0, whiten = 1, d_clu = 3, d_pad = 3;   // d_pad: d_clu rounded up to 1, 2, 3, 4, 8, 16 or 32 (zero coordinates)
    bool pca_done = false;
    int64_t n_pts = 0;             // points resident for the linkage (from the PCA or from vssr_cluster_set_points)
    DevBuf mean, denom, part_sum, part_cov, cov, evec, eval, comp, comp_t, ev, ratio, jac, xr;   // PCA
    DevBuf pts;                    // [n_pts][d_pad] fp64
    DevBuf cen[2], siz[2], cid[2]; // live clusters, double buffered: centroids [m][d_pad], sizes [m], ids [m]
    DevBuf nn, flag, blk, rec, counters;
};

// What a handle is.  The numbers are part of the documentation, so they stay.
enum class Kind : int {
    NONE = 0,
    PAINN = 1,     // PaiNN ensemble (painn.hip, painn_gen.hip)
    TERSOFF = 2,   // tersoff.hip
    EAM = 3,       // funcfl, eam/alloy and eam/fs tables (eam.hip); with eam_adp the angular-dependent potential (adp.hip)
    SW = 4,        // Stillinger-Weber (sw.hip)
    GMM = 5,       // Gaussian-mixture scoring (gmm.hip)
    GMM_FIT = 6,   // Gaussian-mixture fit (gmm_fit.hip)
    CLUSTER = 7,   // latent-space clustering (cluster.hip)
    PAIR = 8,      // pair potentials + damped-shifted-force Coulomb (pair.hip)
    VASHISHTA = 9, // Vashishta two- plus three-body potential (vashishta.hip)
    COUNT
};
constexpr unsigned kind_bit(Kind k) { return 1u << (int)k; }
// kinds that evaluate a resident batch: the vssr_batch_* / vssr_eval* / relaxation / introspection entry points serve these
constexpr unsigned KINDS_EVAL = kind_bit(Kind::PAINN) | kind_bit(Kind::TERSOFF) | kind_bit(Kind::EAM) | kind_bit(Kind::SW) |
                                kind_bit(Kind::PAIR) | kind_bit(Kind::VASHISHTA);

}  // namespace vssr

// Members are destroyed in reverse order: every device buffer after the stream's declaration goes before the stream does.
struct vssr_handle {
    vssr::Kind kind = vssr::Kind::NONE;
    vssr_eam_grid eam_grid = {0, 0, 0.0, 0.0, 0.0};   // EAM: grids; spline tables live in pot_params
    int eam_nel = 0, eam_fs = 0;   // EAM with typed tables (vssr_eam_create_alloy): elements, 1 = eam/fs densities; 0 = one funcfl
    bool eam_adp = false;          // EAM with dipole / quadrupole tables (vssr_eam_create_adp): eam_run / eam_stress hand over to adp.hip
    double vash_r0max = 0.0;       // Vashishta: the largest r0 of the table (slots below it form a centre's short three-body row)
    int device = 0;
    vssr::OwnedStream stream;    // null until the handle reaches a device (open_device)
    std::string err;
    vssr::Profiler prof;

    int edge_impl = 1;  // 1 = LDS-slice + MFMA edge kernels for chains that fit LDS; 0 forces the gather kernels
                        // (VSSR_EDGE_IMPL=gather: debug knob, also the automatic path for very large chains)
    int max_cfg_atoms = 0;
    // chains by neighbor-sum path (EDGE_CLASS_*), fixed at upload from every chain's own atom count: class of every chain,
    // the chain lists of the matrix-pipe classes (concatenated in class order), counts and largest chain per class
    vssr::DevBuf d_chain_class, d_class_list;
    int n_class[5] = {0, 0, 0, 0, 0}, max_class_atoms[5] = {0, 0, 0, 0, 0};   // forward classes (EDGE_CLASS_*)
    int n_bclass[5] = {0, 0, 0, 0, 0}, max_bclass_atoms[5] = {0, 0, 0, 0, 0};   // reverse classes (EDGE_BCLASS_*); lists follow the forward lists
    int fs16_max_atoms = -1, fs8_max_atoms = -1;   // test knobs (VSSR_EDGE_FS16_MAX / _FS8_MAX): lower the class limits
    int max_images = 0;          // largest number of periodic images any configuration of the batch scans per pair

    // configuration
    int n_models = 0, n_rbf = 20, num_conv = 3, n_embed = 100, readout_hidden = 64;
    int feat_dim = vssr::F;      // the handle's own feature width (the compiled F on the 128 / 20 path)
    bool painn_general = false;  // PaiNN served by the general-width fp32 path (painn_gen.hip): every (feat_dim, n_rbf) but (128, 20),
                                 // or any shape with VSSR_PAINN_PATH=general
    float cutoff = 5.f;
    int excl_vol = 1, excl_power = 12;
    float excl_sigma = 1.5f;
    double units_per_ev = 1.0;
    bool has_offset = false;
    double offset_const = 0.0;

    // weights
    vssr::DevBuf weights;        // all model blobs + transposed copies
    vssr::DevBuf wd16;           // fp16-split radial-filter weights in MFMA operand order
    vssr::DevBuf node16;         // fp16-split node-GEMM weights in MFMA fragment order
    vssr::DevBuf model_table;    // ModelW[n_models]
    vssr::DevBuf offset_per_z;   // double[n_embed]

    // the fp64 analytic potentials (Tersoff, EAM, Stillinger-Weber, pair)
    int n_types = 0;
    double pot_cutoff = 0;       // Tersoff, SW, pair: largest cutoff of the table (EAM: eam_grid.cutoff)
    // pair handles with k-space (vssr_pair_create_kspace, ewald.hip): Ewald damping g, reciprocal cutoff, per-type charges; ew_stride:
    // k cells per chain in d_ew_S = the largest half box of the uploaded batch (ewald_dev.h), [n_cfg][ew_stride + EW_EXTRA] double2
    // (vssr_batch_upload is the only writer of d_cell on a handle with k-space: vssr_batch_relax_cell, which changes the cells of the
    // resident chains on the device, refuses such a handle with VSSR_E_STATE -- serving it means recomputing ew_stride and re-sizing
    // d_ew_S as the upload does, a follow-up; vssr_batch_md_npt refuses a barostat there likewise.  Any other new entry point that changes a cell must do the one or the other; a chain whose
    // half box exceeds the stride gets NaN results from the kernels, never a partial sum)
    bool ew_on = false;
    double ew_g = 0, ew_kcut = 0, ew_q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double ew_slab = 0;   // vssr_pair_create_kspace_slab: the factor F of the extended cell (a, b, F c); 0: three periodic axes
    int ew_stride = 0;
    vssr::DevBuf d_ew_S;
    vssr::DevBuf pot_params;     // Tersoff: double[nt^3][14]; SW: SwP[nt^3] (sw_dev.h); EAM: spline tables (eam.hip); pair: PairTable (pair_dev.h)

    // resident batch
    bool batch_valid = false, ran = false;
    int n_cfg = 0, n_atoms = 0;
    std::vector<int> h_n_atoms, h_cfg_start;
    vssr::DevBuf d_pos, d_wpos, d_wrap, d_Z, d_atom_cfg, d_cfg_start, d_cell, d_invcell, d_nimg, d_pbc;
    vssr::DevBuf d_deg, d_row_start, d_edge, d_edge_S, d_rev, d_counters, d_tile_sums;
    vssr::DevBuf d_erec, d_rho, d_dist, d_rho16, d_drho16, d_zslot, d_bundle, d_excl;
    vssr::DevBuf d_bundle_sub;   // [2][n_atoms] per-pass bundle tables of the two-pass forward neighbor sum (chains of the 4-feature class)
    int bwd_multi_pass = 1;      // VSSR_EDGE_BWD_MPASS=0: chains of > 557 atoms take the 8- / 4-feature reverse kernels (round 4) instead of the
                                 // 16-feature kernel in several passes; 2: every chain of the matrix-pipe classes takes the multi-pass form (tests)
    int sub_chunk_fwd = 0, sub_chunk_bwd = 0;   // VSSR_EDGE_SUB_CHUNK=n (tests): atoms per neighbor sub-range instead of what LDS holds
    vssr::DevBuf d_bundle_subb;  // per-pass bundle tables of the reverse multi-pass form (its ranges are larger than the forward's)
    int fwd_two_pass = 16;       // VSSR_EDGE_FWD_2PASS = 0 | 8 | 16: chains of 788 .. 1 462 atoms take the 4-feature forward kernel, or the 8- / 16-feature
                                 // kernel in several passes over neighbor sub-ranges
    int edge_fwd_grid = -1;      // VSSR_EDGE_FWD_GRID=n: workgroups of the persistent 16-wave forward neighbor sum (edge_mfma_init: the CU count,
                                 // or n capped by it; a multiple of 8 is used); 0: one item per workgroup
    vssr::DevBuf d_hits;        // neighbor search: per (centre, candidate) 64-bit hit masks of the counting pass
    // layer-0 species factorisation (painn_l0.hip)
    int l0_enabled = 1, l0_nz = 0;
    bool l0_used = false;                // last run used the factorised layer 0
    vssr::DevBuf d_l0A, d_l0At;          // [M][n_embed][2][24][F] and [M][n_embed][2][F][24], built at create
    vssr::DevBuf d_zmap, d_zlist;        // species index of Z (or -1), distinct Z of the resident batch
    vssr::DevBuf d_l0T, d_l0Q;
    // relaxations (relax.hip, relax_cg.hip, chain_min.hip); d_opt_state / d_opt_vec: handed out typed by FireWork / BfgsWork / CgWork only
    vssr::DevBuf d_opt_state, d_opt_vec, d_bfgs_q, d_bfgs_b, d_fixed, d_relax_steps, d_relax_conv, d_active;
    const unsigned char *active_mask = nullptr;   // set by the lock-step drivers for the duration of a relaxation
    int relax_regrows = 0;
    long long relax_lockstep = 0;   // lock-step evaluations of the batch launched by the last relaxation (vssr_batch_relax_counts)
    int relax_compactions = 0;      // live-chain compactions of the last CG relaxation
    vssr::DevBuf d_cmp;            // arena of the live-chain compaction (Compactor, relax_cg.hip)
    vssr::DevBuf d_cm;             // flags + per-chain evaluation counters of the chain-resident minimiser (chain_min.hip)
    long long relax_chain_evals = 0;   // chain-evaluations those launches actually dispatched (live-chain compaction: < lockstep x B)
    // trajectory recording of the lock-step relaxations (relax.hip k_traj_record): every traj_interval optimizer steps
    int traj_interval = 0, traj_records = 0, traj_B = 0, traj_N = 0;
    vssr::DevBuf d_traj_pos, d_traj_f, d_traj_e, d_traj_n;
    bool graph_partial = false;   // the resident neighbor graph / activations cover only the chains of the last relaxation iteration
    bool l0T_by_geom = false;     // this evaluation's layer-0 T blocks were written by k_edge_geom (<= 4 species)
    int64_t zero_entry_cap = -1;  // capacity / table addresses for which the all-zero table entries were last cleared
    const void *zero_entry_tab[2] = {nullptr, nullptr};
    int cap_per_atom = 64;        // initial neighbor capacity (slots per atom); vssr_debug_capacity
    int cm_cap_per_atom = 0;      // slots per atom the chain-resident CG minimiser's per-chain pools grew to (chain_min.hip)
    int cg_driver = 0;            // VSSR_CG_DRIVER_*: the handle's choice of CG driver (vssr_batch_relax_cg_driver; 0 = automatic)
    int cg_last_driver = 0;       // the driver the last vssr_batch_relax_cg ran: 0 none yet, 1 lock-step, 2 chain-resident
    bool cap_tight = false;       // regrow to the exact need only (tests: forces repeated overflows)
    // molecular dynamics (md.hip): the velocities stay resident between calls and are void after vssr_batch_upload
    vssr::DevBuf d_md_vel;        // [sum N][3] double, A / fs
    vssr::DevBuf d_md_aux;        // stop counters | chain ids [B] | thermo records (MdWork, md.hip)
    bool md_vel_valid = false;
    int md_driver = 0;            // VSSR_MD_DRIVER_*: the handle's choice of MD driver (vssr_batch_md_driver; 0 = automatic)
    int md_last_driver = 0;       // the driver the last vssr_batch_md ran: 0 none yet, 1 lock-step, 2 chain-resident
    vssr::DevBuf d_vib;           // harmonic vibrations (vib.hip): the call's workspace (VibWork)
    vssr::DevBuf d_neb;           // nudged elastic band (neb.hip): NEB forces, per-image partial sums, band records (NebWork)
    vssr::DevBuf d_dimer;         // dimer method (dimer.hip): modes, kept forces, FIRE state, per-dimer records (DimerWork)
    vssr::DevBuf d_npt;           // constant-pressure MD (md_npt.hip): pre-step copies, masses, thermo records, per-chain state (NptWork)
    vssr::DevBuf d_cellrelax;     // variable-cell relaxation (relax_cell.hip): reference positions, velocities, per-chain state (CellWork)
    uint32_t last_want = 0;                       // outputs produced by the last run
    int64_t slot_cap = 0;
    vssr::PinnedInts h_counters; // pinned: [0] total slots, [1] total real edges, [2] overflow flag

    // state
    vssr::DevBuf d_state;        // one arena for all activations
    vssr::StateView sv;
    vssr::DevBuf d_gbar;
    vssr::DevBuf d_upd_save;     // forward intermediates of every update block for the reverse pass (update_save_bytes per layer)
    // Edge gradients: d_gbar is the final buffer, [M][slot_cap] float4.  Layer 0 and the gather kernels write it directly.  The matrix-pipe
    // reverse kernels (layers >= 1) write 12-byte partial records into d_gpart, [M][groups][slot_cap][3] floats with groups = (num_conv - 1)
    // layer sets x the slices of the narrowest class present; k_reduce_gpart adds them to the final buffer.  d_gpart exists exactly
    // when painn_gbar_groups(h) > 1.
    vssr::DevBuf d_gpart;
    int debug_keep = 0;          // VSSR_DEBUG_KEEP=1: also materialise what only vssr_debug_read looks at (the last block's vector output)
    int upd_save = 0;            // VSSR_UPD_SAVE=1: update_fwd stores its intermediates and the reverse kernel loads them instead of
                                 // recomputing (measured: update_bwd 2.45 -> 2.21, update_fwd 1.30 -> 1.57..1.60 ms / step: no gain;
                                 // profiles/r03/NOTES_node_kernels.md)
    // results (device)
    vssr::DevBuf d_energy, d_energy_std, d_energy_models, d_forces, d_forces_std, d_e_atoms;
    vssr::DevBuf d_energy64;   // double [B] E | [B] sigma_E | [B][M] per model: the results before narrowing to float32
    vssr::DevBuf d_pot_e, d_pot_ea, d_pot_f;   // fp64 results of the analytic potentials: energies [B], per atom [N], forces [N][3]
    vssr::DevBuf d_sat, d_sat_out;   // [n_cfg] unsigned: saturation flags raised during a run / reported for the last evaluation of every chain
    std::vector<unsigned> h_sat;     // host copy of d_sat_out taken by vssr_batch_download (vssr_batch_saturated serves it: no second
    bool h_sat_valid = false;        // synchronisation / copy per download, advisor r3); void after every run
    vssr::DevBuf d_stress;           // [2][n_cfg][6] double: virial stress (mean, std over models) of the last evaluation (vssr_batch_stress)

    // Gaussian mixture (Kind::GMM, gmm.hip): K components of dimension D, zero-padded to Dp = 16 ceil(D / 16)
    int gmm_K = 0, gmm_D = 0, gmm_Dp = 0;
    double gmm_log2pi = 0.0;
    vssr::DevBuf d_gmm_P;     // double [K][Dp][Dp]  precision Cholesky factors
    vssr::DevBuf d_gmm_c;     // double [K][Dp]      c_k = mu_k P_k
    vssr::DevBuf d_gmm_kc;    // double [2][K]       log det P_k, log w_k
    vssr::DevBuf d_gmm_mask;  // uint8 [K][Dp/16][Dp/16]  1 = the 16 x 16 block of P_k holds a non-zero entry
    vssr::DevBuf d_gmm_x, d_gmm_lp, d_gmm_nll, d_gmm_sys, d_gmm_start;   // per-call workspaces
    std::unique_ptr<vssr::GmmFit> fit;    // GMM_FIT and CLUSTER (CLUSTER: the resident rows only)
    std::unique_ptr<vssr::Cluster> clu;   // CLUSTER only
};

namespace vssr {

int set_err(vssr_handle *h, int code, const char *fmt, ...);   // h == nullptr: the per-thread error of the create functions
#define VSSR_HIP(h, expr)                                                                    \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return vssr::set_err(h, VSSR_E_DEVICE, "%s failed: %s (%s:%d)", #expr,          \
                                 hipGetErrorString(_e), __FILE__, __LINE__);                 \
    } while (0)

// ---- handle lifecycle and what the api_*.hip files share (api_handle.hip) ----
// Entry-point guard: VSSR_E_BADARG for a null handle or one whose kind is not in `served` (kind_bit set), with the message the
// entry point's family gives ("<func>: a ... handle serves the ... calls only" / "not a ... handle"); VSSR_OK otherwise.
int check_kind(vssr_handle *h, unsigned served, const char *func);
// The device part of a create, in two steps: device count and range; then current device, stream, pinned counters.  Errors go to h->err.
int device_in_range(vssr_handle *h, int device);
int open_device(vssr_handle *h, int device);
void publish_create_error(const vssr_handle *h);   // a non-empty h->err into the per-thread error vssr_last_error(NULL) reads
// One create path: a new handle of `kind` on `device`, then init(h); on failure the error is published, the handle destroyed
// and the code returned.  Arguments that can be refused without a device are checked by the caller first.  range_check = false:
// vssr_gmm_create has always left a bad device to hipSetDevice (VSSR_E_DEVICE), and keeps doing so.
template <class Init>
int create_handle(Kind kind, int device, vssr_handle **out, Init init, bool range_check = true) {
    vssr_handle *h = new vssr_handle();
    h->kind = kind;
    int rc = range_check ? device_in_range(h, device) : VSSR_OK;
    if (!rc) rc = open_device(h, device);
    if (!rc) rc = init(h);
    if (rc) {
        publish_create_error(h);
        vssr_destroy(h);
        return rc;
    }
    *out = h;
    return VSSR_OK;
}
int run_any(vssr_handle *h, uint32_t want);
int sync_and_check(vssr_handle *h);   // synchronise; if the neighbor capacity overflowed, grow and rerun
int grow_slot_cap(vssr_handle *h);    // slot_cap for the rerun after an overflow, from the slots the build counted (h_counters[0])

// neighbor list (nbr.hip)
int build_neighbors(vssr_handle *h, double cutoff);
// PaiNN pipeline (painn.hip)
int painn_alloc_state(vssr_handle *h);
int painn_run(vssr_handle *h, uint32_t want);
int painn_stress(vssr_handle *h);   // enqueues k_stress: d_stress from the edge gradients of the last run (forces wanted)
int painn_alloc_results(vssr_handle *h);   // result buffers and saturation flags (both PaiNN paths)
// energy reduction and force assembly from sv.e_atom / sv.gbar (one reduced edge-gradient buffer per model, stride slot_cap): both paths
void painn_finalize(vssr_handle *h, const GraphView &G, uint32_t want);
GraphView graph_view(const vssr_handle *h);   // every table of the resident neighbor graph (null where the path built none) + the active mask
// general-width PaiNN path (painn_gen.hip): weights of any accepted (feat_dim, n_rbf), and the run
int painn_gen_upload(vssr_handle *h, const vssr_painn_config *cfg);
int painn_gen_run(vssr_handle *h, uint32_t want);
// Tersoff (tersoff.hip)
int tersoff_run(vssr_handle *h, uint32_t want);
// EAM (eam.hip)
int eam_run(vssr_handle *h, uint32_t want);
// ADP (adp.hip): what eam_run / eam_stress do for a handle with eam_adp
int adp_run(vssr_handle *h, uint32_t want);
int adp_stress(vssr_handle *h);
// Stillinger-Weber (sw.hip)
int sw_run(vssr_handle *h, uint32_t want);
// pair potentials (pair.hip)
int pair_run(vssr_handle *h, uint32_t want);
// Vashishta (vashishta.hip)
int vashishta_run(vssr_handle *h, uint32_t want);
// Gaussian-mixture scoring (gmm.hip).  Rows: caller fp64 rows [n][Dp] (padded), or fp32 rows with leading dimension ldx = Dp;
// writes g->d_gmm_lp [n][K] (logp_k) and g->d_gmm_nll [n] on stream st
int gmm_upload(vssr_handle *g, const double *means, const double *prec_chol, const double *weights);
int gmm_score_f64(vssr_handle *g, hipStream_t st, int64_t n, const double *x_dev);
int gmm_score_f32(vssr_handle *g, hipStream_t st, int64_t n, const float *x_dev);
// per-structure mean rows of fp32 features [N][D] into g->d_gmm_x ([B][Dp]); start: device [B + 1] atom offsets
int gmm_mean_rows(vssr_handle *g, hipStream_t st, int B, const int *start, const float *emb);
// per-structure reductions of g->d_gmm_nll (order 1 .. 6 as vssr_gmm_score_batch) into g->d_gmm_sys [B]
int gmm_reduce(vssr_handle *g, hipStream_t st, int B, const int *start, int order);
// Gaussian-mixture fit (gmm_fit.hip): EM on the rows resident in h->fit->rows; the device is initialised by the caller (api_gmm.hip)
int gmm_fit_check_config(const vssr_gmm_fit_config *cfg);
int gmm_fit_append_host(vssr_handle *h, int64_t n_rows, const double *x);
int gmm_fit_append_f32(vssr_handle *h, hipStream_t st, int64_t n_rows, const float *emb_dev);   // device rows [n][D] fp32
int gmm_fit_append_f64p(vssr_handle *h, hipStream_t st, int64_t n_rows, const double *x_dev);   // device rows [n][Dp] fp64
int gmm_fit_set_init(vssr_handle *h, const double *means, const double *weights, const double *precisions, const int32_t *labels);
int gmm_fit_run(vssr_handle *h, vssr_gmm_fit_result *res);
int gmm_fit_params(vssr_handle *h, double *weights, double *means, double *covariances, double *prec_chol);
int gmm_fit_copy_scorer(vssr_handle *h, vssr_handle *g);   // the fitted mixture into the scoring buffers of a Kind::GMM handle
// cov [Dp][Dp] = sum_n (x_n - mean)(x_n - mean)^T / denom[0] on the fit's row-slab MFMA kernel (mean [Dp], denom [1]: device)
int gmm_fit_centered_cov(vssr_handle *h, hipStream_t st, const double *X, int n, int D, int Dp, const double *mean, const double *denom,
                         DevBuf &part, double *cov);
// Latent-space clustering (cluster.hip): PCA of the rows resident in h->fit->rows, Ward linkage of the resident points
int cluster_pca(vssr_handle *h, vssr_cluster_pca_result *res);
int cluster_pca_params(vssr_handle *h, double *mean, double *components, double *explained_variance, double *ratio);
int cluster_projected(vssr_handle *h, int64_t first, int64_t n_rows, double *xr);
int cluster_set_points(vssr_handle *h, int64_t n, const double *pts);
int cluster_linkage(vssr_handle *h, double *Z, int32_t *n_rounds);
int cluster_pad_dims(int d);   // stored width of a point: 1, 2, 3, 4, 8, 16 or 32 coordinates
// vssr_batch_stress on the analytic potentials: enqueue the virial kernel over what the last run left on the device (d_stress, as
// painn_stress); nothing of it runs unless asked for.  (The pieces the analytic potentials share are declared in pot_dev.h.)
int tersoff_stress(vssr_handle *h);
int eam_stress(vssr_handle *h);
int sw_stress(vssr_handle *h);
struct PotView;
void ewald_run(vssr_handle *h, const PotView &V);   // ewald.hip: reciprocal, self and background terms added to d_pot_ea / d_pot_f
int ewald_stress(vssr_handle *h);                   // their virial added to d_stress
int pair_stress(vssr_handle *h);   // runs the site kernel's gradient form first: a plain evaluation keeps no per-slot gradients
int vashishta_stress(vssr_handle *h);   // likewise: a plain evaluation keeps the three-body gradients of the short slots only
// What differs between the kinds that evaluate a batch, one row per Kind (api_handle.hip); run == nullptr: the kind evaluates nothing.
// f64: an analytic potential -- results in d_pot_e / _ea / _f (fp64, one "model"), driven by relax_cg / chain_min as well.
struct Evaluator {
    bool f64;
    int (*run)(vssr_handle *h, uint32_t want);
    int (*stress)(vssr_handle *h);
    double (*cutoff)(const vssr_handle *h);
};
const Evaluator &evaluator(const vssr_handle *h);
inline bool is_analytic(const vssr_handle *h) { return evaluator(h).f64; }
// What an evaluation of the handle fills, for the drivers behind it: the fp64 energy per chain (the potential's, or PaiNN's ensemble
// mean) and the forces -- fp64 of an analytic potential, PaiNN's fp32.  fn(const double *energy, const FT *forces), FT = double | float.
inline const double *chain_energy64(const vssr_handle *h) { return is_analytic(h) ? h->d_pot_e.as<double>() : h->d_energy64.as<double>(); }
template <class Fn>
void with_forces(const vssr_handle *h, Fn fn) {
    if (is_analytic(h)) fn(chain_energy64(h), (const double *)h->d_pot_f.as<double>());
    else fn(chain_energy64(h), (const float *)h->d_forces.as<float>());
}
template <class P>
using force_type = std::remove_cv_t<std::remove_pointer_t<P>>;   // FT of a `forces` argument, for a kernel's template argument
void eam_build_spline(const double *f, int n, double delta, double *spl /*[n + 1][7]*/);
// lock-step FIRE / BFGS relaxation (relax.hip, relax_lockstep<FireWork | BfgsWork>); results in d_relax_steps [B], d_relax_conv [B]; fixed_host may be null
int relax_fire(vssr_handle *h, const vssr_fire_params &p, const uint8_t *fixed_host, uint32_t want);
int relax_bfgs(vssr_handle *h, const vssr_bfgs_params &p, const uint8_t *fixed_host, uint32_t want);
// The frame of a driver call (relax.hip).  driver_guard: first in every entry point -- the handle's kind, then "<func> before
// vssr_batch_upload".  driver_open: behind the last argument check, so that a refused call leaves the handle as it was -- the
// per-relaxation buffers, the mask (-> fixed), the work and regrow counters at zero, last_want = want | forces.  driver_close: the batch
// holds a finished evaluation (partial: of the chains of the last iteration only, or numbered per chain) -- ran, graph_partial,
// sync_and_check (that evaluation may itself have overflowed the capacity: grow and repeat it).
int driver_guard(vssr_handle *h, const char *func);
int driver_open(vssr_handle *h, const uint8_t *fixed_host, int steps_ints_per_chain, const uint8_t *&fixed, uint32_t want);
int driver_close(vssr_handle *h, bool partial);
int relax_regrow(vssr_handle *h, int cap, long long &it, int window);   // after an overflow seen at a poll: grow, give the poll window back
// the tail of a driver's entry point: driver_close, the positions, and d_relax_steps [B][k] de-interleaved into its k columns (null: not wanted)
int relax_results(vssr_handle *h, bool partial, double *pos_out, std::initializer_list<int32_t *> cols);
// lock-step LAMMPS-style CG for the fp64 potentials (relax_cg.hip); results in d_relax_steps [B][3] = {iterations, evaluations, stop reason}
int relax_cg(vssr_handle *h, const vssr_cg_params *cp, const uint8_t *fixed_host, uint32_t want);
// lock-step BFGSLineSearch on every kind that relaxes (relax_bfgsls.hip, bfgsls_dev.h); results in d_relax_steps [B][3] = {steps, evaluations, stop reason}
int relax_bfgsls(vssr_handle *h, const vssr_bfgsls_params *bp, const uint8_t *fixed_host, uint32_t want);
// chain_min.hip: the same minimisation with one workgroup per chain (Tersoff / SW / EAM / pair handles, chains of <= 256 atoms).
// chain_min_supported: this relaxation takes it (the kernel applies AND VSSR_CG_FUSED / the handle's cg_driver / the automatic rule say so)
bool chain_min_supported(const vssr_handle *h);
int chain_min_cg(vssr_handle *h, const vssr_cg_params *cp, const uint8_t *fixed_host, uint32_t want);
// MFMA node stages (painn_node_mfma.hip)
int node_mfma_init(vssr_handle *h);
void launch_msg_mlp_mfma(hipStream_t st, int N, int M, int l, const ActiveView &av, const ModelW *MW, const float *s_in,
                         float *phi);
void launch_msg_mlp_bwd_mfma(hipStream_t st, int N, int M, int l, const ActiveView &av, const ModelW *MW, const float *s_in,
                             const float *phibar, const float *sbar_msg, float *sbar_in);
void launch_update_fwd_mfma(hipStream_t st, int N, int M, int l, const ActiveView &av, const ModelW *MW, const float *s_msg,
                            const float *v_msg, float *s_out, float *v_out, float *phi_next, void *save);
size_t update_save_bytes(int N, int M);   // per layer: forward intermediates of the update block kept for its reverse
bool readout_mfma_supported(int hidden);
void launch_readout_mfma(hipStream_t st, int N, int M, const ActiveView &av, const ModelW *MW, const float *s, const float *e_excl,
                         float *e_atom);
void launch_update_bwd_mfma(hipStream_t st, int N, int M, int l, int mode, int vbar_is_zero, const ActiveView &av, const ModelW *MW,
                            const float *s_msg, const float *v_msg, const float *sbar_src, const float *vbar,
                            const float *s_next, const float *phibar, const float *e_excl, float *e_atom,
                            float *sbar_msg, float *vbar_msg, float *s_last, const void *save);
// layer-0 species factorisation (painn_l0.hip)
void pack_mfma_tiles16(const float *Wsrc, int rows, int K, unsigned *dst /*[rows/32][K/16][2][64][4]*/);
void build_wd16(const float *Wd, const float *bd, unsigned *dst /*[3F][4][2][4]*/);
void l0_build_tables(const float *blob_embed, const float *W1, const float *b1, const float *W2, const float *b2,
                     const float *Wd, const float *bd, int n_embed, float *A, float *At);
void l0_pack_tables(const float *A, int n_embed, unsigned *A16, unsigned *At16);
size_t l0_packed_dwords(int n_embed);
int l0_mfma_init(vssr_handle *h);
int l0_run_forward(vssr_handle *h, const GraphView &G, float *s_msg, float *v_msg);
// fresh_mfma: chains of the matrix-pipe classes have nothing in the final buffer yet (overwrite), gather-class chains accumulate
int l0_run_reverse(vssr_handle *h, const GraphView &G, int first_write, int fresh_mfma, const float *sbar_msg, const float *vbar_msg,
                   float4 *gbar);
// LDS-slice + MFMA edge stages (painn_edge_mfma.hip)
int edge_mfma_init(vssr_handle *h);
// forward neighbor-sum paths: 16-feature slices with / without the scalar residual in LDS, 8- and 4-feature slices, gather kernels
enum { EDGE_CLASS_FS16 = 0, EDGE_CLASS_FS16M = 1, EDGE_CLASS_FS8 = 2, EDGE_CLASS_FS4 = 3, EDGE_CLASS_GATHER = 4, EDGE_CLASSES = 5,
       EDGE_MFMA_CLASSES = 4 };
// reverse paths (the reverse tile is smaller: 16-feature slices serve chains up to 557 atoms): what GraphView::chain_class holds
// (FS16P: 16-feature slices in several passes over neighbor sub-ranges -- chains beyond the 557 atoms of the single-pass form, round 5)
enum { EDGE_BCLASS_FS16 = 0, EDGE_BCLASS_FS8 = 1, EDGE_BCLASS_FS4 = 2, EDGE_BCLASS_FS16P = 3, EDGE_BCLASS_GATHER = 4, EDGE_BCLASSES = 5,
       EDGE_MFMA_BCLASSES = 4 };
// partial edge-gradient buffers (feature slices) a chain of reverse class c writes per layer set and model
__host__ __device__ constexpr int edge_bclass_slices(int c) { return (c == EDGE_BCLASS_FS16 || c == EDGE_BCLASS_FS16P) ? 8 : c == EDGE_BCLASS_FS8 ? 16 : c == EDGE_BCLASS_FS4 ? 32 : 1; }
int edge_bclass_of(int n_atoms);
int edge_class_of(int n_atoms);       // path of a chain by its own atom count
// multi-pass forward neighbor sum (chains of the 4-feature class): the chain's atoms in P equal ranges of at most chunk_max atoms
constexpr int SUB_MAX_PASSES = 4;
__host__ __device__ constexpr int sub_chunk_max(int width) { return width == 16 ? 400 : 784; }   // staged rows that fit 160 KB (400 / 208 B per row) minus the zero row
__host__ __device__ constexpr int sub_chunk_max_bwd() { return 550; }   // reverse tile: 272 B per row + the current-centre records (12 KB) in 160 KB, minus the zero row
__host__ __device__ constexpr int sub_passes(int n_atoms, int chunk_max) { return (n_atoms + chunk_max - 1) / chunk_max; }
__host__ __device__ constexpr int sub_chunk(int n_atoms, int chunk_max) { return (n_atoms + sub_passes(n_atoms, chunk_max) - 1) / sub_passes(n_atoms, chunk_max); }
int edge_class_groups(int cls);       // partial edge-gradient buffers a chain of that class writes per model
// gpart: the partial 12-byte records [M][n_groups][slot_cap][3]; this launch writes groups group_off .. group_off + slices - 1
void launch_edge_bwd_mfma(hipStream_t st, int cls, int N, const int *list, int n_list, int M, int l, int max_atoms,
                          const ModelW *MW, const GraphView &G, const int *counters, int zero_slot,
                          const float *v_in, const float *phi, const float *sbar_msg, const float *vbar_msg,
                          float *phibar, float *vbar_in, float *gpart, long long slot_cap, int n_groups, int group_off,
                          const int4 *bundle_sub, int sub_chunk);
void launch_edge_fwd_mfma(hipStream_t st, int cls, int N, const int *list, int n_list, int M, int l, int max_atoms, const ModelW *MW,
                          const GraphView &G, const int *counters, int zero_slot, const float *s_in, const float *v_in,
                          const float *phi, float *s_msg, float *v_msg, const int4 *bundle_sub, int sub_width, int sub_chunk,
                          int persist_grid);   // persist_grid: vssr_handle::edge_fwd_grid

}  // namespace vssr
