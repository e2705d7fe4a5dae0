// api_batch.hip — the resident batch: upload, run, download, the relaxation entry points and introspection.
#include <cmath>
#include <cstdio>

#include "cell_dev.h"
#include "ewald_dev.h"

using namespace vssr;

extern "C" {

int vssr_batch_upload(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *Z, const double *pos,
                      const double *cell, const uint8_t *pbc) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (n_cfg < 1 || !n_atoms || !Z || !pos || !cell || !pbc) return set_err(h, VSSR_E_BADARG, "null or empty batch");
    VSSR_HIP(h, hipSetDevice(h->device));
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    h->batch_valid = false;
    h->ran = false;
    h->md_vel_valid = false;   // (velocities belong to the batch they were set for)
    std::vector<int> start(n_cfg + 1, 0);
    for (int b = 0; b < n_cfg; ++b) {
        if (n_atoms[b] < 1) return set_err(h, VSSR_E_BADARG, "configuration %d has %d atoms", b, n_atoms[b]);
        if ((int64_t)start[b] + n_atoms[b] > 2000000000LL) return set_err(h, VSSR_E_BADARG, "batch too large");
        start[b + 1] = start[b] + n_atoms[b];
    }
    const int N = start[n_cfg];
    std::vector<int> atom_cfg(N);
    for (int b = 0; b < n_cfg; ++b)
        for (int i = start[b]; i < start[b + 1]; ++i) atom_cfg[i] = b;
    for (int i = 0; i < N; ++i)
        if (Z[i] < 0 || Z[i] >= h->n_embed)
            return set_err(h, VSSR_E_BADARG, "atom %d: species index %d outside [0,%d)", i, Z[i], h->n_embed);
    for (size_t t = 0; t < (size_t)3 * N; ++t)
        if (!std::isfinite(pos[t])) return set_err(h, VSSR_E_BADARG, "non-finite position");
    std::vector<double> inv((size_t)9 * n_cfg);
    std::vector<int> nimg((size_t)3 * n_cfg);
    const double rc = evaluator(h).cutoff(h);
    for (int b = 0; b < n_cfg; ++b) {
        bool ok;
        cell_setup(cell + 9 * b, pbc + 3 * b, rc, inv.data() + 9 * b, nimg.data() + 3 * b, ok);
        if (!ok) return set_err(h, VSSR_E_BADARG, "configuration %d: periodic but singular cell", b);
        for (int k = 0; k < 3; ++k)
            if (nimg[3 * b + k] > 100) {
                // (a pair handle's cutoff is the caller's choice: its refusal says what was exceeded, with the capacity code)
                if (h->kind == Kind::PAIR)
                    return set_err(h, VSSR_E_CAPACITY, "configuration %d: the %g A cutoff needs %d periodic images along axis %d, the neighbor "
                                   "search scans at most 100 on either side (nothing is truncated: shorten the cutoff or repeat the cell)",
                                   b, rc, nimg[3 * b + k], k);
                return set_err(h, VSSR_E_BADARG, "configuration %d: cell too thin for the cutoff", b);
            }
        const long long imgs = (2LL * nimg[3 * b] + 1) * (2 * nimg[3 * b + 1] + 1) * (2 * nimg[3 * b + 2] + 1);
        if (b == 0 || imgs > h->max_images) h->max_images = (int)(imgs > 1000000 ? 1000000 : imgs);
    }
    if (h->ew_on) {   // the k sphere of every chain from its own cell (ewald_dev.h): capacity, and the stride of the S(k) array
        long long stride = 0;
        const bool slab = h->ew_slab > 0;
        for (int b = 0; b < n_cfg; ++b) {
            const double *c = cell + 9 * b;
            if (slab) {   // pbc 1 1 0, a and b in the plane, c along z, the atoms within |c| along z (of these positions: later moves are not re-checked)
                if (!(pbc[3 * b] && pbc[3 * b + 1] && !pbc[3 * b + 2]))
                    return set_err(h, VSSR_E_BADARG, "configuration %d: a slab Ewald sum needs pbc 1 1 0 (pbc %d %d %d)", b, (int)pbc[3 * b],
                                   (int)pbc[3 * b + 1], (int)pbc[3 * b + 2]);
                const double len = std::sqrt(c[6] * c[6] + c[7] * c[7] + c[8] * c[8]), tol = 1e-12 * len;
                if (std::fabs(c[2]) > tol || std::fabs(c[5]) > tol || std::fabs(c[6]) > tol || std::fabs(c[7]) > tol)
                    return set_err(h, VSSR_E_BADARG, "configuration %d: a slab Ewald sum needs a and b in the xy plane and c along z (a_z %g, b_z %g, "
                                   "c_x %g, c_y %g)", b, c[2], c[5], c[6], c[7]);
                double lo = pos[3 * (size_t)start[b] + 2], hi = lo;
                for (int i = start[b]; i < start[b + 1]; ++i) {
                    lo = std::min(lo, pos[3 * (size_t)i + 2]);
                    hi = std::max(hi, pos[3 * (size_t)i + 2]);
                }
                if (hi - lo > len)
                    return set_err(h, VSSR_E_BADARG, "configuration %d: the atoms span %g A along z, more than |c| = %g A: the extended cell of "
                                   "%g A would not keep its vacuum", b, hi - lo, len, h->ew_slab * len);
            } else if (!(pbc[3 * b] && pbc[3 * b + 1] && pbc[3 * b + 2]))
                return set_err(h, VSSR_E_BADARG, "configuration %d: an Ewald sum needs three periodic axes (pbc %d %d %d; no slab correction)", b,
                               (int)pbc[3 * b], (int)pbc[3 * b + 1], (int)pbc[3 * b + 2]);
            EwaldGeom G;
            ewald_geom(c, h->ew_kcut, 1e-9, G, h->ew_slab);
            char ext[96] = "";
            auto name_extended = [&] {   // (refusal paths only) a slab handle: the capacity refusals name the extended length F |c|
                if (slab)
                    snprintf(ext, sizeof ext, " of the cell extended to %g A (slab factor %g)",
                             h->ew_slab * std::sqrt(c[6] * c[6] + c[7] * c[7] + c[8] * c[8]), h->ew_slab);
            };
            for (int k = 0; k < 3; ++k)
                if (G.m[k] > EW_MAX_INDEX) {
                    name_extended();
                    return set_err(h, VSSR_E_CAPACITY, "configuration %d: k_cut %g 1/A needs the reciprocal index %d along axis %d%s, the k-space "
                                   "kernels hold %d at the most (nothing is truncated: lower k_cut with a larger real-space cutoff)",
                                   b, h->ew_kcut, G.m[k], k, ext, EW_MAX_INDEX);
                }
            if (G.cells > EW_MAX_CELLS) {
                name_extended();
                return set_err(h, VSSR_E_CAPACITY, "configuration %d: k_cut %g 1/A needs a box of %lld reciprocal vectors%s, the k-space kernels hold "
                               "%d at the most (nothing is truncated: lower k_cut with a larger real-space cutoff)", b, h->ew_kcut, G.cells,
                               ext, EW_MAX_CELLS);
            }
            stride = std::max(stride, G.cells);
        }
        h->ew_stride = (int)stride;
        if (h->d_ew_S.ensure(sizeof(double) * 2 * (size_t)n_cfg * (size_t)(stride + EW_EXTRA)))
            return set_err(h, VSSR_E_NOMEM, "k-space structure factors: out of device memory");
    }
    if (h->d_pos.ensure(sizeof(double) * 3 * N) || h->d_Z.ensure(sizeof(int) * N) ||
        h->d_atom_cfg.ensure(sizeof(int) * N) || h->d_cfg_start.ensure(sizeof(int) * (n_cfg + 1)) ||
        h->d_cell.ensure(sizeof(double) * 9 * n_cfg) || h->d_invcell.ensure(sizeof(double) * 9 * n_cfg) ||
        h->d_nimg.ensure(sizeof(int) * 3 * n_cfg) || h->d_pbc.ensure((size_t)3 * n_cfg))
        return set_err(h, VSSR_E_NOMEM, "batch buffers: out of device memory");
    VSSR_HIP(h, hipMemcpy(h->d_pos.p, pos, sizeof(double) * 3 * N, hipMemcpyHostToDevice));
    VSSR_HIP(h, hipMemcpy(h->d_Z.p, Z, sizeof(int) * N, hipMemcpyHostToDevice));
    VSSR_HIP(h, hipMemcpy(h->d_atom_cfg.p, atom_cfg.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    VSSR_HIP(h, hipMemcpy(h->d_cfg_start.p, start.data(), sizeof(int) * (n_cfg + 1), hipMemcpyHostToDevice));
    VSSR_HIP(h, hipMemcpy(h->d_cell.p, cell, sizeof(double) * 9 * n_cfg, hipMemcpyHostToDevice));
    VSSR_HIP(h, hipMemcpy(h->d_invcell.p, inv.data(), sizeof(double) * 9 * n_cfg, hipMemcpyHostToDevice));
    VSSR_HIP(h, hipMemcpy(h->d_nimg.p, nimg.data(), sizeof(int) * 3 * n_cfg, hipMemcpyHostToDevice));
    VSSR_HIP(h, hipMemcpy(h->d_pbc.p, pbc, (size_t)3 * n_cfg, hipMemcpyHostToDevice));
    h->n_cfg = n_cfg;
    h->n_atoms = N;
    if (h->kind == Kind::PAINN) {   // species present in this batch (layer-0 factorisation works per neighbor species)
        std::vector<int> zmap(h->n_embed, -1), zlist;
        for (int i = 0; i < N; ++i)
            if (zmap[Z[i]] < 0) { zmap[Z[i]] = 1; }
        for (int z = 0; z < h->n_embed; ++z)
            if (zmap[z] > 0) { zmap[z] = (int)zlist.size(); zlist.push_back(z); }
        h->l0_nz = (int)zlist.size() <= L0_MAX_SPECIES ? (int)zlist.size() : 0;
        if (h->d_zmap.ensure(sizeof(int) * h->n_embed) || h->d_zlist.ensure(sizeof(int) * (zlist.size() + 1)))
            return set_err(h, VSSR_E_NOMEM, "species tables");
        VSSR_HIP(h, hipMemcpy(h->d_zmap.p, zmap.data(), sizeof(int) * h->n_embed, hipMemcpyHostToDevice));
        VSSR_HIP(h, hipMemcpy(h->d_zlist.p, zlist.data(), sizeof(int) * zlist.size(), hipMemcpyHostToDevice));
    }
    h->max_cfg_atoms = 0;
    for (int b = 0; b < n_cfg; ++b) h->max_cfg_atoms = n_atoms[b] > h->max_cfg_atoms ? n_atoms[b] : h->max_cfg_atoms;
    if (h->kind == Kind::PAINN) {
        // Neighbor-sum path of every chain, from its OWN atom count (so a chain's results do not depend on its batch):
        // 16-, 8- or 4-feature slices, or the gather kernels.  (A batch whose largest chain exceeds what the bundle
        // sort stages in LDS has no bundle tables at all: every chain gathers.)
        const bool bundles = (size_t)h->max_cfg_atoms * sizeof(int) <= 48 * 1024;
        std::vector<unsigned char> bcls(n_cfg);
        std::vector<int> lists[EDGE_MFMA_CLASSES], blists[EDGE_MFMA_BCLASSES];
        for (int c = 0; c < EDGE_CLASSES; ++c) { h->n_class[c] = 0; h->max_class_atoms[c] = 0; }
        for (int c = 0; c < EDGE_BCLASSES; ++c) { h->n_bclass[c] = 0; h->max_bclass_atoms[c] = 0; }
        for (int b = 0; b < n_cfg; ++b) {
            int c = (h->edge_impl && bundles) ? edge_class_of(n_atoms[b]) : EDGE_CLASS_GATHER;
            int bc = (h->edge_impl && bundles) ? edge_bclass_of(n_atoms[b]) : EDGE_BCLASS_GATHER;
            if (c <= EDGE_CLASS_FS16M && h->fs16_max_atoms >= 0 && n_atoms[b] > h->fs16_max_atoms) c = EDGE_CLASS_FS8;
            if (bc == EDGE_BCLASS_FS16 && h->fs16_max_atoms >= 0 && n_atoms[b] > h->fs16_max_atoms) bc = EDGE_BCLASS_FS8;
            if (c == EDGE_CLASS_FS8 && h->fs8_max_atoms >= 0 && n_atoms[b] > h->fs8_max_atoms) { c = EDGE_CLASS_FS4; bc = EDGE_BCLASS_FS4; }
            // the 8-feature forward class (406 .. 787 atoms by the chain's own size) also takes the 16-feature multi-pass form (-9 % against
            // the single-pass 8-feature kernel, profiles/r05/NOTES_large_chains.md); VSSR_EDGE_FWD_2PASS=0 | 8 keeps the 8-feature kernel
            if (h->fwd_two_pass == 16 && c == EDGE_CLASS_FS8 && edge_class_of(n_atoms[b]) == EDGE_CLASS_FS8) c = EDGE_CLASS_FS4;
            // reverse pass of chains beyond the single-pass 16-feature form (by the chain's OWN size, not by a test knob that moved it):
            // the same kernel in several passes over neighbor sub-ranges
            if (bc != EDGE_BCLASS_GATHER && ((h->bwd_multi_pass == 1 && edge_bclass_of(n_atoms[b]) != EDGE_BCLASS_FS16) || h->bwd_multi_pass == 2))
                bc = EDGE_BCLASS_FS16P;
            bcls[b] = (unsigned char)bc;
            h->n_class[c] += 1;
            h->n_bclass[bc] += 1;
            if (n_atoms[b] > h->max_class_atoms[c]) h->max_class_atoms[c] = n_atoms[b];
            if (n_atoms[b] > h->max_bclass_atoms[bc]) h->max_bclass_atoms[bc] = n_atoms[b];
            if (c != EDGE_CLASS_GATHER) lists[c].push_back(b);
            if (bc != EDGE_BCLASS_GATHER) blists[bc].push_back(b);
        }
        std::vector<int> cat;
        for (int c = 0; c < EDGE_MFMA_CLASSES; ++c) cat.insert(cat.end(), lists[c].begin(), lists[c].end());
        for (int c = 0; c < EDGE_MFMA_BCLASSES; ++c) cat.insert(cat.end(), blists[c].begin(), blists[c].end());
        cat.push_back(0);
        const std::vector<unsigned char> &cls = bcls;
        if (h->d_chain_class.ensure((size_t)n_cfg) || h->d_class_list.ensure(sizeof(int) * cat.size()))
            return set_err(h, VSSR_E_NOMEM, "chain class tables");
        VSSR_HIP(h, hipMemcpy(h->d_chain_class.p, cls.data(), (size_t)n_cfg, hipMemcpyHostToDevice));
        VSSR_HIP(h, hipMemcpy(h->d_class_list.p, cat.data(), sizeof(int) * cat.size(), hipMemcpyHostToDevice));
    }
    h->h_n_atoms.assign(n_atoms, n_atoms + n_cfg);
    h->h_cfg_start = start;
    h->batch_valid = true;
    return VSSR_OK;
}

int vssr_batch_set_positions(vssr_handle *h, const double *pos) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->batch_valid) return set_err(h, VSSR_E_STATE, "no resident batch");
    if (!pos) return set_err(h, VSSR_E_BADARG, "null positions");
    VSSR_HIP(h, hipSetDevice(h->device));
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    VSSR_HIP(h, hipMemcpy(h->d_pos.p, pos, sizeof(double) * 3 * h->n_atoms, hipMemcpyHostToDevice));
    h->ran = false;   // results on the device belong to the old positions
    return VSSR_OK;
}

int vssr_batch_run(vssr_handle *h, uint32_t want) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->batch_valid) return set_err(h, VSSR_E_STATE, "vssr_batch_run before vssr_batch_upload");
    VSSR_HIP(h, hipSetDevice(h->device));
    int rc = run_any(h, want);
    if (rc) return rc;
    h->ran = true;
    h->graph_partial = false;
    return VSSR_OK;
}

int vssr_synchronize(vssr_handle *h) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    VSSR_HIP(h, hipSetDevice(h->device));
    return sync_and_check(h);
}

int vssr_batch_download(vssr_handle *h, uint32_t want, vssr_out *out) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran) return set_err(h, VSSR_E_STATE, "vssr_batch_download before vssr_batch_run");
    if (!out) return set_err(h, VSSR_E_BADARG, "null output");
    VSSR_HIP(h, hipSetDevice(h->device));
    if ((want & VSSR_WANT_FORCES) && !(h->last_want & VSSR_WANT_FORCES))
        return set_err(h, VSSR_E_STATE, "forces requested, but the last run was asked for energies only");
    int rc = sync_and_check(h);
    if (rc) return rc;
    const size_t B = h->n_cfg, N = h->n_atoms, M = h->n_models;
    if (is_analytic(h)) {
        std::vector<double> e(B), ea(N), f(3 * N);
        VSSR_HIP(h, hipMemcpy(e.data(), h->d_pot_e.p, sizeof(double) * B, hipMemcpyDeviceToHost));
        if (out->energy) for (size_t b = 0; b < B; ++b) out->energy[b] = (float)e[b];
        if (out->energy_atoms && (want & VSSR_WANT_PER_ATOM)) {
            VSSR_HIP(h, hipMemcpy(ea.data(), h->d_pot_ea.p, sizeof(double) * N, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < N; ++i) out->energy_atoms[i] = (float)ea[i];
        }
        if (out->forces && (want & VSSR_WANT_FORCES)) {
            VSSR_HIP(h, hipMemcpy(f.data(), h->d_pot_f.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < 3 * N; ++i) out->forces[i] = (float)f[i];
        }
        return VSSR_OK;
    }
    if (out->energy) VSSR_HIP(h, hipMemcpy(out->energy, h->d_energy.p, sizeof(float) * B, hipMemcpyDeviceToHost));
    if (out->energy_std && (want & VSSR_WANT_STD))
        VSSR_HIP(h, hipMemcpy(out->energy_std, h->d_energy_std.p, sizeof(float) * B, hipMemcpyDeviceToHost));
    if (out->energy_models && (want & VSSR_WANT_PER_MODEL))
        VSSR_HIP(h, hipMemcpy(out->energy_models, h->d_energy_models.p, sizeof(float) * B * M, hipMemcpyDeviceToHost));
    if (out->energy_atoms && (want & VSSR_WANT_PER_ATOM))
        VSSR_HIP(h, hipMemcpy(out->energy_atoms, h->d_e_atoms.p, sizeof(float) * N, hipMemcpyDeviceToHost));
    if (want & VSSR_WANT_FORCES) {
        if (out->forces) VSSR_HIP(h, hipMemcpy(out->forces, h->d_forces.p, sizeof(float) * 3 * N, hipMemcpyDeviceToHost));
        if (out->forces_std && (want & VSSR_WANT_STD))
            VSSR_HIP(h, hipMemcpy(out->forces_std, h->d_forces_std.p, sizeof(float) * 3 * N, hipMemcpyDeviceToHost));
    }
    // the saturation report travels with the results (vssr_batch_saturated then needs no synchronisation / copy of its own)
    h->h_sat.resize(B);
    VSSR_HIP(h, hipMemcpy(h->h_sat.data(), h->d_sat_out.p, sizeof(unsigned) * B, hipMemcpyDeviceToHost));
    h->h_sat_valid = true;
    return VSSR_OK;
}

int vssr_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *Z, const double *pos,
                    const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out) {
    int rc = vssr_batch_upload(h, n_cfg, n_atoms, Z, pos, cell, pbc);
    if (rc) return rc;
    rc = vssr_batch_run(h, want);
    if (rc) return rc;
    return vssr_batch_download(h, want, out);
}

int vssr_eval(vssr_handle *h, int32_t n_atoms, const int32_t *Z, const double *pos, const double cell[9],
              const uint8_t pbc[3], uint32_t want, vssr_out *out) {
    return vssr_eval_batch(h, 1, &n_atoms, Z, pos, cell, pbc, want, out);
}

static int relax_finish(vssr_handle *h, double *pos_out, int32_t *n_steps, uint8_t *converged);

int vssr_batch_relax_cg(vssr_handle *h, const vssr_cg_params *params, const uint8_t *fixed, uint32_t want, double *pos_out,
                        int32_t *n_iter, int32_t *n_eval, int32_t *stop_reason) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!params || params->max_iter < 0 || params->max_eval < 0 || !(params->etol >= 0) || !(params->ftol >= 0) || !(params->dmax > 0))
        return set_err(h, VSSR_E_BADARG, "bad CG parameters");
    VSSR_HIP(h, hipSetDevice(h->device));
    // one workgroup minimises one chain from start to stop (chain_min.hip: analytic kinds, chains of <= 256 atoms, where the handle's
    // driver setting / VSSR_CG_FUSED / the automatic rule choose it); else the lock-step driver (relax_cg.hip).  Same results bit for bit.
    const bool resident = chain_min_supported(h);
    int rc = resident ? chain_min_cg(h, params, fixed, want) : relax_cg(h, params, fixed, want);
    if (rc) return rc;
    h->cg_last_driver = resident ? VSSR_CG_DRIVER_RESIDENT : VSSR_CG_DRIVER_LOCKSTEP;
    // (the lock-step driver ends with a full batch-wide evaluation of the final positions; the chain-resident one numbers its rows per
    // chain: introspection wants one plain run first)
    return relax_results(h, resident, pos_out, {n_iter, n_eval, stop_reason});
}

int vssr_batch_relax_cg_driver(vssr_handle *h, int32_t driver, int32_t *last_used) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!is_analytic(h)) return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cg_driver: a PaiNN handle has no conjugate-gradient minimiser");
    if (driver > VSSR_CG_DRIVER_RESIDENT)
        return set_err(h, VSSR_E_BADARG, "vssr_batch_relax_cg_driver: driver %d is none of 0 (automatic), 1 (lock-step), 2 (chain-resident)", (int)driver);
    if (driver >= 0) h->cg_driver = driver;
    if (last_used) *last_used = h->cg_last_driver;
    return VSSR_OK;
}

int vssr_batch_relax_bfgs_linesearch(vssr_handle *h, const vssr_bfgsls_params *p, const uint8_t *fixed, uint32_t want, double *pos_out,
                                     int32_t *n_steps, int32_t *n_eval, int32_t *stop_reason) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!p) return set_err(h, VSSR_E_BADARG, "bad BFGSLineSearch parameters: null");
    if (p->max_steps < 0) return set_err(h, VSSR_E_BADARG, "bad BFGSLineSearch parameters: max_steps %d < 0", (int)p->max_steps);
    if (p->max_eval < 1) return set_err(h, VSSR_E_BADARG, "bad BFGSLineSearch parameters: max_eval %d < 1", (int)p->max_eval);
    if (!(p->fmax > 0) || !(p->alpha > 0) || !(p->maxstep > 0))
        return set_err(h, VSSR_E_BADARG, "bad BFGSLineSearch parameters: fmax %g, alpha %g and maxstep %g must be positive", p->fmax, p->alpha, p->maxstep);
    if (!(p->c1 > 0 && p->c1 < 1)) return set_err(h, VSSR_E_BADARG, "bad BFGSLineSearch parameters: c1 %g outside (0, 1)", p->c1);
    if (!(p->c2 > 0 && p->c2 < 1)) return set_err(h, VSSR_E_BADARG, "bad BFGSLineSearch parameters: c2 %g outside (0, 1)", p->c2);
    if (!(p->stpmax >= 1)) return set_err(h, VSSR_E_BADARG, "bad BFGSLineSearch parameters: stpmax %g < 1", p->stpmax);
    VSSR_HIP(h, hipSetDevice(h->device));
    if (int rc = relax_bfgsls(h, p, fixed, want)) return rc;
    return relax_results(h, false, pos_out, {n_steps, n_eval, stop_reason});   // (the driver ends with a batch-wide evaluation of the final positions)
}

int vssr_batch_relax_bfgs(vssr_handle *h, const vssr_bfgs_params *params, const uint8_t *fixed, uint32_t want,
                          double *pos_out, int32_t *n_steps, uint8_t *converged) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!params || params->max_steps < 0 || !(params->fmax > 0) || !(params->alpha > 0) || !(params->maxstep > 0))
        return set_err(h, VSSR_E_BADARG, "bad BFGS parameters");
    VSSR_HIP(h, hipSetDevice(h->device));
    if (int rc = relax_bfgs(h, *params, fixed, want)) return rc;
    return relax_finish(h, pos_out, n_steps, converged);
}

int vssr_batch_relax_fire(vssr_handle *h, const vssr_fire_params *params, const uint8_t *fixed, uint32_t want,
                          double *pos_out, int32_t *n_steps, uint8_t *converged) {
    if (int rc = driver_guard(h, __func__)) return rc;
    if (!params || params->max_steps < 0 || !(params->fmax > 0) || !(params->dt > 0) || !(params->maxstep > 0))
        return set_err(h, VSSR_E_BADARG, "bad FIRE parameters");
    VSSR_HIP(h, hipSetDevice(h->device));
    if (int rc = relax_fire(h, *params, fixed, want)) return rc;
    return relax_finish(h, pos_out, n_steps, converged);
}

static int relax_finish(vssr_handle *h, double *pos_out, int32_t *n_steps, uint8_t *converged) {
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    h->prof.collect();
    if (pos_out) VSSR_HIP(h, hipMemcpy(pos_out, h->d_pos.p, sizeof(double) * 3 * h->n_atoms, hipMemcpyDeviceToHost));
    if (n_steps) VSSR_HIP(h, hipMemcpy(n_steps, h->d_relax_steps.p, sizeof(int) * h->n_cfg, hipMemcpyDeviceToHost));
    if (converged) VSSR_HIP(h, hipMemcpy(converged, h->d_relax_conv.p, (size_t)h->n_cfg, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

// ---- introspection ---------------------------------------------------------------------------------------
int vssr_profile_enable(vssr_handle *h, int enable) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    h->prof.collect();
    h->prof.enabled = enable != 0;
    return VSSR_OK;
}
int vssr_profile_reset(vssr_handle *h) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    h->prof.reset();
    return VSSR_OK;
}
int vssr_profile_read(vssr_handle *h, int32_t cap, const char **names, int64_t *launches, double *total_ms,
                      int32_t *n_out) {
    if (!h || !n_out) return VSSR_E_BADARG;
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    h->prof.collect();
    int n = 0;
    for (int k = 0; k < KC_COUNT && n < cap; ++k) {
        if (names) names[n] = kKernelClassNames[k];
        if (launches) launches[n] = h->prof.launches[k];
        if (total_ms) total_ms[n] = h->prof.total_ms[k];
        ++n;
    }
    *n_out = n;
    return VSSR_OK;
}

int vssr_batch_stats(vssr_handle *h, int64_t *n_atoms, int64_t *n_edges, int64_t *n_slots) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran) return set_err(h, VSSR_E_STATE, "no completed run");
    if (h->graph_partial)
        return set_err(h, VSSR_E_STATE, "the resident graph covers only the chains of the last relaxation iteration: run the batch once (vssr_batch_run) first");
    int rc = sync_and_check(h);
    if (rc) return rc;
    if (n_atoms) *n_atoms = h->n_atoms;
    if (n_edges) *n_edges = h->h_counters[1];
    if (n_slots) *n_slots = h->h_counters[0];
    return VSSR_OK;
}

int vssr_batch_neighbors(vssr_handle *h, int64_t cap, int32_t *ei, int32_t *ej, int32_t *eS, float *er,
                         int64_t *n_edges) {
    if (!h || !n_edges) return VSSR_E_BADARG;
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran) return set_err(h, VSSR_E_STATE, "no completed run");
    if (h->graph_partial)
        return set_err(h, VSSR_E_STATE, "the resident graph covers only the chains of the last relaxation iteration: run the batch once (vssr_batch_run) first");
    int rc = sync_and_check(h);
    if (rc) return rc;
    const int N = h->n_atoms;
    const int64_t slots = h->h_counters[0];
    *n_edges = h->h_counters[1];
    if (!ei && !ej && !eS && !er) return VSSR_OK;
    std::vector<int> row(N + 1), S(slots), wrap((size_t)3 * N);
    std::vector<float4> edge(slots);
    VSSR_HIP(h, hipMemcpy(row.data(), h->d_row_start.p, sizeof(int) * (N + 1), hipMemcpyDeviceToHost));
    VSSR_HIP(h, hipMemcpy(S.data(), h->d_edge_S.p, sizeof(int) * slots, hipMemcpyDeviceToHost));
    VSSR_HIP(h, hipMemcpy(edge.data(), h->d_edge.p, sizeof(float4) * slots, hipMemcpyDeviceToHost));
    VSSR_HIP(h, hipMemcpy(wrap.data(), h->d_wrap.p, sizeof(int) * 3 * N, hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (int i = 0; i < N; ++i)
        for (int e = row[i]; e < row[i + 1]; ++e) {
            int j;
            memcpy(&j, &edge[e].w, sizeof(int));
            if (j < 0) continue;
            if (n < cap) {
                if (ei) ei[n] = i;
                if (ej) ej[n] = j;
                if (eS)  // true image shift: S = S' + wrap_i - wrap_j
                    for (int k = 0; k < 3; ++k)
                        eS[3 * n + k] = (((S[e] >> (8 * k)) & 255) - 128) + wrap[3 * i + k] - wrap[3 * j + k];
                if (er) { er[3 * n] = edge[e].x; er[3 * n + 1] = edge[e].y; er[3 * n + 2] = edge[e].z; }
            }
            ++n;
        }
    return VSSR_OK;
}

int vssr_batch_device_results(vssr_handle *h, const float **energy, const float **energy_std) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran || h->kind != Kind::PAINN) return set_err(h, VSSR_E_STATE, "no completed PaiNN run");
    if (energy) *energy = h->d_energy.as<float>();
    if (energy_std) *energy_std = h->d_energy_std.as<float>();
    return VSSR_OK;
}

int vssr_batch_device_results_f64(vssr_handle *h, const double **energy, const double **energy_std) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran || h->kind != Kind::PAINN) return set_err(h, VSSR_E_STATE, "no completed PaiNN run");
    if (energy) *energy = h->d_energy64.as<double>();
    if (energy_std) *energy_std = h->d_energy64.as<double>() + h->n_cfg;
    return VSSR_OK;
}

int vssr_batch_energy_f64(vssr_handle *h, double *energy, double *energy_std, double *energy_models) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran) return set_err(h, VSSR_E_STATE, "vssr_batch_energy_f64 before a run");
    VSSR_HIP(h, hipSetDevice(h->device));
    int rc = sync_and_check(h);
    if (rc) return rc;
    const size_t B = h->n_cfg, M = h->n_models;
    if (is_analytic(h)) {   // one analytic potential: no spread, the "model" is the potential
        if (energy) VSSR_HIP(h, hipMemcpy(energy, h->d_pot_e.p, sizeof(double) * B, hipMemcpyDeviceToHost));
        if (energy_models) VSSR_HIP(h, hipMemcpy(energy_models, h->d_pot_e.p, sizeof(double) * B, hipMemcpyDeviceToHost));
        if (energy_std) for (size_t b = 0; b < B; ++b) energy_std[b] = 0.0;
        return VSSR_OK;
    }
    const double *src = h->d_energy64.as<double>();
    if (energy) VSSR_HIP(h, hipMemcpy(energy, src, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (energy_std) VSSR_HIP(h, hipMemcpy(energy_std, src + B, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (energy_models) VSSR_HIP(h, hipMemcpy(energy_models, src + 2 * B, sizeof(double) * B * M, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int vssr_batch_results_f64(vssr_handle *h, double *energy, double *energy_atoms, double *forces) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!is_analytic(h)) return set_err(h, VSSR_E_STATE, "vssr_batch_results_f64 needs an fp64 potential (Tersoff / EAM / SW / pair handle)");
    if (!h->ran) return set_err(h, VSSR_E_STATE, "vssr_batch_results_f64 before a run");
    VSSR_HIP(h, hipSetDevice(h->device));
    if (forces && !(h->last_want & VSSR_WANT_FORCES))
        return set_err(h, VSSR_E_STATE, "forces requested, but the last run was asked for energies only");
    int rc = sync_and_check(h);
    if (rc) return rc;
    const size_t B = h->n_cfg, N = h->n_atoms;
    if (energy) VSSR_HIP(h, hipMemcpy(energy, h->d_pot_e.p, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (energy_atoms) VSSR_HIP(h, hipMemcpy(energy_atoms, h->d_pot_ea.p, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (forces) VSSR_HIP(h, hipMemcpy(forces, h->d_pot_f.p, sizeof(double) * 3 * N, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int vssr_device_context(vssr_handle *h, int32_t *device, void **stream, const int32_t **overflow_flag) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (device) *device = h->device;
    if (stream) *stream = (void *)h->stream;
    if (overflow_flag) *overflow_flag = h->d_counters.p ? h->d_counters.as<int>() + 2 : nullptr;
    return VSSR_OK;
}

int vssr_batch_traj_configure(vssr_handle *h, int32_t record_interval) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (record_interval < 0) return set_err(h, VSSR_E_BADARG, "record_interval must be >= 0");
    h->traj_interval = record_interval;
    return VSSR_OK;
}

int vssr_batch_traj_read(vssr_handle *h, int32_t cap_records, int32_t *n_records, double *pos, float *forces, double *energy,
                         int32_t *max_records) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (max_records) *max_records = h->traj_records;
    if (!h->traj_records) {
        if (n_records || pos || forces || energy) return set_err(h, VSSR_E_STATE, "the last relaxation recorded no trajectory");
        return VSSR_OK;
    }
    if (!n_records && !pos && !forces && !energy) return VSSR_OK;
    if (h->traj_B != h->n_cfg || h->traj_N != h->n_atoms) return set_err(h, VSSR_E_STATE, "the recorded trajectory belongs to another batch");
    if (cap_records < h->traj_records) return set_err(h, VSSR_E_BADARG, "trajectory buffers hold %d records, %d are needed", cap_records, h->traj_records);
    VSSR_HIP(h, hipSetDevice(h->device));
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    const size_t R = h->traj_records, N3 = (size_t)3 * h->traj_N, B = h->traj_B;
    if (n_records) VSSR_HIP(h, hipMemcpy(n_records, h->d_traj_n.p, sizeof(int) * B, hipMemcpyDeviceToHost));
    if (pos) VSSR_HIP(h, hipMemcpy(pos, h->d_traj_pos.p, sizeof(double) * N3 * R, hipMemcpyDeviceToHost));
    if (forces) VSSR_HIP(h, hipMemcpy(forces, h->d_traj_f.p, sizeof(float) * N3 * R, hipMemcpyDeviceToHost));
    if (energy) VSSR_HIP(h, hipMemcpy(energy, h->d_traj_e.p, sizeof(double) * B * R, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int vssr_batch_embedding(vssr_handle *h, int32_t model, float *dst, int64_t cap, int64_t *n_out) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran || h->kind != Kind::PAINN) return set_err(h, VSSR_E_STATE, "no completed PaiNN run");
    if (model < -1 || model >= h->n_models) return set_err(h, VSSR_E_BADARG, "model index out of range");
    if (h->graph_partial)   // (chains that converged early keep the features of THEIR last iteration, or of a buffer a regrow replaced)
        return set_err(h, VSSR_E_STATE, "the resident activations cover only the chains of the last relaxation iteration: run the batch once (vssr_batch_run) first");
    VSSR_HIP(h, hipSetDevice(h->device));
    int rc = sync_and_check(h);
    if (rc) return rc;
    const size_t per_model = (size_t)h->n_atoms * h->feat_dim, n = model < 0 ? per_model * h->n_models : per_model;
    if (n_out) *n_out = (int64_t)n;
    if (!dst) return VSSR_OK;
    if ((int64_t)n > cap) return set_err(h, VSSR_E_BADARG, "embedding buffer too small (%lld < %zu floats)", (long long)cap, n);
    // the scalar features leaving the last update block: the state the readout consumes ([M][N][F], model-major)
    const float *src = h->sv.s_in[h->num_conv] + (model < 0 ? 0 : (size_t)model * per_model);
    VSSR_HIP(h, hipMemcpy(dst, src, n * sizeof(float), hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int vssr_batch_stress(vssr_handle *h, double *stress, double *stress_std) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran || !evaluator(h).stress) return set_err(h, VSSR_E_STATE, "no completed PaiNN, Tersoff, EAM or Stillinger-Weber run");
    if (!(h->last_want & VSSR_WANT_FORCES))
        return set_err(h, VSSR_E_STATE, "stress needs the edge gradients of a run that produced forces; the last run was asked for energies only");
    if (h->graph_partial)   // (after the chain-resident CG minimiser too: it numbers its rows per chain and leaves no batch-wide gradients)
        return set_err(h, VSSR_E_STATE, "the resident graph covers only the chains of the last relaxation iteration: run the batch once (vssr_batch_run) first");
    VSSR_HIP(h, hipSetDevice(h->device));
    int rc = sync_and_check(h);   // (a capacity overflow is repaired here: the gradients below are those of the repeated run)
    if (rc) return rc;
    rc = evaluator(h).stress(h);   // fp64 potentials: one model, the spread is written as zeros
    if (rc) return rc;
    VSSR_HIP(h, hipStreamSynchronize(h->stream));
    const size_t n = 6 * (size_t)h->n_cfg;
    if (stress) VSSR_HIP(h, hipMemcpy(stress, h->d_stress.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (stress_std) VSSR_HIP(h, hipMemcpy(stress_std, h->d_stress.as<double>() + n, sizeof(double) * n, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int vssr_batch_saturated(vssr_handle *h, uint8_t *flags, int32_t *n_flagged) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran) return set_err(h, VSSR_E_STATE, "no completed run");
    VSSR_HIP(h, hipSetDevice(h->device));
    int count = 0;
    if (h->kind == Kind::PAINN) {   // the fp64 potentials have no reduced-precision stage
        if (!h->h_sat_valid || (int)h->h_sat.size() != h->n_cfg) {
            int rc = sync_and_check(h);
            if (rc) return rc;
            h->h_sat.resize(h->n_cfg);
            VSSR_HIP(h, hipMemcpy(h->h_sat.data(), h->d_sat_out.p, sizeof(unsigned) * h->n_cfg, hipMemcpyDeviceToHost));
            h->h_sat_valid = true;
        }
        const std::vector<unsigned> &f = h->h_sat;
        for (int b = 0; b < h->n_cfg; ++b) {
            if (flags) flags[b] = f[b] ? 1 : 0;
            count += f[b] ? 1 : 0;
        }
    } else if (flags) {
        memset(flags, 0, (size_t)h->n_cfg);
    }
    if (n_flagged) *n_flagged = count;
    return VSSR_OK;
}

int vssr_debug_capacity(vssr_handle *h, int32_t slots_per_atom, int32_t tight, int32_t *n_regrows) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (slots_per_atom > 0) {
        h->cap_per_atom = slots_per_atom;
        h->cm_cap_per_atom = 0;   // (the chain-resident minimiser's pools start from the new value as well)
        h->slot_cap = 0;   // re-derived at the next neighbor build
    }
    if (tight >= 0) h->cap_tight = tight != 0;
    if (n_regrows) *n_regrows = h->relax_regrows;
    return VSSR_OK;
}

int vssr_batch_relax_counts(vssr_handle *h, int64_t *lockstep_evaluations, int64_t *chain_evaluations) {
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (lockstep_evaluations) *lockstep_evaluations = h->relax_lockstep;
    if (chain_evaluations) *chain_evaluations = h->relax_chain_evals;
    return VSSR_OK;
}

int vssr_debug_read(vssr_handle *h, const char *name, int32_t model, float *dst, int64_t cap, int64_t *n_out) {
    if (!h || !name || !n_out) return VSSR_E_BADARG;
    if (int rc = check_kind(h, KINDS_EVAL, __func__)) return rc;
    if (!h->ran || h->kind != Kind::PAINN) return set_err(h, VSSR_E_STATE, "no completed PaiNN run");
    if (model < 0 || model >= h->n_models) return set_err(h, VSSR_E_BADARG, "model index out of range");
    if (h->painn_general) return set_err(h, VSSR_E_STATE, "per-layer intermediates are not kept by the general-width PaiNN path");
    if (h->graph_partial)
        return set_err(h, VSSR_E_STATE, "the resident graph covers only the chains of the last relaxation iteration: run the batch once (vssr_batch_run) first");
    int rc = sync_and_check(h);
    if (rc) return rc;
    const size_t N = h->n_atoms;
    const StateView &sv = h->sv;
    const float *src = nullptr;
    size_t per_atom = 0;
    std::string nm(name);
    auto layer_of = [&](const char *prefix) -> int {
        size_t pl = strlen(prefix);
        if (nm.compare(0, pl, prefix) != 0 || nm.size() != pl + 1) return -1;
        int l = nm[pl] - '0';
        return (l >= 0 && l < h->num_conv) ? l : -1;
    };
    int l;
    if ((l = layer_of("phi")) >= 0) {
        if (l == 0 && h->l0_used)
            return set_err(h, VSSR_E_STATE, "phi0 is not materialised (layer-0 species factorisation is active)");
        src = sv.phi[l]; per_atom = F3;
    }
    else if ((l = layer_of("s_msg")) >= 0) { src = sv.s_msg[l]; per_atom = F; }
    else if ((l = layer_of("v_msg")) >= 0) { src = sv.v_msg[l]; per_atom = F3; }
    else if ((l = layer_of("s_upd")) >= 0) { src = sv.s_in[l + 1]; per_atom = F; }
    else if ((l = layer_of("v_upd")) >= 0) {
        if (l == h->num_conv - 1 && !h->debug_keep)
            return set_err(h, VSSR_E_STATE, "v_upd of the last block is not materialised (nothing consumes it; create the handle with VSSR_DEBUG_KEEP=1)");
        src = sv.v_in[l + 1]; per_atom = F3;
    }
    else if (nm == "e_atom") { src = sv.e_atom; per_atom = 1; }
    else if (nm == "sbar_msg0") { src = sv.sbar_msg_l0; per_atom = F; }   // reverse buffers hold the LAST layer processed
    else if (nm == "vbar_msg0") { src = sv.vbar_msg; per_atom = F3; }
    else return set_err(h, VSSR_E_BADARG, "unknown intermediate '%s'", name);
    size_t n = N * per_atom;
    *n_out = (int64_t)n;
    if (!dst) return VSSR_OK;
    if ((int64_t)n > cap) return set_err(h, VSSR_E_BADARG, "buffer too small for '%s'", name);
    VSSR_HIP(h, hipMemcpy(dst, src + (size_t)model * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return VSSR_OK;
}

}  // extern "C"
