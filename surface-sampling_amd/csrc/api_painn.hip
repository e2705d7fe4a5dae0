// api_painn.hip — vssr_create: the PaiNN ensemble handle and its weight upload (128 / 20 path; painn_gen.hip uploads the general one).
#include <cmath>

#include "vssr_internal.h"

namespace vssr {

// ---- weights ------------------------------------------------------------------------------------------
static void transpose(const float *src, int rows, int cols, float *dst) {  // dst[c][r] = src[r][c]
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) dst[(size_t)c * rows + r] = src[(size_t)r * cols + c];
}

static int upload_weights(vssr_handle *h, const vssr_painn_config *cfg) {
    const int M = cfg->n_models, L = cfg->num_conv, R = cfg->n_rbf, H = cfg->readout_hidden, NE = cfg->n_embed;
    const size_t per_layer = (size_t)F * F + F + (size_t)F3 * F + F3 + (size_t)F3 * R + F3 + 2 * (size_t)F * F +
                             (size_t)F * 2 * F + F + (size_t)F3 * F + F3;
    const size_t blob_len = (size_t)NE * F + L * per_layer + (size_t)H * F + H + H + 1;
    if (cfg->weights_len != blob_len)
        return set_err(h, VSSR_E_BADARG, "weights_len %llu does not match the layout (%zu floats)",
                       (unsigned long long)cfg->weights_len, blob_len);
    // device image per model: [blob][transposed copies]
    const size_t t_per_layer = (size_t)F * F + (size_t)F * F3 + 2 * (size_t)F * F + (size_t)2 * F * F + (size_t)F * F3;
    const size_t img_len = blob_len + L * t_per_layer + (size_t)F * H;
    std::vector<float> img(img_len * M);
    std::vector<ModelW> table(M);
    if (h->weights.ensure(img.size() * sizeof(float)))
        return set_err(h, VSSR_E_NOMEM, "weights: out of device memory");
    float *dbase = h->weights.as<float>();
    // fp16-split fragment-order copies of the node-GEMM weights: 22 F^2 elements x 4 B per (model, layer)
    const size_t node16_per_layer = (size_t)22 * F * F;   // dwords
    const size_t node16_readout = (size_t)2 * H * F;      // W5 and W5^T (used when the width is a multiple of 32)
    std::vector<unsigned> node16(node16_per_layer * L * M + node16_readout * M);
    for (int m = 0; m < M; ++m) {
        float *hb = img.data() + (size_t)m * img_len;
        float *db = dbase + (size_t)m * img_len;
        memcpy(hb, cfg->weights[m], blob_len * sizeof(float));
        for (size_t t = 0; t < blob_len; ++t)
            if (!std::isfinite(hb[t])) return set_err(h, VSSR_E_BADARG, "model %d: non-finite weight", m);
        ModelW &W = table[m];
        size_t o = 0, to = blob_len;
        auto take = [&](size_t n) { size_t r = o; o += n; return r; };
        auto taket = [&](size_t n) { size_t r = to; to += n; return r; };
        W.embed = db + take((size_t)NE * F);
        for (int l = 0; l < L; ++l) {
            LayerW &Lw = W.layer[l];
            size_t w1 = take((size_t)F * F), b1 = take(F), w2 = take((size_t)F3 * F), b2 = take(F3);
            size_t wd = take((size_t)F3 * R), bd = take(F3), u = take((size_t)F * F), v = take((size_t)F * F);
            size_t w3 = take((size_t)F * 2 * F), b3 = take(F), w4 = take((size_t)F3 * F), b4 = take(F3);
            size_t w1t = taket((size_t)F * F), w2t = taket((size_t)F * F3), ut = taket((size_t)F * F);
            size_t vt = taket((size_t)F * F), w3t = taket((size_t)2 * F * F), w4t = taket((size_t)F * F3);
            transpose(hb + w1, F, F, hb + w1t);
            transpose(hb + w2, F3, F, hb + w2t);
            transpose(hb + u, F, F, hb + ut);
            transpose(hb + v, F, F, hb + vt);
            transpose(hb + w3, F, 2 * F, hb + w3t);
            transpose(hb + w4, F3, F, hb + w4t);
            Lw.W1 = db + w1; Lw.W1t = db + w1t; Lw.b1 = db + b1;
            Lw.W2 = db + w2; Lw.W2t = db + w2t; Lw.b2 = db + b2;
            Lw.Wd = db + wd; Lw.bd = db + bd;
            Lw.U = db + u; Lw.Ut = db + ut; Lw.V = db + v; Lw.Vt = db + vt;
            Lw.W3 = db + w3; Lw.W3t = db + w3t; Lw.b3 = db + b3;
            Lw.W4 = db + w4; Lw.W4t = db + w4t; Lw.b4 = db + b4;
            // fp16-split MFMA fragment-order copies of the eleven node-GEMM matrices (painn_node_mfma.hip)
            {   // [U;V]^T: rows g (input feature of U/V), K = 2F: k<F -> U[k][g], k>=F -> V[k-F][g]
                std::vector<float> uvt((size_t)F * 2 * F);
                for (int g = 0; g < F; ++g)
                    for (int k = 0; k < F; ++k) {
                        uvt[(size_t)g * 2 * F + k] = hb[u + (size_t)k * F + g];
                        uvt[(size_t)g * 2 * F + F + k] = hb[v + (size_t)k * F + g];
                    }
                // fp16-split copies, same order as the q* pointers are assigned below
                unsigned *q = node16.data() + ((size_t)m * L + l) * node16_per_layer;
                auto put16 = [&](const float *src, int rows, int K) {
                    pack_mfma_tiles16(src, rows, K, q);
                    q += (size_t)rows * K;
                };
                put16(hb + w1, F, F); put16(hb + w2, F3, F); put16(hb + u, F, F); put16(hb + v, F, F);
                put16(hb + w3, F, 2 * F); put16(hb + w4, F3, F); put16(hb + w1t, F, F); put16(hb + w2t, F, F3);
                put16(hb + w4t, F, F3); put16(hb + w3t, 2 * F, F); put16(uvt.data(), F, 2 * F);
            }
        }
        size_t w5 = take((size_t)H * F), b5 = take(H), w6 = take(H), b6 = take(1);
        size_t w5t = taket((size_t)F * H);
        transpose(hb + w5, H, F, hb + w5t);
        W.W5 = db + w5; W.W5t = db + w5t; W.b5 = db + b5; W.w6 = db + w6; W.b6 = db + b6;
        if (H % 32 == 0) {   // fragment-order pieces of the readout matrices (matrix-pipe readout, painn_node_mfma.hip)
            unsigned *q = node16.data() + node16_per_layer * L * M + node16_readout * m;
            pack_mfma_tiles16(hb + w5, H, F, q);
            pack_mfma_tiles16(hb + w5t, F, H, q + (size_t)H * F);
        }
    }
    VSSR_HIP(h, hipMemcpy(dbase, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    {   // node-GEMM weights as fp16 pieces (painn_node_mfma.hip)
        if (h->node16.ensure(node16.size() * sizeof(unsigned))) return set_err(h, VSSR_E_NOMEM, "split node weights");
        VSSR_HIP(h, hipMemcpy(h->node16.p, node16.data(), node16.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        for (int m = 0; m < M; ++m)
            for (int l = 0; l < L; ++l) {
                LayerW &Lw = table[m].layer[l];
                const uint4 *q = h->node16.as<uint4>() + ((size_t)m * L + l) * node16_per_layer / 4;
                auto next = [&](int rows, int K) { const uint4 *r = q; q += (size_t)rows * K / 4; return r; };
                Lw.qW1 = next(F, F); Lw.qW2 = next(F3, F); Lw.qU = next(F, F); Lw.qV = next(F, F);
                Lw.qW3 = next(F, 2 * F); Lw.qW4 = next(F3, F); Lw.qW1t = next(F, F); Lw.qW2t = next(F, F3);
                Lw.qW4t = next(F, F3); Lw.qW3t = next(2 * F, F); Lw.qUVt = next(F, 2 * F);
            }
        for (int m = 0; m < M; ++m) {
            const uint4 *q = h->node16.as<uint4>() + (node16_per_layer * L * M + node16_readout * m) / 4;
            table[m].qW5 = q;
            table[m].qW5t = q + (size_t)H * F / 4;
        }
    }
    {   // radial-filter weights split into fp16 pieces in MFMA operand order (painn_edge_mfma.hip), per model / layer
        const size_t per_layer16 = (size_t)F3 * 4 * 8;   // dwords
        std::vector<unsigned> w16(per_layer16 * L * M);
        for (int m = 0; m < M; ++m) {
            const float *hb = img.data() + (size_t)m * img_len;
            size_t o = (size_t)NE * F;
            for (int l = 0; l < L; ++l) {
                const float *Wd = hb + o + (size_t)F * F + F + (size_t)F3 * F + F3;
                build_wd16(Wd, Wd + (size_t)F3 * 20, w16.data() + ((size_t)m * L + l) * per_layer16);
                o += per_layer;
            }
        }
        if (h->wd16.ensure(w16.size() * sizeof(unsigned))) return set_err(h, VSSR_E_NOMEM, "split filter weights");
        VSSR_HIP(h, hipMemcpy(h->wd16.p, w16.data(), w16.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        for (int m = 0; m < M; ++m)
            for (int l = 0; l < L; ++l)
                table[m].layer[l].wd16 = h->wd16.as<uint4>() + ((size_t)m * L + l) * per_layer16 / 4;
    }
    {   // layer-0 species factorisation tables (painn_l0.hip), from layer 0 of every model
        const size_t per_model = (size_t)NE * 2 * 24 * F;
        std::vector<float> A(per_model * M), At(per_model * M);
        for (int m = 0; m < M; ++m) {
            const float *hb = img.data() + (size_t)m * img_len;
            size_t o = (size_t)NE * F;
            const float *W1 = hb + o; o += (size_t)F * F;
            const float *b1 = hb + o; o += F;
            const float *W2 = hb + o; o += (size_t)F3 * F;
            const float *b2 = hb + o; o += F3;
            const float *Wd = hb + o; o += (size_t)F3 * R;
            const float *bd = hb + o;
            l0_build_tables(hb, W1, b1, W2, b2, Wd, bd, NE, A.data() + per_model * m, At.data() + per_model * m);
        }
        // the kernels read the fp16-split fragment-order copies (painn_l0.hip); the fp32 tables stay on the host
        const size_t pk = l0_packed_dwords(NE);
        std::vector<unsigned> A16(pk * M), At16(pk * M);
        for (int m = 0; m < M; ++m) l0_pack_tables(A.data() + per_model * m, NE, A16.data() + pk * m, At16.data() + pk * m);
        if (h->d_l0A.ensure(A16.size() * sizeof(unsigned)) || h->d_l0At.ensure(At16.size() * sizeof(unsigned)))
            return set_err(h, VSSR_E_NOMEM, "layer-0 tables");
        VSSR_HIP(h, hipMemcpy(h->d_l0A.p, A16.data(), A16.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        VSSR_HIP(h, hipMemcpy(h->d_l0At.p, At16.data(), At16.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    }
    if (h->model_table.ensure(sizeof(ModelW) * M)) return set_err(h, VSSR_E_NOMEM, "model table");
    VSSR_HIP(h, hipMemcpy(h->model_table.p, table.data(), sizeof(ModelW) * M, hipMemcpyHostToDevice));
    return VSSR_OK;
}

// The environment knobs of a PaiNN handle, read once at create (debugging and tests; DESIGN.md lists them).
static void read_env_knobs(vssr_handle *h) {
    // general: the general-width fp32 path although the shape is 128 / 20 (tests: A/B of the two paths)
    if (const char *e = getenv("VSSR_PAINN_PATH")) h->painn_general = h->painn_general || strcmp(e, "general") == 0;
    // gather: every chain takes the scalar gather kernels
    if (const char *e = getenv("VSSR_EDGE_IMPL")) h->edge_impl = (strcmp(e, "gather") == 0) ? 0 : 1;
    // 0: layer 0 on the gather kernels instead of the species factorisation (the general path never factorises)
    if (const char *e = getenv("VSSR_L0_FACTORISE")) h->l0_enabled = atoi(e);
    if (h->painn_general) h->l0_enabled = 0;
    // 1: update_fwd stores its intermediates, the reverse kernel loads them instead of recomputing
    if (const char *e = getenv("VSSR_UPD_SAVE")) h->upd_save = atoi(e);
    // 1: also materialise what only vssr_debug_read looks at
    if (const char *e = getenv("VSSR_DEBUG_KEEP")) h->debug_keep = atoi(e);
    // chains above this atom count leave the 16-feature classes although they fit (tests)
    if (const char *e = getenv("VSSR_EDGE_FS16_MAX")) h->fs16_max_atoms = atoi(e);
    // chains above this atom count leave the 8-feature class for the 4-feature one although they fit (tests)
    if (const char *e = getenv("VSSR_EDGE_FS8_MAX")) h->fs8_max_atoms = atoi(e);
    // 0: large chains take the 8- / 4-feature reverse kernels; 1: the 16-feature kernel in several passes; 2: every chain multi-pass
    if (const char *e = getenv("VSSR_EDGE_BWD_MPASS")) h->bwd_multi_pass = atoi(e);
    // atoms per neighbor sub-range of the multi-pass forms instead of what LDS holds (>= 8; tests)
    if (const char *e = getenv("VSSR_EDGE_SUB_CHUNK")) { const int c = atoi(e); if (c >= 8) { h->sub_chunk_fwd = c; h->sub_chunk_bwd = c; } }
    // 0 | 8 | 16: the 4-feature forward class runs the 4-feature kernel, or the 8- / 16-feature kernel in several passes
    if (const char *e = getenv("VSSR_EDGE_FWD_2PASS")) { const int w = atoi(e); h->fwd_two_pass = (w == 8 || w == 16) ? w : w ? 16 : 0; }
    // workgroups of the persistent 16-wave forward neighbor sum instead of one per CU; 0: one item per workgroup (tests: the second grid)
    if (const char *e = getenv("VSSR_EDGE_FWD_GRID")) h->edge_fwd_grid = max(atoi(e), 0);
}

}  // namespace vssr

using namespace vssr;

extern "C" {

int vssr_create(const vssr_painn_config *cfg, vssr_handle **out) {
    if (!cfg || !out) return set_err(nullptr, VSSR_E_BADARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(vssr_painn_config))
        return set_err(nullptr, VSSR_E_BADARG, "vssr_painn_config size mismatch (%u vs %zu)", cfg->struct_size,
                       sizeof(vssr_painn_config));
    // accepted shapes: (128, 20) takes the specialised path, every other one the general-width path (painn_gen.hip)
    if (cfg->feat_dim < 16 || cfg->feat_dim > 256 || cfg->feat_dim % 16 != 0 || cfg->n_rbf < 1 || cfg->n_rbf > 32)
        return set_err(nullptr, VSSR_E_BADARG,
                       "feat_dim must be a multiple of 16 in 16..256 and n_rbf in 1..32 (got %d, %d)", cfg->feat_dim, cfg->n_rbf);
    if (cfg->n_models < 1 || cfg->n_models > MAX_MODELS || cfg->num_conv < 1 || cfg->num_conv > MAX_LAYERS ||
        cfg->readout_hidden < 1 || cfg->readout_hidden > F || cfg->n_embed < 1 || !cfg->weights ||
        !(cfg->cutoff > 0) || !(cfg->model_units_per_ev > 0))
        return set_err(nullptr, VSSR_E_BADARG, "bad PaiNN configuration");
    if (cfg->excl_vol && (cfg->excl_power < 1 || cfg->excl_power > 64 || !(cfg->excl_sigma > 0)))
        return set_err(nullptr, VSSR_E_BADARG, "excluded volume: power %d (1 .. 64) / sigma %g out of range", cfg->excl_power,
                       (double)cfg->excl_sigma);
    return create_handle(Kind::PAINN, cfg->device, out, [cfg](vssr_handle *h) {
        h->n_models = cfg->n_models; h->n_rbf = cfg->n_rbf; h->num_conv = cfg->num_conv; h->n_embed = cfg->n_embed;
        h->readout_hidden = cfg->readout_hidden; h->cutoff = cfg->cutoff; h->excl_vol = cfg->excl_vol;
        h->excl_power = cfg->excl_power; h->excl_sigma = cfg->excl_sigma; h->units_per_ev = cfg->model_units_per_ev;
        h->feat_dim = cfg->feat_dim;
        h->painn_general = !(cfg->feat_dim == F && cfg->n_rbf == 20);
        read_env_knobs(h);
        int rc = VSSR_OK;
        if (h->painn_general)   // none of the fp16-split / sliced / species-factorised machinery of the 128 / 20 path
            rc = painn_gen_upload(h, cfg);
        else {
            rc = upload_weights(h, cfg);
            if (!rc) rc = node_mfma_init(h);
            if (!rc) rc = edge_mfma_init(h);
            if (!rc) rc = l0_mfma_init(h);
        }
        if (!rc && cfg->offset_per_z) {
            h->has_offset = true;
            h->offset_const = cfg->offset_const;
            if (h->offset_per_z.ensure(sizeof(double) * cfg->n_embed)) rc = set_err(h, VSSR_E_NOMEM, "offset table");
            else if (hipMemcpy(h->offset_per_z.p, cfg->offset_per_z, sizeof(double) * cfg->n_embed,
                               hipMemcpyHostToDevice) != hipSuccess)
                rc = set_err(h, VSSR_E_DEVICE, "offset table upload failed");
        }
        return rc;
    });
}

}  // extern "C"
