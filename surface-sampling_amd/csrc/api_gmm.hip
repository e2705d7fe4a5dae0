// api_gmm.hip — Gaussian-mixture scoring, Gaussian-mixture fit and latent-space clustering entry points.
#include <cmath>

#include "vssr_internal.h"

using namespace vssr;

extern "C" {

// ---- Gaussian-mixture uncertainty (gmm.hip) -------------------------------------------------------------------------------------
int vssr_gmm_create(const vssr_gmm_config *cfg, vssr_handle **out) {
    if (!cfg || !out) return set_err(nullptr, VSSR_E_BADARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(vssr_gmm_config))
        return set_err(nullptr, VSSR_E_BADARG, "vssr_gmm_config size mismatch (%u vs %zu)", cfg->struct_size, sizeof(vssr_gmm_config));
    const int K = cfg->n_components, D = cfg->dim;
    if (K < 1 || K > 256 || D < 1 || D > 256)
        return set_err(nullptr, VSSR_E_BADARG, "GMM: n_components must be in 1..256 and dim in 1..256 (got %d, %d)", K, D);
    if (!cfg->means || !cfg->prec_chol || !cfg->weights) return set_err(nullptr, VSSR_E_BADARG, "GMM: null parameter array");
    if (!std::isfinite(cfg->log_2pi)) return set_err(nullptr, VSSR_E_BADARG, "GMM: log_2pi is not finite");
    for (size_t i = 0; i < (size_t)K * D; ++i)
        if (!std::isfinite(cfg->means[i])) return set_err(nullptr, VSSR_E_BADARG, "GMM: non-finite mean (component %zu)", i / D);
    for (size_t i = 0; i < (size_t)K * D * D; ++i)
        if (!std::isfinite(cfg->prec_chol[i]))
            return set_err(nullptr, VSSR_E_BADARG, "GMM: non-finite precision Cholesky entry (component %zu)", i / ((size_t)D * D));
    for (int k = 0; k < K; ++k)
        for (int d = 0; d < D; ++d)
            if (!(cfg->prec_chol[((size_t)k * D + d) * D + d] > 0))
                return set_err(nullptr, VSSR_E_BADARG, "GMM: diagonal entry %d of the precision Cholesky factor of component %d is not positive", d, k);
    bool any = false;
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(cfg->weights[k]) || cfg->weights[k] < 0)
            return set_err(nullptr, VSSR_E_BADARG, "GMM: weight %d is negative or not finite", k);
        any = any || cfg->weights[k] > 0;
    }
    if (!any) return set_err(nullptr, VSSR_E_BADARG, "GMM: no positive weight");
    return create_handle(Kind::GMM, cfg->device, out, [=](vssr_handle *h) {
        h->gmm_K = K;
        h->gmm_D = D;
        h->gmm_Dp = 16 * ((D + 15) / 16);
        h->gmm_log2pi = cfg->log_2pi;
        return gmm_upload(h, cfg->means, cfg->prec_chol, cfg->weights);
    }, /*range_check=*/false);
}

int vssr_gmm_score_rows(vssr_handle *g, int64_t n_rows, const double *x, double *nll, double *log_prob) {
    if (int rc = check_kind(g, kind_bit(Kind::GMM), __func__)) return rc;
    if (n_rows < 0 || n_rows > (int64_t)INT32_MAX - 64) return set_err(g, VSSR_E_BADARG, "n_rows %lld out of range", (long long)n_rows);
    if (n_rows > 0 && !x) return set_err(g, VSSR_E_BADARG, "null rows");
    if (n_rows == 0) return VSSR_OK;
    VSSR_HIP(g, hipSetDevice(g->device));
    const int D = g->gmm_D, Dp = g->gmm_Dp, K = g->gmm_K;
    const size_t n = (size_t)n_rows;
    if (g->d_gmm_x.ensure(sizeof(double) * n * Dp)) return set_err(g, VSSR_E_NOMEM, "device allocation failed (GMM rows)");
    if (Dp == D) {
        VSSR_HIP(g, hipMemcpy(g->d_gmm_x.p, x, sizeof(double) * n * D, hipMemcpyHostToDevice));
    } else {   // zero-padded columns D .. Dp-1 (one strided copy)
        VSSR_HIP(g, hipMemset(g->d_gmm_x.p, 0, sizeof(double) * n * Dp));
        VSSR_HIP(g, hipMemcpy2D(g->d_gmm_x.p, sizeof(double) * Dp, x, sizeof(double) * D, sizeof(double) * D, n, hipMemcpyHostToDevice));
    }
    int rc = gmm_score_f64(g, g->stream, n_rows, g->d_gmm_x.as<double>());
    if (rc) return rc;
    VSSR_HIP(g, hipStreamSynchronize(g->stream));
    if (nll) VSSR_HIP(g, hipMemcpy(nll, g->d_gmm_nll.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (log_prob) VSSR_HIP(g, hipMemcpy(log_prob, g->d_gmm_lp.p, sizeof(double) * n * K, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

int vssr_gmm_score_batch(vssr_handle *g, vssr_handle *painn, int32_t model, int32_t rows, int32_t order, double *nll_rows,
                         double *system) {
    if (!g || !painn) return g ? set_err(g, VSSR_E_BADARG, "null PaiNN handle") : VSSR_E_BADARG;
    if (int rc = check_kind(g, kind_bit(Kind::GMM), __func__)) return rc;
    if (painn->kind != Kind::PAINN) return set_err(g, VSSR_E_BADARG, "the second handle is not a PaiNN ensemble");
    if (rows != 0 && rows != 1) return set_err(g, VSSR_E_BADARG, "rows must be 0 (atoms) or 1 (structure means), got %d", rows);
    if (order < 0 || order > 6) return set_err(g, VSSR_E_BADARG, "order must be in 0..6, got %d", order);
    if (model < 0 || model >= painn->n_models)
        return set_err(g, VSSR_E_BADARG, "model index %d out of range (%d models)", model, painn->n_models);
    if (g->device != painn->device)
        return set_err(g, VSSR_E_BADARG, "the GMM handle is on device %d, the PaiNN handle on device %d", g->device, painn->device);
    if (g->gmm_D != painn->feat_dim)
        return set_err(g, VSSR_E_BADARG, "GMM dimension %d differs from the PaiNN feat_dim %d", g->gmm_D, painn->feat_dim);
    if (!painn->ran) return set_err(g, VSSR_E_STATE, "no completed PaiNN run");
    if (painn->graph_partial)
        return set_err(g, VSSR_E_STATE, "the resident activations cover only the chains of the last relaxation iteration: run the batch once (vssr_batch_run) first");
    VSSR_HIP(g, hipSetDevice(g->device));
    int rc = sync_and_check(painn);   // (a capacity overflow is repaired here: the features below are those of the repeated run)
    if (rc) return set_err(g, rc, "PaiNN run failed: %s", painn->err.c_str());
    const int B = painn->n_cfg, N = painn->n_atoms;
    const hipStream_t st = painn->stream;
    if (g->d_gmm_start.ensure(sizeof(int) * (B + 1))) return set_err(g, VSSR_E_NOMEM, "device allocation failed (GMM offsets)");
    VSSR_HIP(g, hipMemcpyAsync(g->d_gmm_start.p, painn->h_cfg_start.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice, st));
    const float *emb = painn->sv.s_in[painn->num_conv] + (size_t)model * N * painn->feat_dim;
    const int *start = g->d_gmm_start.as<int>();
    if (rows == 0) {
        rc = gmm_score_f32(g, st, N, emb);
        if (!rc && order > 0) rc = gmm_reduce(g, st, B, start, order);
    } else {
        rc = gmm_mean_rows(g, st, B, start, emb);
        if (!rc) rc = gmm_score_f64(g, st, B, g->d_gmm_x.as<double>());
    }
    if (rc) return rc;
    VSSR_HIP(g, hipStreamSynchronize(st));
    const size_t n_out = rows == 0 ? (size_t)N : (size_t)B;
    if (nll_rows) VSSR_HIP(g, hipMemcpy(nll_rows, g->d_gmm_nll.p, sizeof(double) * n_out, hipMemcpyDeviceToHost));
    if (system && order > 0) {
        const void *src = rows == 0 ? g->d_gmm_sys.p : g->d_gmm_nll.p;   // one mean row per structure: its own NLL
        VSSR_HIP(g, hipMemcpy(system, src, sizeof(double) * B, hipMemcpyDeviceToHost));
    }
    return VSSR_OK;
}

// ---- Gaussian-mixture fit (gmm_fit.hip) ---------------------------------------------------------------------------------------------
// first use of the device by a fit handle
static int fit_device(vssr_handle *h) {
    if (h->fit->device_ready) {
        VSSR_HIP(h, hipSetDevice(h->device));
        return VSSR_OK;
    }
    int rc = device_in_range(h, h->device);
    if (!rc) rc = open_device(h, h->device);
    if (rc) return rc;
    h->fit->device_ready = true;
    return VSSR_OK;
}

int vssr_gmm_fit_create(const vssr_gmm_fit_config *cfg, vssr_handle **out) {
    if (!cfg || !out) return set_err(nullptr, VSSR_E_BADARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(vssr_gmm_fit_config))
        return set_err(nullptr, VSSR_E_BADARG, "vssr_gmm_fit_config size mismatch (%u vs %zu)", cfg->struct_size, sizeof(vssr_gmm_fit_config));
    int rc = gmm_fit_check_config(cfg);
    if (rc) return rc;
    if (cfg->device < 0) return set_err(nullptr, VSSR_E_BADARG, "device %d out of range", cfg->device);
    vssr_handle *h = new vssr_handle();   // host state only: the device is opened by the first call that needs it (fit_device)
    h->kind = Kind::GMM_FIT;
    h->device = cfg->device;
    h->gmm_K = cfg->n_components;
    h->gmm_D = cfg->dim;
    h->gmm_Dp = 16 * ((cfg->dim + 15) / 16);
    h->gmm_log2pi = 1.8378770664093453;   // log(2 pi) in fp64, as gmm.py; the float32 constant is a scoring quirk of GMMUncertainty
    h->fit.reset(new GmmFit());
    GmmFit *f = h->fit.get();
    f->cov_type = cfg->covariance_type; f->init = cfg->init; f->max_iter = cfg->max_iter; f->n_init = cfg->n_init;
    f->tol = cfg->tol; f->reg_covar = cfg->reg_covar; f->seed = cfg->seed;
    *out = h;
    return VSSR_OK;
}

int vssr_gmm_fit_append_rows(vssr_handle *h, int64_t n_rows, const double *x) {
    if (int rc = check_kind(h, kind_bit(Kind::GMM_FIT), __func__)) return rc;
    if (n_rows < 1 || !x) return set_err(h, VSSR_E_BADARG, "GMM fit: null or empty rows");
    if (n_rows > (int64_t)INT32_MAX - 64) return set_err(h, VSSR_E_BADARG, "GMM fit: n_rows %lld out of range", (long long)n_rows);
    const size_t tot = (size_t)n_rows * h->gmm_D;
    for (size_t i = 0; i < tot; ++i)
        if (!std::isfinite(x[i])) return set_err(h, VSSR_E_BADARG, "GMM fit: row %zu holds a non-finite value", i / h->gmm_D);
    int rc = fit_device(h);
    if (rc) return rc;
    return gmm_fit_append_host(h, n_rows, x);
}

// rows of a PaiNN handle's resident embedding into the resident set of a fit or clustering handle
static int fit_append_batch(vssr_handle *h, vssr_handle *painn, int32_t model, int32_t rows) {
    if (!painn) return set_err(h, VSSR_E_BADARG, "null PaiNN handle");
    if (painn->kind != Kind::PAINN) return set_err(h, VSSR_E_BADARG, "the second handle is not a PaiNN ensemble");
    if (rows != 0 && rows != 1) return set_err(h, VSSR_E_BADARG, "rows must be 0 (atoms) or 1 (structure means), got %d", rows);
    if (model < 0 || model >= painn->n_models)
        return set_err(h, VSSR_E_BADARG, "model index %d out of range (%d models)", model, painn->n_models);
    if (h->device != painn->device)
        return set_err(h, VSSR_E_BADARG, "the GMM fit handle is on device %d, the PaiNN handle on device %d", h->device, painn->device);
    if (h->gmm_D != painn->feat_dim)
        return set_err(h, VSSR_E_BADARG, "GMM dimension %d differs from the PaiNN feat_dim %d", h->gmm_D, painn->feat_dim);
    if (!painn->ran) return set_err(h, VSSR_E_STATE, "no completed PaiNN run");
    if (painn->graph_partial)
        return set_err(h, VSSR_E_STATE, "the resident activations cover only the chains of the last relaxation iteration: run the batch once (vssr_batch_run) first");
    int rc = fit_device(h);
    if (rc) return rc;
    rc = sync_and_check(painn);
    if (rc) return set_err(h, rc, "PaiNN run failed: %s", painn->err.c_str());
    const int B = painn->n_cfg, N = painn->n_atoms;
    const hipStream_t st = painn->stream;
    const float *emb = painn->sv.s_in[painn->num_conv] + (size_t)model * N * painn->feat_dim;
    if (rows == 0) return gmm_fit_append_f32(h, st, N, emb);
    if (h->d_gmm_start.ensure(sizeof(int) * (B + 1))) return set_err(h, VSSR_E_NOMEM, "device allocation failed (GMM offsets)");
    VSSR_HIP(h, hipMemcpyAsync(h->d_gmm_start.p, painn->h_cfg_start.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice, st));
    rc = gmm_mean_rows(h, st, B, h->d_gmm_start.as<int>(), emb);
    if (rc) return rc;
    return gmm_fit_append_f64p(h, st, B, h->d_gmm_x.as<double>());
}

int vssr_gmm_fit_append_batch(vssr_handle *h, vssr_handle *painn, int32_t model, int32_t rows) {
    if (int rc = check_kind(h, kind_bit(Kind::GMM_FIT), __func__)) return rc;
    return fit_append_batch(h, painn, model, rows);
}

int vssr_gmm_fit_clear(vssr_handle *h) {
    if (int rc = check_kind(h, kind_bit(Kind::GMM_FIT), __func__)) return rc;
    h->fit->n = 0;
    h->fit->fitted = false;
    h->fit->i_labels.clear();
    h->fit->has_labels = false;
    return VSSR_OK;
}

int vssr_gmm_fit_set_init(vssr_handle *h, const double *means, const double *weights, const double *precisions,
                          const int32_t *labels) {
    if (int rc = check_kind(h, kind_bit(Kind::GMM_FIT), __func__)) return rc;
    return gmm_fit_set_init(h, means, weights, precisions, labels);
}

int vssr_gmm_fit_run(vssr_handle *h, vssr_gmm_fit_result *res) {
    if (int rc = check_kind(h, kind_bit(Kind::GMM_FIT), __func__)) return rc;
    GmmFit *f = h->fit.get();
    if (f->n < 2) return set_err(h, VSSR_E_BADARG, "GMM fit: at least 2 rows are needed (%lld resident)", (long long)f->n);
    if (h->gmm_K > f->n) return set_err(h, VSSR_E_BADARG, "GMM fit: n_components %d exceeds the %lld resident rows", h->gmm_K, (long long)f->n);
    const bool all_given = f->has_means && f->has_weights && f->has_prec;
    if (f->init == VSSR_GMM_INIT_GIVEN && !all_given && !f->has_labels)
        return set_err(h, VSSR_E_BADARG, "GMM fit: init = given needs labels, or means, weights and precisions (vssr_gmm_fit_set_init)");
    if (f->has_labels && (int64_t)f->i_labels.size() != f->n)
        return set_err(h, VSSR_E_BADARG, "GMM fit: %zu labels for %lld resident rows", f->i_labels.size(), (long long)f->n);
    int rc = fit_device(h);
    if (rc) return rc;
    return gmm_fit_run(h, res);
}

int vssr_gmm_fit_params(vssr_handle *h, double *weights, double *means, double *covariances, double *prec_chol) {
    if (int rc = check_kind(h, kind_bit(Kind::GMM_FIT), __func__)) return rc;
    if (!h->fit->fitted) return set_err(h, VSSR_E_STATE, "GMM fit: no completed fit");
    VSSR_HIP(h, hipSetDevice(h->device));
    return gmm_fit_params(h, weights, means, covariances, prec_chol);
}

int vssr_gmm_fit_scorer(vssr_handle *h, double log_2pi, vssr_handle **gmm) {
    if (int rc = check_kind(h, kind_bit(Kind::GMM_FIT), __func__)) return rc;
    if (!gmm) return set_err(h, VSSR_E_BADARG, "null argument");
    *gmm = nullptr;
    if (!std::isfinite(log_2pi)) return set_err(h, VSSR_E_BADARG, "GMM: log_2pi is not finite");
    if (!h->fit->fitted) return set_err(h, VSSR_E_STATE, "GMM fit: no completed fit");
    vssr_handle *g = new vssr_handle();   // (not create_handle: a failure is the fit handle's error, not a create error)
    g->kind = Kind::GMM;
    g->gmm_K = h->gmm_K; g->gmm_D = h->gmm_D; g->gmm_Dp = h->gmm_Dp;
    g->gmm_log2pi = log_2pi;
    int rc = open_device(g, h->device);
    if (!rc) rc = gmm_fit_copy_scorer(h, g);
    if (rc) {
        set_err(h, rc, "GMM fit: building the scoring handle failed: %s", g->err.c_str());
        vssr_destroy(g);
        return rc;
    }
    *gmm = g;
    return VSSR_OK;
}

// ---- clustering of latent embeddings (cluster.hip) ----------------------------------------------------------------------------------
int vssr_cluster_create(const vssr_cluster_config *cfg, vssr_handle **out) {
    if (!cfg || !out) return set_err(nullptr, VSSR_E_BADARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(vssr_cluster_config))
        return set_err(nullptr, VSSR_E_BADARG, "vssr_cluster_config size mismatch (%u vs %zu)", cfg->struct_size, sizeof(vssr_cluster_config));
    if (cfg->dim < 1 || cfg->dim > 256) return set_err(nullptr, VSSR_E_BADARG, "clustering: dim must be in 1..256 (got %d)", cfg->dim);
    if (cfg->n_components < 1 || cfg->n_components > cfg->dim)
        return set_err(nullptr, VSSR_E_BADARG, "clustering: n_components must be in 1..dim = %d (got %d)", cfg->dim, cfg->n_components);
    if (cfg->cluster_dims < 1 || cfg->cluster_dims > 32)
        return set_err(nullptr, VSSR_E_BADARG, "clustering: cluster_dims must be in 1..32 (got %d)", cfg->cluster_dims);
    if (cfg->whiten != 0 && cfg->whiten != 1) return set_err(nullptr, VSSR_E_BADARG, "clustering: whiten must be 0 or 1 (got %d)", cfg->whiten);
    if (cfg->device < 0) return set_err(nullptr, VSSR_E_BADARG, "device %d out of range", cfg->device);
    vssr_handle *h = new vssr_handle();   // host state only, as vssr_gmm_fit_create
    h->kind = Kind::CLUSTER;
    h->device = cfg->device;
    h->gmm_K = 1;
    h->gmm_D = cfg->dim;
    h->gmm_Dp = 16 * ((cfg->dim + 15) / 16);
    h->fit.reset(new GmmFit());
    h->clu.reset(new Cluster());
    h->clu->n_components = cfg->n_components;
    h->clu->whiten = cfg->whiten;
    h->clu->d_clu = cfg->cluster_dims;
    h->clu->d_pad = cluster_pad_dims(cfg->cluster_dims);
    *out = h;
    return VSSR_OK;
}

int vssr_cluster_append_rows(vssr_handle *h, int64_t n_rows, const double *x) {
    if (int rc = check_kind(h, kind_bit(Kind::CLUSTER), __func__)) return rc;
    if (n_rows < 1 || !x) return set_err(h, VSSR_E_BADARG, "clustering: null or empty rows");
    if (n_rows > (int64_t)INT32_MAX - 64) return set_err(h, VSSR_E_BADARG, "clustering: n_rows %lld out of range", (long long)n_rows);
    const size_t tot = (size_t)n_rows * h->gmm_D;
    for (size_t i = 0; i < tot; ++i)
        if (!std::isfinite(x[i])) return set_err(h, VSSR_E_BADARG, "clustering: row %zu holds a non-finite value", i / h->gmm_D);
    int rc = fit_device(h);
    if (rc) return rc;
    h->clu->pca_done = false;
    return gmm_fit_append_host(h, n_rows, x);
}

int vssr_cluster_append_batch(vssr_handle *h, vssr_handle *painn, int32_t model) {
    if (int rc = check_kind(h, kind_bit(Kind::CLUSTER), __func__)) return rc;
    h->clu->pca_done = false;
    return fit_append_batch(h, painn, model, 1);
}

int vssr_cluster_clear(vssr_handle *h) {
    if (int rc = check_kind(h, kind_bit(Kind::CLUSTER), __func__)) return rc;
    h->fit->n = 0;
    h->clu->pca_done = false;
    h->clu->n_pts = 0;
    return VSSR_OK;
}

int vssr_cluster_pca(vssr_handle *h, vssr_cluster_pca_result *result) {
    if (int rc = check_kind(h, kind_bit(Kind::CLUSTER), __func__)) return rc;
    const int64_t n = h->fit->n;
    if (n < 2) return set_err(h, VSSR_E_BADARG, "clustering: the PCA needs at least 2 rows (%lld resident)", (long long)n);
    if (h->clu->n_components > n)
        return set_err(h, VSSR_E_BADARG, "clustering: n_components = %d must be between 0 and min(n_samples, n_features) = %lld",
                       h->clu->n_components, (long long)std::min<int64_t>(n, h->gmm_D));
    if (h->clu->d_clu > h->clu->n_components)
        return set_err(h, VSSR_E_BADARG, "clustering: cluster_dims %d exceeds n_components %d", h->clu->d_clu, h->clu->n_components);
    int rc = fit_device(h);
    if (rc) return rc;
    return cluster_pca(h, result);
}

int vssr_cluster_pca_params(vssr_handle *h, double *mean, double *components, double *explained_variance, double *ratio) {
    if (int rc = check_kind(h, kind_bit(Kind::CLUSTER), __func__)) return rc;
    if (!h->clu->pca_done) return set_err(h, VSSR_E_STATE, "clustering: no completed PCA");
    VSSR_HIP(h, hipSetDevice(h->device));
    return cluster_pca_params(h, mean, components, explained_variance, ratio);
}

int vssr_cluster_projected(vssr_handle *h, int64_t first, int64_t n_rows, double *xr) {
    if (int rc = check_kind(h, kind_bit(Kind::CLUSTER), __func__)) return rc;
    if (!h->clu->pca_done) return set_err(h, VSSR_E_STATE, "clustering: no completed PCA");
    if (!xr || first < 0 || n_rows < 0 || first + n_rows > h->fit->n)
        return set_err(h, VSSR_E_BADARG, "clustering: rows %lld .. %lld outside the %lld fitted rows", (long long)first,
                       (long long)(first + n_rows), (long long)h->fit->n);
    if (n_rows == 0) return VSSR_OK;
    VSSR_HIP(h, hipSetDevice(h->device));
    return cluster_projected(h, first, n_rows, xr);
}

int vssr_cluster_set_points(vssr_handle *h, int64_t n, const double *p) {
    if (int rc = check_kind(h, kind_bit(Kind::CLUSTER), __func__)) return rc;
    if (n < 2 || !p) return set_err(h, VSSR_E_BADARG, "clustering: at least 2 points are needed");
    if (n > (int64_t)INT32_MAX - 64) return set_err(h, VSSR_E_BADARG, "clustering: %lld points out of range", (long long)n);
    const size_t tot = (size_t)n * h->clu->d_clu;
    for (size_t i = 0; i < tot; ++i)
        if (!std::isfinite(p[i])) return set_err(h, VSSR_E_BADARG, "clustering: point %zu holds a non-finite value", i / h->clu->d_clu);
    int rc = fit_device(h);
    if (rc) return rc;
    return cluster_set_points(h, n, p);
}

int vssr_cluster_linkage(vssr_handle *h, double *Z, int32_t *n_rounds) {
    if (int rc = check_kind(h, kind_bit(Kind::CLUSTER), __func__)) return rc;
    if (!Z) return set_err(h, VSSR_E_BADARG, "null argument");
    if (h->clu->n_pts < 2) return set_err(h, VSSR_E_STATE, "clustering: no points (run vssr_cluster_pca or vssr_cluster_set_points first)");
    VSSR_HIP(h, hipSetDevice(h->device));
    return cluster_linkage(h, Z, n_rounds);
}

}  // extern "C"
