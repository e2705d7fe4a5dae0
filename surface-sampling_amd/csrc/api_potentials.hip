// api_potentials.hip — the fp64 analytic potentials: Tersoff, EAM, Stillinger-Weber, Vashishta and pair creates, the LAMMPS text parsers,
// and the *_eval_batch entry points.
#include <cmath>

#include "vssr_internal.h"
#include "sw_dev.h"
#include "pair_dev.h"
#include "vashishta_dev.h"

using namespace vssr;

// the potential's tables into pot_params; the two messages: out of memory, failed copy
static int upload_params(vssr_handle *h, const void *src, size_t bytes, const char *nomem, const char *failed) {
    if (h->pot_params.ensure(bytes)) return set_err(h, VSSR_E_NOMEM, "%s", nomem);
    if (hipMemcpy(h->pot_params.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return set_err(h, VSSR_E_DEVICE, "%s", failed);
    return VSSR_OK;
}

extern "C" {

int vssr_tersoff_create(int32_t device, int32_t n_types, const double *params, vssr_handle **out) {
    if (!params || !out || n_types < 1 || n_types > 8) return set_err(nullptr, VSSR_E_BADARG, "bad tersoff arguments");
    *out = nullptr;
    return create_handle(Kind::TERSOFF, device, out, [=](vssr_handle *h) {
        h->n_types = n_types;
        h->n_embed = n_types;
        const size_t np = (size_t)n_types * n_types * n_types;
        double cutmax = 0;
        for (size_t t = 0; t < np; ++t) {
            const double *p = params + 14 * t;
            if (!(p[0] == 1.0 || p[0] == 3.0) || !(p[11] > 0) || !(p[4] != 0)) return set_err(h, VSSR_E_BADARG, "bad tersoff entry %zu", t);
            if (p[10] + p[11] > cutmax) cutmax = p[10] + p[11];
        }
        h->pot_cutoff = cutmax;
        return upload_params(h, params, sizeof(double) * 14 * np, "tersoff params", "tersoff params upload failed");
    });
}

// whitespace-separated tokens of a LAMMPS potential file; `#` starts a comment
static std::vector<std::string> potential_tokens(const char *param_text) {
    std::vector<std::string> tok;
    std::string line, text(param_text);
    size_t pos = 0;
    while (pos <= text.size()) {
        size_t nl = text.find('\n', pos);
        if (nl == std::string::npos) nl = text.size();
        line = text.substr(pos, nl - pos);
        pos = nl + 1;
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.erase(hash);
        size_t i = 0;
        while (i < line.size()) {
            while (i < line.size() && isspace((unsigned char)line[i])) ++i;
            size_t j = i;
            while (j < line.size() && !isspace((unsigned char)line[j])) ++j;
            if (j > i) tok.push_back(line.substr(i, j - i));
            i = j;
        }
    }
    return tok;
}

int vssr_tersoff_create_from_text(int32_t device, const char *param_text, int32_t n_species, const char *const *species,
                                  vssr_handle **out) {
    if (!param_text || !species || !out || n_species < 1 || n_species > 8)
        return set_err(nullptr, VSSR_E_BADARG, "bad tersoff arguments");
    *out = nullptr;
    const std::vector<std::string> tok = potential_tokens(param_text);
    if (tok.empty() || tok.size() % 17) return set_err(nullptr, VSSR_E_BADARG, "tersoff file: token count is not a multiple of 17");
    auto index_of = [&](const std::string &s) {
        for (int t = 0; t < n_species; ++t)
            if (species[t] && s == species[t]) return t;
        return -1;
    };
    const size_t np = (size_t)n_species * n_species * n_species;
    std::vector<double> params(14 * np, 0.0);
    std::vector<char> seen(np, 0);
    for (size_t o = 0; o < tok.size(); o += 17) {
        const int a = index_of(tok[o]), b = index_of(tok[o + 1]), c = index_of(tok[o + 2]);
        if (a < 0 || b < 0 || c < 0) continue;   // entry of another element
        const size_t e = ((size_t)a * n_species + b) * n_species + c;
        for (int k = 0; k < 14; ++k) {
            char *end = nullptr;
            params[14 * e + k] = strtod(tok[o + 3 + k].c_str(), &end);
            if (!end || *end) return set_err(nullptr, VSSR_E_BADARG, "tersoff file: bad number '%s'", tok[o + 3 + k].c_str());
        }
        seen[e] = 1;
    }
    for (size_t e = 0; e < np; ++e)
        if (!seen[e]) return set_err(nullptr, VSSR_E_BADARG, "tersoff file lacks entries for some species triplets");
    return vssr_tersoff_create(device, n_species, params.data(), out);
}

int vssr_eam_create(int32_t device, const vssr_eam_grid *grid, const double *frho, const double *zr, const double *rhor,
                    vssr_handle **out) {
    if (!grid || !frho || !zr || !rhor || !out) return set_err(nullptr, VSSR_E_BADARG, "null EAM argument");
    *out = nullptr;
    if (grid->nrho < 5 || grid->nr < 5 || !(grid->drho > 0) || !(grid->dr > 0) || !(grid->cutoff > 0))
        return set_err(nullptr, VSSR_E_BADARG, "bad EAM grid");
    return create_handle(Kind::EAM, device, out, [=](vssr_handle *h) {
        for (int k = 0; k < grid->nrho; ++k)
            if (!std::isfinite(frho[k])) return set_err(h, VSSR_E_BADARG, "non-finite EAM table entry");
        for (int k = 0; k < grid->nr; ++k)
            if (!std::isfinite(zr[k]) || !std::isfinite(rhor[k])) return set_err(h, VSSR_E_BADARG, "non-finite EAM table entry");
        h->n_types = 1;
        h->n_embed = 1;
        h->eam_grid = *grid;
        // spline tables: frho [nrho + 1][7] | rhor [nr + 1][7] | z2r [nr + 1][7]   (LAMMPS file2array + array2spline for one file)
        const size_t nF = 7 * (size_t)(grid->nrho + 1), nR = 7 * (size_t)(grid->nr + 1);
        std::vector<double> tab(nF + 2 * nR), z2r(grid->nr);
        for (int k = 0; k < grid->nr; ++k) z2r[k] = 27.2 * 0.529 * zr[k] * zr[k];
        eam_build_spline(frho, grid->nrho, grid->drho, tab.data());
        eam_build_spline(rhor, grid->nr, grid->dr, tab.data() + nF);
        eam_build_spline(z2r.data(), grid->nr, grid->dr, tab.data() + nF + nR);
        return upload_params(h, tab.data(), sizeof(double) * tab.size(), "EAM tables", "EAM table upload failed");
    });
}

}  // extern "C"

// eam/alloy, eam/fs (u = w = nullptr) and adp (fs = 0; u, w [n_elem (n_elem + 1) / 2][nr]) behind their two exported names
static int eam_create_typed(int32_t device, int32_t n_elem, int32_t fs, const vssr_eam_grid *grid, const double *frho,
                            const double *rhor, const double *z2r, const double *u, const double *w, vssr_handle **out) {
    if (!grid || !frho || !rhor || !z2r || !out) return set_err(nullptr, VSSR_E_BADARG, "null EAM argument");
    *out = nullptr;
    if (n_elem < 1 || n_elem > 8) return set_err(nullptr, VSSR_E_BADARG, "EAM: %d elements (1 .. 8 are supported)", n_elem);
    if (grid->nrho < 5 || grid->nr < 5 || !(grid->drho > 0) || !(grid->dr > 0) || !(grid->cutoff > 0) ||
        !std::isfinite(grid->drho) || !std::isfinite(grid->dr) || !std::isfinite(grid->cutoff))
        return set_err(nullptr, VSSR_E_BADARG, "bad EAM grid");
    const int nR = fs ? n_elem * n_elem : n_elem, nP = n_elem * (n_elem + 1) / 2;
    const size_t cF = (size_t)n_elem * grid->nrho, cR = (size_t)nR * grid->nr, cP = (size_t)nP * grid->nr;
    for (size_t k = 0; k < cF; ++k)
        if (!std::isfinite(frho[k])) return set_err(nullptr, VSSR_E_BADARG, "non-finite EAM table entry (F)");
    for (size_t k = 0; k < cR; ++k)
        if (!std::isfinite(rhor[k])) return set_err(nullptr, VSSR_E_BADARG, "non-finite EAM table entry (rho)");
    for (size_t k = 0; k < cP; ++k)
        if (!std::isfinite(z2r[k])) return set_err(nullptr, VSSR_E_BADARG, "non-finite EAM table entry (r phi)");
    for (size_t k = 0; u && k < cP; ++k)
        if (!std::isfinite(u[k]) || !std::isfinite(w[k])) return set_err(nullptr, VSSR_E_BADARG, "non-finite ADP table entry (u, w)");
    return create_handle(Kind::EAM, device, out, [=](vssr_handle *h) {
        h->n_types = n_elem;
        h->n_embed = n_elem;   // vssr_batch_upload refuses types outside [0, n_elem)
        h->eam_nel = n_elem;
        h->eam_fs = fs ? 1 : 0;
        h->eam_adp = u != nullptr;
        h->eam_grid = *grid;
        // spline tables (eam_dev.h EamTyped): F [n][nrho + 1][7] | rho [nR][nr + 1][7] | r phi [nP][nr + 1][7]; an ADP handle
        // (adp_dev.h AdpTyped) appends u [nP][nr + 1][7] | w [nP][nr + 1][7]
        const size_t sF = 7 * (size_t)(grid->nrho + 1), sR = 7 * (size_t)(grid->nr + 1);
        std::vector<double> tab(sF * n_elem + sR * (nR + nP + (u ? 2 * nP : 0)));
        for (int t = 0; t < n_elem; ++t) eam_build_spline(frho + (size_t)t * grid->nrho, grid->nrho, grid->drho, tab.data() + sF * t);
        double *R = tab.data() + sF * n_elem;
        for (int t = 0; t < nR; ++t) eam_build_spline(rhor + (size_t)t * grid->nr, grid->nr, grid->dr, R + sR * t);
        for (int t = 0; t < nP; ++t) eam_build_spline(z2r + (size_t)t * grid->nr, grid->nr, grid->dr, R + sR * (nR + t));
        for (int t = 0; u && t < nP; ++t) {
            eam_build_spline(u + (size_t)t * grid->nr, grid->nr, grid->dr, R + sR * (nR + nP + t));
            eam_build_spline(w + (size_t)t * grid->nr, grid->nr, grid->dr, R + sR * (nR + 2 * nP + t));
        }
        return upload_params(h, tab.data(), sizeof(double) * tab.size(), "EAM tables", "EAM table upload failed");
    });
}

extern "C" {

int vssr_eam_create_alloy(int32_t device, int32_t n_elem, int32_t fs, const vssr_eam_grid *grid, const double *frho,
                          const double *rhor, const double *z2r, vssr_handle **out) {
    return eam_create_typed(device, n_elem, fs, grid, frho, rhor, z2r, nullptr, nullptr, out);
}

int vssr_eam_create_adp(int32_t device, int32_t n_elem, const vssr_eam_grid *grid, const double *frho, const double *rhor,
                        const double *z2r, const double *u, const double *w, vssr_handle **out) {
    if (out) *out = nullptr;
    if (!u || !w) return set_err(nullptr, VSSR_E_BADARG, "null ADP argument (u, w)");
    return eam_create_typed(device, n_elem, 0, grid, frho, rhor, z2r, u, w, out);
}

// ---- Stillinger-Weber ------------------------------------------------------------------------------------------------------
static const char *const kSwField[11] = {"eps", "sig", "a", "lambda", "gamma", "costheta0", "A", "B", "p", "q", "tol"};

// Checks an [i][j][k] table of 11 LAMMPS columns and derives the kernels' entries (sw_dev.h SwP).  Refused: non-finite numbers,
// eps / sig / a <= 0, negative lambda / gamma / A / B / p / q / tol (pair_sw.cpp refuses those as well), and (i, j, k) / (i, k, j)
// pairs that differ in eps, lambda or costheta0 (the LAMMPS energy would depend on the order of its neighbor list).
static int sw_derive(int nt, const double *params, const char *const *species, std::vector<SwP> &out, double &cutmax) {
    const size_t np = (size_t)nt * nt * nt;
    auto name = [&](size_t e, char *buf, size_t n) {
        const int a = (int)(e / ((size_t)nt * nt)), b = (int)(e / nt % nt), c = (int)(e % nt);
        if (species) snprintf(buf, n, "%s %s %s", species[a], species[b], species[c]);
        else snprintf(buf, n, "(%d,%d,%d)", a, b, c);
    };
    char nm[96];
    out.assign(np, SwP{});
    cutmax = 0.0;
    for (size_t e = 0; e < np; ++e) {
        const double *p = params + 11 * e;
        for (int k = 0; k < 11; ++k) {
            const bool pos = k == 0 || k == 1 || k == 2;   // eps, sig, a
            const bool any = k == 5;                       // costheta0: any finite value
            if (!std::isfinite(p[k]) || (pos && !(p[k] > 0)) || (!pos && !any && !(p[k] >= 0))) {
                name(e, nm, sizeof nm);
                return set_err(nullptr, VSSR_E_BADARG, "sw entry %s: bad %s = %g (%s)", nm, kSwField[k], p[k],
                               pos ? "must be > 0" : any ? "must be finite" : "must be >= 0");
            }
        }
        const double eps = p[0], sig = p[1], a = p[2], lam = p[3], gam = p[4], A = p[6], B = p[7], pp = p[8], qq = p[9];
        SwP &d = out[e];
        d.cut = a * sig; d.sig = sig; d.gs = gam * sig;
        d.c5 = A * eps * B * pow(sig, pp); d.c6 = A * eps * pow(sig, qq);
        d.p = pp; d.q = qq; d.le = lam * eps; d.c0 = p[5]; d.pad0 = 0.0; d.pad1 = 0.0;
        if (!std::isfinite(d.c5) || !std::isfinite(d.c6)) {
            name(e, nm, sizeof nm);
            return set_err(nullptr, VSSR_E_BADARG, "sw entry %s: A eps B sig^p / A eps sig^q overflow", nm);
        }
        cutmax = std::max(cutmax, d.cut);
    }
    for (int i = 0; i < nt; ++i)
        for (int j = 0; j < nt; ++j)
            for (int k = j + 1; k < nt; ++k) {
                const double *x = params + 11 * (((size_t)i * nt + j) * nt + k), *y = params + 11 * (((size_t)i * nt + k) * nt + j);
                for (int f : {0, 3, 5})
                    if (x[f] != y[f]) {
                        name(((size_t)i * nt + j) * nt + k, nm, sizeof nm);
                        char nm2[96];
                        name(((size_t)i * nt + k) * nt + j, nm2, sizeof nm2);
                        return set_err(nullptr, VSSR_E_BADARG,
                                       "sw entries %s and %s differ in %s (%g vs %g): the three-body term would depend on neighbor order",
                                       nm, nm2, kSwField[f], x[f], y[f]);
                    }
            }
    return VSSR_OK;
}

static int sw_create_checked(int32_t device, int32_t n_types, const double *params, const char *const *species, vssr_handle **out) {
    if (!params || !out || n_types < 1 || n_types > 8) return set_err(nullptr, VSSR_E_BADARG, "bad sw arguments (1 .. 8 types)");
    *out = nullptr;
    std::vector<SwP> tab;
    double cutmax = 0.0;
    int rc = sw_derive(n_types, params, species, tab, cutmax);
    if (rc) return rc;
    return create_handle(Kind::SW, device, out, [&](vssr_handle *h) {
        h->n_types = n_types;
        h->n_embed = n_types;
        h->pot_cutoff = cutmax;
        return upload_params(h, tab.data(), sizeof(SwP) * tab.size(), "sw params", "sw params upload failed");
    });
}

int vssr_sw_create(int32_t device, int32_t n_types, const double *params, vssr_handle **out) {
    return sw_create_checked(device, n_types, params, nullptr, out);
}

int vssr_sw_create_from_text(int32_t device, const char *param_text, int32_t n_species, const char *const *species,
                             vssr_handle **out) {
    if (!param_text || !species || !out || n_species < 1 || n_species > 8)
        return set_err(nullptr, VSSR_E_BADARG, "bad sw arguments (1 .. 8 species)");
    *out = nullptr;
    for (int t = 0; t < n_species; ++t)
        if (!species[t] || !species[t][0]) return set_err(nullptr, VSSR_E_BADARG, "sw: species %d has no name", t);
    const std::vector<std::string> tok = potential_tokens(param_text);
    if (tok.empty() || tok.size() % 14)
        return set_err(nullptr, VSSR_E_BADARG, "sw file: %zu tokens, not a multiple of 14 (e1 e2 e3 + 11 numbers)", tok.size());
    auto index_of = [&](const std::string &s) {
        for (int t = 0; t < n_species; ++t)
            if (s == species[t]) return t;
        return -1;
    };
    const size_t np = (size_t)n_species * n_species * n_species;
    std::vector<double> params(11 * np, 0.0);
    std::vector<char> seen(np, 0);
    for (size_t o = 0; o < tok.size(); o += 14) {
        const int a = index_of(tok[o]), b = index_of(tok[o + 1]), c = index_of(tok[o + 2]);
        if (a < 0 || b < 0 || c < 0) continue;   // entry of another element
        const size_t e = ((size_t)a * n_species + b) * n_species + c;
        for (int k = 0; k < 11; ++k) {
            char *end = nullptr;
            params[11 * e + k] = strtod(tok[o + 3 + k].c_str(), &end);
            if (!end || *end || end == tok[o + 3 + k].c_str())
                return set_err(nullptr, VSSR_E_BADARG, "sw file: entry %s %s %s: bad number '%s' for %s", tok[o].c_str(),
                               tok[o + 1].c_str(), tok[o + 2].c_str(), tok[o + 3 + k].c_str(), kSwField[k]);
        }
        seen[e] = 1;
    }
    for (size_t e = 0; e < np; ++e)
        if (!seen[e])
            return set_err(nullptr, VSSR_E_BADARG, "sw file lacks the entry %s %s %s", species[e / ((size_t)n_species * n_species)],
                           species[e / n_species % n_species], species[e % n_species]);
    return sw_create_checked(device, n_species, params.data(), species, out);
}

// ---- Vashishta -----------------------------------------------------------------------------------------------------------------
static const char *const kVaField[14] = {"H", "eta", "Zi", "Zj", "lambda1", "D", "lambda4", "W", "rc", "B", "gamma", "r0", "C", "costheta"};

// Checks an [i][j][k] table of 14 LAMMPS columns and derives the kernels' entries (vashishta_dev.h VashP).  Refused: non-finite
// numbers and negative B / gamma / r0 in any entry; in the entries (i, j, j), whose two-body and radial columns are the ones read:
// rc <= 0, eta <= 0, lambda1 <= 0 with Zi Zj != 0, lambda4 <= 0 with D != 0, r0 > rc; (i, j, j) / (j, i, i) pairs that differ in
// H, eta, Zi Zj, lambda1, D, lambda4, W or rc and (i, j, k) / (i, k, j) pairs that differ in B, C or costheta (the LAMMPS energy would
// depend on the order of its neighbor list).  The two-body columns of an entry with j != k are read by nobody and only have to be finite.
static int vashishta_derive(int nt, const double *params, const char *const *species, std::vector<VashP> &out, double &cutmax,
                            double &r0max) {
    const size_t np = (size_t)nt * nt * nt;
    auto name = [&](size_t e, char *buf, size_t n) {
        const int a = (int)(e / ((size_t)nt * nt)), b = (int)(e / nt % nt), c = (int)(e % nt);
        if (species) snprintf(buf, n, "%s %s %s", species[a], species[b], species[c]);
        else snprintf(buf, n, "(%d,%d,%d)", a, b, c);
    };
    char nm[96], nm2[96];
    auto bad = [&](size_t e, int k, const char *rule) {
        name(e, nm, sizeof nm);
        return set_err(nullptr, VSSR_E_BADARG, "vashishta entry %s: bad %s = %g (%s)", nm, kVaField[k], params[14 * e + k], rule);
    };
    out.assign(np, VashP{});
    cutmax = 0.0;
    r0max = 0.0;
    for (size_t e = 0; e < np; ++e) {
        const double *p = params + 14 * e;
        for (int k = 0; k < 14; ++k)
            if (!std::isfinite(p[k])) return bad(e, k, "must be finite");
        for (int k : {9, 10, 11})
            if (!(p[k] >= 0)) return bad(e, k, "must be >= 0");
        VashP &d = out[e];
        d.tri.B = p[9]; d.tri.C = p[12]; d.tri.c0 = p[13];
        const int b = (int)(e / nt % nt), c = (int)(e % nt);
        if (b != c) continue;
        const double zz = p[2] * p[3];
        if (!(p[8] > 0)) return bad(e, 8, "must be > 0");
        if (!(p[1] > 0)) return bad(e, 1, "must be > 0");
        if (zz != 0.0 && !(p[4] > 0)) return bad(e, 4, "must be > 0 with Zi Zj != 0");
        if (p[5] != 0.0 && !(p[6] > 0)) return bad(e, 6, "must be > 0 with D != 0");
        if (p[11] > p[8]) return bad(e, 11, "must be <= rc");
        VashPairP &t = d.two;
        t.H = p[0]; t.eta = p[1]; t.zz = PAIR_QQRD2E * zz; t.il1 = zz != 0.0 ? 1.0 / p[4] : 0.0;
        t.D = p[5]; t.il4 = p[5] != 0.0 ? 1.0 / p[6] : 0.0; t.W = p[7]; t.rc = p[8];
        t.gamma = p[10]; t.r0 = p[11];
        vash_v(t, t.rc, t.vrc, t.dvrc);
        if (!std::isfinite(t.vrc) || !std::isfinite(t.dvrc)) {
            name(e, nm, sizeof nm);
            return set_err(nullptr, VSSR_E_BADARG, "vashishta entry %s: V(rc) / V'(rc) overflow", nm);
        }
        cutmax = std::max(cutmax, t.rc);
        r0max = std::max(r0max, t.r0);
    }
    auto differ = [&](size_t x, size_t y, const char *field, double a, double b, const char *what) {
        name(x, nm, sizeof nm);
        name(y, nm2, sizeof nm2);
        return set_err(nullptr, VSSR_E_BADARG, "vashishta entries %s and %s differ in %s (%g vs %g): the %s term would depend on neighbor order",
                       nm, nm2, field, a, b, what);
    };
    for (int i = 0; i < nt; ++i)
        for (int j = i + 1; j < nt; ++j) {
            const size_t x = ((size_t)i * nt + j) * nt + j, y = ((size_t)j * nt + i) * nt + i;
            const double *a = params + 14 * x, *b = params + 14 * y;
            for (int f : {0, 1, 4, 5, 6, 7, 8})
                if (a[f] != b[f]) return differ(x, y, kVaField[f], a[f], b[f], "two-body");
            if (a[2] * a[3] != b[2] * b[3]) return differ(x, y, "Zi Zj", a[2] * a[3], b[2] * b[3], "two-body");
        }
    for (int i = 0; i < nt; ++i)
        for (int j = 0; j < nt; ++j)
            for (int k = j + 1; k < nt; ++k) {
                const size_t x = ((size_t)i * nt + j) * nt + k, y = ((size_t)i * nt + k) * nt + j;
                for (int f : {9, 12, 13})
                    if (params[14 * x + f] != params[14 * y + f])
                        return differ(x, y, kVaField[f], params[14 * x + f], params[14 * y + f], "three-body");
            }
    return VSSR_OK;
}

static int vashishta_create_checked(int32_t device, int32_t n_types, const double *params, const char *const *species, vssr_handle **out) {
    if (!params || !out || n_types < 1 || n_types > VA_MAXT) return set_err(nullptr, VSSR_E_BADARG, "bad vashishta arguments (1 .. 8 types)");
    *out = nullptr;
    std::vector<VashP> tab;
    double cutmax = 0.0, r0max = 0.0;
    int rc = vashishta_derive(n_types, params, species, tab, cutmax, r0max);
    if (rc) return rc;
    return create_handle(Kind::VASHISHTA, device, out, [&](vssr_handle *h) {
        h->n_types = n_types;
        h->n_embed = n_types;
        h->pot_cutoff = cutmax;
        h->vash_r0max = r0max;
        return upload_params(h, tab.data(), sizeof(VashP) * tab.size(), "vashishta params", "vashishta params upload failed");
    });
}

int vssr_vashishta_create(int32_t device, int32_t n_types, const double *params, vssr_handle **out) {
    return vashishta_create_checked(device, n_types, params, nullptr, out);
}

int vssr_vashishta_create_from_text(int32_t device, const char *param_text, int32_t n_species, const char *const *species,
                                    vssr_handle **out) {
    if (!param_text || !species || !out || n_species < 1 || n_species > VA_MAXT)
        return set_err(nullptr, VSSR_E_BADARG, "bad vashishta arguments (1 .. 8 species)");
    *out = nullptr;
    for (int t = 0; t < n_species; ++t)
        if (!species[t] || !species[t][0]) return set_err(nullptr, VSSR_E_BADARG, "vashishta: species %d has no name", t);
    const std::vector<std::string> tok = potential_tokens(param_text);
    if (tok.empty() || tok.size() % 17)
        return set_err(nullptr, VSSR_E_BADARG, "vashishta file: %zu tokens, not a multiple of 17 (e1 e2 e3 + 14 numbers)", tok.size());
    auto index_of = [&](const std::string &s) {
        for (int t = 0; t < n_species; ++t)
            if (s == species[t]) return t;
        return -1;
    };
    const size_t np = (size_t)n_species * n_species * n_species;
    std::vector<double> params(14 * np, 0.0);
    std::vector<char> seen(np, 0);
    for (size_t o = 0; o < tok.size(); o += 17) {
        const int a = index_of(tok[o]), b = index_of(tok[o + 1]), c = index_of(tok[o + 2]);
        if (a < 0 || b < 0 || c < 0) continue;   // entry of another element
        const size_t e = ((size_t)a * n_species + b) * n_species + c;
        for (int k = 0; k < 14; ++k) {
            char *end = nullptr;
            params[14 * e + k] = strtod(tok[o + 3 + k].c_str(), &end);
            if (!end || *end || end == tok[o + 3 + k].c_str())
                return set_err(nullptr, VSSR_E_BADARG, "vashishta file: entry %s %s %s: bad number '%s' for %s", tok[o].c_str(),
                               tok[o + 1].c_str(), tok[o + 2].c_str(), tok[o + 3 + k].c_str(), kVaField[k]);
        }
        seen[e] = 1;
    }
    for (size_t e = 0; e < np; ++e)
        if (!seen[e])
            return set_err(nullptr, VSSR_E_BADARG, "vashishta file lacks the entry %s %s %s", species[e / ((size_t)n_species * n_species)],
                           species[e / n_species % n_species], species[e % n_species]);
    return vashishta_create_checked(device, n_species, params.data(), species, out);
}

// ---- pair potentials --------------------------------------------------------------------------------------------------------
static const char *const kPairStyle[7] = {"none", "lj/cut", "morse", "buck", "born", "coul/dsf", "coul/long"};

// Checks one caller term and derives the kernel's entry (pair_dev.h PairTerm); qq = q_a q_b, g: the Ewald damping of a coul/long term.
static int pair_derive(const vssr_pair_term &t, int idx, double qq, double g, PairTerm &d) {
    static const int n_coef[7] = {0, 2, 3, 3, 5, 1, 0};
    const char *nm = kPairStyle[t.style];
    for (int k = 0; k < n_coef[t.style]; ++k)
        if (!std::isfinite(t.c[k])) return set_err(nullptr, VSSR_E_BADARG, "pair term %d (%s %d %d): coefficient %d is not finite", idx, nm, t.type_a, t.type_b, k);
    if (!std::isfinite(t.rc) || !(t.rc > 0)) return set_err(nullptr, VSSR_E_BADARG, "pair term %d (%s %d %d): bad cutoff %g (must be > 0)", idx, nm, t.type_a, t.type_b, t.rc);
    d = PairTerm{};
    d.style = t.style;
    d.rc = t.rc;
    const double rc = t.rc;
    double e_rc = 0.0;
    switch (t.style) {
    case VSSR_PAIR_LJ_CUT: {
        if (!(t.c[1] > 0)) return set_err(nullptr, VSSR_E_BADARG, "pair term %d (lj/cut %d %d): bad sigma %g (must be > 0)", idx, t.type_a, t.type_b, t.c[1]);
        d.c[0] = t.c[0]; d.c[1] = t.c[1];
        const double s6 = pow(t.c[1] / rc, 6.0);
        e_rc = 4.0 * t.c[0] * s6 * (s6 - 1.0);
        break;
    }
    case VSSR_PAIR_MORSE: {
        d.c[0] = t.c[0]; d.c[1] = t.c[1]; d.c[2] = t.c[2];
        const double x = exp(-t.c[1] * (rc - t.c[2]));
        e_rc = t.c[0] * (x * x - 2.0 * x);
        break;
    }
    case VSSR_PAIR_BUCK:
    case VSSR_PAIR_BORN: {
        if (!(t.c[1] > 0)) return set_err(nullptr, VSSR_E_BADARG, "pair term %d (%s %d %d): bad rho %g (must be > 0)", idx, nm, t.type_a, t.type_b, t.c[1]);
        d.c[0] = t.c[0]; d.c[1] = 1.0 / t.c[1];
        if (t.style == VSSR_PAIR_BUCK) {
            d.c[2] = t.c[2];
            e_rc = t.c[0] * exp(-rc * d.c[1]) - t.c[2] / pow(rc, 6.0);
        } else {
            d.c[2] = t.c[2]; d.c[3] = t.c[3]; d.c[4] = t.c[4];
            e_rc = t.c[0] * exp((t.c[2] - rc) * d.c[1]) - t.c[3] / pow(rc, 6.0) + t.c[4] / pow(rc, 8.0);
        }
        break;
    }
    case VSSR_PAIR_COUL_LONG:
        d.c[0] = g;
        d.c[3] = PAIR_QQRD2E * qq;
        break;
    default: {   // coul/dsf
        const double a = t.c[0];
        if (!(a >= 0)) return set_err(nullptr, VSSR_E_BADARG, "pair term %d (coul/dsf %d %d): bad alpha %g (must be >= 0)", idx, t.type_a, t.type_b, a);
        const double ec = erfc(a * rc);
        d.c[0] = a;
        d.c[1] = ec / rc;
        d.c[2] = ec / (rc * rc) + PAIR_2_SQRTPI * a * exp(-a * a * rc * rc) / rc;
        d.c[3] = PAIR_QQRD2E * qq;
        break;
    }
    }
    if (t.style != VSSR_PAIR_COUL_DSF && t.style != VSSR_PAIR_COUL_LONG && t.shift) {
        if (!std::isfinite(e_rc)) return set_err(nullptr, VSSR_E_BADARG, "pair term %d (%s %d %d): E(rc) is not finite", idx, nm, t.type_a, t.type_b);
        d.eshift = e_rc;
    }
    return VSSR_OK;
}

// vssr_pair_create (ks == nullptr), vssr_pair_create_kspace (slab 0) and vssr_pair_create_kspace_slab (the slab factor, checked there)
static int pair_create(int32_t device, int32_t n_types, int32_t n_terms, const vssr_pair_term *terms, const double *charge,
                       const vssr_kspace *ks, double slab, vssr_handle **out) {
    if (!terms || !out || n_terms < 1) return set_err(nullptr, VSSR_E_BADARG, "bad pair arguments");
    *out = nullptr;
    if (ks) {
        if (!charge) return set_err(nullptr, VSSR_E_BADARG, "pair: an Ewald sum needs per-type charges (charge is NULL)");
        if (!std::isfinite(ks->g_ewald) || !(ks->g_ewald > 0) || !std::isfinite(ks->k_cut) || !(ks->k_cut > 0))
            return set_err(nullptr, VSSR_E_BADARG, "pair: bad k-space parameters g_ewald %g, k_cut %g (both must be finite and > 0)", ks->g_ewald, ks->k_cut);
    }
    if (n_types < 1 || n_types > PAIR_MAX_TYPES) return set_err(nullptr, VSSR_E_BADARG, "pair: %d types (1 .. 8 are supported)", n_types);
    if (charge)
        for (int t = 0; t < n_types; ++t)
            if (!std::isfinite(charge[t])) return set_err(nullptr, VSSR_E_BADARG, "pair: the charge of type %d is not finite", t);
    std::vector<PairTable> tab(1);
    memset(tab.data(), 0, sizeof(PairTable));
    PairTable &T = tab[0];
    int count[PAIR_MAX_TYPES][PAIR_MAX_TYPES] = {};
    double cutmax = 0.0, dsf_alpha = 0.0, dsf_rc = 0.0;
    bool dsf = false, dsf_type[PAIR_MAX_TYPES] = {};
    bool long_pair[PAIR_MAX_TYPES][PAIR_MAX_TYPES] = {};
    int n_long = 0;
    double long_rc = 0.0;
    for (int n = 0; n < n_terms; ++n) {
        const vssr_pair_term &t = terms[n];
        if (t.type_a < 0 || t.type_a >= n_types || t.type_b < 0 || t.type_b >= n_types)
            return set_err(nullptr, VSSR_E_BADARG, "pair term %d: types %d %d outside [0,%d)", n, t.type_a, t.type_b, n_types);
        if (t.style < VSSR_PAIR_LJ_CUT || t.style > VSSR_PAIR_COUL_LONG) return set_err(nullptr, VSSR_E_BADARG, "pair term %d: unknown style %d", n, t.style);
        if (t.style == VSSR_PAIR_COUL_LONG && !ks)
            return set_err(nullptr, VSSR_E_BADARG, "pair term %d: coul/long is the real-space part of an Ewald sum: create the handle with "
                           "vssr_pair_create_kspace", n);
        if (t.style == VSSR_PAIR_COUL_DSF && !charge)
            return set_err(nullptr, VSSR_E_BADARG, "pair term %d: coul/dsf needs per-type charges (charge is NULL)", n);
        PairTerm d;
        if (int rc = pair_derive(t, n, charge ? charge[t.type_a] * charge[t.type_b] : 0.0, ks ? ks->g_ewald : 0.0, d)) return rc;
        if (t.style == VSSR_PAIR_COUL_LONG) {
            if (n_long && t.rc != long_rc)
                return set_err(nullptr, VSSR_E_BADARG, "pair term %d: coul/long terms differ in rc (%g vs %g)", n, t.rc, long_rc);
            if (long_pair[t.type_a][t.type_b])
                return set_err(nullptr, VSSR_E_BADARG, "pair term %d: a second coul/long term on the type pair %d %d", n, t.type_a, t.type_b);
            long_pair[t.type_a][t.type_b] = long_pair[t.type_b][t.type_a] = true;
            long_rc = t.rc;
            ++n_long;
        }
        if (t.style == VSSR_PAIR_COUL_DSF) {
            if (dsf && (t.c[0] != dsf_alpha || t.rc != dsf_rc))
                return set_err(nullptr, VSSR_E_BADARG, "pair term %d: coul/dsf terms differ in alpha or rc (%g %g vs %g %g)", n, t.c[0], t.rc, dsf_alpha, dsf_rc);
            dsf = true; dsf_alpha = t.c[0]; dsf_rc = t.rc;
            dsf_type[t.type_a] = dsf_type[t.type_b] = true;
        }
        const int a = t.type_a, b = t.type_b;
        if (count[a][b] >= PAIR_MAX_TERMS)
            return set_err(nullptr, VSSR_E_BADARG, "pair term %d: more than %d terms on the type pair %d %d", n, PAIR_MAX_TERMS, a, b);
        T.term[(a * PAIR_MAX_TYPES + b) * PAIR_MAX_TERMS + count[a][b]] = d;
        if (a != b) T.term[(b * PAIR_MAX_TYPES + a) * PAIR_MAX_TERMS + count[a][b]] = d;
        count[a][b] += 1;
        count[b][a] = count[a][b];
        cutmax = std::max(cutmax, t.rc);
    }
    if (dsf)
        for (int t = 0; t < n_types; ++t)
            if (dsf_type[t])
                T.self_e[t] = -(erfc(dsf_alpha * dsf_rc) / (2.0 * dsf_rc) + 0.5 * PAIR_2_SQRTPI * dsf_alpha) * PAIR_QQRD2E * charge[t] * charge[t];
    if (ks) {
        if (dsf) return set_err(nullptr, VSSR_E_BADARG, "pair: coul/long and coul/dsf terms in one handle (one Coulomb sum at a time)");
        for (int a = 0; a < n_types; ++a)
            for (int b = a; b < n_types; ++b)
                if (!long_pair[a][b])
                    return set_err(nullptr, VSSR_E_BADARG, "pair: the coul/long terms do not cover the type pair %d %d (the reciprocal sum runs over every "
                                   "pair of charges, so must the real-space part)", a, b);
    }
    return create_handle(Kind::PAIR, device, out, [&](vssr_handle *h) {
        h->n_types = n_types;
        h->n_embed = n_types;
        h->pot_cutoff = cutmax;
        if (ks) {
            h->ew_on = true;
            h->ew_g = ks->g_ewald;
            h->ew_kcut = ks->k_cut;
            h->ew_slab = slab;
            for (int t = 0; t < n_types; ++t) h->ew_q[t] = charge[t];
        }
        return upload_params(h, tab.data(), sizeof(PairTable), "pair table", "pair table upload failed");
    });
}

int vssr_pair_create(int32_t device, int32_t n_types, int32_t n_terms, const vssr_pair_term *terms, const double *charge,
                     vssr_handle **out) {
    return pair_create(device, n_types, n_terms, terms, charge, nullptr, 0.0, out);
}

int vssr_pair_create_kspace(int32_t device, int32_t n_types, int32_t n_terms, const vssr_pair_term *terms, const double *charge,
                            const vssr_kspace *ks, vssr_handle **out) {
    if (!ks) return set_err(nullptr, VSSR_E_BADARG, "vssr_pair_create_kspace: null k-space parameters");
    return pair_create(device, n_types, n_terms, terms, charge, ks, 0.0, out);
}

int vssr_pair_create_kspace_slab(int32_t device, int32_t n_types, int32_t n_terms, const vssr_pair_term *terms, const double *charge,
                                 const vssr_kspace *ks, double slab_factor, vssr_handle **out) {
    if (!ks) return set_err(nullptr, VSSR_E_BADARG, "vssr_pair_create_kspace_slab: null k-space parameters");
    if (!std::isfinite(slab_factor) || !(slab_factor > 1.0))
        return set_err(nullptr, VSSR_E_BADARG, "pair: bad slab parameter %g (the slab factor must be finite and > 1.0)", slab_factor);
    return pair_create(device, n_types, n_terms, terms, charge, ks, slab_factor, out);
}

}  // extern "C"

// ---- evaluation with fp64 results: one body behind the five exported names ------------------------------------------------------
static int analytic_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                               const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                               double *energy_atoms_f64, double *forces_f64) {
    // (a refusal names the Tersoff entry point whichever of the five was called: the message is kept as it always was)
    if (int rc = check_kind(h, KINDS_EVAL, "vssr_tersoff_eval_batch")) return rc;
    if (!is_analytic(h)) return set_err(h, VSSR_E_STATE, "not a Tersoff / EAM / SW handle");
    vssr_out dummy;
    memset(&dummy, 0, sizeof dummy);
    int rc = vssr_eval_batch(h, n_cfg, n_atoms, type, pos, cell, pbc, want, out ? out : &dummy);
    if (rc) return rc;
    if (energy_f64) VSSR_HIP(h, hipMemcpy(energy_f64, h->d_pot_e.p, sizeof(double) * h->n_cfg, hipMemcpyDeviceToHost));
    if (energy_atoms_f64)
        VSSR_HIP(h, hipMemcpy(energy_atoms_f64, h->d_pot_ea.p, sizeof(double) * h->n_atoms, hipMemcpyDeviceToHost));
    if (forces_f64)
        VSSR_HIP(h, hipMemcpy(forces_f64, h->d_pot_f.p, sizeof(double) * 3 * h->n_atoms, hipMemcpyDeviceToHost));
    return VSSR_OK;
}

extern "C" {

int vssr_tersoff_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type,
                            const double *pos, const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out,
                            double *energy_f64, double *energy_atoms_f64, double *forces_f64) {
    return analytic_eval_batch(h, n_cfg, n_atoms, type, pos, cell, pbc, want, out, energy_f64, energy_atoms_f64, forces_f64);
}

int vssr_eam_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                        const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                        double *energy_atoms_f64, double *forces_f64) {
    return analytic_eval_batch(h, n_cfg, n_atoms, type, pos, cell, pbc, want, out, energy_f64, energy_atoms_f64, forces_f64);
}

int vssr_sw_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                       const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                       double *energy_atoms_f64, double *forces_f64) {
    return analytic_eval_batch(h, n_cfg, n_atoms, type, pos, cell, pbc, want, out, energy_f64, energy_atoms_f64, forces_f64);
}

int vssr_vashishta_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                              const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                              double *energy_atoms_f64, double *forces_f64) {
    return analytic_eval_batch(h, n_cfg, n_atoms, type, pos, cell, pbc, want, out, energy_f64, energy_atoms_f64, forces_f64);
}

int vssr_pair_eval_batch(vssr_handle *h, int32_t n_cfg, const int32_t *n_atoms, const int32_t *type, const double *pos,
                         const double *cell, const uint8_t *pbc, uint32_t want, vssr_out *out, double *energy_f64,
                         double *energy_atoms_f64, double *forces_f64) {
    return analytic_eval_batch(h, n_cfg, n_atoms, type, pos, cell, pbc, want, out, energy_f64, energy_atoms_f64, forces_f64);
}

}  // extern "C"
