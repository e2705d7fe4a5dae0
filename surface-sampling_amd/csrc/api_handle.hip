// api_handle.hip — handle lifecycle and what the api_*.hip files share: errors, the profiler, the create path, the kind guard,
// the evaluator table, run / synchronise, vssr_destroy.
#include <cmath>
#include <cstdarg>

#include "vssr_internal.h"

namespace vssr {

const char *const kKernelClassNames[KC_COUNT] = {
    "neighbor_list", "embed", "message_mlp", "edge_message_fwd", "update_fwd", "readout",
    "update_bwd", "edge_message_bwd", "message_mlp_bwd", "finalize", "tersoff", "layer0_factorised_fwd",
    "layer0_factorised_bwd", "neb_project", "neb_step", "dimer_advance"};

static thread_local std::string g_create_error;   // per thread: handles may be created concurrently (one host thread per engine)

int set_err(vssr_handle *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_error = buf;
    return code;
}

// ---- profiler ------------------------------------------------------------------------------------------
hipEvent_t Profiler::get_event() {
    if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
void Profiler::begin(int kc, hipStream_t s) {
    if (!enabled) return;
    Rec r{kc, get_event(), get_event()};
    (void)hipEventRecord(r.a, s);
    pending.push_back(r);
}
void Profiler::end(hipStream_t s) {
    if (!enabled) return;
    (void)hipEventRecord(pending.back().b, s);
}
void Profiler::collect() {
    for (auto &r : pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            total_ms[r.kc] += ms;
            launches[r.kc] += 1;
        }
        pool.push_back(r.a);
        pool.push_back(r.b);
    }
    pending.clear();
}
void Profiler::reset() {
    collect();
    for (int k = 0; k < KC_COUNT; ++k) { launches[k] = 0; total_ms[k] = 0; }
}
Profiler::~Profiler() {
    collect();
    for (auto e : pool) (void)hipEventDestroy(e);
}

// ---- kinds ---------------------------------------------------------------------------------------------
const Evaluator &evaluator(const vssr_handle *h) {
    static const Evaluator table[(int)Kind::COUNT] = {
        /* NONE    */ {false, nullptr, nullptr, nullptr},
        /* PAINN   */ {false, painn_run, painn_stress, [](const vssr_handle *h) { return (double)h->cutoff; }},
        /* TERSOFF */ {true, tersoff_run, tersoff_stress, [](const vssr_handle *h) { return h->pot_cutoff; }},
        /* EAM     */ {true, eam_run, eam_stress, [](const vssr_handle *h) { return h->eam_grid.cutoff; }},
        /* SW      */ {true, sw_run, sw_stress, [](const vssr_handle *h) { return h->pot_cutoff; }},
        /* GMM     */ {false, nullptr, nullptr, nullptr},
        /* GMM_FIT */ {false, nullptr, nullptr, nullptr},
        /* CLUSTER */ {false, nullptr, nullptr, nullptr},
        /* PAIR    */ {true, pair_run, pair_stress, [](const vssr_handle *h) { return h->pot_cutoff; }},
        /* VASHISHTA */ {true, vashishta_run, vashishta_stress, [](const vssr_handle *h) { return h->pot_cutoff; }},
    };
    return table[(int)h->kind];
}

// A Gaussian-mixture handle serves vssr_gmm_*, vssr_destroy and vssr_last_error only: every other entry point refuses it; likewise
// a fit handle and vssr_gmm_fit_*, a clustering handle and vssr_cluster_*.
int check_kind(vssr_handle *h, unsigned served, const char *func) {
    if (!h) return VSSR_E_BADARG;
    if (served & kind_bit(h->kind)) return VSSR_OK;
    if (served == kind_bit(Kind::GMM)) return set_err(h, VSSR_E_BADARG, "not a GMM handle");
    if (served == kind_bit(Kind::GMM_FIT)) return set_err(h, VSSR_E_BADARG, "not a GMM fit handle");
    if (served == kind_bit(Kind::CLUSTER)) return set_err(h, VSSR_E_BADARG, "not a clustering handle");
    switch (h->kind) {
    case Kind::GMM: return set_err(h, VSSR_E_BADARG, "%s: a Gaussian-mixture handle serves the vssr_gmm_* calls only", func);
    case Kind::GMM_FIT: return set_err(h, VSSR_E_BADARG, "%s: a Gaussian-mixture fit handle serves the vssr_gmm_fit_* calls only", func);
    case Kind::CLUSTER: return set_err(h, VSSR_E_BADARG, "%s: a clustering handle serves the vssr_cluster_* calls only", func);
    default: return set_err(h, VSSR_E_BADARG, "%s: not served by this handle", func);
    }
}

// ---- create --------------------------------------------------------------------------------------------
int device_in_range(vssr_handle *h, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return set_err(h, VSSR_E_DEVICE, "no HIP device available (this backend has no CPU fallback)");
    if (device < 0 || device >= ndev) return set_err(h, VSSR_E_BADARG, "device %d out of range", device);
    return VSSR_OK;
}

int open_device(vssr_handle *h, int device) {
    h->device = device;
    VSSR_HIP(h, hipSetDevice(device));
    VSSR_HIP(h, hipStreamCreateWithFlags(&h->stream.s, hipStreamNonBlocking));
    VSSR_HIP(h, hipHostMalloc((void **)&h->h_counters.p, sizeof(int) * 4));
    h->h_counters[0] = h->h_counters[1] = h->h_counters[2] = 0;
    return VSSR_OK;
}

void publish_create_error(const vssr_handle *h) {
    if (!h->err.empty()) g_create_error = h->err;
}

// ---- run -----------------------------------------------------------------------------------------------
int run_any(vssr_handle *h, uint32_t want) {
    h->last_want = want;
    return evaluator(h).run(h, want);
}

// The neighbor build overflowed (h_counters[2]): slot_cap becomes what the build counted plus an eighth (cap_tight: the exact need)
int grow_slot_cap(vssr_handle *h) {
    if (h->h_counters[0] <= 0) return set_err(h, VSSR_E_CAPACITY, "neighbor list exceeds 2^31 slots");
    h->slot_cap = (int64_t)h->h_counters[0] + (h->cap_tight ? 0 : (int64_t)h->h_counters[0] / 8) + 64;
    return VSSR_OK;
}

int sync_and_check(vssr_handle *h) {
    const uint32_t want = h->last_want;   // a rerun after a capacity overflow produces what the original run was asked for
    for (int attempt = 0; attempt < 4; ++attempt) {
        VSSR_HIP(h, hipStreamSynchronize(h->stream));
        h->prof.collect();
        if (!h->ran || !h->h_counters[2]) return VSSR_OK;
        int rc = grow_slot_cap(h);
        if (!rc) rc = run_any(h, want);
        if (rc) return rc;
    }
    return set_err(h, VSSR_E_CAPACITY, "neighbor list capacity could not be satisfied");
}

}  // namespace vssr

using namespace vssr;

extern "C" {

int vssr_abi_version(void) { return VSSR_ABI_VERSION; }

const char *vssr_last_error(const vssr_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// The handle's members free what they own (vssr_internal.h); a handle that never reached a device makes no HIP call here.
void vssr_destroy(vssr_handle *h) {
    if (!h) return;
    if (h->stream) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
    }
    delete h;
}

}  // extern "C"
