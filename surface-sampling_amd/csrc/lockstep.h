// lockstep.h -- the host frame of the lock-step drivers (md.hip, md_npt.hip, vib.hip, neb.hip, dimer.hip, relax_cell.hip, relax_bfgsls.hip, relax_cg.hip): evaluate
// the batch, enqueue the driver's kernels behind the evaluation, poll every few evaluations, regrow after a neighbor-capacity
// overflow, stop, leave the batch complete.  A driver brings its kernels (`launch`), a plan, and where it has work at a poll (CG's
// Compactor) a `poll` callable.  The host only enqueues between polls: a driver's kernels test counters[2] and move nothing behind
// an overflowed evaluation, and every chain is held by its own counters, so the window a regrow gives back retraces nothing twice.
// relax_lockstep<FireWork | BfgsWork> (relax.hip) keeps its own loop: a fixed trip count, a counter cleared every iteration, the
// trajectory observer.
#ifndef VSSR_LOCKSTEP_H
#define VSSR_LOCKSTEP_H
#include <climits>
#include "vssr_internal.h"

namespace vssr {

enum LockstepMask {
    LOCKSTEP_MASK_NEVER,        // every evaluation covers every chain
    LOCKSTEP_MASK_AT_STOP,      // d_active reaches the evaluation kernels at the first poll that sees a stop: a run in which nothing
                                // stops early never pays for the masked forms of the kernels (as relax_lockstep)
    LOCKSTEP_MASK_FROM_START
};

struct LockstepPlan {
    int poll;                   // evaluations per poll
    long long max_launch;       // evaluation budget; once it is spent nothing is launched, and the last window is polled as well
    LockstepMask mask;
    // The progress word.  stopped != null: a device record of stop_ints (1 or 2) ints the driver's kernels add to -- [0] groups
    // stopped, [1] of those that need the closing evaluation -- read at every poll; the loop has finished at [0] == groups.
    // stopped == null: the driver's kernels count the chains still running into counters[3], which is cleared and copied back in
    // the poll iterations only (two dispatches less per evaluation in between); the loop has finished at 0.
    const int *stopped = nullptr;
    int stop_ints = 2, groups = 0;
    bool always_close = false;                  // else the closing evaluation runs only where [1] > 0 or the mask was installed
    long long poll_all_from = LLONG_MAX;        // every iteration polls once it + 1 >= this (vibrations: the count the longest chain needs)
    bool finished_at_start = false;             // nothing to drive: only the closing evaluation
};

// poll(false): at a poll after which the loop goes on; poll(true): before the closing evaluation.  Returns VSSR_OK or the error.
// finished: whether the loop ended because every group had stopped (and not because the budget ran out): the caller decides
// what an unfinished loop means.
template <class Launch, class Poll>
int lockstep_run(vssr_handle *h, const LockstepPlan &P, uint32_t want, bool &finished, Launch launch, Poll poll) {
    hipStream_t st = h->stream;
    unsigned char *active = h->d_active.as<unsigned char>();
    int *running_d = h->d_counters.as<int>() + 3;
    struct Unmask { vssr_handle *h; ~Unmask() { h->active_mask = nullptr; } } unmask{h};   // on every exit path
    h->active_mask = P.mask == LOCKSTEP_MASK_FROM_START ? active : nullptr;
    bool masked = false;
    int stopped[2] = {0, 0};
    auto evaluate = [&]() -> int {
        if (int rc = evaluator(h).run(h, want | VSSR_WANT_FORCES)) return rc;
        ++h->relax_lockstep;
        h->relax_chain_evals += h->n_cfg;   // (the resident batch: CG's compaction shrinks it)
        return VSSR_OK;
    };
    finished = P.finished_at_start;
    int rc = VSSR_OK;
    for (long long it = 0; !rc && !P.finished_at_start; ++it) {
        const bool spent = it >= P.max_launch;   // the budget ran out between two polls: look at the last window as well
        const bool poll_it = spent || (it + 1) % P.poll == 0 || it + 1 >= P.poll_all_from;
        if (!spent) {
            if ((rc = evaluate())) break;
            if (!P.stopped && poll_it) VSSR_HIP(h, hipMemsetAsync(running_d, 0, sizeof(int), st));
            launch();
            if (!P.stopped && poll_it) VSSR_HIP(h, hipMemcpyAsync(h->h_counters + 3, running_d, sizeof(int), hipMemcpyDeviceToHost, st));
        }
        if (!poll_it) continue;
        if (P.stopped) VSSR_HIP(h, hipMemcpyAsync(stopped, P.stopped, sizeof(int) * P.stop_ints, hipMemcpyDeviceToHost, st));
        VSSR_HIP(h, hipStreamSynchronize(st));
        // (spent: `it` is one past the window's last launch)
        if (h->h_counters[2]) { rc = relax_regrow(h, 64, it, P.poll + spent); continue; }
        finished = P.stopped ? stopped[0] == P.groups : h->h_counters[3] == 0;
        if (spent || finished) break;
        if (P.mask == LOCKSTEP_MASK_AT_STOP && !masked && stopped[0] > 0) { h->active_mask = active; masked = true; }
        rc = poll(false);
    }
    h->active_mask = nullptr;
    if (rc) return rc;
    // Chains were switched off at different times, or a group went back to where its step opened: one evaluation over all chains
    // leaves the batch complete.  Otherwise the last evaluation of the loop is that evaluation already.
    if (P.always_close || stopped[1] > 0 || masked)
        if ((rc = poll(true)) || (rc = evaluate())) return rc;
    return VSSR_OK;
}

template <class Launch>
int lockstep_run(vssr_handle *h, const LockstepPlan &P, uint32_t want, bool &finished, Launch launch) {
    return lockstep_run(h, P, want, finished, launch, [](bool) { return (int)VSSR_OK; });
}

}  // namespace vssr
#endif
