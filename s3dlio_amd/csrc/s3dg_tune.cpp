// s3dg_tune.cpp — the zero-class launch tuner: a context times its own large
// launches of the mid-line zero class and runs the fitted rule or the plain
// launch, whichever wrote faster (ZcTuner, s3dg_ctx.h).
#include "s3dg_ctx.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace s3dg;

namespace {

bool tune_enabled() {
    static const bool on = [] {
        const char *e = getenv("S3DG_ZC_TUNE");
        return !(e && strcmp(e, "0") == 0);
    }();
    return on;
}

// Mean rate (GB/s) of candidate q's last kTuneKeep timed launches (0: none).
double tune_mean(const ZcTuner &T, int q) {
    const int n = std::min(T.samples[q], kTuneKeep);
    if (n == 0) return 0.0;
    double sum = 0.0;
    for (int k = 0; k < n; ++k) sum += T.recent[q][k];
    return sum / n;
}

}  // namespace

namespace s3dg {

// A launch of class zc writing `bytes`: the candidate to run (0 = the fitted
// rule, 1 = plain) and whether to time it (*timed, events in *probe).
int tune_pick(s3dg_ctx *c, int zc, uint64_t bytes, bool *timed, ZcTuner::Pending *probe) {
    *timed = false;
    if (zc != kZcMidHeavy || c->occ_batch >= 0 || c->batch_rt_floor >= 0 || !tune_enabled()) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    ZcTuner &T = c->tune[zc];
    // harvest finished measurements (never waits)
    int probed = 0;   // new samples of the candidate not chosen
    for (size_t k = 0; k < T.pend.size();) {
        ZcTuner::Pending &p = T.pend[k];
        if (hipEventQuery(p.b) != hipSuccess) {
            (void)hipGetLastError();
            ++k;
            continue;
        }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess && ms > 0.f) {
            if (!T.warm) {
                T.warm = true;   // the context's first timed launch: warm-up, not a sample
            } else {
                T.recent[p.cand][T.samples[p.cand] % kTuneKeep] = p.bytes / (ms * 1e6);
                ++T.samples[p.cand];
                if (p.cand != T.best) ++probed;
            }
        }
        (void)hipGetLastError();
        T.spare.push_back(p.a);
        T.spare.push_back(p.b);
        T.pend[k] = T.pend.back();
        T.pend.pop_back();
    }
    if (T.samples[0] >= kTuneFirst && T.samples[1] >= kTuneFirst) {
        const double mean[2] = {tune_mean(T, 0), tune_mean(T, 1)};
        // switch only when the other candidate is clearly faster (hysteresis)
        if (mean[1 - T.best] > mean[T.best] * (1.0 + kTuneMargin)) {
            T.best = 1 - T.best;
            T.interval = kTuneReprobe;
        } else if (probed) {   // a probe confirmed the choice: probe less often
            T.interval = std::min(2 * T.interval, kTuneReprobeMax);
        }
    }
    if (bytes < kTuneMinBytes) return T.best;
    int cand;
    if (T.issued[0] < (uint64_t)kTuneFirst + 1 || T.issued[1] < (uint64_t)kTuneFirst) {
        cand = (int)(T.launches & 1);   // rule, plain, rule, plain (the first launch is the warm-up)
    } else {
        if (T.next_probe == 0) T.next_probe = T.launches + T.interval;
        cand = T.best;
        if (T.launches >= T.next_probe) {
            cand = 1 - T.best;
            T.next_probe = T.launches + T.interval;
        }
    }
    if (T.pend.size() < 16) {
        for (int q = 0; q < 2; ++q) {
            hipEvent_t &e = q ? probe->b : probe->a;
            if (!T.spare.empty()) {
                e = T.spare.back();
                T.spare.pop_back();
            } else if (hipEventCreate(&e) != hipSuccess) {
                (void)hipGetLastError();
                if (q) T.spare.push_back(probe->a);
                return cand;
            }
        }
        probe->bytes = (double)bytes;
        probe->cand = cand;
        *timed = true;
    }
    ++T.launches;
    ++T.issued[cand];
    return cand;
}

// Record the timed launch's events around it (start before, end after).  A
// probe whose launch failed (launched = false at the end mark) records no rate:
// its events go straight back to the spares (its near-zero elapsed
// time would otherwise enter the medians as a huge GB/s sample).
void tune_mark(s3dg_ctx *c, int zc, const ZcTuner::Pending &probe, bool end, hipStream_t s, bool launched) {
    if (end && !launched) {
        std::lock_guard<std::mutex> g(c->mu);
        c->tune[zc].spare.push_back(probe.a);
        c->tune[zc].spare.push_back(probe.b);
        return;
    }
    (void)hipEventRecord(end ? probe.b : probe.a, s);
    if (end) {
        std::lock_guard<std::mutex> g(c->mu);
        c->tune[zc].pend.push_back(probe);
    }
}

}  // namespace s3dg

extern "C" int s3dg_query_zero_tune(s3dg_ctx *c, int zclass, int *best, double *rule_gbs, double *plain_gbs,
                                    uint64_t *timed) {
    if (!c || zclass < 0 || zclass > 2) return fail(S3DG_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    const ZcTuner &T = c->tune[zclass];
    if (best) *best = T.best;
    if (rule_gbs) *rule_gbs = tune_mean(T, 0);
    if (plain_gbs) *plain_gbs = tune_mean(T, 1);
    if (timed) *timed = T.launches;
    return S3DG_OK;
}
