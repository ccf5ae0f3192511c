// s3dg_chunks.cpp — C ABI of the content-defined chunking analysis
// (include/s3dlio_gpu.h): the accumulating handle over the
// kernels of s3dg_chunks.hip, and the host-buffer form, which stages the whole
// buffer on a host slot's GPU.  Argument checks, slot counts and scratch sizes
// come from s3dg_chunk_plan.h.
#include "s3dg_chunks.h"
#include "s3dg_ctx.h"

#include <cstring>

// What one stream of a handle owns: the add's scratch (bitmap, records,
// counts; adds on one stream are ordered, adds on two streams share nothing
// but the handle's arrays and totals), the event of its latest add, and the
// events around its passes when the handle times them.
struct ChunkStream {
    hipEvent_t ev = nullptr;
    void *scratch = nullptr;
    uint64_t cap = 0;
    hipEvent_t tev[4] = {nullptr, nullptr, nullptr, nullptr};
};

struct s3dg_chunks {
    s3dg_ctx *ctx = nullptr;
    int device = 0;
    uint64_t min_bytes = 0, avg_bytes = 0, max_bytes = 0;
    uint32_t bits = 0;
    std::mutex mu;                     // one call at a time per handle
    MeasureFp *fp = nullptr;           // device: fingerprint of slot i in [0, used)
    uint32_t *flen = nullptr;          // device: its chunk's length, 0 = the slot holds no chunk
    uint64_t cap = 0, used = 0;
    uint64_t bytes = 0;                // host-side total
    uint64_t *tot = nullptr;           // device: kChunkTot* words
    std::map<hipStream_t, ChunkStream> streams;
    hipStream_t gs = nullptr;          // get's and growth's own stream
    void *work = nullptr;              // sort keys and indices + hipCUB scratch
    uint64_t work_cap = 0;
    bool table = true;                 // pass A reads the gear values from LDS
    bool timing = false;
    ChunkStream *timed = nullptr;      // the stream state of the latest timed add
};

namespace {

constexpr uint64_t kHostCopy = 64ull << 20;   // s3dg_chunk_data's copies

int wait_adds(s3dg_chunks *h) {
    for (auto &kv : h->streams)
        if (kv.second.ev) HIP_TRY(hipEventSynchronize(kv.second.ev), "hipEventSynchronize(chunks add)");
    return S3DG_OK;
}

// The arrays hold `need` slots: doubled until they do, the old ones copied
// once every add that writes them is done.
int slots_reserve(s3dg_chunks *h, uint64_t need) {
    if (need <= h->cap) return S3DG_OK;
    const uint64_t cap = chunk_grow_cap(h->cap, need);
    MeasureFp *nfp = nullptr;
    uint32_t *nlen = nullptr;
    HIP_TRY(hipMalloc((void **)&nfp, cap * sizeof(MeasureFp)), "hipMalloc(chunk fingerprints)");
    hipError_t e = hipMalloc((void **)&nlen, cap * sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipFree(nfp);
        return hipfail(e, "hipMalloc(chunk lengths)");
    }
    int r = wait_adds(h);
    if (r == S3DG_OK && h->used) {
        e = hipMemcpyAsync(nfp, h->fp, h->used * sizeof(MeasureFp), hipMemcpyDeviceToDevice, h->gs);
        if (e == hipSuccess)
            e = hipMemcpyAsync(nlen, h->flen, h->used * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->gs);
        if (e == hipSuccess) e = hipStreamSynchronize(h->gs);
        if (e != hipSuccess) r = hipfail(e, "hipMemcpy(chunk fingerprints)");
    }
    if (r != S3DG_OK) {
        (void)hipFree(nfp);
        (void)hipFree(nlen);
        return r;
    }
    if (h->fp) (void)hipFree(h->fp);
    if (h->flen) (void)hipFree(h->flen);
    h->fp = nfp;
    h->flen = nlen;
    h->cap = cap;
    return S3DG_OK;
}

int add_plan(s3dg_chunks *h, const ChunkPlan &P, const void *src, uint64_t stride, hipStream_t s) {
    if (P.n_objs == 0) return S3DG_OK;
    if (h->used + P.slots > kChunkMaxSlots) return fail(S3DG_EINVAL, "more than 2^31 - 1 chunk slots in one handle");
    if (int r = slots_reserve(h, h->used + P.slots)) return r;
    ChunkStream &S = h->streams[s];
    if (!S.ev) HIP_TRY(hipEventCreateWithFlags(&S.ev, hipEventDisableTiming), "hipEventCreate");
    if (P.scratch_bytes > S.cap) {
        // the stream's earlier add may still use the old scratch
        HIP_TRY(hipEventSynchronize(S.ev), "hipEventSynchronize(chunks add)");
        if (S.scratch) (void)hipFree(S.scratch);
        S.scratch = nullptr;
        S.cap = 0;
        HIP_TRY(hipMalloc(&S.scratch, P.scratch_bytes), "hipMalloc(chunk scratch)");
        S.cap = P.scratch_bytes;
    }
    const bool timing = h->timing;
    if (timing)
        for (int k = 0; k < 4; ++k)
            if (!S.tev[k]) HIP_TRY(hipEventCreate(&S.tev[k]), "hipEventCreate");
    if (timing) HIP_TRY(hipEventRecord(S.tev[0], s), "hipEventRecord(chunks pass)");
    HIP_TRY(launch_chunk_candidates(P, (const uint8_t *)src, stride, 32 - h->bits, h->table, S.scratch, h->tot, s),
            "launch k_chunk_candidates");
    if (timing) HIP_TRY(hipEventRecord(S.tev[1], s), "hipEventRecord(chunks pass)");
    HIP_TRY(launch_chunk_cuts(P, h->min_bytes, h->max_bytes, S.scratch, h->tot, s), "launch k_chunk_cuts");
    if (timing) HIP_TRY(hipEventRecord(S.tev[2], s), "hipEventRecord(chunks pass)");
    HIP_TRY(launch_chunk_fingerprints(P, (const uint8_t *)src, stride, S.scratch, h->fp + h->used, h->flen + h->used,
                                      s),
            "launch k_chunk_fp");
    if (timing) {
        HIP_TRY(hipEventRecord(S.tev[3], s), "hipEventRecord(chunks pass)");
        h->timed = &S;
    }
    HIP_TRY(hipEventRecord(S.ev, s), "hipEventRecord(chunks add)");
    h->used += P.slots;
    h->bytes += P.bytes;
    return S3DG_OK;
}

void result_clear(s3dg_chunk_result *out) { memset(out, 0, sizeof(*out)); }

}  // namespace

#define CHUNKS_SCOPE(h)                                               \
    if (!(h)) return fail(S3DG_EINVAL, "null chunks handle");         \
    std::lock_guard<std::mutex> guard_((h)->mu);                      \
    DeviceScope dscope_((h)->device);                                 \
    if (!dscope_.ok()) return hipfail(dscope_.err, "hipSetDevice")

extern "C" {

int s3dg_chunks_create(s3dg_ctx *c, uint64_t min_bytes, uint64_t avg_bytes, uint64_t max_bytes, s3dg_chunks **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    *out = nullptr;
    uint32_t bits = 0;
    if (const char *w = chunk_params_check(min_bytes, avg_bytes, max_bytes, &bits)) return fail(S3DG_EINVAL, w);
    CTX_SCOPE(c);
    s3dg_chunks *h = new s3dg_chunks();
    h->ctx = c;
    h->device = c->device;
    h->min_bytes = min_bytes;
    h->avg_bytes = avg_bytes;
    h->max_bytes = max_bytes;
    h->bits = bits;
    hipError_t e = hipMalloc((void **)&h->tot, kChunkTotWords * sizeof(uint64_t));
    const char *what = "hipMalloc(chunk totals)";
    if (e == hipSuccess) {
        e = hipMemset(h->tot, 0, kChunkTotWords * sizeof(uint64_t));
        what = "hipMemset(chunk totals)";
    }
    if (e == hipSuccess) {
        e = hipStreamCreateWithFlags(&h->gs, hipStreamNonBlocking);
        what = "hipStreamCreate";
    }
    if (e != hipSuccess) {
        if (h->tot) (void)hipFree(h->tot);
        delete h;
        return hipfail(e, what);
    }
    *out = h;
    return S3DG_OK;
}

int s3dg_chunks_destroy(s3dg_chunks *h) {
    if (!h) return S3DG_OK;
    {
        CHUNKS_SCOPE(h);
        for (auto &kv : h->streams) {
            ChunkStream &S = kv.second;
            if (S.ev) {
                (void)hipEventSynchronize(S.ev);
                (void)hipEventDestroy(S.ev);
            }
            for (int k = 0; k < 4; ++k)
                if (S.tev[k]) (void)hipEventDestroy(S.tev[k]);
            if (S.scratch) (void)hipFree(S.scratch);
        }
        if (h->gs) {
            (void)hipStreamSynchronize(h->gs);
            (void)hipStreamDestroy(h->gs);
        }
        if (h->fp) (void)hipFree(h->fp);
        if (h->flen) (void)hipFree(h->flen);
        if (h->work) (void)hipFree(h->work);
        if (h->tot) (void)hipFree(h->tot);
    }
    delete h;
    return S3DG_OK;
}

int s3dg_chunks_reset(s3dg_chunks *h) {
    CHUNKS_SCOPE(h);
    if (int r = wait_adds(h)) return r;
    HIP_TRY(hipMemsetAsync(h->tot, 0, kChunkTotWords * sizeof(uint64_t), h->gs), "hipMemsetAsync(chunk totals)");
    HIP_TRY(hipStreamSynchronize(h->gs), "hipStreamSynchronize(chunks)");
    h->used = 0;
    h->bytes = 0;
    return S3DG_OK;
}

int s3dg_chunks_add_stream(s3dg_chunks *h, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                           void *stream) {
    CHUNKS_SCOPE(h);
    ChunkPlan P;
    if (const char *w = chunk_plan_stream(&P, (uint64_t)(uintptr_t)src, obj_size, stride, n_objs, h->min_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(h, P, src, stride, (hipStream_t)stream);
}

int s3dg_chunks_get(s3dg_chunks *h, s3dg_chunk_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    CHUNKS_SCOPE(h);
    if (int r = wait_adds(h)) return r;
    if (h->used == 0) return S3DG_OK;
    size_t tmp = 0;
    HIP_TRY(launch_chunk_distinct(nullptr, nullptr, h->used, nullptr, &tmp, nullptr, h->gs), "hipcub sort size");
    const uint64_t need = chunk_sort_bytes(h->used) + tmp;
    if (need > h->work_cap) {
        if (h->work) (void)hipFree(h->work);
        h->work = nullptr;
        h->work_cap = 0;
        HIP_TRY(hipMalloc(&h->work, need), "hipMalloc(distinct count)");
        h->work_cap = need;
    }
    uint64_t host[kChunkTotWords];
    HIP_TRY(hipMemsetAsync(&h->tot[kChunkTotUnique], 0, 2 * sizeof(uint64_t), h->gs), "hipMemsetAsync(distinct count)");
    HIP_TRY(launch_chunk_distinct(h->fp, h->flen, h->used, h->work, &tmp, h->tot, h->gs), "launch distinct count");
    HIP_TRY(hipMemcpyAsync(host, h->tot, sizeof(host), hipMemcpyDeviceToHost, h->gs), "hipMemcpyAsync(chunk totals)");
    HIP_TRY(hipStreamSynchronize(h->gs), "hipStreamSynchronize(chunks)");
    out->bytes = h->bytes;
    out->chunks = host[kChunkTotChunks];
    out->unique_chunks = host[kChunkTotUnique];
    out->unique_bytes = host[kChunkTotUniqueBytes];
    out->candidates = host[kChunkTotCandidates];
    out->forced_cuts = host[kChunkTotForced];
    return S3DG_OK;
}

int s3dg_chunks_set_option(s3dg_chunks *h, int option, int value) {
    CHUNKS_SCOPE(h);
    if (option == S3DG_CHUNKS_TIME_PASSES) h->timing = value != 0;
    else if (option == S3DG_CHUNKS_GEAR_TABLE) h->table = value != 0;
    else return fail(S3DG_EINVAL, "unknown chunks option");
    return S3DG_OK;
}

int s3dg_chunks_pass_seconds(s3dg_chunks *h, double *seconds) {
    if (!seconds) return fail(S3DG_EINVAL, "null output");
    seconds[0] = seconds[1] = seconds[2] = 0.0;
    CHUNKS_SCOPE(h);
    if (!h->timed) return fail(S3DG_EINVAL, "no timed add: set S3DG_CHUNKS_TIME_PASSES before the add");
    ChunkStream &S = *h->timed;
    HIP_TRY(hipEventSynchronize(S.tev[3]), "hipEventSynchronize(chunks pass)");
    for (int k = 0; k < 3; ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, S.tev[k], S.tev[k + 1]), "hipEventElapsedTime(chunks pass)");
        seconds[k] = ms * 1e-3;
    }
    return S3DG_OK;
}

int s3dg_chunk_data(const uint8_t *buf, uint64_t len, uint64_t min_bytes, uint64_t avg_bytes, uint64_t max_bytes,
                    s3dg_chunk_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    if (const char *w = chunk_params_check(min_bytes, avg_bytes, max_bytes, nullptr)) return fail(S3DG_EINVAL, w);
    if (len == 0) return S3DG_OK;
    if (!buf) return fail(S3DG_EINVAL, "null buffer");
    int slot = 0;
    if (int r = host_next_slot(&slot)) return r;
    HostStaging *sg = nullptr;
    if (int r = host_staging_acquire(slot, &sg)) return r;
    s3dg_chunks *h = nullptr;
    void *dev = nullptr;
    auto run = [&]() -> int {
        s3dg_ctx *c = nullptr;
        if (int r = s3dg_host_slot_context(slot, &c)) return r;
        if (int r = s3dg_chunks_create(c, min_bytes, avg_bytes, max_bytes, &h)) return r;
        DeviceScope ds(c->device);
        if (!ds.ok()) return hipfail(ds.err, "hipSetDevice");
        // the window hash and the chunks cross every copy's edge, so the whole object is staged
        HIP_TRY(hipMalloc(&dev, (len + 15) / 16 * 16), "hipMalloc(chunk staging: the buffer does not fit the device)");
        for (uint64_t lo = 0; lo < len; lo += kHostCopy) {
            const uint64_t n = len - lo < kHostCopy ? len - lo : kHostCopy;
            HIP_TRY(hipMemcpyAsync((uint8_t *)dev + lo, buf + lo, n, hipMemcpyHostToDevice, sg->st[0]),
                    "hipMemcpyAsync(H2D)");
        }
        if (int r = s3dg_chunks_add_stream(h, dev, len, 0, 1, sg->st[0])) return r;
        return s3dg_chunks_get(h, out);
    };
    const int r = run();
    std::string err = r != S3DG_OK ? s3dg_last_error() : "";
    (void)hipStreamSynchronize(sg->st[0]);   // no copy still reads buf
    if (h) (void)s3dg_chunks_destroy(h);
    if (dev) (void)hipFree(dev);
    host_staging_release(sg);
    if (r != S3DG_OK) {
        result_clear(out);
        return fail(r, err);
    }
    return S3DG_OK;
}

}  // extern "C"
