// s3dg_measure.cpp — C ABI of the measurement pass (include/s3dlio_gpu.h,
// DESIGN.md §5.10): the accumulating handle over the kernels of
// s3dg_measure.hip, and the host-buffer form over a host slot's staging set.
// Argument checks and layouts come from s3dg_measure_plan.h.
#include "s3dg_ctx.h"
#include "s3dg_measure.h"

#include <cstring>

// What one stream of a handle owns: pass 1's records and the histogram's
// per-workgroup slots (adds on one stream are ordered, adds on two streams
// share nothing but the handle's arrays), and the event of its latest add.
struct MeasureStream {
    hipEvent_t ev = nullptr;
    void *rec = nullptr;
    uint64_t rec_cap = 0;
    void *part = nullptr;
};

struct s3dg_measure {
    s3dg_ctx *ctx = nullptr;
    int device = 0, cus = 256;
    uint64_t block_bytes = 0;
    int flags = 0;
    std::mutex mu;                     // one call at a time per handle
    MeasureFp *fp = nullptr;           // device: the fingerprints of blocks [0, used)
    uint64_t cap = 0, used = 0;
    uint64_t bytes = 0;                // host-side totals (blocks = used)
    // device: [0] zero bytes, [1] get's distinct count, [2, 258) the histogram
    uint64_t *tot = nullptr;
    std::map<hipStream_t, MeasureStream> streams;
    hipStream_t gs = nullptr;          // get's and growth's own stream
    void *work = nullptr;              // sort copy + hipCUB scratch
    uint64_t work_cap = 0;
};

namespace {

constexpr size_t kTotWords = 2 + 256;
constexpr uint64_t kHostChunk = 64ull << 20;   // a host slot's staging chunk

int wait_adds(s3dg_measure *m) {
    for (auto &kv : m->streams)
        if (kv.second.ev) HIP_TRY(hipEventSynchronize(kv.second.ev), "hipEventSynchronize(measure add)");
    return S3DG_OK;
}

// The array holds `need` fingerprints: doubled until it does, the old ones
// copied once every add that writes them is done.
int fp_reserve(s3dg_measure *m, uint64_t need) {
    if (need <= m->cap) return S3DG_OK;
    const uint64_t cap = measure_grow_cap(m->cap, need);
    MeasureFp *nfp = nullptr;
    HIP_TRY(hipMalloc((void **)&nfp, cap * sizeof(MeasureFp)), "hipMalloc(fingerprints)");
    int r = wait_adds(m);
    if (r == S3DG_OK && m->used) {
        hipError_t e = hipMemcpyAsync(nfp, m->fp, m->used * sizeof(MeasureFp), hipMemcpyDeviceToDevice, m->gs);
        if (e == hipSuccess) e = hipStreamSynchronize(m->gs);
        if (e != hipSuccess) r = hipfail(e, "hipMemcpy(fingerprints)");
    }
    if (r != S3DG_OK) {
        (void)hipFree(nfp);
        return r;
    }
    if (m->fp) (void)hipFree(m->fp);
    m->fp = nfp;
    m->cap = cap;
    return S3DG_OK;
}

int add_plan(s3dg_measure *m, const MeasurePlan &P, const void *src, uint64_t stride, hipStream_t s) {
    if (P.n_objs == 0) return S3DG_OK;
    if (m->used + P.slots > kMeasureMaxSlots) return fail(S3DG_EINVAL, "more than 2^40 blocks in one handle");
    if (int r = fp_reserve(m, m->used + P.slots)) return r;
    MeasureStream &S = m->streams[s];
    if (!S.ev) HIP_TRY(hipEventCreateWithFlags(&S.ev, hipEventDisableTiming), "hipEventCreate");
    const uint64_t rb = measure_record_bytes(P.records);
    if (rb > S.rec_cap) {
        // the stream's earlier add may still read the old records
        HIP_TRY(hipEventSynchronize(S.ev), "hipEventSynchronize(measure add)");
        if (S.rec) (void)hipFree(S.rec);
        S.rec = nullptr;
        S.rec_cap = 0;
        HIP_TRY(hipMalloc(&S.rec, rb), "hipMalloc(measure records)");
        S.rec_cap = rb;
    }
    const bool hist = m->flags & S3DG_MEASURE_HIST;
    if (hist && !S.part) HIP_TRY(hipMalloc(&S.part, measure_hist_part_bytes(m->cus)), "hipMalloc(histogram slots)");
    // waves per granule: the context's knob; auto = 1 (the fewest cross-wave sums, measured fastest)
    const int waves = m->ctx->waves_per_block ? m->ctx->waves_per_block : 1;
    HIP_TRY(launch_measure_granules(P, (const uint8_t *)src, stride, waves, S.rec, s), "launch k_measure");
    HIP_TRY(launch_measure_blocks(P, m->block_bytes, S.rec, m->fp + m->used, &m->tot[0], s),
            "launch k_measure_blocks");
    if (hist)
        HIP_TRY(launch_byte_hist(P, (const uint8_t *)src, stride, m->cus, S.part, &m->tot[2], s),
                "launch k_byte_hist");
    HIP_TRY(hipEventRecord(S.ev, s), "hipEventRecord(measure add)");
    m->used += P.slots;
    m->bytes += P.bytes;
    return S3DG_OK;
}

void result_clear(s3dg_measure_result *out) { memset(out, 0, sizeof(*out)); }

}  // namespace

#define MEASURE_SCOPE(m)                                              \
    if (!(m)) return fail(S3DG_EINVAL, "null measure handle");        \
    std::lock_guard<std::mutex> guard_((m)->mu);                      \
    DeviceScope dscope_((m)->device);                                 \
    if (!dscope_.ok()) return hipfail(dscope_.err, "hipSetDevice")

extern "C" {

int s3dg_measure_create(s3dg_ctx *c, uint64_t block_bytes, int flags, s3dg_measure **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    *out = nullptr;
    if (const char *w = measure_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    if (flags & ~S3DG_MEASURE_HIST) return fail(S3DG_EINVAL, "unknown measure flags");
    CTX_SCOPE(c);
    s3dg_measure *m = new s3dg_measure();
    m->ctx = c;
    m->device = c->device;
    m->cus = c->cus;
    m->block_bytes = block_bytes;
    m->flags = flags;
    hipError_t e = hipMalloc((void **)&m->tot, kTotWords * sizeof(uint64_t));
    const char *what = "hipMalloc(measure totals)";
    if (e == hipSuccess) {
        e = hipMemset(m->tot, 0, kTotWords * sizeof(uint64_t));
        what = "hipMemset(measure totals)";
    }
    if (e == hipSuccess) {
        e = hipStreamCreateWithFlags(&m->gs, hipStreamNonBlocking);
        what = "hipStreamCreate";
    }
    if (e != hipSuccess) {
        if (m->tot) (void)hipFree(m->tot);
        delete m;
        return hipfail(e, what);
    }
    *out = m;
    return S3DG_OK;
}

int s3dg_measure_destroy(s3dg_measure *m) {
    if (!m) return S3DG_OK;
    {
        MEASURE_SCOPE(m);
        for (auto &kv : m->streams) {
            MeasureStream &S = kv.second;
            if (S.ev) {
                (void)hipEventSynchronize(S.ev);
                (void)hipEventDestroy(S.ev);
            }
            if (S.rec) (void)hipFree(S.rec);
            if (S.part) (void)hipFree(S.part);
        }
        if (m->gs) {
            (void)hipStreamSynchronize(m->gs);
            (void)hipStreamDestroy(m->gs);
        }
        if (m->fp) (void)hipFree(m->fp);
        if (m->work) (void)hipFree(m->work);
        if (m->tot) (void)hipFree(m->tot);
    }
    delete m;
    return S3DG_OK;
}

int s3dg_measure_reset(s3dg_measure *m) {
    MEASURE_SCOPE(m);
    if (int r = wait_adds(m)) return r;
    HIP_TRY(hipMemsetAsync(m->tot, 0, kTotWords * sizeof(uint64_t), m->gs), "hipMemsetAsync(measure totals)");
    HIP_TRY(hipStreamSynchronize(m->gs), "hipStreamSynchronize(measure)");
    m->used = 0;
    m->bytes = 0;
    return S3DG_OK;
}

int s3dg_measure_add_stream(s3dg_measure *m, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                            void *stream) {
    MEASURE_SCOPE(m);
    MeasurePlan P;
    if (const char *w = measure_plan_stream(&P, (uint64_t)(uintptr_t)src, obj_size, stride, n_objs, m->block_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(m, P, src, stride, (hipStream_t)stream);
}

int s3dg_measure_add_range(s3dg_measure *m, const void *src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                           void *stream) {
    MEASURE_SCOPE(m);
    MeasurePlan P;
    if (const char *w = measure_plan_range(&P, (uint64_t)(uintptr_t)src, obj_size, blk_lo, blk_hi, m->block_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(m, P, src, 0, (hipStream_t)stream);
}

int s3dg_measure_get(s3dg_measure *m, s3dg_measure_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    MEASURE_SCOPE(m);
    if (int r = wait_adds(m)) return r;
    if (m->used == 0) return S3DG_OK;
    size_t tmp = 0;
    HIP_TRY(launch_measure_distinct(nullptr, m->used, nullptr, &tmp, nullptr, m->gs), "hipcub sort size");
    const uint64_t need = measure_sort_bytes(m->used) + tmp;
    if (need > m->work_cap) {
        if (m->work) (void)hipFree(m->work);
        m->work = nullptr;
        m->work_cap = 0;
        HIP_TRY(hipMalloc(&m->work, need), "hipMalloc(distinct count)");
        m->work_cap = need;
    }
    uint64_t host[kTotWords];
    HIP_TRY(hipMemsetAsync(&m->tot[1], 0, sizeof(uint64_t), m->gs), "hipMemsetAsync(distinct count)");
    HIP_TRY(launch_measure_distinct(m->fp, m->used, m->work, &tmp, &m->tot[1], m->gs), "launch distinct count");
    HIP_TRY(hipMemcpyAsync(host, m->tot, sizeof(host), hipMemcpyDeviceToHost, m->gs), "hipMemcpyAsync(measure totals)");
    HIP_TRY(hipStreamSynchronize(m->gs), "hipStreamSynchronize(measure)");
    out->bytes = m->bytes;
    out->zero_bytes = host[0];
    out->blocks = m->used;
    out->unique_blocks = host[1];
    if (m->flags & S3DG_MEASURE_HIST) memcpy(out->hist, host + 2, sizeof(out->hist));
    return S3DG_OK;
}

int s3dg_measure_data(const uint8_t *buf, uint64_t len, uint64_t block_bytes, int flags, s3dg_measure_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    if (const char *w = measure_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    if (flags & ~S3DG_MEASURE_HIST) return fail(S3DG_EINVAL, "unknown measure flags");
    if (len == 0) return S3DG_OK;
    if (!buf) return fail(S3DG_EINVAL, "null buffer");
    int slot = 0;
    if (int r = host_next_slot(&slot)) return r;
    HostStaging *sg = nullptr;
    if (int r = host_staging_acquire(slot, &sg)) return r;
    s3dg_measure *m = nullptr;
    void *own[2] = {nullptr, nullptr};   // blocks larger than a staging chunk: two buffers of the call's own
    auto run = [&]() -> int {
        s3dg_ctx *c = nullptr;
        if (int r = s3dg_host_slot_context(slot, &c)) return r;
        if (int r = s3dg_measure_create(c, block_bytes, flags, &m)) return r;
        DeviceScope ds(c->device);
        if (!ds.ok()) return hipfail(ds.err, "hipSetDevice");
        // chunks of whole blocks: as many as fit a staging chunk, or one block
        const uint64_t per = block_bytes <= kHostChunk ? kHostChunk / block_bytes : 1;
        const uint64_t chunk = per * block_bytes;
        void *dev[2] = {sg->buf[0], sg->buf[1]};
        if (chunk > kHostChunk) {
            const uint64_t sz = ((chunk < len ? chunk : len) + 15) / 16 * 16;
            for (int q = 0; q < 2 && (q == 0 || len > chunk); ++q) {
                HIP_TRY(hipMalloc(&own[q], sz), "hipMalloc(measure chunk)");
                dev[q] = own[q];
            }
        }
        const uint64_t nb = (len + block_bytes - 1) / block_bytes;
        int k = 0;
        for (uint64_t pb = 0; pb < nb; pb += per, ++k) {
            const int sl = k & 1;
            const uint64_t lo = pb * block_bytes, hi = lo + chunk < len ? lo + chunk : len;
            HIP_TRY(hipMemcpyAsync(dev[sl], buf + lo, hi - lo, hipMemcpyHostToDevice, sg->st[sl]),
                    "hipMemcpyAsync(H2D)");
            if (int r = s3dg_measure_add_range(m, dev[sl], len, pb, pb + per, sg->st[sl])) return r;
        }
        return s3dg_measure_get(m, out);
    };
    const int r = run();
    std::string err = r != S3DG_OK ? s3dg_last_error() : "";
    for (int q = 0; q < 2; ++q) (void)hipStreamSynchronize(sg->st[q]);   // no copy still reads buf
    if (m) (void)s3dg_measure_destroy(m);
    for (int q = 0; q < 2; ++q)
        if (own[q]) (void)hipFree(own[q]);
    host_staging_release(sg);
    if (r != S3DG_OK) {
        result_clear(out);
        return fail(r, err);
    }
    return S3DG_OK;
}

}  // extern "C"
