// s3dg_measure.cpp — C ABI of the measurement pass (include/s3dlio_gpu.h,
// DESIGN.md §5.10): the accumulating handle (s3dg_accum.h) over the kernels of
// s3dg_measure.hip, and the host-buffer form over a host slot's staging set.
// Argument checks and layouts come from s3dg_measure_plan.h.
#include "s3dg_accum.h"
#include "s3dg_measure.h"

// What one stream of a handle owns besides its event: pass 1's records and the
// histogram's per-workgroup slots.
struct MeasureStream : AccumStream {
    void *rec = nullptr;
    uint64_t rec_cap = 0;
    void *part = nullptr;
};

// The totals: [0] zero bytes, [1] get's distinct count, [2, 258) the histogram.
struct s3dg_measure : Accum<MeasureStream> {
    uint64_t block_bytes = 0;
    int flags = 0;
    MeasureFp *fp = nullptr;           // device: the fingerprints of blocks [0, used)
    uint64_t cap = 0, used = 0;
    uint64_t bytes = 0;                // host-side totals (blocks = used)
    void *work = nullptr;              // sort copy + hipCUB scratch
    uint64_t work_cap = 0;
};

namespace {

constexpr size_t kTotWords = 2 + 256;
const char kNullHandle[] = "null measure handle";

// The array holds `need` fingerprints: doubled until it does, the old ones
// copied once every add that writes them is done.
int fp_reserve(s3dg_measure *m, uint64_t need) {
    if (need <= m->cap) return S3DG_OK;
    const uint64_t cap = measure_grow_cap(m->cap, need);
    const s3dg_measure::Kept a[] = {{(void **)&m->fp, sizeof(MeasureFp), "hipMalloc(fingerprints)"}};
    if (int r = m->grow_kept(a, 1, m->used, cap, "hipMemcpy(fingerprints)")) return r;
    m->cap = cap;
    return S3DG_OK;
}

// What a stream add and a batch add share around their launches: room for
// `slots` more fingerprints, stream s's state with the records of `records`
// granules and, for a histogram, its slots; then launch(S, waves, hist)
// enqueues the passes, and the add becomes the stream's latest.
template <class Launch>
int add_on_stream(s3dg_measure *m, uint64_t slots, uint64_t records, uint64_t bytes, hipStream_t s, Launch launch) {
    if (m->used + slots > kMeasureMaxSlots) return fail(S3DG_EINVAL, "more than 2^40 blocks in one handle");
    if (int r = fp_reserve(m, m->used + slots)) return r;
    MeasureStream *Sp = nullptr;
    if (int r = m->stream_enter(s, &Sp)) return r;
    MeasureStream &S = *Sp;
    // the stream's earlier add may still read the old records
    if (int r = accum_regrow(&S.rec, &S.rec_cap, measure_record_bytes(records), S.ev,
                             "hipEventSynchronize(measure add)", "hipMalloc(measure records)"))
        return r;
    const bool hist = m->flags & S3DG_MEASURE_HIST;
    if (hist && !S.part) HIP_TRY(hipMalloc(&S.part, measure_hist_part_bytes(m->cus)), "hipMalloc(histogram slots)");
    // waves per granule: the context's knob; auto = 1 (the fewest cross-wave sums, measured fastest)
    const int waves = m->ctx->waves_per_block ? m->ctx->waves_per_block : 1;
    if (int r = launch(S, waves, hist)) return r;
    if (int r = m->stream_mark(S, s)) return r;
    m->used += slots;
    m->bytes += bytes;
    return S3DG_OK;
}

int add_plan(s3dg_measure *m, const MeasurePlan &P, const void *src, uint64_t stride, hipStream_t s) {
    if (P.n_objs == 0) return S3DG_OK;
    return add_on_stream(m, P.slots, P.records, P.bytes, s, [&](MeasureStream &S, int waves, bool hist) -> int {
        HIP_TRY(launch_measure_granules(P, (const uint8_t *)src, stride, waves, S.rec, s), "launch k_measure");
        HIP_TRY(launch_measure_blocks(P, m->block_bytes, S.rec, m->fp + m->used, &m->tot[0], s),
                "launch k_measure_blocks");
        if (hist)
            HIP_TRY(launch_byte_hist(P, (const uint8_t *)src, stride, m->cus, S.part, &m->tot[2], s),
                    "launch k_byte_hist");
        return S3DG_OK;
    });
}

// One batch add: every span checked, then slots and records
// reserved on the host, then the table's upload and the passes.
int add_batch(s3dg_measure *m, const void *src_base, const s3dg_span *spans, uint64_t n, hipStream_t s) {
    SpanBatchCounts C;
    std::string why;
    if (!span_batch_check((uint64_t)(uintptr_t)src_base, spans, n, m->block_bytes, 0, &C, &why))
        return fail(S3DG_EINVAL, why);
    if (C.live == 0) return S3DG_OK;
    return add_on_stream(m, C.blocks, C.granules, C.bytes, s, [&](MeasureStream &S, int waves, bool hist) -> int {
        SpanTable T;
        if (int r = m->batch_table(S, spans, n, C, m->block_bytes, 0, true, s, &T)) return r;
        HIP_TRY(launch_measure_granules_batch((const uint8_t *)src_base, T.tiles, T.ntiles, T.tshift, C.granules,
                                              (uint32_t)(m->block_bytes / kMeasureGranule), waves, S.rec, s),
                "launch k_measure_batch");
        HIP_TRY(launch_measure_blocks_batch(T.ents, C.live, C.blocks, C.granules, m->block_bytes, S.rec,
                                            m->fp + m->used, &m->tot[0], s),
                "launch k_measure_blocks_batch");
        if (hist)
            HIP_TRY(launch_byte_hist_batch((const uint8_t *)src_base, T.tiles, T.ntiles, T.tshift, m->cus, S.part,
                                           &m->tot[2], s),
                    "launch k_byte_hist_batch");
        return S3DG_OK;
    });
}

void result_clear(s3dg_measure_result *out) { memset(out, 0, sizeof(*out)); }

}  // namespace

extern "C" {

int s3dg_measure_create(s3dg_ctx *c, uint64_t block_bytes, int flags, s3dg_measure **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    *out = nullptr;
    if (const char *w = measure_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    if (flags & ~S3DG_MEASURE_HIST) return fail(S3DG_EINVAL, "unknown measure flags");
    CTX_SCOPE(c);
    s3dg_measure *m = new s3dg_measure();
    m->block_bytes = block_bytes;
    m->flags = flags;
    if (int r = m->init(c, "measure", kTotWords)) {
        delete m;
        return r;
    }
    *out = m;
    return S3DG_OK;
}

int s3dg_measure_destroy(s3dg_measure *m) {
    return accum_destroy(
        m, kNullHandle,
        [](MeasureStream &S) {
            if (S.rec) (void)hipFree(S.rec);
            if (S.part) (void)hipFree(S.part);
        },
        [m] {
            if (m->fp) (void)hipFree(m->fp);
            if (m->work) (void)hipFree(m->work);
        });
}

int s3dg_measure_reset(s3dg_measure *m) {
    ACCUM_SCOPE(m, kNullHandle);
    if (int r = m->reset_totals()) return r;
    m->used = 0;
    m->bytes = 0;
    return S3DG_OK;
}

int s3dg_measure_add_stream(s3dg_measure *m, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                            void *stream) {
    ACCUM_SCOPE(m, kNullHandle);
    MeasurePlan P;
    if (const char *w = measure_plan_stream(&P, (uint64_t)(uintptr_t)src, obj_size, stride, n_objs, m->block_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(m, P, src, stride, (hipStream_t)stream);
}

int s3dg_measure_add_range(s3dg_measure *m, const void *src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                           void *stream) {
    ACCUM_SCOPE(m, kNullHandle);
    MeasurePlan P;
    if (const char *w = measure_plan_range(&P, (uint64_t)(uintptr_t)src, obj_size, blk_lo, blk_hi, m->block_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(m, P, src, 0, (hipStream_t)stream);
}

int s3dg_measure_add_batch(s3dg_measure *m, const void *src_base, const s3dg_span *spans, uint64_t n, void *stream) {
    ACCUM_SCOPE(m, kNullHandle);
    return add_batch(m, src_base, spans, n, (hipStream_t)stream);
}

int s3dg_measure_get(s3dg_measure *m, s3dg_measure_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    ACCUM_SCOPE(m, kNullHandle);
    if (int r = m->wait_adds()) return r;
    if (m->used == 0) return S3DG_OK;
    size_t tmp = 0;
    HIP_TRY(launch_measure_distinct(nullptr, m->used, nullptr, &tmp, nullptr, m->gs), "hipcub sort size");
    if (int r = accum_regrow(&m->work, &m->work_cap, measure_sort_bytes(m->used) + tmp, nullptr, "",
                             "hipMalloc(distinct count)"))
        return r;
    uint64_t host[kTotWords];
    HIP_TRY(hipMemsetAsync(&m->tot[1], 0, sizeof(uint64_t), m->gs), "hipMemsetAsync(distinct count)");
    HIP_TRY(launch_measure_distinct(m->fp, m->used, m->work, &tmp, &m->tot[1], m->gs), "launch distinct count");
    if (int r = m->read_totals(host, kTotWords)) return r;
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
    return accum_host_form(
        out, 2, [&](s3dg_ctx *c, s3dg_measure **m) { return s3dg_measure_create(c, block_bytes, flags, m); },
        s3dg_measure_destroy, [&](s3dg_measure *m, HostStaging *sg, void **own) -> int {
            // chunks of whole blocks: as many as fit a staging chunk, or one block
            const uint64_t per = block_bytes <= kStagingChunk ? kStagingChunk / block_bytes : 1;
            const uint64_t chunk = per * block_bytes;
            void *dev[2] = {sg->buf[0], sg->buf[1]};
            if (chunk > kStagingChunk) {   // two buffers of the call's own
                const uint64_t sz = ((chunk < len ? chunk : len) + 15) / 16 * 16;
                for (int q = 0; q < 2 && (q == 0 || len > chunk); ++q) {
                    HIP_TRY(hipMalloc(&own[q], sz), "hipMalloc(measure chunk)");
                    dev[q] = own[q];
                }
            }
            if (int r = accum_feed_blocks(buf, len, block_bytes, per, dev, sg,
                                          [&](void *d, uint64_t lo, uint64_t hi, hipStream_t st) {
                                              return s3dg_measure_add_range(m, d, len, lo, hi, st);
                                          }))
                return r;
            return s3dg_measure_get(m, out);
        });
}

}  // extern "C"
