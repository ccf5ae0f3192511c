// s3dg_chunks.cpp — C ABI of the content-defined chunking analysis
// (include/s3dlio_gpu.h): the accumulating handle
// (s3dg_accum.h) over the kernels of s3dg_chunks.hip, and the host-buffer form,
// which stages the whole buffer on a host slot's GPU.  Argument checks, slot
// counts and scratch sizes come from s3dg_chunk_plan.h.
#include "s3dg_accum.h"
#include "s3dg_chunks.h"

// What one stream of a handle owns besides its event: the add's scratch
// (bitmap, records, counts) and the events around its passes when the handle
// times them.
struct ChunkStream : AccumStream {
    void *scratch = nullptr;
    uint64_t cap = 0;
    hipEvent_t tev[4] = {nullptr, nullptr, nullptr, nullptr};
};

// The totals: kChunkTot* words.
struct s3dg_chunks : Accum<ChunkStream> {
    uint64_t min_bytes = 0, avg_bytes = 0, max_bytes = 0;
    uint32_t bits = 0;
    MeasureFp *fp = nullptr;           // device: fingerprint of slot i in [0, used)
    uint32_t *flen = nullptr;          // device: its chunk's length, 0 = the slot holds no chunk
    uint64_t cap = 0, used = 0;
    uint64_t bytes = 0;                // host-side total
    void *work = nullptr;              // sort keys and indices + hipCUB scratch
    uint64_t work_cap = 0;
    bool table = true;                 // pass A reads the gear values from LDS
    bool timing = false;
    ChunkStream *timed = nullptr;      // the stream state of the latest timed add
};

namespace {

const char kNullHandle[] = "null chunks handle";

// The arrays hold `need` slots: doubled until they do, the old ones copied
// once every add that writes them is done.
int slots_reserve(s3dg_chunks *h, uint64_t need) {
    if (need <= h->cap) return S3DG_OK;
    const uint64_t cap = chunk_grow_cap(h->cap, need);
    const s3dg_chunks::Kept a[] = {{(void **)&h->fp, sizeof(MeasureFp), "hipMalloc(chunk fingerprints)"},
                                   {(void **)&h->flen, sizeof(uint32_t), "hipMalloc(chunk lengths)"}};
    if (int r = h->grow_kept(a, 2, h->used, cap, "hipMemcpy(chunk fingerprints)")) return r;
    h->cap = cap;
    return S3DG_OK;
}

// One add of plan P on stream s.  C null: the stream form, objects `stride`
// apart from base on.  Else the batch form of the n checked
// spans counted in *C, offsets from base: its table is uploaded once the slots
// and the scratch are reserved.
int add_plan(s3dg_chunks *h, const ChunkPlan &P, const void *base, uint64_t stride, const s3dg_span *spans, uint64_t n,
             const SpanBatchCounts *C, hipStream_t s) {
    if (P.n_objs == 0) return S3DG_OK;
    if (h->used + P.slots > kChunkMaxSlots) return fail(S3DG_EINVAL, "more than 2^31 - 1 chunk slots in one handle");
    if (int r = slots_reserve(h, h->used + P.slots)) return r;
    ChunkStream *Sp = nullptr;
    if (int r = h->stream_enter(s, &Sp)) return r;
    ChunkStream &S = *Sp;
    // the stream's earlier add may still use the old scratch
    if (int r = accum_regrow(&S.scratch, &S.cap, P.scratch_bytes, S.ev, "hipEventSynchronize(chunks add)",
                             "hipMalloc(chunk scratch)"))
        return r;
    ChunkSrc src{(const uint8_t *)base, stride, nullptr, nullptr, 0, 0};
    if (C) {
        SpanTable T;
        if (int r = h->batch_table(S, spans, n, *C, 0, h->min_bytes, true, s, &T)) return r;
        src = ChunkSrc{src.base, 0, T.ents, T.tiles, T.ntiles, T.tshift};
    }
    const bool timing = h->timing;
    if (timing)
        for (int k = 0; k < 4; ++k)
            if (!S.tev[k]) HIP_TRY(hipEventCreate(&S.tev[k]), "hipEventCreate");
    const char *step = "";
    HIP_TRY(launch_chunk_passes(P, src, 32 - h->bits, h->table, h->min_bytes, h->max_bytes, S.scratch,
                                h->fp + h->used, h->flen + h->used, h->tot, timing ? S.tev : nullptr, &step, s),
            C ? "launch chunk batch passes" : step);
    if (timing) h->timed = &S;
    if (int r = h->stream_mark(S, s)) return r;
    h->used += P.slots;
    h->bytes += P.bytes;
    return S3DG_OK;
}

void result_clear(s3dg_chunk_result *out) { memset(out, 0, sizeof(*out)); }

}  // namespace

extern "C" {

int s3dg_chunks_create(s3dg_ctx *c, uint64_t min_bytes, uint64_t avg_bytes, uint64_t max_bytes, s3dg_chunks **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    *out = nullptr;
    uint32_t bits = 0;
    if (const char *w = chunk_params_check(min_bytes, avg_bytes, max_bytes, &bits)) return fail(S3DG_EINVAL, w);
    CTX_SCOPE(c);
    s3dg_chunks *h = new s3dg_chunks();
    h->min_bytes = min_bytes;
    h->avg_bytes = avg_bytes;
    h->max_bytes = max_bytes;
    h->bits = bits;
    if (int r = h->init(c, "chunks", kChunkTotWords)) {
        delete h;
        return r;
    }
    *out = h;
    return S3DG_OK;
}

int s3dg_chunks_destroy(s3dg_chunks *h) {
    return accum_destroy(
        h, kNullHandle,
        [](ChunkStream &S) {
            for (int k = 0; k < 4; ++k)
                if (S.tev[k]) (void)hipEventDestroy(S.tev[k]);
            if (S.scratch) (void)hipFree(S.scratch);
        },
        [h] {
            if (h->fp) (void)hipFree(h->fp);
            if (h->flen) (void)hipFree(h->flen);
            if (h->work) (void)hipFree(h->work);
        });
}

int s3dg_chunks_reset(s3dg_chunks *h) {
    ACCUM_SCOPE(h, kNullHandle);
    if (int r = h->reset_totals()) return r;
    h->used = 0;
    h->bytes = 0;
    return S3DG_OK;
}

int s3dg_chunks_add_stream(s3dg_chunks *h, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                           void *stream) {
    ACCUM_SCOPE(h, kNullHandle);
    ChunkPlan P;
    if (const char *w = chunk_plan_stream(&P, (uint64_t)(uintptr_t)src, obj_size, stride, n_objs, h->min_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(h, P, src, stride, nullptr, 0, nullptr, (hipStream_t)stream);
}

int s3dg_chunks_add_batch(s3dg_chunks *h, const void *src_base, const s3dg_span *spans, uint64_t n, void *stream) {
    ACCUM_SCOPE(h, kNullHandle);
    SpanBatchCounts C;
    std::string why;
    if (!span_batch_check((uint64_t)(uintptr_t)src_base, spans, n, 0, h->min_bytes, &C, &why))
        return fail(S3DG_EINVAL, why);
    if (C.live == 0) return S3DG_OK;
    ChunkPlan P;
    chunk_plan_batch(&P, C.live, C.granules, C.slots, C.bytes);
    return add_plan(h, P, src_base, 0, spans, n, &C, (hipStream_t)stream);
}

int s3dg_chunks_get(s3dg_chunks *h, s3dg_chunk_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    ACCUM_SCOPE(h, kNullHandle);
    if (int r = h->wait_adds()) return r;
    if (h->used == 0) return S3DG_OK;
    size_t tmp = 0;
    HIP_TRY(launch_chunk_distinct(nullptr, nullptr, h->used, nullptr, &tmp, nullptr, h->gs), "hipcub sort size");
    if (int r = accum_regrow(&h->work, &h->work_cap, chunk_sort_bytes(h->used) + tmp, nullptr, "",
                             "hipMalloc(distinct count)"))
        return r;
    uint64_t host[kChunkTotWords];
    HIP_TRY(hipMemsetAsync(&h->tot[kChunkTotUnique], 0, 2 * sizeof(uint64_t), h->gs), "hipMemsetAsync(distinct count)");
    HIP_TRY(launch_chunk_distinct(h->fp, h->flen, h->used, h->work, &tmp, h->tot, h->gs), "launch distinct count");
    if (int r = h->read_totals(host, kChunkTotWords)) return r;
    out->bytes = h->bytes;
    out->chunks = host[kChunkTotChunks];
    out->unique_chunks = host[kChunkTotUnique];
    out->unique_bytes = host[kChunkTotUniqueBytes];
    out->candidates = host[kChunkTotCandidates];
    out->forced_cuts = host[kChunkTotForced];
    return S3DG_OK;
}

int s3dg_chunks_set_option(s3dg_chunks *h, int option, int value) {
    ACCUM_SCOPE(h, kNullHandle);
    if (option == S3DG_CHUNKS_TIME_PASSES) h->timing = value != 0;
    else if (option == S3DG_CHUNKS_GEAR_TABLE) h->table = value != 0;
    else return fail(S3DG_EINVAL, "unknown chunks option");
    return S3DG_OK;
}

int s3dg_chunks_pass_seconds(s3dg_chunks *h, double *seconds) {
    if (!seconds) return fail(S3DG_EINVAL, "null output");
    seconds[0] = seconds[1] = seconds[2] = 0.0;
    ACCUM_SCOPE(h, kNullHandle);
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
    return accum_host_form(
        out, 1,
        [&](s3dg_ctx *c, s3dg_chunks **h) { return s3dg_chunks_create(c, min_bytes, avg_bytes, max_bytes, h); },
        s3dg_chunks_destroy, [&](s3dg_chunks *h, HostStaging *sg, void **own) -> int {
            // the window hash and the chunks cross every copy's edge, so the whole object is staged
            void *&dev = own[0];
            HIP_TRY(hipMalloc(&dev, (len + 15) / 16 * 16),
                    "hipMalloc(chunk staging: the buffer does not fit the device)");
            for (uint64_t lo = 0; lo < len; lo += kStagingChunk) {
                const uint64_t n = len - lo < kStagingChunk ? len - lo : kStagingChunk;
                HIP_TRY(hipMemcpyAsync((uint8_t *)dev + lo, buf + lo, n, hipMemcpyHostToDevice, sg->st[0]),
                        "hipMemcpyAsync(H2D)");
            }
            if (int r = s3dg_chunks_add_stream(h, dev, len, 0, 1, sg->st[0])) return r;
            return s3dg_chunks_get(h, out);
        });
}

}  // extern "C"
