// s3dg_crc_batch.cpp — s3dg_crc32_batch and s3dg_crc32_batch_async: the CRC-32
// of every object of a mixed-size batch in one call.  The
// spans are checked by span_batch_check, as the batch adds check theirs; the
// regions, their records and the fold's algebra are pure functions in
// s3dg_crc_batch_plan.h; here is the HIP choreography.
//
// One call: every span is checked before anything is reserved or enqueued.
// The table (one 32-byte entry per non-empty span, one 24-byte record per
// region) is built in one of the stream's two pinned tables and uploaded on the
// caller's stream, where k_crc32_batch_regions and k_crc32_batch_fold follow
// it.  The stream orders the upload, the launches and the next call's upload
// into the same device table, so the asynchronous form returns without
// waiting and without a copy back; the synchronous form is that into scratch
// of the stream's, one copy of 4 n bytes and one wait.  The context's mutex
// for the CRC tables is held for their one-time upload only.
#include "s3dg_ctx.h"

#include <cstring>

using namespace s3dg;

namespace {

// The next of the stream's two tables with room for the call; its pinned side
// is free once its last upload finished.
int table_reserve(StreamState *S, const CrcBatchCounts &C, hipStream_t s, StreamState::CrcTable **out) {
    StreamState::CrcTable &T = S->ctab[S->cnext];
    S->cnext ^= 1;
    if (!T.uploaded) HIP_TRY(hipEventCreateWithFlags(&T.uploaded, hipEventDisableTiming), "hipEventCreate");
    HIP_TRY(hipEventSynchronize(T.uploaded), "hipEventSynchronize(crc table)");
    const uint64_t hb = crc_batch_table_bytes(C), db = crc_batch_device_bytes(C);
    if (hb > T.host_cap) {
        if (T.host) (void)hipHostFree(T.host);
        T.host = nullptr;
        T.host_cap = 0;
        const uint64_t cap = hb < (1u << 16) ? (1u << 16) : hb + hb / 4;
        HIP_TRY(hipHostMalloc((void **)&T.host, cap, hipHostMallocDefault), "hipHostMalloc(crc table)");
        T.host_cap = cap;
    }
    if (db > T.dev_cap) {
        // launches of an earlier call may still read the device side
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(crc table)");
        if (T.dev) (void)hipFree(T.dev);
        T.dev = nullptr;
        T.dev_cap = 0;
        const uint64_t cap = db < (1u << 16) ? (1u << 16) : db + db / 4;
        HIP_TRY(hipMalloc((void **)&T.dev, cap), "hipMalloc(crc table)");
        T.dev_cap = cap;
    }
    *out = &T;
    return S3DG_OK;
}

// The arguments and the spans, then the call's counts; S3DG_EINVAL with the
// refusal's message.  n > 0.
int check_call(const void *src_base, const s3dg_span *spans, uint64_t n, const void *crcs, CrcBatchCounts *C) {
    if (!crcs) return fail(S3DG_EINVAL, "null output");
    SpanBatchCounts B;
    std::string why;
    if (!span_batch_check((uint64_t)(uintptr_t)src_base, spans, n, 0, 0, &B, &why)) return fail(S3DG_EINVAL, why);
    *C = crc_batch_count(spans, n);
    return S3DG_OK;
}

// The whole call on s, C.live > 0: the table, the zeros of the empty spans,
// the two launches.  Returns without waiting.
int enqueue(s3dg_ctx *c, StreamState *S, const uint8_t *src_base, const s3dg_span *spans, uint64_t n,
            const CrcBatchCounts &C, hipStream_t s, uint32_t *crcs_dev) {
    {
        std::lock_guard<std::mutex> g(c->crc_mu);
        HIP_TRY(crc_tables_device(&c->crc_tab), "crc tables");
    }
    StreamState::CrcTable *T = nullptr;
    if (int r = table_reserve(S, C, s, &T)) return r;
    crc_batch_build(spans, n, C, reinterpret_cast<CrcBatchEnt *>(T->host),
                    reinterpret_cast<CrcBatchRec *>(T->host + crc_batch_rec_offset(C.live)));
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, crc_batch_table_bytes(C), hipMemcpyHostToDevice, s),
            "hipMemcpyAsync(crc table)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    if (C.live < n) HIP_TRY(hipMemsetAsync(crcs_dev, 0, n * 4, s), "hipMemsetAsync(crc results)");
    HIP_TRY(crc_batch_launch(src_base, T->dev, C, c->crc_tab, c->cus, crcs_dev, s), "launch k_crc32_batch");
    return S3DG_OK;
}

}  // namespace

extern "C" int s3dg_crc32_batch_async(s3dg_ctx *c, const void *src_base, const s3dg_span *spans, uint64_t n,
                                      void *stream, uint32_t *crcs_dev) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    CrcBatchCounts C;
    if (int r = check_call(src_base, spans, n, crcs_dev, &C)) return r;
    hipStream_t s = (hipStream_t)stream;
    if (C.live == 0) {   // no kernel: the zeros alone, in stream order
        HIP_TRY(hipMemsetAsync(crcs_dev, 0, n * 4, s), "hipMemsetAsync(crc results)");
        return S3DG_OK;
    }
    StreamLock SL(c, s);
    return enqueue(c, SL.get(), (const uint8_t *)src_base, spans, n, C, s, crcs_dev);
}

extern "C" int s3dg_crc32_batch(s3dg_ctx *c, const void *src_base, const s3dg_span *spans, uint64_t n, void *stream,
                                uint32_t *crcs) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    CrcBatchCounts C;
    if (int r = check_call(src_base, spans, n, crcs, &C)) return r;
    if (C.live == 0) {
        memset(crcs, 0, n * 4);
        return S3DG_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    StreamState *S = SL.get();
    if (n > S->crc_out_cap) {   // idle: every earlier synchronous call on this stream has drained it
        if (S->crc_out) (void)hipFree(S->crc_out);
        S->crc_out = nullptr;
        S->crc_out_cap = 0;
        const uint64_t cap = n < 1024 ? 1024 : n;
        HIP_TRY(hipMalloc((void **)&S->crc_out, cap * 4), "hipMalloc(crc results)");
        S->crc_out_cap = cap;
    }
    if (int r = enqueue(c, S, (const uint8_t *)src_base, spans, n, C, s, S->crc_out)) return r;
    HIP_TRY(hipMemcpyAsync(crcs, S->crc_out, n * 4, hipMemcpyDeviceToHost, s), "hipMemcpyAsync(crc results)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(crc batch)");
    return S3DG_OK;
}
