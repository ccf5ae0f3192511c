// s3dg_lz.cpp — C ABI of the LZ4 size measurement (include/s3dlio_gpu.h,
// DESIGN.md §5.12): the accumulating handle (s3dg_accum.h) over k_lz
// (s3dg_lz.hip), and the host-buffer form over a host slot's staging set.
// Argument checks and layouts come from s3dg_lz_plan.h.
#include "s3dg_accum.h"
#include "s3dg_lz.h"

// The totals are kLzTotWords sums; a stream owns nothing but its event.
struct s3dg_lz : Accum<> {
    uint64_t block_bytes = 0;
};

namespace {

const char kNullHandle[] = "null lz handle";

int add_plan(s3dg_lz *h, const LzPlan &P, const void *src, uint64_t stride, hipStream_t s) {
    if (P.n_objs == 0) return S3DG_OK;
    AccumStream *S = nullptr;
    if (int r = h->stream_enter(s, &S)) return r;
    HIP_TRY(launch_lz(P, (const uint8_t *)src, stride, h->block_bytes, h->cus, h->tot, s), "launch k_lz");
    return h->stream_mark(*S, s);
}

}  // namespace

extern "C" {

int s3dg_lz_create(s3dg_ctx *c, uint64_t block_bytes, s3dg_lz **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    *out = nullptr;
    if (const char *w = lz_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    CTX_SCOPE(c);
    HIP_TRY(lz_kernel_prepare(), "hipFuncSetAttribute(k_lz)");
    s3dg_lz *h = new s3dg_lz();
    h->block_bytes = block_bytes;
    if (int r = h->init(c, "lz", kLzTotWords)) {
        delete h;
        return r;
    }
    *out = h;
    return S3DG_OK;
}

int s3dg_lz_destroy(s3dg_lz *h) {
    return accum_destroy(h, kNullHandle, [](AccumStream &) {}, [] {});
}

int s3dg_lz_reset(s3dg_lz *h) {
    ACCUM_SCOPE(h, kNullHandle);
    return h->reset_totals();
}

int s3dg_lz_add_stream(s3dg_lz *h, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                       void *stream) {
    ACCUM_SCOPE(h, kNullHandle);
    LzPlan P;
    if (const char *w = lz_plan_stream(&P, (uint64_t)(uintptr_t)src, obj_size, stride, n_objs, h->block_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(h, P, src, stride, (hipStream_t)stream);
}

int s3dg_lz_add_range(s3dg_lz *h, const void *src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                      void *stream) {
    ACCUM_SCOPE(h, kNullHandle);
    LzPlan P;
    if (const char *w = lz_plan_range(&P, (uint64_t)(uintptr_t)src, obj_size, blk_lo, blk_hi, h->block_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(h, P, src, 0, (hipStream_t)stream);
}

int s3dg_lz_add_batch(s3dg_lz *h, const void *src_base, const s3dg_span *spans, uint64_t n, void *stream) {
    ACCUM_SCOPE(h, kNullHandle);
    hipStream_t s = (hipStream_t)stream;
    SpanBatchCounts C;
    std::string why;
    if (!span_batch_check((uint64_t)(uintptr_t)src_base, spans, n, h->block_bytes, 0, &C, &why))
        return fail(S3DG_EINVAL, why);
    if (C.live == 0) return S3DG_OK;
    AccumStream *S = nullptr;
    if (int r = h->stream_enter(s, &S)) return r;
    // the entries alone: k_lz_batch walks blocks, not tiles
    SpanTable T;
    if (int r = h->batch_table(*S, spans, n, C, h->block_bytes, 0, false, s, &T)) return r;
    HIP_TRY(launch_lz_batch((const uint8_t *)src_base, T.ents, C.live, C.blocks, h->block_bytes, h->cus, h->tot, s),
            "launch k_lz_batch");
    return h->stream_mark(*S, s);
}

int s3dg_lz_get(s3dg_lz *h, s3dg_lz_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    memset(out, 0, sizeof(*out));
    ACCUM_SCOPE(h, kNullHandle);
    if (int r = h->wait_adds()) return r;
    uint64_t host[kLzTotWords];
    if (int r = h->read_totals(host, kLzTotWords)) return r;
    out->bytes = host[kLzTotBytes];
    out->blocks = host[kLzTotBlocks];
    out->lz_bytes = host[kLzTotLz];
    out->stored_bytes = host[kLzTotStored];
    out->raw_blocks = host[kLzTotRaw];
    out->matches = host[kLzTotMatches];
    out->match_bytes = host[kLzTotMatchBytes];
    out->literal_bytes = host[kLzTotLiterals];
    return S3DG_OK;
}

int s3dg_lz_data(const uint8_t *buf, uint64_t len, uint64_t block_bytes, s3dg_lz_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    memset(out, 0, sizeof(*out));
    if (const char *w = lz_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    if (len == 0) return S3DG_OK;
    if (!buf) return fail(S3DG_EINVAL, "null buffer");
    return accum_host_form(
        out, 2, [&](s3dg_ctx *c, s3dg_lz **h) { return s3dg_lz_create(c, block_bytes, h); }, s3dg_lz_destroy,
        [&](s3dg_lz *h, HostStaging *sg, void **) -> int {
            // chunks of whole blocks, as many as fit a staging chunk
            if (int r = accum_feed_blocks(buf, len, block_bytes, lz_host_chunk_blocks(block_bytes), sg->buf, sg,
                                          [&](void *dev, uint64_t lo, uint64_t hi, hipStream_t st) {
                                              return s3dg_lz_add_range(h, dev, len, lo, hi, st);
                                          }))
                return r;
            return s3dg_lz_get(h, out);
        });
}

}  // extern "C"
