// s3dg_reduce.cpp — C ABI of the dedup-then-compress measurement
// (include/s3dlio_gpu.h): the accumulating handle
// (s3dg_accum.h) over the measure's fingerprint passes (s3dg_measure.hip) and
// k_reduce (s3dg_reduce.hip), and the host-buffer form over a host slot's
// staging set.  Argument checks and layouts come from s3dg_lz_plan.h and
// s3dg_measure_plan.h, the table's capacity rule from s3dg_reduce_plan.h.
#include "s3dg_accum.h"
#include "s3dg_reduce.h"

// What one stream of a handle owns besides its event: pass 1's records.
struct ReduceStream : AccumStream {
    void *rec = nullptr;
    uint64_t rec_cap = 0;
};

struct s3dg_reduce : Accum<ReduceStream> {
    uint64_t block_bytes = 0;
    MeasureFp *fp = nullptr;           // device: the fingerprints of blocks [0, used)
    uint64_t cap = 0, used = 0;
    uint64_t bytes = 0;                // host-side totals (blocks = used)
    uint64_t *table = nullptr;         // device: the claim table
    uint64_t slots = 0;
    // an add failed after its first launch: the table may hold claims of
    // fingerprints that were never counted, so adds and get refuse until reset
    bool broken = false;

    ReduceState state() const { return ReduceState{fp, table, slots, tot}; }
};

namespace {

const char kNullHandle[] = "null reduce handle";
const char kBroken[] = "an earlier add on this reduce handle failed after its launch; reset the handle";

// The kept array holds `need` fingerprints: doubled until it does, the old
// ones copied once every add that writes them is done.
int fp_reserve(s3dg_reduce *h, uint64_t need) {
    if (need <= h->cap) return S3DG_OK;
    const uint64_t cap = measure_grow_cap(h->cap, need);
    const s3dg_reduce::Kept a[] = {{(void **)&h->fp, sizeof(MeasureFp), "hipMalloc(fingerprints)"}};
    if (int r = h->grow_kept(a, 1, h->used, cap, "hipMemcpy(fingerprints)")) return r;
    h->cap = cap;
    return S3DG_OK;
}

// The table has reduce_table_slots(., blocks) slots: a larger one is zeroed and
// takes the old one's indices (k_reduce_rebuild) on the handle's stream, once
// every add that claims in the old one is done.
int table_reserve(s3dg_reduce *h, uint64_t blocks) {
    const uint64_t slots = reduce_table_slots(h->slots, blocks);
    if (slots == h->slots) return S3DG_OK;
    uint64_t *fresh = nullptr;
    HIP_TRY(hipMalloc((void **)&fresh, slots * kReduceSlotBytes), "hipMalloc(claim table)");
    int r = h->wait_adds();
    if (r == S3DG_OK) {
        hipError_t e = hipMemsetAsync(fresh, 0, slots * kReduceSlotBytes, h->gs);
        if (e == hipSuccess && h->table)
            e = launch_reduce_rebuild(h->table, h->slots, ReduceState{h->fp, fresh, slots, h->tot}, h->gs);
        if (e == hipSuccess) e = hipStreamSynchronize(h->gs);
        if (e != hipSuccess) r = hipfail(e, "launch k_reduce_rebuild");
    }
    if (r != S3DG_OK) {
        (void)hipFree(fresh);
        return r;
    }
    if (h->table) (void)hipFree(h->table);
    h->table = fresh;
    h->slots = slots;
    return S3DG_OK;
}

// What a stream add and a batch add share around their launches: room for
// `blocks` more fingerprints and their claims, stream s's state with the
// records of `records` granules; then launch(S) enqueues the two passes, and
// the add becomes the stream's latest.  A failure from the first launch on
// leaves the handle broken (its kept slots may already be claimed).
template <class Launch>
int add_on_stream(s3dg_reduce *h, uint64_t blocks, uint64_t records, uint64_t bytes, hipStream_t s, Launch launch) {
    if (h->broken) return fail(S3DG_EHIP, kBroken);
    if (h->used + blocks > kReduceMaxBlocks) return fail(S3DG_EINVAL, "more than 2^40 blocks in one handle");
    if (int r = fp_reserve(h, h->used + blocks)) return r;
    if (int r = table_reserve(h, h->used + blocks)) return r;
    ReduceStream *Sp = nullptr;
    if (int r = h->stream_enter(s, &Sp)) return r;
    // the stream's earlier add may still read the old records
    if (int r = accum_regrow(&Sp->rec, &Sp->rec_cap, measure_record_bytes(records), Sp->ev,
                             "hipEventSynchronize(reduce add)", "hipMalloc(reduce records)"))
        return r;
    int r = launch(*Sp);
    if (r == S3DG_OK) r = h->stream_mark(*Sp, s);
    if (r != S3DG_OK) {
        h->broken = true;
        return r;
    }
    h->used += blocks;
    h->bytes += bytes;
    return S3DG_OK;
}

// waves per granule of pass 1: the context's knob, as the measure takes it
int fp_waves(const s3dg_reduce *h) { return h->ctx->waves_per_block ? h->ctx->waves_per_block : 1; }

int add_plan(s3dg_reduce *h, const LzPlan &P, const MeasurePlan &M, const void *src, uint64_t stride, hipStream_t s) {
    if (P.n_objs == 0) return S3DG_OK;
    return add_on_stream(h, M.slots, M.records, M.bytes, s, [&](ReduceStream &S) -> int {
        HIP_TRY(launch_measure_granules(M, (const uint8_t *)src, stride, fp_waves(h), S.rec, s), "launch k_measure");
        HIP_TRY(launch_measure_blocks(M, h->block_bytes, S.rec, h->fp + h->used, &h->tot[kRedTotZero], s),
                "launch k_measure_blocks");
        HIP_TRY(launch_reduce(P, (const uint8_t *)src, stride, h->block_bytes, h->cus, h->state(), h->used, s),
                "launch k_reduce");
        return S3DG_OK;
    });
}

void result_clear(s3dg_reduce_result *out) { memset(out, 0, sizeof(*out)); }

}  // namespace

extern "C" {

int s3dg_reduce_geometry(uint32_t *initial_slots, uint32_t *slot_bytes) {
    if (!initial_slots || !slot_bytes) return fail(S3DG_EINVAL, "null output");
    *initial_slots = (uint32_t)kReduceInitialSlots;
    *slot_bytes = (uint32_t)kReduceSlotBytes;
    return S3DG_OK;
}

int s3dg_reduce_create(s3dg_ctx *c, uint64_t block_bytes, s3dg_reduce **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    *out = nullptr;
    if (const char *w = lz_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    CTX_SCOPE(c);
    HIP_TRY(reduce_kernel_prepare(), "hipFuncSetAttribute(k_reduce)");
    s3dg_reduce *h = new s3dg_reduce();
    h->block_bytes = block_bytes;
    if (int r = h->init(c, "reduce", kReduceTotWords)) {
        delete h;
        return r;
    }
    if (int r = table_reserve(h, 0)) {
        (void)s3dg_reduce_destroy(h);   // leaves the failure's text as it is
        return r;
    }
    *out = h;
    return S3DG_OK;
}

int s3dg_reduce_destroy(s3dg_reduce *h) {
    return accum_destroy(
        h, kNullHandle,
        [](ReduceStream &S) {
            if (S.rec) (void)hipFree(S.rec);
        },
        [h] {
            if (h->fp) (void)hipFree(h->fp);
            if (h->table) (void)hipFree(h->table);
        });
}

int s3dg_reduce_reset(s3dg_reduce *h) {
    ACCUM_SCOPE(h, kNullHandle);
    if (int r = h->wait_adds()) return r;
    HIP_TRY(hipMemsetAsync(h->table, 0, h->slots * kReduceSlotBytes, h->gs), "hipMemsetAsync(claim table)");
    if (int r = h->reset_totals()) return r;
    h->used = 0;
    h->bytes = 0;
    h->broken = false;
    return S3DG_OK;
}

int s3dg_reduce_add_stream(s3dg_reduce *h, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                           void *stream) {
    ACCUM_SCOPE(h, kNullHandle);
    LzPlan P;
    MeasurePlan M;
    const char *w = lz_plan_stream(&P, (uint64_t)(uintptr_t)src, obj_size, stride, n_objs, h->block_bytes);
    if (!w) w = measure_plan_stream(&M, (uint64_t)(uintptr_t)src, obj_size, stride, n_objs, h->block_bytes);
    if (w) return fail(S3DG_EINVAL, w);
    return add_plan(h, P, M, src, stride, (hipStream_t)stream);
}

int s3dg_reduce_add_range(s3dg_reduce *h, const void *src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                          void *stream) {
    ACCUM_SCOPE(h, kNullHandle);
    LzPlan P;
    MeasurePlan M;
    const char *w = lz_plan_range(&P, (uint64_t)(uintptr_t)src, obj_size, blk_lo, blk_hi, h->block_bytes);
    if (!w) w = measure_plan_range(&M, (uint64_t)(uintptr_t)src, obj_size, blk_lo, blk_hi, h->block_bytes);
    if (w) return fail(S3DG_EINVAL, w);
    return add_plan(h, P, M, src, 0, (hipStream_t)stream);
}

int s3dg_reduce_add_batch(s3dg_reduce *h, const void *src_base, const s3dg_span *spans, uint64_t n, void *stream) {
    ACCUM_SCOPE(h, kNullHandle);
    hipStream_t s = (hipStream_t)stream;
    SpanBatchCounts C;
    std::string why;
    if (!span_batch_check((uint64_t)(uintptr_t)src_base, spans, n, h->block_bytes, 0, &C, &why))
        return fail(S3DG_EINVAL, why);
    if (C.live == 0) return S3DG_OK;
    return add_on_stream(h, C.blocks, C.granules, C.bytes, s, [&](ReduceStream &S) -> int {
        // entries and tiles: pass 1 walks granules through the tiles, pass 2 blocks through the entries
        SpanTable T;
        if (int r = h->batch_table(S, spans, n, C, h->block_bytes, 0, true, s, &T)) return r;
        HIP_TRY(launch_measure_granules_batch((const uint8_t *)src_base, T.tiles, T.ntiles, T.tshift, C.granules,
                                              (uint32_t)(h->block_bytes / kMeasureGranule), fp_waves(h), S.rec, s),
                "launch k_measure_batch");
        HIP_TRY(launch_measure_blocks_batch(T.ents, C.live, C.blocks, C.granules, h->block_bytes, S.rec,
                                            h->fp + h->used, &h->tot[kRedTotZero], s),
                "launch k_measure_blocks_batch");
        HIP_TRY(launch_reduce_batch((const uint8_t *)src_base, T.ents, C.live, C.blocks, h->block_bytes, h->cus,
                                    h->state(), h->used, s),
                "launch k_reduce_batch");
        return S3DG_OK;
    });
}

int s3dg_reduce_get(s3dg_reduce *h, s3dg_reduce_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    ACCUM_SCOPE(h, kNullHandle);
    if (h->broken) return fail(S3DG_EHIP, kBroken);
    if (int r = h->wait_adds()) return r;
    uint64_t host[kReduceTotWords];
    if (int r = h->read_totals(host, kReduceTotWords)) return r;
    out->bytes = h->bytes;
    out->blocks = h->used;
    out->unique_blocks = host[kRedTotUniqueBlocks];
    out->unique_bytes = host[kRedTotUniqueBytes];
    out->lz_bytes = host[kRedTotLz];
    out->stored_bytes = host[kRedTotStored];
    out->raw_blocks = host[kRedTotRaw];
    out->matches = host[kRedTotMatches];
    out->match_bytes = host[kRedTotMatchBytes];
    out->literal_bytes = host[kRedTotLiterals];
    return S3DG_OK;
}

int s3dg_reduce_data(const uint8_t *buf, uint64_t len, uint64_t block_bytes, s3dg_reduce_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    if (const char *w = lz_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    if (len == 0) return S3DG_OK;
    if (!buf) return fail(S3DG_EINVAL, "null buffer");
    return accum_host_form(
        out, 2, [&](s3dg_ctx *c, s3dg_reduce **h) { return s3dg_reduce_create(c, block_bytes, h); },
        s3dg_reduce_destroy, [&](s3dg_reduce *h, HostStaging *sg, void **) -> int {
            // chunks of whole blocks, as many as fit a staging chunk
            if (int r = accum_feed_blocks(buf, len, block_bytes, lz_host_chunk_blocks(block_bytes), sg->buf, sg,
                                          [&](void *dev, uint64_t lo, uint64_t hi, hipStream_t st) {
                                              return s3dg_reduce_add_range(h, dev, len, lo, hi, st);
                                          }))
                return r;
            return s3dg_reduce_get(h, out);
        });
}

}  // extern "C"
