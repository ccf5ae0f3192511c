// s3dg_accum.h — the core of an accumulating handle: what s3dg_measure,
// s3dg_chunks and s3dg_lz share behind their C ABI.
// A handle takes adds on any stream, sums into device totals that only take
// atomics, and reads them back on a stream of its own.  Also the driver of the
// host-buffer forms (s3dg_measure_data, s3dg_chunk_data, s3dg_lz_data) over a
// host slot's staging set.  Private to those three units.
#pragma once
#include "s3dg_ctx.h"
#include "s3dg_span_batch_plan.h"

#include <cstring>

namespace s3dg {

// A batch add's uploaded table (s3dg_span_batch_plan.h) on the device: its
// entries and, for a granule pass, its ntiles tiles of 2^tshift granules.
struct SpanTable {
    const SpanEnt *ents;
    const SpanTile *tiles;
    uint64_t ntiles;
    uint32_t tshift;
};

// What one stream of a handle owns: the event of its latest add.  Adds on one
// stream are ordered; adds on two streams share nothing but the handle's
// arrays and totals.  A handle with scratch per stream derives from this.
struct AccumStream {
    hipEvent_t ev = nullptr;
    // a batch add's span table (s3dg_span_batch_plan.h): built in `stage`
    // (pinned), uploaded to `table`; up = the latest upload out of `stage`
    void *stage = nullptr, *table = nullptr;
    uint64_t stage_cap = 0, table_cap = 0;
    hipEvent_t up = nullptr;
};

// Handle entry points: a null handle is an error; one call at a time per
// handle, with its device current for the call.
#define ACCUM_SCOPE(h, null_text)                                     \
    if (!(h)) return fail(S3DG_EINVAL, null_text);                    \
    std::lock_guard<std::mutex> guard_((h)->mu);                      \
    DeviceScope dscope_((h)->device);                                 \
    if (!dscope_.ok()) return hipfail(dscope_.err, "hipSetDevice")

// HIP_TRY with the failure's label composed from the handle's name: "op(name what)".
#define ACCUM_TRY(expr, op, what)                                  \
    do {                                                           \
        hipError_t e_ = (expr);                                    \
        if (e_ != hipSuccess) return hip_failed(e_, op, what);     \
    } while (0)

// *buf holds `need` bytes; its contents are not kept.  It is replaced only
// after `ev` (the latest user of the old one; null: it is idle).
inline int accum_regrow(void **buf, uint64_t *cap, uint64_t need, hipEvent_t ev, const char *wait_what,
                        const char *malloc_what) {
    if (need <= *cap) return S3DG_OK;
    if (ev) HIP_TRY(hipEventSynchronize(ev), wait_what);
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(buf, need), malloc_what);
    *cap = need;
    return S3DG_OK;
}

template <class Stream = AccumStream>
struct Accum {
    const char *name = "";             // in the labels of HIP failures
    s3dg_ctx *ctx = nullptr;
    int device = 0, cus = 256;
    std::mutex mu;                     // one call at a time per handle
    uint64_t *tot = nullptr;           // device: the totals, added to by every add's kernels
    size_t tot_words = 0;
    // node-based: a handle may keep a pointer to a stream's state
    std::map<hipStream_t, Stream> streams;
    hipStream_t gs = nullptr;          // get's, reset's and growth's own stream

    int hip_failed(hipError_t e, const char *op, const char *what) const {
        return hipfail(e, (std::string(op) + "(" + name + what + ")").c_str());
    }

    // The zeroed totals and the handle's stream; the caller has the context's device current.
    int init(s3dg_ctx *c, const char *handle_name, size_t words) {
        name = handle_name;
        ctx = c;
        device = c->device;
        cus = c->cus;
        tot_words = words;
        hipError_t e = hipMalloc((void **)&tot, words * sizeof(uint64_t));
        const char *op = "hipMalloc";
        if (e == hipSuccess) {
            e = hipMemset(tot, 0, words * sizeof(uint64_t));
            op = "hipMemset";
        }
        if (e == hipSuccess) {
            e = hipStreamCreateWithFlags(&gs, hipStreamNonBlocking);
            op = nullptr;
        }
        if (e == hipSuccess) return S3DG_OK;
        if (tot) (void)hipFree(tot);
        tot = nullptr;
        return op ? hip_failed(e, op, " totals") : hipfail(e, "hipStreamCreate");
    }

    int wait_adds() {
        for (auto &kv : streams)
            if (kv.second.ev) ACCUM_TRY(hipEventSynchronize(kv.second.ev), "hipEventSynchronize", " add");
        return S3DG_OK;
    }

    // Stream s's state, its event made on the stream's first add.
    int stream_enter(hipStream_t s, Stream **out) {
        Stream &S = streams[s];
        if (!S.ev) HIP_TRY(hipEventCreateWithFlags(&S.ev, hipEventDisableTiming), "hipEventCreate");
        *out = &S;
        return S3DG_OK;
    }
    // The add enqueued on s is the stream's latest.
    int stream_mark(Stream &S, hipStream_t s) {
        ACCUM_TRY(hipEventRecord(S.ev, s), "hipEventRecord", " add");
        return S3DG_OK;
    }

    // A batch add's table on stream s, after the caller's span_batch_check
    // filled C (C.live > 0): built in S's pinned buffer, uploaded to S's device
    // buffer, *T its parts there.  tiled false: the entries alone.  The pinned
    // buffer must be idle (a later add on the stream reuses it, so the earlier
    // upload is waited for); the copy is enqueued on s behind the stream's
    // earlier adds, which read the old table.
    int batch_table(Stream &S, const s3dg_span *spans, uint64_t n, const SpanBatchCounts &C, uint64_t block_bytes,
                    uint64_t min_bytes, bool tiled, hipStream_t s, SpanTable *T) {
        const uint32_t tshift = tiled ? span_batch_tile_shift(C, ctx->tile_shift) : 0;
        const uint64_t ntiles = tiled ? C.ntiles[tshift] : 0, toff = span_batch_tile_offset(C.live);
        const uint64_t bytes = span_batch_table_bytes(C.live, ntiles);
        if (!S.up) HIP_TRY(hipEventCreateWithFlags(&S.up, hipEventDisableTiming), "hipEventCreate");
        else ACCUM_TRY(hipEventSynchronize(S.up), "hipEventSynchronize", " table upload");
        if (bytes > S.stage_cap) {
            if (S.stage) (void)hipHostFree(S.stage);
            S.stage = nullptr;
            S.stage_cap = 0;
            const uint64_t cap = span_grow_cap(S.stage_cap, bytes);
            ACCUM_TRY(hipHostMalloc(&S.stage, cap, hipHostMallocDefault), "hipHostMalloc", " table");
            S.stage_cap = cap;
        }
        span_batch_build(spans, n, block_bytes, min_bytes, tshift, (SpanEnt *)S.stage,
                         tiled ? (SpanTile *)((uint8_t *)S.stage + toff) : nullptr);
        // the stream's earlier add may still read the old table
        if (int r = accum_regrow(&S.table, &S.table_cap, span_grow_cap(S.table_cap, bytes), S.ev,
                                 "hipEventSynchronize(add)", "hipMalloc(span table)"))
            return r;
        ACCUM_TRY(hipMemcpyAsync(S.table, S.stage, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync", " table");
        ACCUM_TRY(hipEventRecord(S.up, s), "hipEventRecord", " table upload");
        *T = SpanTable{(const SpanEnt *)S.table, tiled ? (const SpanTile *)((const uint8_t *)S.table + toff) : nullptr,
                       ntiles, tshift};
        return S3DG_OK;
    }

    int reset_totals() {
        if (int r = wait_adds()) return r;
        ACCUM_TRY(hipMemsetAsync(tot, 0, tot_words * sizeof(uint64_t), gs), "hipMemsetAsync", " totals");
        ACCUM_TRY(hipStreamSynchronize(gs), "hipStreamSynchronize", "");
        return S3DG_OK;
    }
    // The first n totals once everything enqueued on gs is done.
    int read_totals(uint64_t *host, size_t n) {
        ACCUM_TRY(hipMemcpyAsync(host, tot, n * sizeof(uint64_t), hipMemcpyDeviceToHost, gs), "hipMemcpyAsync",
                  " totals");
        ACCUM_TRY(hipStreamSynchronize(gs), "hipStreamSynchronize", "");
        return S3DG_OK;
    }

    // A handle's array that keeps its contents when it grows.
    struct Kept {
        void **ptr;
        uint64_t elem;                 // bytes per slot
        const char *what;              // the label of its hipMalloc
    };
    // The n <= 2 arrays hold `cap` slots each: the first `used` copied on gs
    // once every add that writes them is done, then the old ones freed.
    int grow_kept(const Kept *a, int n, uint64_t used, uint64_t cap, const char *copy_what) {
        void *fresh[2] = {nullptr, nullptr};
        int r = S3DG_OK;
        for (int k = 0; k < n && r == S3DG_OK; ++k) {
            const hipError_t e = hipMalloc(&fresh[k], cap * a[k].elem);
            if (e != hipSuccess) r = hipfail(e, a[k].what);
        }
        if (r == S3DG_OK) r = wait_adds();
        if (r == S3DG_OK && used) {
            hipError_t e = hipSuccess;
            for (int k = 0; k < n && e == hipSuccess; ++k)
                e = hipMemcpyAsync(fresh[k], *a[k].ptr, used * a[k].elem, hipMemcpyDeviceToDevice, gs);
            if (e == hipSuccess) e = hipStreamSynchronize(gs);
            if (e != hipSuccess) r = hipfail(e, copy_what);
        }
        for (int k = 0; k < n; ++k) {
            void *drop = r == S3DG_OK ? *a[k].ptr : fresh[k];
            if (drop) (void)hipFree(drop);
            if (r == S3DG_OK) *a[k].ptr = fresh[k];
        }
        return r;
    }
};

// s3dg_*_destroy: under the handle's lock with its device current, every
// stream's event waited for and destroyed (then per_stream(S) for what else
// the stream owns), the handle's stream drained and destroyed, arrays() for
// the handle's own buffers, the totals freed; the delete outside the lock.
template <class H, class PerStream, class Arrays>
int accum_destroy(H *h, const char *null_text, PerStream per_stream, Arrays arrays) {
    if (!h) return S3DG_OK;
    {
        ACCUM_SCOPE(h, null_text);
        for (auto &kv : h->streams) {
            if (kv.second.ev) {
                (void)hipEventSynchronize(kv.second.ev);
                (void)hipEventDestroy(kv.second.ev);
            }
            if (kv.second.up) (void)hipEventDestroy(kv.second.up);   // the upload precedes the add just waited for
            if (kv.second.stage) (void)hipHostFree(kv.second.stage);
            if (kv.second.table) (void)hipFree(kv.second.table);
            per_stream(kv.second);
        }
        if (h->gs) {
            (void)hipStreamSynchronize(h->gs);
            (void)hipStreamDestroy(h->gs);
        }
        arrays();
        if (h->tot) (void)hipFree(h->tot);
    }
    delete h;
    return S3DG_OK;
}

// A host-buffer form, after its argument checks: a host slot's staging set and
// context, a handle from create(ctx, &h), then body(h, sg, own) with the
// slot's device current; `own` takes up to two device buffers of the call's
// own.  Afterwards the first n_streams staging streams are drained (no copy
// still reads the caller's buffer) before the handle, the buffers and the
// staging set go.  A failure leaves *out zero and its text the last error.
template <class H, class R, class Create, class Body>
int accum_host_form(R *out, int n_streams, Create create, int (*destroy)(H *), Body body) {
    int slot = 0;
    if (int r = host_next_slot(&slot)) return r;
    HostStaging *sg = nullptr;
    if (int r = host_staging_acquire(slot, &sg)) return r;
    H *h = nullptr;
    void *own[2] = {nullptr, nullptr};
    auto run = [&]() -> int {
        s3dg_ctx *c = nullptr;
        if (int r = s3dg_host_slot_context(slot, &c)) return r;
        if (int r = create(c, &h)) return r;
        DeviceScope ds(c->device);
        if (!ds.ok()) return hipfail(ds.err, "hipSetDevice");
        return body(h, sg, own);
    };
    const int r = run();
    std::string err = r != S3DG_OK ? s3dg_last_error() : "";   // the cleanup below overwrites it
    for (int q = 0; q < n_streams; ++q) (void)hipStreamSynchronize(sg->st[q]);
    if (h) (void)destroy(h);
    for (int q = 0; q < 2; ++q)
        if (own[q]) (void)hipFree(own[q]);
    host_staging_release(sg);
    if (r != S3DG_OK) {
        memset(out, 0, sizeof(*out));
        return fail(r, err);
    }
    return S3DG_OK;
}

// The double-buffered feed of a host buffer in chunks of `per` whole blocks:
// chunk k copied to dev[k & 1] on staging stream k & 1, then
// add_range(dev, blk_lo, blk_hi, stream) of it on the same stream.
template <class AddRange>
int accum_feed_blocks(const uint8_t *buf, uint64_t len, uint64_t block_bytes, uint64_t per, void *const dev[2],
                      HostStaging *sg, AddRange add_range) {
    const uint64_t chunk = per * block_bytes, nb = span_ceil_div(len, block_bytes);
    int k = 0;
    for (uint64_t pb = 0; pb < nb; pb += per, ++k) {
        const int sl = k & 1;
        const uint64_t lo = pb * block_bytes, hi = lo + chunk < len ? lo + chunk : len;
        HIP_TRY(hipMemcpyAsync(dev[sl], buf + lo, hi - lo, hipMemcpyHostToDevice, sg->st[sl]), "hipMemcpyAsync(H2D)");
        if (int r = add_range(dev[sl], pb, pb + per, sg->st[sl])) return r;
    }
    return S3DG_OK;
}

}  // namespace s3dg
