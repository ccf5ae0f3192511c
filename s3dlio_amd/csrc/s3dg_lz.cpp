// s3dg_lz.cpp — C ABI of the LZ4 size measurement (include/s3dlio_gpu.h,
// DESIGN.md §5.12): the accumulating handle over k_lz (s3dg_lz.hip), and the
// host-buffer form over a host slot's staging set.  Argument checks and
// layouts come from s3dg_lz_plan.h.
#include "s3dg_ctx.h"
#include "s3dg_lz.h"

#include <cstring>

struct s3dg_lz {
    s3dg_ctx *ctx = nullptr;
    int device = 0, cus = 256;
    uint64_t block_bytes = 0;
    std::mutex mu;                     // one call at a time per handle
    uint64_t *tot = nullptr;           // device: kLzTotWords sums, added to by every add's waves
    // the event of each stream's latest add (adds on one stream are ordered;
    // adds on two streams share nothing but the totals, which only take atomics)
    std::map<hipStream_t, hipEvent_t> streams;
    hipStream_t gs = nullptr;          // get's and reset's own stream
};

namespace {

int wait_adds(s3dg_lz *h) {
    for (auto &kv : h->streams)
        if (kv.second) HIP_TRY(hipEventSynchronize(kv.second), "hipEventSynchronize(lz add)");
    return S3DG_OK;
}

int add_plan(s3dg_lz *h, const LzPlan &P, const void *src, uint64_t stride, hipStream_t s) {
    if (P.n_objs == 0) return S3DG_OK;
    hipEvent_t &ev = h->streams[s];
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
    HIP_TRY(launch_lz(P, (const uint8_t *)src, stride, h->block_bytes, h->cus, h->tot, s), "launch k_lz");
    HIP_TRY(hipEventRecord(ev, s), "hipEventRecord(lz add)");
    return S3DG_OK;
}

void result_clear(s3dg_lz_result *out) { memset(out, 0, sizeof(*out)); }

}  // namespace

#define LZ_SCOPE(h)                                                   \
    if (!(h)) return fail(S3DG_EINVAL, "null lz handle");             \
    std::lock_guard<std::mutex> guard_((h)->mu);                      \
    DeviceScope dscope_((h)->device);                                 \
    if (!dscope_.ok()) return hipfail(dscope_.err, "hipSetDevice")

extern "C" {

int s3dg_lz_create(s3dg_ctx *c, uint64_t block_bytes, s3dg_lz **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    *out = nullptr;
    if (const char *w = lz_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    CTX_SCOPE(c);
    HIP_TRY(lz_kernel_prepare(), "hipFuncSetAttribute(k_lz)");
    s3dg_lz *h = new s3dg_lz();
    h->ctx = c;
    h->device = c->device;
    h->cus = c->cus;
    h->block_bytes = block_bytes;
    hipError_t e = hipMalloc((void **)&h->tot, kLzTotWords * sizeof(uint64_t));
    const char *what = "hipMalloc(lz totals)";
    if (e == hipSuccess) {
        e = hipMemset(h->tot, 0, kLzTotWords * sizeof(uint64_t));
        what = "hipMemset(lz totals)";
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

int s3dg_lz_destroy(s3dg_lz *h) {
    if (!h) return S3DG_OK;
    {
        LZ_SCOPE(h);
        for (auto &kv : h->streams)
            if (kv.second) {
                (void)hipEventSynchronize(kv.second);
                (void)hipEventDestroy(kv.second);
            }
        if (h->gs) {
            (void)hipStreamSynchronize(h->gs);
            (void)hipStreamDestroy(h->gs);
        }
        if (h->tot) (void)hipFree(h->tot);
    }
    delete h;
    return S3DG_OK;
}

int s3dg_lz_reset(s3dg_lz *h) {
    LZ_SCOPE(h);
    if (int r = wait_adds(h)) return r;
    HIP_TRY(hipMemsetAsync(h->tot, 0, kLzTotWords * sizeof(uint64_t), h->gs), "hipMemsetAsync(lz totals)");
    HIP_TRY(hipStreamSynchronize(h->gs), "hipStreamSynchronize(lz)");
    return S3DG_OK;
}

int s3dg_lz_add_stream(s3dg_lz *h, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                       void *stream) {
    LZ_SCOPE(h);
    LzPlan P;
    if (const char *w = lz_plan_stream(&P, (uint64_t)(uintptr_t)src, obj_size, stride, n_objs, h->block_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(h, P, src, stride, (hipStream_t)stream);
}

int s3dg_lz_add_range(s3dg_lz *h, const void *src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                      void *stream) {
    LZ_SCOPE(h);
    LzPlan P;
    if (const char *w = lz_plan_range(&P, (uint64_t)(uintptr_t)src, obj_size, blk_lo, blk_hi, h->block_bytes))
        return fail(S3DG_EINVAL, w);
    return add_plan(h, P, src, 0, (hipStream_t)stream);
}

int s3dg_lz_get(s3dg_lz *h, s3dg_lz_result *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    result_clear(out);
    LZ_SCOPE(h);
    if (int r = wait_adds(h)) return r;
    uint64_t host[kLzTotWords];
    HIP_TRY(hipMemcpyAsync(host, h->tot, sizeof(host), hipMemcpyDeviceToHost, h->gs), "hipMemcpyAsync(lz totals)");
    HIP_TRY(hipStreamSynchronize(h->gs), "hipStreamSynchronize(lz)");
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
    result_clear(out);
    if (const char *w = lz_block_bytes_check(block_bytes)) return fail(S3DG_EINVAL, w);
    if (len == 0) return S3DG_OK;
    if (!buf) return fail(S3DG_EINVAL, "null buffer");
    int slot = 0;
    if (int r = host_next_slot(&slot)) return r;
    HostStaging *sg = nullptr;
    if (int r = host_staging_acquire(slot, &sg)) return r;
    s3dg_lz *h = nullptr;
    auto run = [&]() -> int {
        s3dg_ctx *c = nullptr;
        if (int r = s3dg_host_slot_context(slot, &c)) return r;
        if (int r = s3dg_lz_create(c, block_bytes, &h)) return r;
        DeviceScope ds(c->device);
        if (!ds.ok()) return hipfail(ds.err, "hipSetDevice");
        // chunks of whole blocks, as many as fit a staging chunk
        const uint64_t per = lz_host_chunk_blocks(block_bytes);
        const uint64_t chunk = per * block_bytes;
        const uint64_t nb = (len + block_bytes - 1) / block_bytes;
        int k = 0;
        for (uint64_t pb = 0; pb < nb; pb += per, ++k) {
            const int sl = k & 1;
            const uint64_t lo = pb * block_bytes, hi = lo + chunk < len ? lo + chunk : len;
            HIP_TRY(hipMemcpyAsync(sg->buf[sl], buf + lo, hi - lo, hipMemcpyHostToDevice, sg->st[sl]),
                    "hipMemcpyAsync(H2D)");
            if (int r = s3dg_lz_add_range(h, sg->buf[sl], len, pb, pb + per, sg->st[sl])) return r;
        }
        return s3dg_lz_get(h, out);
    };
    const int r = run();
    std::string err = r != S3DG_OK ? s3dg_last_error() : "";
    for (int q = 0; q < 2; ++q) (void)hipStreamSynchronize(sg->st[q]);   // no copy still reads buf
    if (h) (void)s3dg_lz_destroy(h);
    host_staging_release(sg);
    if (r != S3DG_OK) {
        result_clear(out);
        return fail(r, err);
    }
    return S3DG_OK;
}

}  // extern "C"
