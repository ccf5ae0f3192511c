// s3dg_inflate.cpp — s3dg_inflate_batch, s3dg_npz_zindex_batch and
// s3dg_npz_zunpack_batch: DEFLATE streams and NPZ archives with stored and
// deflated members decoded on the device.  The rules and the
// decoder are in s3dg_inflate_plan.h, the kernels in s3dg_inflate.hip; here is
// the HIP choreography, which is s3dg_npz_unpack.cpp's: every descriptor is
// checked before anything is reserved or enqueued, the descriptors go up in
// one copy, the results come back in one.
#include "s3dg_ctx.h"

#include <string.h>

#include <vector>

using namespace s3dg;

namespace {

// s3dg_npz_unpack.cpp's: the next of the stream's two tables with hb pinned
// and db device bytes.
int table_reserve(StreamState *S, uint64_t hb, uint64_t db, hipStream_t s, StreamState::CrcTable **out) {
    StreamState::CrcTable &T = S->ttab[S->tnext];
    S->tnext ^= 1;
    if (!T.uploaded) HIP_TRY(hipEventCreateWithFlags(&T.uploaded, hipEventDisableTiming), "hipEventCreate");
    HIP_TRY(hipEventSynchronize(T.uploaded), "hipEventSynchronize(inflate table)");
    if (hb > T.host_cap) {
        if (T.host) (void)hipHostFree(T.host);
        T.host = nullptr;
        T.host_cap = 0;
        const uint64_t cap = hb < (1u << 14) ? (1u << 14) : hb + hb / 4;
        HIP_TRY(hipHostMalloc((void **)&T.host, cap, hipHostMallocDefault), "hipHostMalloc(inflate table)");
        T.host_cap = cap;
    }
    if (db > T.dev_cap) {
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(inflate table)");
        if (T.dev) (void)hipFree(T.dev);
        T.dev = nullptr;
        T.dev_cap = 0;
        const uint64_t cap = db < (1u << 14) ? (1u << 14) : db + db / 4;
        HIP_TRY(hipMalloc((void **)&T.dev, cap), "hipMalloc(inflate table)");
        T.dev_cap = cap;
    }
    *out = &T;
    return S3DG_OK;
}

constexpr s3dg_inflate_result kClean{0, 0, 0, 0, UINT64_MAX};
constexpr s3dg_npz_zunpack_result kCleanTake{0, 0, 0, 0, 0, 0, UINT64_MAX, UINT64_MAX};

}  // namespace

extern "C" int s3dg_inflate_batch(s3dg_ctx *c, const void *src_base, void *dst_base, const s3dg_inflate_item *items, uint64_t n,
                                  void *stream, s3dg_inflate_result *total, s3dg_inflate_result *per_item) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    std::string why;
    if (!inf_check((uint64_t)(uintptr_t)src_base, (uint64_t)(uintptr_t)dst_base, items, n, total != nullptr, &why))
        return fail(S3DG_EINVAL, why);
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    // the work items up, the results behind them on the device side
    const uint64_t hb = n * sizeof(InfWork), res_off = span_align256(hb);
    StreamState::CrcTable *T = nullptr;
    if (int r = table_reserve(SL.get(), hb, res_off + n * sizeof(InfDevRes), s, &T)) return r;
    InfWork *w = reinterpret_cast<InfWork *>(T->host);
    for (uint64_t k = 0; k < n; ++k) w[k] = inf_work((uint64_t)(uintptr_t)src_base, (uint64_t)(uintptr_t)dst_base, items[k]);
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, hb, hipMemcpyHostToDevice, s), "hipMemcpyAsync(inflate items)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    InfDevRes *res_dev = reinterpret_cast<InfDevRes *>(T->dev + res_off);
    HIP_TRY(inflate_launch(reinterpret_cast<const InfWork *>(T->dev), n, res_dev, s), "launch k_inflate");
    std::vector<InfDevRes> got(n);
    HIP_TRY(hipMemcpyAsync(got.data(), res_dev, n * sizeof(InfDevRes), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(inflate results)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(inflate)");
    s3dg_inflate_result tot = kClean;
    for (uint64_t k = 0; k < n; ++k) {
        const InfDevRes &g = got[k];
        const bool bad = g.status != S3DG_INFLATE_OK || g.bad_crc;
        const s3dg_inflate_result r{g.status, g.out_bytes, g.in_bytes, g.bad_crc, bad ? k : UINT64_MAX};
        if (r.status > tot.status) tot.status = r.status;
        tot.out_bytes += r.out_bytes;
        tot.in_bytes += r.in_bytes;
        tot.bad_crc += r.bad_crc;
        if (bad && tot.first_item == UINT64_MAX) tot.first_item = k;
        if (per_item) per_item[k] = r;
    }
    *total = tot;
    return S3DG_OK;
}

extern "C" int s3dg_npz_zindex_batch(s3dg_ctx *c, const void *base, void *table, const s3dg_npz_stream *archives, uint64_t n,
                                     void *stream, s3dg_npz_walk_result *results) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    std::string why;
    if (!nzi_check((uint64_t)(uintptr_t)base, (uint64_t)(uintptr_t)table, archives, n, results != nullptr, &why))
        return fail(S3DG_EINVAL, why);
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    const uint64_t hb = n * sizeof(s3dg_npz_stream), res_off = span_align256(hb);
    StreamState::CrcTable *T = nullptr;
    if (int r = table_reserve(SL.get(), hb, res_off + n * sizeof(s3dg_npz_walk_result), s, &T)) return r;
    memcpy(T->host, archives, hb);
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, hb, hipMemcpyHostToDevice, s), "hipMemcpyAsync(npz archives)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    s3dg_npz_walk_result *res_dev = reinterpret_cast<s3dg_npz_walk_result *>(T->dev + res_off);
    HIP_TRY(npz_zindex_launch((const uint8_t *)base, (uint8_t *)table, reinterpret_cast<const s3dg_npz_stream *>(T->dev), n, res_dev, s),
            "launch k_inz_walk");
    HIP_TRY(hipMemcpyAsync(results, res_dev, n * sizeof(s3dg_npz_walk_result), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(npz walk results)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(npz zindex)");
    return S3DG_OK;
}

extern "C" int s3dg_npz_zunpack_batch(s3dg_ctx *c, const void *base, const void *table, void *dst_base, const s3dg_npz_take *takes,
                                      uint64_t n, void *stream, s3dg_npz_zunpack_result *total, s3dg_npz_zunpack_result *per_take) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    uint64_t ents = 0;
    std::string why;
    if (!inz_check((uint64_t)(uintptr_t)base, (uint64_t)(uintptr_t)table, (uint64_t)(uintptr_t)dst_base, takes, n, total != nullptr,
                   &ents, &why))
        return fail(S3DG_EINVAL, why);
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    // up: the takes with their running entry counts.  Behind them on the device:
    // a verdict per take, a work item and a result per member.
    const uint64_t hb = (n + 1) * sizeof(TfxTake), ver_off = span_align256(hb);
    const uint64_t work_off = span_align256(ver_off + n * sizeof(InzDevTake)), res_off = span_align256(work_off + ents * sizeof(InfWork));
    StreamState::CrcTable *T = nullptr;
    if (int r = table_reserve(SL.get(), hb, res_off + ents * sizeof(InfDevRes), s, &T)) return r;
    TfxTake *tk = reinterpret_cast<TfxTake *>(T->host);
    uint64_t e0 = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_npz_take t = takes[k];
        tk[k] = TfxTake{t.off, t.bytes, t.tab_off, t.first, t.count, t.dst_off, t.dst_cap, e0};
        e0 += t.count;
    }
    tk[n] = TfxTake{0, 0, 0, 0, 0, 0, 0, e0};
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, hb, hipMemcpyHostToDevice, s), "hipMemcpyAsync(npz takes)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    InzDevTake *ver_dev = reinterpret_cast<InzDevTake *>(T->dev + ver_off);
    InfDevRes *res_dev = reinterpret_cast<InfDevRes *>(T->dev + res_off);
    HIP_TRY(npz_zunpack_launch((const uint8_t *)base, (const uint8_t *)table, (uint8_t *)dst_base, reinterpret_cast<const TfxTake *>(T->dev),
                               n, ents, ver_dev, reinterpret_cast<InfWork *>(T->dev + work_off), res_dev, s),
            "launch k_inz_plan");
    std::vector<InzDevTake> ver(n);
    std::vector<InfDevRes> got(ents);
    HIP_TRY(hipMemcpyAsync(ver.data(), ver_dev, n * sizeof(InzDevTake), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(npz verdicts)");
    if (ents)
        HIP_TRY(hipMemcpyAsync(got.data(), res_dev, ents * sizeof(InfDevRes), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(inflate results)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(npz zunpack)");
    s3dg_npz_zunpack_result tot = kCleanTake;
    e0 = 0;
    for (uint64_t k = 0; k < n; ++k) {
        s3dg_npz_zunpack_result r = kCleanTake;
        r.status = ver[k].status;
        r.span = ver[k].span;
        if (r.status == S3DG_NPZ_TAKE_TAKEN) {
            r.members = takes[k].count;
            for (uint64_t i = 0; i < takes[k].count; ++i) {
                const InfDevRes &g = got[e0 + i];
                r.bytes += g.out_bytes;
                r.bad_crc += g.bad_crc;
                r.bad_stream += g.status != S3DG_INFLATE_OK;
                if ((g.bad_crc || g.status != S3DG_INFLATE_OK) && r.first_take == UINT64_MAX) {
                    r.first_take = k;
                    r.first_member = takes[k].first + i;
                }
            }
        }
        e0 += takes[k].count;
        tot.members += r.members;
        tot.bytes += r.bytes;
        tot.span += r.span;
        if (r.status > tot.status) tot.status = r.status;
        tot.bad_crc += r.bad_crc;
        tot.bad_stream += r.bad_stream;
        if (r.first_take != UINT64_MAX && tot.first_take == UINT64_MAX) {
            tot.first_take = k;
            tot.first_member = r.first_member;
        }
        if (per_take) per_take[k] = r;
    }
    *total = tot;
    return S3DG_OK;
}
