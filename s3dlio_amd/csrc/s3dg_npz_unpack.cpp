// s3dg_npz_unpack.cpp — s3dg_npz_index_batch, s3dg_npz_unpack_batch and its
// timed form: stored ZIP archives indexed from their bytes and their members'
// array bytes copied out by that index, checked in the copy, one device call
// per list.  The rules are pure functions in
// s3dg_npz_unpack_plan.h, the kernels are in s3dg_npz_unpack.hip; here is the
// HIP choreography, which is s3dg_tfrecord_extract.cpp's.
//
// One call: every descriptor is checked before anything is reserved or
// enqueued.  The descriptors go up (the takes with their running entry
// counts); everything an archive or a table says is read on the device, so
// nothing else crosses the bus but the results on the way back.
#include "s3dg_ctx.h"

#include <string.h>

#include <vector>

using namespace s3dg;

namespace {

// s3dg_tfrecord_var.cpp's: the next of the stream's two tables with hb pinned
// and db device bytes.
int table_reserve(StreamState *S, uint64_t hb, uint64_t db, hipStream_t s, StreamState::CrcTable **out) {
    StreamState::CrcTable &T = S->ttab[S->tnext];
    S->tnext ^= 1;
    if (!T.uploaded) HIP_TRY(hipEventCreateWithFlags(&T.uploaded, hipEventDisableTiming), "hipEventCreate");
    HIP_TRY(hipEventSynchronize(T.uploaded), "hipEventSynchronize(npz table)");
    if (hb > T.host_cap) {
        if (T.host) (void)hipHostFree(T.host);
        T.host = nullptr;
        T.host_cap = 0;
        const uint64_t cap = hb < (1u << 14) ? (1u << 14) : hb + hb / 4;
        HIP_TRY(hipHostMalloc((void **)&T.host, cap, hipHostMallocDefault), "hipHostMalloc(npz table)");
        T.host_cap = cap;
    }
    if (db > T.dev_cap) {
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(npz table)");
        if (T.dev) (void)hipFree(T.dev);
        T.dev = nullptr;
        T.dev_cap = 0;
        const uint64_t cap = db < (1u << 14) ? (1u << 14) : db + db / 4;
        HIP_TRY(hipMalloc((void **)&T.dev, cap), "hipMalloc(npz table)");
        T.dev_cap = cap;
    }
    *out = &T;
    return S3DG_OK;
}

const uint32_t *powers() {
    static const struct P {
        uint32_t pw[kTfvPowers];
        P() { tfv_powers(pw); }
    } p;
    return p.pw;
}

constexpr int kMarks = 4;   // start, planned, scanned, copied and folded

struct Marks {
    hipEvent_t ev[kMarks] = {};
    ~Marks() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

constexpr s3dg_npz_unpack_result kClean{0, 0, 0, 0, 0, UINT64_MAX, UINT64_MAX};

int unpack(s3dg_ctx *c, const void *base, const void *table, void *dst_base, const s3dg_npz_take *takes, uint64_t n,
           void *stream, s3dg_npz_unpack_result *total, s3dg_npz_unpack_result *per_take, float *pass_ms) {
    NzuCounts C;
    std::string why;
    if (!nzu_check((uint64_t)(uintptr_t)base, (uint64_t)(uintptr_t)table, (uint64_t)(uintptr_t)dst_base, takes, n,
                   total != nullptr, &C, &why))
        return fail(S3DG_EINVAL, why);
    std::vector<NzuDevRes> got;
    if (C.ents) {
        hipStream_t s = (hipStream_t)stream;
        StreamLock SL(c, s);
        {
            std::lock_guard<std::mutex> g(c->crc_mu);
            HIP_TRY(crc_tables_device(&c->crc_tab), "crc tables");
        }
        Marks M;
        if (pass_ms)
            for (hipEvent_t &e : M.ev) HIP_TRY(hipEventCreate(&e), "hipEventCreate");
        size_t tmp_bytes = 0;
        HIP_TRY(tfrecord_search_scan(nullptr, &tmp_bytes, nullptr, C.ents, s), "hipcub scan size");
        const NzuLayout L = nzu_layout(C, n, tmp_bytes);
        StreamState::CrcTable *T = nullptr;
        if (int r = table_reserve(SL.get(), L.upload, L.bytes, s, &T)) return r;
        nzu_build(takes, n, powers(), T->host);
        HIP_TRY(hipMemcpyAsync(T->dev, T->host, L.upload, hipMemcpyHostToDevice, s), "hipMemcpyAsync(npz takes)");
        HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
        HIP_TRY(hipMemsetAsync(T->dev + L.res, 0, kNzuCounterBytes + n * sizeof(NzuDevRes), s), "hipMemsetAsync(npz unpack results)");
        HIP_TRY(npz_unpack_launch((const uint8_t *)base, (const uint8_t *)table, (uint8_t *)dst_base, T->dev, L, C, n, tmp_bytes,
                                  c->crc_tab, c->cus, pass_ms ? M.ev : nullptr, s),
                "launch k_nzu");
        got.resize(n);
        HIP_TRY(hipMemcpyAsync(got.data(), T->dev + L.res + kNzuCounterBytes, n * sizeof(NzuDevRes), hipMemcpyDeviceToHost, s),
                "hipMemcpyAsync(npz unpack results)");
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(npz unpack)");
        if (pass_ms)
            for (int i = 0; i + 1 < kMarks; ++i) HIP_TRY(hipEventElapsedTime(&pass_ms[i], M.ev[i], M.ev[i + 1]), "hipEventElapsedTime");
    }
    s3dg_npz_unpack_result tot = kClean;
    for (uint64_t k = 0; k < n; ++k) {
        s3dg_npz_unpack_result r = kClean;
        if (takes[k].count) {
            const NzuDevRes &g = got[k];
            r.status = g.status;
            r.span = g.span;
            if (g.status == S3DG_NPZ_TAKE_TAKEN) {
                r.members = takes[k].count;
                r.bytes = g.bytes;
            }
            if (g.bad_crc) {
                r.bad_crc = g.bad_crc;
                r.first_take = k;
                r.first_member = ~(uint64_t)g.first_inv;
                if (tot.first_take == UINT64_MAX) {
                    tot.first_take = k;
                    tot.first_member = r.first_member;
                }
            }
        }
        tot.members += r.members;
        tot.bytes += r.bytes;
        tot.span += r.span;
        if (r.status > tot.status) tot.status = r.status;
        tot.bad_crc += r.bad_crc;
        if (per_take) per_take[k] = r;
    }
    *total = tot;
    return S3DG_OK;
}

}  // namespace

extern "C" int s3dg_npz_index_batch(s3dg_ctx *c, const void *base, void *table, const s3dg_npz_stream *archives, uint64_t n,
                                    void *stream, s3dg_npz_walk_result *results) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    std::string why;
    if (!nzi_check((uint64_t)(uintptr_t)base, (uint64_t)(uintptr_t)table, archives, n, results != nullptr, &why))
        return fail(S3DG_EINVAL, why);
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    // the descriptors up, the results behind them on the device side
    const uint64_t hb = n * sizeof(s3dg_npz_stream), res_off = span_align256(hb);
    StreamState::CrcTable *T = nullptr;
    if (int r = table_reserve(SL.get(), hb, res_off + n * sizeof(s3dg_npz_walk_result), s, &T)) return r;
    memcpy(T->host, archives, hb);
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, hb, hipMemcpyHostToDevice, s), "hipMemcpyAsync(npz archives)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    s3dg_npz_walk_result *res_dev = reinterpret_cast<s3dg_npz_walk_result *>(T->dev + res_off);
    HIP_TRY(npz_index_launch((const uint8_t *)base, (uint8_t *)table, reinterpret_cast<const s3dg_npz_stream *>(T->dev), n, res_dev, s),
            "launch k_nzi_walk");
    HIP_TRY(hipMemcpyAsync(results, res_dev, n * sizeof(s3dg_npz_walk_result), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(npz walk results)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(npz index)");
    return S3DG_OK;
}

extern "C" int s3dg_npz_unpack_batch(s3dg_ctx *c, const void *base, const void *table, void *dst_base, const s3dg_npz_take *takes,
                                     uint64_t n, void *stream, s3dg_npz_unpack_result *total, s3dg_npz_unpack_result *per_take) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    return unpack(c, base, table, dst_base, takes, n, stream, total, per_take, nullptr);
}

extern "C" int s3dg_npz_unpack_timed(s3dg_ctx *c, const void *base, const void *table, void *dst_base, const s3dg_npz_take *takes,
                                     uint64_t n, void *stream, s3dg_npz_unpack_result *total, s3dg_npz_unpack_result *per_take,
                                     float *pass_ms) {
    CTX_SCOPE(c);
    if (!pass_ms) return fail(S3DG_EINVAL, "null pass_ms");
    for (int i = 0; i < 3; ++i) pass_ms[i] = 0.f;
    if (n == 0) return S3DG_OK;
    return unpack(c, base, table, dst_base, takes, n, stream, total, per_take, pass_ms);
}
