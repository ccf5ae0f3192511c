// s3dg_tfrecord_extract.cpp — s3dg_tfrecord_extract_batch and its timed form:
// the payloads of indexed records copied out of framed streams and checked in
// the copy, one device call per list of takes.  The rules
// are pure functions in s3dg_tfrecord_extract_plan.h, the kernels are in
// s3dg_tfrecord_extract.hip; here is the HIP choreography, which is
// s3dg_tfrecord_var.cpp's check form over one of the stream's two tables.
//
// One call: every take is checked before anything is reserved or enqueued.
// The takes go up with their running entry counts; the per-record plan is
// built on the device from the index, so nothing else crosses the bus but the
// results on the way back.
#include "s3dg_ctx.h"

#include <vector>

using namespace s3dg;

namespace {

// s3dg_tfrecord_var.cpp's: the next of the stream's two tables with hb pinned
// and db device bytes.
int table_reserve(StreamState *S, uint64_t hb, uint64_t db, hipStream_t s, StreamState::CrcTable **out) {
    StreamState::CrcTable &T = S->ttab[S->tnext];
    S->tnext ^= 1;
    if (!T.uploaded) HIP_TRY(hipEventCreateWithFlags(&T.uploaded, hipEventDisableTiming), "hipEventCreate");
    HIP_TRY(hipEventSynchronize(T.uploaded), "hipEventSynchronize(tfrecord table)");
    if (hb > T.host_cap) {
        if (T.host) (void)hipHostFree(T.host);
        T.host = nullptr;
        T.host_cap = 0;
        const uint64_t cap = hb < (1u << 14) ? (1u << 14) : hb + hb / 4;
        HIP_TRY(hipHostMalloc((void **)&T.host, cap, hipHostMallocDefault), "hipHostMalloc(tfrecord table)");
        T.host_cap = cap;
    }
    if (db > T.dev_cap) {
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(tfrecord table)");
        if (T.dev) (void)hipFree(T.dev);
        T.dev = nullptr;
        T.dev_cap = 0;
        const uint64_t cap = db < (1u << 14) ? (1u << 14) : db + db / 4;
        HIP_TRY(hipMalloc((void **)&T.dev, cap), "hipMalloc(tfrecord table)");
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

int extract(s3dg_ctx *c, const void *base, const void *idx_base, void *dst_base, const s3dg_tfrecord_take *takes, uint64_t n,
            void *stream, s3dg_tfrecord_extract_result *total, s3dg_tfrecord_extract_result *per_take, float *pass_ms) {
    TfxCounts C;
    std::string why;
    if (!tfx_check((uint64_t)(uintptr_t)base, (uint64_t)(uintptr_t)idx_base, (uint64_t)(uintptr_t)dst_base, takes, n,
                   total != nullptr, &C, &why))
        return fail(S3DG_EINVAL, why);
    std::vector<TfxDevRes> got;
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
        const TfxLayout L = tfx_layout(C, n, tmp_bytes);
        StreamState::CrcTable *T = nullptr;
        if (int r = table_reserve(SL.get(), L.upload, L.bytes, s, &T)) return r;
        tfx_build(takes, n, powers(), T->host);
        HIP_TRY(hipMemcpyAsync(T->dev, T->host, L.upload, hipMemcpyHostToDevice, s), "hipMemcpyAsync(tfrecord takes)");
        HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
        HIP_TRY(hipMemsetAsync(T->dev + L.res, 0, kTfxCounterBytes + n * sizeof(TfxDevRes), s), "hipMemsetAsync(tfrecord results)");
        HIP_TRY(tfrecord_extract_launch((const uint8_t *)base, (const uint8_t *)idx_base, (uint8_t *)dst_base, T->dev, L, C, n,
                                        tmp_bytes, c->crc_tab, c->cus, pass_ms ? M.ev : nullptr, s),
                "launch k_tfx");
        got.resize(n);
        HIP_TRY(hipMemcpyAsync(got.data(), T->dev + L.res + kTfxCounterBytes, n * sizeof(TfxDevRes), hipMemcpyDeviceToHost, s),
                "hipMemcpyAsync(tfrecord results)");
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(tfrecord extract)");
        if (pass_ms)
            for (int i = 0; i + 1 < kMarks; ++i) HIP_TRY(hipEventElapsedTime(&pass_ms[i], M.ev[i], M.ev[i + 1]), "hipEventElapsedTime");
    }
    s3dg_tfrecord_extract_result tot{0, 0, 0, 0, 0, 0, 0, UINT64_MAX, UINT64_MAX};
    for (uint64_t k = 0; k < n; ++k) {
        s3dg_tfrecord_extract_result r{0, 0, 0, 0, 0, 0, 0, UINT64_MAX, UINT64_MAX};
        if (takes[k].count) {
            const TfxDevRes &g = got[k];
            r.status = g.status;
            if (g.status == 0) {
                r.records = takes[k].count;
                r.bytes = g.payload;
            }
            if (g.bad_records) {
                r.bad_records = g.bad_records;
                r.bad_length = g.bad_length;
                r.bad_length_crc = g.bad_length_crc;
                r.bad_data_crc = g.bad_data_crc;
                r.first_take = k;
                r.first_record = ~(uint64_t)g.first_inv;
                if (tot.first_take == UINT64_MAX) {
                    tot.first_take = k;
                    tot.first_record = r.first_record;
                }
            }
        }
        tot.records += r.records;
        tot.bytes += r.bytes;
        if (r.status > tot.status) tot.status = r.status;
        tot.bad_records += r.bad_records;
        tot.bad_length += r.bad_length;
        tot.bad_length_crc += r.bad_length_crc;
        tot.bad_data_crc += r.bad_data_crc;
        if (per_take) per_take[k] = r;
    }
    *total = tot;
    return S3DG_OK;
}

}  // namespace

extern "C" int s3dg_tfrecord_extract_batch(s3dg_ctx *c, const void *base, const void *idx_base, void *dst_base,
                                           const s3dg_tfrecord_take *takes, uint64_t n, void *stream,
                                           s3dg_tfrecord_extract_result *total, s3dg_tfrecord_extract_result *per_take) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    return extract(c, base, idx_base, dst_base, takes, n, stream, total, per_take, nullptr);
}

extern "C" int s3dg_tfrecord_extract_timed(s3dg_ctx *c, const void *base, const void *idx_base, void *dst_base,
                                           const s3dg_tfrecord_take *takes, uint64_t n, void *stream,
                                           s3dg_tfrecord_extract_result *total, s3dg_tfrecord_extract_result *per_take,
                                           float *pass_ms) {
    CTX_SCOPE(c);
    if (!pass_ms) return fail(S3DG_EINVAL, "null pass_ms");
    for (int i = 0; i < 3; ++i) pass_ms[i] = 0.f;
    if (n == 0) return S3DG_OK;
    return extract(c, base, idx_base, dst_base, takes, n, stream, total, per_take, pass_ms);
}
