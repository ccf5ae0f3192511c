// s3dg_tfrecord_var.cpp — s3dg_tfrecord_var_size, s3dg_tfrecord_frame_var_batch,
// s3dg_tfrecord_check_var_batch and s3dg_tfrecord_index_batch: TFRecord shards
// of records of any length framed and checked in HBM, and framed streams
// nobody has described indexed there, one device call per list (DESIGN.md
// §5.5.2).  The checks, the per-record table and the walk's rule are pure
// functions in s3dg_tfrecord_var_plan.h; the kernels are in
// s3dg_tfrecord_var.hip; here is the HIP choreography, which is
// s3dg_tfrecord.cpp's, over the same two tables of the stream.
//
// One call: every descriptor and every length is checked before anything is
// reserved or enqueued.  The table (16 bytes per record) is built in one of the
// stream's two pinned tables and uploaded on the caller's stream, where the
// launches follow it: `shards` and `lengths` are consumed when the call
// returns, and the frame form returns without waiting.
#include "s3dg_ctx.h"

#include <cstring>
#include <vector>

using namespace s3dg;

namespace {

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
        // launches of an earlier call may still read the device side
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

// The whole call on s, C.live > 0.  Returns without waiting.
int enqueue(s3dg_ctx *c, StreamState *S, bool frame, const uint8_t *src, uint8_t *dst, uint8_t *idx,
            const s3dg_tfrecord_var_shard *shards, uint64_t n, const uint64_t *lengths, const TfvCounts &C, TfrDevRes *res,
            hipStream_t s) {
    {
        std::lock_guard<std::mutex> g(c->crc_mu);
        HIP_TRY(crc_tables_device(&c->crc_tab), "crc tables");
    }
    StreamState::CrcTable *T = nullptr;
    if (int r = table_reserve(S, tfv_table_bytes(C), tfv_device_bytes(C), s, &T)) return r;
    tfv_build(shards, n, lengths, C, powers(), T->host);
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, tfv_table_bytes(C), hipMemcpyHostToDevice, s),
            "hipMemcpyAsync(tfrecord table)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    HIP_TRY(tfrecord_var_launch(frame, src, dst, idx, T->dev, C, c->crc_tab, c->cus, res, s), "launch k_tfrecord_var");
    return S3DG_OK;
}

}  // namespace

extern "C" int s3dg_tfrecord_var_size(const uint64_t *lengths, uint64_t records, uint64_t *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    if (records && !lengths) return fail(S3DG_EINVAL, "null lengths array");
    if (!tfv_size(lengths, records, out)) return fail(S3DG_EINVAL, "sum(16 + length) overflows");
    return S3DG_OK;
}

extern "C" int s3dg_tfrecord_frame_var_batch(s3dg_ctx *c, const void *src_base, void *dst_base, void *idx_base,
                                             const s3dg_tfrecord_var_shard *shards, uint64_t n, const uint64_t *lengths,
                                             uint64_t nlengths, void *stream) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    TfvCounts C;
    std::string why;
    if (!tfv_check(true, (uint64_t)(uintptr_t)src_base, (uint64_t)(uintptr_t)dst_base, (uint64_t)(uintptr_t)idx_base, shards,
                   n, lengths, nlengths, &C, &why))
        return fail(S3DG_EINVAL, why);
    if (C.live == 0) return S3DG_OK;
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    return enqueue(c, SL.get(), true, (const uint8_t *)src_base, (uint8_t *)dst_base, (uint8_t *)idx_base, shards, n, lengths,
                   C, nullptr, s);
}

extern "C" int s3dg_tfrecord_check_var_batch(s3dg_ctx *c, const void *base, const s3dg_tfrecord_var_shard *shards, uint64_t n,
                                             const uint64_t *lengths, uint64_t nlengths, void *stream,
                                             s3dg_tfrecord_result *total, s3dg_tfrecord_result *per_shard) {
    CTX_SCOPE(c);
    if (!total) return fail(S3DG_EINVAL, "null output");
    TfvCounts C;
    std::string why;
    if (!tfv_check(false, 0, (uint64_t)(uintptr_t)base, 0, shards, n, lengths, nlengths, &C, &why))
        return fail(S3DG_EINVAL, why);
    s3dg_tfrecord_result tot{0, 0, 0, 0, 0, UINT64_MAX, UINT64_MAX};
    std::vector<TfrDevRes> got;
    if (C.live) {
        hipStream_t s = (hipStream_t)stream;
        StreamLock SL(c, s);
        StreamState *S = SL.get();
        if (n > S->tfr_out_cap) {   // idle: every earlier check on this stream has drained it
            if (S->tfr_out) (void)hipFree(S->tfr_out);
            S->tfr_out = nullptr;
            S->tfr_out_cap = 0;
            const uint64_t cap = n < 256 ? 256 : n;
            HIP_TRY(hipMalloc((void **)&S->tfr_out, cap * sizeof(TfrDevRes)), "hipMalloc(tfrecord results)");
            S->tfr_out_cap = cap;
        }
        HIP_TRY(hipMemsetAsync(S->tfr_out, 0, n * sizeof(TfrDevRes), s), "hipMemsetAsync(tfrecord results)");
        if (int r = enqueue(c, S, false, (const uint8_t *)base, nullptr, nullptr, shards, n, lengths, C, S->tfr_out, s))
            return r;
        got.resize(n);
        HIP_TRY(hipMemcpyAsync(got.data(), S->tfr_out, n * sizeof(TfrDevRes), hipMemcpyDeviceToHost, s),
                "hipMemcpyAsync(tfrecord results)");
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(tfrecord check)");
    }
    for (uint64_t k = 0; k < n; ++k) {
        s3dg_tfrecord_result r{shards[k].records, 0, 0, 0, 0, UINT64_MAX, UINT64_MAX};
        if (C.live && got[k].bad_records) {
            const TfrDevRes &g = got[k];
            r = s3dg_tfrecord_result{shards[k].records, g.bad_records, g.bad_length, g.bad_length_crc, g.bad_data_crc, k,
                                     ~(uint64_t)g.first_inv};
            if (tot.first_shard == UINT64_MAX) {
                tot.first_shard = k;
                tot.first_record = r.first_record;
            }
        }
        tot.records += r.records;
        tot.bad_records += r.bad_records;
        tot.bad_length += r.bad_length;
        tot.bad_length_crc += r.bad_length_crc;
        tot.bad_data_crc += r.bad_data_crc;
        if (per_shard) per_shard[k] = r;
    }
    *total = tot;
    return S3DG_OK;
}

extern "C" int s3dg_tfrecord_index_batch(s3dg_ctx *c, const void *base, void *idx_base, const s3dg_tfrecord_stream *streams,
                                         uint64_t n, void *stream, s3dg_tfrecord_walk_result *results) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    std::string why;
    if (!tfv_walk_check((uint64_t)(uintptr_t)base, (uint64_t)(uintptr_t)idx_base, streams, n, results != nullptr, &why))
        return fail(S3DG_EINVAL, why);
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    // the descriptors up, the results behind them on the device side
    const uint64_t hb = n * sizeof(s3dg_tfrecord_stream), res_off = span_align256(hb);
    StreamState::CrcTable *T = nullptr;
    if (int r = table_reserve(SL.get(), hb, res_off + n * sizeof(s3dg_tfrecord_walk_result), s, &T)) return r;
    memcpy(T->host, streams, hb);
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, hb, hipMemcpyHostToDevice, s), "hipMemcpyAsync(tfrecord streams)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    s3dg_tfrecord_walk_result *res_dev = reinterpret_cast<s3dg_tfrecord_walk_result *>(T->dev + res_off);
    HIP_TRY(tfrecord_walk_launch((const uint8_t *)base, (uint8_t *)idx_base,
                                 reinterpret_cast<const s3dg_tfrecord_stream *>(T->dev), n, res_dev, c->cus, s),
            "launch k_tfrecord_walk");
    HIP_TRY(hipMemcpyAsync(results, res_dev, n * sizeof(s3dg_tfrecord_walk_result), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(tfrecord walk results)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(tfrecord index)");
    return S3DG_OK;
}
