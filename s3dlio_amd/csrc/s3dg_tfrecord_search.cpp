// s3dg_tfrecord_search.cpp — s3dg_tfrecord_index_search_batch,
// s3dg_tfrecord_index_search_timed and s3dg_tfrecord_search_geometry:
// s3dg_tfrecord_index_batch's results for framed streams nobody has described,
// found with parallelism inside a stream.  The rules are
// pure functions in s3dg_tfrecord_search_plan.h, the kernels are in
// s3dg_tfrecord_search.hip; here is the HIP choreography.
//
// One call, two halves.  The first workspace is sized from the streams' bytes
// (a bit per position and two bytes per 64 of them) and takes the candidate
// pass and the sum over the tiles' counts; the call then waits for the number
// of candidates, sizes the second workspace from it (52 bytes each) and
// enqueues the link, the doubling, the anchor walk and the fill.  Both
// workspaces are the stream's two TFRecord tables, so a call leaves nothing of
// its own behind and the next call on the stream finds them idle: the call
// returns with the stream drained.
#include "s3dg_ctx.h"

#include <cstring>
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

constexpr int kMarks = 8;   // start, searched, summed | resolve's start, linked, doubled, walked, filled

struct Marks {
    hipEvent_t ev[kMarks] = {};
    bool on = false;
    ~Marks() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

int search(s3dg_ctx *c, const void *base, void *idx_base, const s3dg_tfrecord_stream *streams, uint64_t n, void *stream,
           s3dg_tfrecord_walk_result *results, float *pass_ms) {
    std::string why;
    if (!tfv_walk_check((uint64_t)(uintptr_t)base, (uint64_t)(uintptr_t)idx_base, streams, n, results != nullptr, &why))
        return fail(S3DG_EINVAL, why);
    std::vector<uint64_t> tile0(n + 1);
    if (!tfs_tile_table(streams, n, tile0.data())) return fail(S3DG_EINVAL, "more than 2^31 - 2 search tiles in one call");
    const uint64_t tiles = tile0[n];
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    Marks M;
    if (pass_ms) {
        M.on = true;
        for (hipEvent_t &e : M.ev) HIP_TRY(hipEventCreate(&e), "hipEventCreate");
    }
    auto mark = [&](int i) -> hipError_t { return M.on ? hipEventRecord(M.ev[i], s) : hipSuccess; };
    size_t tmp_bytes = 0;
    HIP_TRY(tfrecord_search_scan(nullptr, &tmp_bytes, nullptr, tiles, s), "hipcub scan size");
    const TfsPlanA A = tfs_plan_a(n, tiles, tmp_bytes);
    StreamState::CrcTable *TA = nullptr, *TB = nullptr;
    if (int r = table_reserve(SL.get(), A.upload_bytes, A.bytes, s, &TA)) return r;
    memcpy(TA->host, streams, n * sizeof(s3dg_tfrecord_stream));
    memcpy(TA->host + A.tile0_off, tile0.data(), (n + 1) * 8);
    HIP_TRY(hipMemcpyAsync(TA->dev, TA->host, A.upload_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync(tfrecord streams)");
    HIP_TRY(hipEventRecord(TA->uploaded, s), "hipEventRecord");
    HIP_TRY(mark(0), "hipEventRecord");
    HIP_TRY(tfrecord_search_candidates((const uint8_t *)base, TA->dev, A, n, tiles, tmp_bytes, c->cus, M.on ? M.ev[1] : nullptr, s),
            "launch k_tfs_candidates");
    HIP_TRY(mark(2), "hipEventRecord");
    uint64_t nodes = 0;
    HIP_TRY(hipMemcpyAsync(&nodes, TA->dev + A.tbase_off + tiles * 8, 8, hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(tfrecord candidates)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(tfrecord search)");
    if (nodes > kTfsMaxNodes) return fail(S3DG_EINVAL, "more than 2^32 - 16 header candidates in one call");
    const TfsPlanB B = tfs_plan_b(nodes);
    if (int r = table_reserve(SL.get(), 0, B.bytes, s, &TB)) return r;
    HIP_TRY(mark(3), "hipEventRecord");
    HIP_TRY(tfrecord_search_resolve((const uint8_t *)base, (uint8_t *)idx_base, TA->dev, A, TB->dev, B, n, tiles, (uint32_t)nodes,
                                    c->cus, M.on ? M.ev + 4 : nullptr, s),
            "launch k_tfs_anchor");
    HIP_TRY(hipMemcpyAsync(results, TA->dev + A.res_off, n * sizeof(s3dg_tfrecord_walk_result), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(tfrecord walk results)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(tfrecord search)");
    if (pass_ms) {
        const int from[6] = {0, 1, 3, 4, 5, 6};   // candidates, sum | link, doubling, anchor walk, fill
        for (int i = 0; i < 6; ++i) HIP_TRY(hipEventElapsedTime(&pass_ms[i], M.ev[from[i]], M.ev[from[i] + 1]), "hipEventElapsedTime");
    }
    return S3DG_OK;
}

}  // namespace

extern "C" int s3dg_tfrecord_search_geometry(uint32_t *tile_bytes, uint32_t *hop_records) {
    if (!tile_bytes || !hop_records) return fail(S3DG_EINVAL, "null output");
    *tile_bytes = kTfsTile;
    *hop_records = kTfsHop;
    return S3DG_OK;
}

extern "C" int s3dg_tfrecord_index_search_batch(s3dg_ctx *c, const void *base, void *idx_base, const s3dg_tfrecord_stream *streams,
                                                uint64_t n, void *stream, s3dg_tfrecord_walk_result *results) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    return search(c, base, idx_base, streams, n, stream, results, nullptr);
}

extern "C" int s3dg_tfrecord_index_search_timed(s3dg_ctx *c, const void *base, void *idx_base, const s3dg_tfrecord_stream *streams,
                                                uint64_t n, void *stream, s3dg_tfrecord_walk_result *results, float *pass_ms) {
    CTX_SCOPE(c);
    if (!pass_ms) return fail(S3DG_EINVAL, "null pass_ms");
    for (int i = 0; i < 6; ++i) pass_ms[i] = 0.f;
    if (n == 0) return S3DG_OK;
    return search(c, base, idx_base, streams, n, stream, results, pass_ms);
}
