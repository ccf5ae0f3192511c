// s3dg_npz_batch.cpp — s3dg_npz_archive_size, s3dg_npz_frame_batch and
// s3dg_npz_check_batch: a list of NPZ archives framed and checked in HBM, one
// device call per list.  The checks, the layouts and the
// ready-made header bytes are pure functions in s3dg_npz_plan.h; the kernels
// are in s3dg_npz_batch.hip; here is the HIP choreography, which is
// s3dg_tfrecord_var.cpp's, over the same two tables of the stream.
//
// One call: every descriptor is checked before anything is reserved or
// enqueued.  Tables, fronts and backs are built in one of the stream's two
// pinned tables and uploaded on the caller's stream in one copy, where the
// launches follow it: the host arrays are consumed when the call returns, and
// the frame form returns without waiting.
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
        // launches of an earlier call may still read the device side
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

// The whole call on s, n > 0.  Returns without waiting; *ws is the device side.
int enqueue(s3dg_ctx *c, StreamState *S, bool frame, const uint8_t *src, uint8_t *base, const s3dg_npz_archive *archives,
            uint64_t n, const s3dg_npz_member *members, const uint8_t *blob, const NpzCounts &C, const NpzLayout &L,
            hipStream_t s, uint8_t **ws) {
    {
        std::lock_guard<std::mutex> g(c->crc_mu);
        HIP_TRY(crc_tables_device(&c->crc_tab), "crc tables");
    }
    StreamState::CrcTable *T = nullptr;
    if (int r = table_reserve(S, L.upload, L.bytes, s, &T)) return r;
    npz_build(archives, n, members, blob, C, L, powers(),
              [](const uint8_t *p, uint64_t len) { return crc32_host_update(0, p, len); }, T->host);
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, L.upload, hipMemcpyHostToDevice, s), "hipMemcpyAsync(npz table)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    if (!frame) HIP_TRY(hipMemsetAsync(T->dev + L.res, 0, n * sizeof(NpzDevRes), s), "hipMemsetAsync(npz results)");
    HIP_TRY(npz_batch_launch(frame, src, base, T->dev, L, C, c->crc_tab, c->cus, s), "launch k_npz");
    *ws = T->dev;
    return S3DG_OK;
}

}  // namespace

extern "C" int s3dg_npz_archive_size(const s3dg_npz_member *m, uint64_t members, uint64_t *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    if (members && !m) return fail(S3DG_EINVAL, "null member array");
    if (!npz_archive_size(m, members, out)) return fail(S3DG_EINVAL, "the archive's size overflows");
    return S3DG_OK;
}

extern "C" int s3dg_npz_frame_batch(s3dg_ctx *c, const void *src_base, void *dst_base, const s3dg_npz_archive *archives,
                                    uint64_t n, const s3dg_npz_member *members, uint64_t nmembers, const uint8_t *blob,
                                    uint64_t blob_len, void *stream) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    NpzCounts C;
    std::string why;
    if (!npz_check(true, (uint64_t)(uintptr_t)src_base, (uint64_t)(uintptr_t)dst_base, archives, n, members, nmembers,
                   blob != nullptr, blob_len, &C, &why))
        return fail(S3DG_EINVAL, why);
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    uint8_t *ws = nullptr;
    return enqueue(c, SL.get(), true, (const uint8_t *)src_base, (uint8_t *)dst_base, archives, n, members, blob, C,
                   npz_layout(C, n), s, &ws);
}

extern "C" int s3dg_npz_check_batch(s3dg_ctx *c, const void *base, const s3dg_npz_archive *archives, uint64_t n,
                                    const s3dg_npz_member *members, uint64_t nmembers, const uint8_t *blob, uint64_t blob_len,
                                    void *stream, s3dg_npz_result *total, s3dg_npz_result *per_archive) {
    CTX_SCOPE(c);
    if (!total) return fail(S3DG_EINVAL, "null output");
    NpzCounts C;
    std::string why;
    if (!npz_check(false, 0, (uint64_t)(uintptr_t)base, archives, n, members, nmembers, blob != nullptr, blob_len, &C, &why))
        return fail(S3DG_EINVAL, why);
    std::vector<NpzDevRes> got;
    if (n) {
        hipStream_t s = (hipStream_t)stream;
        StreamLock SL(c, s);
        const NpzLayout L = npz_layout(C, n);
        uint8_t *ws = nullptr;
        // the kernels only read through this pointer in the check form
        if (int r = enqueue(c, SL.get(), false, nullptr, const_cast<uint8_t *>((const uint8_t *)base), archives, n, members, blob,
                            C, L, s, &ws))
            return r;
        got.resize(n);
        HIP_TRY(hipMemcpyAsync(got.data(), ws + L.res, n * sizeof(NpzDevRes), hipMemcpyDeviceToHost, s),
                "hipMemcpyAsync(npz results)");
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(npz check)");
    }
    s3dg_npz_result tot{0, 0, 0, 0, 0, UINT64_MAX, UINT64_MAX};
    for (uint64_t k = 0; k < n; ++k) {
        const NpzDevRes &g = got[k];
        s3dg_npz_result r{archives[k].members, g.bad_members, g.bad_local, g.bad_crc, g.bad_directory ? 1u : 0u, UINT64_MAX,
                          UINT64_MAX};
        if (g.bad_members || g.bad_directory) {
            r.first_archive = k;
            if (g.bad_members) r.first_member = ~(uint64_t)g.first_inv;
            if (tot.first_archive == UINT64_MAX) {
                tot.first_archive = k;
                tot.first_member = r.first_member;
            }
        }
        tot.members += r.members;
        tot.bad_members += r.bad_members;
        tot.bad_local += r.bad_local;
        tot.bad_crc += r.bad_crc;
        tot.bad_directory += r.bad_directory;
        if (per_archive) per_archive[k] = r;
    }
    *total = tot;
    return S3DG_OK;
}
