// s3dg_dgen_batch.cpp — s3dg_dgen_fill_batch and s3dg_verify_dgen_batch: a
// mixed-size batch of DG1 objects in one call.  The checks,
// the chunk records, their size classes and the launches are pure functions in
// s3dg_dgen_batch_plan.h; here is the HIP choreography.
//
// One call: every descriptor is checked before anything is enqueued.  The
// record table (one 32-byte record per 1 MiB block, sorted by size class) is
// built in one of the stream's two pinned tables, uploaded on the caller's
// stream, and read by one launch per class present: at most ten.  The stream
// orders the upload before the launches and both before the next call's
// upload into the same device table, so the fill returns without waiting.
#include "s3dg_ctx.h"

using namespace s3dg;

namespace {

// The next of the stream's two record tables with room for `recs` records; its
// pinned side is free once its last upload finished.
int table_reserve(StreamState *S, uint64_t recs, hipStream_t s, StreamState::DgenTable **out) {
    StreamState::DgenTable &T = S->dtab[S->dnext];
    S->dnext ^= 1;
    if (!T.uploaded) HIP_TRY(hipEventCreateWithFlags(&T.uploaded, hipEventDisableTiming), "hipEventCreate");
    HIP_TRY(hipEventSynchronize(T.uploaded), "hipEventSynchronize(chunk records)");
    if (recs > T.cap) {
        // launches of an earlier call may still read the device side
        HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(chunk records)");
        if (T.host) (void)hipHostFree(T.host);
        if (T.dev) (void)hipFree(T.dev);
        T.host = nullptr;
        T.dev = nullptr;
        T.cap = 0;
        const uint64_t cap = recs < 4096 ? 4096 : recs + recs / 4;
        HIP_TRY(hipHostMalloc((void **)&T.host, cap * sizeof(DgenChunkRec), hipHostMallocDefault),
                "hipHostMalloc(chunk records)");
        HIP_TRY(hipMalloc((void **)&T.dev, cap * sizeof(DgenChunkRec)), "hipMalloc(chunk records)");
        T.cap = cap;
    }
    *out = &T;
    return S3DG_OK;
}

// The call's arguments and descriptors, then its plan; S3DG_EINVAL with the
// refusal's message.  *live: something to launch.
int plan_call(s3dg_ctx *c, const void *base, const s3dg_obj_desc *d, uint64_t n, bool verify, const void *out,
              DgenBatchCheck &C, DgenBatchPlan &P) {
    if (const char *m = dgen_batch_args(base, d, n, verify, out)) return fail(S3DG_EINVAL, m);
    C = dgen_batch_check(d, n);
    if (C.msg) return fail(S3DG_EINVAL, dgen_batch_message(C.bad, C.msg));
    uint64_t knob;
    uint32_t draws;
    {
        std::lock_guard<std::mutex> g(c->mu);
        const uint64_t md = c->ks_min_draws[1];
        knob = md == kDefaultKsMinDraws[1] ? 0 : md;   // 0: not set by the caller
        draws = verify ? 64u : (uint32_t)c->ks[1].draws;
    }
    P = dgen_batch_plan(C, (uint32_t)c->cus, knob, draws, verify);
    if (P.msg) return fail(S3DG_EINVAL, P.msg);
    return S3DG_OK;
}

// Records built and on their way to the device; the launches may follow on s.
int upload_records(StreamState *S, const s3dg_obj_desc *d, uint64_t n, const DgenBatchCheck &C,
                   const DgenBatchPlan &P, hipStream_t s, const DgenChunkRec **dev) {
    StreamState::DgenTable *T = nullptr;
    if (int r = table_reserve(S, C.chunks, s, &T)) return r;
    dgen_batch_records(d, n, P, T->host);
    HIP_TRY(hipMemcpyAsync(T->dev, T->host, C.chunks * sizeof(DgenChunkRec), hipMemcpyHostToDevice, s),
            "hipMemcpyAsync(chunk records)");
    HIP_TRY(hipEventRecord(T->uploaded, s), "hipEventRecord");
    *dev = T->dev;
    return S3DG_OK;
}

}  // namespace

extern "C" int s3dg_dgen_fill_batch(s3dg_ctx *c, void *dst_base, const s3dg_obj_desc *d, uint64_t n, void *stream) {
    CTX_SCOPE(c);
    DgenBatchCheck C;
    DgenBatchPlan P;
    if (int r = plan_call(c, dst_base, d, n, false, nullptr, C, P)) return r;
    if (C.live == 0) return S3DG_OK;
    // every jump table before the first launch: a failure there leaves nothing enqueued
    const uint64_t *jt[kDgbClasses] = {};
    for (uint32_t k = 0; k < P.nlaunch; ++k)
        if (int r = jump_table(c, P.launch[k].lanes.lpc, P.launch[k].lanes.span, 0, &jt[k])) return r;
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    const DgenChunkRec *recs = nullptr;
    if (int r = upload_records(SL.get(), d, n, C, P, s, &recs)) return r;
    for (uint32_t k = 0; k < P.nlaunch; ++k) {
        const DgenLaunch &L = P.launch[k];
        KsShape sh = c->ks[1];
        if (L.zeros) {   // zero prefixes inside the lanes: the one-launch path's 4-wave workgroups, groups of 32 waves
            if (c->ks_auto_waves[1]) sh.waves = kDgenPrefixWaves;
            if (c->ks_auto_xcd[1]) sh.xcd_waves = kDgenPrefixXcdWaves;
        }
        HIP_TRY(launch_keystream_batch((uint8_t *)dst_base, recs + L.rec0, L.nrec, L.lanes.lpc, L.lanes.span, jt[k], sh,
                                       s),
                "launch k_keystream_batch");
    }
    return S3DG_OK;
}

extern "C" int s3dg_verify_dgen_batch(s3dg_ctx *c, const void *src_base, const s3dg_obj_desc *d, uint64_t n,
                                      void *stream, s3dg_verify_result *out, s3dg_verify_result *per_obj) {
    CTX_SCOPE(c);
    DgenBatchCheck C;
    DgenBatchPlan P;
    if (int r = plan_call(c, src_base, d, n, true, out, C, P)) return r;
    const s3dg_verify_result clean{0, 0, UINT64_MAX};
    VerifyRec host{0, 0, UINT64_MAX};
    if (C.live) {
        const uint64_t *jt[kDgbClasses] = {};
        for (uint32_t k = 0; k < P.nlaunch; ++k)
            if (int r = jump_table(c, P.launch[k].lanes.lpc, P.launch[k].lanes.span, 0, &jt[k])) return r;
        hipStream_t s = (hipStream_t)stream;
        StreamLock SL(c, s);
        StreamState *S = SL.get();
        if (per_obj && n > S->vobj_cap) {   // idle: every earlier verify on this stream has drained it
            if (S->vobj) (void)hipFree(S->vobj);
            S->vobj = nullptr;
            S->vobj_cap = 0;
            const uint64_t cap = n < 1024 ? 1024 : n;
            HIP_TRY(hipMalloc((void **)&S->vobj, verify_batch_obj_bytes(cap)), "hipMalloc(verify records)");
            S->vobj_cap = cap;
        }
        VerifyRec *tot = nullptr;
        {
            std::lock_guard<std::mutex> g(c->mu);
            if (!c->vrecs.empty()) {
                tot = c->vrecs.back();
                c->vrecs.pop_back();
            }
        }
        if (!tot) HIP_TRY(hipMalloc((void **)&tot, sizeof(VerifyRec)), "hipMalloc(verify record)");
        int r = S3DG_OK;
        hipError_t e = verify_rec_reset(tot, s);
        if (e == hipSuccess && per_obj) e = launch_verify_recs_reset(S->vobj, n, s);
        if (e != hipSuccess) r = hipfail(e, "reset verify records");
        const DgenChunkRec *recs = nullptr;
        if (r == S3DG_OK) r = upload_records(S, d, n, C, P, s, &recs);
        for (uint32_t k = 0; r == S3DG_OK && k < P.nlaunch; ++k) {
            const DgenLaunch &L = P.launch[k];
            e = launch_verify_keystream_batch((const uint8_t *)src_base, recs + L.rec0, L.nrec, L.lanes.lpc,
                                              L.lanes.span, jt[k], tot, per_obj ? S->vobj : nullptr, s);
            if (e != hipSuccess) r = hipfail(e, "launch k_verify_keystream_batch");
        }
        if (r == S3DG_OK) {
            e = hipMemcpyAsync(&host, tot, sizeof(host), hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) r = hipfail(e, "hipMemcpyAsync(verify record)");
        }
        // drained on every path: the totals record goes back to the list only when idle
        const hipError_t se = hipStreamSynchronize(s);
        if (se == hipSuccess) {
            std::lock_guard<std::mutex> g(c->mu);
            c->vrecs.push_back(tot);
        } else if (r == S3DG_OK) {
            r = hipfail(se, "hipStreamSynchronize(verify)");
        }
        if (r != S3DG_OK) return r;
        if (per_obj && host.bytes) {   // the one copy of the per-object records: only for a call that found something
            static_assert(sizeof(s3dg_verify_result) == 24, "per-object records are copied as they are");
            HIP_TRY(hipMemcpyAsync(per_obj, S->vobj, verify_batch_obj_bytes(n), hipMemcpyDeviceToHost, s),
                    "hipMemcpyAsync(verify records)");
            HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(verify)");
        }
    }
    if (per_obj && !host.bytes)
        for (uint64_t k = 0; k < n; ++k) per_obj[k] = clean;
    out->mismatched_bytes = host.bytes;
    out->mismatched_blocks = host.blocks;
    out->first_offset = host.first;
    return S3DG_OK;
}
