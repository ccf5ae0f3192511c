// s3dg_verify_batch.cpp — s3dg_verify_controlled_batch: the read-side twin of
// s3dg_fill_controlled_batch with a result per object.  The
// argument checks, the pass over the descriptors, the cuts and the record
// counts are in s3dg_verify_batch_plan.h; here is the HIP choreography.
//
// One call: every descriptor is checked before anything is enqueued.  Then the
// sub-batches (16 Ki objects first, doubling to 256 Ki) are staged as they are
// and uploaded on the stream's side stream, where a scan of the tile counts
// and k_verify_batch_map build the records while the previous sub-batch is
// compared on the caller's stream.  Staging sets, record maps and their events
// are the stream's batch state, shared with the fill.  All sub-batches add
// into one totals record (from the context's idle list) and into the call's
// per-object records (the stream's, n x 24 bytes, reset on the stream first);
// there is one wait, at the end, and the per-object records are copied back
// only when the totals are not clean.
#include "s3dg_ctx.h"

using namespace s3dg;

namespace {

// Scan scratch of staging set G for its capacity under the verify's scan.
int scan_tmp_reserve(StreamState::Stage &G, hipStream_t up) {
    size_t need = 0;
    HIP_TRY(launch_verify_batch_scan(nullptr, G.cap, kTileShiftMin, nullptr, nullptr, &need, up), "hipcub scan size");
    if (need <= G.scan_tmp_bytes) return S3DG_OK;
    HIP_TRY(hipEventSynchronize(G.consumed), "hipEventSynchronize(batch staging)");
    if (G.scan_tmp) (void)hipFree(G.scan_tmp);
    G.scan_tmp = nullptr;
    G.scan_tmp_bytes = 0;
    HIP_TRY(hipMalloc(&G.scan_tmp, need), "hipMalloc(batch scan)");
    G.scan_tmp_bytes = need;
    return S3DG_OK;
}

// Enqueues the whole call: sub-batch k+1's upload and records on S->up while
// sub-batch k is compared on s.  tot and pobj (null: totals only) are reset on s already.
int enqueue(s3dg_ctx *c, StreamState *S, hipStream_t s, const uint8_t *src, const s3dg_obj_desc *d, uint64_t n,
            VerifyRec *tot, VerifyRec *pobj) {
    const int waves = cfg_for(c).waves_per_block;   // auto: the stream verify's
    uint64_t sub = kVerifySubFirst;
    for (uint64_t k0 = 0, k1; k0 < n; k0 = k1) {
        k1 = verify_batch_cut(k0, n, sub);
        const uint64_t cnt = k1 - k0;
        StreamState::Stage &G = S->stage[S->next];
        S->next ^= 1;
        if (int r = stage_reserve(G, cnt, S->up)) return r;
        if (int r = scan_tmp_reserve(G, S->up)) return r;
        const VerifyBatchScan P = verify_batch_scan(d, k0, k1, G.host);
        if (P.m == 0) continue;
        const uint32_t tshift = verify_batch_tile_shift(P, c->tile_shift);
        const uint64_t recs = P.ntiles[tshift];
        // record map tb: free once the launch two sub-batches back has read it
        const int tb = S->bnext;
        S->bnext ^= 1;
        if (recs > S->btile_cap[tb]) {
            HIP_TRY(hipEventSynchronize(S->filled[tb]), "hipEventSynchronize(tile map)");
            if (int r = tile_map_grow(&S->btiles[tb], &S->btile_cap[tb], recs)) return r;
        }
        VTileRec *map = reinterpret_cast<VTileRec *>(S->btiles[tb]);
        HIP_TRY(hipMemcpyAsync(G.dev, G.host, cnt * sizeof(s3dg_obj_desc), hipMemcpyHostToDevice, S->up),
                "hipMemcpyAsync(batch descriptors)");
        HIP_TRY(hipEventRecord(G.uploaded, S->up), "hipEventRecord");
        size_t tmp = G.scan_tmp_bytes;
        HIP_TRY(launch_verify_batch_scan(G.dev, cnt, tshift, G.rec_lo, G.scan_tmp, &tmp, S->up), "hipcub scan");
        HIP_TRY(hipStreamWaitEvent(S->up, S->filled[tb], 0), "hipStreamWaitEvent");
        HIP_TRY(launch_verify_batch_map(G.dev, cnt, G.rec_lo, map, tshift, S->up), "launch k_verify_batch_map");
        HIP_TRY(hipEventRecord(G.consumed, S->up), "hipEventRecord");
        HIP_TRY(hipEventRecord(S->mapped[tb], S->up), "hipEventRecord");
        HIP_TRY(hipStreamWaitEvent(s, S->mapped[tb], 0), "hipStreamWaitEvent");
        HIP_TRY(launch_verify_batch(waves, src, map, recs, tshift, c->base_dev, tot, pobj ? pobj + k0 : nullptr, s),
                "launch k_verify_batch");
        HIP_TRY(hipEventRecord(S->filled[tb], s), "hipEventRecord");
    }
    return S3DG_OK;
}

}  // namespace

extern "C" int s3dg_verify_controlled_batch(s3dg_ctx *c, const void *src_base, const s3dg_obj_desc *d, uint64_t n,
                                            void *stream, s3dg_verify_result *out, s3dg_verify_result *per_obj) {
    CTX_SCOPE(c);
    if (const char *m = verify_batch_args(src_base, d, n, out)) return fail(S3DG_EINVAL, m);
    const VerifyBatchCheck C = verify_batch_check(d, n);
    if (C.msg) return fail(S3DG_EINVAL, C.msg);
    const s3dg_verify_result clean{0, 0, UINT64_MAX};
    VerifyRec host{0, 0, UINT64_MAX};
    if (C.live) {
        hipStream_t s = (hipStream_t)stream;
        StreamLock SL(c, s);
        StreamState *S = SL.get();
        if (int r = batch_state_init(S)) return r;
        if (per_obj && n > S->vobj_cap) {   // idle: every earlier call on this stream has drained it
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
        if (r == S3DG_OK) r = enqueue(c, S, s, (const uint8_t *)src_base, d, n, tot, per_obj ? S->vobj : nullptr);
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
