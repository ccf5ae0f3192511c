// s3dg_batchfill.cpp — s3dg_fill_controlled_batch: mixed-size batches through
// the tiled batch kernel.  The pass over the descriptors and the choice of
// layout are in s3dg_batch_plan.h; here are the host threads that run the
// pass, the staging and the HIP choreography around it.
#include "s3dg_ctx.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <thread>

using namespace s3dg;

namespace {

// Mixed-size batch ("Batches"): the descriptors are cut into
// sub-batches (kBatchSubFirst objects first, doubling to kBatchSubMax) so the host's pass
// over sub-batch k+1 overlaps the GPU's fill of sub-batch k.  Per sub-batch
// the host makes one pass on up to 8 threads: it validates, counts slots and
// copies the 40-B descriptors into pinned staging (empty ones squeezed out
// afterwards); the upload runs on the stream's side
// stream, where a device scan of the tile counts gives each object's record
// offset and k_batch_map derives prefix parameters and tile records.
// Record layout per sub-batch (plan_sub_batch, s3dg_batch_plan.h):
//   * tiles of 2^tshift blocks (2..64) per object, the object's block 0 at
//     slot `lead` = its 4 KiB granule (mod 8): dead slots at both ends of
//     every object, and XCD-aligned (slot = granule mod 8) from 8-block
//     tiles up; forced 2- and 4-block tiles align mod 2 and mod 4 only;
//   * dense (tshift 0): objects 4 KiB-aligned, sorted and non-overlapping;
//     one record per 4 KiB granule of the sub-batch's address range, so slot
//     = granule and only gaps are dead.
// Descriptors are checked per sub-batch: on an error the objects of earlier
// sub-batches may already be enqueued.

// A few persistent host threads for the batch passes: run(parts, fn) calls
// fn(0..parts-1), part 0 in the caller.  One run at a time; a second caller
// meanwhile runs its parts itself.
class PrepPool {
public:
    static PrepPool &get() {
        static PrepPool *p = new PrepPool();   // never destroyed: workers outlive main
        return *p;
    }
    void run(int parts, const std::function<void(int)> &fn) {
        std::unique_lock<std::mutex> busy(run_mu_, std::try_to_lock);
        if (!busy.owns_lock() || parts <= 1) {
            for (int q = 0; q < parts; ++q) fn(q);
            return;
        }
        {
            std::lock_guard<std::mutex> g(mu_);
            fn_ = &fn;
            parts_ = parts;
            next_.store(1);
            left_ = parts - 1;
            ++gen_;
        }
        cv_.notify_all();
        fn(0);
        for (int q; (q = next_.fetch_add(1)) < parts;) finish_one(q);
        std::unique_lock<std::mutex> g(mu_);
        done_cv_.wait(g, [&] { return left_ == 0; });
        fn_ = nullptr;
    }

private:
    PrepPool() {
        for (int k = 0; k < kPrepParts - 1; ++k) std::thread([this] { loop(); }).detach();
    }
    void finish_one(int q) {
        (*fn_)(q);
        std::lock_guard<std::mutex> g(mu_);
        if (--left_ == 0) done_cv_.notify_all();
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return gen_ != seen; });
                seen = gen_;
            }
            for (int q; (q = next_.fetch_add(1)) < parts_;) finish_one(q);
        }
    }
    std::mutex run_mu_, mu_;
    std::condition_variable cv_, done_cv_;
    const std::function<void(int)> *fn_ = nullptr;
    int parts_ = 0, left_ = 0;
    std::atomic<int> next_{0};
    uint64_t gen_ = 0;
};

}  // namespace

namespace s3dg {

// The stream's batch state, made on its first batch: the upload stream and
// the events of both staging sets and both record maps.
int batch_state_init(StreamState *S) {
    if (!S->up) HIP_TRY(hipStreamCreateWithFlags(&S->up, hipStreamNonBlocking), "hipStreamCreate(upload)");
    for (auto &G : S->stage)
        for (hipEvent_t *ev : {&G.uploaded, &G.consumed})
            if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming), "hipEventCreate");
    for (int q = 0; q < 2; ++q)
        for (hipEvent_t *ev : {&S->mapped[q], &S->filled[q]})
            if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming), "hipEventCreate");
    return S3DG_OK;
}

// Staging for n descriptors: the host buffer is free once its last upload
// finished, the device copy once the k_batch_map that read it finished.
int stage_reserve(StreamState::Stage &G, uint64_t n, hipStream_t up) {
    HIP_TRY(hipEventSynchronize(G.uploaded), "hipEventSynchronize(batch staging)");
    if (n <= G.cap) return S3DG_OK;
    HIP_TRY(hipEventSynchronize(G.consumed), "hipEventSynchronize(batch staging)");
    if (G.host) (void)hipHostFree(G.host);
    for (void *p : {(void *)G.dev, (void *)G.rec_lo, G.scan_tmp})
        if (p) (void)hipFree(p);
    G.host = nullptr; G.dev = nullptr; G.rec_lo = nullptr; G.scan_tmp = nullptr;
    G.cap = 0; G.scan_tmp_bytes = 0;
    const uint64_t cap = n < 1024 ? 1024 : n;
    size_t tmp = 0;
    HIP_TRY(launch_batch_scan(nullptr, cap, kTileShiftMin, 0, nullptr, nullptr, &tmp, up), "hipcub scan size");
    HIP_TRY(hipHostMalloc((void **)&G.host, cap * sizeof(s3dg_obj_desc), hipHostMallocDefault),
            "hipHostMalloc(batch staging)");
    HIP_TRY(hipMalloc((void **)&G.dev, cap * sizeof(s3dg_obj_desc)), "hipMalloc(batch staging)");
    HIP_TRY(hipMalloc((void **)&G.rec_lo, cap * sizeof(uint64_t)), "hipMalloc(batch records)");
    HIP_TRY(hipMalloc(&G.scan_tmp, tmp ? tmp : 1), "hipMalloc(batch scan)");
    G.scan_tmp_bytes = tmp;
    G.cap = cap;
    return S3DG_OK;
}

}  // namespace s3dg

namespace {

// One pass over d[k0, k1) in parts (validate, count, stage into H), merged in order.
BatchScan scan_sub_batch(const s3dg_obj_desc *d, uint64_t k0, uint64_t k1, uintptr_t base, s3dg_obj_desc *H,
                         uint64_t split) {
    const int parts = batch_parts(k1 - k0);
    uint64_t cut[kPrepParts + 1];
    for (int q = 0; q <= parts; ++q) cut[q] = batch_cut(k0, k1, q, parts);
    BatchScan part[kPrepParts];
    PrepPool::get().run(parts,
                        [&](int q) { batch_scan(d, cut[q], cut[q + 1], base, part[q], H + (cut[q] - k0), split); });
    return batch_scan_merge(part, parts);
}

}  // namespace

extern "C" int s3dg_fill_controlled_batch(s3dg_ctx *c, void *dst_base, const s3dg_obj_desc *d, uint64_t n,
                                          void *stream) {
    CTX_SCOPE(c);
    if (n == 0) return S3DG_OK;
    if (!d) return fail(S3DG_EINVAL, "null descriptor array");
    if (!dst_base || !aligned16(dst_base)) return fail(S3DG_EINVAL, "dst_base must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const uintptr_t base = (uintptr_t)dst_base;
    StreamLock SL(c, s);
    StreamState *S = SL.get();
    if (int r = batch_state_init(S)) return r;
    uint64_t sub = kBatchSubFirst;
    for (uint64_t k0 = 0, k1; k0 < n; k0 = k1) {
        k1 = n - k0 < sub ? n : k0 + sub;
        sub = sub * 2 < kBatchSubMax ? sub * 2 : kBatchSubMax;
        StreamState::Stage &G = S->stage[S->next];
        S->next ^= 1;
        if (int r = stage_reserve(G, k1 - k0, S->up)) return r;
        const BatchKnobs K{c->tile_shift, c->tile_force_dense, c->split_blocks};
        const BatchScan P = scan_sub_batch(d, k0, k1, base, G.host, K.split_blocks);
        if (P.err) return fail(P.err, P.msg);
        const uint64_t m = P.m;
        if (m == 0) continue;
        const BatchPlan B = plan_sub_batch(P, base, K);
        if (B.uniform) {   // a stream: no records per tile or granule
            const uint64_t nb = obj_blocks(P.ufirst.size);
            PrefixParams pp;
            if (int r = make_prefix(nb, P.ufirst.dedup, P.ufirst.f_num, P.ufirst.f_den, &pp)) return r;
            if (int r = fill_uniform(c, (uint8_t *)dst_base + P.ufirst.dst_off, P.ufirst.size, P.ustride, m, pp,
                                     P.ufirst.entropy, 0, s, S))
                return r;
            continue;
        }
        order_staging(G.host, k1 - k0, m, B, K.split_blocks);
        // record map tb: free once the fill two sub-batches back has read it
        const int tb = S->bnext;
        S->bnext ^= 1;
        if (B.recs > S->btile_cap[tb]) {
            HIP_TRY(hipEventSynchronize(S->filled[tb]), "hipEventSynchronize(tile map)");
            if (int r = tile_map_grow(&S->btiles[tb], &S->btile_cap[tb], B.recs)) return r;
        }
        // upload and map on the side stream, overlapping the previous fill
        HIP_TRY(hipMemcpyAsync(G.dev, G.host, m * sizeof(s3dg_obj_desc), hipMemcpyHostToDevice, S->up),
                "hipMemcpyAsync(batch descriptors)");
        HIP_TRY(hipEventRecord(G.uploaded, S->up), "hipEventRecord");
        // each class's scan and records, the small class's records first (the dense layout needs no scan)
        for (int q = 0; q < B.nclass; ++q) {
            const auto &C = B.cls[q];
            if (!C.tshift) continue;
            size_t tmp = G.scan_tmp_bytes;
            HIP_TRY(launch_batch_scan(G.dev + C.first, C.count, C.tshift, base, G.rec_lo + C.first, G.scan_tmp, &tmp,
                                      S->up),
                    "hipcub scan");
        }
        HIP_TRY(hipStreamWaitEvent(S->up, S->filled[tb], 0), "hipStreamWaitEvent");
        for (int q = 0; q < B.nclass; ++q) {
            const auto &C = B.cls[q];
            HIP_TRY(launch_batch_map(G.dev + C.first, C.count, G.rec_lo + C.first, S->btiles[tb] + C.rec0, C.tshift,
                                     base, B.lead0, P.first_off, S->up),
                    "launch k_batch_map");
        }
        HIP_TRY(hipEventRecord(G.consumed, S->up), "hipEventRecord");
        HIP_TRY(hipEventRecord(S->mapped[tb], S->up), "hipEventRecord");
        HIP_TRY(hipStreamWaitEvent(s, S->mapped[tb], 0), "hipStreamWaitEvent");
        bool timed = false;
        ZcTuner::Pending probe{};
        const int cand = tune_pick(c, B.zclass, P.blocks * kBlk, &timed, &probe);
        LaunchCfg lcs = cfg_for(c, true, cand ? kZcNone : B.zclass);
        if (B.tshift == 0) lcs.store = c->store_dense;
        if (timed) tune_mark(c, B.zclass, probe, false, s);
        hipError_t le = hipSuccess;
        for (int q = 0; q < B.nclass && le == hipSuccess; ++q) {
            const auto &C = B.cls[q];
            le = launch_batch_tiles(lcs, (uint8_t *)dst_base, C.recs, C.tshift, S->btiles[tb] + C.rec0, c->base_dev, s);
        }
        // the probe's end mark even when a launch failed: its events go back
        // to the tuner's spares instead of leaking, with no rate
        if (timed) tune_mark(c, B.zclass, probe, true, s, le == hipSuccess);
        HIP_TRY(le, "launch k_fill_batch");
        HIP_TRY(hipEventRecord(S->filled[tb], s), "hipEventRecord");
    }
    return S3DG_OK;
}
