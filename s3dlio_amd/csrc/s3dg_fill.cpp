// s3dg_fill.cpp — uniform fills and their verification: one object, a range of
// its blocks or a stream of equal objects (k_fill_stream, or the tiled batch
// kernel for large streams), k_verify_stream over the same layouts, and the
// store-only write ceilings.
#include "s3dg_ctx.h"

#include <memory>

using namespace s3dg;

namespace s3dg {

int tile_map_grow(TileRec **map, uint64_t *cap, uint64_t tiles) {
    if (*map) (void)hipFree(*map);
    *map = nullptr;
    *cap = 0;
    const uint64_t n = tiles < 4096 ? 4096 : tiles + tiles / 4;
    HIP_TRY(hipMalloc(map, n * sizeof(TileRec)), "hipMalloc(tile map)");
    *cap = n;
    return S3DG_OK;
}

// At least `tiles` records in the stream's map.  Earlier launches on this
// stream may still read the old map: growing drains the stream first.
// Caller holds S->mu.
static int tiles_reserve(StreamState *S, uint64_t tiles, hipStream_t s) {
    if (tiles <= S->tile_cap) return S3DG_OK;
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize(tile map)");
    return tile_map_grow(&S->tiles, &S->tile_cap, tiles);
}

// n_objs objects of obj_size bytes at dst + j*stride, entropy seed_base +
// ((first_obj + j) << 32), prefix parameters pp.  Large streams whose objects
// all start on the same 4 KiB granule (mod 8) run through the tiled batch
// kernel; the rest through the 2D stream kernel.
// held: the stream's state when the caller already holds it (batch sub-batches).
int fill_uniform(s3dg_ctx *c, uint8_t *dst, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                 const PrefixParams &pp, uint64_t seed_base, uint64_t first_obj, hipStream_t s, StreamState *held) {
    const uint64_t nb = obj_blocks(obj_size);
    const uint32_t lead = (uint32_t)obj_lead((uintptr_t)dst, 0);   // the batch's record rules (s3dg_batch_plan.h)
    if (c->stream_tiles && (n_objs == 1 || stride % (8 * kBlk) == 0) && n_objs * nb >= kStreamTilesMinBlocks &&
        nb + lead < (1ull << 31)) {
        uint64_t ntiles[kTileShiftMax + 1] = {};
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) ntiles[sh] = n_objs * obj_tiles(nb, lead, sh);
        const uint32_t tshift = c->tile_shift ? c->tile_shift : pick_tile_shift(ntiles);
        const uint64_t tpo = obj_tiles(nb, lead, tshift);
        std::unique_ptr<StreamLock> SL;
        if (!held) SL.reset(new StreamLock(c, s));
        StreamState *S = held ? held : SL->get();
        if (int r = tiles_reserve(S, n_objs * tpo, s)) return r;
        // the prefix's class from its exact length (pp: 4096 f_num / f_den = floor_len + rem / f_den)
        const int zc = pp.f_den == 0 || (pp.floor_len == 0 && pp.rem == 0) ? kZcNone
                       : pp.rem == 0 && (pp.floor_len & 63u) == 0      ? kZcLines
                       : 2 * (uint64_t)pp.floor_len >= kBlk            ? kZcMidHeavy
                                                                        : kZcNone;
        bool timed = false;
        ZcTuner::Pending probe{};
        const int cand = tune_pick(c, zc, obj_size * n_objs, &timed, &probe);
        if (timed) tune_mark(c, zc, probe, false, s);
        LaunchCfg lc = cfg_for(c, true, cand ? kZcNone : zc);
        if (zc == kZcNone && c->batch_rt_floor < 0 && nb >= kRtFloorLargeBlocks) lc.rt_floor = kRtFloorLargeUniform;
        const hipError_t le = launch_fill_uniform_tiles(lc, dst, obj_size, stride, n_objs, (uint32_t)tpo, tshift, lead,
                                                        seed_base + (first_obj << 32), pp, S->tiles, c->base_dev, s);
        if (timed) tune_mark(c, zc, probe, true, s, le == hipSuccess);
        HIP_TRY(le,
                "launch k_fill_batch(stream)");
        return S3DG_OK;
    }
    HIP_TRY(launch_fill_stream(cfg_for(c), dst, obj_size, stride, n_objs, 0, (uint32_t)nb, seed_base, first_obj,
                               pp, c->base_dev, s),
            "launch k_fill_stream");
    return S3DG_OK;
}

// Chunk of n_objs equal objects for the put pipeline: blocks [blk_lo, blk_hi)
// of objects first_obj..first_obj+n_objs-1, object k's block blk_lo at
// dst + k*stride; controlled layout or (random_layout) generate_random_data's.
int fill_chunk(s3dg_ctx *c, void *dst, uint64_t obj_size, uint64_t stride, uint64_t n_objs, uint64_t blk_lo,
               uint64_t blk_hi, int random_layout, uint64_t dedup, uint32_t f_num, uint32_t f_den,
               uint64_t seed_base, uint64_t first_obj, void *stream) {
    CTX_SCOPE(c);
    if (obj_size == 0 || n_objs == 0) return S3DG_OK;
    const uint64_t nb = (obj_size + kBlk - 1) / kBlk;
    if (blk_hi > nb) blk_hi = nb;
    if (blk_lo >= blk_hi) return S3DG_OK;
    if (!dst || !aligned16(dst) || (stride & 15u)) return fail(S3DG_EINVAL, "dst and stride must be 16-byte aligned");
    PrefixParams pp{};
    if (random_layout) {
        if (nb > 0xFFFFFFFFull) return fail(S3DG_EINVAL, "object larger than 2^32 blocks");
        pp = random_layout_prefix();
    } else if (int r = make_prefix(nb, dedup, f_num, f_den, &pp)) {
        return r;
    }
    HIP_TRY(launch_fill_stream(cfg_for(c), (uint8_t *)dst, obj_size, stride, n_objs, (uint32_t)blk_lo,
                               (uint32_t)blk_hi, seed_base, first_obj, pp, c->base_dev, (hipStream_t)stream),
            "launch k_fill_stream(put chunk)");
    return S3DG_OK;
}

}  // namespace s3dg

extern "C" {

int s3dg_fill_controlled_range(s3dg_ctx *c, void *dst, uint64_t len, uint64_t blk_lo,
                               uint64_t blk_hi, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                               uint64_t entropy, void *stream) {
    CTX_SCOPE(c);
    if (len == 0) return S3DG_OK;                                   // :154-156
    const uint64_t nb = (len + kBlk - 1) / kBlk;
    if (blk_hi > nb) blk_hi = nb;
    if (blk_lo >= blk_hi) return S3DG_OK;
    if (!dst || !aligned16(dst)) return fail(S3DG_EINVAL, "dst must be a 16-byte aligned device pointer");
    // a whole large buffer is a one-object stream: the tiled kernel (entropy
    // of stream object 0 with seed_base = entropy is entropy itself)
    if (blk_lo == 0 && blk_hi == nb && c->stream_tiles && nb >= kStreamTilesMinBlocks)
        return s3dg_fill_controlled_stream(c, dst, len, (len + 15) & ~15ull, 1, dedup, f_num, f_den, entropy, 0,
                                           stream);
    PrefixParams pp;
    if (int r = make_prefix(nb, dedup, f_num, f_den, &pp)) return r;
    HIP_TRY(launch_fill_stream(cfg_for(c), (uint8_t *)dst, len, 0, 1, (uint32_t)blk_lo,
                               (uint32_t)blk_hi, entropy, 0, pp, c->base_dev,
                               (hipStream_t)stream),
            "launch k_fill_stream");
    return S3DG_OK;
}

int s3dg_random_data(s3dg_ctx *c, void *dst, uint64_t len, uint64_t entropy, void *stream) {
    CTX_SCOPE(c);
    if (len == 0) return S3DG_OK;
    if (!dst || !aligned16(dst)) return fail(S3DG_EINVAL, "dst must be a 16-byte aligned device pointer");
    const uint64_t nb = (len + kBlk - 1) / kBlk;
    if (nb > 0xFFFFFFFFull) return fail(S3DG_EINVAL, "object larger than 2^32 blocks");
    const PrefixParams pp = random_layout_prefix();
    return fill_uniform(c, (uint8_t *)dst, len, (len + 15) & ~15ull, 1, pp, entropy, 0, (hipStream_t)stream);
}

int s3dg_fill_controlled(s3dg_ctx *c, void *dst, uint64_t len, uint64_t dedup, uint32_t f_num,
                         uint32_t f_den, uint64_t entropy, void *stream) {
    return s3dg_fill_controlled_range(c, dst, len, 0, ~0ull, dedup, f_num, f_den, entropy, stream);
}

int s3dg_fill_controlled_stream(s3dg_ctx *c, void *dst, uint64_t obj_size, uint64_t stride,
                                uint64_t n_objs, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                                uint64_t seed_base, uint64_t first_obj, void *stream) {
    CTX_SCOPE(c);
    if (obj_size == 0 || n_objs == 0) return S3DG_OK;
    if (!dst || !aligned16(dst) || (stride & 15u))
        return fail(S3DG_EINVAL, "dst and stride must be 16-byte aligned");
    if (n_objs > 1 && stride < obj_size) return fail(S3DG_EINVAL, "stride < obj_size: objects overlap");
    const uint64_t nb = (obj_size + kBlk - 1) / kBlk;
    PrefixParams pp;
    if (int r = make_prefix(nb, dedup, f_num, f_den, &pp)) return r;
    return fill_uniform(c, (uint8_t *)dst, obj_size, stride, n_objs, pp, seed_base, first_obj, (hipStream_t)stream);
}

// ---- verification (k_verify_stream) -------------------------------------------
}  // extern "C"

namespace s3dg {

// One call: a result record of its own (from the context's idle list, so two
// threads on two streams never share one), reset on the stream, the launch,
// the record copied back, the stream drained.
int verify_with_record(s3dg_ctx *c, hipStream_t s, const char *launch_what,
                       const std::function<hipError_t(VerifyRec *)> &launch, s3dg_verify_result *out) {
    VerifyRec *rec = nullptr;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->vrecs.empty()) {
            rec = c->vrecs.back();
            c->vrecs.pop_back();
        }
    }
    if (!rec) HIP_TRY(hipMalloc((void **)&rec, sizeof(VerifyRec)), "hipMalloc(verify record)");
    VerifyRec host{0, 0, UINT64_MAX};
    hipError_t e = verify_rec_reset(rec, s);
    const char *what = "hipMemsetAsync(verify record)";
    if (e == hipSuccess) {
        e = launch(rec);
        what = launch_what;
    }
    if (e == hipSuccess) {
        e = hipMemcpyAsync(&host, rec, sizeof(host), hipMemcpyDeviceToHost, s);
        what = "hipMemcpyAsync(verify record)";
    }
    // drained on every path: the record goes back to the list only when idle
    const hipError_t se = hipStreamSynchronize(s);
    if (e == hipSuccess && se != hipSuccess) {
        e = se;
        what = "hipStreamSynchronize(verify)";
    }
    if (se == hipSuccess) {
        std::lock_guard<std::mutex> g(c->mu);
        c->vrecs.push_back(rec);
    }
    HIP_TRY(e, what);
    out->mismatched_bytes = host.bytes;
    out->mismatched_blocks = host.blocks;
    out->first_offset = host.first;
    return S3DG_OK;
}

}  // namespace s3dg

extern "C" {

static int verify_run(s3dg_ctx *c, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                      uint64_t blk_lo, uint64_t blk_hi, uint64_t seed_base, uint64_t first_obj,
                      const PrefixParams &pp, hipStream_t s, s3dg_verify_result *out) {
    return verify_with_record(c, s, "launch k_verify_stream", [&](VerifyRec *rec) {
        return launch_verify_stream(cfg_for(c), (const uint8_t *)src, obj_size, stride, n_objs, (uint32_t)blk_lo,
                                    (uint32_t)blk_hi, seed_base, first_obj, pp, c->base_dev, 0, rec, s);
    }, out);
}

static void verify_clean(s3dg_verify_result *out) {
    out->mismatched_bytes = 0;
    out->mismatched_blocks = 0;
    out->first_offset = UINT64_MAX;
}

int s3dg_verify_controlled_range(s3dg_ctx *c, const void *src, uint64_t len, uint64_t blk_lo, uint64_t blk_hi,
                                 uint64_t dedup, uint32_t f_num, uint32_t f_den, uint64_t entropy, void *stream,
                                 s3dg_verify_result *out) {
    CTX_SCOPE(c);
    if (!out) return fail(S3DG_EINVAL, "null output");
    verify_clean(out);
    if (len == 0) return S3DG_OK;
    const uint64_t nb = (len + kBlk - 1) / kBlk;
    if (blk_hi > nb) blk_hi = nb;
    if (blk_lo >= blk_hi) return S3DG_OK;
    if (!src || !aligned16(src)) return fail(S3DG_EINVAL, "src must be a 16-byte aligned device pointer");
    PrefixParams pp;
    if (int r = make_prefix(nb, dedup, f_num, f_den, &pp)) return r;
    return verify_run(c, src, len, 0, 1, blk_lo, blk_hi, entropy, 0, pp, (hipStream_t)stream, out);
}

int s3dg_verify_controlled(s3dg_ctx *c, const void *src, uint64_t len, uint64_t dedup, uint32_t f_num,
                           uint32_t f_den, uint64_t entropy, void *stream, s3dg_verify_result *out) {
    return s3dg_verify_controlled_range(c, src, len, 0, ~0ull, dedup, f_num, f_den, entropy, stream, out);
}

int s3dg_verify_random_data(s3dg_ctx *c, const void *src, uint64_t len, uint64_t entropy, void *stream,
                            s3dg_verify_result *out) {
    CTX_SCOPE(c);
    if (!out) return fail(S3DG_EINVAL, "null output");
    verify_clean(out);
    if (len == 0) return S3DG_OK;
    if (!src || !aligned16(src)) return fail(S3DG_EINVAL, "src must be a 16-byte aligned device pointer");
    const uint64_t nb = (len + kBlk - 1) / kBlk;
    if (nb > 0xFFFFFFFFull) return fail(S3DG_EINVAL, "object larger than 2^32 blocks");
    return verify_run(c, src, len, 0, 1, 0, nb, entropy, 0, random_layout_prefix(), (hipStream_t)stream, out);
}

int s3dg_verify_controlled_stream(s3dg_ctx *c, const void *src, uint64_t obj_size, uint64_t stride,
                                  uint64_t n_objs, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                                  uint64_t seed_base, uint64_t first_obj, void *stream, s3dg_verify_result *out) {
    CTX_SCOPE(c);
    if (!out) return fail(S3DG_EINVAL, "null output");
    verify_clean(out);
    if (obj_size == 0 || n_objs == 0) return S3DG_OK;
    if (!src || !aligned16(src) || (stride & 15u))
        return fail(S3DG_EINVAL, "src and stride must be 16-byte aligned");
    if (n_objs > 1 && stride < obj_size) return fail(S3DG_EINVAL, "stride < obj_size: objects overlap");
    const uint64_t nb = (obj_size + kBlk - 1) / kBlk;
    PrefixParams pp;
    if (int r = make_prefix(nb, dedup, f_num, f_den, &pp)) return r;
    return verify_run(c, src, obj_size, stride, n_objs, 0, nb, seed_base, first_obj, pp, (hipStream_t)stream, out);
}

int s3dg_write_ceiling(s3dg_ctx *c, void *dst, uint64_t len, uint32_t pattern, void *stream) {
    CTX_SCOPE(c);
    if (!dst || !aligned16(dst) || (len % kBlk))
        return fail(S3DG_EINVAL, "dst must be 16-byte aligned and len a multiple of 4096");
    HIP_TRY(launch_write_ceiling(cfg_for(c), (uint8_t *)dst, len, pattern, nullptr, 0, (hipStream_t)stream),
            "launch k_write_ceiling");
    return S3DG_OK;
}

int s3dg_write_ceiling_tiled(s3dg_ctx *c, void *dst, uint64_t len, uint32_t pattern, void *stream) {
    CTX_SCOPE(c);
    if (!dst || !aligned16(dst) || (len % kBlk))
        return fail(S3DG_EINVAL, "dst must be 16-byte aligned and len a multiple of 4096");
    if (len == 0) return S3DG_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t nthr = (len / kBlk + 63) / 64;
    StreamLock SL(c, s);
    StreamState *S = SL.get();
    if (int r = tiles_reserve(S, nthr, s)) return r;
    HIP_TRY(launch_write_ceiling(cfg_for(c, true), (uint8_t *)dst, len, pattern, S->tiles, nthr, s),
            "launch k_write_ceiling(tiled)");
    return S3DG_OK;
}

int s3dg_write_ceiling_fill(s3dg_ctx *c, void *dst, uint64_t len, uint32_t pace, void *stream) {
    CTX_SCOPE(c);
    if (!dst || !aligned16(dst) || (len % kBlk))
        return fail(S3DG_EINVAL, "dst must be 16-byte aligned and len a multiple of 4096");
    if (len == 0) return S3DG_OK;
    hipStream_t s = (hipStream_t)stream;
    // the tiled fill's launch for len bytes as 8 MiB objects (d1 c1 prefix
    // parameters; one object when len < 8 MiB)
    constexpr uint64_t kObj = 8ull << 20;
    if (len > kObj && len % kObj) return fail(S3DG_EINVAL, "len must be < 8 MiB or a multiple of 8 MiB");
    const uint64_t n_objs = (len + kObj - 1) / kObj;
    const uint64_t obj = len < kObj ? len : kObj;
    PrefixParams pp;
    if (int r = make_prefix(obj / kBlk, 1, 0, 1, &pp)) return r;
    const uint32_t lead = (uint32_t)(((uintptr_t)dst >> 12) & 7);
    const uint32_t tshift = kTileShiftMax;
    const uint64_t tpo = (obj / kBlk + lead + (1ull << tshift) - 1) >> tshift;
    StreamLock SL(c, s);
    StreamState *S = SL.get();
    if (int r = tiles_reserve(S, n_objs * tpo, s)) return r;
    LaunchCfg lc = cfg_for(c, true);
    lc.pace = pace;
    HIP_TRY(launch_fill_uniform_tiles(lc, (uint8_t *)dst, obj, kObj, n_objs, (uint32_t)tpo, tshift, lead, 0, pp,
                                      S->tiles, c->base_dev, s, true),
            "launch k_fill_batch(ablated)");
    return S3DG_OK;
}

}  // extern "C"
