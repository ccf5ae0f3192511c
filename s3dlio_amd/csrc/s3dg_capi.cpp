// s3dg_capi.cpp — C ABI (include/s3dlio_gpu.h) over the gfx950 kernels.
//
// Host-side parameter math follows the reference's src/data_gen.rs:151-224:
// unique_blocks (:162-167), (f_num, f_den) (:169-173), floor_len/rem
// (:174-175).  No CPU generation path exists in this library: every byte is
// produced by a HIP kernel, and a missing/failed GPU is an error.
#include "s3dg_ctx.h"

#include <cmath>
#include <cstring>

using namespace s3dg;

namespace {

thread_local std::string g_err;

// SmallRng seeding + Xoshiro256++ on the host, only to derive a base block
// from a seed (4 KiB, once per set call).
uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
void base_from_seed(uint64_t seed, uint8_t *out) {
    uint64_t x = seed, s[4];
    for (int k = 0; k < 4; ++k) {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        s[k] = z ^ (z >> 31);
    }
    for (uint32_t off = 0; off < kBlk; off += 8) {
        const uint64_t r = rotl(s[0] + s[3], 23) + s[0];
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t;
        s[3] = rotl(s[3], 45);
        std::memcpy(out + off, &r, 8);   // little-endian host
    }
}

constexpr uint64_t kDefaultBaseSeed = 0xBA5EB10C00000000ull;

}  // namespace

namespace s3dg {

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int hipfail(hipError_t e, const char *what) {
    return fail(S3DG_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// zclass: the launch's zero-prefix class (zero_class; batches: the class of
// most of its blocks); picks the batch kernel's occupancy cap and store floor
// when they are not set explicitly (s3dg_set_occupancy, s3dg_set_batch_pace).
LaunchCfg cfg_for(s3dg_ctx *c, bool batch, int zclass) {
    LaunchCfg lc;
    lc.store = batch ? c->store_batch : c->store_stream;
    lc.waves_per_block = c->waves_per_block ? c->waves_per_block : (batch ? 1 : 2);
    const int occ = !batch ? c->occ_stream : c->occ_batch >= 0 ? c->occ_batch
                                           : zclass == kZcLines ? kOccZeroLines : 0;
    lc.dyn_lds = occupancy_lds(occ, kFillStaticLds);
    if (batch)
        lc.rt_floor = c->batch_rt_floor >= 0 ? (uint32_t)c->batch_rt_floor
                                             : zclass == kZcMidHeavy ? kRtFloorMidZeros : 0u;
    lc.prefetch_tiles = batch ? c->prefetch_tiles : 0;
    return lc;
}

int make_prefix(uint64_t nblocks, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                PrefixParams *pp) {
    if (f_den == 0) return fail(S3DG_EINVAL, "f_den must be >= 1");
    if (f_num >= f_den) return fail(S3DG_EINVAL, "f_num must be < f_den (zero ratio < 1)");
    if (nblocks > 0xFFFFFFFFull) return fail(S3DG_EINVAL, "object larger than 2^32 blocks");
    *pp = prefix_params(nblocks, dedup, f_num, f_den);   // s3dg_prefix.h: the device's function too
    return S3DG_OK;
}

PrefixParams random_layout_prefix() {
    PrefixParams pp{};
    pp.unique = 0xFFFFFFFFu;            // block i seeded entropy + i
    pp.f_den = 0;                       // generate_random_data layout
    pp.m_unique = fastmod_magic(1);
    pp.m_fden = fastmod_magic(1);
    return pp;
}

LaunchCfg ctx_stream_cfg(const s3dg_ctx *c) { return cfg_for(const_cast<s3dg_ctx *>(c)); }
const void *ctx_base(const s3dg_ctx *c) { return c->base_dev; }

// Frees one stream's launch state; the caller has drained the stream (and
// its upload stream).
void stream_state_free(StreamState *S) {
    if (S->tiles) (void)hipFree(S->tiles);
    for (int q = 0; q < 2; ++q) {
        if (S->btiles[q]) (void)hipFree(S->btiles[q]);
        if (S->mapped[q]) (void)hipEventDestroy(S->mapped[q]);
        if (S->filled[q]) (void)hipEventDestroy(S->filled[q]);
    }
    for (auto &G : S->stage) {
        if (G.host) (void)hipHostFree(G.host);
        for (void *p : {(void *)G.dev, (void *)G.rec_lo, G.scan_tmp})
            if (p) (void)hipFree(p);
        if (G.uploaded) (void)hipEventDestroy(G.uploaded);
        if (G.consumed) (void)hipEventDestroy(G.consumed);
    }
    if (S->up) (void)hipStreamDestroy(S->up);
    if (S->zs) (void)hipStreamDestroy(S->zs);
    for (hipEvent_t e : {S->zfork, S->zjoin})
        if (e) (void)hipEventDestroy(e);
    if (S->ks.dev) (void)hipFree(S->ks.dev);
    if (S->vobj) (void)hipFree(S->vobj);
    for (auto &T : S->dtab) {
        if (T.host) (void)hipHostFree(T.host);
        if (T.dev) (void)hipFree(T.dev);
        if (T.uploaded) (void)hipEventDestroy(T.uploaded);
    }
    for (auto &T : S->ctab) {
        if (T.host) (void)hipHostFree(T.host);
        if (T.dev) (void)hipFree(T.dev);
        if (T.uploaded) (void)hipEventDestroy(T.uploaded);
    }
    if (S->crc_out) (void)hipFree(S->crc_out);
    for (auto &T : S->ttab) {
        if (T.host) (void)hipHostFree(T.host);
        if (T.dev) (void)hipFree(T.dev);
        if (T.uploaded) (void)hipEventDestroy(T.uploaded);
    }
    if (S->tfr_out) (void)hipFree(S->tfr_out);
    delete S;
}

// The context's device (callers make it current with a DeviceScope).
int ctx_device(s3dg_ctx *c, int *dev) {
    if (!c || !dev) return fail(S3DG_EINVAL, "null context");
    *dev = c->device;
    return S3DG_OK;
}

}  // namespace s3dg

extern "C" {

const char *s3dg_last_error(void) { return g_err.c_str(); }
const char *s3dg_version(void) { return "s3dlio_amd 0.1.0 (gfx950)"; }

// The source digest this library was built from (build.py compiles it in;
// the marker lets build.py read it from the file without loading it).
#ifndef S3DG_BUILD_DIGEST
#define S3DG_BUILD_DIGEST "unknown-digest00"
#endif
static const char kBuildDigestRecord[] __attribute__((used)) = "S3DG_BUILD_DIGEST=" S3DG_BUILD_DIGEST;
const char *s3dg_build_digest(void) { return kBuildDigestRecord + sizeof("S3DG_BUILD_DIGEST=") - 1; }

uint64_t s3dg_unique_blocks(uint64_t nblocks, uint64_t dedup) {
    return unique_blocks(nblocks, dedup);
}

int s3dg_zero_class(uint32_t f_num, uint32_t f_den) { return zero_class(f_num, f_den); }

int s3dg_compress_ratio(uint64_t compress, uint32_t *f_num, uint32_t *f_den) {
    if (!f_num || !f_den) return fail(S3DG_EINVAL, "null output");
    if (compress > 0xFFFFFFFFull) return fail(S3DG_EINVAL, "compress must fit in 32 bits");
    if (compress > 1) { *f_num = (uint32_t)(compress - 1); *f_den = (uint32_t)compress; }
    else { *f_num = 0; *f_den = 1; }
    return S3DG_OK;
}

uint64_t s3dg_object_entropy(uint64_t seed_base, uint64_t j) { return seed_base + (j << 32); }

int s3dg_device_count(int *out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    HIP_TRY(hipGetDeviceCount(out), "hipGetDeviceCount");
    return S3DG_OK;
}

int s3dg_ctx_create(int device, s3dg_ctx **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n), "hipGetDeviceCount");
    if (device < 0 || device >= n) return fail(S3DG_EINVAL, "device index out of range");
    DeviceScope ds(device);
    if (!ds.ok()) return hipfail(ds.err, "hipSetDevice");
    s3dg_ctx *c = new s3dg_ctx();
    c->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        c->cus = cus;
    hipError_t e = hipMalloc(&c->base_dev, kBlk);
    if (e != hipSuccess) { delete c; return hipfail(e, "hipMalloc(base block)"); }
    base_from_seed(kDefaultBaseSeed, c->base_host);
    e = hipMemcpy(c->base_dev, c->base_host, kBlk, hipMemcpyHostToDevice);
    if (e != hipSuccess) { s3dg_ctx_destroy(c); return hipfail(e, "hipMemcpy(base block)"); }
    *out = c;
    return S3DG_OK;
}

int s3dg_ctx_destroy(s3dg_ctx *c) {
    if (!c) return S3DG_OK;
    DeviceScope ds(c->device);
    (void)hipDeviceSynchronize();
    if (c->base_dev) (void)hipFree(c->base_dev);
    for (auto &kv : c->streams) stream_state_free(kv.second);
    for (auto &kv : c->jtabs) (void)hipFree(kv.second);
    if (c->crc_tab) (void)hipFree(c->crc_tab);
    if (c->crc_seg) (void)hipFree(c->crc_seg);
    for (VerifyRec *r : c->vrecs) (void)hipFree(r);
    for (auto &T : c->tune) {
        for (auto &p : T.pend) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
        for (auto e : T.spare) (void)hipEventDestroy(e);
    }
    delete c;
    return S3DG_OK;
}

// a context keeps tile maps and batch staging per stream it has
// seen; a caller that retires a stream releases them here (after draining
// the stream), so short-lived streams do not accumulate device memory and a
// reused handle value starts from fresh state.
int s3dg_stream_release(s3dg_ctx *c, void *stream) {
    CTX_SCOPE(c);
    StreamState *S = nullptr;
    {
        std::lock_guard<std::mutex> g(c->mu);
        auto it = c->streams.find((hipStream_t)stream);
        if (it == c->streams.end()) return S3DG_OK;
        S = it->second;
        c->streams.erase(it);
        S->dead = true;
        ++S->refs;                               // held by this release until the drain below
    }
    hipError_t e;
    {
        std::lock_guard<std::mutex> g(S->mu);    // wait for an enqueue in progress
        e = hipStreamSynchronize((hipStream_t)stream);
        if (e == hipSuccess && S->up) e = hipStreamSynchronize(S->up);
        if (e == hipSuccess && S->zs) e = hipStreamSynchronize(S->zs);
    }
    bool last;
    {
        std::lock_guard<std::mutex> g(c->mu);
        last = --S->refs == 0;
    }
    if (last) stream_state_free(S);              // else the last holder drains and frees it (StreamLock)
    HIP_TRY(e, "hipStreamSynchronize(release)");
    return S3DG_OK;
}

// Streams with launch state in this context (diagnostics and tests).
int s3dg_stream_state_count(s3dg_ctx *c, uint64_t *n) {
    if (!c || !n) return fail(S3DG_EINVAL, "bad argument");
    std::lock_guard<std::mutex> g(c->mu);
    *n = c->streams.size();
    return S3DG_OK;
}

int s3dg_ctx_device(s3dg_ctx *c, int *device) {
    if (!c || !device) return fail(S3DG_EINVAL, "null argument");
    *device = c->device;
    return S3DG_OK;
}

int s3dg_set_base_block(s3dg_ctx *c, const uint8_t *base) {
    CTX_SCOPE(c);
    if (!base) return fail(S3DG_EINVAL, "null base block");
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");   // no launch may read the old block
    std::memcpy(c->base_host, base, kBlk);
    HIP_TRY(hipMemcpy(c->base_dev, c->base_host, kBlk, hipMemcpyHostToDevice), "hipMemcpy(base)");
    return S3DG_OK;
}

int s3dg_set_base_block_seed(s3dg_ctx *c, uint64_t seed) {
    uint8_t b[kBlk];
    base_from_seed(seed, b);
    return s3dg_set_base_block(c, b);
}

int s3dg_get_base_block(s3dg_ctx *c, uint8_t *out) {
    if (!c || !out) return fail(S3DG_EINVAL, "null argument");
    std::memcpy(out, c->base_host, kBlk);
    return S3DG_OK;
}

int s3dg_set_waves_per_block(s3dg_ctx *c, int waves) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    if (waves != 0 && waves != 1 && waves != 2 && waves != 4) return fail(S3DG_EINVAL, "waves per block must be 1, 2 or 4");
    c->waves_per_block = waves;
    return S3DG_OK;
}

int s3dg_set_nontemporal(s3dg_ctx *c, int on) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    c->store_stream = on ? kStoreNT : kDefaultStoreStream;
    c->store_batch = on ? kStoreNT : kDefaultStoreBatch;
    c->store_dense = on ? kStoreNT : kDefaultStoreDense;
    return S3DG_OK;
}

int s3dg_set_store_policy(s3dg_ctx *c, int stream_policy, int batch_policy) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    if (stream_policy > kStoreNTSC1 || batch_policy > kStoreNTSC1)
        return fail(S3DG_EINVAL, "store policy must be 0 (plain), 1 (nt), 2 (sc1), 3 (nt sc1) or negative (default)");
    c->store_stream = stream_policy < 0 ? kDefaultStoreStream : stream_policy;
    c->store_batch = batch_policy < 0 ? kDefaultStoreBatch : batch_policy;
    c->store_dense = batch_policy < 0 ? kDefaultStoreDense : batch_policy;
    return S3DG_OK;
}

int s3dg_set_occupancy(s3dg_ctx *c, int stream_wgs_per_cu, int batch_wgs_per_cu) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    if (stream_wgs_per_cu > 40 || batch_wgs_per_cu > 40)
        return fail(S3DG_EINVAL, "workgroups per CU must be at most 40");
    c->occ_stream = stream_wgs_per_cu < 0 ? kDefaultOccStream : stream_wgs_per_cu;
    c->occ_batch = batch_wgs_per_cu < 0 ? kDefaultOccBatch : batch_wgs_per_cu;
    return S3DG_OK;
}

int s3dg_set_batch_pace(s3dg_ctx *c, int ticks) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    if (ticks > 100000) return fail(S3DG_EINVAL, "store floor must be at most 100000 ticks (1 ms)");
    c->batch_rt_floor = ticks < 0 ? kDefaultBatchRtFloor : ticks;
    return S3DG_OK;
}

int s3dg_set_batch_prefetch(s3dg_ctx *c, uint32_t tiles) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    c->prefetch_tiles = tiles == UINT32_MAX ? kDefaultPrefetch : tiles;
    return S3DG_OK;
}

int s3dg_set_batch_tile(s3dg_ctx *c, uint32_t blocks) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    uint32_t sh = 0;
    if (blocks > 1) {
        while ((1u << sh) < blocks) ++sh;
        if ((1u << sh) != blocks || sh < kTileShiftMin || sh > kTileShiftMax)
            return fail(S3DG_EINVAL, "tile blocks must be 0 (per launch), 1 (dense), 2, 4, 8, 16, 32 or 64");
    }
    c->tile_shift = sh;
    c->tile_force_dense = blocks == 1;
    return S3DG_OK;
}

int s3dg_set_batch_split(s3dg_ctx *c, int blocks) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    c->split_blocks = blocks < 0 ? kDefaultSplitBlocks : (uint32_t)blocks;
    return S3DG_OK;
}

int s3dg_set_keystream_shape(s3dg_ctx *c, int mode, int draws, int waves, int wgs_per_cu,
                             uint64_t min_lane_draws, int store_policy) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    if (mode != 0 && mode != 1) return fail(S3DG_EINVAL, "mode must be 0 (keystream) or 1 (dgen)");
    if (draws != 0 && draws != 16 && draws != 32 && draws != 64)
        return fail(S3DG_EINVAL, "draws per stage must be 16, 32 or 64");
    if (waves != 0 && waves != 1 && waves != 2 && waves != 4) return fail(S3DG_EINVAL, "waves must be 1, 2 or 4");
    if (wgs_per_cu < 0 || wgs_per_cu > 40) return fail(S3DG_EINVAL, "workgroups per CU must be 0..40");
    if (min_lane_draws != 0 && min_lane_draws < 64) return fail(S3DG_EINVAL, "min_lane_draws must be >= 64");
    if (store_policy > kStoreNTSC1) return fail(S3DG_EINVAL, "store policy must be 0, 1, 2, 3 or negative");
    std::lock_guard<std::mutex> g(c->mu);
    const KsShape &def = kDefaultKsShape[mode];
    c->ks[mode].draws = draws ? draws : def.draws;
    c->ks[mode].waves = waves ? waves : def.waves;
    c->ks_auto_waves[mode] = waves == 0;
    c->ks[mode].wgs_per_cu = wgs_per_cu;
    c->ks[mode].store = store_policy < 0 ? def.store : store_policy;
    c->ks_min_draws[mode] = min_lane_draws ? min_lane_draws : kDefaultKsMinDraws[mode];
    return S3DG_OK;
}

int s3dg_set_keystream_xcd_group(s3dg_ctx *c, int mode, uint32_t waves) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    if (mode != 0 && mode != 1) return fail(S3DG_EINVAL, "mode must be 0 (keystream) or 1 (dgen)");
    if (waves > 4096 || (waves & (waves - 1))) return fail(S3DG_EINVAL, "waves per XCD group must be 0 or a power of two <= 4096");
    std::lock_guard<std::mutex> g(c->mu);
    c->ks[mode].xcd_waves = waves ? (int)waves : kDefaultKsXcdWaves;
    c->ks_auto_xcd[mode] = waves == 0;
    return S3DG_OK;
}

int s3dg_set_keystream_persist(s3dg_ctx *c, int rounds) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    std::lock_guard<std::mutex> g(c->mu);
    c->ks_persist = rounds < 0 ? -1 : rounds;
    return S3DG_OK;
}

int s3dg_set_dgen_zero_split(s3dg_ctx *c, int chunks, int waves, int occupancy, int store, int overlap) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    if (waves != 0 && waves != 1 && waves != 2 && waves != 4 && waves >= 0)
        return fail(S3DG_EINVAL, "waves must be 1, 2 or 4 (0 or negative: default)");
    if (occupancy > 64) return fail(S3DG_EINVAL, "occupancy must be <= 64 workgroups per CU");
    if (store > kStoreNTSC1) return fail(S3DG_EINVAL, "store policy must be 0, 1, 2, 3 or negative");
    std::lock_guard<std::mutex> g(c->mu);
    c->dgen_zero_split = chunks < 0 ? kDefaultDgenZeroSplit : (uint64_t)chunks;
    c->zp_waves = waves <= 0 ? -1 : waves;
    c->zp_occ = occupancy < 0 ? -1 : occupancy;
    c->zp_store = store < 0 ? -1 : store;
    c->zp_overlap = overlap < 0 ? -1 : (overlap ? 1 : 0);
    return S3DG_OK;
}

int s3dg_set_keystream_tail(s3dg_ctx *c, int chunks) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    std::lock_guard<std::mutex> g(c->mu);
    c->ks_tail = chunks < 0 ? -1 : chunks;
    return S3DG_OK;
}

int s3dg_query_keystream_occupancy(s3dg_ctx *c, int mode, int *wgs_per_cu) {
    CTX_SCOPE(c);
    if (!wgs_per_cu || (mode != 0 && mode != 1)) return fail(S3DG_EINVAL, "bad argument");
    HIP_TRY(keystream_occupancy(c->ks[mode], wgs_per_cu), "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    return S3DG_OK;
}

int s3dg_query_occupancy(s3dg_ctx *c, int batch, int *wgs_per_cu) {
    CTX_SCOPE(c);
    if (!wgs_per_cu) return fail(S3DG_EINVAL, "null output");
    HIP_TRY(fill_occupancy(cfg_for(c, batch != 0, batch == 2 ? kZcLines : kZcNone), batch != 0, wgs_per_cu),
            "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    return S3DG_OK;
}

int s3dg_set_stream_tiles(s3dg_ctx *c, int on) {
    if (!c) return fail(S3DG_EINVAL, "null context");
    c->stream_tiles = on < 0 ? kDefaultStreamTiles : (on != 0);
    return S3DG_OK;
}

int s3dg_crc32(s3dg_ctx *c, const void *dev, uint64_t len, void *stream, uint32_t *out) {
    CTX_SCOPE(c);
    if (!out || (len && !dev)) return fail(S3DG_EINVAL, "null argument");
    if (len && !aligned16(dev)) return fail(S3DG_EINVAL, "dev must be 16-byte aligned");
    std::lock_guard<std::mutex> g(c->crc_mu);
    HIP_TRY(crc32_device((const uint8_t *)dev, len, (hipStream_t)stream, out, &c->crc_tab, &c->crc_seg,
                         &c->crc_seg_cap),
            "crc32 kernel");
    return S3DG_OK;
}

uint32_t s3dg_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
    return crc32_combine(crc1, crc2, len2);
}

uint32_t s3dg_crc32_host(uint32_t crc, const uint8_t *p, uint64_t n) {
    return crc32_host_update(crc, p, n);
}

int s3dg_device_alloc(s3dg_ctx *c, uint64_t bytes, void **out) {
    CTX_SCOPE(c);
    if (!out) return fail(S3DG_EINVAL, "null output");
    HIP_TRY(hipMalloc(out, bytes), "hipMalloc");
    return S3DG_OK;
}

int s3dg_device_free(s3dg_ctx *c, void *p) {
    CTX_SCOPE(c);
    HIP_TRY(hipFree(p), "hipFree");
    return S3DG_OK;
}

int s3dg_host_alloc_pinned(uint64_t bytes, void **out) {
    if (!out) return fail(S3DG_EINVAL, "null output");
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault), "hipHostMalloc");
    pinned_register(*out, bytes);   // kernels may store into it directly (s3dg_host.cpp small calls)
    return S3DG_OK;
}

int s3dg_host_free_pinned(void *p) {
    pinned_unregister(p);
    HIP_TRY(hipHostFree(p), "hipHostFree");
    return S3DG_OK;
}

int s3dg_d2h_async(s3dg_ctx *c, void *host, const void *dev, uint64_t len, void *stream) {
    CTX_SCOPE(c);
    HIP_TRY(hipMemcpyAsync(host, dev, len, hipMemcpyDeviceToHost, (hipStream_t)stream),
            "hipMemcpyAsync(D2H)");
    return S3DG_OK;
}

int s3dg_h2d_async(s3dg_ctx *c, void *dev, const void *host, uint64_t len, void *stream) {
    CTX_SCOPE(c);
    HIP_TRY(hipMemcpyAsync(dev, host, len, hipMemcpyHostToDevice, (hipStream_t)stream),
            "hipMemcpyAsync(H2D)");
    return S3DG_OK;
}

int s3dg_stream_create(s3dg_ctx *c, void **out) {
    CTX_SCOPE(c);
    if (!out) return fail(S3DG_EINVAL, "null output");
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
    *out = (void *)s;
    return S3DG_OK;
}

int s3dg_stream_destroy(s3dg_ctx *c, void *stream) {
    CTX_SCOPE(c);
    const int r = s3dg_stream_release(c, stream);
    std::string first = r ? s3dg_last_error() : "";
    const hipError_t e = hipStreamDestroy((hipStream_t)stream);   // even when the drain failed
    if (r) return fail(r, first.c_str());
    HIP_TRY(e, "hipStreamDestroy");
    return S3DG_OK;
}

int s3dg_sync(s3dg_ctx *c, void *stream) {
    CTX_SCOPE(c);
    if (stream) HIP_TRY(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    else HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
    return S3DG_OK;
}

}  // extern "C"

extern "C" int s3dg_internal_fail(int code, const char *msg) { return fail(code, msg); }
