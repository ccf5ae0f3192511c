// s3dg_keystream.cpp — the keystream generators over k_keystream: the K2
// keystream of the npz payload (s3dg_xoshiro_fill) and DG1, the dgen-contract
// generator in 1 MiB blocks.
#include "s3dg_ctx.h"
#include "s3dg_jump.h"
#include "s3dg_ks_verify_plan.h"

using namespace s3dg;

// lanes per chunk + draws per lane for a chunk size; jump table cached per ctx
// The device jump table of lanes sub < lpc starting at draws z0 + sub*span
// (cached per context): jtab[sub] = x^(z0 + sub*span) mod P.
int s3dg::jump_table(s3dg_ctx *c, uint32_t lpc, uint64_t span, uint64_t z0, const uint64_t **jtab) {
    std::lock_guard<std::mutex> g(c->mu);
    const std::pair<uint64_t, uint64_t> key{((uint64_t)lpc << 32) | span, z0};
    auto it = c->jtabs.find(key);
    if (it == c->jtabs.end()) {
        // x^(z0 + k*span) = x^(z0 + (k-1)*span) * x^span: one product mod P
        // per lane (a 512-lane table in ~5 ms on the host; round 4 raised a
        // power per lane with bit-wise products, 3 ms each: ~1.6 s on the
        // first small-object DG1 or K2 call of a context)
        std::vector<uint64_t> h(4 * (size_t)lpc, 0);
        uint64_t S[4];
        if (!jump_poly(z0, &h[0]) || !jump_poly(span, S))
            return fail(S3DG_EINVAL, "xoshiro characteristic polynomial unavailable");
        for (uint32_t k = 1; k < lpc; ++k) jump_mul(&h[4 * (k - 1)], S, &h[4 * k]);
        uint64_t *d = nullptr;
        HIP_TRY(hipMalloc(&d, h.size() * 8), "hipMalloc(jump table)");
        HIP_TRY(hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice), "hipMemcpy(jump table)");
        it = c->jtabs.emplace(key, d).first;
    }
    *jtab = it->second;
    return S3DG_OK;
}

// z0 > 0: the lanes cover draws [z0, chunk_bytes / 8) of every chunk (the
// tails of a DG1 zero-prefix split), one wave per tail when it has >= 64 x 256 draws.
static int keystream_plan(s3dg_ctx *c, int mode, uint64_t chunk_bytes, uint64_t nchunks, bool zero_prefix,
                          KeystreamArgs &A, const uint64_t **jtab, uint64_t z0 = 0) {
    // the rules: ks_lanes (s3dg_ks_plan.h); a lane stages ks[mode].draws draws per iteration
    const KsLanes L = ks_lanes(mode, chunk_bytes, nchunks, zero_prefix, z0, c->ks_min_draws[mode],
                               (uint64_t)c->ks[mode].draws, (uint64_t)c->cus);
    if (!L.ok) return fail(S3DG_EINVAL, "chunk too large");
    A.lpc = L.lpc;
    A.span = (uint32_t)L.span;
    A.z0 = z0;
    return jump_table(c, L.lpc, L.span, z0, jtab);
}

// The stream's queue counters for persistent keystream launches, allocated
// and zeroed on the stream's first keystream launch.  Caller holds S->mu.
static int ks_counters(StreamState *S, KsCounters **out) {
    if (!S->ks.dev) {
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, kKsCtrBytes), "hipMalloc(keystream counters)");
        const hipError_t e = hipMemset(p, 0, kKsCtrBytes);
        if (e != hipSuccess) {
            (void)hipFree(p);
            HIP_TRY(e, "hipMemset(keystream counters)");
        }
        S->ks.dev = (uint64_t *)p;
        S->ks.par = 0;
    }
    *out = &S->ks;
    return S3DG_OK;
}

extern "C" {

int s3dg_xoshiro_jump(uint64_t *state4, uint64_t n) {
    if (!state4) return fail(S3DG_EINVAL, "null state");
    uint64_t J[4];
    if (!jump_poly(n, J)) return fail(S3DG_EINVAL, "xoshiro characteristic polynomial unavailable");
    apply_jump(state4, J);
    return S3DG_OK;
}

int s3dg_xoshiro_fill(s3dg_ctx *c, void *dst, uint64_t len, uint64_t chunk_bytes,
                      uint64_t seed_base, void *stream) {
    CTX_SCOPE(c);
    if (len == 0) return S3DG_OK;
    if (chunk_bytes == 0 || (chunk_bytes & 127u))
        return fail(S3DG_EINVAL, "chunk_bytes must be a positive multiple of 128");
    if (!dst || !aligned16(dst)) return fail(S3DG_EINVAL, "dst must be a 16-byte aligned device pointer");
    KeystreamArgs A{};
    const uint64_t *jt = nullptr;
    if (int r = keystream_plan(c, 0, chunk_bytes, (len + chunk_bytes - 1) / chunk_bytes, false, A, &jt)) return r;
    A.nchunks = (len + chunk_bytes - 1) / chunk_bytes;
    A.chunk_bytes = chunk_bytes;
    A.obj_len = len;
    A.chunk0 = 0;
    A.seed_base = seed_base;
    A.seed_mode = 0;
    A.unique = 0xFFFFFFFFu;
    A.m_unique = 0;
    A.zf_num = 0;
    A.zf_den = 1;
    StreamLock SL(c, (hipStream_t)stream);
    KsCounters *kc = nullptr;
    if (int r = ks_counters(SL.get(), &kc)) return r;
    HIP_TRY(launch_keystream((uint8_t *)dst, A, jt, c->ks[0], (hipStream_t)stream, kc, c->cus, c->ks_persist),
            "launch k_keystream");
    return S3DG_OK;
}

int s3dg_dgen_fill(s3dg_ctx *c, void *dst, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                   uint64_t dedup, uint32_t f_num, uint32_t f_den, uint64_t seed, void *stream) {
    return dgen_chunk(c, dst, obj_size, 0, 1, blk_lo, blk_hi, dedup, f_num, f_den, seed, 0,
                                    stream);
}

int s3dg_dgen_fill_stream(s3dg_ctx *c, void *dst, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                          uint64_t dedup, uint32_t f_num, uint32_t f_den, uint64_t seed_base,
                          uint64_t first_obj, void *stream) {
    if (n_objs > 1 && stride < obj_size) return fail(S3DG_EINVAL, "stride < obj_size: objects overlap");
    return dgen_chunk(c, dst, obj_size, stride, n_objs, 0, ~0ull, dedup, f_num, f_den, seed_base,
                                    first_obj, stream);
}

}  // extern "C"

namespace {

// dgen_chunk's argument checks, for blocks [blk_lo, blk_hi) of an object of nb blocks.
int dgen_check(const void *dst, uint64_t obj_size, uint64_t stride, uint64_t n_objs, uint64_t blk_lo, uint64_t blk_hi,
               uint64_t nb, uint32_t f_num, uint32_t f_den, const char *ptr_name = "dst") {
    if (!dst || !aligned16(dst) || (stride & 15u))
        return fail(S3DG_EINVAL, std::string(ptr_name) + " and stride must be 16-byte aligned");
    const uint64_t span_bytes = (blk_hi * kDgenBlock < obj_size ? blk_hi * kDgenBlock : obj_size) - blk_lo * kDgenBlock;
    if (n_objs > 1 && stride < span_bytes) return fail(S3DG_EINVAL, "stride too small: objects overlap");
    if (f_den == 0 || f_num >= f_den) return fail(S3DG_EINVAL, "need f_num < f_den");
    if (nb > 0xFFFFFFFFull) return fail(S3DG_EINVAL, "object larger than 2^32 blocks");
    return S3DG_OK;
}

// The zero prefix + tail split (s3dg_set_dgen_zero_split): from how many
// blocks, and the zero launch's shape and stream for the ratio's prefix class.
struct ZeroSplit {
    uint64_t split;
    LaunchCfg zlc;
    bool overlap;   // on the side stream, concurrent with the tails
};
ZeroSplit zero_split_cfg(s3dg_ctx *c, uint32_t f_num, uint32_t f_den) {
    ZeroSplit Z;
    const int k = (kDgenBlock * f_num) % f_den == 0 && (kDgenBlock * f_num / f_den) % 64 == 0 ? 0 : 1;
    std::lock_guard<std::mutex> g(c->mu);
    Z.split = c->dgen_zero_split;
    Z.zlc.store = c->zp_store >= 0 ? c->zp_store : kZeroPrefixStore[k];
    Z.zlc.waves_per_block = c->zp_waves > 0 ? c->zp_waves : kZeroPrefixWaves[k];
    Z.zlc.dyn_lds = occupancy_lds(c->zp_occ >= 0 ? c->zp_occ : kZeroPrefixOcc[k], 0);
    Z.overlap = (c->zp_overlap >= 0 ? c->zp_overlap : kZeroPrefixOverlap[k]) != 0;
    return Z;
}

// An error after the side stream's zero launch was queued must not return
// while that launch may still write the caller's buffer (the caller's
// stream never got to wait on zjoin): drain the side stream first.
struct ZeroJoinGuard {
    hipStream_t zs = nullptr;
    ~ZeroJoinGuard() {
        if (zs) (void)hipStreamSynchronize(zs);
    }
};

// The zero launch of a split: the first zw bytes of each of nchunks blocks,
// on the caller's stream before the tails, or (Z.overlap) forked to the side
// stream, which `guard` then holds until the caller's stream waits on zjoin.
int zero_launch(StreamState *SS, uint8_t *dst, uint64_t nchunks, uint64_t cpo, uint64_t stride, uint32_t zw,
                const ZeroSplit &Z, hipStream_t s, ZeroJoinGuard &guard) {
    if (!Z.overlap) {   // the prefixes' whole granules first (the tail launch masks a partial one)
        HIP_TRY(launch_zero_prefix(dst, nchunks, cpo, stride, kDgenBlock, zw, Z.zlc, s), "launch k_zero_prefix");
        return S3DG_OK;
    }
    // on the side stream, concurrent with the tails (disjoint bytes)
    if (!SS->zs) HIP_TRY(hipStreamCreateWithFlags(&SS->zs, hipStreamNonBlocking), "hipStreamCreate(zero)");
    for (hipEvent_t *e : {&SS->zfork, &SS->zjoin})
        if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate");
    HIP_TRY(hipEventRecord(SS->zfork, s), "hipEventRecord");
    HIP_TRY(hipStreamWaitEvent(SS->zs, SS->zfork, 0), "hipStreamWaitEvent");
    guard.zs = SS->zs;   // from here an error return first drains the side stream
    HIP_TRY(launch_zero_prefix(dst, nchunks, cpo, stride, kDgenBlock, zw, Z.zlc, SS->zs), "launch k_zero_prefix");
    HIP_TRY(hipEventRecord(SS->zjoin, SS->zs), "hipEventRecord");
    return S3DG_OK;
}

// One object: its last T chunks in lanes of half the length, handed out
// after the others by a persistent launch, so the launch drains on units
// half as long (default T: half a resident round of 1-wave units, i.e. one
// round of half units).  *tail: A2 / *jt2 hold that set and
// A is cut to the chunks before it.
int half_tail_set(s3dg_ctx *c, const KsShape &sh, uint64_t n_objs, uint64_t nchunks, KeystreamArgs &A,
                  KeystreamArgs &A2, const uint64_t **jt2, bool *tail) {
    *tail = false;
    int64_t tail_chunks;
    {
        std::lock_guard<std::mutex> g(c->mu);
        tail_chunks = c->ks_tail;
    }
    int res = 0;
    if (tail_chunks < 0) {
        if (keystream_occupancy(sh, &res) != hipSuccess) res = 0;
        (void)hipGetLastError();
    }
    // the conditions and both sets' chunks: ks_half_tail (s3dg_ks_plan.h)
    const KsHalfTail H = ks_half_tail(tail_chunks, (uint64_t)res, (uint64_t)c->cus, (uint32_t)sh.waves,
                                      (uint32_t)sh.draws, n_objs, nchunks, A.chunk0, A.lpc, A.span);
    if (H.take) {
        A2 = A;
        A2.lpc = H.lpc2;
        A2.span = H.span2;
        A2.nchunks = H.T;
        A2.cpo = H.cpo2;
        A2.chunk0 = H.chunk0_2;
        A2.doff = H.doff;
        A.nchunks = H.nchunks1;
        A.cpo = H.cpo1;
        if (int r = jump_table(c, A2.lpc, A2.span, A2.z0, jt2)) return r;
        *tail = true;
    }
    return S3DG_OK;
}

}  // namespace

namespace s3dg {

int dgen_chunk(s3dg_ctx *c, void *dst, uint64_t obj_size, uint64_t stride, uint64_t n_objs, uint64_t blk_lo,
               uint64_t blk_hi, uint64_t dedup, uint32_t f_num, uint32_t f_den, uint64_t seed_base,
               uint64_t first_obj, void *stream) {
    CTX_SCOPE(c);
    if (obj_size == 0 || n_objs == 0) return S3DG_OK;
    const uint64_t nb = (obj_size + kDgenBlock - 1) / kDgenBlock;
    if (blk_hi > nb) blk_hi = nb;
    if (blk_lo >= blk_hi) return S3DG_OK;
    if (int r = dgen_check(dst, obj_size, stride, n_objs, blk_lo, blk_hi, nb, f_num, f_den)) return r;
    // zero prefix + tail split: every block of the launch full length, the
    // prefix at least 8 whole granules, enough blocks to pay for two launches
    const ZeroSplit Z = zero_split_cfg(c, f_num, f_den);
    // the zero launch writes each block's whole 4 KiB granules of zeros (zw
    // bytes); the tail launch starts at draw z0 = zw / 8 and zeroes the rest
    // of the prefix (< 4 KiB) in its lane rows.  Tails that start inside a
    // granule (zw down to 16 B) ran 25-35 % slower: lane regions off the
    // 128-B lines (profiles/r05/g).
    // The decisions: ks_dgen_call (s3dg_ks_plan.h).
    const KsDgenCall P = ks_dgen_call(obj_size, n_objs, blk_lo, blk_hi, f_num, f_den, Z.split);
    const uint64_t nchunks = P.nchunks;
    const uint32_t zw = P.zw;
    if (P.cut_last) {
        // the objects' full blocks split, their short last blocks in a launch of their own
        if (int r = dgen_chunk(c, dst, obj_size, stride, n_objs, blk_lo, blk_hi - 1, dedup, f_num, f_den, seed_base,
                               first_obj, stream))
            return r;
        return dgen_chunk(c, (uint8_t *)dst + (blk_hi - 1 - blk_lo) * kDgenBlock, obj_size, stride, n_objs, blk_hi - 1,
                          blk_hi, dedup, f_num, f_den, seed_base, first_obj, stream);
    }
    const bool zsplit = P.zsplit;
    KeystreamArgs A{};
    const uint64_t *jt = nullptr;
    if (int r = keystream_plan(c, 1, kDgenBlock, nchunks, f_num > 0 && !zsplit, A, &jt, P.z0))
        return r;
    const uint64_t U = s3dg_unique_blocks(nb, dedup);
    A.cpo = blk_hi - blk_lo;
    A.nchunks = A.cpo * n_objs;
    A.chunk_bytes = kDgenBlock;
    A.obj_len = obj_size;
    A.chunk0 = blk_lo;
    A.obj_stride = stride;
    A.seed_base = seed_base + (first_obj << 32);
    A.seed_step = 1ull << 32;
    A.seed_mode = 1;
    A.unique = U == nb ? 0xFFFFFFFFu : (uint32_t)U;
    A.m_unique = fastmod_magic(U == nb ? 1u : (uint32_t)U);
    A.zf_num = f_num;
    A.zf_den = f_den;
    KsShape sh = c->ks[1];
    if (f_num > 0 && !zsplit) {   // zero-prefix launches (512-draw lanes): 4-wave workgroups, groups of 32 waves
        if (c->ks_auto_waves[1]) sh.waves = kDgenPrefixWaves;
        if (c->ks_auto_xcd[1]) sh.xcd_waves = kDgenPrefixXcdWaves;
    }
    hipStream_t s = (hipStream_t)stream;
    StreamLock SL(c, s);
    StreamState *SS = SL.get();
    KsCounters *kc = nullptr;
    if (int r = ks_counters(SS, &kc)) return r;
    ZeroJoinGuard zguard;   // spans everything between the side stream's launch and the join below
    if (zsplit)
        if (int r = zero_launch(SS, (uint8_t *)dst, nchunks, A.cpo, stride, zw, Z, s, zguard)) return r;
    KeystreamArgs A2{};
    const uint64_t *jt2 = nullptr;
    bool tail = false;
    if (int r = half_tail_set(c, sh, n_objs, nchunks, A, A2, &jt2, &tail)) return r;
    HIP_TRY(launch_keystream((uint8_t *)dst, A, jt, sh, s, kc, c->cus, c->ks_persist, tail ? &A2 : nullptr, jt2),
            "launch k_keystream(dgen)");
    if (zsplit && Z.overlap) HIP_TRY(hipStreamWaitEvent(s, SS->zjoin, 0), "hipStreamWaitEvent");
    zguard.zs = nullptr;   // joined: the caller's stream now orders after the zero launch
    return S3DG_OK;
}

}  // namespace s3dg

// ---- verification (k_verify_keystream) -----------------------
namespace {

// The verify launch's own lane plan (ks_verify_plan: lane regions of whole
// 4 KiB granules, z0 = 0) from the mode's min_lane_draws knob, and its jump
// table from the context's cache.
int ks_verify_lanes(s3dg_ctx *c, int mode, uint64_t chunk_bytes, uint64_t nchunks, bool zero_prefix,
                    KeystreamArgs &A, const uint64_t **jtab) {
    const uint64_t md = c->ks_min_draws[mode];
    uint64_t knob = md == kDefaultKsMinDraws[mode] ? 0 : md;        // 0: not set by the caller
    if (mode == 1 && zero_prefix && !knob) knob = kDgenPrefixMinDraws;   // as the fill: more all-zero waves
    const KsVerifyPlan P = ks_verify_plan(chunk_bytes, nchunks, (uint32_t)c->cus, knob);
    if (P.span > 0xFFFFFFFFull) return fail(S3DG_EINVAL, "chunk too large");
    A.lpc = P.lpc;
    A.span = (uint32_t)P.span;
    A.z0 = 0;
    return jump_table(c, P.lpc, P.span, 0, jtab);
}

void verify_clean(s3dg_verify_result *out) {
    out->mismatched_bytes = 0;
    out->mismatched_blocks = 0;
    out->first_offset = UINT64_MAX;
}

}  // namespace

namespace s3dg {

int dgen_verify_launch(s3dg_ctx *c, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                       uint64_t blk_lo, uint64_t blk_hi, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                       uint64_t seed_base, uint64_t first_obj, uint64_t off0, VerifyRec *rec, void *stream) {
    if (obj_size == 0 || n_objs == 0) return S3DG_OK;
    const uint64_t nb = (obj_size + kDgenBlock - 1) / kDgenBlock;
    if (blk_hi > nb) blk_hi = nb;
    if (blk_lo >= blk_hi) return S3DG_OK;
    if (int r = dgen_check(src, obj_size, stride, n_objs, blk_lo, blk_hi, nb, f_num, f_den, "src")) return r;
    KeystreamArgs A{};
    const uint64_t *jt = nullptr;
    if (int r = ks_verify_lanes(c, 1, kDgenBlock, (blk_hi - blk_lo) * n_objs, f_num > 0, A, &jt)) return r;
    const uint64_t U = s3dg_unique_blocks(nb, dedup);
    A.cpo = blk_hi - blk_lo;
    A.nchunks = A.cpo * n_objs;
    A.chunk_bytes = kDgenBlock;
    A.obj_len = obj_size;
    A.chunk0 = blk_lo;
    A.obj_stride = stride;
    A.seed_base = seed_base + (first_obj << 32);
    A.seed_step = 1ull << 32;
    A.seed_mode = 1;
    A.unique = U == nb ? 0xFFFFFFFFu : (uint32_t)U;
    A.m_unique = fastmod_magic(U == nb ? 1u : (uint32_t)U);
    A.zf_num = f_num;
    A.zf_den = f_den;
    HIP_TRY(launch_verify_keystream((const uint8_t *)src, A, jt, off0, rec, (hipStream_t)stream),
            "launch k_verify_keystream(dgen)");
    return S3DG_OK;
}

}  // namespace s3dg

namespace {

// A device verify call over DG1 objects: the launch's argument errors come
// back as they are (with their text), HIP errors through the record handling.
int dgen_verify(s3dg_ctx *c, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs, uint64_t blk_lo,
                uint64_t blk_hi, uint64_t dedup, uint32_t f_num, uint32_t f_den, uint64_t seed_base,
                uint64_t first_obj, void *stream, s3dg_verify_result *out) {
    CTX_SCOPE(c);
    if (!out) return fail(S3DG_EINVAL, "null output");
    verify_clean(out);
    if (obj_size == 0 || n_objs == 0) return S3DG_OK;
    const uint64_t nb = (obj_size + kDgenBlock - 1) / kDgenBlock;
    if (blk_hi > nb) blk_hi = nb;
    if (blk_lo >= blk_hi) return S3DG_OK;
    if (int r = dgen_check(src, obj_size, stride, n_objs, blk_lo, blk_hi, nb, f_num, f_den, "src")) return r;
    int lr = S3DG_OK;
    std::string lmsg;
    const int r = verify_with_record(c, (hipStream_t)stream, "launch k_verify_keystream(dgen)", [&](VerifyRec *rec) {
        lr = dgen_verify_launch(c, src, obj_size, stride, n_objs, blk_lo, blk_hi, dedup, f_num, f_den, seed_base,
                                first_obj, 0, rec, stream);
        if (lr != S3DG_OK) lmsg = s3dg_last_error();
        return lr == S3DG_OK ? hipSuccess : hipErrorInvalidValue;
    }, out);
    return lr != S3DG_OK ? fail(lr, lmsg) : r;
}

}  // namespace

extern "C" {

int s3dg_verify_xoshiro(s3dg_ctx *c, const void *src, uint64_t len, uint64_t chunk_bytes, uint64_t seed_base,
                        void *stream, s3dg_verify_result *out) {
    CTX_SCOPE(c);
    if (!out) return fail(S3DG_EINVAL, "null output");
    verify_clean(out);
    if (len == 0) return S3DG_OK;
    if (chunk_bytes == 0 || (chunk_bytes & (kBlk - 1)))
        return fail(S3DG_EINVAL, "chunk_bytes must be a positive multiple of 4096 (the verify's 4 KiB granules; "
                                 "s3dg_xoshiro_fill itself takes multiples of 128)");
    if (!src || !aligned16(src)) return fail(S3DG_EINVAL, "src must be a 16-byte aligned device pointer");
    const uint64_t nchunks = (len + chunk_bytes - 1) / chunk_bytes;
    KeystreamArgs A{};
    const uint64_t *jt = nullptr;
    if (int r = ks_verify_lanes(c, 0, chunk_bytes, nchunks, false, A, &jt)) return r;
    A.nchunks = nchunks;
    A.chunk_bytes = chunk_bytes;
    A.obj_len = len;
    A.chunk0 = 0;
    A.seed_base = seed_base;
    A.seed_mode = 0;
    A.unique = 0xFFFFFFFFu;
    A.m_unique = 0;
    A.zf_num = 0;
    A.zf_den = 1;
    return verify_with_record(c, (hipStream_t)stream, "launch k_verify_keystream", [&](VerifyRec *rec) {
        return launch_verify_keystream((const uint8_t *)src, A, jt, 0, rec, (hipStream_t)stream);
    }, out);
}

int s3dg_verify_dgen(s3dg_ctx *c, const void *src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                     uint64_t dedup, uint32_t f_num, uint32_t f_den, uint64_t seed, void *stream,
                     s3dg_verify_result *out) {
    return dgen_verify(c, src, obj_size, 0, 1, blk_lo, blk_hi, dedup, f_num, f_den, seed, 0, stream, out);
}

int s3dg_verify_dgen_stream(s3dg_ctx *c, const void *src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                            uint64_t dedup, uint32_t f_num, uint32_t f_den, uint64_t seed_base, uint64_t first_obj,
                            void *stream, s3dg_verify_result *out) {
    if (n_objs > 1 && stride < obj_size) return fail(S3DG_EINVAL, "stride < obj_size: objects overlap");
    return dgen_verify(c, src, obj_size, stride, n_objs, 0, ~0ull, dedup, f_num, f_den, seed_base, first_obj, stream,
                       out);
}

}  // extern "C"
