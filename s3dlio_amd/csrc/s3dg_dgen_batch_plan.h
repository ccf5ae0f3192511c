// s3dg_dgen_batch_plan.h — the host's part of s3dg_dgen_fill_batch and
// s3dg_verify_dgen_batch as pure functions: the argument and
// descriptor checks with their messages, the chunk records, the size class of
// a chunk, the lane plan of a class and the launches with their record ranges.
// No HIP, no context: it compiles with g++ alone
// (tests/capi/dgen_batch_plan_sweep.cpp).
//
// A call becomes one record per 1 MiB block of every non-empty object, sorted
// by size class: all full blocks (class kDgbFull) form one launch, the ragged
// last blocks one launch per power-of-two class (4 KiB and below .. 1 MiB),
// each planned as if its chunks were the class's ceiling.  Within a class the
// records keep the descriptors' order.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "s3dlio_gpu.h"
#include "s3dg_ks_verify_plan.h"

namespace s3dg {

constexpr uint64_t kDgbBlock = 1ull << 20;               // DG1's block
constexpr uint64_t kDgbPhi = 0x9E3779B97F4A7C15ull;      // block u's seed = entropy ^ (u * phi)
constexpr uint32_t kDgbMinShift = 12, kDgbMaxShift = 20; // ragged classes: ceilings 4 KiB .. 1 MiB
constexpr uint32_t kDgbFull = kDgbMaxShift - kDgbMinShift + 1;   // the class of full 1 MiB chunks
constexpr uint32_t kDgbClasses = kDgbFull + 1;           // at most this many launches per call
// lanes of one launch: its work items fit the dispatch packet's 32 bits with room for 4-wave workgroups
constexpr uint64_t kDgbMaxLanes = 1ull << 31;
// the fill's lane rules (keystream_plan): draws per lane with and without a
// zero prefix, the floor for small launches, lanes per chunk at most
constexpr uint64_t kDgbDraws = 2048, kDgbPrefixDraws = 512, kDgbMinSpan = 256;
constexpr uint32_t kDgbMaxLpc = 1024;

// One chunk: a 1 MiB block of an object, or its ragged last one.  32 bytes,
// read by the kernels as two 16-byte loads.
struct DgenChunkRec {
    uint64_t off;     // byte offset of the chunk from the base pointer
    uint64_t seed;    // entropy ^ ((blk % U) * phi): the chunk's xoshiro seed input
    uint32_t len;     // bytes, 1 .. 1 MiB
    uint32_t zlen;    // zero prefix: floor(len * f_num / f_den)
    uint32_t obj;     // the caller's descriptor index (the verify's per-object record)
    uint32_t blk;     // block index within the object (the verify's per-object offsets)
};
static_assert(sizeof(DgenChunkRec) == 32, "DgenChunkRec is two 16-byte loads");

// s3dg_unique_blocks, restated so this header stands alone.
inline uint64_t dgen_unique_blocks(uint64_t nblocks, uint64_t dedup) {
    if (dedup <= 1) return nblocks;
    double r = round((double)nblocks / (double)dedup);   // f64::round, half away
    if (r < 1.0) r = 1.0;
    return (uint64_t)r;
}

inline uint64_t dgen_blocks(uint64_t size) { return size / kDgbBlock + (size % kDgbBlock != 0); }

// Size class of a chunk of len bytes (1 .. 1 MiB): kDgbFull for a full block,
// else the smallest k with len <= 4 KiB << k.
inline uint32_t dgen_chunk_class(uint64_t len) {
    if (len >= kDgbBlock) return kDgbFull;
    uint32_t k = 0;
    while (((uint64_t)1 << (kDgbMinShift + k)) < len) ++k;
    return k;
}
// Bytes a class is planned for.
inline uint64_t dgen_class_ceiling(uint32_t cls) {
    return cls >= kDgbFull ? kDgbBlock : (uint64_t)1 << (kDgbMinShift + cls);
}

// The call's pointer arguments, in the order they are refused; nullptr: fine.
// verify: `out` is required and named first, as s3dg_verify_controlled_batch does.
inline const char *dgen_batch_args(const void *base, const s3dg_obj_desc *d, uint64_t n, bool verify,
                                   const void *out) {
    if (verify && !out) return "null output";
    if (n == 0) return nullptr;
    if (!d) return "null descriptor array";
    if (n > 0xFFFFFFFFull) return "more than 2^32 objects";   // a record names its object in 32 bits
    if (!base || ((uintptr_t)base & 15u))
        return verify ? "src_base must be 16-byte aligned" : "dst_base must be 16-byte aligned";
    return nullptr;
}

// One non-empty descriptor; nullptr: fine.
inline const char *dgen_desc_check(const s3dg_obj_desc &o) {
    if (o.dst_off & 15u) return "dst_off must be a multiple of 16";
    if (o.f_den == 0 || o.f_num >= o.f_den) return "need f_num < f_den";
    if (dgen_blocks(o.size) > 0xFFFFFFFFull) return "object larger than 2^32 blocks";
    return nullptr;
}

// "object 7: need f_num < f_den"
inline std::string dgen_batch_message(uint64_t bad, const char *msg) {
    char b[40];
    snprintf(b, sizeof b, "object %llu: ", (unsigned long long)bad);
    return std::string(b) + msg;
}

// All n descriptors, before anything is enqueued: the first offending one
// names the refusal (msg, bad).  live = non-empty objects; count[c] = chunks of
// class c; zeros[c] = those with a zero prefix.
struct DgenBatchCheck {
    const char *msg = nullptr;
    uint64_t bad = UINT64_MAX, live = 0, chunks = 0;
    uint64_t count[kDgbClasses] = {}, zeros[kDgbClasses] = {};
};
inline DgenBatchCheck dgen_batch_check(const s3dg_obj_desc *d, uint64_t n) {
    DgenBatchCheck C;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_obj_desc &o = d[k];
        if (o.size == 0) continue;   // empty objects are allowed anywhere, whatever else they say
        if (const char *m = dgen_desc_check(o)) {
            C = DgenBatchCheck();
            C.msg = m;
            C.bad = k;
            return C;
        }
        ++C.live;
        const uint64_t full = o.size / kDgbBlock, rag = o.size % kDgbBlock;
        C.count[kDgbFull] += full;
        if (o.f_num) C.zeros[kDgbFull] += full;
        if (rag) {
            const uint32_t c = dgen_chunk_class(rag);
            ++C.count[c];
            if (rag * o.f_num / o.f_den) ++C.zeros[c];
        }
        C.chunks += full + (rag != 0);
    }
    return C;
}

// Lanes of a launch whose chunks are planned as `ceil_bytes` long: lpc lanes
// per chunk (a power of two), each over `span` draws (8 bytes each).
//   fill: keystream_plan's rule.  Lanes of at least min_draws draws (the knob
//   of s3dg_set_keystream_shape, 0 = not set: 2048, or 512 when the launch has
//   zero prefixes); when the knob is not set a launch of few chunks is spread
//   over more lanes, down to 256 draws, until it has about 4 waves per CU.
//   span is a multiple of the stage's `draws`.
//   verify: ks_verify_plan's rule (span a multiple of 512: whole granules).
struct DgenLanes {
    uint32_t lpc;
    uint64_t span;
};
inline DgenLanes dgen_class_lanes(uint64_t ceil_bytes, uint64_t nchunks, uint32_t cus, uint64_t knob, bool zeros,
                                  uint32_t draws, bool verify) {
    if (verify) {
        const KsVerifyPlan P = ks_verify_plan(ceil_bytes, nchunks, cus, knob ? knob : zeros ? kDgbPrefixDraws : 0);
        return DgenLanes{P.lpc, P.span};
    }
    const uint64_t nd = ceil_bytes / 8;
    const uint64_t min_draws = knob ? knob : zeros ? kDgbPrefixDraws : kDgbDraws;
    uint32_t lpc = 1;
    while (lpc < kDgbMaxLpc && nd / (2 * (uint64_t)lpc) >= min_draws) lpc *= 2;
    if (!knob) {
        const uint64_t target_lanes = (uint64_t)cus * 4 * 64;
        while (lpc < kDgbMaxLpc && nchunks * lpc < target_lanes && nd / (2 * (uint64_t)lpc) >= kDgbMinSpan) lpc *= 2;
    }
    uint64_t span = (nd + lpc - 1) / lpc;
    span = (span + draws - 1) / draws * draws;
    return DgenLanes{lpc, span};
}

// Lane `sub` of a chunk of len bytes: its region [rb, rb + rlen) of the chunk
// (rlen 0: nothing), as the kernels derive it.
struct DgenRegion {
    uint64_t rb, rlen;
};
inline DgenRegion dgen_lane_region(uint64_t len, uint64_t span, uint32_t sub) {
    const uint64_t rb = (uint64_t)sub * span * 8;
    if (len <= rb) return DgenRegion{rb, 0};
    return DgenRegion{rb, len - rb < span * 8 ? len - rb : span * 8};
}

// The launches of a call: the full chunks first, then the ragged classes from
// the largest down.  Launch L covers records [rec0, rec0 + nrec) of the table.
struct DgenLaunch {
    uint32_t cls;
    bool zeros;       // some chunk has a zero prefix: the fill's prefix shape
    uint64_t rec0, nrec;
    DgenLanes lanes;
};
struct DgenBatchPlan {
    uint32_t nlaunch = 0;
    DgenLaunch launch[kDgbClasses];
    uint64_t start[kDgbClasses] = {};   // first record of each class
    const char *msg = nullptr;          // a launch beyond the grid's reach
};
inline DgenBatchPlan dgen_batch_plan(const DgenBatchCheck &C, uint32_t cus, uint64_t knob, uint32_t draws,
                                     bool verify) {
    DgenBatchPlan P;
    uint64_t at = 0;
    for (uint32_t q = 0; q < kDgbClasses; ++q) {
        const uint32_t cls = kDgbFull - q;
        P.start[cls] = at;
        if (C.count[cls] == 0) continue;
        DgenLaunch &L = P.launch[P.nlaunch++];
        L.cls = cls;
        L.zeros = C.zeros[cls] != 0;
        L.rec0 = at;
        L.nrec = C.count[cls];
        L.lanes = dgen_class_lanes(dgen_class_ceiling(cls), L.nrec, cus, knob, L.zeros, draws, verify);
        if (L.nrec > kDgbMaxLanes / L.lanes.lpc) P.msg = "more than 2^31 lanes in one launch";
        at += L.nrec;
    }
    return P;
}

// The record table of checked descriptors: out has C.chunks records, class c's
// from P.start[c] in the descriptors' order.
inline void dgen_batch_records(const s3dg_obj_desc *d, uint64_t n, const DgenBatchPlan &P, DgenChunkRec *out) {
    uint64_t cur[kDgbClasses];
    for (uint32_t c = 0; c < kDgbClasses; ++c) cur[c] = P.start[c];
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_obj_desc &o = d[k];
        if (o.size == 0) continue;
        const uint64_t nb = dgen_blocks(o.size), U = dgen_unique_blocks(nb, o.dedup);
        for (uint64_t i = 0; i < nb; ++i) {
            const uint64_t len = i + 1 < nb || o.size % kDgbBlock == 0 ? kDgbBlock : o.size % kDgbBlock;
            DgenChunkRec &R = out[cur[dgen_chunk_class(len)]++];
            R.off = o.dst_off + i * kDgbBlock;
            R.seed = o.entropy ^ ((i % U) * kDgbPhi);
            R.len = (uint32_t)len;
            R.zlen = (uint32_t)(len * o.f_num / o.f_den);
            R.obj = (uint32_t)k;
            R.blk = (uint32_t)i;
        }
    }
}

}  // namespace s3dg
