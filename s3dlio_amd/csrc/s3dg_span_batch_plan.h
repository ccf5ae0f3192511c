// s3dg_span_batch_plan.h — the host's part of a batch add of the read-only
// analyses (s3dg_measure_add_batch, s3dg_chunks_add_batch, s3dg_lz_add_batch;
// DESIGN.md §5.13) as pure functions: the checks of the spans with their
// messages, the per-object granule, block and slot counts, their 64-bit prefix
// sums, the tile records of the granule passes and the sub-launch cuts.  No
// HIP, no context: it compiles with g++ alone
// (tests/capi/span_batch_plan_sweep.cpp).
//
// The table of one add is built on the host and uploaded: one SpanEnt per
// non-empty span, in the caller's order (empty spans are squeezed out: they
// own no granule, block or slot), then one SpanTile per tile of 2^tshift
// granules of an object.  Nothing is reordered or merged: two spans over the
// same bytes are two entries.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "s3dg_batch_plan.h"   // the tile-shift range, best_tile_shift and the tiled costs
#include "s3dg_span_plan.h"

#if defined(__HIPCC__)
#define S3DG_SB_HD __host__ __device__
#else
#define S3DG_SB_HD
#endif

namespace s3dg {

constexpr uint64_t kSpanBatchGranule = 4096;
constexpr uint64_t kSpanBatchMaxObj = (1ull << 31) * kSpanBatchGranule;   // the fill's largest object
constexpr uint64_t kSpanBatchMaxGranules = 1ull << 40;                    // granules of one add
constexpr uint64_t kSpanBatchMaxLive = 0xFFFFFFFFull;                     // a tile names its object in 32 bits
constexpr uint64_t kSpanBatchMaxSlots = 0x7FFFFFFFull;                    // chunk slots of one add (= of one handle)
constexpr uint64_t kSpanBatchMaxGrid = 1ull << 22;                        // slots of one sub-launch; a multiple of every tile

// A non-empty span and where its results go: the prefix sums over the entries before it.
struct SpanEnt {
    uint64_t off, size;   // bytes from src_base; bytes (> 0)
    uint64_t g0;          // its first 4 KiB granule among the add's granules
    uint64_t b0;          // its first block among the add's blocks (block_bytes > 0)
    uint64_t s0;          // its first chunk slot among the add's slots (min_bytes > 0)
};

// 2^tshift granules of one object from granule `first` on; slot k of the tile
// is granule first + k, dead when k * 4096 >= left.
struct SpanTile {
    uint64_t off;         // bytes from src_base to the tile's first byte
    uint64_t left;        // bytes from there to the object's end (> 0)
    uint64_t rec;         // the tile's first granule among the add's granules (g0 + first)
    uint32_t first;       // the tile's first granule within its object
    uint32_t obj;         // the object's entry
};

// What one add counts: filled by span_batch_check.
struct SpanBatchCounts {
    uint64_t live = 0;       // non-empty spans
    uint64_t bytes = 0, granules = 0, blocks = 0, slots = 0;
    uint64_t ntiles[kTileShiftMax + 1] = {};
};

inline uint64_t span_obj_granules(uint64_t size) { return span_ceil_div(size, kSpanBatchGranule); }
inline uint64_t span_obj_blocks(uint64_t size, uint64_t block_bytes) {
    return block_bytes ? span_ceil_div(size, block_bytes) : 0;
}
// chunk slots of an object: s3dg_chunk_plan.h's rpo
inline uint64_t span_obj_slots(uint64_t size, uint64_t min_bytes) {
    return min_bytes ? span_ceil_div(size, min_bytes) + 1 : 0;
}
inline uint64_t span_obj_tiles(uint64_t size, uint32_t tshift) {
    return (span_obj_granules(size) + (1ull << tshift) - 1) >> tshift;
}

inline std::string span_batch_at(uint64_t k, const char *what) {
    char b[160];
    snprintf(b, sizeof(b), "span %llu: %s", (unsigned long long)k, what);
    return b;
}

// The rules of one non-empty span, in the order they are refused; nullptr: fine.
inline const char *span_check_one(const s3dg_span &p) {
    if (p.off & 15u) return "off must be a multiple of 16";
    if (p.size > kSpanBatchMaxObj) return "object larger than 2^31 blocks";
    return nullptr;
}

// All of an add's arguments, before anything is reserved or enqueued.  Returns
// true and fills *C, or false with the refusal's text in *why; a refusal of a
// span names the first offending index.  block_bytes: the handle's (0: it has
// no blocks); min_bytes: the chunker's (0: the handle has no chunk slots).
// n == 0 is accepted whatever the pointers, empty spans whatever their offset,
// and a batch of empty spans alone whatever src_base.
inline bool span_batch_check(uint64_t src_base, const s3dg_span *spans, uint64_t n, uint64_t block_bytes,
                             uint64_t min_bytes, SpanBatchCounts *C, std::string *why) {
    *C = SpanBatchCounts{};
    if (n == 0) return true;
    if (!spans) return *why = "null span array", false;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_span p = spans[k];
        if (p.size == 0) continue;
        if (!src_base || (src_base & 15u)) return *why = "src_base must be a 16-byte aligned device pointer", false;
        if (const char *w = span_check_one(p)) return *why = span_batch_at(k, w), false;
        if (p.off > UINT64_MAX - p.size) return *why = span_batch_at(k, "off + size overflows"), false;
        ++C->live;
        C->bytes += p.size;                                   // <= 2^40 granules' bytes = 2^52
        C->granules += span_obj_granules(p.size);
        C->blocks += span_obj_blocks(p.size, block_bytes);
        C->slots += span_obj_slots(p.size, min_bytes);        // <= size / 32 + 1: below 2^48
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) C->ntiles[sh] += span_obj_tiles(p.size, sh);
        if (C->live > kSpanBatchMaxLive) return *why = span_batch_at(k, "more than 2^32 - 1 spans in one add"), false;
        if (C->granules > kSpanBatchMaxGranules)
            return *why = span_batch_at(k, "more than 2^40 granules in one add"), false;
        if (C->slots > kSpanBatchMaxSlots)
            return *why = span_batch_at(k, "more than 2^31 - 1 chunk slots in one add"), false;
    }
    return true;
}

// Tile size of an add: the forced one (s3dg_set_batch_tile: 2..64 granules,
// knob = its shift) or the 8..64-granule tile of least tiled cost, as
// verify_batch chooses.
inline uint32_t span_batch_tile_shift(const SpanBatchCounts &C, uint32_t knob) {
    if (knob >= kTileShiftMin && knob <= kTileShiftMax) return knob;
    return best_tile_shift(C.ntiles, C.granules, kDeadSlotCostTiled, kRecordCostTiled);
}

// The uploaded table: [entries | tiles], the tiles at a multiple of 256 bytes.
inline uint64_t span_batch_tile_offset(uint64_t live) { return span_align256(live * sizeof(SpanEnt)); }
inline uint64_t span_batch_table_bytes(uint64_t live, uint64_t tiles) {
    return span_batch_tile_offset(live) + tiles * sizeof(SpanTile);
}

// The table of checked spans: ents[0, C.live) and, when tiles is not null,
// tiles[0, C.ntiles[tshift]), an object's tiles in a row.
inline void span_batch_build(const s3dg_span *spans, uint64_t n, uint64_t block_bytes, uint64_t min_bytes,
                             uint32_t tshift, SpanEnt *ents, SpanTile *tiles) {
    uint64_t j = 0, g0 = 0, b0 = 0, s0 = 0, t = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_span p = spans[k];
        if (p.size == 0) continue;
        ents[j] = SpanEnt{p.off, p.size, g0, b0, s0};
        const uint64_t ng = span_obj_granules(p.size);
        if (tiles) {
            for (uint64_t f = 0; f < ng; f += 1ull << tshift)
                tiles[t++] = SpanTile{p.off + f * kSpanBatchGranule, p.size - f * kSpanBatchGranule, g0 + f,
                                      (uint32_t)f, (uint32_t)j};
        }
        g0 += ng;
        b0 += span_obj_blocks(p.size, block_bytes);
        s0 += span_obj_slots(p.size, min_bytes);
        ++j;
    }
}

// Sub-launches of a granule pass over `tiles` tiles: each covers whole tiles
// and at most kSpanBatchMaxGrid slots.
inline uint64_t span_batch_sub_tiles(uint32_t tshift) { return kSpanBatchMaxGrid >> tshift; }
inline uint64_t span_batch_sub_launches(uint64_t tiles, uint32_t tshift) {
    return span_ceil_div(tiles, span_batch_sub_tiles(tshift));
}
// Sub-launch i: tiles [*t0, *t0 + *nt), a grid of *nt << tshift slots.
inline void span_batch_sub_launch(uint64_t tiles, uint32_t tshift, uint64_t i, uint64_t *t0, uint64_t *nt) {
    const uint64_t per = span_batch_sub_tiles(tshift);
    *t0 = i * per;
    *nt = tiles - *t0 < per ? tiles - *t0 : per;
}

// The entry that owns block i of the add: the last entry whose first block is
// at or below i.  i is below the add's blocks, so the entry exists; about
// log2(n) dependent loads.
S3DG_SB_HD inline uint64_t span_batch_find(const SpanEnt *e, uint64_t n, uint64_t i) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (e[mid].b0 <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace s3dg
