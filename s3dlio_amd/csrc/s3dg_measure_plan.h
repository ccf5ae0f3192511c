// s3dg_measure_plan.h — the layout of one measure add (k_measure and
// k_measure_blocks) as pure functions: no HIP, no context, so
// every argument check of s3dg_measure_* can be compiled and tested on its own
// (tests/capi/measure_plan_sweep.cpp, tests/test_measure_cpu.py).
#pragma once
#include <stdint.h>

#include "s3dg_span_plan.h"

namespace s3dg {

constexpr uint64_t kMeasureGranule = 4096;          // pass 1's unit: one workgroup
constexpr uint64_t kMeasureMaxBlock = 1ull << 30;   // largest block_bytes
constexpr uint64_t kMeasureMaxSlots = 1ull << 40;   // fingerprints one handle may hold
// the shared limits under the names this plan's callers and sweep know them by
constexpr uint64_t kMeasureMaxGridX = kSpanMaxGridX, kMeasureMaxGridY = kSpanMaxGridY, kMeasureMinCap = kSpanMinCap;

// block_bytes: a positive multiple of 4096, at most 2^30.
inline const char *measure_block_bytes_check(uint64_t block_bytes) {
    if (block_bytes == 0 || block_bytes % kMeasureGranule || block_bytes > kMeasureMaxBlock)
        return "block_bytes must be a positive multiple of 4096, at most 2^30";
    return nullptr;
}

// One add: n_objs object ranges of `len` bytes each (len > 0 unless the add is
// empty), range j at src + j*stride, each cut into blocks of block_bytes from
// its start (the last one may be ragged) and into 4 KiB granules.
struct MeasurePlan {
    uint64_t n_objs;         // 0: an empty add, nothing is launched
    uint64_t len;            // bytes measured per object
    uint64_t skip;           // add_range: bytes of the object before src (blk_lo * block_bytes)
    uint32_t gpb;            // granules per full block
    uint64_t gpo, bpo;       // granules and blocks per object
    uint64_t last_block;     // length of an object's last block, in (0, block_bytes]
    uint32_t last_granule;   // length of an object's last granule, in (0, 4096]
    uint64_t slots;          // fingerprint slots to reserve = blocks = n_objs * bpo
    uint64_t bytes;          // payload bytes = n_objs * len
    uint64_t records;        // per-granule records of pass 1 = n_objs * gpo
    uint64_t nx, ny;         // sub-launches along the granules and along the objects
};

inline const char *measure_plan_fill(MeasurePlan *P, uint64_t len, uint64_t n_objs, uint64_t block_bytes) {
    P->n_objs = n_objs;
    P->len = len;
    P->gpb = (uint32_t)(block_bytes / kMeasureGranule);
    P->gpo = span_ceil_div(len, kMeasureGranule);
    P->bpo = span_ceil_div(len, block_bytes);
    if (P->gpo > 0xFFFFFFFFull) return "object range larger than 2^32 granules";
    if (n_objs > kMeasureMaxSlots / P->gpo) return "more than 2^40 granules in one add";
    P->last_block = len - (P->bpo - 1) * block_bytes;
    P->last_granule = (uint32_t)(len - (P->gpo - 1) * kMeasureGranule);
    P->slots = n_objs * P->bpo;
    P->records = n_objs * P->gpo;
    P->bytes = n_objs * len;   // <= 2^40 * 4096
    P->nx = span_nx(P->gpo);
    P->ny = span_ny(n_objs);
    return nullptr;
}

// s3dg_measure_add_stream's arguments.  Returns null and fills *P, or the
// refusal's text (S3DG_EINVAL).  An empty add (obj_size or n_objs 0) is
// accepted whatever the pointer: P->n_objs == 0.
inline const char *measure_plan_stream(MeasurePlan *P, uint64_t src, uint64_t obj_size, uint64_t stride,
                                       uint64_t n_objs, uint64_t block_bytes) {
    *P = MeasurePlan{};
    if (const char *w = measure_block_bytes_check(block_bytes)) return w;
    if (obj_size == 0 || n_objs == 0) return nullptr;
    if (const char *w = span_check(src, obj_size, stride, n_objs)) return w;
    return measure_plan_fill(P, obj_size, n_objs, block_bytes);
}

// s3dg_measure_add_range's: blocks [blk_lo, blk_hi) of one obj_size-byte
// object, block blk_lo at src; blk_hi is clipped to the object's blocks.
inline const char *measure_plan_range(MeasurePlan *P, uint64_t src, uint64_t obj_size, uint64_t blk_lo,
                                      uint64_t blk_hi, uint64_t block_bytes) {
    *P = MeasurePlan{};
    if (const char *w = measure_block_bytes_check(block_bytes)) return w;
    uint64_t skip, len;
    if (const char *w = span_clip(src, obj_size, blk_lo, blk_hi, block_bytes, &skip, &len)) return w;
    if (len == 0) return nullptr;
    P->skip = skip;
    return measure_plan_fill(P, len, 1, block_bytes);
}

// Sub-launch (ix, iy) of a plan: objects [y0, y0 + gy), granules [x0, x0 + gx).
inline void measure_sub_launch(const MeasurePlan &P, uint64_t ix, uint64_t iy, uint64_t *x0, uint32_t *gx,
                               uint64_t *y0, uint32_t *gy) {
    span_sub_launch(P.gpo, P.n_objs, ix, iy, x0, gx, y0, gy);
}

// Bytes of pass 1's per-granule records: a 16-byte partial fingerprint and a
// 4-byte zero count each (two arrays, the counts behind the fingerprints).
inline uint64_t measure_record_bytes(uint64_t records) { return records * 16 + records * 4; }
inline uint64_t measure_record_zero_offset(uint64_t records) { return records * 16; }

// Distinct count of n fingerprints: four arrays of n 64-bit words (the low and
// high halves, in and out of the radix sort), each rounded up to 256 bytes;
// hipCUB's own scratch comes on top (asked from hipCUB at run time).
inline uint64_t measure_sort_array_bytes(uint64_t n) { return span_align256(n * 8); }
inline uint64_t measure_sort_bytes(uint64_t n) { return 4 * measure_sort_array_bytes(n); }

// The fingerprint array grows by doubling from kMeasureMinCap slots.
inline uint64_t measure_grow_cap(uint64_t cap, uint64_t need) { return span_grow_cap(cap, need); }

}  // namespace s3dg
