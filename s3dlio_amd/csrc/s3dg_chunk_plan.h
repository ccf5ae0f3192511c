// s3dg_chunk_plan.h — the parameters and the layout of one content-defined
// chunking add (s3dg_chunks.hip) as pure functions: no HIP, no
// context, so every argument check and scratch size of s3dg_chunks_* can be
// compiled and tested on its own (tests/capi/chunk_plan_sweep.cpp,
// tests/test_chunks_cpu.py).
#pragma once
#include <stdint.h>

#include "s3dg_measure_plan.h"

namespace s3dg {

constexpr uint64_t kChunkWindow = 32;               // bytes of the window hash; smallest min_bytes
constexpr uint64_t kChunkMaxMax = 1ull << 30;       // largest max_bytes
constexpr uint64_t kChunkAvgLo = 64, kChunkAvgHi = 1ull << 24;
// Chunk slots one handle may hold: hipCUB counts the sorted items in an int.
constexpr uint64_t kChunkMaxSlots = 0x7FFFFFFFull;

// min_bytes, avg_bytes, max_bytes of s3dg_chunks_create / s3dg_chunk_data.
// Returns null and sets *bits = log2(avg_bytes), or the refusal's text.
inline const char *chunk_params_check(uint64_t min_bytes, uint64_t avg_bytes, uint64_t max_bytes, uint32_t *bits) {
    if (avg_bytes < kChunkAvgLo || avg_bytes > kChunkAvgHi || (avg_bytes & (avg_bytes - 1)))
        return "avg_bytes must be a power of two from 64 to 2^24";
    if (min_bytes < kChunkWindow) return "min_bytes must be at least 32 (the hash window)";
    if (min_bytes > max_bytes) return "min_bytes must not exceed max_bytes";
    if (max_bytes > kChunkMaxMax) return "max_bytes must be at most 2^30";
    uint32_t b = 0;
    while ((1ull << b) < avg_bytes) ++b;
    if (bits) *bits = b;
    return nullptr;
}

// One add: n_objs objects of `len` bytes each, object j at src + j*stride,
// each chunked on its own.  Pass A writes one candidate bit per byte (a
// 64-bit word per 64 bytes, 64 words per 4 KiB granule) and the number of
// candidates per granule, pass B up to rpo (offset, length) records per object
// and the object's chunk count, pass C one fingerprint slot per record slot
// (unused ones marked by length 0).
struct ChunkPlan {
    uint64_t n_objs;         // 0: an empty add, nothing is launched
    uint64_t len;            // bytes per object
    uint64_t gpo;            // 4 KiB granules per object
    uint64_t wpo;            // bitmap words per object = 64 * gpo
    uint64_t rpo;            // record (and fingerprint) slots per object = ceil(len / min_bytes) + 1
    uint64_t slots;          // n_objs * rpo
    uint64_t bytes;          // payload bytes = n_objs * len
    uint64_t granules;       // n_objs * gpo
    uint64_t nx, ny;         // pass A's sub-launches along the granules and along the objects
    // the stream's scratch: [bitmap | record offsets (8 B) | record lengths (4 B) | chunk counts (4 B per
    // object) | candidate counts (4 B per granule)]
    uint64_t off_offset, len_offset, cnt_offset, gcnt_offset, scratch_bytes;
    uint64_t own_offset;     // a batch add: behind those, the object of every record slot (4 B per slot)
};

// The scratch offsets of a plan whose n_objs, granules and slots are set.
inline void chunk_plan_scratch(ChunkPlan *P) {
    P->off_offset = P->granules * 512;                               // a multiple of 256
    P->len_offset = P->off_offset + span_align256(P->slots * 8);
    P->cnt_offset = P->len_offset + span_align256(P->slots * 4);
    P->gcnt_offset = P->cnt_offset + span_align256(P->n_objs * 4);
    P->scratch_bytes = P->gcnt_offset + span_align256(P->granules * 4);
}

// s3dg_chunks_add_stream's arguments (the refusals of
// s3dg_measure_add_stream).  Returns null and fills *P, or the refusal's text.
// An empty add (obj_size or n_objs 0) is accepted whatever the pointer.
inline const char *chunk_plan_stream(ChunkPlan *P, uint64_t src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                                     uint64_t min_bytes) {
    *P = ChunkPlan{};
    if (min_bytes < kChunkWindow || min_bytes > kChunkMaxMax) return "min_bytes out of range";
    if (obj_size == 0 || n_objs == 0) return nullptr;
    if (const char *w = span_check(src, obj_size, stride, n_objs)) return w;
    const uint64_t gpo = span_ceil_div(obj_size, kMeasureGranule);
    if (gpo > 0xFFFFFFFFull) return "object range larger than 2^32 granules";
    if (n_objs > kMeasureMaxSlots / gpo) return "more than 2^40 granules in one add";
    const uint64_t rpo = span_ceil_div(obj_size, min_bytes) + 1;
    if (n_objs > kChunkMaxSlots / rpo) return "more than 2^31 - 1 chunk slots in one add";
    P->n_objs = n_objs;
    P->len = obj_size;
    P->gpo = gpo;
    P->wpo = gpo * 64;
    P->rpo = rpo;
    P->slots = n_objs * rpo;
    P->bytes = n_objs * obj_size;
    P->granules = n_objs * gpo;
    P->nx = span_nx(gpo);
    P->ny = span_ny(n_objs);
    chunk_plan_scratch(P);
    return nullptr;
}

// A batch add (s3dg_span_batch_plan.h) of `live` non-empty spans with the
// sums of their granules, record slots and bytes: the same scratch, the
// objects' parts at their prefix sums.  len, gpo, wpo, rpo, nx and ny stay
// zero: the objects differ and the granule pass is cut by tiles.
inline void chunk_plan_batch(ChunkPlan *P, uint64_t live, uint64_t granules, uint64_t slots, uint64_t bytes) {
    *P = ChunkPlan{};
    P->n_objs = live;
    P->granules = granules;
    P->slots = slots;
    P->bytes = bytes;
    chunk_plan_scratch(P);
    P->own_offset = P->scratch_bytes;
    P->scratch_bytes += span_align256(slots * 4);
}

// Sub-launch (ix, iy) of pass A: objects [y0, y0 + gy), granules [x0, x0 + gx).
inline void chunk_sub_launch(const ChunkPlan &P, uint64_t ix, uint64_t iy, uint64_t *x0, uint32_t *gx, uint64_t *y0,
                             uint32_t *gy) {
    span_sub_launch(P.gpo, P.n_objs, ix, iy, x0, gx, y0, gy);
}

// The handle's arrays (a 16-byte fingerprint and a 4-byte length per slot)
// grow by doubling from kSpanMinCap slots, never beyond kChunkMaxSlots.
inline uint64_t chunk_grow_cap(uint64_t cap, uint64_t need) {
    uint64_t c = span_grow_cap(cap, need);
    return c > kChunkMaxSlots && need <= kChunkMaxSlots ? kChunkMaxSlots : c;
}

// Distinct count of n slots: two arrays of n 64-bit keys and two of n 32-bit
// slot indices (in and out of the radix sort), each rounded up to 256 bytes;
// hipCUB's own scratch comes on top (asked from hipCUB at run time).
inline uint64_t chunk_sort_key_bytes(uint64_t n) { return span_align256(n * 8); }
inline uint64_t chunk_sort_idx_bytes(uint64_t n) { return span_align256(n * 4); }
inline uint64_t chunk_sort_bytes(uint64_t n) { return 2 * chunk_sort_key_bytes(n) + 2 * chunk_sort_idx_bytes(n); }

}  // namespace s3dg
