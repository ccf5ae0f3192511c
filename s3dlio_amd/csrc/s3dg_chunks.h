// s3dg_chunks.h — launchers of the content-defined chunking kernels
// (s3dg_chunks.hip) for the C ABI over them (s3dg_chunks.cpp).  DESIGN.md §5.11.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "s3dg_chunk_plan.h"
#include "s3dg_chunk_search_plan.h"
#include "s3dg_measure.h"

namespace s3dg {

// The handle's device totals (64-bit words).
enum { kChunkTotCandidates = 0, kChunkTotForced, kChunkTotChunks, kChunkTotUnique, kChunkTotUniqueBytes, kChunkTotWords };

// Where an add's objects are.  The stream form (ents null): P.n_objs objects
// of P.len bytes, `stride` apart from base on.  The batch form (DESIGN.md
// §5.13): the add's uploaded table (s3dg_span_batch_plan.h), offsets from base,
// P from chunk_plan_batch; granule g of entry j owns bitmap words from
// 64 (g0_j + g), entry j's records and slots start at s0_j.
struct ChunkSrc {
    const uint8_t *base;
    uint64_t stride;
    const SpanEnt *ents;
    const SpanTile *tiles;
    uint64_t ntiles;
    uint32_t tshift;
};

// An add whose objects of at least `threshold` bytes take the parallel cut walk
// (S3DG_CHUNKS_SEARCH_WALK): its part of the scratch, behind
// the plan's, and the bytes of hipCUB scratch in it.
struct ChunkSearch {
    uint64_t threshold;
    CsPlan plan;
    size_t tmp_bytes;
};

// The three passes of one add, all through `scratch` (P.scratch_bytes, or Q->plan.end).
// A: the candidate bitmap (bit b of word 64 g + l of an object: its byte
// 4096 g + 64 l + b is a candidate cut) and the candidates per granule, summed
// into tot[kChunkTotCandidates]; shift = 32 - bits; table: the gear values from
// 256 words of LDS, else computed per byte.  B: one wave per object walks its
// bitmap and writes the (offset, length) records of its chunks and their
// count; chunks and forced cuts are added to tot.  C: one wave per record
// slot: fp[i], flen[i] for slot i of the add (flen 0: the slot holds no chunk).
// Q not null: pass B is launch_chunk_search for the objects it takes and the
// wave per object for the rest, in the same add.
// tev: null, or four events recorded around the passes.  *step names what was
// being enqueued, for the label of a failure.
hipError_t launch_chunk_passes(const ChunkPlan &P, const ChunkSrc &src, uint32_t shift, bool table,
                               uint64_t min_bytes, uint64_t max_bytes, void *scratch, MeasureFp *fp, uint32_t *flen,
                               uint64_t *tot, hipEvent_t *tev, const char **step, hipStream_t s, const ChunkSearch *Q = nullptr,
                               uint64_t avg_bytes = 0);
// The parallel form of pass B (s3dg_chunk_search.hip) over pass A's bitmap and
// counts: the records, counts and totals of every object that CsObj.take marks
// in the table it leaves at Q.plan.obj_off; the others are left to chunk_walk.
hipError_t launch_chunk_search(const ChunkPlan &P, const ChunkSrc &src, const ChunkSearch &Q, uint64_t min_bytes,
                               uint64_t avg_bytes, uint64_t max_bytes, void *scratch, uint64_t *tot, hipStream_t s);
// hipCUB's scratch for the two sums of such an add.
hipError_t chunk_search_tmp_bytes(uint64_t n_objs, uint64_t granules, size_t *bytes);
// Distinct fingerprints among the n slots and the summed length of one chunk
// each: two stable radix sorts of (key, slot index) in `work`
// (chunk_sort_bytes(n) bytes, then *tmp_bytes of hipCUB scratch), added to
// tot[kChunkTotUnique] and tot[kChunkTotUniqueBytes] (zeroed on the stream
// first).  work == nullptr: only *tmp_bytes is set.
hipError_t launch_chunk_distinct(const MeasureFp *fp, const uint32_t *flen, uint64_t n, void *work, size_t *tmp_bytes,
                                 uint64_t *tot, hipStream_t s);

}  // namespace s3dg
