// s3dg_chunks.h — launchers of the content-defined chunking kernels
// (s3dg_chunks.hip) for the C ABI over them (s3dg_chunks.cpp).  DESIGN.md §5.11.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "s3dg_chunk_plan.h"
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

// The three passes of one add, all through `scratch` (P.scratch_bytes).
// A: the candidate bitmap (bit b of word 64 g + l of an object: its byte
// 4096 g + 64 l + b is a candidate cut) and the candidates per granule, summed
// into tot[kChunkTotCandidates]; shift = 32 - bits; table: the gear values from
// 256 words of LDS, else computed per byte.  B: one wave per object walks its
// bitmap and writes the (offset, length) records of its chunks and their
// count; chunks and forced cuts are added to tot.  C: one wave per record
// slot: fp[i], flen[i] for slot i of the add (flen 0: the slot holds no chunk).
// tev: null, or four events recorded around the passes.  *step names what was
// being enqueued, for the label of a failure.
hipError_t launch_chunk_passes(const ChunkPlan &P, const ChunkSrc &src, uint32_t shift, bool table,
                               uint64_t min_bytes, uint64_t max_bytes, void *scratch, MeasureFp *fp, uint32_t *flen,
                               uint64_t *tot, hipEvent_t *tev, const char **step, hipStream_t s);
// Distinct fingerprints among the n slots and the summed length of one chunk
// each: two stable radix sorts of (key, slot index) in `work`
// (chunk_sort_bytes(n) bytes, then *tmp_bytes of hipCUB scratch), added to
// tot[kChunkTotUnique] and tot[kChunkTotUniqueBytes] (zeroed on the stream
// first).  work == nullptr: only *tmp_bytes is set.
hipError_t launch_chunk_distinct(const MeasureFp *fp, const uint32_t *flen, uint64_t n, void *work, size_t *tmp_bytes,
                                 uint64_t *tot, hipStream_t s);

}  // namespace s3dg
