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

// Pass A: the candidate bitmap of the plan's objects at src, into scratch
// (bit b of word 64 g + l of object j: byte 4096 g + 64 l + b is a candidate
// cut); their number per granule too, summed into tot[kChunkTotCandidates].  shift = 32 - bits.
// table: the gear values from 256 words of LDS, else computed per byte.
hipError_t launch_chunk_candidates(const ChunkPlan &P, const uint8_t *src, uint64_t stride, uint32_t shift, bool table,
                                   void *scratch, uint64_t *tot, hipStream_t s);
// Pass B: one wave per object walks its bitmap and writes the (offset, length)
// records of its chunks and their count into scratch; chunks and forced cuts
// are added to tot.
hipError_t launch_chunk_cuts(const ChunkPlan &P, uint64_t min_bytes, uint64_t max_bytes, void *scratch, uint64_t *tot,
                             hipStream_t s);
// Pass C: one wave per record slot: fp[i], flen[i] for slot i of the add
// (flen 0: the slot holds no chunk).
hipError_t launch_chunk_fingerprints(const ChunkPlan &P, const uint8_t *src, uint64_t stride, const void *scratch,
                                     MeasureFp *fp, uint32_t *flen, hipStream_t s);
// The batch form of the three passes over an add's uploaded
// table (s3dg_span_batch_plan.h): P from chunk_plan_batch; granule g of entry j
// owns bitmap words from 64 (g0_j + g), entry j's records and slots start at
// s0_j.  tev: null, or four events recorded around the passes.
hipError_t launch_chunk_batch(const ChunkPlan &P, const uint8_t *src_base, const SpanEnt *ents, const SpanTile *tiles,
                              uint64_t ntiles, uint32_t tshift, uint32_t shift, bool table, uint64_t min_bytes,
                              uint64_t max_bytes, void *scratch, MeasureFp *fp, uint32_t *flen, uint64_t *tot,
                              hipEvent_t *tev, hipStream_t s);
// Distinct fingerprints among the n slots and the summed length of one chunk
// each: two stable radix sorts of (key, slot index) in `work`
// (chunk_sort_bytes(n) bytes, then *tmp_bytes of hipCUB scratch), added to
// tot[kChunkTotUnique] and tot[kChunkTotUniqueBytes] (zeroed on the stream
// first).  work == nullptr: only *tmp_bytes is set.
hipError_t launch_chunk_distinct(const MeasureFp *fp, const uint32_t *flen, uint64_t n, void *work, size_t *tmp_bytes,
                                 uint64_t *tot, hipStream_t s);

}  // namespace s3dg
