// s3dg_measure.h — launchers of the measure kernels (s3dg_measure.hip) for the
// C ABI over them (s3dg_measure.cpp).  DESIGN.md §5.10.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "s3dg_measure_plan.h"
#include "s3dg_span_batch_plan.h"

namespace s3dg {

// One 128-bit block fingerprint (or a granule's partial sums).
struct MeasureFp {
    uint64_t lo, hi;
};

// Pass 1: a partial fingerprint and a zero-byte count per 4 KiB granule of the
// plan's objects at src, into rec (measure_record_bytes(P.records) bytes:
// record of granule g of object j at index j * P.gpo + g).  waves: 1, 2 or 4
// wave64s per granule.
hipError_t launch_measure_granules(const MeasurePlan &P, const uint8_t *src, uint64_t stride, int waves, void *rec,
                                   hipStream_t s);
// Pass 2: the records of every block summed and finalised into fp[0, P.slots)
// (block b of object j at j * P.bpo + b); the zero counts added to *zero_total.
hipError_t launch_measure_blocks(const MeasurePlan &P, uint64_t block_bytes, const void *rec, MeasureFp *fp,
                                 uint64_t *zero_total, hipStream_t s);
// Byte histogram of the same bytes, added to hist[256]; part: scratch of
// measure_hist_part_bytes(cus) bytes, private to the stream.
uint64_t measure_hist_part_bytes(int cus);
hipError_t launch_byte_hist(const MeasurePlan &P, const uint8_t *src, uint64_t stride, int cus, void *part,
                            uint64_t *hist, hipStream_t s);
// The batch forms over an add's uploaded table
// (s3dg_span_batch_plan.h).  Pass 1: the record of granule g of entry j at
// index ents[j].g0 + g of rec (measure_record_bytes(granules) bytes), through
// ntiles tiles of 2^tshift granules; gpb: granules per full block.
hipError_t launch_measure_granules_batch(const uint8_t *src_base, const SpanTile *tiles, uint64_t ntiles,
                                         uint32_t tshift, uint64_t granules, uint32_t gpb, int waves, void *rec,
                                         hipStream_t s);
// Pass 2: block b of entry j into fp[ents[j].b0 + b].
hipError_t launch_measure_blocks_batch(const SpanEnt *ents, uint64_t live, uint64_t blocks, uint64_t granules,
                                       uint64_t block_bytes, const void *rec, MeasureFp *fp, uint64_t *zero_total,
                                       hipStream_t s);
hipError_t launch_byte_hist_batch(const uint8_t *src_base, const SpanTile *tiles, uint64_t ntiles, uint32_t tshift,
                                  int cus, void *part, uint64_t *hist, hipStream_t s);
// Distinct fingerprints among fp[0, n): two stable radix sorts on a copy in
// `work` (measure_sort_bytes(n) bytes, then *tmp_bytes of hipCUB scratch), the
// count added to *distinct (zeroed on the stream first).  work == nullptr:
// only *tmp_bytes, the hipCUB scratch n fingerprints need, is set.
hipError_t launch_measure_distinct(const MeasureFp *fp, uint64_t n, void *work, size_t *tmp_bytes,
                                   uint64_t *distinct, hipStream_t s);

}  // namespace s3dg
