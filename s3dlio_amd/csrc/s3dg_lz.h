// s3dg_lz.h — launcher of the LZ4 size kernel (s3dg_lz.hip) for the C ABI over
// it (s3dg_lz.cpp).  DESIGN.md §5.12.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "s3dg_lz_plan.h"
#include "s3dg_span_batch_plan.h"

namespace s3dg {

// Words of the handle's device totals: s3dg_lz_result's fields, in order.
enum { kLzTotBytes, kLzTotBlocks, kLzTotLz, kLzTotStored, kLzTotRaw, kLzTotMatches, kLzTotMatchBytes, kLzTotLiterals };

// Once per device before the first launch: lets k_lz take lz_lds_bytes(65536).
hipError_t lz_kernel_prepare();
// The greedy LZ4 parse of every block of the plan's objects at src; the sums
// of the eight result fields are added to tot[kLzTotWords], one set of vector
// atomics per wave of the grid (lz_grid).
hipError_t launch_lz(const LzPlan &P, const uint8_t *src, uint64_t stride, uint64_t block_bytes, int cus,
                     uint64_t *tot, hipStream_t s);
// The batch form: the add's `blocks` blocks over the `live`
// entries of its uploaded table, block b of entry j at src_base + off_j + b * block_bytes.
hipError_t launch_lz_batch(const uint8_t *src_base, const SpanEnt *ents, uint64_t live, uint64_t blocks,
                           uint64_t block_bytes, int cus, uint64_t *tot, hipStream_t s);

}  // namespace s3dg
