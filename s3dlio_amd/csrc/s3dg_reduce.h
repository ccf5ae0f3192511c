// s3dg_reduce.h — launchers of the dedup-then-compress kernels
// (s3dg_reduce.hip) for the C ABI over them (s3dg_reduce.cpp).  DESIGN.md §5.14.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "s3dg_measure.h"
#include "s3dg_reduce_plan.h"
#include "s3dg_span_batch_plan.h"

namespace s3dg {

// What pass 2 of every add shares: the handle's kept fingerprints, its claim
// table of `slots` slots and its totals (kReduceTotWords).
struct ReduceState {
    const MeasureFp *fp;
    uint64_t *table;
    uint64_t slots;
    uint64_t *tot;
};

// Once per device before the first launch: lets k_reduce take lz_lds_bytes(65536).
hipError_t reduce_kernel_prepare();
// Pass 2 of a stream or range add: block i of the plan's objects at src has the
// fingerprint R.fp[fp0 + i] (pass 1 wrote it on the same stream).  A wave
// claims the fingerprint in R.table and parses the block only when the claim
// is new; the sums over the new blocks are added to R.tot, one set of vector
// atomics per wave of the grid (lz_grid).
hipError_t launch_reduce(const LzPlan &P, const uint8_t *src, uint64_t stride, uint64_t block_bytes, int cus,
                         const ReduceState &R, uint64_t fp0, hipStream_t s);
// The batch form: block b of entry j at src_base + off_j +
// b * block_bytes, its fingerprint at R.fp[fp0 + ents[j].b0 + b].
hipError_t launch_reduce_batch(const uint8_t *src_base, const SpanEnt *ents, uint64_t live, uint64_t blocks,
                               uint64_t block_bytes, int cus, const ReduceState &R, uint64_t fp0, hipStream_t s);
// Every index of old_table[0, old_slots) entered into R.table (zeroed, larger)
// by the fingerprint it stands for.
hipError_t launch_reduce_rebuild(const uint64_t *old_table, uint64_t old_slots, const ReduceState &R, hipStream_t s);

}  // namespace s3dg
