// s3dg_reduce_plan.h — the claim table of the dedup-then-compress measurement
// (k_reduce) as pure functions: no HIP, no context, so its
// capacity rule can be compiled and tested on its own
// (tests/test_reduce_cpu.py).  An add's layout is s3dg_lz_plan.h's (pass 2) and
// s3dg_measure_plan.h's (pass 1).
#pragma once
#include <stdint.h>

#include "s3dg_lz_plan.h"

#if defined(__HIPCC__)
#define S3DG_RD_HD __host__ __device__
#else
#define S3DG_RD_HD
#endif

namespace s3dg {

constexpr uint64_t kReduceInitialSlots = 4096;    // the table a handle starts with
constexpr uint64_t kReduceSlotBytes = 8;          // a slot: the index + 1 of a kept fingerprint, 0 = empty
constexpr uint64_t kReduceMaxBlocks = 1ull << 40; // fingerprints one handle may hold
constexpr int kReduceTotWords = 9;                // the device totals, below

// Words of the handle's device totals: over the distinct blocks, then pass 1's
// zero-byte count (the measure launches add it; the result has no field for it).
enum {
    kRedTotUniqueBlocks, kRedTotUniqueBytes, kRedTotLz, kRedTotStored, kRedTotRaw, kRedTotMatches, kRedTotMatchBytes,
    kRedTotLiterals, kRedTotZero
};

// The table's slots once the handle holds `blocks` blocks (those of the add
// about to be launched included): a power of two, never smaller than `slots`,
// at least twice `blocks`.  Every block claims at most one slot, so a table is
// never more than half full and every probe ends at an empty slot or at the
// block's own fingerprint.
inline uint64_t reduce_table_slots(uint64_t slots, uint64_t blocks) {
    uint64_t c = slots < kReduceInitialSlots ? kReduceInitialSlots : slots;
    while (c < 2 * blocks) c *= 2;
    return c;
}

// Where a fingerprint's probe starts in a table of `slots` (a power of two)
// and where it goes next: the low bits of the fingerprint's low half, which
// fp_final passed through fmix64, then linearly.
S3DG_RD_HD inline uint64_t reduce_probe_start(uint64_t fp_lo, uint64_t slots) { return fp_lo & (slots - 1); }
S3DG_RD_HD inline uint64_t reduce_probe_next(uint64_t q, uint64_t slots) { return (q + 1) & (slots - 1); }

}  // namespace s3dg
