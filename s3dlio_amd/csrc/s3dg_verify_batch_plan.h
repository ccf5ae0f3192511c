// s3dg_verify_batch_plan.h — the host's part of s3dg_verify_controlled_batch
//  as pure functions: the argument checks with their
// messages, the pass over all descriptors that runs before the first launch,
// the sub-batch cuts, the record counts per tile size, the slot -> (object,
// block) mapping of k_verify_batch and the scratch sizes.  No HIP, no context:
// it compiles with g++ alone (tests/capi/verify_batch_plan_sweep.cpp).
//
// A verify launch needs no XCD lead (the lead orders the fill's stores), so an
// object of nb blocks takes ceil(nb / 2^tshift) records and an empty object
// none.  Nothing is squeezed out or reordered: the object index a record
// carries is the descriptor's place in its sub-batch, and per_obj is indexed
// by the caller's k.
#pragma once
#include <stdint.h>

#include "s3dg_batch_plan.h"   // kBlk, the tile-shift range, best_tile_shift and the tiled costs

#if defined(__HIPCC__)
#define S3DG_VB_HD __host__ __device__
#else
#define S3DG_VB_HD
#endif

namespace s3dg {

// sub-batches as the fill cuts them: 16 Ki objects first, doubling to 256 Ki
constexpr uint64_t kVerifySubFirst = 16384, kVerifySubMax = 262144;
// a sub-launch covers at most this many slots (the launchers' 2^22 workgroups
// per grid dimension; a multiple of every tile size)
constexpr uint64_t kVerifyMaxGrid = 1ull << 22;

// The call's pointer arguments, in the order they are refused; nullptr: fine.
inline const char *verify_batch_args(const void *src_base, const s3dg_obj_desc *d, uint64_t n, const void *out) {
    if (!out) return "null output";
    if (n == 0) return nullptr;
    if (!d) return "null descriptor array";
    if (!src_base || ((uintptr_t)src_base & 15u)) return "src_base must be 16-byte aligned";
    return nullptr;
}

// The fill's rules for one non-empty descriptor with the fill's messages
// (batch_scan, s3dg_batch_plan.h), in the fill's order; nullptr: fine.
inline const char *verify_desc_check(const s3dg_obj_desc &o) {
    if (o.dst_off & 15u) return "dst_off must be a multiple of 16";
    if (o.f_den == 0 || o.f_num >= o.f_den) return "need f_num < f_den";
    if ((o.size + kBlk - 1) / kBlk >= (1ull << 31)) return "object larger than 2^31 blocks";
    return nullptr;
}

// All n descriptors, before anything is enqueued: the first offending one
// names the refusal (msg, bad); live = non-empty objects, blocks = their 4 KiB blocks.
struct VerifyBatchCheck {
    const char *msg = nullptr;
    uint64_t bad = UINT64_MAX, live = 0, blocks = 0;
};
inline VerifyBatchCheck verify_batch_check(const s3dg_obj_desc *d, uint64_t n) {
    VerifyBatchCheck C;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_obj_desc &o = d[k];
        if (o.size == 0) continue;   // empty objects are allowed anywhere, whatever else they say
        if (const char *m = verify_desc_check(o)) {
            C.msg = m;
            C.bad = k;
            return C;
        }
        ++C.live;
        C.blocks += (o.size + kBlk - 1) / kBlk;
    }
    return C;
}

// End of the sub-batch that starts at k0; `sub` (kVerifySubFirst at k0 = 0) steps to the next one's size.
inline uint64_t verify_batch_cut(uint64_t k0, uint64_t n, uint64_t &sub) {
    const uint64_t k1 = n - k0 < sub ? n : k0 + sub;
    sub = sub * 2 < kVerifySubMax ? sub * 2 : kVerifySubMax;
    return k1;
}

// Records of an object of `size` bytes in tiles of 2^tshift blocks.
S3DG_VB_HD inline uint64_t verify_obj_tiles(uint64_t size, uint32_t tshift) {
    const uint64_t nb = (size + kBlk - 1) / kBlk;
    return (nb + (1ull << tshift) - 1) >> tshift;
}

// Slot `slot` of a launch reads record slot >> tshift; with that record's first
// block and the object's size: the slot's block, or -1 for a dead slot past
// the object's end.
S3DG_VB_HD inline int64_t verify_slot_block(uint32_t rec_first, uint64_t slot, uint32_t tshift, uint64_t size) {
    const uint64_t ib = (uint64_t)rec_first + (slot & ((1ull << tshift) - 1));
    return ib * kBlk < size ? (int64_t)ib : -1;
}

// The caller's index of the object a record names: records carry the
// descriptor's place in its sub-batch, and staging keeps every descriptor in place.
S3DG_VB_HD inline uint64_t verify_obj_index(uint64_t k0, uint32_t rec_obj) { return k0 + rec_obj; }

// One pass over sub-batch [k0, k1) of checked descriptors: staged as they are
// (out[k - k0] = d[k], empty ones too) and counted per tile size.
struct VerifyBatchScan {
    uint64_t m = 0, blocks = 0, ntiles[kTileShiftMax + 1] = {};
};
inline VerifyBatchScan verify_batch_scan(const s3dg_obj_desc *d, uint64_t k0, uint64_t k1, s3dg_obj_desc *out) {
    VerifyBatchScan P;
    for (uint64_t k = k0; k < k1; ++k) {
        const s3dg_obj_desc o = d[k];
        out[k - k0] = o;
        if (o.size == 0) continue;
        ++P.m;
        P.blocks += (o.size + kBlk - 1) / kBlk;
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) P.ntiles[sh] += verify_obj_tiles(o.size, sh);
    }
    return P;
}

// Tile size of a sub-batch: the forced one (s3dg_set_batch_tile: 2..64 blocks,
// knob = its shift) or the 8..64-block tile of least tiled cost.  The dense
// layout and the split classes tune the fill's stores and have no part here.
inline uint32_t verify_batch_tile_shift(const VerifyBatchScan &P, uint32_t knob) {
    if (knob >= kTileShiftMin && knob <= kTileShiftMax) return knob;
    return best_tile_shift(P.ntiles, P.blocks, kDeadSlotCostTiled, kRecordCostTiled);
}

// Device scratch of a call: its per-object result records (3 x u64 each).  A
// sub-batch's tile records (64 B each) live in the stream's record maps.
inline uint64_t verify_batch_obj_bytes(uint64_t n) { return n * 24; }

}  // namespace s3dg
