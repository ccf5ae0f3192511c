// s3dg_batch.hip — device side of the batch record layout:
// the exclusive scan that turns a sub-batch's descriptors into record offsets
// (hipCUB device scan over a transform of the 40-B descriptors).  A unit apart
// from s3dg_block.hip so the library templates compile once.
#include <hipcub/hipcub.hpp>

#include "s3dg_internal.h"

namespace s3dg {
namespace {

// tile records of one object: its blocks behind `lead` dead slots (its 4 KiB
// granule mod 8), rounded up to tiles: the record rules of s3dg_batch_plan.h
struct TileCount {
    uint64_t base;
    uint32_t tshift;
    __host__ __device__ uint64_t operator()(const s3dg_obj_desc &o) const {
        return obj_tiles(obj_blocks(o.size), obj_lead(base, o.dst_off), tshift);
    }
};

// tile records of one object of a verify launch (no lead; an empty object has none)
struct VerifyTileCount {
    uint32_t tshift;
    __host__ __device__ uint64_t operator()(const s3dg_obj_desc &o) const { return verify_obj_tiles(o.size, tshift); }
};

}  // namespace

hipError_t launch_verify_batch_scan(const s3dg_obj_desc *d, uint64_t n, uint32_t tshift, uint64_t *rec_lo, void *tmp,
                                    size_t *tmp_bytes, hipStream_t s) {
    hipcub::TransformInputIterator<uint64_t, VerifyTileCount, const s3dg_obj_desc *> it(d, VerifyTileCount{tshift});
    if (n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, it, rec_lo, (int)n, s);
}

hipError_t launch_batch_scan(const s3dg_obj_desc *d, uint64_t n, uint32_t tshift, uintptr_t base, uint64_t *rec_lo,
                             void *tmp, size_t *tmp_bytes, hipStream_t s) {
    hipcub::TransformInputIterator<uint64_t, TileCount, const s3dg_obj_desc *> it(d, TileCount{(uint64_t)base, tshift});
    if (n > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, it, rec_lo, (int)n, s);
}

}  // namespace s3dg
