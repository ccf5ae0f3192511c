// s3dg_span_plan.h — what the plans of the read-only analyses share
// (s3dg_measure_plan.h, s3dg_chunk_plan.h, s3dg_lz_plan.h; DESIGN.md
// §5.10-5.12): the checks of a span of strided objects, the clip of a block
// range, the split of a (granules x objects) grid into sub-launches, and the
// sizes they round and grow by.  Pure functions: no HIP, no context
// (tests/capi/span_plan_sweep.cpp).
#pragma once
#include <stdint.h>

namespace s3dg {

constexpr uint64_t kSpanMaxGridX = 1ull << 22;   // granules of one object per sub-launch
constexpr uint64_t kSpanMaxGridY = 65535;        // objects per sub-launch
constexpr uint64_t kSpanMinCap = 4096;           // slots a handle's arrays start at
// A host slot's staging chunk: the size of each HostStaging::buf, so the most
// a host-buffer form copies at once.
constexpr uint64_t kStagingChunk = 64ull << 20;

inline uint64_t span_ceil_div(uint64_t n, uint64_t unit) { return n / unit + (n % unit != 0); }
inline uint64_t span_align256(uint64_t n) { return (n + 255) / 256 * 256; }

// n_objs > 0 objects of obj_size > 0 bytes, object j at src + j*stride.
inline const char *span_check(uint64_t src, uint64_t obj_size, uint64_t stride, uint64_t n_objs) {
    if (!src || (src & 15u) || (stride & 15u)) return "src and stride must be 16-byte aligned";
    if (n_objs > 1 && stride < obj_size) return "stride < obj_size: objects overlap";
    return nullptr;
}

// Blocks [blk_lo, blk_hi) of one obj_size-byte object, block blk_lo at src;
// blk_hi is clipped to the object's blocks.  Sets the range's bytes
// [*skip, *skip + *len) of the object: *len == 0 for an empty range, which is
// accepted whatever the pointer.
inline const char *span_clip(uint64_t src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi, uint64_t block_bytes,
                             uint64_t *skip, uint64_t *len) {
    *skip = *len = 0;
    const uint64_t nb = span_ceil_div(obj_size, block_bytes);
    if (blk_hi > nb) blk_hi = nb;
    if (blk_lo >= blk_hi) return nullptr;
    if (!src || (src & 15u)) return "src must be a 16-byte aligned device pointer";
    *skip = blk_lo * block_bytes;                                   // < obj_size
    *len = (blk_hi == nb ? obj_size : blk_hi * block_bytes) - *skip;
    return nullptr;
}

// Sub-launches along the granules of an object and along the objects.
inline uint64_t span_nx(uint64_t gpo) { return (gpo + kSpanMaxGridX - 1) / kSpanMaxGridX; }
inline uint64_t span_ny(uint64_t n_objs) { return (n_objs + kSpanMaxGridY - 1) / kSpanMaxGridY; }
// Sub-launch (ix, iy) of n_objs objects of gpo granules: objects
// [y0, y0 + gy), granules [x0, x0 + gx).
inline void span_sub_launch(uint64_t gpo, uint64_t n_objs, uint64_t ix, uint64_t iy, uint64_t *x0, uint32_t *gx,
                            uint64_t *y0, uint32_t *gy) {
    *x0 = ix * kSpanMaxGridX;
    *y0 = iy * kSpanMaxGridY;
    const uint64_t rx = gpo - *x0, ry = n_objs - *y0;
    *gx = (uint32_t)(rx < kSpanMaxGridX ? rx : kSpanMaxGridX);
    *gy = (uint32_t)(ry < kSpanMaxGridY ? ry : kSpanMaxGridY);
}

// A handle's arrays grow by doubling from kSpanMinCap slots.
inline uint64_t span_grow_cap(uint64_t cap, uint64_t need) {
    uint64_t c = cap < kSpanMinCap ? kSpanMinCap : cap;
    while (c < need) c *= 2;
    return c;
}

// Grid of a grid-stride kernel over n items: up to 2048 workgroups of 256.
inline uint32_t span_grid_for(uint64_t n) {
    const uint64_t g = (n + 255) / 256;
    return (uint32_t)(g < 2048 ? (g ? g : 1) : 2048);
}

}  // namespace s3dg
