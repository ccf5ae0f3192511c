// s3dg_lz_plan.h — the layout of one LZ add (k_lz) as pure
// functions: no HIP, no context, so every argument check of s3dg_lz_* can be
// compiled and tested on its own (tests/capi/lz_plan_sweep.cpp,
// tests/test_lz_cpu.py).
#pragma once
#include <stdint.h>

#include "s3dg_span_plan.h"

namespace s3dg {

constexpr uint64_t kLzGranule = 4096;             // block_bytes is a multiple of this
constexpr uint64_t kLzMaxBlock = 65536;           // every match offset fits LZ4's 16 bits
constexpr uint64_t kLzTableBytes = 4096 * 2;      // the hash table: 4096 entries of 16 bits
constexpr uint64_t kLzCuLds = 160 * 1024;         // LDS of one gfx950 CU
constexpr uint64_t kLzMaxWavesPerCu = 32;
constexpr uint64_t kLzMaxBlocks = 1ull << 40;     // blocks of one add
constexpr uint64_t kLzMaxGrid = 0x7FFFFFFFull;
constexpr uint64_t kLzHostChunk = kStagingChunk;  // a host slot's staging chunk
constexpr int kLzTotWords = 8;                    // s3dg_lz_result's fields, in order

// block_bytes: a multiple of 4096 from 4096 to 65536.
inline const char *lz_block_bytes_check(uint64_t block_bytes) {
    if (block_bytes == 0 || block_bytes % kLzGranule || block_bytes > kLzMaxBlock)
        return "block_bytes must be a multiple of 4096 from 4096 to 65536";
    return nullptr;
}

// One add: n_objs object ranges of `len` bytes each (len > 0 unless the add is
// empty), range j at src + j*stride, each cut into blocks of block_bytes from
// its start (the last one may be ragged).
struct LzPlan {
    uint64_t n_objs;       // 0: an empty add, nothing is launched
    uint64_t len;          // bytes measured per object
    uint64_t bpo;          // blocks per object
    uint64_t last_block;   // length of an object's last block, in (0, block_bytes]
    uint64_t blocks;       // n_objs * bpo: the wave's work items, block i = object i / bpo, its block i % bpo
};

inline const char *lz_plan_fill(LzPlan *P, uint64_t len, uint64_t n_objs, uint64_t block_bytes) {
    P->n_objs = n_objs;
    P->len = len;
    P->bpo = span_ceil_div(len, block_bytes);
    if (n_objs > kLzMaxBlocks / P->bpo) return "more than 2^40 blocks in one add";
    P->last_block = len - (P->bpo - 1) * block_bytes;
    P->blocks = n_objs * P->bpo;
    return nullptr;
}

// s3dg_lz_add_stream's arguments.  Returns null and fills *P, or the
// refusal's text (S3DG_EINVAL).  An empty add (obj_size or n_objs 0) is
// accepted whatever the pointer: P->n_objs == 0.
inline const char *lz_plan_stream(LzPlan *P, uint64_t src, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                                  uint64_t block_bytes) {
    *P = LzPlan{};
    if (const char *w = lz_block_bytes_check(block_bytes)) return w;
    if (obj_size == 0 || n_objs == 0) return nullptr;
    if (const char *w = span_check(src, obj_size, stride, n_objs)) return w;
    if (obj_size > (1ull << 56)) return "object larger than 2^56 bytes";
    return lz_plan_fill(P, obj_size, n_objs, block_bytes);
}

// s3dg_lz_add_range's: blocks [blk_lo, blk_hi) of one obj_size-byte object,
// block blk_lo at src; blk_hi is clipped to the object's blocks.
inline const char *lz_plan_range(LzPlan *P, uint64_t src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                                 uint64_t block_bytes) {
    *P = LzPlan{};
    if (const char *w = lz_block_bytes_check(block_bytes)) return w;
    uint64_t skip, len;
    if (const char *w = span_clip(src, obj_size, blk_lo, blk_hi, block_bytes, &skip, &len)) return w;
    return len ? lz_plan_fill(P, len, 1, block_bytes) : nullptr;
}

// One wave (a workgroup of its own) per block at a time: the block staged in
// LDS in front of the table.
inline uint64_t lz_lds_bytes(uint64_t block_bytes) { return block_bytes + kLzTableBytes; }
// Workgroups of one CU that hold their LDS at once: 13 at 4 KiB, 2 at 64 KiB.
inline uint64_t lz_waves_per_cu(uint64_t block_bytes) {
    const uint64_t w = kLzCuLds / lz_lds_bytes(block_bytes);
    return w < kLzMaxWavesPerCu ? w : kLzMaxWavesPerCu;
}
// The grid: one resident set of waves, each walking blocks i, i + grid, ...
// with a 64-bit index, so no add is split along objects or blocks.
inline uint64_t lz_grid(uint64_t blocks, uint64_t block_bytes, int cus) {
    const uint64_t g = (uint64_t)(cus > 0 ? cus : 256) * lz_waves_per_cu(block_bytes);
    return blocks < g ? blocks : (g < kLzMaxGrid ? g : kLzMaxGrid);
}

// s3dg_lz_data: whole blocks per staging chunk, and the chunk's bytes.
inline uint64_t lz_host_chunk_blocks(uint64_t block_bytes) { return kLzHostChunk / block_bytes; }

}  // namespace s3dg
