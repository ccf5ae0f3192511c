// s3dg_crc_batch_plan.h — the host's part of s3dg_crc32_batch (DESIGN.md
// §5.4.1) as pure functions: the region size of a call, the regions of every
// object with their records, the entries the fold walks, and the CRC algebra
// of that fold as host-and-device functions, so a CPU sweep runs the very
// code the fold kernel runs.  No HIP, no context: it compiles with g++ alone
// (tests/capi/crc_batch_plan_sweep.cpp).  The spans are checked by
// span_batch_check (s3dg_span_batch_plan.h) as the batch adds check theirs.
//
// An object is cut into regions of `rows` whole 1 KiB rows; the size % 1024
// bytes after its last row (the tail) belong to its last region, and an object
// shorter than one row is one region of no rows.  One wave hashes one region
// from a zero register (its raw CRC); the fold combines an object's raws in
// order.  raw(M) is linear in M over GF(2) and A^n ("advance n zero bytes") is
// multiplication by x^(8n) mod P, so
//   raw(M1 || M2) = A^|M2| raw(M1) ^ raw(M2),   crc32(M) = ~(A^|M| (~0) ^ raw(M)).
#pragma once
#include <stdint.h>

#include "s3dg_span_batch_plan.h"

#if defined(__HIPCC__)
#define S3DG_CB_HD __host__ __device__
#else
#define S3DG_CB_HD
#endif

namespace s3dg {

constexpr uint32_t kCrcRowBytes = 1024;
// Region size of a call (crc_seg_plan's rule): 256 rows, or, when that leaves
// fewer than one region per resident wave, the call's whole rows over the
// resident waves, at least 32.  Not a power of two in general.
constexpr uint32_t kCrcBatchMinRows = 32, kCrcBatchMaxRows = 256;
constexpr uint64_t kCrcBatchWaves = 4096;
// An object of more regions doubles its own region until it has at most this
// many: one thread folds an object, so this bounds its serial work.
constexpr uint64_t kCrcBatchMaxRegions = 4096;

// One region: `rows` whole rows from src_base + off, then `tail` bytes.
struct CrcBatchRec {
    uint64_t off;
    uint32_t rows;
    uint32_t tail;   // < 1024; non-zero only in an object's last region
    uint32_t ent;    // the entry that owns it
    uint32_t pad;
};
static_assert(sizeof(CrcBatchRec) == 24, "CrcBatchRec is 24 bytes");

// One non-empty span: regions [reg0, reg0 + nreg) of the call, all of `rows`
// rows but the last, which holds what is left; k is the caller's index.
struct CrcBatchEnt {
    uint64_t size;
    uint64_t reg0;
    uint64_t k;
    uint32_t nreg;
    uint32_t rows;
};
static_assert(sizeof(CrcBatchEnt) == 32, "CrcBatchEnt is 32 bytes");

struct CrcBatchCounts {
    uint64_t live = 0;         // non-empty spans
    uint64_t total_rows = 0;   // their whole rows
    uint64_t regions = 0;
    uint32_t rows = 0;         // the call's region, in rows
};

inline uint32_t crc_batch_region_rows(uint64_t total_rows) {
    if (total_rows / kCrcBatchMaxRows >= kCrcBatchWaves) return kCrcBatchMaxRows;
    const uint64_t r = total_rows / kCrcBatchWaves;
    return (uint32_t)(r < kCrcBatchMinRows ? kCrcBatchMinRows : r);
}

// The region of one object of a call whose region is `rows`: doubled until the
// object has at most kCrcBatchMaxRegions.  size <= kSpanBatchMaxObj = 2^33
// rows, so the result is at most 2^21.
inline uint32_t crc_batch_obj_rows(uint64_t size, uint32_t rows) {
    const uint64_t obj_rows = size / kCrcRowBytes;
    uint64_t r = rows;
    while (span_ceil_div(obj_rows, r) > kCrcBatchMaxRegions) r *= 2;
    return (uint32_t)r;
}
inline uint64_t crc_batch_obj_regions(uint64_t size, uint32_t obj_region_rows) {
    const uint64_t n = span_ceil_div(size / kCrcRowBytes, obj_region_rows);
    return n ? n : 1;   // shorter than a row: one region of its bytes alone
}

// What a call of checked spans takes.
inline CrcBatchCounts crc_batch_count(const s3dg_span *spans, uint64_t n) {
    CrcBatchCounts C;
    for (uint64_t k = 0; k < n; ++k) {
        if (spans[k].size == 0) continue;
        ++C.live;
        C.total_rows += spans[k].size / kCrcRowBytes;
    }
    C.rows = crc_batch_region_rows(C.total_rows);
    for (uint64_t k = 0; k < n; ++k)
        if (spans[k].size) C.regions += crc_batch_obj_regions(spans[k].size, crc_batch_obj_rows(spans[k].size, C.rows));
    return C;
}

// The uploaded table: [entries | records]; the device copy has the regions'
// raw CRCs behind it, at a multiple of 256 bytes.
inline uint64_t crc_batch_rec_offset(uint64_t live) { return live * sizeof(CrcBatchEnt); }
inline uint64_t crc_batch_table_bytes(const CrcBatchCounts &C) {
    return crc_batch_rec_offset(C.live) + C.regions * sizeof(CrcBatchRec);
}
inline uint64_t crc_batch_raw_offset(const CrcBatchCounts &C) { return span_align256(crc_batch_table_bytes(C)); }
inline uint64_t crc_batch_device_bytes(const CrcBatchCounts &C) { return crc_batch_raw_offset(C) + C.regions * 4; }

// ents[0, C.live) in the caller's order and recs[0, C.regions), an object's
// regions in a row.
inline void crc_batch_build(const s3dg_span *spans, uint64_t n, const CrcBatchCounts &C, CrcBatchEnt *ents,
                            CrcBatchRec *recs) {
    uint64_t j = 0, r = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_span p = spans[k];
        if (p.size == 0) continue;
        const uint32_t rows = crc_batch_obj_rows(p.size, C.rows);
        const uint64_t nreg = crc_batch_obj_regions(p.size, rows), obj_rows = p.size / kCrcRowBytes;
        ents[j] = CrcBatchEnt{p.size, r, k, (uint32_t)nreg, rows};
        for (uint64_t q = 0; q < nreg; ++q) {
            const uint64_t row0 = q * rows;
            const bool last = q + 1 == nreg;
            recs[r++] = CrcBatchRec{p.off + row0 * kCrcRowBytes, (uint32_t)(last ? obj_rows - row0 : rows),
                                    last ? (uint32_t)(p.size % kCrcRowBytes) : 0u, (uint32_t)j, 0u};
        }
        ++j;
    }
}

// ---- the fold's algebra --------------------------------------------------------
constexpr uint32_t kCrcBatchPoly = 0xEDB88320u;

// a * b mod P in the reflected representation (x^0 = 0x80000000), as zlib's
// multmodp.  Always 32 steps and no branch on the data: the lanes of the fold
// kernel hold different objects and would diverge at every early exit.
S3DG_CB_HD inline uint32_t crcb_multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (kCrcBatchPoly & (0u - (b & 1)));
    }
    return p;
}

// x^(8 n) mod P by square-and-multiply over the bits of 8 n; n < 2^61.
S3DG_CB_HD inline uint32_t crcb_x8n(uint64_t n) {
    uint32_t p = 1u << 31, sq = 1u << 30;   // x^0, x^1
    for (uint64_t e = n * 8; e; e >>= 1) {
        if (e & 1) p = crcb_multmodp(sq, p);
        sq = crcb_multmodp(sq, sq);
    }
    return p;
}

// The CRC-32 of an object of `size` bytes from its regions' raw CRCs, in
// order: nreg regions of `rows` rows, the last one holding what is left.
S3DG_CB_HD inline uint32_t crcb_fold(const uint32_t *raw, uint32_t nreg, uint32_t rows, uint64_t size) {
    const uint64_t region = (uint64_t)rows * kCrcRowBytes;
    uint32_t acc = 0;
    if (nreg > 1) {
        const uint32_t xr = crcb_x8n(region);
        for (uint32_t q = 0; q + 1 < nreg; ++q) acc = crcb_multmodp(xr, acc) ^ raw[q];
        acc = crcb_multmodp(crcb_x8n(size - (uint64_t)(nreg - 1) * region), acc);
    }
    acc ^= raw[nreg - 1];
    return ~(crcb_multmodp(crcb_x8n(size), 0xFFFFFFFFu) ^ acc);
}

}  // namespace s3dg
