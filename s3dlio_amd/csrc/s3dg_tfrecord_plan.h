// s3dg_tfrecord_plan.h — the host's part of s3dg_tfrecord_frame_batch and
// s3dg_tfrecord_check_batch as pure functions: the checks of
// the shard descriptors with their messages, the one table entry per shard, how
// a record is cut into regions, which writer owns each byte of a stream, and
// the fold of a record's raw CRCs, as host-and-device functions, so a CPU sweep
// runs the very code the kernels run.  No HIP, no context: it compiles with
// g++ alone (tests/capi/tfrecord_plan_sweep.cpp).
//
// A shard is `records` records of `record_size` payload bytes; record i is
// framed as  u64 len | masked_crc(len) | data | masked_crc(data)  at
// i * (16 + record_size) of the stream (src/data_formats/tfrecord.rs:10-75).
//
// The padded record.  Record i's data starts `a` bytes past a 16-byte boundary
// (frame: a = i rs mod 16 in the source; check: a = 12 + i rs mod 16 in the
// stream).  A zero register stays zero over zero bytes, so raw(0^a || data) =
// raw(data): a wave hashes the record as the L = a + rs bytes from that
// boundary with the first a bytes masked to zero, and everything after the
// first 16-byte piece is what k_crc32_batch_regions hashes: aligned 16-byte
// row loads, whole tail pieces, the last e bytes one by one.  The a bytes
// before the data lie inside the shard (the record before, or this record's
// header in the check form), never before it: a != 0 needs i rs >= a.
//
// Regions.  A record's padded rows (whole KiB of L) are cut into regions of
// `rows` rows.  Every record of a shard has rpr regions, from the shard's
// longest possible L = rs + 15: all but the last hold `rows` rows, the last
// one holds the rows that are left (possibly none) and the L mod 1024 tail
// bytes.  A region never spans two records.  rpr == 1: the wave finishes the
// record (mask, header, footer, index entry); otherwise a fold launch of one
// thread per record does.
//
// Bytes of the stream and their writers (frame form).  Padded offset y of a
// record goes to stream offset i (16 + rs) + 12 + y - a: the two differ by
// 12 (mod 16) for every record.  Region g's wave writes the data bytes of its
// padded span [max(a, g rows 1024), end of region); the record's finisher
// writes the 12 header bytes and the 4 footer bytes.  No byte has two writers.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "s3dg_crc_batch_plan.h"
#include "s3dlio_gpu.h"

namespace s3dg {

constexpr uint64_t kTfrFraming = 16, kTfrHeader = 12;
constexpr uint64_t kTfrMaxRecord = kSpanBatchMaxObj;     // the span limit of the batch adds
constexpr uint64_t kTfrMaxBytes = 1ull << 46;            // framed bytes of one call: the fold grid fits 32 bits
constexpr uint64_t kTfrMaxShards = 0xFFFFFFFFull;        // an entry names its shard in 32 bits

// One shard with records: what a wave needs to find its record and region by
// division.  The uploaded table is these alone.
struct TfrShard {
    uint64_t src_off, dst_off, idx_off;
    uint64_t records, record_size;
    uint64_t reg0;      // its first region among the call's regions
    uint64_t lrec0;     // its first record among the records of shards with rpr > 1
    uint64_t raw0;      // its first raw slot (rpr per record) when rpr > 1
    uint32_t rpr;       // regions per record
    uint32_t rows;      // rows of a region
    uint32_t k;         // the caller's index
    uint32_t init;      // A^rs (~0): crc32(data) = ~(init ^ raw(data))
    uint32_t len_mcrc;  // masked_crc of the 8 length bytes
    uint32_t pad;
};
static_assert(sizeof(TfrShard) == 88, "TfrShard is 88 bytes");

struct TfrCounts {
    uint64_t live = 0;           // shards with records
    uint64_t regions = 0;
    uint64_t long_records = 0;   // records of shards with rpr > 1
    uint64_t raw_slots = 0;      // their regions
    uint64_t total_rows = 0;
    uint32_t rows = 0;           // the call's region, in rows
};

// One record's region as the wave walks it.
struct TfrRegion {
    uint64_t rec;       // record index within the shard
    uint64_t data;      // frame: source offset of the record's data from src_base; check: stream offset from base
    uint64_t out;       // offset of the record's first framed byte (its header) from the destination / check base
    uint64_t pad_lo;    // first padded offset of this region (a multiple of 1024)
    uint32_t g;         // region within the record
    uint32_t a;         // bytes from the 16-byte boundary to the data
    uint32_t nrows;     // whole rows of this region
    uint32_t tail;      // bytes after them (< 1024; last region only)
};

S3DG_CB_HD inline uint32_t tfr_masked(uint32_t crc) { return ((crc >> 15) | (crc << 17)) + 0xA282EAD8u; }

// CRC-32 of a few bytes, bit by bit (the 8 length bytes of a shard).
S3DG_CB_HD inline uint32_t tfr_crc_small(const uint8_t *p, uint32_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (kCrcBatchPoly & (0u - (c & 1)));
    }
    return ~c;
}
inline uint32_t tfr_len_mcrc(uint64_t record_size) {
    uint8_t lb[8];
    for (int b = 0; b < 8; ++b) lb[b] = (uint8_t)(record_size >> (8 * b));
    return tfr_masked(tfr_crc_small(lb, 8));
}

inline bool tfr_size(uint64_t records, uint64_t record_size, uint64_t *out) {
    if (record_size > UINT64_MAX - kTfrFraming) return false;
    const uint64_t per = record_size + kTfrFraming;
    if (records && per > UINT64_MAX / records) return false;
    *out = records * per;
    return true;
}

// Regions per record of a shard whose call region is `rows`: from the longest
// padded record, the region doubled until a record has at most
// kCrcBatchMaxRegions (crc_batch_obj_rows' rule).
inline uint32_t tfr_shard_rows(uint64_t record_size, uint32_t rows) {
    return crc_batch_obj_rows(record_size + 15, rows);
}
inline uint32_t tfr_shard_rpr(uint64_t record_size, uint32_t shard_rows) {
    return (uint32_t)crc_batch_obj_regions(record_size + 15, shard_rows);
}

inline std::string tfr_at(uint64_t k, const char *what) {
    char b[160];
    snprintf(b, sizeof(b), "shard %llu: %s", (unsigned long long)k, what);
    return b;
}

// All of a call's arguments, before anything is reserved or enqueued.  frame:
// src_base, dst_base and (nullable) idx_base with src_off, dst_off, idx_off;
// check: dst_base alone with dst_off.  Shards without records are not looked
// at.  Returns true and fills *C, or false with the refusal's text in *why.
inline bool tfr_check(bool frame, uint64_t src_base, uint64_t dst_base, uint64_t idx_base,
                      const s3dg_tfrecord_shard *shards, uint64_t n, TfrCounts *C, std::string *why) {
    *C = TfrCounts{};
    if (n == 0) return true;
    if (!shards) return *why = "null shard array", false;
    if (frame && (!src_base || (src_base & 15u))) return *why = "src_base must be a 16-byte aligned device pointer", false;
    if (!dst_base || (dst_base & 15u))
        return *why = frame ? "dst_base must be a 16-byte aligned device pointer" : "base must be a 16-byte aligned device pointer", false;
    if (frame && (idx_base & 15u)) return *why = "idx_base must be 16-byte aligned", false;
    if (n > kTfrMaxShards) return *why = "more than 2^32 - 1 shards in one call", false;
    uint64_t bytes = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_shard p = shards[k];
        if (p.records == 0) continue;
        if (frame && (p.src_off & 15u)) return *why = tfr_at(k, "src_off must be a multiple of 16"), false;
        if (p.dst_off & 15u) return *why = tfr_at(k, "dst_off must be a multiple of 16"), false;
        if (frame && idx_base && (p.idx_off & 15u)) return *why = tfr_at(k, "idx_off must be a multiple of 16"), false;
        if (p.record_size > kTfrMaxRecord) return *why = tfr_at(k, "record_size larger than 2^31 blocks"), false;
        uint64_t framed = 0;
        if (!tfr_size(p.records, p.record_size, &framed))
            return *why = tfr_at(k, "records * (16 + record_size) overflows"), false;
        const uint64_t payload = p.records * p.record_size;
        if (framed > kTfrMaxBytes || bytes > kTfrMaxBytes - framed)
            return *why = tfr_at(k, "more than 2^46 framed bytes in one call"), false;
        bytes += framed;
        if (dst_base > UINT64_MAX - p.dst_off || dst_base + p.dst_off > UINT64_MAX - framed)
            return *why = tfr_at(k, "dst_off + stream overflows"), false;
        if (frame) {
            if (src_base > UINT64_MAX - p.src_off || src_base + p.src_off > UINT64_MAX - payload)
                return *why = tfr_at(k, "src_off + payload overflows"), false;
            if (idx_base && (p.records > (UINT64_MAX >> 4) || idx_base > UINT64_MAX - p.idx_off ||
                             idx_base + p.idx_off > UINT64_MAX - 16 * p.records))
                return *why = tfr_at(k, "idx_off + index overflows"), false;
            const uint64_t s0 = src_base + p.src_off, d0 = dst_base + p.dst_off;
            if (payload && s0 < d0 + framed && d0 < s0 + payload)
                return *why = tfr_at(k, "the stream overlaps its own source"), false;
        }
        ++C->live;
        C->total_rows += p.records * (p.record_size / kCrcRowBytes);
    }
    C->rows = crc_batch_region_rows(C->total_rows);
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_shard p = shards[k];
        if (p.records == 0) continue;
        const uint32_t rpr = tfr_shard_rpr(p.record_size, tfr_shard_rows(p.record_size, C->rows));
        C->regions += p.records * rpr;   // at most the framed bytes: below 2^46
        if (rpr > 1) {
            C->long_records += p.records;
            C->raw_slots += p.records * rpr;
        }
    }
    return true;
}

// The uploaded table; the device copy has the raw slots behind it, at a
// multiple of 256 bytes.
inline uint64_t tfr_table_bytes(const TfrCounts &C) { return C.live * sizeof(TfrShard); }
inline uint64_t tfr_raw_offset(const TfrCounts &C) { return span_align256(tfr_table_bytes(C)); }
inline uint64_t tfr_device_bytes(const TfrCounts &C) { return tfr_raw_offset(C) + C.raw_slots * 4; }

// ents[0, C.live) in the caller's order, shards without records squeezed out.
inline void tfr_build(const s3dg_tfrecord_shard *shards, uint64_t n, const TfrCounts &C, TfrShard *ents) {
    uint64_t j = 0, reg0 = 0, lrec0 = 0, raw0 = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_shard p = shards[k];
        if (p.records == 0) continue;
        const uint32_t rows = tfr_shard_rows(p.record_size, C.rows), rpr = tfr_shard_rpr(p.record_size, rows);
        ents[j++] = TfrShard{p.src_off, p.dst_off, p.idx_off, p.records, p.record_size, reg0, lrec0, raw0, rpr, rows,
                             (uint32_t)k, crcb_multmodp(crcb_x8n(p.record_size), 0xFFFFFFFFu),
                             tfr_len_mcrc(p.record_size), 0u};
        reg0 += p.records * rpr;
        if (rpr > 1) {
            lrec0 += p.records;
            raw0 += p.records * rpr;
        }
    }
}

// The entry that owns region w of the call (w below the call's regions): the
// last one whose first region is at or below w.  About log2(n) dependent loads.
S3DG_CB_HD inline uint32_t tfr_find_region(const TfrShard *e, uint32_t n, uint64_t w) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (e[mid].reg0 <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The entry that owns long record t (t below the call's long records).  Entries
// with rpr == 1 own none and share their lrec0 with the entry after them, so
// the last entry at or below t is one with rpr > 1.
S3DG_CB_HD inline uint32_t tfr_find_long(const TfrShard *e, uint32_t n, uint64_t t) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (e[mid].lrec0 <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Where record i of a shard reads its data and `a`.
S3DG_CB_HD inline uint32_t tfr_align(bool frame, uint64_t i, uint64_t record_size) {
    return (uint32_t)(((frame ? 0u : kTfrHeader) + i * record_size) & 15u);
}

// Region q (0 <= q < records * rpr) of shard E.
S3DG_CB_HD inline TfrRegion tfr_region(const TfrShard &E, uint64_t q, bool frame) {
    TfrRegion R;
    R.rec = q / E.rpr;
    R.g = (uint32_t)(q - R.rec * E.rpr);
    R.a = tfr_align(frame, R.rec, E.record_size);
    R.out = E.dst_off + R.rec * (E.record_size + kTfrFraming);
    R.data = frame ? E.src_off + R.rec * E.record_size : R.out + kTfrHeader;
    const uint64_t L = R.a + E.record_size, total_rows = L / kCrcRowBytes, row0 = (uint64_t)R.g * E.rows;
    const uint64_t left = total_rows > row0 ? total_rows - row0 : 0;
    const bool last = R.g + 1 == E.rpr;
    R.pad_lo = row0 * kCrcRowBytes;
    R.nrows = (uint32_t)(left < E.rows ? left : E.rows);
    R.tail = last ? (uint32_t)(L % kCrcRowBytes) : 0u;
    return R;
}

// The data bytes region R hashes and, in the frame form, writes: record
// offsets [*lo, *hi) of its record's data.
S3DG_CB_HD inline void tfr_region_span(const TfrRegion &R, uint64_t *lo, uint64_t *hi) {
    const uint64_t plo = R.pad_lo > R.a ? R.pad_lo : R.a;
    *lo = plo - R.a;
    *hi = R.pad_lo + (uint64_t)R.nrows * kCrcRowBytes + R.tail - R.a;
}

// Byte l (0..15) of a record's framing: 8 length bytes, the length's masked
// CRC, then the footer; and its offset from the record's first framed byte.
S3DG_CB_HD inline uint32_t tfr_framing_byte(uint32_t l, uint64_t record_size, uint32_t len_mcrc, uint32_t data_mcrc) {
    return l < 8 ? (uint32_t)(record_size >> (8 * l)) & 0xFFu
                 : ((l < 12 ? len_mcrc : data_mcrc) >> (8 * (l & 3))) & 0xFFu;
}
S3DG_CB_HD inline uint64_t tfr_framing_at(uint32_t l, uint64_t record_size) { return l < 12 ? l : record_size + l; }

// The CRC-32 of a record's data from one region's raw CRC (rpr == 1).
S3DG_CB_HD inline uint32_t tfr_crc_one(uint32_t raw, uint32_t init) { return ~(init ^ raw); }

// The CRC-32 of a record's data from its regions' raws, in order.  crcb_fold
// over the padded record gives ~(A^L (~0) ^ raw) with L = a + rs; the data's
// own CRC starts its register rs bytes before the end, not L.
S3DG_CB_HD inline uint32_t tfr_crc_fold(const uint32_t *raw, uint32_t rpr, uint32_t rows, uint32_t a, uint64_t record_size,
                                        uint32_t init) {
    const uint64_t L = a + record_size;
    return crcb_fold(raw, rpr, rows, L) ^ crcb_multmodp(crcb_x8n(L), 0xFFFFFFFFu) ^ init;
}

}  // namespace s3dg
