// s3dg_tfrecord_var_plan.h — the host's part of s3dg_tfrecord_frame_var_batch,
// s3dg_tfrecord_check_var_batch and s3dg_tfrecord_index_batch (DESIGN.md
// §5.5.2) as pure functions: the checks of the descriptors with their
// messages, the per-record table, how a record is cut into regions, which run
// of regions a wave takes, a record's constants from the power table, and the
// rule of the walk, as host-and-device functions, so a CPU sweep runs the very
// code the kernels run.  No HIP, no context: it compiles with g++ alone
// (tests/capi/tfrecord_var_plan_sweep.cpp).
//
// A shard is `records` records whose lengths are lengths[len0 .. len0 +
// records); its payload is packed.  With P_i the sum of the lengths before
// record i, the record's data is at src_off + P_i and it is framed at
// dst_off + P_i + 16 i.  The padded record of s3dg_tfrecord_plan.h carries
// over with a = P_i mod 16 (frame) or (12 + P_i) mod 16 (check): source and
// stream still differ by 12 (mod 16) for every record, whatever the lengths.
//
// The table.  One 16-byte entry per record, <P_i, first region of the record
// among the call's regions>, and one more behind each shard's last record
// holding the shard's payload bytes and the next shard's first region: a
// record's length and its number of regions are differences of neighbouring
// entries.  Every record has at least one region, so the entry that owns
// region r is the last one whose first region is at or below r, and the extra
// entries are never found.  One 40-byte entry per shard with records names
// its first entry; the entry after the last shard names the table's end.
//
// Regions per record follow s3dg_tfrecord_plan.h's rule, per record: the
// call's region (crc_batch_region_rows over the call's whole rows), doubled
// for a record of more than kCrcBatchMaxRegions.  Records of one region are
// finished by their wave; the others leave one raw CRC per region, at the
// region's own number, and a fold launch over the compact list of such
// records finishes them.
#pragma once
#include <stdint.h>

#include <string>

#include "s3dg_tfrecord_plan.h"

namespace s3dg {

struct TfvShard {
    uint64_t src_off, dst_off, idx_off;
    uint64_t ent0;   // its first record's entry
    uint64_t k;      // the caller's index
};
static_assert(sizeof(TfvShard) == 40, "TfvShard is 40 bytes");

struct TfvRec {
    uint64_t pre;    // payload bytes of the shard before this record
    uint64_t reg0;   // its first region among the call's regions
};
static_assert(sizeof(TfvRec) == 16, "TfvRec is 16 bytes");

// A record's constants, written on the device behind the table.
struct TfvConst {
    uint32_t init;       // A^len (~0)
    uint32_t len_mcrc;   // masked_crc of the 8 length bytes
};

struct TfvCounts {
    uint64_t live = 0;           // shards with records
    uint64_t records = 0;        // their records
    uint64_t ents = 0;           // records + live: the table's entries
    uint64_t regions = 0;
    uint64_t long_records = 0;   // records of more than one region
    uint64_t total_rows = 0;
    uint64_t max_len = 0;
    uint32_t rows = 0;           // the call's region, in rows
};

constexpr uint32_t kTfvPowers = 64;   // A^(2^b): x^(8 2^b) mod P, b < 61 (crcb_x8n's range); the rest unused
constexpr uint64_t kTfvShardOff = kTfvPowers * 4;

// ---- a record's regions -------------------------------------------------------------
// crc_batch_obj_rows / crc_batch_obj_regions over the longest padded record,
// len + 15, restated for the device.
S3DG_CB_HD inline uint32_t tfv_rec_rows(uint64_t len, uint32_t rows) {
    const uint64_t obj_rows = (len + 15) / kCrcRowBytes;
    uint64_t r = rows;
    while (obj_rows > kCrcBatchMaxRegions * r) r *= 2;   // ceil(obj_rows / r) above the cap, without a division
    return (uint32_t)r;
}
S3DG_CB_HD inline uint64_t tfv_rec_regions(uint64_t len, uint32_t rec_rows) {
    const uint64_t n = ((len + 15) / kCrcRowBytes + rec_rows - 1) / rec_rows;
    return n ? n : 1;
}

// ---- a record's constants --------------------------------------------------------------
inline void tfv_powers(uint32_t *pw) {
    for (uint32_t b = 0; b < kTfvPowers; ++b) pw[b] = b < 61 ? crcb_x8n(1ull << b) : 0u;
}
// A^len (~0) as the product of the powers at len's set bits; len < 2^61.
S3DG_CB_HD inline uint32_t tfv_init(uint64_t len, const uint32_t *pw) {
    uint32_t p = 0xFFFFFFFFu;
    for (uint32_t b = 0; len >> b; ++b)
        if ((len >> b) & 1) p = crcb_multmodp(pw[b], p);
    return p;
}
// masked_crc of the 8 little-endian bytes of len: the reflected CRC takes a
// 32-bit word at a time as it takes a byte.
S3DG_CB_HD inline uint32_t tfv_len_mcrc(uint64_t len) {
    uint32_t c = 0xFFFFFFFFu ^ (uint32_t)len;
    for (int b = 0; b < 32; ++b) c = (c >> 1) ^ (kCrcBatchPoly & (0u - (c & 1)));
    c ^= (uint32_t)(len >> 32);
    for (int b = 0; b < 32; ++b) c = (c >> 1) ^ (kCrcBatchPoly & (0u - (c & 1)));
    return tfr_masked(~c);
}

inline bool tfv_size(const uint64_t *lengths, uint64_t records, uint64_t *out) {
    if (records > (UINT64_MAX >> 4)) return false;
    uint64_t sum = 16 * records;
    for (uint64_t i = 0; i < records; ++i) {
        if (lengths[i] > UINT64_MAX - sum) return false;
        sum += lengths[i];
    }
    *out = sum;
    return true;
}

// The regions and long records of checked shards at the call region C->rows.
inline void tfv_count_regions(const s3dg_tfrecord_var_shard *shards, uint64_t n, const uint64_t *lengths, TfvCounts *C) {
    C->regions = C->long_records = 0;
    if (tfv_rec_regions(C->max_len, tfv_rec_rows(C->max_len, C->rows)) == 1) {   // the longest record is one region: all are
        C->regions = C->records;
        return;
    }
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_var_shard p = shards[k];
        for (uint64_t i = 0; i < p.records; ++i) {
            const uint64_t len = lengths[p.len0 + i], nr = tfv_rec_regions(len, tfv_rec_rows(len, C->rows));
            C->regions += nr;   // at most the framed bytes: below 2^46
            C->long_records += nr > 1;
        }
    }
}

// ---- the checks ------------------------------------------------------------------------
// tfr_check's list over shards of given lengths, and: null lengths with records
// present, len0 + records beyond nlengths, a length above kTfrMaxRecord, the
// sum of a shard beyond what a call frames (which is below any overflow).
inline bool tfv_check(bool frame, uint64_t src_base, uint64_t dst_base, uint64_t idx_base,
                      const s3dg_tfrecord_var_shard *shards, uint64_t n, const uint64_t *lengths, uint64_t nlengths,
                      TfvCounts *C, std::string *why) {
    *C = TfvCounts{};
    if (n == 0) return true;
    if (!shards) return *why = "null shard array", false;
    if (frame && (!src_base || (src_base & 15u))) return *why = "src_base must be a 16-byte aligned device pointer", false;
    if (!dst_base || (dst_base & 15u))
        return *why = frame ? "dst_base must be a 16-byte aligned device pointer" : "base must be a 16-byte aligned device pointer", false;
    if (frame && (idx_base & 15u)) return *why = "idx_base must be 16-byte aligned", false;
    if (n > kTfrMaxShards) return *why = "more than 2^32 - 1 shards in one call", false;
    uint64_t bytes = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_var_shard p = shards[k];
        if (p.records == 0) continue;
        if (!lengths) return *why = "null lengths array", false;
        if (p.len0 > nlengths || p.records > nlengths - p.len0) return *why = tfr_at(k, "len0 + records beyond the lengths"), false;
        if (frame && (p.src_off & 15u)) return *why = tfr_at(k, "src_off must be a multiple of 16"), false;
        if (p.dst_off & 15u) return *why = tfr_at(k, "dst_off must be a multiple of 16"), false;
        if (frame && idx_base && (p.idx_off & 15u)) return *why = tfr_at(k, "idx_off must be a multiple of 16"), false;
        if (p.records > kTfrMaxBytes / kTfrFraming) return *why = tfr_at(k, "more than 2^46 framed bytes in one call"), false;
        uint64_t payload = 0;
        const uint64_t room = kTfrMaxBytes - kTfrFraming * p.records;
        for (uint64_t i = 0; i < p.records; ++i) {
            const uint64_t len = lengths[p.len0 + i];
            if (len > kTfrMaxRecord) return *why = tfr_at(k, "a record longer than 2^31 blocks"), false;
            payload += len;   // both below 2^47
            if (payload > room) return *why = tfr_at(k, "more than 2^46 framed bytes in one call"), false;
            C->total_rows += len / kCrcRowBytes;
            if (len > C->max_len) C->max_len = len;
        }
        const uint64_t framed = payload + kTfrFraming * p.records;
        if (bytes > kTfrMaxBytes - framed) return *why = tfr_at(k, "more than 2^46 framed bytes in one call"), false;
        bytes += framed;
        if (dst_base > UINT64_MAX - p.dst_off || dst_base + p.dst_off > UINT64_MAX - framed)
            return *why = tfr_at(k, "dst_off + stream overflows"), false;
        if (frame) {
            if (src_base > UINT64_MAX - p.src_off || src_base + p.src_off > UINT64_MAX - payload)
                return *why = tfr_at(k, "src_off + payload overflows"), false;
            if (idx_base && (idx_base > UINT64_MAX - p.idx_off || idx_base + p.idx_off > UINT64_MAX - 16 * p.records))
                return *why = tfr_at(k, "idx_off + index overflows"), false;
            const uint64_t s0 = src_base + p.src_off, d0 = dst_base + p.dst_off;
            if (payload && s0 < d0 + framed && d0 < s0 + payload)
                return *why = tfr_at(k, "the stream overlaps its own source"), false;
        }
        ++C->live;
        C->records += p.records;
    }
    C->ents = C->records + C->live;
    C->rows = crc_batch_region_rows(C->total_rows);
    tfv_count_regions(shards, n, lengths, C);
    return true;
}

// ---- the table -------------------------------------------------------------------------
// Uploaded: [powers, 256 B][live + 1 shard entries][ents record entries][long
// records' entries, 8 bytes each]; the device copy has the records' constants
// behind it at a multiple of 256 bytes, then one raw CRC per region when the
// call has long records.
inline uint64_t tfv_rec_offset(const TfvCounts &C) { return (kTfvShardOff + (C.live + 1) * sizeof(TfvShard) + 15) & ~15ull; }
inline uint64_t tfv_long_offset(const TfvCounts &C) { return tfv_rec_offset(C) + C.ents * sizeof(TfvRec); }
inline uint64_t tfv_table_bytes(const TfvCounts &C) { return tfv_long_offset(C) + C.long_records * 8; }
inline uint64_t tfv_const_offset(const TfvCounts &C) { return span_align256(tfv_table_bytes(C)); }
inline uint64_t tfv_raw_offset(const TfvCounts &C) { return span_align256(tfv_const_offset(C) + C.ents * sizeof(TfvConst)); }
inline uint64_t tfv_device_bytes(const TfvCounts &C) { return tfv_raw_offset(C) + (C.long_records ? C.regions * 4 : 0); }

// Fills tab[0, tfv_table_bytes(C)) for checked arguments.
inline void tfv_build(const s3dg_tfrecord_var_shard *shards, uint64_t n, const uint64_t *lengths, const TfvCounts &C,
                      const uint32_t *powers, uint8_t *tab) {
    uint32_t *pw = reinterpret_cast<uint32_t *>(tab);
    for (uint32_t b = 0; b < kTfvPowers; ++b) pw[b] = powers[b];
    TfvShard *sh = reinterpret_cast<TfvShard *>(tab + kTfvShardOff);
    TfvRec *rec = reinterpret_cast<TfvRec *>(tab + tfv_rec_offset(C));
    uint64_t *longs = reinterpret_cast<uint64_t *>(tab + tfv_long_offset(C));
    const bool short_only = C.long_records == 0;
    uint64_t j = 0, e = 0, reg = 0, nl = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_var_shard p = shards[k];
        if (p.records == 0) continue;
        sh[j++] = TfvShard{p.src_off, p.dst_off, p.idx_off, e, k};
        uint64_t pre = 0;
        const uint64_t *len = lengths + p.len0;
        if (short_only) {
            for (uint64_t i = 0; i < p.records; ++i) {
                rec[e++] = TfvRec{pre, reg++};
                pre += len[i];
            }
        } else {
            for (uint64_t i = 0; i < p.records; ++i) {
                const uint64_t nr = tfv_rec_regions(len[i], tfv_rec_rows(len[i], C.rows));
                if (nr > 1) longs[nl++] = e;
                rec[e++] = TfvRec{pre, reg};
                pre += len[i];
                reg += nr;
            }
        }
        rec[e++] = TfvRec{pre, reg};   // the shard's payload and the next shard's first region
    }
    sh[j] = TfvShard{0, 0, 0, e, UINT64_MAX};
}

// ---- finding the record ------------------------------------------------------------------
// Wave w of `waves` takes regions [*lo, *hi) of the call's nreg: equal runs,
// so a wave searches once and then steps through neighbouring entries.
S3DG_CB_HD inline uint64_t tfv_run_len(uint64_t nreg, uint64_t waves) { return (nreg + waves - 1) / waves; }
S3DG_CB_HD inline void tfv_run(uint64_t nreg, uint64_t per, uint64_t w, uint64_t *lo, uint64_t *hi) {
    const uint64_t a = w * per;   // per * waves is below 2^47
    *lo = a < nreg ? a : nreg;
    *hi = nreg - *lo < per ? nreg : *lo + per;
}
// The entry that owns region r (below the call's regions): the last one whose
// first region is at or below r; about log2(ents) dependent loads.
S3DG_CB_HD inline uint64_t tfv_find_rec(const TfvRec *rec, uint64_t ents, uint64_t r) {
    uint64_t lo = 0, hi = ents;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (rec[mid].reg0 <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The shard that owns entry j: the last one whose first entry is at or below j.
S3DG_CB_HD inline uint32_t tfv_find_shard(const TfvShard *sh, uint32_t live, uint64_t j) {
    uint32_t lo = 0, hi = live;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sh[mid].ent0 <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Region g of record i (payload prefix pre, length len, rpr regions of
// rec_rows rows) of shard E.
S3DG_CB_HD inline TfrRegion tfv_region(const TfvShard &E, uint64_t i, uint64_t pre, uint64_t len, uint32_t g, uint32_t rpr,
                                       uint32_t rec_rows, bool frame) {
    TfrRegion R;
    R.rec = i;
    R.g = g;
    R.a = (uint32_t)(((frame ? 0u : kTfrHeader) + pre) & 15u);
    R.out = E.dst_off + pre + kTfrFraming * i;
    R.data = frame ? E.src_off + pre : R.out + kTfrHeader;
    const uint64_t L = R.a + len, total_rows = L / kCrcRowBytes, row0 = (uint64_t)g * rec_rows;
    const uint64_t left = total_rows > row0 ? total_rows - row0 : 0;
    const bool last = g + 1 == rpr;
    R.pad_lo = row0 * kCrcRowBytes;
    R.nrows = (uint32_t)(left < rec_rows ? left : rec_rows);
    R.tail = last ? (uint32_t)(L % kCrcRowBytes) : 0u;
    return R;
}

// ---- the walk ----------------------------------------------------------------------------
// index_entries_from_bytes (src/tfrecord_index.rs:34-80) one record at a time.
// `left` bytes of the stream remain at the record's start.
enum : uint32_t { kTfvWalkRecord = 0, kTfvWalkEnd = 1, kTfvWalkTruncated = 2 };
// Before the header is read: fewer than 12 bytes end the walk silently.
S3DG_CB_HD inline bool tfv_walk_has_header(uint64_t left) { return left >= kTfrHeader; }
// With the header's length field: the record's 12 + len + 4 bytes fit or it is
// truncated; len up to 2^64 - 1 is compared without overflow.
S3DG_CB_HD inline uint32_t tfv_walk_step(uint64_t left, uint64_t len, uint64_t *size) {
    if (left < kTfrHeader) return kTfvWalkEnd;
    if (left < kTfrFraming || len > left - kTfrFraming) return kTfvWalkTruncated;
    *size = len + kTfrFraming;
    return kTfvWalkRecord;
}

// The walk of one stream on the host, the kernel's loop statement by statement:
// entries (nullable) get <offset, size> pairs.
inline s3dg_tfrecord_walk_result tfv_walk_host(const uint8_t *p, uint64_t bytes, uint64_t max_records, uint64_t *entries) {
    s3dg_tfrecord_walk_result R{0, 0, 0, 0, 0, UINT64_MAX};
    uint64_t pos = 0;
    for (;;) {
        const uint64_t left = bytes - pos;
        if (!tfv_walk_has_header(left)) break;
        if (R.records == max_records) {
            R.status = 2;
            break;
        }
        uint64_t len = 0, size = 0;
        uint32_t crc = 0;
        for (int b = 0; b < 8; ++b) len |= (uint64_t)p[pos + b] << (8 * b);
        for (int b = 0; b < 4; ++b) crc |= (uint32_t)p[pos + 8 + b] << (8 * b);
        if (tfv_walk_step(left, len, &size) != kTfvWalkRecord) {
            R.status = 1;
            break;
        }
        if (entries) {
            entries[2 * R.records] = pos;
            entries[2 * R.records + 1] = size;
        }
        if (tfv_len_mcrc(len) != crc) {
            ++R.bad_length_crc;
            if (R.first_bad_record == UINT64_MAX) R.first_bad_record = R.records;
        }
        ++R.records;
        pos += size;
    }
    R.stop_offset = pos;
    R.trailing = bytes - pos;
    return R;
}

inline std::string tfv_stream_at(uint64_t k, const char *what) {
    char b[160];
    snprintf(b, sizeof(b), "stream %llu: %s", (unsigned long long)k, what);
    return b;
}
// A stream of `bytes` holds at most bytes / 16 records: max_records beyond that
// asks for no more entries.
inline uint64_t tfv_walk_cap(const s3dg_tfrecord_stream &t) {
    return t.max_records < t.bytes / kTfrFraming ? t.max_records : t.bytes / kTfrFraming;
}
inline bool tfv_walk_check(uint64_t base, uint64_t idx_base, const s3dg_tfrecord_stream *streams, uint64_t n, bool results,
                           std::string *why) {
    if (n == 0) return true;
    if (!base) return *why = "null base", false;
    if (!idx_base) return *why = "null idx_base", false;
    if (!results) return *why = "null results", false;
    if (!streams) return *why = "null stream array", false;
    if (idx_base & 15u) return *why = "idx_base must be 16-byte aligned", false;
    if (n > kTfrMaxShards) return *why = "more than 2^32 - 1 streams in one call", false;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_stream t = streams[k];
        if (t.idx_off & 15u) return *why = tfv_stream_at(k, "idx_off must be a multiple of 16"), false;
        if (base > UINT64_MAX - t.off || base + t.off > UINT64_MAX - t.bytes) return *why = tfv_stream_at(k, "off + bytes overflows"), false;
        const uint64_t cap = tfv_walk_cap(t);   // below 2^60
        if (idx_base > UINT64_MAX - t.idx_off || idx_base + t.idx_off > UINT64_MAX - 16 * cap)
            return *why = tfv_stream_at(k, "idx_off + index overflows"), false;
    }
    return true;
}

}  // namespace s3dg
