// s3dg_tfrecord_extract_plan.h — the pure rules of s3dg_tfrecord_extract_batch
// (DESIGN.md §5.5.4): the checks of the takes with their messages, the layout
// of the call's workspace, and, as host-and-device functions, when an index
// entry describes its stream, where a record's payload lands, how a record is
// cut into regions and how the pieces of a region lie in source and
// destination.  No HIP, no context: it compiles with g++ alone.
//
// A take is records [first, first + count) of the index at idx_off, read from
// the stream at off.  With e_i = <o_i, s_i> its i-th entry, record i's payload
// is the s_i - 16 bytes at off + o_i + 12 and lands at dst_off + P_i,
// P_i = (o_i - o_first) - 16 (i - first): a closed form of two entries.
//
// The lengths exist only on the device, so the host plans with bounds.  A take
// that is taken reads at most reach = min(bytes, dst_cap + 16 count) bytes of
// its stream (its payload fits dst_cap); the call's region is the var kernels'
// (crc_batch_region_rows) over the sum of the reaches, and the bounds on
// regions and long records below follow from that sum and the entry count.
//
// The padded record is s3dg_tfrecord_plan.h's with the lanes aligned to the
// destination: a = (dst_off + P_i) mod 16 = P_i mod 16, a wave hashes the
// L = a + len bytes from the 16-byte boundary below the record's first
// destination byte with the first a bytes masked, stores aligned 16-byte
// pieces, and reads each piece's 16 source bytes from wherever they lie.
// Regions per record are tfv_rec_rows / tfv_rec_regions, so tfr_crc_fold folds
// a long record's raws unchanged.
#pragma once
#include <stdint.h>

#include <string>

#include "s3dg_tfrecord_var_plan.h"

namespace s3dg {

// One take as uploaded: the caller's fields and the running entry count.
// tk[n] closes the table with ent0 = the call's entries.  A take of no records
// shares its ent0 with its successor and is never found.
struct TfxTake {
    uint64_t off, bytes, idx_off, first, count, dst_off, dst_cap;
    uint64_t ent0;
};
static_assert(sizeof(TfxTake) == 64, "TfxTake is 64 bytes");

// A take's verdict and findings on the device, reset to zeros.  status is
// raised by atomicMax and only by a take that is not taken; payload has one
// writer, the thread of the take's last entry; the rest is TfrDevRes.
struct TfxDevRes {
    unsigned long long status, payload;
    unsigned long long bad_records, bad_length, bad_length_crc, bad_data_crc, first_inv;
    unsigned long long pad;
};
static_assert(sizeof(TfxDevRes) == 64, "TfxDevRes is 64 bytes");

constexpr uint64_t kTfxMaxEntries = 0x7FFFFFFEull;   // the scan counts entries + 1 in an int

struct TfxCounts {
    uint64_t ents = 0;      // sum of the takes' counts
    uint64_t reach = 0;     // sum of the takes' reaches
    uint32_t rows = 0;      // the call's region, in rows
    uint64_t max_regions = 0, max_long = 0;
};

// ---- an entry against its stream -------------------------------------------------------
// Entry <o, s> of a stream of `bytes`: a whole record inside it, compared
// without a sum that could wrap.
S3DG_CB_HD inline bool tfx_entry_fits(uint64_t o, uint64_t s, uint64_t bytes) {
    return s >= kTfrFraming && s <= bytes && o <= bytes - s;
}
// ... and its successor in the run starts where it ends (o + s cannot wrap once it fits).
S3DG_CB_HD inline bool tfx_entry_chains(uint64_t o, uint64_t s, uint64_t o_next) { return o + s == o_next; }
// Payload bytes of a run whose entries fit and chain: first entry's offset,
// last entry, number of records.
S3DG_CB_HD inline uint64_t tfx_run_payload(uint64_t o_first, uint64_t o_last, uint64_t s_last, uint64_t count) {
    return o_last + s_last - o_first - kTfrFraming * count;
}
// Where record i of the run (i counted from the run's first) lands, from dst_off.
S3DG_CB_HD inline uint64_t tfx_dst_pos(uint64_t o_first, uint64_t o, uint64_t i) { return o - o_first - kTfrFraming * i; }

// ---- a record's region ---------------------------------------------------------------------
// Region g of rpr of a record of len bytes whose first destination byte is a
// bytes past a 16-byte boundary: padded offsets [pad_lo, pad_lo + 1024 nrows +
// tail) of the L = a + len bytes from that boundary (tfv_region's cut).
struct TfxRegion {
    uint64_t pad_lo;
    uint32_t nrows, tail;
};
S3DG_CB_HD inline TfxRegion tfx_region(uint32_t a, uint64_t len, uint32_t g, uint32_t rpr, uint32_t rec_rows) {
    const uint64_t L = a + len, total_rows = L / kCrcRowBytes, row0 = (uint64_t)g * rec_rows;
    const uint64_t left = total_rows > row0 ? total_rows - row0 : 0;
    TfxRegion R;
    R.pad_lo = row0 * kCrcRowBytes;
    R.nrows = (uint32_t)(left < rec_rows ? left : rec_rows);
    R.tail = g + 1 == rpr ? (uint32_t)(L % kCrcRowBytes) : 0u;
    return R;
}

// A 16-byte piece whose source bytes start u bytes past a multiple of 4 is read
// as the four dwords from that multiple and, when u != 0, a fifth: each of them
// holds a byte of the piece.  In a record's first piece only bytes [a, 16) are
// the record's: dword k (0..4) is read when it holds one of them.
S3DG_CB_HD inline bool tfx_first_needs(uint32_t k, uint32_t a, uint32_t u) {
    return 4 * k + 4 > a + u && (k < 4 || u != 0);
}

// The take that owns entry j (below the call's entries): the last one whose
// first entry is at or below j.
S3DG_CB_HD inline uint64_t tfx_find_take(const TfxTake *tk, uint64_t n, uint64_t j) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (tk[mid].ent0 <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The entry that owns region r (below reg0[ents]): the last one whose first
// region is at or below r.  Entries without regions share theirs with the next.
S3DG_CB_HD inline uint64_t tfx_find_rec(const uint64_t *reg0, uint64_t ents, uint64_t r) {
    uint64_t lo = 0, hi = ents;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (reg0[mid] <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- the checks ----------------------------------------------------------------------------
inline std::string tfx_at(uint64_t k, const char *what) {
    char b[160];
    snprintf(b, sizeof(b), "take %llu: %s", (unsigned long long)k, what);
    return b;
}
inline uint64_t tfx_reach(const s3dg_tfrecord_take &t) {
    if (t.count == 0) return 0;
    const uint64_t framing = kTfrFraming * t.count;   // count is below 2^31 here
    return t.dst_cap > t.bytes || framing > t.bytes - t.dst_cap ? t.bytes : t.dst_cap + framing;
}
inline bool tfx_check(uint64_t base, uint64_t idx_base, uint64_t dst_base, const s3dg_tfrecord_take *takes, uint64_t n,
                      bool total, TfxCounts *C, std::string *why) {
    *C = TfxCounts{};
    if (n == 0) return true;
    if (!base) return *why = "null base", false;
    if (!idx_base) return *why = "null idx_base", false;
    if (!dst_base) return *why = "null dst_base", false;
    if (!total) return *why = "null output", false;
    if (!takes) return *why = "null take array", false;
    if (idx_base & 15u) return *why = "idx_base must be 16-byte aligned", false;
    if (dst_base & 15u) return *why = "dst_base must be 16-byte aligned", false;
    if (n > kTfrMaxShards) return *why = "more than 2^32 - 1 takes in one call", false;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_take t = takes[k];
        if (t.idx_off & 15u) return *why = tfx_at(k, "idx_off must be a multiple of 16"), false;
        if (t.dst_off & 15u) return *why = tfx_at(k, "dst_off must be a multiple of 16"), false;
        if (t.first > UINT64_MAX - t.count) return *why = tfx_at(k, "first + count overflows"), false;
        if (base > UINT64_MAX - t.off || base + t.off > UINT64_MAX - t.bytes) return *why = tfx_at(k, "off + bytes overflows"), false;
        if (dst_base > UINT64_MAX - t.dst_off || dst_base + t.dst_off > UINT64_MAX - t.dst_cap)
            return *why = tfx_at(k, "dst_off + dst_cap overflows"), false;
        const uint64_t last = t.first + t.count;
        if (last > (UINT64_MAX >> 4) || idx_base > UINT64_MAX - t.idx_off || idx_base + t.idx_off > UINT64_MAX - 16 * last)
            return *why = tfx_at(k, "idx_off + index overflows"), false;
        if (t.count > kTfxMaxEntries - C->ents) return *why = tfx_at(k, "more than 2^31 - 2 records in one call"), false;
        C->ents += t.count;
        const uint64_t reach = tfx_reach(t);
        if (reach > kTfrMaxBytes - C->reach) return *why = tfx_at(k, "more than 2^46 stream bytes in one call"), false;
        C->reach += reach;
    }
    C->rows = crc_batch_region_rows(C->reach / kCrcRowBytes);
    // A record has at most 1 + (len + 15) / region regions and the lengths sum to
    // at most the reach; a record of more than one region is longer than one.
    const uint64_t region = (uint64_t)C->rows * kCrcRowBytes;
    C->max_regions = C->ents + C->ents / 2048 + C->reach / region + 2;
    C->max_long = C->reach / region < C->ents ? C->reach / region : C->ents;
    return true;
}

// ---- the workspace -------------------------------------------------------------------------
// Uploaded: [powers, 256 B][n + 1 takes].  Behind them on the device, each at a
// multiple of 256 bytes: [the long records' counter, 64 B | n results], both
// reset before the plan pass; [ents + 1 first regions]; [ents constants];
// [long records]; [one raw CRC per region]; [the scan's scratch].
struct TfxLayout {
    uint64_t upload, res, reg0, cst, longs, raw, tmp, bytes;
};
constexpr uint64_t kTfxTakeOff = kTfvPowers * 4, kTfxCounterBytes = 64;
inline TfxLayout tfx_layout(const TfxCounts &C, uint64_t n, uint64_t scan_tmp_bytes) {
    TfxLayout L;
    L.upload = kTfxTakeOff + (n + 1) * sizeof(TfxTake);
    L.res = span_align256(L.upload);
    L.reg0 = span_align256(L.res + kTfxCounterBytes + n * sizeof(TfxDevRes));
    L.cst = span_align256(L.reg0 + (C.ents + 1) * 8);
    L.longs = span_align256(L.cst + C.ents * sizeof(TfvConst));
    L.raw = span_align256(L.longs + C.max_long * 8);
    L.tmp = span_align256(L.raw + C.max_regions * 4);
    L.bytes = L.tmp + scan_tmp_bytes;
    return L;
}
inline void tfx_build(const s3dg_tfrecord_take *takes, uint64_t n, const uint32_t *powers, uint8_t *tab) {
    uint32_t *pw = reinterpret_cast<uint32_t *>(tab);
    for (uint32_t b = 0; b < kTfvPowers; ++b) pw[b] = powers[b];
    TfxTake *tk = reinterpret_cast<TfxTake *>(tab + kTfxTakeOff);
    uint64_t e = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_tfrecord_take t = takes[k];
        tk[k] = TfxTake{t.off, t.bytes, t.idx_off, t.first, t.count, t.dst_off, t.dst_cap, e};
        e += t.count;
    }
    tk[n] = TfxTake{0, 0, 0, 0, 0, 0, 0, e};
}

}  // namespace s3dg
