// s3dg_npz_unpack_plan.h — the pure rules of s3dg_npz_index_batch and
// s3dg_npz_unpack_batch: the checks of the descriptors with
// their messages, the layout of the unpack's workspace, and, as host-and-device
// functions, what the walk accepts of an end record, a central entry, a local
// header and an NPY preamble, when a table entry describes its archive, where a
// member lands and how its stored file is cut into regions.  No HIP, no
// context: it compiles with g++ alone (tests/capi/npz_unpack_plan_sweep.cpp).
//
// The table.  One 32-byte entry of eight little-endian uint32 per member, in
// central-directory order, every offset from the archive's first byte:
// <local_off, name_len | flags << 16, hdr_off, hdr_len, data_off, size, crc, 0>.
// The member's stored file is the hdr_len + size bytes at hdr_off; its CRC-32
// covers all of them.
//
// The padded member.  Member i of a take lands at dst_off + P_i, P_i the sum of
// round_up(size_j, 16) over the members before it, so a = 0 on the store side
// for every member.  The hashed run starts hdr_len bytes earlier: with
// hp = ceil(hdr_len / 16) header pieces and a = 16 hp - hdr_len, the wave
// hashes the L = a + hdr_len + size bytes from 16 hp bytes in front of the
// payload's destination, the first a of them masked, which is
// s3dg_tfrecord_extract_plan.h's padded record of len = hdr_len + size.  Pieces
// below hp are hashed and not stored.  Regions are tfv_rec_rows /
// tfv_rec_regions over len, cut by tfx_region, so tfr_crc_fold folds a long
// member's raws unchanged.  A stored file of no bytes has no region.
//
// The sizes exist only on the device, so the host plans with bounds.  Entries
// may name the same bytes more than once, so a take's reach is not bounded by
// its archive: it is min(count * bytes, dst_cap + 65535 count), every stored
// file being at most `bytes` and the payloads of a taken take fitting dst_cap.
#pragma once
#include <stdint.h>

#include <string>

#include "s3dg_npz_plan.h"

namespace s3dg {

constexpr uint32_t kNzuEntry = 32;                     // bytes of a table entry
constexpr uint32_t kNzuMaxHdr = 65535;                 // the longest NPY header an entry may name
constexpr uint64_t kNzuSearch = kNpzEnd + 65535;       // bytes from the end in which the end record starts
constexpr uint32_t kNzuSigEnd = 0x06054b50u, kNzuSigCentral = 0x02014b50u, kNzuSigLocal = 0x04034b50u;
constexpr uint64_t kNzuMaxEntries = kTfxMaxEntries;    // the scans count entries + 1 in an int
constexpr uint64_t kNzuNone = UINT64_MAX;

struct NzuEntry {
    uint32_t local_off, name_flags, hdr_off, hdr_len, data_off, size, crc, zero;
};
static_assert(sizeof(NzuEntry) == kNzuEntry, "a table entry is 32 bytes");

// ---- the walk's rules ------------------------------------------------------------------
// The fields of an end record found at `pos` of an archive whose directory may
// be walked: one disk, equal counts, no ZIP64 marker, the directory ending
// where the end record starts.
S3DG_CB_HD inline bool nzi_end_ok(uint32_t disk, uint32_t cd_disk, uint32_t here, uint32_t total, uint32_t cd_size,
                                  uint32_t cd_off, uint64_t pos) {
    return disk == 0 && cd_disk == 0 && here == total && total != 0xFFFFu && cd_size != 0xFFFFFFFFu &&
           cd_off != 0xFFFFFFFFu && (uint64_t)cd_off + cd_size == pos;
}
// A central entry's fixed fields: no ZIP64 marker, disk 0.  That a stored
// member has one size is asked once its method is known to be 0.
S3DG_CB_HD inline bool nzi_central_ok(uint32_t sig, uint32_t csize, uint32_t usize, uint32_t disk, uint32_t local_off) {
    return sig == kNzuSigCentral && csize != 0xFFFFFFFFu && usize != 0xFFFFFFFFu && local_off != 0xFFFFFFFFu &&
           disk == 0;
}
S3DG_CB_HD inline bool nzi_supported(uint32_t flags, uint32_t method) { return method == 0 && (flags & 9u) == 0; }
// The NPY preamble of a stored file of `stored` bytes whose first min(stored,
// 12) bytes are b: the header's length with its preamble, or 0 for a raw file.
S3DG_CB_HD inline uint32_t nzi_npy_header(const uint8_t *b, uint64_t stored) {
    const uint8_t magic[6] = {0x93, 'N', 'U', 'M', 'P', 'Y'};
    if (stored < 10) return 0;
    for (int q = 0; q < 6; ++q)
        if (b[q] != magic[q]) return 0;
    uint64_t len;
    if (b[6] == 1) len = 10 + ((uint64_t)b[8] | (uint64_t)b[9] << 8);
    else if ((b[6] == 2 || b[6] == 3) && stored >= 12)
        len = 12 + ((uint64_t)b[8] | (uint64_t)b[9] << 8 | (uint64_t)b[10] << 16 | (uint64_t)b[11] << 24);
    else return 0;
    return len <= stored && len <= kNzuMaxHdr ? (uint32_t)len : 0u;
}

// ---- an entry against its archive --------------------------------------------------------
S3DG_CB_HD inline bool nzu_entry_fits(const NzuEntry &e, uint64_t bytes) {
    const uint64_t name_len = e.name_flags & 0xFFFFu;
    return (uint64_t)e.local_off + kNpzLocal + name_len <= e.hdr_off && (uint64_t)e.hdr_off + e.hdr_len == e.data_off &&
           e.hdr_len <= kNzuMaxHdr && (uint64_t)e.data_off + e.size <= bytes;
}
S3DG_CB_HD inline uint64_t nzu_packed(uint64_t size) { return (size + 15) & ~15ull; }
S3DG_CB_HD inline uint32_t nzu_hdr_pieces(uint32_t hdr_len) { return (hdr_len + 15) / 16; }
S3DG_CB_HD inline uint32_t nzu_align(uint32_t hdr_len) { return 16 * nzu_hdr_pieces(hdr_len) - hdr_len; }
S3DG_CB_HD inline uint64_t nzu_regions(uint64_t len, uint32_t rows) {
    return len ? tfv_rec_regions(len, tfv_rec_rows(len, rows)) : 0;
}
// Rows [0, n) of a region of nrows rows starting at padded row row0 hold a
// header piece: their stores are predicated, the others' are not.
S3DG_CB_HD inline uint32_t nzu_header_rows(uint32_t hp, uint64_t row0, uint32_t nrows) {
    const uint64_t hr = ((uint64_t)hp + 63) / 64;
    const uint64_t n = hr > row0 ? hr - row0 : 0;
    return (uint32_t)(n < nrows ? n : nrows);
}

// ---- the checks ----------------------------------------------------------------------------
struct NzuCounts {
    uint64_t ents = 0;      // sum of the takes' counts
    uint64_t reach = 0;     // sum of the takes' reaches
    uint32_t rows = 0;      // the call's region, in rows
    uint64_t max_regions = 0, max_long = 0;
};

inline bool nzi_check(uint64_t base, uint64_t tab_base, const s3dg_npz_stream *archives, uint64_t n, bool results,
                      std::string *why) {
    if (n == 0) return true;
    if (!base) return *why = "null base", false;
    if (!tab_base) return *why = "null table", false;
    if (!results) return *why = "null results", false;
    if (!archives) return *why = "null archive array", false;
    if (tab_base & 15u) return *why = "table must be 16-byte aligned", false;
    if (n > kNpzMaxArchives) return *why = "more than 2^32 - 1 archives in one call", false;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_npz_stream t = archives[k];
        if (t.tab_off & 15u) return *why = npz_at("archive", k, "tab_off must be a multiple of 16"), false;
        if (base > UINT64_MAX - t.off || base + t.off > UINT64_MAX - t.bytes) return *why = npz_at("archive", k, "off + bytes overflows"), false;
        if (t.bytes >= kNpzLimit32) return *why = npz_at("archive", k, "an archive of 2^32 bytes or more (no ZIP64)"), false;
        const uint64_t cap = t.max_members < kNpzMaxMembers ? t.max_members : kNpzMaxMembers;
        if (tab_base > UINT64_MAX - t.tab_off || tab_base + t.tab_off > UINT64_MAX - kNzuEntry * cap)
            return *why = npz_at("archive", k, "tab_off + table overflows"), false;
    }
    return true;
}

inline uint64_t nzu_reach(const s3dg_npz_take &t) {
    if (t.count == 0) return 0;
    const uint64_t hdrs = (uint64_t)kNzuMaxHdr * t.count;   // count is below 2^31 here
    const uint64_t by_cap = t.dst_cap > UINT64_MAX - hdrs ? UINT64_MAX : t.dst_cap + hdrs;
    const uint64_t by_arch = t.bytes > UINT64_MAX / t.count ? UINT64_MAX : t.bytes * t.count;
    return by_cap < by_arch ? by_cap : by_arch;
}
inline bool nzu_check(uint64_t base, uint64_t tab_base, uint64_t dst_base, const s3dg_npz_take *takes, uint64_t n, bool total,
                      NzuCounts *C, std::string *why) {
    *C = NzuCounts{};
    if (n == 0) return true;
    if (!base) return *why = "null base", false;
    if (!tab_base) return *why = "null table", false;
    if (!dst_base) return *why = "null dst_base", false;
    if (!total) return *why = "null output", false;
    if (!takes) return *why = "null take array", false;
    if (tab_base & 15u) return *why = "table must be 16-byte aligned", false;
    if (dst_base & 15u) return *why = "dst_base must be 16-byte aligned", false;
    if (n > kNpzMaxArchives) return *why = "more than 2^32 - 1 takes in one call", false;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_npz_take t = takes[k];
        if (t.tab_off & 15u) return *why = tfx_at(k, "tab_off must be a multiple of 16"), false;
        if (t.dst_off & 15u) return *why = tfx_at(k, "dst_off must be a multiple of 16"), false;
        if (t.first > UINT64_MAX - t.count) return *why = tfx_at(k, "first + count overflows"), false;
        if (base > UINT64_MAX - t.off || base + t.off > UINT64_MAX - t.bytes) return *why = tfx_at(k, "off + bytes overflows"), false;
        if (dst_base > UINT64_MAX - t.dst_off || dst_base + t.dst_off > UINT64_MAX - t.dst_cap)
            return *why = tfx_at(k, "dst_off + dst_cap overflows"), false;
        const uint64_t last = t.first + t.count;
        if (last > (UINT64_MAX >> 5) || tab_base > UINT64_MAX - t.tab_off || tab_base + t.tab_off > UINT64_MAX - kNzuEntry * last)
            return *why = tfx_at(k, "tab_off + table overflows"), false;
        if (t.count > kNzuMaxEntries - C->ents) return *why = tfx_at(k, "more than 2^31 - 2 members in one call"), false;
        C->ents += t.count;
        const uint64_t reach = nzu_reach(t);
        if (reach > kNpzMaxBytes - C->reach) return *why = tfx_at(k, "more than 2^46 archive bytes in one call"), false;
        C->reach += reach;
    }
    C->rows = crc_batch_region_rows(C->reach / kCrcRowBytes);
    // A member has at most 1 + (len + 15) / region regions and the stored files of
    // the taken takes sum to at most the reach; one of more than one region is
    // longer than a region less 15 bytes.
    const uint64_t region = (uint64_t)C->rows * kCrcRowBytes;
    C->max_regions = C->ents + C->ents / 2048 + C->reach / region + 2;
    const uint64_t longs = C->reach / (region - 15);
    C->max_long = longs < C->ents ? longs : C->ents;
    return true;
}

// ---- the workspace -------------------------------------------------------------------------
// A take as uploaded is TfxTake with the table's offset as idx_off.  A take's
// verdict and findings on the device, reset to zeros: status 2 is raised by
// atomicMax in the validation, status 1, span and bytes have one writer, the
// thread of the take's first entry; first_inv is ~(lowest bad member).
struct NzuDevRes {
    unsigned long long status, span, bytes, bad_crc, first_inv;
    unsigned long long pad[3];
};
static_assert(sizeof(NzuDevRes) == 64, "NzuDevRes is 64 bytes");

// Uploaded: [powers, 256 B][n + 1 takes].  Behind them on the device, each at a
// multiple of 256 bytes: [the long members' counter, 64 B | n results], both
// reset before the plan pass; three arrays of ents + 1: [packed offsets]
// [payload prefix][first regions]; [ents A^len (~0)]; [long members]; [one raw
// CRC per region]; [the scan's scratch].
struct NzuLayout {
    uint64_t upload, res, pk, sz, reg0, cst, longs, raw, tmp, bytes;
};
constexpr uint64_t kNzuTakeOff = kTfvPowers * 4, kNzuCounterBytes = 64;
inline NzuLayout nzu_layout(const NzuCounts &C, uint64_t n, uint64_t scan_tmp_bytes) {
    NzuLayout L;
    L.upload = kNzuTakeOff + (n + 1) * sizeof(TfxTake);
    L.res = span_align256(L.upload);
    L.pk = span_align256(L.res + kNzuCounterBytes + n * sizeof(NzuDevRes));
    L.sz = span_align256(L.pk + (C.ents + 1) * 8);
    L.reg0 = span_align256(L.sz + (C.ents + 1) * 8);
    L.cst = span_align256(L.reg0 + (C.ents + 1) * 8);
    L.longs = span_align256(L.cst + C.ents * 4);
    L.raw = span_align256(L.longs + C.max_long * 8);
    L.tmp = span_align256(L.raw + C.max_regions * 4);
    L.bytes = L.tmp + scan_tmp_bytes;
    return L;
}
inline void nzu_build(const s3dg_npz_take *takes, uint64_t n, const uint32_t *powers, uint8_t *tab) {
    uint32_t *pw = reinterpret_cast<uint32_t *>(tab);
    for (uint32_t b = 0; b < kTfvPowers; ++b) pw[b] = powers[b];
    TfxTake *tk = reinterpret_cast<TfxTake *>(tab + kNzuTakeOff);
    uint64_t e = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_npz_take t = takes[k];
        tk[k] = TfxTake{t.off, t.bytes, t.tab_off, t.first, t.count, t.dst_off, t.dst_cap, e};
        e += t.count;
    }
    tk[n] = TfxTake{0, 0, 0, 0, 0, 0, 0, e};
}

}  // namespace s3dg
