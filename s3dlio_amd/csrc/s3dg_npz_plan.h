// s3dg_npz_plan.h — the host's part of s3dg_npz_frame_batch and
// s3dg_npz_check_batch as pure functions: the checks of the
// descriptors with their messages, the layout of every archive, the call's
// workspace with its per-member table, the ready-made header bytes, and, as
// host-and-device functions, how a member is cut into regions and how its CRC
// is put together.  No HIP, no context: it compiles with g++ alone
// (tests/capi/npz_plan_sweep.cpp).
//
// An archive is a stored ZIP.  With f_i = 30 + name_len_i + hdr_len_i the bytes
// in front of member i's payload (local header, name, NPY header), member i
// starts at the end of member i - 1, its payload f_i later; behind the last
// member lie one central entry of 46 + name_len_i bytes per member and the
// 22-byte end record.  A member's CRC-32 covers its NPY header and its payload
// and stands before both (local header + 14) and behind everything (central
// entry + 16).
//
// Writers (frame form).  The host builds one "front" per member (local header,
// name, NPY header) and one "back" per archive (central directory, end record),
// all CRC fields zero, and uploads them with the tables in one copy.  The
// regions kernel writes payload bytes and nothing else; the finish kernel writes
// fronts and backs with the CRCs patched in.  No byte has two writers.
//
// The padded member is s3dg_tfrecord_extract_plan.h's padded record: a =
// (payload's destination) mod 16 differs from member to member, a wave hashes
// the L = a + size bytes from the 16-byte boundary below the payload with the
// first a bytes masked, and stores aligned 16-byte pieces whose source bytes
// lie anywhere.  Regions are tfv_rec_rows / tfv_rec_regions over the call's
// region (crc_batch_region_rows), cut by tfx_region, so tfr_crc_fold folds a
// member's raws unchanged.  An empty member has no region.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

#include "s3dg_tfrecord_extract_plan.h"

namespace s3dg {

constexpr uint64_t kNpzLocal = 30, kNpzCentral = 46, kNpzEnd = 22;
constexpr uint64_t kNpzLocalCrc = 14, kNpzCentralCrc = 16;   // the CRC field in a local header and in a central entry
constexpr uint64_t kNpzLimit32 = 1ull << 32;                // no ZIP64: sizes and offsets stay below this
constexpr uint64_t kNpzMaxMembers = 65535, kNpzMaxName = 65535;
constexpr uint64_t kNpzMaxBytes = kTfrMaxBytes;              // archive bytes of one call
constexpr uint64_t kNpzMaxArchives = 0xFFFFFFFFull;          // an entry names its archive in 32 bits

// One member of one archive as uploaded; a member that two archives name has
// two entries.  ent[ents] closes the table with reg0 = the call's regions.
struct NpzEnt {
    uint64_t src;        // payload's source from src_base, or S3DG_NPZ_ZEROS
    uint64_t dst;        // payload's first byte from dst_base (check: from base)
    uint64_t size;       // payload bytes
    uint64_t reg0;       // its first region among the call's regions
    uint64_t front;      // its ready-made front in the workspace
    uint32_t front_len;  // 30 + name_len + hdr_len
    uint32_t hcrc;       // CRC-32 of the NPY header (0 for none)
    uint32_t arch;       // its archive, the caller's index
    uint32_t mem;        // its number in that archive
    uint32_t cen;        // its central entry in the archive's back
    uint32_t cen_len;    // 46 + name_len
};                       // a, the payload's place past a 16-byte boundary, is dst mod 16
static_assert(sizeof(NpzEnt) == 64, "NpzEnt is one s_load_dwordx16");

struct NpzArch {
    uint64_t back_dst;   // central directory's first byte from dst_base
    uint64_t back;       // the ready-made back in the workspace
    uint32_t cd_len;     // bytes of the central directory; the end record follows
    uint32_t pad;
};
static_assert(sizeof(NpzArch) == 24, "NpzArch is 24 bytes");

// An archive's findings on the device, reset to zeros.  first_inv is ~(lowest
// bad member), kept by atomicMax; bad_directory is set, not counted.
struct NpzDevRes {
    unsigned long long bad_members, bad_local, bad_crc, bad_directory, first_inv;
    unsigned long long pad[3];
};
static_assert(sizeof(NpzDevRes) == 64, "NpzDevRes is 64 bytes");

struct NpzCounts {
    uint64_t ents = 0;         // members over all archives
    uint64_t bytes = 0;        // archive bytes of the call
    uint64_t fronts = 0;       // bytes of all fronts
    uint64_t backs = 0;        // bytes of all backs
    uint64_t total_rows = 0;   // whole rows of all payloads
    uint64_t regions = 0;
    uint32_t rows = 0;         // the call's region, in rows
};

// ---- sizes -----------------------------------------------------------------------------
inline uint64_t npz_front_len(const s3dg_npz_member &m) { return kNpzLocal + m.name_len + (uint64_t)m.hdr_len; }
inline uint64_t npz_central_len(const s3dg_npz_member &m) { return kNpzCentral + m.name_len; }
// Bytes of an archive of these members, whatever their names say.
inline bool npz_archive_size(const s3dg_npz_member *m, uint64_t members, uint64_t *out) {
    uint64_t sum = kNpzEnd;
    for (uint64_t i = 0; i < members; ++i) {
        const uint64_t fixed = npz_front_len(m[i]) + npz_central_len(m[i]);   // below 2^33
        if (m[i].size > UINT64_MAX - fixed || sum > UINT64_MAX - fixed - m[i].size) return false;
        sum += fixed + m[i].size;
    }
    *out = sum;
    return true;
}

// ---- a member's regions and CRC ----------------------------------------------------------
S3DG_CB_HD inline uint64_t npz_regions(uint64_t size, uint32_t rows) {
    return size ? tfv_rec_regions(size, tfv_rec_rows(size, rows)) : 0;
}
// x^(8 n) mod P as the product of the powers at n's set bits (tfv_powers' table).
S3DG_CB_HD inline uint32_t npz_x8n(uint64_t n, const uint32_t *pw) {
    uint32_t p = 1u << 31;
    for (uint32_t b = 0; n >> b; ++b)
        if ((n >> b) & 1) p = crcb_multmodp(pw[b], p);
    return p;
}
// A member's CRC as a sum of terms, one per region and one for the NPY header,
// so the lanes of a wave share it.  The CRC register behind the header is
// ~crc(h); advanced over the payload and summed with the payload's raw value it
// gives crc(h || p) = ~(x^(8 |p|) ~crc(h) ^ raw(p)), which is zlib's
// crc32_combine, crc(h) x^(8 |p|) ^ crc(p).  raw(p) is the raw value of the
// padded member (zeros in front change nothing): region q's raw advanced over
// the padded bytes behind that region.
S3DG_CB_HD inline uint64_t npz_bytes_behind(uint32_t q, uint32_t nreg, uint32_t rec_rows, uint64_t padded) {
    return q + 1 == nreg ? 0 : padded - (uint64_t)(q + 1) * rec_rows * kCrcRowBytes;
}
S3DG_CB_HD inline uint32_t npz_term(uint32_t v, uint64_t behind, const uint32_t *pw) {
    return crcb_multmodp(npz_x8n(behind, pw), v);
}
// Term t of a member of nreg regions: t < nreg is region t, t == nreg the header.
S3DG_CB_HD inline uint32_t npz_member_term(uint32_t t, uint32_t hcrc, const uint32_t *raw, uint32_t nreg, uint32_t rec_rows,
                                           uint32_t a, uint64_t size, const uint32_t *pw) {
    const bool hdr = t == nreg;
    return npz_term(hdr ? ~hcrc : raw[t], hdr ? size : npz_bytes_behind(t, nreg, rec_rows, a + size), pw);
}
inline uint32_t npz_member_crc(uint32_t hcrc, const uint32_t *raw, uint32_t nreg, uint32_t rows, uint32_t a, uint64_t size,
                               const uint32_t *pw) {
    uint32_t acc = 0;
    for (uint32_t t = 0; t <= nreg; ++t) acc ^= npz_member_term(t, hcrc, raw, nreg, tfv_rec_rows(size, rows), a, size, pw);
    return ~acc;
}
// The entry that owns region r (below the call's regions): the last one whose
// first region is at or below r.  Entries without regions share theirs with the
// next and are never found.
S3DG_CB_HD inline uint64_t npz_find_ent(const NpzEnt *ent, uint64_t ents, uint64_t r) {
    uint64_t lo = 0, hi = ents;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ent[mid].reg0 <= r) lo = mid;
        else hi = mid;
    }
    return lo;
}
// A central entry's CRC field c is wrong when it is neither the CRC of the bytes
// in memory nor the local header's field: where those two differ, the member is
// bad_crc already, and a damaged payload is reported once.
S3DG_CB_HD inline bool npz_central_crc_bad(uint32_t c, uint32_t computed, uint32_t local) {
    return c != computed && c != local;
}

// ---- the checks --------------------------------------------------------------------------
inline std::string npz_at(const char *what, uint64_t k, const char *why) {
    char b[192];
    snprintf(b, sizeof(b), "%s %llu: %s", what, (unsigned long long)k, why);
    return b;
}
// All of a call's arguments, before anything is reserved or enqueued.  frame:
// src_base and dst_base; check: dst_base alone, src_off is not looked at.
inline bool npz_check(bool frame, uint64_t src_base, uint64_t dst_base, const s3dg_npz_archive *archives, uint64_t n,
                      const s3dg_npz_member *members, uint64_t nmembers, bool blob, uint64_t blob_len, NpzCounts *C,
                      std::string *why) {
    *C = NpzCounts{};
    if (n == 0) return true;
    if (!archives) return *why = "null archive array", false;
    if (!members) return *why = "null member array", false;
    if (!blob) return *why = "null blob", false;
    if (frame && (!src_base || (src_base & 15u))) return *why = "src_base must be a 16-byte aligned device pointer", false;
    if (!dst_base || (dst_base & 15u))
        return *why = frame ? "dst_base must be a 16-byte aligned device pointer" : "base must be a 16-byte aligned device pointer", false;
    if (n > kNpzMaxArchives) return *why = "more than 2^32 - 1 archives in one call", false;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_npz_archive A = archives[k];
        if (A.dst_off & 15u) return *why = npz_at("archive", k, "dst_off must be a multiple of 16"), false;
        if (A.style != S3DG_NPZ_STYLE_RAW && A.style != S3DG_NPZ_STYLE_LEGACY) return *why = npz_at("archive", k, "unknown style"), false;
        if (A.members == 0) return *why = npz_at("archive", k, "an archive has at least one member"), false;
        if (A.members > kNpzMaxMembers) return *why = npz_at("archive", k, "more than 65535 members"), false;
        if (A.member0 > nmembers || A.members > nmembers - A.member0)
            return *why = npz_at("archive", k, "member0 + members beyond the members"), false;
        uint64_t at = 0, cd = 0;   // the next local header from the archive's start, the directory's bytes
        for (uint64_t i = 0; i < A.members; ++i) {
            const uint64_t j = A.member0 + i;
            const s3dg_npz_member m = members[j];
            if (m.name_len == 0 || m.name_len > kNpzMaxName) return *why = npz_at("member", j, "name_len must be 1..65535"), false;
            if (m.name_off > blob_len || m.name_len > blob_len - m.name_off) return *why = npz_at("member", j, "name outside the blob"), false;
            if (m.hdr_off > blob_len || m.hdr_len > blob_len - m.hdr_off) return *why = npz_at("member", j, "NPY header outside the blob"), false;
            if (m.size >= kNpzLimit32 - m.hdr_len) return *why = npz_at("member", j, "hdr_len + size reaches 2^32 (no ZIP64)"), false;
            if (at >= kNpzLimit32) return *why = npz_at("member", j, "local header offset reaches 2^32 (no ZIP64)"), false;
            const bool zeros = m.src_off == S3DG_NPZ_ZEROS;
            if (frame && !zeros) {
                if (m.src_off & 15u) return *why = npz_at("member", j, "src_off must be a multiple of 16"), false;
                if (src_base > UINT64_MAX - m.src_off || src_base + m.src_off > UINT64_MAX - m.size)
                    return *why = npz_at("member", j, "src_off + size overflows"), false;
            }
            at += npz_front_len(m) + m.size;   // below 2^32 + 2^33
            cd += npz_central_len(m);          // below 2^33
            C->total_rows += m.size / kCrcRowBytes;
            C->fronts += npz_front_len(m);
        }
        if (at >= kNpzLimit32) return *why = npz_at("archive", k, "central directory offset reaches 2^32 (no ZIP64)"), false;
        if (cd >= kNpzLimit32) return *why = npz_at("archive", k, "central directory size reaches 2^32 (no ZIP64)"), false;
        const uint64_t total = at + cd + kNpzEnd;
        if (total > kNpzMaxBytes - C->bytes) return *why = npz_at("archive", k, "more than 2^46 archive bytes in one call"), false;
        if (dst_base > UINT64_MAX - A.dst_off || dst_base + A.dst_off > UINT64_MAX - total)
            return *why = npz_at("archive", k, "dst_off + archive overflows"), false;
        if (frame) {
            const uint64_t d0 = dst_base + A.dst_off;
            for (uint64_t i = 0; i < A.members; ++i) {
                const s3dg_npz_member m = members[A.member0 + i];
                const uint64_t s0 = src_base + m.src_off;
                if (m.src_off != S3DG_NPZ_ZEROS && m.size && s0 < d0 + total && d0 < s0 + m.size)
                    return *why = npz_at("archive", k, "the archive overlaps its own source"), false;
            }
        }
        C->bytes += total;
        C->backs += cd + kNpzEnd;
        C->ents += A.members;
    }
    C->rows = crc_batch_region_rows(C->total_rows);
    for (uint64_t k = 0; k < n; ++k)
        for (uint64_t i = 0; i < archives[k].members; ++i)
            C->regions += npz_regions(members[archives[k].member0 + i].size, C->rows);   // at most the call's bytes
    return true;
}

// ---- the workspace -------------------------------------------------------------------------
// Uploaded: [powers, 256 B][n archives][ents + 1 entries][fronts][backs].  Behind
// them on the device, each at a multiple of 256 bytes: [n results], reset
// before a check; [one raw CRC per region].
struct NpzLayout {
    uint64_t arch, ent, fronts, backs, upload, res, raw, bytes;
};
inline NpzLayout npz_layout(const NpzCounts &C, uint64_t n) {
    NpzLayout L;
    L.arch = kTfvPowers * 4;
    L.ent = (L.arch + n * sizeof(NpzArch) + 63) & ~63ull;
    L.fronts = L.ent + (C.ents + 1) * sizeof(NpzEnt);
    L.backs = L.fronts + C.fronts;
    L.upload = L.backs + C.backs;
    L.res = span_align256(L.upload);
    L.raw = span_align256(L.res + n * sizeof(NpzDevRes));
    L.bytes = L.raw + C.regions * 4;
    return L;
}

inline void npz_put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
inline void npz_put32(uint8_t *p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k)); }
// write_local_file_header (src/data_formats/npz.rs:256-270) or object_frame's, CRC zero
inline void npz_local(uint8_t *p, uint32_t style, uint32_t npy, const uint8_t *name, uint32_t name_len) {
    const bool raw = style == S3DG_NPZ_STYLE_RAW;
    memcpy(p, "PK\x03\x04", 4);
    npz_put16(p + 4, raw ? 20 : 10); npz_put16(p + 6, 0); npz_put16(p + 8, 0); npz_put16(p + 10, 0);
    npz_put16(p + 12, raw ? 0 : 0x21);
    npz_put32(p + 14, 0); npz_put32(p + 18, npy); npz_put32(p + 22, npy);
    npz_put16(p + 26, name_len); npz_put16(p + 28, 0);
    memcpy(p + kNpzLocal, name, name_len);
}
// write_central_dir_entry (npz.rs:273-297) or object_frame's, CRC zero
inline void npz_central(uint8_t *p, uint32_t style, uint32_t npy, uint32_t off, const uint8_t *name, uint32_t name_len) {
    const bool raw = style == S3DG_NPZ_STYLE_RAW;
    memcpy(p, "PK\x01\x02", 4);
    npz_put16(p + 4, 20); npz_put16(p + 6, raw ? 20 : 10); npz_put16(p + 8, 0); npz_put16(p + 10, 0); npz_put16(p + 12, 0);
    npz_put16(p + 14, raw ? 0 : 0x21);
    npz_put32(p + 16, 0); npz_put32(p + 20, npy); npz_put32(p + 24, npy);
    npz_put16(p + 28, name_len); npz_put16(p + 30, 0); npz_put16(p + 32, 0); npz_put16(p + 34, 0); npz_put16(p + 36, 0);
    npz_put32(p + 38, 0); npz_put32(p + 42, off);
    memcpy(p + kNpzCentral, name, name_len);
}
// write_eocd (npz.rs:300-309)
inline void npz_end(uint8_t *p, uint32_t entries, uint32_t cd_len, uint32_t cd_off) {
    memcpy(p, "PK\x05\x06", 4);
    npz_put16(p + 4, 0); npz_put16(p + 6, 0); npz_put16(p + 8, entries); npz_put16(p + 10, entries);
    npz_put32(p + 12, cd_len); npz_put32(p + 16, cd_off); npz_put16(p + 20, 0);
}

// Fills ws[0, L.upload) for checked arguments.  hcrc(bytes, len) is the CRC-32
// of an NPY header (crc32_host_update in the library).
template <class HeaderCrc>
inline void npz_build(const s3dg_npz_archive *archives, uint64_t n, const s3dg_npz_member *members, const uint8_t *blob,
                      const NpzCounts &C, const NpzLayout &L, const uint32_t *powers, HeaderCrc hcrc, uint8_t *ws) {
    uint32_t *pw = reinterpret_cast<uint32_t *>(ws);
    for (uint32_t b = 0; b < kTfvPowers; ++b) pw[b] = powers[b];
    NpzArch *arch = reinterpret_cast<NpzArch *>(ws + L.arch);
    NpzEnt *ent = reinterpret_cast<NpzEnt *>(ws + L.ent);
    uint64_t e = 0, reg = 0, front = L.fronts, back = L.backs;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_npz_archive A = archives[k];
        uint64_t at = 0, cen = 0;
        const uint64_t back0 = back;
        for (uint64_t i = 0; i < A.members; ++i) {
            const s3dg_npz_member m = members[A.member0 + i];
            const uint32_t flen = (uint32_t)npz_front_len(m), clen = (uint32_t)npz_central_len(m);
            const uint32_t npy = (uint32_t)(m.hdr_len + m.size);
            const uint8_t *name = blob + m.name_off, *hdr = blob + m.hdr_off;
            npz_local(ws + front, A.style, npy, name, m.name_len);
            if (m.hdr_len) memcpy(ws + front + kNpzLocal + m.name_len, hdr, m.hdr_len);
            npz_central(ws + back, A.style, npy, (uint32_t)at, name, m.name_len);
            const uint64_t dst = A.dst_off + at + flen;
            ent[e++] = NpzEnt{m.src_off, dst, m.size, reg, front, flen, m.hdr_len ? hcrc(hdr, (uint64_t)m.hdr_len) : 0u,
                              (uint32_t)k, (uint32_t)i, (uint32_t)cen, clen};
            reg += npz_regions(m.size, C.rows);
            at += flen + m.size;
            cen += clen;
            front += flen;
            back += clen;
        }
        npz_end(ws + back, (uint32_t)A.members, (uint32_t)cen, (uint32_t)at);
        back += kNpzEnd;
        arch[k] = NpzArch{A.dst_off + at, back0, (uint32_t)cen, 0u};
    }
    ent[e] = NpzEnt{0, 0, 0, reg, 0, 0, 0, 0, 0, 0, 0};
}

}  // namespace s3dg
