// s3dg_inflate_plan.h — the decode core of s3dg_inflate_batch and the rules of
// s3dg_npz_zindex_batch / s3dg_npz_zunpack_batch: the
// checks of the descriptors with their messages, the work-item layout, and, as
// host-and-device functions, an RFC 1951 decoder written once over an
// environment E: the bit reader over a bounded byte span, the block headers,
// the canonical codes with zlib's acceptance rule, the length and distance
// rules and the output limits.  The kernel (s3dg_inflate.hip) supplies an E of
// one wave with its tables, input tile and history ring in LDS; the sweep
// (tests/capi/inflate_core_sweep.cpp) supplies a serial E over plain arrays.
// Both run inf_run, so every acceptance rule and every loop bound is proved
// without a GPU.  No HIP, no context: it compiles with g++ alone.
//
// The environment.  E.word(w) is the 32-bit little-endian word w of the span,
// counted from E.lead() bytes in front of its first byte (the span lies at any
// byte address, the words at aligned ones); bytes outside the span read as
// zero.  E.T() are the tables.  E.build(lens, n, ...) fills one canonical code
// from its lengths (serially by inf_build_serial, or by all lanes with the same
// result); E.put_lens / E.get_len / E.put_fixed write and read T().lens.
// E.literal / E.match / E.stored emit; the core has checked the
// limits and the distance before it calls them.  E.u(x) marks a value as
// uniform over the wave (v_readfirstlane; the identity on the host).
//
// Termination.  The core counts the bits it consumes.  Every iteration of
// every loop consumes at least one bit or ends the stream, and a stream that
// has consumed more than 8 * src_bytes bits ends TRUNCATED before anything
// decoded from the bits behind its end is acted on.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "s3dg_npz_unpack_plan.h"

namespace s3dg {

constexpr uint32_t kInfLitBits = 10, kInfDistBits = 8;   // first-level lookup widths
constexpr uint32_t kInfWindow = 32768;
constexpr uint32_t kInfMaxLit = 286, kInfMaxDist = 30;   // HLIT and HDIST bounds (codes 286, 287, 30, 31 never valid)
constexpr uint64_t kInfAny = UINT64_MAX;
constexpr uint32_t kInfCrcPoly = 0xEDB88320u;
// A work item's flags.  Bit 0 is the caller's (S3DG_INFLATE_CRC).
constexpr uint32_t kInfCrc = 1, kInfStored = 2, kInfSkip = 4;

// One stream as the kernel consumes it.
struct InfWork {
    uint64_t src, src_bytes;   // device address of the stream's first byte
    uint64_t dst, dst_cap;     // device address, a multiple of 16
    uint64_t want;             // kInfAny: any size
    uint32_t crc, flags;
};
static_assert(sizeof(InfWork) == 48, "InfWork is 48 bytes");
struct InfDevRes {
    uint32_t status, bad_crc;
    uint64_t out_bytes, in_bytes, pad;
};
static_assert(sizeof(InfDevRes) == 32, "InfDevRes is 32 bytes");

// The tables of one wave.  A lookup entry is symbol << 4 | code length, 0 for
// "not in the first level"; count[l] codes of length l; sym the symbols in
// canonical order.  lens holds the code lengths being read: [0, 320) literal /
// length then distance, [320, 339) the code-length code's own.
struct InfTables {
    uint16_t lit_lut[1u << kInfLitBits], dist_lut[1u << kInfDistBits];
    uint16_t lit_count[16], dist_count[16];
    uint16_t lit_sym[288], dist_sym[32];
    uint8_t lens[352];
};
constexpr uint32_t kInfClAt = 320;

// ---- the tables' rules ---------------------------------------------------------------------
// Length symbol s - 257 in [0, 29) and distance code d in [0, 30): base value and extra bits.
S3DG_CB_HD inline uint32_t inf_len_extra(uint32_t s) { return s < 8 || s == 28 ? 0u : (s - 4) >> 2; }
S3DG_CB_HD inline uint32_t inf_len_base(uint32_t s) { return s < 8 ? 3 + s : s == 28 ? 258u : 3 + ((4 + (s & 3)) << ((s - 4) >> 2)); }
S3DG_CB_HD inline uint32_t inf_dist_extra(uint32_t d) { return d < 4 ? 0u : (d - 2) >> 1; }
S3DG_CB_HD inline uint32_t inf_dist_base(uint32_t d) { return d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << ((d - 2) >> 1)); }
// The fixed code: literal / length symbol i of 288, then 32 distance codes of 5 bits.
S3DG_CB_HD inline uint32_t inf_fixed_len(uint32_t i) { return i < 144 ? 8u : i < 256 ? 9u : i < 280 ? 7u : i < 288 ? 8u : 5u; }
// The order in which a dynamic header stores the code-length code's lengths:
// 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15.
S3DG_CB_HD inline uint32_t inf_cl_order(uint32_t i) {
    return i < 3 ? 16 + i : i == 3 ? 0u : ((i - 4) & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1);
}
// A set of code lengths, by its counts: the sum of count[l] 2^(15 - l) against
// 2^15.  Over-subscribed: refused.  Incomplete: refused, unless it is one code
// of length 1 and not the code-length code.  No code at all: accepted here, and
// every symbol read with it is refused.
S3DG_CB_HD inline bool inf_code_ok(uint32_t kraft, uint32_t total, uint32_t count1, bool cl) {
    if (total == 0) return true;
    if (kraft > 32768u) return false;
    if (kraft < 32768u) return !cl && total == 1 && count1 == 1;
    return true;
}
S3DG_CB_HD inline uint32_t inf_rev(uint32_t code, uint32_t len) {
    uint32_t r = 0;
    for (uint32_t q = 0; q < len; ++q) r |= ((code >> q) & 1u) << (len - 1 - q);
    return r;
}
// One canonical code from lens[0, n), one symbol after the other; no array of
// its own, so one lane may run it without scratch memory.
S3DG_CB_HD inline bool inf_build_serial(const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *sym, uint16_t *lut,
                                        uint32_t lut_bits, bool cl) {
    for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
    if (lut)
        for (uint32_t q = 0; q < (1u << lut_bits); ++q) lut[q] = 0;
    uint32_t kraft = 0, total = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (lens[i]) {
            count[lens[i]] = (uint16_t)(count[lens[i]] + 1);
            kraft += 1u << (15 - lens[i]);
            ++total;
        }
    if (!inf_code_ok(kraft, total, count[1], cl)) return false;
    uint32_t code = 0, at = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        for (uint32_t i = 0; i < n; ++i)
            if (lens[i] == l) {
                sym[at++] = (uint16_t)i;
                if (lut && l <= lut_bits)
                    for (uint32_t q = inf_rev(code, l); q < (1u << lut_bits); q += 1u << l) lut[q] = (uint16_t)(i << 4 | l);
                ++code;
            }
        code <<= 1;
    }
    return true;
}
// A word whose bytes lie at span offsets [off, off + 4): those outside [0, n) zeroed.
S3DG_CB_HD inline uint32_t inf_mask_word(uint32_t v, int64_t off, uint64_t n) {
    if (off >= 0 && (uint64_t)off + 4 <= n) return v;
    uint32_t m = 0;
    for (int q = 0; q < 4; ++q)
        if (off + q >= 0 && (uint64_t)(off + q) < n) m |= 0xFFu << (8 * q);
    return v & m;
}

// ---- the bit reader ------------------------------------------------------------------------
template <class E>
struct InfBits {
    E &env;
    uint64_t hold = 0, next = 0, used = 0;   // the bits not yet consumed, the next word, bits consumed
    uint32_t n = 0;                          // valid bits of hold
    S3DG_CB_HD explicit InfBits(E &e) : env(e) {}
    // Continue at byte `pos` of the span.
    S3DG_CB_HD void seek(uint64_t pos) {
        const uint64_t p = pos + env.lead();
        next = p / 4;
        const uint32_t drop = 8 * (uint32_t)(p & 3);
        hold = (uint64_t)env.word(next++) >> drop;
        n = 32 - drop;
        used = 8 * pos;
    }
    // At least 32 valid bits; the low ones of the result are the next of the stream.
    S3DG_CB_HD uint32_t peek() {
        if (n < 32) {
            hold |= (uint64_t)env.word(next++) << n;
            n += 32;
        }
        return (uint32_t)hold;
    }
    S3DG_CB_HD void drop(uint32_t k) {
        hold >>= k;
        n -= k;
        used += k;
    }
    S3DG_CB_HD uint32_t take(uint32_t k) {   // k <= 32
        const uint32_t v = peek() & (k == 32 ? 0xFFFFFFFFu : (1u << k) - 1);
        drop(k);
        return v;
    }
};

// The next symbol of a code: the first level, then the canonical walk bit by
// bit (counts and sorted symbols) for a longer code.  -1: the bits are no code.
template <class E>
S3DG_CB_HD inline int inf_symbol(InfBits<E> &B, const uint16_t *lut, uint32_t lut_bits, const uint16_t *count, const uint16_t *sym) {
    const uint32_t b = B.peek();
    const uint32_t e = lut_bits ? B.env.u(lut[b & ((1u << lut_bits) - 1)]) : 0u;
    if (e) {
        B.drop(e & 15);
        return (int)(e >> 4);
    }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= (b >> (l - 1)) & 1u;
        const uint32_t c = B.env.u(count[l]);
        if (code < first + c) {
            B.drop(l);
            return (int)B.env.u(sym[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// ---- the decoder ---------------------------------------------------------------------------
struct InfEnd {
    uint32_t status;
    uint64_t out_bytes, in_bytes;
};

// The bits that were no code may have been the zeros behind the span's end.
template <class E>
S3DG_CB_HD inline uint32_t inf_no_code(const InfBits<E> &B, uint64_t limit) {
    return B.used + 15 > limit ? (uint32_t)S3DG_INFLATE_TRUNCATED : (uint32_t)S3DG_INFLATE_BAD_STREAM;
}
// Room for `len` more bytes behind `out`: 0, or the status that ends the stream.
S3DG_CB_HD inline uint32_t inf_room(uint64_t out, uint64_t len, uint64_t cap, uint64_t want) {
    if (len > cap - out) return S3DG_INFLATE_CAPACITY;   // out <= cap always
    if (want != kInfAny && len > want - out) return S3DG_INFLATE_SIZE;
    return 0;
}

// The code lengths of a dynamic block into T.lens[0, nlit + ndist): 0, or the status.
template <class E>
S3DG_CB_HD inline uint32_t inf_dynamic_header(E &env, InfBits<E> &B, uint64_t limit, uint32_t *nlit_out, uint32_t *ndist_out) {
    InfTables &T = env.T();
    const uint32_t nlit = B.take(5) + 257, ndist = B.take(5) + 1, ncl = B.take(4) + 4;
    if (B.used > limit) return S3DG_INFLATE_TRUNCATED;
    if (nlit > kInfMaxLit || ndist > kInfMaxDist) return S3DG_INFLATE_BAD_STREAM;
    for (uint32_t i = 0; i < 19; ++i) env.put_lens(kInfClAt + inf_cl_order(i), 1, i < ncl ? B.take(3) : 0u);
    if (B.used > limit) return S3DG_INFLATE_TRUNCATED;
    // the code-length code uses the distance code's counts and symbols until the real one is built
    if (!env.build(T.lens + kInfClAt, 19, T.dist_count, T.dist_sym, nullptr, 0, true)) return S3DG_INFLATE_BAD_STREAM;
    uint32_t at = 0, prev = 0;
    while (at < nlit + ndist) {
        const int s = inf_symbol(B, (const uint16_t *)nullptr, 0, T.dist_count, T.dist_sym);
        if (s < 0) return inf_no_code(B, limit);
        uint32_t rep = 1, val = (uint32_t)s;
        if (s == 16) rep = 3 + B.take(2), val = prev;
        else if (s == 17) rep = 3 + B.take(3), val = 0;
        else if (s == 18) rep = 11 + B.take(7), val = 0;
        if (B.used > limit) return S3DG_INFLATE_TRUNCATED;
        if (s == 16 && at == 0) return S3DG_INFLATE_BAD_STREAM;
        if (rep > nlit + ndist - at) return S3DG_INFLATE_BAD_STREAM;
        env.put_lens(at, rep, val);
        at += rep;
        prev = val;
    }
    if (env.u(env.get_len(256)) == 0) return S3DG_INFLATE_BAD_STREAM;   // no end-of-block code
    *nlit_out = nlit;
    *ndist_out = ndist;
    return 0;
}

// One stream of src_bytes bytes into at most cap bytes (want: the size it must
// have, or kInfAny).  stored: the bytes are the output (a method 0 member).
template <class E>
S3DG_CB_HD inline InfEnd inf_run(E &env, uint64_t src_bytes, uint64_t cap, uint64_t want, bool stored) {
    const uint64_t limit = 8 * src_bytes;   // src_bytes is below 2^61: the descriptor check
    uint64_t out = 0;
    auto end = [&](uint32_t status, uint64_t used) -> InfEnd {
        const uint64_t in = used > limit ? src_bytes : (used + 7) / 8;
        if (status == 0 && want != kInfAny && out < want) status = S3DG_INFLATE_SIZE;
        return InfEnd{status, out, in};
    };
    if (stored) {
        if (const uint32_t r = inf_room(0, src_bytes, cap, want)) return end(r, 0);
        env.stored(0, src_bytes);
        out = src_bytes;
        return end(0, limit);
    }
    InfTables &T = env.T();
    InfBits<E> B(env);
    B.seek(0);
    for (;;) {
        const uint32_t hdr = B.take(3);
        if (B.used > limit) return end(S3DG_INFLATE_TRUNCATED, B.used);
        const uint32_t type = hdr >> 1;
        if (type == 3) return end(S3DG_INFLATE_BAD_STREAM, B.used);
        if (type == 0) {
            B.drop((uint32_t)(-(int64_t)B.used & 7));
            const uint32_t v = B.take(32), len = v & 0xFFFFu;
            if (B.used > limit) return end(S3DG_INFLATE_TRUNCATED, B.used);
            if (len != (~(v >> 16) & 0xFFFFu)) return end(S3DG_INFLATE_BAD_STREAM, B.used);
            const uint64_t pos = B.used / 8;
            if (len > src_bytes - pos) return end(S3DG_INFLATE_TRUNCATED, limit + 1);
            if (const uint32_t r = inf_room(out, len, cap, want)) return end(r, B.used);
            env.stored(pos, len);
            out += len;
            B.seek(pos + len);
        } else {
            uint32_t nlit = 288, ndist = 32;
            if (type == 1) {
                env.put_fixed();
            } else if (const uint32_t r = inf_dynamic_header(env, B, limit, &nlit, &ndist)) {
                return end(r, B.used);
            }
            if (!env.build(T.lens, nlit, T.lit_count, T.lit_sym, T.lit_lut, kInfLitBits, false) ||
                !env.build(T.lens + nlit, ndist, T.dist_count, T.dist_sym, T.dist_lut, kInfDistBits, false))
                return end(S3DG_INFLATE_BAD_STREAM, B.used);
            for (;;) {
                const int s = inf_symbol(B, T.lit_lut, kInfLitBits, T.lit_count, T.lit_sym);
                if (s < 0) return end(inf_no_code(B, limit), B.used);
                if (B.used > limit) return end(S3DG_INFLATE_TRUNCATED, B.used);
                if (s < 256) {
                    if (const uint32_t r = inf_room(out, 1, cap, want)) return end(r, B.used);
                    env.literal((uint32_t)s);
                    ++out;
                    continue;
                }
                if (s == 256) break;
                const uint32_t ls = (uint32_t)s - 257;
                if (ls >= 29) return end(S3DG_INFLATE_BAD_STREAM, B.used);
                const uint32_t len = inf_len_base(ls) + B.take(inf_len_extra(ls));
                const int d = inf_symbol(B, T.dist_lut, kInfDistBits, T.dist_count, T.dist_sym);
                if (d < 0) return end(inf_no_code(B, limit), B.used);
                if (B.used > limit) return end(S3DG_INFLATE_TRUNCATED, B.used);
                if (d >= 30) return end(S3DG_INFLATE_BAD_STREAM, B.used);
                const uint32_t dist = inf_dist_base((uint32_t)d) + B.take(inf_dist_extra((uint32_t)d));
                if (B.used > limit) return end(S3DG_INFLATE_TRUNCATED, B.used);
                if (dist > out) return end(S3DG_INFLATE_BAD_STREAM, B.used);   // in front of the first output byte
                if (const uint32_t r = inf_room(out, len, cap, want)) return end(r, B.used);
                env.match(len, dist);
                out += len;
            }
        }
        if (hdr & 1) return end(0, B.used);
    }
}

// ---- CRC-32 of a finished output ------------------------------------------------------------
// Entry i of the byte table; a * b mod P in the reflected domain with a fixed
// trip count (any a, zero included); x^(8 n) mod P.  With them the CRC-32 of
// A || B is mulmod(crc(A), x8n(|B|)) ^ crc(B), so 64 lanes hash 64 pieces.
S3DG_CB_HD inline uint32_t inf_crc_entry(uint32_t i) {
    for (int q = 0; q < 8; ++q) i = (i & 1) ? (i >> 1) ^ kInfCrcPoly : i >> 1;
    return i;
}
S3DG_CB_HD inline uint32_t inf_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int q = 0; q < 32; ++q) {
        if (a & (0x80000000u >> q)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ kInfCrcPoly : b >> 1;
    }
    return p;
}
S3DG_CB_HD inline uint32_t inf_x8n(uint64_t n) {
    uint32_t r = 0x80000000u, p = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1) r = inf_mulmod(r, p);
        p = inf_mulmod(p, p);
    }
    return r;
}
// Bytes per lane when 64 lanes share n bytes in pieces of 16.
S3DG_CB_HD inline uint64_t inf_crc_share(uint64_t n) { return ((n + 63) / 64 + 15) & ~15ull; }

// ---- the checks ----------------------------------------------------------------------------
inline std::string inf_at(uint64_t k, const char *what) {
    char b[160];
    snprintf(b, sizeof(b), "item %llu: %s", (unsigned long long)k, what);
    return b;
}
inline bool inf_check(uint64_t src_base, uint64_t dst_base, const s3dg_inflate_item *items, uint64_t n, bool total,
                      std::string *why) {
    if (n == 0) return true;
    if (!src_base) return *why = "null src_base", false;
    if (!dst_base) return *why = "null dst_base", false;
    if (!total) return *why = "null output", false;
    if (!items) return *why = "null item array", false;
    if (dst_base & 15u) return *why = "dst_base must be 16-byte aligned", false;
    if (n > kNpzMaxArchives) return *why = "more than 2^32 - 1 items in one call", false;
    for (uint64_t k = 0; k < n; ++k) {
        const s3dg_inflate_item t = items[k];
        if (t.dst_off & 15u) return *why = inf_at(k, "dst_off must be a multiple of 16"), false;
        if (t.src_bytes >= (1ull << 61) || src_base > UINT64_MAX - t.src_off || src_base + t.src_off > UINT64_MAX - t.src_bytes)
            return *why = inf_at(k, "src_off + src_bytes overflows"), false;
        if (dst_base > UINT64_MAX - t.dst_off || dst_base + t.dst_off > UINT64_MAX - t.dst_cap)
            return *why = inf_at(k, "dst_off + dst_cap overflows"), false;
        if (t.flags & ~1u) return *why = inf_at(k, "flags beyond bit 0"), false;
    }
    return true;
}
inline InfWork inf_work(uint64_t src_base, uint64_t dst_base, const s3dg_inflate_item &t) {
    return InfWork{src_base + t.src_off, t.src_bytes, dst_base + t.dst_off, t.dst_cap, t.want_bytes, t.crc, t.flags & kInfCrc};
}

// ---- NPZ with deflated members ---------------------------------------------------------------
// A z entry: the whole stored file of a member, compressed or not.
struct InzEntry {
    uint32_t local_off, name_flags, data_off, csize, usize, crc, method, zero;
};
static_assert(sizeof(InzEntry) == kNzuEntry, "a z entry is 32 bytes");
S3DG_CB_HD inline bool inz_supported(uint32_t flags, uint32_t method) { return (method == 0 || method == 8) && (flags & 9u) == 0; }
S3DG_CB_HD inline bool inz_entry_fits(const InzEntry &e, uint64_t bytes) {
    const uint64_t name_len = e.name_flags & 0xFFFFu;
    return (uint64_t)e.local_off + kNpzLocal + name_len <= e.data_off && (uint64_t)e.data_off + e.csize <= bytes &&
           (e.method == 8 || (e.method == 0 && e.csize == e.usize));
}
// A take's verdict on the device: status, span and the bytes its members should deliver.
struct InzDevTake {
    unsigned long long status, span, bytes, pad;
};
// nzu_check's refusals, less the bound on archive bytes; *ents the call's members.
inline bool inz_check(uint64_t base, uint64_t tab_base, uint64_t dst_base, const s3dg_npz_take *takes, uint64_t n, bool total,
                      uint64_t *ents, std::string *why) {
    *ents = 0;
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
        if (t.bytes >= (1ull << 61) || base > UINT64_MAX - t.off || base + t.off > UINT64_MAX - t.bytes)
            return *why = tfx_at(k, "off + bytes overflows"), false;
        if (dst_base > UINT64_MAX - t.dst_off || dst_base + t.dst_off > UINT64_MAX - t.dst_cap)
            return *why = tfx_at(k, "dst_off + dst_cap overflows"), false;
        const uint64_t last = t.first + t.count;
        if (last > (UINT64_MAX >> 5) || tab_base > UINT64_MAX - t.tab_off || tab_base + t.tab_off > UINT64_MAX - kNzuEntry * last)
            return *why = tfx_at(k, "tab_off + table overflows"), false;
        if (t.count > kNzuMaxEntries - *ents) return *why = tfx_at(k, "more than 2^31 - 2 members in one call"), false;
        *ents += t.count;
    }
    return true;
}

}  // namespace s3dg
