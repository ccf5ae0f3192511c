// s3dg_tfrecord_search_plan.h — the pure part of s3dg_tfrecord_index_search_batch
// (DESIGN.md §5.5.3): tfv_walk_host's result for every stream of a list, found
// with parallelism inside a stream.  Host-and-device functions, so the CPU
// sweep (tests/capi/tfrecord_search_plan_sweep.cpp) runs the very code the
// kernels of s3dg_tfrecord_search.hip run.  No HIP, no context.
//
// The walk never looks at the length CRC to decide where it goes, so the call
// has two halves: a search for the positions that look like headers, and the
// resolution of the one chain that starts at byte 0.
//
// Candidates.  Position p of a stream is a candidate when its record fits
// (16 + len <= bytes - p) and masked_crc of its 8 length bytes is its CRC
// field.  A candidate therefore always fits, and a position the walk reaches
// that is no candidate is read from the raw bytes, by the walk's own rule
// (tfv_walk_step): that read says whether the walk ends there, is truncated
// there or steps through a header whose CRC is wrong, so a link needs no kind
// of terminal, only kTfsNone.
//
// Tiles.  Stream k is cut into tfs_tiles(bytes) tiles of kTfsTile positions;
// tile0[k] is its first tile among the call's.  A tile has one bit per
// position (kTfsTileWords 64-bit words), the number of candidates before each
// word inside the tile (16 bits), and, after an exclusive sum over the tiles'
// counts, the number of candidates before the tile in the call: a candidate's
// node number is the sum of the three (tfs_node_at, two loads once the word is
// there).  A stream listed twice has two sets of tiles and of nodes.
//
// Nodes.  Per node: its index entry <pos, 16 + len>, next (the node at
// pos + 16 + len, or kTfsNone), and after kTfsHopLog rounds of doubling the pair
// <node, steps> reached by at most kTfsHop links: steps below kTfsHop say that
// the chain ends at that node, whose own next is kTfsNone.  A pair always names
// a node, so the position behind a chain's last record is one load away.
//
// Anchors.  One wave per stream follows the hops from byte 0 and leaves one
// anchor <node, count, where in the index> per hop; a thread per anchor then
// follows `count` single links and stores the entries.  Every anchor starts at
// another node of the stream's chain, so the stream's own range of node
// numbers has room for them.
#pragma once
#include <stdint.h>

#include "s3dg_tfrecord_var_plan.h"

namespace s3dg {

constexpr uint32_t kTfsTile = 16384;                 // positions per tile: 64 per lane of a 256-thread workgroup
constexpr uint32_t kTfsTileWords = kTfsTile / 64;
constexpr uint32_t kTfsHopLog = 9, kTfsHop = 1u << kTfsHopLog;
constexpr uint32_t kTfsNone = 0xFFFFFFFFu;
constexpr uint64_t kTfsMaxNodes = 0xFFFFFFF0ull;     // node numbers are 32 bits
constexpr uint64_t kTfsMaxTiles = 0x7FFFFFFEull;     // the scan counts tiles + 1 in an int
constexpr uint32_t kTfsCrcTabWords = 8 * 256;

struct alignas(16) TfsEnt {
    uint64_t pos, size;   // the index entry
};
struct TfsHop {
    uint32_t node, steps;
};
struct alignas(16) TfsAnchor {
    uint32_t node, count;   // count == 0: unused
    uint64_t idx_at;        // idx_off + 16 * (the first record's number)
};
static_assert(sizeof(TfsEnt) == 16 && sizeof(TfsHop) == 8 && sizeof(TfsAnchor) == 16, "node records");

struct TfsMap {
    const uint64_t *bm;      // one bit per position, kTfsTileWords words per tile
    const uint16_t *wpre;    // candidates of the tile before the word
    const uint64_t *tbase;   // candidates of the call before the tile
};

// ---- tiles ---------------------------------------------------------------------------
S3DG_CB_HD inline uint64_t tfs_tiles(uint64_t bytes) { return bytes / kTfsTile + (bytes % kTfsTile != 0); }
// tile0[0 .. n]: every stream's first tile and the call's tiles; false beyond kTfsMaxTiles.
inline bool tfs_tile_table(const s3dg_tfrecord_stream *streams, uint64_t n, uint64_t *tile0) {
    uint64_t t = 0;
    for (uint64_t k = 0; k < n; ++k) {
        tile0[k] = t;
        const uint64_t m = tfs_tiles(streams[k].bytes);
        if (m > kTfsMaxTiles - t) return false;
        t += m;
    }
    tile0[n] = t;
    return true;
}
// The stream that owns tile g (below the call's tiles): the last one whose first tile is at or below g.
S3DG_CB_HD inline uint64_t tfs_find_stream(const uint64_t *tile0, uint64_t n, uint64_t g) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (tile0[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- the workspace -------------------------------------------------------------------
// Before the count: [streams][tile0] uploaded, then the results, the tiles'
// bases (tiles + 1), the bitmap, the words' prefixes and the scan's scratch.
struct TfsPlanA {
    uint64_t tile0_off, upload_bytes, res_off, tbase_off, bm_off, wpre_off, tmp_off, bytes;
};
inline TfsPlanA tfs_plan_a(uint64_t n, uint64_t tiles, uint64_t scan_tmp_bytes) {
    TfsPlanA A;
    A.tile0_off = span_align256(n * sizeof(s3dg_tfrecord_stream));
    A.upload_bytes = A.tile0_off + (n + 1) * 8;
    A.res_off = span_align256(A.upload_bytes);
    A.tbase_off = A.res_off + span_align256(n * sizeof(s3dg_tfrecord_walk_result));
    A.bm_off = A.tbase_off + span_align256((tiles + 1) * 8);
    A.wpre_off = A.bm_off + span_align256(tiles * kTfsTileWords * 8);
    A.tmp_off = A.wpre_off + span_align256(tiles * kTfsTileWords * 2);
    A.bytes = A.tmp_off + span_align256(scan_tmp_bytes);
    return A;
}
// After it: 52 bytes per candidate.
struct TfsPlanB {
    uint64_t ent_off, anch_off, hop_off[2], next_off, bytes;
};
inline TfsPlanB tfs_plan_b(uint64_t nodes) {
    TfsPlanB B;
    B.ent_off = 0;
    B.anch_off = span_align256(nodes * sizeof(TfsEnt));
    B.hop_off[0] = B.anch_off + span_align256(nodes * sizeof(TfsAnchor));
    B.hop_off[1] = B.hop_off[0] + span_align256(nodes * sizeof(TfsHop));
    B.next_off = B.hop_off[1] + span_align256(nodes * sizeof(TfsHop));
    B.bytes = B.next_off + span_align256(nodes * 4);
    return B;
}

// ---- the length CRC from byte tables -------------------------------------------------
// tfv_len_mcrc is f(f(~0 ^ lo) ^ hi) with f 32 shift steps, which are linear:
// f(f(~0)) ^ sum over the bytes of lo of f(f(byte)) ^ sum over hi's of f(byte).
S3DG_CB_HD inline uint32_t tfs_shift32(uint32_t c) {
    for (int b = 0; b < 32; ++b) c = (c >> 1) ^ (kCrcBatchPoly & (0u - (c & 1)));
    return c;
}
// Entry e of the 8 tables of 256: byte e >> 8 of the length with value e & 255.
S3DG_CB_HD inline uint32_t tfs_crc_tab_entry(uint32_t e) {
    const uint32_t b = e >> 8;
    uint32_t x = tfs_shift32((e & 255u) << (8 * (b & 3)));
    if (b < 4) x = tfs_shift32(x);
    return x;
}
S3DG_CB_HD inline uint32_t tfs_crc_const() { return tfs_shift32(tfs_shift32(0xFFFFFFFFu)); }
S3DG_CB_HD inline uint32_t tfs_len_mcrc_tab(const uint32_t *tab, uint32_t k, uint64_t len) {
    uint32_t c = k;
    for (uint32_t b = 0; b < 8; ++b) c ^= tab[256 * b + (uint32_t)((len >> (8 * b)) & 255u)];
    return tfr_masked(~c);
}

// ---- candidates and nodes ------------------------------------------------------------
S3DG_CB_HD inline bool tfs_fits(uint64_t left, uint64_t len) { return left >= kTfrFraming && len <= left - kTfrFraming; }
// The 12 header bytes at p, all inside the stream: byte loads.
S3DG_CB_HD inline void tfs_header(const uint8_t *p, uint64_t *len, uint32_t *crc) {
    uint64_t l = 0;
    uint32_t c = 0;
    for (int b = 0; b < 8; ++b) l |= (uint64_t)p[b] << (8 * b);
    for (int b = 0; b < 4; ++b) c |= (uint32_t)p[8 + b] << (8 * b);
    *len = l;
    *crc = c;
}
// The node at position pos of the stream whose first tile is tile_first, or kTfsNone.
S3DG_CB_HD inline uint32_t tfs_node_at(const TfsMap &M, uint64_t tile_first, uint64_t pos) {
    const uint64_t g = tile_first + pos / kTfsTile, w = g * kTfsTileWords + (pos % kTfsTile) / 64;
    const uint32_t b = (uint32_t)(pos & 63u);
    const uint64_t word = M.bm[w];
    if (!((word >> b) & 1u)) return kTfsNone;
    return (uint32_t)(M.tbase[g] + M.wpre[w] + (uint64_t)__builtin_popcountll(word & ((1ull << b) - 1)));
}
// Where the record <pos, size> of a stream of `bytes` leads.
S3DG_CB_HD inline uint32_t tfs_link(const TfsMap &M, uint64_t tile_first, uint64_t bytes, uint64_t pos, uint64_t size) {
    const uint64_t next = pos + size;   // at most bytes: the record fits
    if (!tfv_walk_has_header(bytes - next)) return kTfsNone;
    return tfs_node_at(M, tile_first, next);
}

// ---- hops ----------------------------------------------------------------------------
S3DG_CB_HD inline TfsHop tfs_hop0(uint32_t x, uint32_t next) { return next != kTfsNone ? TfsHop{next, 1u} : TfsHop{x, 0u}; }
// From pairs of at most `full` links to pairs of at most 2 * full.
S3DG_CB_HD inline TfsHop tfs_double(const TfsHop *in, uint32_t x, uint32_t full) {
    const TfsHop a = in[x];
    if (a.steps != full) return a;   // the chain ended on the way
    const TfsHop b = in[a.node];
    return TfsHop{b.node, a.steps + b.steps};
}

// ---- the anchor walk -----------------------------------------------------------------
// tfv_walk_host over the graph: p is the stream's first byte, node numbers of
// the stream start at tbase[tile_first] and so do its anchors.  A position that
// is no node takes the walk's own step from the raw bytes and stores its entry
// here.  Only `writer` stores (lane 0 of the wave; the host).
S3DG_CB_HD inline s3dg_tfrecord_walk_result tfs_anchor_walk(const uint8_t *p, const s3dg_tfrecord_stream &Sd, const TfsMap &M,
                                                            uint64_t tile_first, const TfsEnt *ent, const uint32_t *next,
                                                            const TfsHop *hop, TfsAnchor *anch, uint8_t *idx, bool writer) {
    s3dg_tfrecord_walk_result R{0, 0, 0, 0, 0, UINT64_MAX};
    uint64_t pos = 0, na = 0;
    uint32_t x = kTfsNone;
    for (;;) {
        if (x == kTfsNone) {
            const uint64_t left = Sd.bytes - pos;
            if (!tfv_walk_has_header(left)) break;
            if (R.records == Sd.max_records) {
                R.status = 2;
                break;
            }
            x = tfs_node_at(M, tile_first, pos);
            if (x == kTfsNone) {
                uint64_t len, size = 0;
                uint32_t crc;
                tfs_header(p + pos, &len, &crc);
                if (tfv_walk_step(left, len, &size) != kTfvWalkRecord) {
                    R.status = 1;
                    break;
                }
                if (writer) *reinterpret_cast<TfsEnt *>(idx + Sd.idx_off + 16 * R.records) = TfsEnt{pos, size};
                if (tfv_len_mcrc(len) != crc) {
                    ++R.bad_length_crc;
                    if (R.first_bad_record == UINT64_MAX) R.first_bad_record = R.records;
                }
                ++R.records;
                pos += size;
                continue;
            }
        }
        if (R.records == Sd.max_records) {   // a node has its 12 bytes
            R.status = 2;
            pos = ent[x].pos;
            break;
        }
        const uint64_t room = Sd.max_records - R.records;
        const TfsHop h = hop[x];
        const bool ends = h.steps != kTfsHop;               // at h.node, which is the chain's last record
        const uint32_t avail = ends ? h.steps + 1 : kTfsHop;
        const uint32_t take = room < avail ? (uint32_t)room : avail;
        if (writer) anch[M.tbase[tile_first] + na] = TfsAnchor{x, take, Sd.idx_off + 16 * R.records};
        ++na;
        R.records += take;
        if (take != avail) {                                // max_records inside the hop: the node it stops at
            for (uint32_t i = 0; i < take; ++i) x = next[x];
        } else if (ends) {
            const TfsEnt e = ent[h.node];
            pos = e.pos + e.size;
            x = kTfsNone;
        } else {
            x = h.node;
        }
    }
    R.stop_offset = pos;
    R.trailing = Sd.bytes - pos;
    return R;
}

// One anchor's entries.
S3DG_CB_HD inline void tfs_fill(const TfsAnchor &A, const TfsEnt *ent, const uint32_t *next, uint8_t *idx) {
    TfsEnt *out = reinterpret_cast<TfsEnt *>(idx + A.idx_at);
    uint32_t x = A.node;
    for (uint32_t i = 0; i < A.count; ++i) {
        const TfsEnt e = ent[x];
        x = next[x];
        out[i] = e;
    }
}

}  // namespace s3dg
