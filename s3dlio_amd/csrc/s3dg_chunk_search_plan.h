// s3dg_chunk_search_plan.h — the pure part of the chunker's parallel cut walk
// (S3DG_CHUNKS_SEARCH_WALK): chunk_walk's records for an
// object, found with parallelism inside the object.  Host-and-device functions,
// so the CPU sweep (tests/capi/chunk_search_plan_sweep.cpp) runs the very code
// the kernels of s3dg_chunk_search.hip run.  No HIP, no context.
//
// Nodes.  The nodes of an object are a root (the chunk start 0), an end (the
// object's last byte) and its candidates, the set bits of pass A's bitmap, in
// the order of their offsets: local numbers kCsRoot, kCsEnd, kCsFirst + i.  A
// node stands for "a chunk ended here": the walk goes on at its offset + 1.
// An exclusive sum over the per-granule candidate counts (gpre) numbers the
// candidates, so the first candidate at or after a position is found from two
// of its sums and a search among its own granule's candidates: empty granules
// are never looked at (cs_first_at).
//
// Links.  cs_link applies the cut rule from a node's chunk start to the next
// candidate that closes a chunk.  A stretch without candidates is taken in
// closed form: its forced chunks all start max_bytes apart, so a link is
// <target, forced chunks before the closing one>, and its records follow from
// the node's offset alone.  The end node links to itself with no chunk, and so
// does every unused node slot: doubling needs no test, and a node whose
// 1-link pair names itself has no record.
//
// Hops.  kCsHopLog rounds of doubling give <node, chunks> after 2^r links for
// every r; all levels are kept.  One wave per object follows the top level
// from the root and leaves an anchor <node, first record slot> per hop
// (cs_follow); link i of a hop is then reached through the set bits of i, at
// most kCsHopLog dependent loads (cs_fill_lane).
//
// Scratch.  An object's nodes are bounded by a function of its length alone
// (cs_node_bound: its record slots, twice its expected candidates and 64);
// kCsNodeBytes bytes per node: the offset (8), the forced count (4) and
// kCsHopLog + 1 levels of pairs (8 each).  An object with more candidates than
// that (a run of one byte that is a candidate everywhere) is walked by the
// serial chunk_walk: the decision is made on the device from the summed counts
// (CsObj.take), and each of the two walks leaves at once for the other's objects.
#pragma once
#include <stdint.h>

#include "s3dg_chunk_plan.h"
#include "s3dg_span_batch_plan.h"

namespace s3dg {

constexpr uint32_t kCsHopLog = 8, kCsHop = 1u << kCsHopLog;
constexpr uint32_t kCsRoot = 0, kCsEnd = 1, kCsFirst = 2;   // local node numbers
constexpr uint32_t kCsNone = 0xFFFFFFFFu;
constexpr uint64_t kCsMaxNodes = 0xFFFFFFF0ull;     // node numbers of one add are 32 bits
constexpr uint64_t kCsMaxGranules = 0x7FFFFFFEull;  // the scan counts granules + 1 in an int
constexpr uint32_t kCsNodeBytes = 8 + 4 + 8 * (kCsHopLog + 1);

struct CsHop {
    uint32_t node, chunks;   // the node reached and the chunks closed on the way
};
struct CsAnchor {
    uint32_t node, slot;     // a hop's first node and its first record slot; node kCsNone: unused
};
// One object of an add, built on the device once the counts are summed.
struct CsObj {
    uint64_t len, g0, nb;    // bytes; first granule among the add's; first node slot among the add's
    uint32_t r0, count;      // first record slot; candidates (when taken)
    uint32_t take, pad;      // 1: the search walks it; 0: chunk_walk does
};
static_assert(sizeof(CsHop) == 8 && sizeof(CsAnchor) == 8 && sizeof(CsObj) == 40, "node records");

// ---- the bound and the layout -----------------------------------------------------------
S3DG_SB_HD inline uint64_t cs_node_bound(uint64_t len, uint64_t min_bytes, uint64_t avg_bytes) {
    return (len + min_bytes - 1) / min_bytes + 1 + 2 * ((len + avg_bytes - 1) / avg_bytes) + 64;
}
// Node slots an object reserves: none below the threshold (threshold 0: the search is off).
S3DG_SB_HD inline uint64_t cs_reserved(uint64_t len, uint64_t threshold, uint64_t min_bytes, uint64_t avg_bytes) {
    return threshold && len >= threshold ? cs_node_bound(len, min_bytes, avg_bytes) : 0;
}
// Object j's first anchor slot when nb node slots are reserved before it: it
// has room for floor(bound / kCsHop) + 1 hops, and a path has fewer links than nodes.
S3DG_SB_HD inline uint64_t cs_anchor_base(uint64_t nb, uint64_t j) { return (nb >> kCsHopLog) + j; }

// The search's part of the stream's scratch, from `base` (a multiple of 256) on.
struct CsPlan {
    uint64_t nodes, anchors;   // node slots and anchor slots of the add
    uint64_t gpre_off, nb_off, obj_off, off_off, kf_off, lvl_off, anch_off, tmp_off, end;
};
inline CsPlan cs_plan(uint64_t base, uint64_t n_objs, uint64_t granules, uint64_t nodes, uint64_t scan_tmp_bytes) {
    CsPlan C;
    C.nodes = nodes;
    C.anchors = cs_anchor_base(nodes, n_objs);   // the objects' ranges, end to end
    C.gpre_off = base;
    C.nb_off = C.gpre_off + span_align256((granules + 1) * 8);
    C.obj_off = C.nb_off + span_align256((n_objs + 1) * 8);
    C.off_off = C.obj_off + span_align256(n_objs * sizeof(CsObj));
    C.kf_off = C.off_off + span_align256(nodes * 8);
    C.lvl_off = C.kf_off + span_align256(nodes * 4);
    C.anch_off = C.lvl_off + span_align256((kCsHopLog + 1) * nodes * sizeof(CsHop));
    C.tmp_off = C.anch_off + span_align256(C.anchors * sizeof(CsAnchor));
    C.end = C.tmp_off + span_align256(scan_tmp_bytes);
    return C;
}

// ---- objects ----------------------------------------------------------------------------
// The object that owns item i, objects sorted by `key` (obj[j].*key <= i for
// some j): the last such j.  Two objects may share a key (an object that
// reserves nothing); the last one is the one that owns something.
S3DG_SB_HD inline uint64_t cs_find_obj(const CsObj *obj, uint64_t n, uint64_t CsObj::*key, uint64_t i) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (obj[mid].*key <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
// Object j of len bytes from granule g0 and record slot r0 on, nb its first
// node slot and `reserved` their number; gpre the summed counts of the add.
S3DG_SB_HD inline CsObj cs_object(uint64_t len, uint64_t g0, uint64_t r0, uint64_t nb, uint64_t reserved,
                                  const uint64_t *gpre) {
    const uint64_t ng = (len + kMeasureGranule - 1) / kMeasureGranule, count = gpre[g0 + ng] - gpre[g0];
    const bool take = reserved != 0 && count + kCsFirst <= reserved;
    return CsObj{len, g0, nb, (uint32_t)r0, take ? (uint32_t)count : 0u, take ? 1u : 0u, 0u};
}

// ---- nodes --------------------------------------------------------------------------------
// The candidates of one bitmap word whose bit 0 is position p0, to out[0 ..).
S3DG_SB_HD inline void cs_word_nodes(uint64_t word, uint64_t p0, uint64_t *out) {
    for (uint32_t k = 0; word; word &= word - 1, ++k) out[k] = p0 + (uint32_t)__builtin_ctzll(word);
}

// What a link needs of its object: the add's node offsets, the summed counts
// from the object's first granule on, its first node slot, length and candidates.
struct CsView {
    const uint64_t *off, *gpre;
    uint64_t nb, len;
    uint32_t count;
};
// The first candidate at or after position x < len, as its index among the
// object's candidates; count: there is none.
S3DG_SB_HD inline uint32_t cs_first_at(const CsView &V, uint64_t x) {
    const uint64_t g = x / kMeasureGranule;
    uint64_t a = V.gpre[g] - V.gpre[0], b = V.gpre[g + 1] - V.gpre[0];   // granule g's candidates
    const uint64_t *o = V.off + V.nb + kCsFirst;
    while (a < b) {
        const uint64_t mid = a + (b - a) / 2;
        if (o[mid] < x) a = mid + 1;
        else b = mid;
    }
    return (uint32_t)a;   // none in the granule: the first one of a later granule
}

// ---- links --------------------------------------------------------------------------------
// chunk_walk from chunk start s up to the next candidate that closes a chunk:
// the local number of that node (kCsEnd: the object ends first), the forced
// chunks before it in *forced and all chunks, the closing one included, in
// *chunks.  The end closes a chunk only when bytes are left for one.
S3DG_SB_HD inline uint32_t cs_link(const CsView &V, uint64_t s, uint64_t minb, uint64_t maxb, uint32_t *forced,
                                   uint32_t *chunks) {
    uint64_t K = 0;
    for (;;) {
        if (s + minb - 1 >= V.len) break;          // a last chunk shorter than min, or nothing
        const uint32_t i = cs_first_at(V, s + minb - 1);
        if (i == V.count) break;
        const uint64_t d = V.off[V.nb + kCsFirst + i];
        if (d - s >= maxb) {                       // no candidate up to s + max - 1: chunks of max bytes up to d
            const uint64_t k = (d - s) / maxb;
            K += k;
            s += k * maxb;
            if (d < s + minb - 1) continue;        // d is skipped: below min in the chunk it falls in
        }
        *forced = (uint32_t)K;
        *chunks = (uint32_t)K + 1;
        return kCsFirst + i;
    }
    const uint64_t k = (V.len - s) / maxb;         // chunk_walk's cap < len: the chunks of max bytes that fit
    K += k;
    s += k * maxb;
    *forced = (uint32_t)K;
    *chunks = (uint32_t)K + (s < V.len);
    return kCsEnd;
}

// From pairs over 2^r links to pairs over 2^(r + 1).
S3DG_SB_HD inline CsHop cs_double(const CsHop *in, uint32_t x) {
    const CsHop a = in[x], b = in[a.node];
    return CsHop{b.node, a.chunks + b.chunks};
}

// ---- the follow and the fill ----------------------------------------------------------------
// The hops of object O from its root over the top level: an anchor per hop
// from anch[0] on (at most cap), their number in *hops; returns the object's
// chunks.  Only `writer` stores (lane 0 of the wave; the host).
S3DG_SB_HD inline uint32_t cs_follow(const CsObj &O, const CsHop *top, CsAnchor *anch, uint64_t cap, bool writer,
                                     uint64_t *hops) {
    const uint32_t end = (uint32_t)O.nb + kCsEnd;
    uint32_t x = (uint32_t)O.nb + kCsRoot, ord = 0;
    uint64_t k = 0;
    while (x != end && k < cap) {
        if (writer) anch[k] = CsAnchor{x, O.r0 + ord};
        const CsHop h = top[x];
        ord += h.chunks;
        x = h.node;
        ++k;
    }
    *hops = k;
    return ord;
}

// The records of one link: `forced` chunks of max bytes from byte s and slot
// `slot` on, then one of `last` bytes (0: none).
struct CsRec {
    uint64_t s;
    uint32_t forced, slot, last;
};
// Link idx (below kCsHop) of the hop that anchor A starts; false: the path
// ended before it.  lvl: the kept levels, `nodes` pairs each.
S3DG_SB_HD inline bool cs_fill_lane(const CsHop *lvl, uint64_t nodes, const uint64_t *off, const uint32_t *kf,
                                    CsAnchor A, uint32_t idx, uint64_t maxb, CsRec *out) {
    uint32_t x = A.node, slot = A.slot;
    for (int b = (int)kCsHopLog - 1; b >= 0; --b) {
        if (!((idx >> b) & 1u)) continue;
        const CsHop h = lvl[(uint64_t)b * nodes + x];
        slot += h.chunks;
        x = h.node;
    }
    const CsHop l = lvl[x];
    if (l.node == x) return false;                 // the end node
    const uint32_t K = kf[x];
    const uint64_t s = off[x] + 1;                 // the root's offset is -1
    *out = CsRec{s, K, slot, (uint32_t)(off[l.node] + 1 - (s + (uint64_t)K * maxb))};
    return true;
}

}  // namespace s3dg
