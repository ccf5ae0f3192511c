// Stand-alone sweep of the batch fill's records (s3dg_batch_plan.h and
// s3dg_prefix.h, g++ alone, no HIP): for a descriptor set it runs the host's
// pass, the plan, a host exclusive sum of the shared tile-count function per
// class and the shared record-range functions, the very functions the device's
// scan functor and k_batch_map call, then walks every slot of every class's
// launch as k_fill_batch maps it, and asserts
//   (i)    every 4 KiB block of every non-empty object is hit by exactly one live slot;
//   (ii)   no live slot maps outside [0, nb): lead slots and slots past the end are dead;
//   (iii)  every record in [0, B.recs) is written by exactly one object (dense gap
//          records included), and B.recs, each class's recs and rec0 are the walk's;
//   (iv)   P.ntiles[sh] and P.ntiles_s[sh] are the sums of the shared tile count;
//   (v)    two classes partition the staged objects by nb < split, stably, no empties;
//   (vi)   slot = granule of the block it writes, modulo 8 for the dense layout
//          and tiles of 8 blocks and more, modulo the tile for 2- and 4-block
//          tiles (where modulo 8 does not hold: counted and printed);
//   (vii)  the pass merged from 1..8 parts equals the pass in one part;
//   (viii) the own / whole-wave writer of k_batch_map is chosen at 16 records.
// A uniform sub-batch (a stream) must be exactly the stream its descriptors say,
// and the tiled stream route's records are walked the same way.
//
// No arguments: the generated sets and the prefix sweep; prints counters.
// "cases": reads lists from stdin ("list name base tile split n", then n lines
// "off size entropy dedup f_num f_den"), cuts each into the call's sub-batches
// and prints every sub-batch's plan.  Exits non-zero on the first miss.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "s3dg_batch_plan.h"
#include "s3dg_prefix.h"

using namespace s3dg;

#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond);  \
            fprintf(stderr, __VA_ARGS__);                                             \
            fprintf(stderr, "\n");                                                    \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

typedef std::vector<s3dg_obj_desc> Descs;

static uint64_t n_sub = 0, n_uniform = 0, n_dense = 0, n_two = 0, n_merge = 0, n_prefix = 0;
static uint64_t recs16[kTileShiftMax + 1], recs17[kTileShiftMax + 1], wave2[kTileShiftMax + 1];
static uint64_t xcd8_miss[kTileShiftMax + 1], live_slots[kTileShiftMax + 1];

static bool same_desc(const s3dg_obj_desc &a, const s3dg_obj_desc &b) {
    return a.dst_off == b.dst_off && a.size == b.size && a.entropy == b.entropy && a.dedup == b.dedup &&
           a.f_num == b.f_num && a.f_den == b.f_den;
}

// (vii) the pass over d[0, n) cut at `cut[0..parts]` and merged, against the pass in one part
static void check_merge(const Descs &d, uintptr_t base, uint64_t split, const BatchScan &P1, const Descs &H1,
                        const uint64_t *cut, int parts) {
    BatchScan part[kPrepParts];
    Descs H(d.size() + 1);
    for (int q = 0; q < parts; ++q) batch_scan(d.data(), cut[q], cut[q + 1], base, part[q], H.data() + cut[q], split);
    const BatchScan P = batch_scan_merge(part, parts);
    CHECK(P.err == P1.err, "merge err");
    if (P.err) return;
    CHECK(P.m == P1.m && P.blocks == P1.blocks && P.ms == P1.ms && P.blocks_s == P1.blocks_s, "merge counts");
    for (int k = 0; k < 3; ++k) CHECK(P.zc_blocks[k] == P1.zc_blocks[k], "merge zc %d", k);
    for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh)
        CHECK(P.ntiles[sh] == P1.ntiles[sh] && P.ntiles_s[sh] == P1.ntiles_s[sh], "merge ntiles %u", sh);
    if (P.m) {
        CHECK(P.first_off == P1.first_off && P.last_end == P1.last_end, "merge range");
        CHECK(P.dense_ok == P1.dense_ok, "merge dense %d parts", parts);
        CHECK(P.uni == P1.uni, "merge uni %d parts", parts);
        CHECK(same_desc(P.ufirst, P1.ufirst) && same_desc(P.ulast, P1.ulast), "merge run ends");
        if (P.uni && P.m >= 2) CHECK(P.ustride == P1.ustride, "merge stride");
    }
    for (size_t k = 0; k < d.size(); ++k) CHECK(same_desc(H[k], H1[k]), "merge staging %zu", k);
    ++n_merge;
}

// Walk of one class's launch: records of staged objects S[0, count) at tile shift tshift (0: dense).
static void walk_class(const s3dg_obj_desc *S, uint64_t count, uint32_t tshift, uint64_t recs, uintptr_t base,
                       uint64_t lead0, uint64_t first_off) {
    std::vector<uint64_t> scan(count + 1, 0);
    if (tshift)   // (the device: hipCUB exclusive sum of the same function)
        for (uint64_t k = 0; k < count; ++k)
            scan[k + 1] = scan[k] + obj_tiles(obj_blocks(S[k].size), obj_lead(base, S[k].dst_off), tshift);
    std::vector<RecRange> R(count);
    std::vector<int64_t> owner(recs, -1);
    uint64_t written = 0;
    for (uint64_t k = 0; k < count; ++k) {
        const s3dg_obj_desc &o = S[k];
        const uint64_t nb = obj_blocks(o.size);
        CHECK(o.size != 0, "an empty object is staged");
        R[k] = tshift ? tiled_records(scan[k], nb, base, o.dst_off, tshift)
                      : dense_records(k == 0, lead0, first_off, o.dst_off, nb, k + 1 < count,
                                      k + 1 < count ? S[k + 1].dst_off : 0);
        CHECK(R[k].lo <= R[k].hi && R[k].hi <= recs, "object %" PRIu64 ": records [%" PRIu64 ", %" PRIu64 ") of %" PRIu64,
              k, R[k].lo, R[k].hi, recs);
        CHECK(R[k].lead < (1ull << 32), "lead");
        const uint64_t nrec = R[k].hi - R[k].lo;
        // (viii) the writer k_batch_map picks
        CHECK(map_own_records(nrec) == (nrec <= 16), "own/wave cut at %" PRIu64 " records", nrec);
        recs16[tshift] += nrec == 16;
        recs17[tshift] += nrec == 17;
        wave2[tshift] += nrec > 64;
        for (uint64_t q = R[k].lo; q < R[k].hi; ++q) {   // (iii)
            CHECK(owner[q] < 0, "record %" PRIu64 " written by objects %" PRId64 " and %" PRIu64, q, owner[q], k);
            owner[q] = (int64_t)k;
        }
        written += nrec;
    }
    CHECK(written == recs, "records written %" PRIu64 ", launched %" PRIu64 " (shift %u)", written, recs, tshift);
    // every slot of the launch, as k_fill_batch maps it
    std::vector<std::vector<uint8_t>> hit(count);
    for (uint64_t k = 0; k < count; ++k) hit[k].assign(obj_blocks(S[k].size), 0);
    const uint64_t modulo = tshift == 0 || tshift >= 3 ? 8 : 1ull << tshift;
    for (uint64_t g = 0; g < recs << tshift; ++g) {
        const uint64_t q = g >> tshift;
        const uint32_t kk = (uint32_t)(g & ((1u << tshift) - 1));
        const uint64_t k = (uint64_t)owner[q];
        const s3dg_obj_desc &o = S[k];
        const uint32_t first = (uint32_t)((q - R[k].lo) << tshift);
        CHECK(((q - R[k].lo) << tshift) < (1ull << 32), "first overflows");
        const int64_t ib = slot_block(first, kk, (uint32_t)R[k].lead);
        // a lead slot is dead by the kernel's size test alone too: as unsigned it lies far past any object
        if (ib < 0) CHECK((uint64_t)ib * kBlk >= o.size && (uint64_t)(uint32_t)ib * kBlk >= o.size, "lead slot %" PRIu64, g);
        if (ib < 0 || (uint64_t)ib * kBlk >= o.size) continue;   // dead: lead slot or past the end
        CHECK((uint64_t)ib < hit[k].size(), "slot %" PRIu64 ": block %" PRId64 " outside the object", g, ib);   // (ii)
        CHECK(hit[k][ib] == 0, "object %" PRIu64 " block %" PRId64 " hit twice", k, ib);                      // (i)
        hit[k][ib] = 1;
        const uint64_t granule = ((uint64_t)base + o.dst_off + (uint64_t)ib * kBlk) >> 12;
        CHECK((g - granule) % modulo == 0, "slot %" PRIu64 " writes granule %" PRIu64 " (shift %u)", g, granule, tshift);  // (vi)
        ++live_slots[tshift];
        xcd8_miss[tshift] += (g - granule) % 8 != 0;
    }
    for (uint64_t k = 0; k < count; ++k)
        for (size_t i = 0; i < hit[k].size(); ++i) CHECK(hit[k][i] == 1, "object %" PRIu64 " block %zu never hit", k, i);
}

// A uniform sub-batch: the stream (ufirst, ustride, m) is the descriptors' objects,
// and the tiled stream route's records (fill_uniform, k_tile_map_uniform) cover one object.
static void check_uniform(const Descs &live, const BatchScan &P, uintptr_t base) {
    CHECK(P.m == live.size() && P.m >= 2, "uniform m");
    for (uint64_t j = 0; j < P.m; ++j) {
        const s3dg_obj_desc &o = live[j];
        CHECK(o.dst_off == P.ufirst.dst_off + j * P.ustride && o.size == P.ufirst.size &&
                  o.entropy == P.ufirst.entropy + (j << 32) && o.dedup == P.ufirst.dedup &&
                  o.f_num == P.ufirst.f_num && o.f_den == P.ufirst.f_den,
              "stream object %" PRIu64, j);
    }
    CHECK(P.ustride >= P.ufirst.size && P.ustride % 16 == 0, "stride");
    const uint64_t nb = obj_blocks(P.ufirst.size), dst = (uint64_t)base + P.ufirst.dst_off;
    const uint64_t lead = obj_lead(dst, 0);
    CHECK(lead == obj_lead(base, P.ufirst.dst_off), "stream lead");
    for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) {
        const uint64_t tpo = obj_tiles(nb, lead, sh);
        std::vector<uint8_t> hit(nb, 0);
        for (uint64_t s = 0; s < tpo << sh; ++s) {
            const int64_t ib = slot_block((uint32_t)((s >> sh) << sh), (uint32_t)(s & ((1u << sh) - 1)), (uint32_t)lead);
            if (ib < 0 || (uint64_t)ib * kBlk >= P.ufirst.size) continue;
            CHECK((uint64_t)ib < nb && !hit[ib], "stream slot %" PRIu64, s);
            hit[ib] = 1;
            // objects at a multiple of 32 KiB (the tiled route's condition) keep slot = granule
            if (P.ustride % (8 * kBlk) == 0) {
                const uint64_t modulo = sh >= 3 ? 8 : 1ull << sh;
                for (uint64_t j : {(uint64_t)0, (uint64_t)1, P.m - 1})
                    CHECK(((j * tpo << sh) + s - ((dst + j * P.ustride + (uint64_t)ib * kBlk) >> 12)) % modulo == 0,
                          "stream slot %" PRIu64 " of object %" PRIu64, s, j);
            }
        }
        for (uint64_t i = 0; i < nb; ++i) CHECK(hit[i], "stream block %" PRIu64 " never hit", i);
    }
    ++n_uniform;
}

// One sub-batch d[0, n) under knobs K.  Returns its plan as text.
static std::string check_sub(const Descs &d, uintptr_t base, const BatchKnobs &K, bool merges) {
    const uint64_t n = d.size(), split = K.split_blocks;
    BatchScan P;
    Descs H(n + 1);
    batch_scan(d.data(), 0, n, base, P, H.data(), split);
    CHECK(!P.err, "refused: %s", P.msg);
    if (merges) {   // (vii)
        uint64_t cut[kPrepParts + 1];
        for (int parts = 1; parts <= kPrepParts; ++parts) {
            for (int q = 0; q <= parts; ++q) cut[q] = batch_cut(0, n, q, parts);
            check_merge(d, base, split, P, H, cut, parts);
        }
        for (uint64_t c = 0; c <= n; ++c) {
            const uint64_t two[3] = {0, c, n};
            check_merge(d, base, split, P, H, two, 2);
            const uint64_t three[4] = {0, c / 2, c, n};
            check_merge(d, base, split, P, H, three, 3);
        }
    }
    // (iv) the pass's sums, from the shared functions
    Descs live;
    uint64_t blocks = 0, ms = 0, blocks_s = 0, nt[kTileShiftMax + 1] = {}, nts[kTileShiftMax + 1] = {};
    for (const auto &o : d) {
        if (!o.size) continue;
        live.push_back(o);
        const uint64_t nb = (o.size + 4095) / 4096;
        CHECK(nb == obj_blocks(o.size), "obj_blocks");
        blocks += nb;
        ms += nb < split;
        blocks_s += nb < split ? nb : 0;
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) {
            const uint64_t t = obj_tiles(nb, obj_lead(base, o.dst_off), sh);
            nt[sh] += t;
            if (nb < split) nts[sh] += t;
        }
    }
    CHECK(P.m == live.size() && P.blocks == blocks && P.ms == ms && P.blocks_s == blocks_s, "pass counts");
    for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh)
        CHECK(P.ntiles[sh] == nt[sh] && P.ntiles_s[sh] == nts[sh], "ntiles at shift %u", sh);
    ++n_sub;
    if (P.m == 0) return "empty";
    const BatchPlan B = plan_sub_batch(P, base, K);
    if (B.uniform) {
        CHECK(!K.tile_shift && !K.force_dense, "a forced layout ran as a stream");
        check_uniform(live, P, base);
        return "uniform";
    }
    CHECK(B.lead0 == ((((uint64_t)base + live[0].dst_off) >> 12) & 7), "lead0");
    order_staging(H.data(), n, P.m, B, split);
    CHECK(B.nclass == 1 || B.nclass == 2, "nclass");
    // (v) the staged order
    if (B.nclass == 1) {
        CHECK(B.cls[0].first == 0 && B.cls[0].count == P.m, "one class holds every object");
        for (uint64_t k = 0; k < P.m; ++k) CHECK(same_desc(H[k], live[k]), "staged %" PRIu64, k);
    } else {
        CHECK(B.tshift != 0 && !K.tile_shift && split, "two classes need a split and no forced layout");
        CHECK(B.cls[0].first == 0 && B.cls[0].count == ms && B.cls[1].first == ms && B.cls[1].count == P.m - ms &&
                  ms > 0 && ms < P.m,
              "classes by nb < split");
        CHECK(B.cls[0].tshift != B.cls[1].tshift, "two classes of one tile");
        uint64_t a = 0, b = ms;
        for (const auto &o : live) {   // stable: each class in the caller's order
            uint64_t &at = (o.size + 4095) / 4096 < split ? a : b;
            CHECK(same_desc(H[at], o), "staged %" PRIu64, at);
            ++at;
        }
        CHECK(a == ms && b == P.m, "partition");
        ++n_two;
    }
    // (iii) the classes tile the record map
    uint64_t rec0 = 0;
    std::string text = B.tshift ? "tiled" : "dense";
    for (int q = 0; q < B.nclass; ++q) {
        const auto &C = B.cls[q];
        CHECK(C.rec0 == rec0, "class %d rec0", q);
        CHECK(B.tshift ? C.tshift >= kTileShiftMin && C.tshift <= kTileShiftMax : C.tshift == 0, "class shift");
        if (K.tile_shift) CHECK(C.tshift == K.tile_shift, "forced tile");
        walk_class(H.data() + C.first, C.count, C.tshift, C.recs, base, B.lead0, P.first_off);
        rec0 += C.recs;
        if (B.tshift) text += (q ? "+" : ":") + std::to_string(C.tshift);
    }
    CHECK(rec0 == B.recs, "B.recs");
    if (!B.tshift) {
        CHECK(P.dense_ok && B.recs == B.span, "dense span");
        ++n_dense;
    }
    return text;
}

// ---- the generated sets ------------------------------------------------------------

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One object of the size edges: blocks nb = m * T - lead + delta at its place
// (so nb + lead = m T - 1, m T, m T + 1), the last block holding `tail` bytes.
struct Edge {
    uint32_t m, T;
    int delta;
    uint32_t tail;
};

static Descs make_set(const std::vector<Edge> &edges, uintptr_t base, bool packed, int order, int empties,
                      uint64_t gap_granules) {
    Descs d;
    uint64_t off = 0, seed = 1;
    const uint32_t ratios[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}};
    for (size_t j = 0; j < edges.size(); ++j) {
        const Edge &e = edges[j];
        if (empties == 2 || (empties == 1 && (j == 0 || j + 1 == edges.size())))
            d.push_back(s3dg_obj_desc{off, 0, 77, 9, 5, 0});   // an empty object may say anything
        const uint64_t lead = obj_lead(base, off);
        int64_t nb = (int64_t)e.m * e.T - (int64_t)lead + e.delta;
        if (nb < 1) nb = 1;
        const uint64_t size = (uint64_t)(nb - 1) * kBlk + e.tail;
        d.push_back(s3dg_obj_desc{off, size, (seed++ << 32) ^ 0xABCD, j % 4, ratios[j % 4][0], ratios[j % 4][1]});
        off += packed ? (size + 15) / 16 * 16 + 16 * (j % 3) : (uint64_t)nb * kBlk + ((j % 4 == 1) ? gap_granules * kBlk : 0);
    }
    if (empties == 1) d.push_back(s3dg_obj_desc{0, 0, 0, 1, 0, 1});
    if (order == 1) std::reverse(d.begin(), d.end());
    if (order == 2)
        for (size_t k = d.size(); k > 1; --k) std::swap(d[k - 1], d[rnd() % k]);
    return d;
}

static void sweep_sets() {
    const uint32_t tiles[] = {0, 1, 2, 4, 8, 16, 32, 64};   // 0 auto, 1 dense where the layout allows
    const uint32_t splits[] = {0, 2, 16};
    const uint32_t tails[] = {1, 4095, 4096, 16};
    for (uint32_t T : {2u, 4u, 8u, 16u, 32u, 64u}) {
        // the size edges around one and two tiles, and 16 / 17 / 65 records
        std::vector<Edge> edges;
        uint32_t t = 0;
        for (uint32_t m : {1u, 2u, 16u, 17u, 65u})
            for (int delta : {-1, 0, 1}) {
                if (m == 65 && (T > 8 || delta)) continue;   // the second pass of the wave loop, small tiles only
                edges.push_back(Edge{m, T, delta, tails[t++ % 4]});
            }
        edges.push_back(Edge{0, T, 0, 1});    // a 1-byte object
        edges.push_back(Edge{0, T, 0, 16});   // a 16-byte object
        for (uint32_t gran = 0; gran < 8; ++gran)
            for (uint32_t sub : {0u, 16u}) {
                const uintptr_t base = (uintptr_t)0x7F3A00000000ull + gran * kBlk + sub;
                for (int packed = 0; packed < 2; ++packed)
                    for (int order = 0; order < 3; ++order)
                        for (int empties = 0; empties < 3; ++empties) {
                            const uint64_t gaps[] = {0, 1, 15, 16, 17, 63, 64, 65, 200};
                            const Descs d = make_set(edges, base, packed, order, empties, gaps[(gran + T + order) % 9]);
                            const bool merges = T == 2 && sub == 0 && gran % 3 == 0;
                            for (uint32_t tile : tiles)
                                for (uint32_t split : splits) {
                                    uint32_t sh = 0;
                                    while ((1u << sh) < tile) ++sh;
                                    const BatchKnobs K{tile > 1 ? sh : 0, tile == 1, split};
                                    (void)check_sub(d, base, K, merges && tile == 0);
                                }
                        }
            }
    }
    // dense gaps: 16 and 17 records of an object through the gap behind it, every first granule
    for (uint32_t gran = 0; gran < 8; ++gran)
        for (uint64_t gap : {0, 1, 15, 16, 17, 63, 64, 65, 200})
            for (uint64_t nb : {1, 16, 17, 64, 65, 129})
                for (int small_last = 0; small_last < 2; ++small_last) {
                    const uintptr_t base = (uintptr_t)0x7F3A00000000ull + 16;
                    Descs d;
                    uint64_t off = gran * kBlk;
                    d.push_back(s3dg_obj_desc{off, 4097, 1, 1, 0, 1});
                    off += 2 * kBlk + gap * kBlk;
                    d.push_back(s3dg_obj_desc{off, nb * kBlk - 5, 2, 2, 1, 2});
                    off += (nb + gap) * kBlk;
                    d.push_back(s3dg_obj_desc{off, small_last ? 1 : 129 * kBlk, 3, 1, 0, 1});
                    const std::string plan = check_sub(d, base, BatchKnobs{0, true, 0}, gran == 0);
                    CHECK(plan == "dense", "a forced dense layout ran as %s", plan.c_str());
                    (void)check_sub(d, base, BatchKnobs{0, false, 16}, false);
                }
    // one object, and uniform runs
    for (uint64_t size : {1, 16, 4096, 4097, 129 * 4096})
        for (uint64_t off : {0, 4080, 5 * 4096, 7 * 4096 + 4080}) {
            const uintptr_t base = (uintptr_t)0x7F3A00000000ull + 3 * kBlk;
            for (uint32_t sh = 0; sh <= kTileShiftMax; ++sh)
                (void)check_sub({s3dg_obj_desc{off, size, 5, 1, 0, 1}}, base, BatchKnobs{sh, false, 0}, true);
            if (off % kBlk == 0) CHECK(check_sub({s3dg_obj_desc{off, size, 5, 1, 0, 1}}, base, BatchKnobs{0, true, 0}, false) == "dense", "n = 1 dense");
            for (uint64_t m : {2, 3, 9}) {
                const uint64_t stride = (size + 15) / 16 * 16;
                for (uint64_t st : {stride, stride + 16, (stride / 32768 + 1) * 32768}) {
                    Descs d;
                    const uint64_t e0 = ~0ull - (1ull << 32) + 6;   // the step wraps 2^64
                    for (uint64_t j = 0; j < m; ++j) d.push_back(s3dg_obj_desc{off + j * st, size, e0 + (j << 32), 2, 1, 3});
                    CHECK(check_sub(d, base, BatchKnobs{0, false, 16}, true) == "uniform", "a stream of %" PRIu64, m);
                    d[m - 1].entropy ^= 1;
                    CHECK(check_sub(d, base, BatchKnobs{0, false, 16}, true) != "uniform", "a broken run ran as a stream");
                }
            }
        }
}

// ---- the prefix parameters ---------------------------------------------------------

// round(nb / d), half away from zero, at least 1: in integers (s3dg_unique_blocks)
static uint64_t unique_ref(uint64_t nb, uint64_t dedup) {
    const uint64_t d = dedup == 0 ? 1 : dedup;
    if (d <= 1) return nb;
    const unsigned __int128 r = ((unsigned __int128)2 * nb + d) / ((unsigned __int128)2 * d);
    return r < 1 ? 1 : (uint64_t)r;
}

static void check_prefix(uint64_t nb, uint64_t dedup, uint32_t f_num, uint32_t f_den) {
    const PrefixParams pp = prefix_params(nb, dedup, f_num, f_den);
    const uint64_t U = unique_ref(nb, dedup);
    CHECK(unique_blocks(nb, dedup) == U, "unique_blocks(%" PRIu64 ", %" PRIu64 ")", nb, dedup);
    CHECK(pp.unique == (U == nb ? 0xFFFFFFFFu : (uint32_t)U), "unique(%" PRIu64 ", %" PRIu64 ")", nb, dedup);
    CHECK((uint64_t)pp.floor_len * f_den + pp.rem == 4096ull * f_num && pp.rem < f_den && pp.f_den == f_den,
          "prefix length %u / %u", f_num, f_den);
    const uint32_t du = pp.unique == 0xFFFFFFFFu ? 1u : pp.unique;
    for (uint32_t d : {du, f_den})
        for (uint64_t i : {(uint64_t)0, (uint64_t)d - 1, (uint64_t)d, (uint64_t)0x7FFFFFFF, (uint64_t)0xFFFFFFFF}) {
            const uint64_t M = d == du ? pp.m_unique : pp.m_fden;
            CHECK(fastmod((uint32_t)i, M, d) == (uint32_t)i % d, "fastmod(%" PRIu64 ", %u)", i, d);
        }
    CHECK(pp.m_unique == fastmod_magic(du) && pp.m_fden == fastmod_magic(f_den), "magic");
    ++n_prefix;
}

static void sweep_prefix() {
    std::vector<uint64_t> nbs;
    for (uint64_t nb = 1; nb <= 4097; ++nb) nbs.push_back(nb);
    for (uint32_t k = 13; k <= 31; ++k)
        for (int dlt : {-1, 1}) nbs.push_back((1ull << k) + dlt);
    const uint32_t ratios[][2] = {{0, 1},         {1, 2},         {2, 3},         {65534, 65535},        {65535, 65536},
                                  {65536, 65537}, {1, 65536},     {3, 65537},     {0xFFFFFFFEu, 0xFFFFFFFFu}, {1, 0xFFFFFFFFu},
                                  {99999, 100000}};
    size_t r = 0;
    for (uint64_t nb : nbs) {
        std::vector<uint64_t> dedups = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 100, nb, nb + 1, 1ull << 40};
        if (nb > 1) dedups.push_back(nb - 1);
        for (uint64_t dd : dedups) {
            const auto &q = ratios[r++ % (sizeof ratios / sizeof ratios[0])];
            check_prefix(nb, dd, q[0], q[1]);
        }
    }
    for (const auto &q : ratios)
        for (uint64_t nb : {1, 7, 4097}) check_prefix(nb, 3, q[0], q[1]);
}

// ---- the named lists (tests/batch_record_cases.py) -----------------------------------

static int run_cases() {
    char name[128];
    unsigned long long base, n;
    unsigned tile, split;
    while (scanf(" list %127s %llu %u %u %llu", name, &base, &tile, &split, &n) == 5) {
        Descs d(n);
        for (auto &o : d) {
            unsigned long long off, size, ent, dd;
            unsigned fn, fd;
            if (scanf("%llu %llu %llu %llu %u %u", &off, &size, &ent, &dd, &fn, &fd) != 6) return 2;
            o = s3dg_obj_desc{off, size, ent, dd, fn, fd};
        }
        uint32_t sh = 0;
        while ((1u << sh) < tile) ++sh;
        const BatchKnobs K{tile > 1 ? sh : 0, tile == 1, split};
        memset(recs16, 0, sizeof recs16);
        memset(recs17, 0, sizeof recs17);
        memset(wave2, 0, sizeof wave2);
        printf("plan %s", name);
        uint64_t sub = kBatchSubFirst;   // the call's cuts (s3dg_fill_controlled_batch)
        for (uint64_t k0 = 0, k1; k0 < n; k0 = k1) {
            k1 = n - k0 < sub ? n : k0 + sub;
            sub = sub * 2 < kBatchSubMax ? sub * 2 : kBatchSubMax;
            const Descs part(d.begin() + k0, d.begin() + k1);
            printf(" %s", check_sub(part, (uintptr_t)base, K, n <= 64).c_str());
        }
        uint64_t r16 = 0, r17 = 0, w2 = 0;
        for (uint32_t s = 0; s <= kTileShiftMax; ++s) r16 += recs16[s], r17 += recs17[s], w2 += wave2[s];
        printf(" | recs16=%" PRIu64 " recs17=%" PRIu64 " over64=%" PRIu64 "\n", r16, r17, w2);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "cases")) return run_cases();
    sweep_sets();
    sweep_prefix();
    printf("subs %" PRIu64 "\nuniform %" PRIu64 "\ndense %" PRIu64 "\ntwo_class %" PRIu64 "\nmerges %" PRIu64
           "\nprefix %" PRIu64 "\n",
           n_sub, n_uniform, n_dense, n_two, n_merge, n_prefix);
    for (uint32_t sh = 0; sh <= kTileShiftMax; ++sh)
        printf("shift %u recs16 %" PRIu64 " recs17 %" PRIu64 " over64 %" PRIu64 " live %" PRIu64 " off_mod8 %" PRIu64 "\n", sh,
               recs16[sh], recs17[sh], wave2[sh], live_slots[sh], xcd8_miss[sh]);
    return 0;
}
