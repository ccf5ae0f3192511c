// span_batch_plan_sweep.cpp — s3dg_span_batch_plan.h on its own (g++, no HIP):
// over a sweep of batches, block sizes, chunk minimums and tile sizes the
// prefixes cover every granule, block and slot exactly once, empty spans take
// nothing, a sub-launch never splits a tile, every refusal names the first
// offender, and the sums stay below 2^64 at the size limits.  The program
// asserts all of it and prints what tests/test_measure_batch_cpu.py compares
// with the C calls' texts.
#include <assert.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "s3dg_span_batch_plan.h"

using namespace s3dg;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static const uint64_t kSizes[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289,
                                  20485, 32768, 65535, 65536, 65537, 69631, 69632, 69633, 262143, 262144, 262145,
                                  3 * 69632 + 5, 1 << 20};
static const uint64_t kSrc = 0x7000000000ull;
static uint64_t plans = 0;

static void check_batch(const std::vector<s3dg_span> &v, uint64_t bb, uint64_t minb) {
    SpanBatchCounts C;
    std::string why;
    const bool ok = span_batch_check(kSrc, v.data(), v.size(), bb, minb, &C, &why);
    assert(ok && why.empty());
    uint64_t live = 0, bytes = 0, gr = 0, bl = 0, sl = 0;
    for (const s3dg_span &p : v) {
        if (!p.size) continue;
        ++live;
        bytes += p.size;
        gr += (p.size + 4095) / 4096;
        bl += bb ? (p.size + bb - 1) / bb : 0;
        sl += minb ? (p.size + minb - 1) / minb + 1 : 0;
    }
    assert(C.live == live && C.bytes == bytes && C.granules == gr && C.blocks == bl && C.slots == sl);
    if (!live) return;
    for (uint32_t knob = 0; knob <= kTileShiftMax; ++knob) {
        const uint32_t tsh = span_batch_tile_shift(C, knob);
        assert(tsh >= kTileShiftMin && tsh <= kTileShiftMax && (knob == 0 ? tsh >= kTileShiftAutoMin : tsh == knob));
        const uint64_t nt = C.ntiles[tsh];
        std::vector<uint8_t> tab(span_batch_table_bytes(live, nt), 0xEE);
        assert(span_batch_tile_offset(live) % 256 == 0 && span_batch_tile_offset(live) >= live * sizeof(SpanEnt));
        SpanEnt *e = (SpanEnt *)tab.data();
        SpanTile *t = (SpanTile *)(tab.data() + span_batch_tile_offset(live));
        span_batch_build(v.data(), v.size(), bb, minb, tsh, e, t);
        // entries: the non-empty spans in order, prefixes without gap or overlap
        uint64_t j = 0, g0 = 0, b0 = 0, s0 = 0;
        for (const s3dg_span &p : v) {
            if (!p.size) continue;
            assert(e[j].off == p.off && e[j].size == p.size && e[j].g0 == g0 && e[j].b0 == b0 && e[j].s0 == s0);
            g0 += span_obj_granules(p.size);
            b0 += span_obj_blocks(p.size, bb);
            s0 += span_obj_slots(p.size, minb);
            ++j;
        }
        assert(j == live && g0 == gr && b0 == bl && s0 == sl);
        // tiles through the sub-launches: every granule once, with its bytes
        std::vector<uint8_t> seen(gr, 0);
        const uint64_t subs = span_batch_sub_launches(nt, tsh);
        uint64_t tiles_seen = 0;
        for (uint64_t i = 0; i < subs; ++i) {
            uint64_t t0, n;
            span_batch_sub_launch(nt, tsh, i, &t0, &n);
            assert(t0 == tiles_seen && n > 0 && (n << tsh) <= kSpanBatchMaxGrid);
            tiles_seen += n;
            for (uint64_t w = 0; w < (n << tsh); ++w) {
                const SpanTile &T = t[t0 + (w >> tsh)];
                const uint64_t k = w & ((1ull << tsh) - 1), o = k * 4096;
                const SpanEnt &E = e[T.obj];
                assert(T.obj < live && T.left > 0 && T.first % (1u << tsh) == 0);
                assert(T.off == E.off + (uint64_t)T.first * 4096 && T.left == E.size - (uint64_t)T.first * 4096);
                assert(T.rec == E.g0 + T.first);
                if (o >= T.left) continue;   // a dead slot
                assert(T.off + o >= E.off && T.off + o < E.off + E.size);
                assert(T.rec + k < gr && !seen[T.rec + k]);
                seen[T.rec + k] = 1;
            }
        }
        assert(tiles_seen == nt);
        for (uint64_t g = 0; g < gr; ++g) assert(seen[g]);
        ++plans;
    }
    // the search: every block finds its entry
    SpanEnt *e = nullptr;
    std::vector<SpanEnt> ents(live);
    e = ents.data();
    span_batch_build(v.data(), v.size(), bb, minb, 3, e, nullptr);
    for (uint64_t j = 0; j < live; ++j) {
        const uint64_t nb = span_obj_blocks(e[j].size, bb);
        const uint64_t bs[] = {0, nb / 2, nb ? nb - 1 : 0};
        for (int q = 0; q < 3 && nb; ++q) assert(span_batch_find(e, live, e[j].b0 + bs[q]) == j);
    }
}

static void refusal(const char *name, uint64_t src, const s3dg_span *s, uint64_t n, uint64_t bb, uint64_t minb) {
    SpanBatchCounts C;
    std::string why;
    const bool ok = span_batch_check(src, s, n, bb, minb, &C, &why);
    assert(!ok && !why.empty());
    printf("%s|%s\n", name, why.c_str());
}

int main() {
    static_assert(sizeof(SpanEnt) == 40 && sizeof(SpanTile) == 32 && sizeof(s3dg_span) == 16, "table layout");
    // the sweep: random batches of the listed sizes, empties anywhere, any order, repeats and overlaps
    const uint64_t bbs[] = {4096, 12288, 65536, 69632, 0}, mins[] = {0, 32, 2048};
    for (int round = 0; round < 60; ++round) {
        std::vector<s3dg_span> v;
        const uint64_t n = 1 + rnd() % 40;
        for (uint64_t k = 0; k < n; ++k) {
            const uint64_t size = kSizes[rnd() % (sizeof kSizes / sizeof kSizes[0])];
            v.push_back(s3dg_span{(rnd() % (1ull << 33)) * 16, size});
        }
        if (round % 5 == 0) v.push_back(v[0]);                              // a repeat
        if (round % 7 == 0) v.push_back(s3dg_span{v[0].off + 16, v[0].size});   // an overlap
        for (uint64_t bb : bbs)
            for (uint64_t minb : mins) check_batch(v, bb, minb);
    }
    // 70 000 small spans; one span above a sub-launch
    {
        std::vector<s3dg_span> v;
        for (uint64_t k = 0; k < 70000; ++k) v.push_back(s3dg_span{k * 112, 100});
        check_batch(v, 4096, 32);
        v.assign(1, s3dg_span{0, (kSpanBatchMaxGrid + 3) * 4096 + 1});
        check_batch(v, 65536, 2048);
    }
    // empties take nothing, whatever they say
    {
        const s3dg_span e[] = {{7, 0}, {UINT64_MAX, 0}, {1, 0}};
        SpanBatchCounts C;
        std::string why;
        assert(span_batch_check(kSrc, e, 3, 4096, 32, &C, &why));
        assert(!C.live && !C.bytes && !C.granules && !C.blocks && !C.slots);
        assert(span_batch_check(0, nullptr, 0, 4096, 32, &C, &why) && !C.live);
        assert(span_batch_check(0, e, 3, 4096, 32, &C, &why) && !C.live);   // nothing would be read
        const s3dg_span m[] = {{7, 0}, {32, 5}, {3, 0}};
        assert(span_batch_check(kSrc, m, 3, 4096, 32, &C, &why) && C.live == 1 && C.bytes == 5 && C.slots == 2);
    }
    // the size limits: the largest object, and as many of them as one add takes
    {
        const s3dg_span big{0, kSpanBatchMaxObj};
        SpanBatchCounts C;
        std::string why;
        assert(span_batch_check(kSrc, &big, 1, 4096, 0, &C, &why));
        assert(C.granules == 1ull << 31 && C.blocks == 1ull << 31 && C.bytes == kSpanBatchMaxObj);
        std::vector<s3dg_span> v(513, big);
        assert(span_batch_check(kSrc, v.data(), 512, 4096, 0, &C, &why));
        assert(C.granules == kSpanBatchMaxGranules && C.bytes == 1ull << 52 && (C.ntiles[1] << 1) == C.granules);
        assert(!span_batch_check(kSrc, v.data(), 513, 4096, 0, &C, &why));
        assert(why == "span 512: more than 2^40 granules in one add");
        // chunk slots: 2^31 - 1 exactly fits, one more does not
        const s3dg_span s1{0, 32ull * (kSpanBatchMaxSlots - 1)}, s2[] = {{0, 32ull * (kSpanBatchMaxSlots - 2)}, {0, 1}};
        assert(span_batch_check(kSrc, &s1, 1, 0, 32, &C, &why) && C.slots == kSpanBatchMaxSlots);
        assert(!span_batch_check(kSrc, s2, 2, 0, 32, &C, &why));
        assert(why == "span 1: more than 2^31 - 1 chunk slots in one add");
    }
    // each refusal names the first offender
    const s3dg_span good[] = {{0, 100}, {128, 50}};
    const s3dg_span odd[] = {{0, 100}, {8, 0}, {24, 5}, {8, 5}};
    const s3dg_span large[] = {{3, 0}, {16, kSpanBatchMaxObj + 1}, {8, 1}};
    const s3dg_span wrap[] = {{0, 16}, {UINT64_MAX - 15, 32}};
    refusal("null_spans", kSrc, nullptr, 2, 4096, 0);
    refusal("null_src", 0, good, 2, 4096, 0);
    refusal("odd_src", kSrc + 8, good, 2, 4096, 0);
    refusal("odd_off", kSrc, odd, 4, 4096, 0);
    refusal("large", kSrc, large, 3, 4096, 0);
    refusal("wrap", kSrc, wrap, 2, 4096, 0);
    printf("plans|%llu\n", (unsigned long long)plans);
    return 0;
}
