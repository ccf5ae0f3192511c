// Stand-alone sweep of s3dg_dgen_batch_plan.h (g++ alone, no HIP): over sizes
// around every class edge and block edge, dedups, ratios and list shapes, for
// the fill's and the verify's lanes at every knob, it asserts that
//   * every byte of every non-empty object is covered by exactly one lane
//     region of exactly one launch, and no region passes its chunk's end;
//   * verify regions are whole granules (all but a chunk's last, which ends
//     with the chunk);
//   * a record's seed is entropy ^ ((i % U) * phi), its zero prefix
//     floor(len * f_num / f_den), its offset dst_off + i MiB;
//   * a record lies in its class's launch and is no longer than the ceiling;
//   * each refusal is found at the first offending index, with its text.
// Prints "plans N" and one line per refusal; exits non-zero on the first miss.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "s3dg_dgen_batch_plan.h"

using namespace s3dg;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static const uint64_t MiB = 1ull << 20;

// round(nb / d), half away from zero, at least 1: in integers
static uint64_t unique_ref(uint64_t nb, uint64_t d) {
    if (d <= 1) return nb;
    const uint64_t r = (2 * nb + d) / (2 * d);
    return r < 1 ? 1 : r;
}

static uint64_t plans = 0;

static void check_plan(const std::vector<s3dg_obj_desc> &d, uint32_t cus, uint64_t knob, uint32_t draws, bool verify) {
    const uint64_t n = d.size();
    const DgenBatchCheck C = dgen_batch_check(d.data(), n);
    CHECK(!C.msg && C.bad == UINT64_MAX);
    uint64_t live = 0, chunks = 0;
    for (const auto &o : d) {
        live += o.size != 0;
        chunks += (o.size + MiB - 1) / MiB;
    }
    CHECK(C.live == live && C.chunks == chunks);
    const DgenBatchPlan P = dgen_batch_plan(C, cus, knob, draws, verify);
    CHECK(!P.msg && P.nlaunch <= kDgbClasses && (P.nlaunch > 0) == (live > 0));
    std::vector<DgenChunkRec> recs(chunks + 1);
    const DgenChunkRec guard{~0ull, ~0ull, ~0u, ~0u, ~0u, ~0u};
    recs[chunks] = guard;
    dgen_batch_records(d.data(), n, P, recs.data());
    CHECK(recs[chunks].off == guard.off && recs[chunks].len == guard.len);   // nothing past the table
    // the launches tile the table, the full chunks first, then the classes downwards
    uint64_t at = 0;
    std::map<std::pair<uint32_t, uint32_t>, uint64_t> seen;   // (obj, blk) -> bytes covered
    for (uint32_t q = 0; q < P.nlaunch; ++q) {
        const DgenLaunch &L = P.launch[q];
        CHECK(L.rec0 == at && L.nrec > 0 && L.cls < kDgbClasses);
        if (q) CHECK(L.cls < P.launch[q - 1].cls);
        at += L.nrec;
        const uint64_t ceil = dgen_class_ceiling(L.cls);
        const uint32_t lpc = L.lanes.lpc;
        const uint64_t span = L.lanes.span;
        CHECK(lpc >= 1 && lpc <= 1024 && (lpc & (lpc - 1)) == 0 && span > 0 && span <= 0xFFFFFFFFull);
        CHECK((uint64_t)lpc * span * 8 >= ceil);
        if (verify) CHECK(span % 512 == 0);
        else CHECK(span % draws == 0);
        if (knob && !verify && ceil / 8 / 2 >= knob) CHECK(span >= knob || lpc == 1024);
        bool zeros = false;
        for (uint64_t r = L.rec0; r < L.rec0 + L.nrec; ++r) {
            const DgenChunkRec &R = recs[r];
            CHECK(R.obj < n);
            const s3dg_obj_desc &o = d[R.obj];
            const uint64_t nb = (o.size + MiB - 1) / MiB;
            CHECK(R.blk < nb);
            const uint64_t len = R.blk + 1 < nb ? MiB : o.size - (nb - 1) * MiB;
            CHECK(R.len == len && R.len >= 1 && R.len <= ceil && dgen_chunk_class(len) == L.cls);
            if (L.cls == kDgbFull) CHECK(len == MiB);
            else CHECK(len < MiB && (L.cls == 0 || len > ceil / 2));
            CHECK(R.off == o.dst_off + (uint64_t)R.blk * MiB);
            CHECK(R.seed == (o.entropy ^ ((R.blk % unique_ref(nb, o.dedup)) * 0x9E3779B97F4A7C15ull)));
            CHECK(R.zlen == len * o.f_num / o.f_den && R.zlen < len + (len == 0));
            zeros |= R.zlen != 0;
            if (r > L.rec0) {   // the descriptors' order within a class
                const DgenChunkRec &Q = recs[r - 1];
                CHECK(Q.obj < R.obj || (Q.obj == R.obj && Q.blk < R.blk));
            }
            // the lanes' regions tile [0, len)
            uint64_t pos = 0;
            for (uint32_t sub = 0; sub < lpc; ++sub) {
                const DgenRegion G = dgen_lane_region(len, span, sub);
                CHECK(G.rb == (uint64_t)sub * span * 8);
                if (G.rlen == 0) {
                    CHECK(G.rb >= len);
                    continue;
                }
                CHECK(G.rb == pos && G.rb + G.rlen <= len);
                if (verify) CHECK(G.rb % 4096 == 0 && (G.rlen % 4096 == 0 || G.rb + G.rlen == len));
                pos += G.rlen;
            }
            CHECK(pos == len);
            CHECK(seen.emplace(std::make_pair(R.obj, R.blk), len).second);   // once, in one launch
        }
        CHECK(zeros == L.zeros);
    }
    CHECK(at == chunks && seen.size() == chunks);
    for (uint64_t k = 0; k < n; ++k) {   // every block of every object, summing to its size
        uint64_t sum = 0;
        const uint64_t nb = (d[k].size + MiB - 1) / MiB;
        for (uint64_t i = 0; i < nb; ++i) {
            auto it = seen.find(std::make_pair((uint32_t)k, (uint32_t)i));
            CHECK(it != seen.end());
            sum += it->second;
        }
        CHECK(sum == d[k].size);
    }
    ++plans;
}

static void check_all(const std::vector<s3dg_obj_desc> &d) {
    static const uint64_t knobs[] = {0, 512, 2048, 4096, 131072, 100, 1ull << 40};
    for (uint32_t cus : {256u, 8u})
        for (uint64_t knob : knobs) {
            for (uint32_t draws : {16u, 32u, 64u}) check_plan(d, cus, knob, draws, false);
            check_plan(d, cus, knob, 64, true);
        }
}

static void refusal(const char *what, const std::vector<s3dg_obj_desc> &d, uint64_t bad, const char *msg) {
    const DgenBatchCheck C = dgen_batch_check(d.data(), d.size());
    CHECK(C.msg && C.bad == bad && C.live == 0 && C.chunks == 0);
    const std::string m = dgen_batch_message(C.bad, C.msg);
    CHECK(m == "object " + std::to_string(bad) + ": " + msg);
    printf("%s|%s\n", what, m.c_str());
}

int main() {
    std::vector<uint64_t> sizes = {0, 1, 4, 5, 7, 8, 9, 15, 16, 17, 127, 128, 129, 2064};
    for (uint32_t sh = 12; sh <= 20; ++sh)
        for (int64_t dlt : {-17, -1, 0, 1, 16})
            sizes.push_back(((uint64_t)1 << sh) + (uint64_t)dlt);
    for (uint64_t b : {2, 3, 5})
        for (int64_t dlt : {-1, 0, 1, 3, 4097})
            sizes.push_back(b * MiB + (uint64_t)dlt);
    const uint32_t ratios[][2] = {{0, 1}, {1, 2}, {2, 3}, {1, 3}, {0xFFFFFFFEu, 0xFFFFFFFFu}};
    uint64_t off = 0, seed = 0x1234567;
    // one object per list; then lists of all sizes in order, reversed, interleaved with empties, doubled
    for (uint64_t size : sizes)
        for (uint64_t dd : {1, 2, 3})
            for (const auto &r : ratios) check_all({s3dg_obj_desc{48, size, ++seed, dd, r[0], r[1]}});
    for (uint64_t dd : {0, 1, 2, 3, 7})
        for (const auto &r : ratios) {
            std::vector<s3dg_obj_desc> d;
            off = 16;
            for (uint64_t size : sizes) {
                d.push_back(s3dg_obj_desc{off, size, ++seed, dd, r[0], r[1]});
                off += (size + 15) / 16 * 16 + 16 * (1 + size % 7);
            }
            check_all(d);
            std::vector<s3dg_obj_desc> rev(d.rbegin(), d.rend());
            check_all(rev);
            std::vector<s3dg_obj_desc> holes;
            holes.push_back(s3dg_obj_desc{8, 0, 0, 0, 5, 0});   // an empty object may say anything
            for (size_t k = 0; k < d.size(); ++k) {
                holes.push_back(d[k]);
                if (k % 5 == 2) holes.push_back(s3dg_obj_desc{3, 0, 1, 1, 9, 9});
                if (k % 11 == 3) holes.push_back(d[k]);        // a repeat
            }
            holes.push_back(s3dg_obj_desc{0, 0, 0, 1, 0, 1});
            check_all(holes);
        }
    // mixed parameters per object, many small objects, and nothing at all
    {
        std::vector<s3dg_obj_desc> d;
        off = 0;
        for (uint64_t k = 0; k < 700; ++k) {
            const uint64_t size = k % 2 ? 4096 + 16 : 2064;
            d.push_back(s3dg_obj_desc{off, size, k * 77, 1 + k % 3, ratios[k % 4][0], ratios[k % 4][1]});
            off += 4128;
        }
        check_all(d);
        check_all({});
        check_all({s3dg_obj_desc{0, 0, 0, 1, 0, 1}, s3dg_obj_desc{0, 0, 0, 1, 0, 1}});
    }
    printf("plans|%llu\n", (unsigned long long)plans);

    // the calls' pointer arguments, in the order they are refused
    const s3dg_obj_desc one{0, 16, 1, 1, 0, 1};
    CHECK(dgen_batch_args((void *)16, &one, 1, false, nullptr) == nullptr);
    CHECK(dgen_batch_args(nullptr, nullptr, 0, false, nullptr) == nullptr);   // n == 0: nothing to look at
    CHECK(dgen_batch_args(nullptr, nullptr, 0, true, &one) == nullptr);
    printf("null_out|%s\n", dgen_batch_args((void *)16, &one, 1, true, nullptr));
    printf("null_out_empty|%s\n", dgen_batch_args(nullptr, nullptr, 0, true, nullptr));
    printf("null_descs|%s\n", dgen_batch_args((void *)16, nullptr, 1, false, nullptr));
    printf("null_dst|%s\n", dgen_batch_args(nullptr, &one, 1, false, nullptr));
    printf("odd_dst|%s\n", dgen_batch_args((void *)24, &one, 1, false, nullptr));
    printf("null_src|%s\n", dgen_batch_args(nullptr, &one, 1, true, &one));
    printf("odd_src|%s\n", dgen_batch_args((void *)8, &one, 1, true, &one));
    // the descriptors: the first offending one names the refusal, wherever it stands
    const s3dg_obj_desc good{32, 5 * MiB + 3, 9, 2, 1, 2};
    const s3dg_obj_desc odd{40, 100, 1, 1, 0, 1}, ratio{0, 100, 1, 1, 3, 3}, noden{0, 100, 1, 1, 0, 0};
    const s3dg_obj_desc large{0, ((1ull << 32) + 1) * MiB, 1, 1, 0, 1}, fits{0, ((1ull << 32) - 1) * MiB, 1, 1, 0, 1};
    CHECK(!dgen_batch_check(&fits, 1).msg && dgen_batch_check(&fits, 1).chunks == 0xFFFFFFFFull);
    const s3dg_obj_desc huge{0, ~0ull, 1, 1, 0, 1};
    CHECK(dgen_batch_check(&huge, 1).msg);
    for (uint64_t at = 0; at < 4; ++at) {
        std::vector<s3dg_obj_desc> d(4, good);
        d[at] = odd;
        CHECK(dgen_batch_check(d.data(), 4).bad == at);
        d[at] = ratio;
        CHECK(dgen_batch_check(d.data(), 4).bad == at);
        d[at] = large;
        CHECK(dgen_batch_check(d.data(), 4).bad == at);
    }
    refusal("odd_off", {good, good, odd, ratio}, 2, "dst_off must be a multiple of 16");
    refusal("ratio", {good, ratio, odd, good}, 1, "need f_num < f_den");
    refusal("f_den", {good, good, good, noden}, 3, "need f_num < f_den");
    refusal("large", {large, odd}, 0, "object larger than 2^32 blocks");
    refusal("far", [&] {
        std::vector<s3dg_obj_desc> d(70000, good);
        d.push_back(ratio);
        return d;
    }(), 70000, "need f_num < f_den");
    // a launch beyond the grid's reach is refused by the plan, not launched
    {
        DgenBatchCheck C;
        C.live = 1;
        C.count[0] = C.chunks = (1ull << 31) + 1;
        CHECK(dgen_batch_plan(C, 256, 0, 64, false).msg);
        C.count[0] = C.chunks = 1ull << 31;
        CHECK(!dgen_batch_plan(C, 256, 0, 64, false).msg && !dgen_batch_plan(C, 256, 0, 64, true).msg);
        C.count[0] = 0;
        C.count[kDgbFull] = C.chunks = (1ull << 31) / 64 + 1;
        CHECK(dgen_batch_plan(C, 256, 0, 64, false).msg);   // 64 lanes per full chunk
        printf("grid|%s\n", dgen_batch_plan(C, 256, 0, 64, false).msg);
    }
    return 0;
}
