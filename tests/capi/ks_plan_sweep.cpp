// Properties of the uniform keystream launches' plan (csrc/s3dg_ks_plan.h)
// over a sweep of chunk sizes, stage widths, knobs, chunk counts, CU counts
// and zero prefixes.  g++ alone, plain and sanitized
// (tests/test_ks_plan_cpu.py); prints the number of plans it checked.
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "s3dg_ks_plan.h"

using namespace s3dg;
typedef unsigned long long ull;

#define CHECK(c, ...)                                          \
    do {                                                       \
        if (!(c)) {                                            \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c); \
            fprintf(stderr, __VA_ARGS__);                      \
            fprintf(stderr, "\n");                             \
            exit(1);                                           \
        }                                                      \
    } while (0)

static const uint64_t MIB = 1ull << 20;
static ull plans = 0;

// The regions of a chunk of clen bytes tile [8 z0, clen) exactly once, in lane
// order, and none passes clen.
static void check_regions(uint64_t clen, uint64_t z0, const KsLanes &L) {
    uint64_t at = 8 * z0;
    for (uint32_t sub = 0; sub < L.lpc; ++sub) {
        const KsRegion R = ks_lane_region(clen, z0, (uint32_t)L.span, sub);
        CHECK(R.rb == 8 * (z0 + sub * L.span), "rb");
        CHECK(R.rlen <= L.span * 8, "rlen");
        if (R.rlen) {
            CHECK(R.rb == at && R.rb + R.rlen <= clen, "clen %llu sub %u", (ull)clen, sub);
            at += R.rlen;
        } else {
            CHECK(R.rb >= clen || clen <= 8 * z0, "an empty lane below the end");
        }
    }
    CHECK(at == (clen > 8 * z0 ? clen : 8 * z0), "clen %llu z0 %llu lpc %u span %llu: covered to %llu", (ull)clen,
          (ull)z0, L.lpc, (ull)L.span, (ull)at);
}

static void check_lanes(int mode, uint64_t cb, uint64_t nc, bool zp, uint64_t z0, uint64_t knob, uint64_t D,
                        uint64_t cus) {
    const uint64_t md = knob ? knob : kDefaultKsMinDraws[mode];
    const KsLanes L = ks_lanes(mode, cb, nc, zp, z0, md, D, cus);
    const uint64_t nd = cb / 8 - z0;
    ++plans;
    CHECK(L.lpc >= 1 && L.lpc <= 1024 && (L.lpc & (L.lpc - 1)) == 0, "lpc %u", L.lpc);
    CHECK(L.span % D == 0 && L.lpc * L.span >= nd, "span %llu", (ull)L.span);
    CHECK(L.span < (nd + L.lpc - 1) / L.lpc + D, "span rounded up by less than a stage");
    CHECK(L.ok == (L.span <= 0xFFFFFFFFull), "ok");
    if (!L.ok) return;
    // the rule, restated independently: the lanes the knob gives, then the tail rule, then the spread
    uint64_t m = md;
    if (mode == 1 && zp && md == 2048) m = 512;
    if (mode == 0 && md == 2048 && nd >= 64 * 4096 && nc * (nd / 4096) / 64 >= 4 * cus * 4) m = 4096;
    uint32_t want = 1;
    while (want < 1024 && nd / (2 * want) >= m) want *= 2;
    const bool forced = z0 && want < 64 && nd >= 64 * 256;
    if (forced) want = 64;
    while (want < 1024 && nc * want < cus * 256 && nd / (2 * want) >= 256) want *= 2;
    CHECK(L.lpc == want, "lpc %u, the rules give %u", L.lpc, want);
    if (z0 && nd >= 64 * 256) CHECK(L.lpc >= 64, "a tail of %llu draws in %u lanes", (ull)nd, L.lpc);
    if (z0 && nd < 64 * 256 && nd / 2 < m && nd / 2 < 256) CHECK(L.lpc == 1, "a short tail");
    // regions: the full chunk, ragged ends around every kind of boundary
    const uint64_t lens[] = {cb, cb - 1, cb - 7, cb / 2 + 3, 8 * z0 + 1, 8 * z0, 1, L.span * 8 * (L.lpc / 2) + 8 * z0 + 5,
                             L.span * 8 * (L.lpc - 1) + 8 * z0, L.span * 8 * (L.lpc - 1) + 8 * z0 + 1};
    for (uint64_t len : lens)
        if (len >= 1 && len <= cb) check_regions(len, z0, L);
}

static void check_grid(uint64_t nc, uint32_t lpc) {
    for (int W : {1, 2, 4})
        for (int xcd : {1, 4, 16, 32, 64}) {
            const KsGrid G = ks_static_grid(nc, lpc, W, xcd);
            CHECK(G.wgs * W * 64 >= nc * lpc && (G.wgs - 1) * W * 64 < nc * lpc, "grid");
            CHECK(G.xg >= 1 && (G.xg & (G.xg - 1)) == 0, "xg");
            if (G.wgs > 5000) continue;
            // the remap is a permutation of [0, nwg) that keeps the partial last group in place
            std::vector<char> seen(G.nwg, 0);
            for (uint64_t b = 0; b < G.nwg; ++b) {
                const uint64_t r = ks_remap(G.xg, G.nwg, b);
                CHECK(r < G.nwg && !seen[r], "remap xg %u nwg %u b %llu -> %llu", G.xg, G.nwg, (ull)b, (ull)r);
                seen[r] = 1;
                if (b >= G.nwg / (8 * G.xg) * (8 * G.xg)) CHECK(r == b, "partial group");
                else CHECK(r / G.xg % 8 == b % 8 || G.xg == 1, "XCD b mod 8 takes run r / xg mod 8");
            }
            // the eight quotas sum to W * nwg; every (queue, q) below quota is a distinct (workgroup, wave)
            uint64_t sum = 0;
            std::vector<char> unit((size_t)G.nwg * W, 0);
            for (uint32_t v = 0; v < 8; ++v) {
                const uint64_t quota = ks_queue_quota(G.nwg, v, (uint32_t)W);
                sum += quota;
                for (uint64_t q = 0; q < quota; ++q) {
                    const uint64_t b = ks_queue_wg(q, v, (uint32_t)W);
                    const uint32_t w = ks_queue_wave(q, (uint32_t)W);
                    CHECK(b < G.nwg && b % 8 == v && w < (uint32_t)W && !unit[b * W + w], "queue %u unit %llu", v, (ull)q);
                    unit[b * W + w] = 1;
                }
            }
            CHECK(sum == (uint64_t)W * G.nwg, "quotas");
            ++plans;
        }
}

static void check_half_tail() {
    for (int64_t tail : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)3, (int64_t)32, (int64_t)1000})
        for (uint64_t res : {(uint64_t)0, (uint64_t)1, (uint64_t)8})
            for (uint64_t cus : {(uint64_t)1, (uint64_t)256, (uint64_t)304})
                for (uint32_t W : {1u, 2u, 4u})
                    for (uint32_t D : {16u, 32u, 64u})
                        for (uint64_t n_objs : {(uint64_t)1, (uint64_t)2})
                            for (uint64_t nc : {(uint64_t)1, (uint64_t)8, (uint64_t)24, (uint64_t)255, (uint64_t)256, (uint64_t)8000})
                                for (uint32_t lpc = 1; lpc <= 1024; lpc *= 2)
                                    for (uint32_t span : {256u, 352u, 510u, 512u, 544u, 1024u, 2048u}) {
                                        const uint64_t c0 = 3;
                                        const KsHalfTail H = ks_half_tail(tail, res, cus, W, D, n_objs, nc, c0, lpc, span);
                                        ++plans;
                                        const int64_t T = tail < 0 ? (int64_t)(res * cus * W * 64 / lpc / 2) : tail;
                                        const bool want = n_objs == 1 && T > 0 && W == 1 && lpc >= 64 && lpc <= 512 &&
                                                          span / 2 >= 256 && span / 2 % D == 0 && nc >= 8 * (uint64_t)T;
                                        CHECK(H.take == want, "take");
                                        if (!H.take) continue;
                                        // A and A2 together cover each chunk of the object once, A2 with lanes
                                        // half as long that cover the same draws
                                        CHECK(H.T == (uint64_t)T && H.nchunks1 + H.T == nc && H.cpo1 == H.nchunks1, "T");
                                        CHECK(H.chunk0_2 == c0 + H.nchunks1 && H.cpo2 == H.T, "chunk0");
                                        CHECK(H.doff == H.nchunks1 * MIB, "doff");
                                        CHECK(H.lpc2 == 2 * lpc && 2 * H.span2 == span && (uint64_t)H.lpc2 * H.span2 == (uint64_t)lpc * span,
                                              "lanes");
                                        CHECK(H.nchunks1 >= 7 * H.T, "the first set keeps 7/8");
                                    }
}

static void check_dgen_call() {
    // ratios n / (n + 1), and wide denominators from a ratio near 0 to one near 1
    std::vector<std::pair<uint32_t, uint32_t>> ratios;
    for (uint32_t k = 1; k <= 130; ++k) {
        ratios.push_back({k, k + 1});
        for (uint32_t den : {65535u, 1000003u, 0xFFFFFFFFu}) {
            ratios.push_back({den - k, den});                       // tails of a granule or two
            ratios.push_back({(uint32_t)((uint64_t)den * k / 131), den});
        }
    }
    for (auto &r : ratios) {
        const uint32_t n = r.first, den = r.second;
            if (n == 0 || n >= den) continue;
            for (uint64_t size : {MIB, 2 * MIB, 2 * MIB + 1, 5 * MIB + 4095, 70 * MIB, 70 * MIB + 9})
                for (uint64_t n_objs : {(uint64_t)1, (uint64_t)3})
                    for (uint64_t split : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)64}) {
                        const uint64_t nb = (size + MIB - 1) / MIB;
                        for (uint64_t lo : {(uint64_t)0, (uint64_t)1})
                            for (uint64_t hi : {nb, nb - 1}) {
                                if (lo >= hi) continue;
                                const KsDgenCall P = ks_dgen_call(size, n_objs, lo, hi, n, den, split);
                                ++plans;
                                const uint64_t zlen = MIB * (uint64_t)n / den;
                                CHECK(P.zw % 4096 == 0 && P.zw <= zlen && zlen - P.zw < 4096, "zw");
                                CHECK(!(P.cut_last && P.zsplit), "one decision");
                                const bool ragged = size % MIB && hi == nb;
                                if (P.zsplit) CHECK(!ragged && split && P.nchunks >= split && P.zw >= 32768 && P.z0 * 8 == P.zw, "zsplit");
                                else CHECK(P.z0 == 0, "z0");
                                if (P.cut_last) CHECK(ragged && hi - 1 > lo && (hi - 1 - lo) * n_objs >= split && split, "cut");
                                if (split && !ragged && P.zw >= 32768 && P.nchunks >= split) CHECK(P.zsplit, "a split missed");
                                if (P.cut_last) {   // both halves: the full blocks split, the last block does not
                                    const KsDgenCall F = ks_dgen_call(size, n_objs, lo, hi - 1, n, den, split);
                                    const KsDgenCall R = ks_dgen_call(size, n_objs, hi - 1, hi, n, den, split);
                                    CHECK(F.zsplit && !F.cut_last && !R.zsplit && !R.cut_last, "the halves");
                                    CHECK(F.nchunks + R.nchunks == P.nchunks, "chunks");
                                }
                                // the tail's lanes and regions at every stage width
                                if (P.zsplit)
                                    for (uint64_t D : {(uint64_t)16, (uint64_t)32, (uint64_t)64})
                                        for (uint64_t cus : {(uint64_t)1, (uint64_t)256, (uint64_t)304})
                                            check_lanes(1, MIB, P.nchunks, false, P.z0, 0, D, cus);
                            }
                    }
        }
}

static void check_persist() {
    for (uint64_t wgs = 0; wgs < 5000; wgs += 37)
        for (uint64_t wgs2 : {(uint64_t)0, (uint64_t)1, (uint64_t)64})
            for (int rounds : {-1, 0, 1, 3, 6})
                for (uint64_t res : {(uint64_t)0, (uint64_t)1, (uint64_t)3, (uint64_t)8})
                    for (uint64_t cus : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)8, (uint64_t)256, (uint64_t)304})
                        for (int W : {1, 2, 4}) {
                            const uint64_t g = ks_persistent_grid(wgs, wgs2, rounds, res, cus, W);
                            ++plans;
                            const uint64_t r = rounds < 0 ? (W == 1 ? 6 : 0) : (uint64_t)rounds;
                            const uint64_t cap = res * cus / 8 * 8;
                            CHECK(g == (r && cap >= 8 && wgs + wgs2 >= r * cap ? cap : 0), "persist");
                            CHECK(g % 8 == 0 && g <= res * cus, "one resident round, a multiple of 8");
                        }
}

static void check_fastmod() {
    const uint32_t Us[] = {1u, 2u, 3u, 5u, 65535u, 65537u, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t U : Us) {
        const uint64_t M = fastmod_magic(U);
        std::vector<uint32_t> as = {0u, U - 1, U, U + 1, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x80000000u, 0x7FFFFFFFu};
        for (uint64_t k = 1; k * U <= 0xFFFFFFFFull && k < 70000; k = k < 16 ? k + 1 : k * 3 + 1)
            for (int64_t d = -1; d <= 1; ++d) as.push_back((uint32_t)(k * U + d));
        const uint64_t top = 0xFFFFFFFFull / U * U;   // the largest multiple
        for (int64_t d = -1; d <= 1; ++d) as.push_back((uint32_t)(top + d));
        for (uint32_t a : as) {
            CHECK(fastmod(a, M, U) == a % U, "fastmod(%u, %u) = %u", a, U, fastmod(a, M, U));
            ++plans;
        }
    }
    CHECK(fastmod_magic(1) == 0, "magic(1) wraps to 0");
}

int main() {
    std::vector<uint64_t> chunks;
    for (uint64_t k = 1; k <= 40; ++k) chunks.push_back(128 * k);
    for (uint64_t p = 1ull << 12; p <= 1ull << 22; p <<= 1) {
        chunks.push_back(p - 128);
        chunks.push_back(p);
        chunks.push_back(p + 128);
    }
    for (uint64_t m : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)8, (uint64_t)16, (uint64_t)64}) chunks.push_back(m * MIB);
    chunks.push_back(65664);
    chunks.push_back(4202496);
    const uint64_t knobs[] = {0, 64, 256, 512, 2048, 4096, 131072};
    const uint64_t ncs[] = {1, 2, 3, 33, 64, 255, 700, 4096, 1ull << 20};
    for (uint64_t cb : chunks)
        for (uint64_t D : {(uint64_t)16, (uint64_t)32, (uint64_t)64})
            for (uint64_t knob : knobs)
                for (uint64_t nc : ncs)
                    for (uint64_t cus : {(uint64_t)1, (uint64_t)256, (uint64_t)304}) {
                        check_lanes(0, cb, nc, false, 0, knob, D, cus);
                        if (cb == MIB)
                            for (int zp = 0; zp < 2; ++zp) check_lanes(1, cb, nc, zp, 0, knob, D, cus);
                    }
    // z0 tails at every knob (the issue's ratios at the default knob: check_dgen_call)
    for (uint32_t n : {1u, 2u, 6u, 19u, 99u, 127u})
        for (uint64_t D : {(uint64_t)16, (uint64_t)32, (uint64_t)64})
            for (uint64_t knob : knobs)
                for (uint64_t nc : ncs)
                    for (uint64_t cus : {(uint64_t)1, (uint64_t)256, (uint64_t)304})
                        check_lanes(1, MIB, nc, false, (MIB * n / (n + 1) & ~4095ull) / 8, knob, D, cus);
    // every z0 a split can give: 512 k draws, from 8 granules to the whole block but one
    for (uint64_t k = 8; k < 256; ++k)
        for (uint64_t D : {(uint64_t)16, (uint64_t)32, (uint64_t)64})
            for (uint64_t nc : {(uint64_t)1, (uint64_t)2, (uint64_t)6, (uint64_t)64, (uint64_t)4096})
                for (uint64_t cus : {(uint64_t)1, (uint64_t)256, (uint64_t)304}) check_lanes(1, MIB, nc, false, 512 * k, 0, D, cus);
    // a span that does not fit 32 bits is refused, not truncated
    const KsLanes big = ks_lanes(0, 1ull << 46, 1, false, 0, 2048, 64, 256);
    CHECK(!big.ok && big.lpc == 1024 && big.span == (1ull << 33), "2^46-byte chunk");
    CHECK(ks_lanes(0, 1ull << 45, 1, false, 0, 2048, 64, 256).ok == false, "2^45: span 2^32");
    CHECK(ks_lanes(0, (1ull << 45) - 512 * 1024, 1, false, 0, 2048, 64, 256).ok, "span 2^32 - 64");
    CHECK(!ks_lanes(0, (1ull << 45) - 128 * 1024, 1, false, 0, 2048, 64, 256).ok, "2^32 - 16 rounds up to 2^32");
    for (uint64_t nc : ncs)
        for (uint32_t lpc = 1; lpc <= 1024; lpc *= 2) check_grid(nc, lpc);
    for (uint64_t nc : {(uint64_t)5, (uint64_t)7, (uint64_t)9, (uint64_t)15, (uint64_t)17, (uint64_t)129, (uint64_t)1001}) check_grid(nc, 64);
    const KsGrid huge = ks_static_grid(1ull << 40, 1024, 1, 16);
    CHECK(huge.wgs == 1ull << 44 && huge.nwg == 0x7FFFFFFFu, "the kernel's nwg is capped");
    check_half_tail();
    check_dgen_call();
    check_persist();
    check_fastmod();
    printf("plans|%llu\n", plans);
    return 0;
}
