// crc_batch_plan_sweep.cpp — s3dg_crc_batch_plan.h on its own (g++, no HIP):
// over a sweep of batches the regions tile every object exactly once and in
// order, only an object's last region has a tail, an object shorter than a row
// is one region of no rows, empty spans are squeezed out but keep their index,
// the region follows the call's whole rows between 32 and 256, and an object
// never has more than 4096 regions up to the largest size.  Then the algebra:
// for byte strings cut by the plan, the fold of the regions' raw CRCs (taken
// bytewise from a zero register) is the CRC-32 of the string.  The program
// asserts all of it and prints what tests/test_crc_batch_cpu.py compares with
// zlib.crc32 and s3dg_crc32_host.
#include <assert.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "s3dg_crc_batch_plan.h"

using namespace s3dg;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static const uint64_t kSrc = 0x7000000000ull;
static const uint64_t KiB = 1024, MiB = 1024 * KiB, GiB = 1024 * MiB;
static uint64_t plans = 0, folds = 0;

// bit by bit, from the definition: the judge of the fold
static uint32_t raw_bitwise(uint32_t reg, const uint8_t *p, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        reg ^= p[i];
        for (int b = 0; b < 8; ++b) reg = (reg & 1) ? (reg >> 1) ^ 0xEDB88320u : reg >> 1;
    }
    return reg;
}
static uint32_t crc32_bitwise(const uint8_t *p, uint64_t n) { return ~raw_bitwise(0xFFFFFFFFu, p, n); }

struct Plan {
    CrcBatchCounts C;
    std::vector<CrcBatchEnt> ents;
    std::vector<CrcBatchRec> recs;
};

static Plan plan_of(const std::vector<s3dg_span> &v) {
    SpanBatchCounts B;
    std::string why;
    const bool ok = span_batch_check(kSrc, v.data(), v.size(), 0, 0, &B, &why);
    assert(ok && why.empty());
    Plan P;
    P.C = crc_batch_count(v.data(), v.size());
    assert(P.C.live == B.live);
    assert(P.C.rows >= kCrcBatchMinRows && P.C.rows <= kCrcBatchMaxRows);
    assert(crc_batch_rec_offset(P.C.live) == P.C.live * 32 && crc_batch_raw_offset(P.C) % 256 == 0);
    assert(crc_batch_raw_offset(P.C) >= crc_batch_table_bytes(P.C));
    assert(crc_batch_device_bytes(P.C) == crc_batch_raw_offset(P.C) + 4 * P.C.regions);
    P.ents.assign(P.C.live + 1, CrcBatchEnt{0xEEEE, 0xEEEE, 0xEEEE, 0xEEEE, 0xEEEE});   // one past: never written
    P.recs.assign(P.C.regions + 1, CrcBatchRec{0xEEEE, 0xEEEE, 0xEEEE, 0xEEEE, 0xEEEE});
    crc_batch_build(v.data(), v.size(), P.C, P.ents.data(), P.recs.data());
    assert(P.ents[P.C.live].size == 0xEEEE && P.recs[P.C.regions].off == 0xEEEE);
    return P;
}

static void check_plan(const std::vector<s3dg_span> &v) {
    const Plan P = plan_of(v);
    uint64_t j = 0, r = 0, total_rows = 0;
    for (uint64_t k = 0; k < v.size(); ++k) {
        const s3dg_span p = v[k];
        if (!p.size) continue;   // squeezed out: the next entry names a later k
        const CrcBatchEnt &E = P.ents[j];
        assert(E.k == k && E.size == p.size && E.reg0 == r && E.nreg >= 1 && E.nreg <= kCrcBatchMaxRegions);
        // the object's region: the call's, doubled no further than the cap asks
        assert(E.rows >= P.C.rows && E.rows % P.C.rows == 0 && ((E.rows / P.C.rows) & (E.rows / P.C.rows - 1)) == 0);
        const uint64_t obj_rows = p.size / 1024;
        if (E.rows > P.C.rows) assert((obj_rows + E.rows / 2 - 1) / (E.rows / 2) > kCrcBatchMaxRegions);
        uint64_t at = p.off, rows = 0;
        for (uint32_t q = 0; q < E.nreg; ++q, ++r) {
            const CrcBatchRec &R = P.recs[r];
            const bool last = q + 1 == E.nreg;
            assert(R.ent == j && R.off == at && R.tail < 1024);
            if (!last) assert(R.rows == E.rows && R.tail == 0);
            else assert(R.rows <= E.rows && R.tail == p.size % 1024 && (R.rows > 0 || (E.nreg == 1 && p.size < 1024)));
            at += (uint64_t)R.rows * 1024 + R.tail;
            rows += R.rows;
        }
        assert(at == p.off + p.size && rows == obj_rows);   // tiled exactly once, in order
        if (p.size < 1024) assert(E.nreg == 1 && P.recs[E.reg0].rows == 0 && P.recs[E.reg0].tail == p.size);
        total_rows += obj_rows;
        ++j;
    }
    assert(j == P.C.live && r == P.C.regions && total_rows == P.C.total_rows);
    ++plans;
}

// The fold over a buffer cut by the plan against the definition.
static void check_fold(const std::vector<uint8_t> &buf, const std::vector<s3dg_span> &v) {
    const Plan P = plan_of(v);
    std::vector<uint32_t> raw(P.C.regions);
    for (uint64_t r = 0; r < P.C.regions; ++r)
        raw[r] = raw_bitwise(0, buf.data() + P.recs[r].off, (uint64_t)P.recs[r].rows * 1024 + P.recs[r].tail);
    std::vector<uint32_t> crcs(v.size(), 0);   // what the zeros of the empty spans leave
    for (uint64_t j = 0; j < P.C.live; ++j) {
        const CrcBatchEnt &E = P.ents[j];
        crcs[E.k] = crcb_fold(raw.data() + E.reg0, E.nreg, E.rows, E.size);
    }
    for (uint64_t k = 0; k < v.size(); ++k) {
        assert(crcs[k] == crc32_bitwise(buf.data() + v[k].off * (v[k].size != 0), v[k].size));
        ++folds;
    }
}

// crcb_fold at a region of the caller's choosing (the plan's smallest is 32 rows).
static void check_fold_rows(const uint8_t *p, uint64_t size, uint32_t rows) {
    const uint64_t obj_rows = size / 1024, region = (uint64_t)rows * 1024;
    const uint32_t nreg = obj_rows ? (uint32_t)((obj_rows + rows - 1) / rows) : 1;
    std::vector<uint32_t> raw(nreg);
    for (uint32_t q = 0; q < nreg; ++q) {
        const uint64_t lo = q * region, hi = q + 1 == nreg ? size : lo + region;
        raw[q] = raw_bitwise(0, p + lo, hi - lo);
    }
    assert(crcb_fold(raw.data(), nreg, rows, size) == crc32_bitwise(p, size));
    ++folds;
}

int main() {
    static_assert(sizeof(CrcBatchRec) == 24 && sizeof(CrcBatchEnt) == 32 && sizeof(s3dg_span) == 16, "table layout");
    // ---- the region of a call -------------------------------------------------
    assert(crc_batch_region_rows(0) == 32 && crc_batch_region_rows(4096 * 32) == 32);
    assert(crc_batch_region_rows(4096 * 33 - 1) == 32 && crc_batch_region_rows(4096 * 33) == 33);
    assert(crc_batch_region_rows(180 * 1024) == 45);   // 180 MiB of whole rows: not a power of two
    assert(crc_batch_region_rows(4096 * 256 - 1) == 255 && crc_batch_region_rows(4096 * 256) == 256);
    assert(crc_batch_region_rows(1ull << 43) == 256);
    {
        std::vector<s3dg_span> v;
        for (int k = 0; k < 90; ++k) v.push_back(s3dg_span{(uint64_t)k * 4 * MiB, 2 * MiB + (k % 3) * 1023});   // 180 MiB
        assert(plan_of(v).C.rows == 45);
        check_plan(v);
        v.assign(3, s3dg_span{0, 40 * KiB});
        assert(plan_of(v).C.rows == 32);
        check_plan(v);
        v.assign(5, s3dg_span{16, 256 * MiB + 5});
        assert(plan_of(v).C.rows == 256);
        check_plan(v);
    }
    // ---- plans: sizes around a row, a region and the cap, empties mixed in -------
    const uint64_t sizes[] = {1,         15,          16,         17,          1008,        1023,      1024,
                              1025,      2047,        2048,       2049,        32 * KiB - 1, 32 * KiB, 32 * KiB + 1,
                              33 * KiB,  64 * KiB - 1025, 64 * KiB, 64 * KiB + 1024, 96 * KiB + 1023, MiB + 5,
                              45 * KiB,  90 * KiB + 1, 256 * KiB,  256 * KiB + 1, 7 * MiB + 17};
    for (uint64_t s : sizes) check_plan({s3dg_span{48, s}});
    for (int round = 0; round < 1500; ++round) {
        std::vector<s3dg_span> v;
        const uint64_t n = 1 + rnd() % 24;
        for (uint64_t k = 0; k < n; ++k) {
            const uint64_t pick = rnd() % 10;
            uint64_t size = pick < 2 ? 0 : pick < 8 ? sizes[rnd() % (sizeof(sizes) / sizeof(sizes[0]))] : rnd() % (300 * MiB);
            if (round % 5 == 0 && pick == 9) size = rnd() % (6 * GiB);
            v.push_back(size ? s3dg_span{(rnd() % (1ull << 33)) * 16, size} : s3dg_span{rnd(), 0});   // empties: any off
        }
        if (round % 7 == 0) v.push_back(v[0]);   // a repeat: two entries, two sets of regions
        check_plan(v);
    }
    {   // only empties: nothing at all
        const std::vector<s3dg_span> v = {{7, 0}, {UINT64_MAX, 0}, {1, 0}};
        const Plan P = plan_of(v);
        assert(P.C.live == 0 && P.C.regions == 0 && crc_batch_table_bytes(P.C) == 0);
        check_plan(v);
        check_plan({});
    }
    // ---- the cap: counts only, up to the largest object ---------------------------
    const uint64_t big[] = {128 * MiB,         128 * MiB + KiB,  GiB - 1,          GiB,        GiB + 1024,
                            GiB + MiB + 17,    2 * GiB + 5,      1ull << 40,       (1ull << 40) + 1024, (1ull << 43) - 1,
                            kSpanBatchMaxObj};
    for (uint64_t s : big) {
        const uint32_t call_rows = crc_batch_region_rows(s / 1024);
        const uint32_t r = crc_batch_obj_rows(s, call_rows);
        const uint64_t n = crc_batch_obj_regions(s, r);
        assert(n >= 1 && n <= kCrcBatchMaxRegions && n * r >= s / 1024 && (n - 1) * (uint64_t)r < s / 1024);
        if (r > call_rows) assert(crc_batch_obj_regions(s, r / 2) > kCrcBatchMaxRegions);
        check_plan({s3dg_span{0, s}});
        check_plan({s3dg_span{64, 100}, s3dg_span{0, s}, s3dg_span{3, 0}, s3dg_span{4096, 40 * KiB}});
    }
    assert(crc_batch_obj_rows(GiB + MiB + 17, 256) == 512 && crc_batch_obj_regions(GiB + MiB + 17, 512) == 2050);
    assert(crc_batch_obj_rows(kSpanBatchMaxObj, 256) == (1u << 21) && crc_batch_obj_regions(kSpanBatchMaxObj, 1u << 21) == 4096);
    // ---- the algebra ---------------------------------------------------------------
    assert(crcb_multmodp(0, 0x12345678u) == 0 && crcb_multmodp(1u << 31, 0x12345678u) == 0x12345678u);
    assert(crcb_x8n(0) == 1u << 31 && crcb_x8n(1) == 1u << 23 && crcb_x8n(3) == 1u << 7);
    for (int k = 0; k < 200; ++k) {
        const uint64_t a = rnd() >> (4 + rnd() % 50), b = rnd() >> (4 + rnd() % 50);
        assert(crcb_x8n(a + b) == crcb_multmodp(crcb_x8n(a), crcb_x8n(b)));
        const uint32_t u = (uint32_t)rnd(), w = (uint32_t)rnd();
        assert(crcb_multmodp(u, w) == crcb_multmodp(w, u));
    }
    std::vector<uint8_t> buf(4 * 32 * KiB + 4096);
    for (uint8_t &b : buf) b = (uint8_t)(rnd() >> 32);
    for (uint64_t len = 0; len <= 2100; ++len) check_fold(buf, {s3dg_span{(len % 64) * 16, len}});
    for (int d = -17; d <= 17; ++d) check_fold(buf, {s3dg_span{32, (uint64_t)(32 * KiB + d)}});
    check_fold(buf, {s3dg_span{16, 3 * 32 * KiB + 1023}});
    check_fold(buf, {s3dg_span{0, 2 * 32 * KiB}});
    check_fold(buf, {s3dg_span{5, 0}, s3dg_span{1024, 3 * 32 * KiB + 1023}, s3dg_span{0, 33 * KiB}, s3dg_span{0, 33 * KiB},
                     s3dg_span{UINT64_MAX, 0}, s3dg_span{2048, 1023}, s3dg_span{64, 32 * KiB - 1}, s3dg_span{9, 0}});
    {   // content the algebra could hide a slip behind
        std::vector<uint8_t> z(70 * KiB, 0), f(70 * KiB, 0xFF);
        const uint64_t lens[] = {1, 16, 1024, 33 * KiB + 7, 70 * KiB};
        for (uint64_t len : lens) {
            check_fold(z, {s3dg_span{0, len}});
            check_fold(f, {s3dg_span{0, len}});
        }
    }
    const uint64_t cut_lens[] = {0, 1, 1023, 1024, 1025, 2048, 3071, 3072, 3073, 10 * KiB + 5, 15 * KiB, 16 * KiB + 1023};
    for (uint32_t rows : {1u, 2u, 3u, 5u})
        for (uint64_t len : cut_lens) check_fold_rows(buf.data() + 16, len, rows);
    // ---- for the Python side: CRC-32s of strings it can rebuild ----------------------
    const uint64_t out_lens[] = {0, 1, 1023, 1024, 2100, 32 * KiB + 17, 3 * 32 * KiB + 1023};
    for (uint64_t len : out_lens) {
        std::vector<uint8_t> s(len + 1);
        for (uint64_t i = 0; i < len; ++i) s[i] = (uint8_t)(i * 131 + 7);
        const Plan P = plan_of({s3dg_span{0, len}});
        uint32_t crc = 0;
        if (len) {
            std::vector<uint32_t> raw(P.C.regions);
            for (uint64_t r = 0; r < P.C.regions; ++r)
                raw[r] = raw_bitwise(0, s.data() + P.recs[r].off, (uint64_t)P.recs[r].rows * 1024 + P.recs[r].tail);
            crc = crcb_fold(raw.data(), P.ents[0].nreg, P.ents[0].rows, len);
        }
        printf("crc_%llu|%08x\n", (unsigned long long)len, crc);
    }
    printf("plans|%llu\nfolds|%llu\n", (unsigned long long)plans, (unsigned long long)folds);
    return 0;
}
