// tfrecord_extract_plan_sweep.cpp — the pure rules of s3dg_tfrecord_extract_batch
// (csrc/s3dg_tfrecord_extract_plan.h) on the CPU.  Asserted here:
//
//   tiles     tfx_region's regions g = 0..rpr-1 tile [0, a + len) in order, only
//             the last has a tail, none but a len == 0 record's holds no payload
//             byte, and rpr stays at or below kCrcBatchMaxRegions after doubling:
//             rows {32, 33, 45, 64, 255, 256} x a 0..15 x the length family
//             (0..70, m region + d, one length past the cap).
//   folds     each region's raw bit by bit over the padded bytes with the first a
//             masked; tfr_crc_fold over them is the bit-by-bit CRC-32 of the
//             payload.  The subset: rows 32 and 33 with lengths 0..70 at every a
//             and the m region + d lengths at a in {0, 1, 8, 15}; rows 45 and 256
//             with m in {1, 2}, d in {-15, 1009}, a in {0, 15}.  No length past
//             the cap (128 MiB bit by bit).
//   needs     tfx_first_needs(k, a, u) for every (a, u, k) is "dword k holds one
//             of the piece's bytes [a, 16)", and the piece rebuilt as the kernel
//             does (get_first, the alignbyte shift, mask_first, restated below)
//             from a buffer whose other dwords are poison is the byte copy with
//             the first a bytes zero.
//   bounds    for seeded random and adversarial sets of takes at every rows value,
//             reached by padding the reach: the regions and long records of the
//             taken takes stay at or below max_regions and max_long; so does the
//             header's own count, 1 + (len + 15) / region per record, for lengths
//             that sum to the reach; tfx_layout's sections are disjoint, in
//             order, each at a multiple of 256.
//   searches  tfx_find_take and tfx_find_rec against a linear scan over tables
//             with empty takes and zero-region entries in front, behind, and in
//             runs of 1..3 in the middle.
//   wraps     tfx_entry_fits, tfx_entry_chains, tfx_run_payload, tfx_dst_pos and
//             tfx_reach against 128-bit arithmetic near 0, 16, 2^63 and 2^64.
//   refusals  every refusal of tfx_check with its exact message.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <vector>

#include "s3dg_tfrecord_extract_plan.h"

using namespace s3dg;
typedef unsigned __int128 u128;

#define CHECK(cond, what)                                                          \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fprintf(stderr, "line %d: %s: %s\n", __LINE__, what, #cond);           \
            abort();                                                               \
        }                                                                          \
    } while (0)

static uint32_t raw_bits(uint32_t c, const uint8_t *p, uint64_t n) {   // the CRC register over n bytes, no inversion
    for (uint64_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (kCrcBatchPoly & (0u - (c & 1)));
    }
    return c;
}
static uint32_t crc_bits(const uint8_t *p, uint64_t n) { return ~raw_bits(0xFFFFFFFFu, p, n); }

static uint64_t g_seed = 0x7F4A7C15u;
static uint64_t rnd() {   // splitmix64: the same draws on every machine
    uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static const uint32_t kRows[] = {32, 33, 45, 64, 255, 256};
static const int kDeltas[] = {-17, -16, -15, -1, 0, 1, 1008, 1009, 1010};

static std::vector<uint64_t> long_family(uint32_t rows) {
    std::vector<uint64_t> v;
    for (uint64_t m = 1; m <= 3; ++m)
        for (int d : kDeltas) v.push_back(m * rows * kCrcRowBytes + (uint64_t)(int64_t)d);
    return v;
}
static uint64_t past_the_cap(uint32_t rows) { return kCrcBatchMaxRegions * rows * kCrcRowBytes + 2 * 1024 + 5; }

// ---- tiles ---------------------------------------------------------------------------------
static uint64_t tiles() {
    uint64_t cases = 0;
    for (uint32_t rows : kRows) {
        std::vector<uint64_t> lens;
        for (uint64_t n = 0; n <= 70; ++n) lens.push_back(n);
        for (uint64_t n : long_family(rows)) lens.push_back(n);
        lens.push_back(past_the_cap(rows));
        for (uint64_t len : lens) {
            const uint32_t rec_rows = tfv_rec_rows(len, rows);
            const uint64_t rpr = tfv_rec_regions(len, rec_rows);
            CHECK(rpr >= 1 && rpr <= kCrcBatchMaxRegions, "regions per record after doubling");
            CHECK(rec_rows % rows == 0 && (rec_rows == rows || tfv_rec_regions(len, rec_rows / 2) > kCrcBatchMaxRegions),
                  "the region is doubled only past the cap");
            CHECK((len == past_the_cap(rows)) == (rec_rows != rows), "only the length past the cap is doubled");
            for (uint32_t a = 0; a < 16; ++a) {
                uint64_t cursor = 0;
                for (uint32_t g = 0; g < rpr; ++g) {
                    const TfxRegion R = tfx_region(a, len, g, (uint32_t)rpr, rec_rows);
                    CHECK(R.pad_lo == cursor, "a region starts where the one before ends");
                    CHECK(R.tail < kCrcRowBytes && R.nrows <= rec_rows, "a region's rows and tail");
                    CHECK(g + 1 == rpr || (R.tail == 0 && R.nrows == rec_rows), "only the last region has a tail");
                    const uint64_t hi = R.pad_lo + (uint64_t)R.nrows * kCrcRowBytes + R.tail, lo = R.pad_lo > a ? R.pad_lo : a;
                    CHECK(len == 0 ? hi == lo : hi > lo, "no region but an empty record's is empty");
                    cursor = hi;
                }
                CHECK(cursor == a + len, "the regions end at a + len");
                ++cases;
            }
        }
    }
    return cases;
}

// ---- folds ---------------------------------------------------------------------------------
static void fold_one(uint32_t rows, uint32_t a, uint64_t len, const uint32_t *pw) {
    std::vector<uint8_t> pad(a + len, 0);   // the padded record, its first a bytes masked
    for (uint64_t i = 0; i < len; ++i) pad[a + i] = (uint8_t)(i * 131 + (i >> 8) * 29 + len + 7);
    const uint32_t rec_rows = tfv_rec_rows(len, rows), rpr = (uint32_t)tfv_rec_regions(len, rec_rows);
    std::vector<uint32_t> raw(rpr);
    for (uint32_t g = 0; g < rpr; ++g) {
        const TfxRegion R = tfx_region(a, len, g, rpr, rec_rows);
        raw[g] = raw_bits(0, pad.data() + R.pad_lo, (uint64_t)R.nrows * kCrcRowBytes + R.tail);
    }
    const uint32_t crc = crc_bits(pad.data() + a, len), init = tfv_init(len, pw);
    CHECK(tfr_crc_fold(raw.data(), rpr, rec_rows, a, len, init) == crc, "the fold of the regions' raws is the payload's CRC");
    if (rpr == 1) CHECK(tfr_crc_one(raw[0], init) == crc, "a record of one region is finished from its raw");
}
static uint64_t folds() {
    uint32_t pw[kTfvPowers];
    tfv_powers(pw);
    uint64_t cases = 0;
    for (uint32_t rows : {32u, 33u}) {
        for (uint64_t len = 0; len <= 70; ++len)
            for (uint32_t a = 0; a < 16; ++a, ++cases) fold_one(rows, a, len, pw);
        for (uint64_t len : long_family(rows))
            for (uint32_t a : {0u, 1u, 8u, 15u}) fold_one(rows, a, len, pw), ++cases;
    }
    for (uint32_t rows : {45u, 256u})
        for (uint64_t m = 1; m <= 2; ++m)
            for (int d : {-15, 1009})
                for (uint32_t a : {0u, 15u}) fold_one(rows, a, m * rows * kCrcRowBytes + (uint64_t)(int64_t)d, pw), ++cases;
    return cases;
}

// ---- needs: a record's first piece, as k_tfx_regions and k_npz_regions build it -----------
struct U4 {
    uint32_t x, y, z, w;
};
// v_alignbyte_b32: bytes [u, u + 4) of the eight bytes lo, hi
static uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t u) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (u & 3))); }
// v with its first a bytes zeroed
static U4 mask_first(const U4 v, uint32_t a) {
    auto m = [&](uint32_t w, uint32_t k) -> uint32_t { return a <= k ? w : a >= k + 4 ? 0u : w & (0xFFFFFFFFu << (8 * (a - k))); };
    return U4{m(v.x, 0), m(v.y, 4), m(v.z, 8), m(v.w, 12)};
}
static uint64_t needs() {
    uint64_t cases = 0;
    for (uint32_t a = 0; a < 16; ++a)
        for (uint32_t u = 0; u < 4; ++u) {
            // the piece's byte y lies at stream byte u + y of the five dwords from the multiple of 4 below it
            uint8_t stream[20], mem[20];
            for (uint32_t i = 0; i < 20; ++i) stream[i] = (uint8_t)(0x11 + 9 * i + 16 * a + u);   // never zero
            bool holds[5] = {false, false, false, false, false};
            for (uint32_t y = a; y < 16; ++y) holds[(u + y) / 4] = true;
            for (uint32_t k = 0; k < 5; ++k, ++cases) {
                CHECK(tfx_first_needs(k, a, u) == holds[k], "tfx_first_needs is exact");
                for (uint32_t b = 0; b < 4; ++b) mem[4 * k + b] = holds[k] ? stream[4 * k + b] : (uint8_t)0xA5;
            }
            uint32_t w[5];   // get_first
            for (uint32_t d = 0; d < 5; ++d) {
                uint32_t q;
                memcpy(&q, mem + 4 * d, 4);
                w[d] = tfx_first_needs(d, a, u) ? q : 0u;
            }
            const U4 v{alignbyte(w[1], w[0], u), alignbyte(w[2], w[1], u), alignbyte(w[3], w[2], u), alignbyte(w[4], w[3], u)};
            const U4 h = mask_first(v, a);
            uint8_t stored[16], hashed[16];
            memcpy(stored, &v, 16);
            memcpy(hashed, &h, 16);
            for (uint32_t y = 0; y < 16; ++y) {
                if (y >= a) CHECK(stored[y] == stream[u + y], "the bytes put_bytes stores are the record's");
                CHECK(hashed[y] == (y < a ? 0 : stream[u + y]), "the hashed piece is the byte copy with the first a bytes zero");
            }
        }
    return cases;
}

// ---- bounds --------------------------------------------------------------------------------
struct Set {
    std::vector<s3dg_tfrecord_take> takes;
    std::vector<std::vector<uint64_t>> lens;
    std::vector<bool> taken;
};
enum { kExact, kGenerous, kShort };
static void add_take(Set &S, const std::vector<uint64_t> &lens, int cap_mode, uint64_t more_bytes) {
    uint64_t payload = 0;
    for (uint64_t n : lens) payload += n;
    const uint64_t count = lens.size();
    const uint64_t cap = cap_mode == kGenerous ? payload + 1 + below(5000) : cap_mode == kShort && payload ? payload - 1 : payload;
    S.takes.push_back(s3dg_tfrecord_take{64 + below(16), payload + kTfrFraming * count + more_bytes, 16 * below(4), below(5), count,
                                         16 * below(1000), cap});
    S.lens.push_back(lens);
    S.taken.push_back(payload <= cap);
}
static uint64_t reach128(const s3dg_tfrecord_take &t) {
    if (t.count == 0) return 0;
    const u128 want = (u128)t.dst_cap + (u128)kTfrFraming * t.count;
    return want < t.bytes ? (uint64_t)want : t.bytes;
}
// A take of one empty record whose reach brings the call to regions of `rows` rows.
static void pad_to(Set &S, uint32_t rows) {
    uint64_t reach = 0;
    for (const auto &t : S.takes) reach += reach128(t);
    const uint64_t target = (uint64_t)rows * kCrcBatchWaves * kCrcRowBytes;
    if (reach >= target) return;
    S.takes.push_back(s3dg_tfrecord_take{0, target - reach, 0, 0, 1, 0, target - reach});
    S.lens.push_back(std::vector<uint64_t>(1, 0));
    S.taken.push_back(true);
}
static void check_bounds(const Set &S, uint32_t rows) {
    const uint64_t n = S.takes.size();
    TfxCounts C;
    std::string why;
    CHECK(tfx_check(4096, 8192, 1 << 20, S.takes.data(), n, true, &C, &why), "a set of takes passes the checks");
    uint64_t ents = 0, reach = 0, regions = 0, longs = 0;
    for (uint64_t k = 0; k < n; ++k) {
        ents += S.takes[k].count;
        reach += reach128(S.takes[k]);
        CHECK(tfx_reach(S.takes[k]) == reach128(S.takes[k]), "a take's reach");
        if (!S.taken[k]) continue;
        for (uint64_t len : S.lens[k]) {
            const uint64_t nr = tfv_rec_regions(len, tfv_rec_rows(len, C.rows));
            regions += nr;
            longs += nr > 1;
        }
    }
    CHECK(C.ents == ents && C.reach == reach, "the counts of a call");
    CHECK(C.rows == (n ? rows : 0u), "the padding reaches the region size under test");
    CHECK(regions <= C.max_regions, "max_regions holds the regions of the taken takes");
    CHECK(longs <= C.max_long, "max_long holds the long records of the taken takes");
    const uint64_t tmp = 1 + below(100000);
    const TfxLayout L = tfx_layout(C, n, tmp);
    CHECK(L.upload == kTfxTakeOff + (n + 1) * sizeof(TfxTake), "the uploaded bytes");
    CHECK(L.res >= L.upload && L.reg0 >= L.res + kTfxCounterBytes + n * sizeof(TfxDevRes) && L.cst >= L.reg0 + (C.ents + 1) * 8 &&
              L.longs >= L.cst + C.ents * sizeof(TfvConst) && L.raw >= L.longs + C.max_long * 8 &&
              L.tmp >= L.raw + C.max_regions * 4 && L.bytes == L.tmp + tmp,
          "the sections are disjoint and in order");
    CHECK((L.res | L.reg0 | L.cst | L.longs | L.raw | L.tmp) % 256 == 0, "every section at a multiple of 256");
}
// The header's own argument: a record has at most 1 + (len + 15) / region regions
// and the lengths sum to at most the reach.  One take whose reach is exactly the
// sum of the lengths, padded to `rows`.
static void check_premise(const std::vector<uint64_t> &lens, uint32_t rows) {
    uint64_t sum = 0;
    for (uint64_t n : lens) sum += n;
    Set S;
    S.takes.push_back(s3dg_tfrecord_take{0, sum, 0, 0, lens.size(), 0, sum});
    pad_to(S, rows);
    TfxCounts C;
    std::string why;
    CHECK(tfx_check(4096, 8192, 1 << 20, S.takes.data(), S.takes.size(), true, &C, &why) && C.rows == rows, "the premise's call");
    const uint64_t region = (uint64_t)rows * kCrcRowBytes;
    uint64_t regions = S.takes.size() - 1, longs = 0;   // the padding's empty record
    for (uint64_t len : lens) {
        regions += 1 + (len + 15) / region;
        longs += len > region;
    }
    CHECK(regions <= C.max_regions, "max_regions holds 1 + (len + 15) / region per record of lengths that sum to the reach");
    CHECK(longs <= C.max_long, "max_long holds the records longer than a region");
}
static uint64_t bounds() {
    uint64_t sets = 0;
    for (uint32_t rows : kRows) {
        const uint64_t region = (uint64_t)rows * kCrcRowBytes;
        const std::vector<uint64_t> fam = long_family(rows);
        // what the call may reach before its region grows past `rows`
        const uint64_t budget = rows == kCrcBatchMaxRows ? 1ull << 40 : (uint64_t)rows * kCrcBatchWaves * kCrcRowBytes + (3ull << 20);
        for (int round = 0; round < 40; ++round, ++sets) {
            Set S;
            uint64_t used = 0;
            for (uint64_t k = 0, n = 1 + below(6); k < n; ++k) {
                std::vector<uint64_t> lens(round == 0 && k == 0 ? 0 : below(301));
                for (uint64_t &len : lens) {
                    len = below(8) ? below(71) : fam[below(fam.size())];
                    if (used + len + 6000 > budget) len %= 71;
                    used += len + kTfrFraming;
                }
                used += 5000;   // a generous dst_cap
                add_take(S, lens, (int)below(3), below(3) ? 0 : below(4096));
            }
            pad_to(S, rows);
            check_bounds(S, rows);
        }
        {   // a record past the cap between two short ones
            Set S;
            add_take(S, {5, past_the_cap(rows), 70}, kExact, 0);
            pad_to(S, rows);
            check_bounds(S, rows);
            ++sets;
        }
        // aimed at the bound: as many records as the region size under test lets a call hold
        const uint64_t many = rows == kCrcBatchMaxRows ? 100000 : 3000;
        const std::vector<uint64_t> just_two(many, region + 1009), just_one(many, region - 15);
        for (const auto &lens : {just_two, just_one}) {
            Set S;
            add_take(S, lens, kExact, 0);
            pad_to(S, rows);
            check_bounds(S, rows);
            check_premise(lens, rows);
            ++sets;
        }
        for (uint64_t k = 1; k <= 4; ++k, ++sets) {
            std::vector<uint64_t> lens(2048 * k, 0);
            lens.insert(lens.begin() + (long)(k * 511), 3 * region + 1010);
            Set S;
            add_take(S, lens, kExact, 0);
            pad_to(S, rows);
            check_bounds(S, rows);
            check_premise(lens, rows);
        }
    }
    Set none;
    check_bounds(none, 0);
    return sets;
}

// ---- searches ------------------------------------------------------------------------------
static uint64_t searches() {
    uint64_t probes = 0;
    const uint64_t some[][3] = {{1, 1, 1}, {2, 5, 1}, {7, 1, 3}};
    for (const auto &c : some)
        for (uint32_t front = 0; front <= 3; ++front)
            for (uint32_t back = 0; back <= 3; ++back)
                for (uint32_t m1 = 1; m1 <= 3; ++m1)
                    for (uint32_t m2 = 1; m2 <= 3; ++m2) {
                        std::vector<uint64_t> counts(front, 0);   // empty takes, or entries without regions
                        counts.push_back(c[0]);
                        counts.insert(counts.end(), m1, 0);
                        counts.push_back(c[1]);
                        counts.insert(counts.end(), m2, 0);
                        counts.push_back(c[2]);
                        counts.insert(counts.end(), back, 0);
                        const uint64_t n = counts.size();
                        std::vector<s3dg_tfrecord_take> takes;
                        for (uint64_t v : counts) takes.push_back(s3dg_tfrecord_take{0, 64, 0, 0, v, 0, 64});
                        uint32_t pw[kTfvPowers] = {0};
                        std::vector<uint8_t> tab(kTfxTakeOff + (n + 1) * sizeof(TfxTake));
                        tfx_build(takes.data(), n, pw, tab.data());
                        const TfxTake *tk = reinterpret_cast<const TfxTake *>(tab.data() + kTfxTakeOff);
                        std::vector<uint64_t> reg0(n + 1, 0);   // the scan of the counts, read as regions per entry
                        for (uint64_t k = 0; k < n; ++k) reg0[k + 1] = reg0[k] + counts[k];
                        CHECK(tk[n].ent0 == reg0[n], "the table's closing entry");
                        for (uint64_t j = 0; j < reg0[n]; ++j, ++probes) {
                            uint64_t owner = n;
                            for (uint64_t k = 0; k < n; ++k)
                                if (reg0[k] <= j && j < reg0[k + 1]) owner = k;
                            CHECK(owner < n && counts[owner], "one owner");
                            CHECK(tk[owner].ent0 == reg0[owner], "a take's first entry");
                            CHECK(tfx_find_take(tk, n, j) == owner, "tfx_find_take against the linear scan");
                            CHECK(tfx_find_rec(reg0.data(), n, j) == owner, "tfx_find_rec against the linear scan");
                        }
                    }
    return probes;
}

// ---- wraps ---------------------------------------------------------------------------------
static uint64_t wraps() {
    const uint64_t T63 = 1ull << 63, M = UINT64_MAX;
    const uint64_t V[] = {0, 1, 15, 16, 17, 31, 32, T63 - 16, T63 - 1, T63, T63 + 1, T63 + 16, M - 32, M - 17, M - 16, M - 15, M - 1, M};
    const u128 one = 1, T64 = one << 64;
    uint64_t cases = 0;
    for (uint64_t o : V)
        for (uint64_t s : V)
            for (uint64_t x : V) {
                ++cases;
                CHECK(tfx_entry_fits(o, s, x) == (s >= kTfrFraming && (u128)o + s <= x), "tfx_entry_fits");
                if ((u128)o + s < T64) CHECK(tfx_entry_chains(o, s, x) == ((u128)o + s == x), "tfx_entry_chains");
                // o_first = x, the last entry <o, s>, 0..3 records and as many as fit
                const u128 end = (u128)o + s;
                if (x <= o && end < T64 && s >= kTfrFraming)
                    for (uint64_t count : {(uint64_t)1, (uint64_t)2, (uint64_t)((end - x) / kTfrFraming)}) {
                        if (count == 0 || (u128)kTfrFraming * count > end - x) continue;
                        CHECK((u128)tfx_run_payload(x, o, s, count) == end - x - (u128)kTfrFraming * count, "tfx_run_payload");
                        const uint64_t i = count - 1;   // the last record's place: behind i records of no payload at the least
                        if ((u128)kTfrFraming * i <= (u128)o - x)
                            CHECK((u128)tfx_dst_pos(x, o, i) == (u128)o - x - (u128)kTfrFraming * i, "tfx_dst_pos");
                    }
                for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)15, (uint64_t)16, kTfxMaxEntries}) {
                    const s3dg_tfrecord_take t{0, o, 0, 0, count, 0, s};
                    CHECK(tfx_reach(t) == reach128(t), "tfx_reach");
                }
            }
    return cases;
}

// ---- refusals ------------------------------------------------------------------------------
static int refusals() {
    const uint64_t B = 4096, I = 8192, D = 1 << 20, M = UINT64_MAX;
    std::set<std::string> seen;   // the refusals met, without their "take k: "
    TfxCounts C;
    std::string why;
    using Ts = std::vector<s3dg_tfrecord_take>;   // (off, bytes, idx_off, first, count, dst_off, dst_cap)
    const s3dg_tfrecord_take good{16, 64, 0, 0, 1, 0, 64};
    auto call = [&](uint64_t base, uint64_t idx, uint64_t dst, const Ts &t, bool total = true) {
        why.clear();
        return tfx_check(base, idx, dst, t.data(), t.size(), total, &C, &why);
    };
    auto refused = [&](bool ok, const char *msg) {
        if (ok || why != msg) {
            fprintf(stderr, "expected \"%s\", got \"%s\"\n", msg, why.c_str());
            abort();
        }
        seen.insert(why.compare(0, 5, "take ") ? why : why.substr(why.find(": ") + 2));
    };
    CHECK(call(B, I, D, {good}) && C.ents == 1 && C.reach == 64 && C.rows == 32 && C.max_regions == 3 && C.max_long == 0, "a good take");
    CHECK(call(0, 0, 0, {}, false) && C.ents == 0 && C.rows == 0, "n == 0 succeeds whatever the pointers");
    refused(call(0, I, D, {good}), "null base");
    refused(call(B, 0, D, {good}), "null idx_base");
    refused(call(B, I, 0, {good}), "null dst_base");
    refused(call(B, I, D, {good}, false), "null output");
    why.clear();
    refused(tfx_check(B, I, D, nullptr, 1, true, &C, &why), "null take array");
    refused(call(B, I + 8, D, {good}), "idx_base must be 16-byte aligned");
    refused(call(B, I, D + 8, {good}), "dst_base must be 16-byte aligned");
    why.clear();
    CHECK(kTfrMaxShards == 0xFFFFFFFFull, "the limit on takes");
    refused(tfx_check(B, I, D, &good, kTfrMaxShards + 1, true, &C, &why), "more than 2^32 - 1 takes in one call");
    refused(call(B, I, D, {good, {16, 64, 8, 0, 1, 0, 64}}), "take 1: idx_off must be a multiple of 16");
    refused(call(B, I, D, {good, {16, 64, 0, 0, 1, 8, 64}}), "take 1: dst_off must be a multiple of 16");
    CHECK(call(B, I, D, {{16, 64, 0, M - 2, 2, 0, 64}}) == false && why == "take 0: idx_off + index overflows", "first + count at 2^64 - 1");
    refused(call(B, I, D, {{16, 64, 0, M - 1, 2, 0, 64}}), "take 0: first + count overflows");
    CHECK(call(B, I, D, {{M - B - 64, 64, 0, 0, 1, 0, 64}}), "off + bytes ends at 2^64 - 1");
    refused(call(B, I, D, {{M - B - 63, 64, 0, 0, 1, 0, 64}}), "take 0: off + bytes overflows");
    refused(call(B, I, D, {{M, 64, 0, 0, 1, 0, 64}}), "take 0: off + bytes overflows");
    CHECK(call(B, I, D, {{16, 64, 0, 0, 1, M - D - 15 - 64, 64}}), "dst_off + dst_cap ends below 2^64");
    refused(call(B, I, D, {{16, 64, 0, 0, 1, M - D - 15, 64}}), "take 0: dst_off + dst_cap overflows");
    refused(call(B, I, D, {{16, 64, 0, 0, 1, M - 15, 64}}), "take 0: dst_off + dst_cap overflows");
    CHECK(call(B, I, D, {{16, 64, 0, (M >> 4) - 1 - (I >> 4), 1, 0, 64}}), "the index ends at 2^64 - 16");
    refused(call(B, I, D, {{16, 64, 0, (M >> 4) - (I >> 4), 1, 0, 64}}), "take 0: idx_off + index overflows");
    refused(call(B, I, D, {{16, 64, 0, M >> 4, 1, 0, 64}}), "take 0: idx_off + index overflows");
    refused(call(B, I, D, {{16, 64, M - 15 - I + 16, 0, 1, 0, 64}}), "take 0: idx_off + index overflows");
    CHECK(call(B, I, D, {{16, 64, 0, 0, kTfxMaxEntries, 0, 64}}) && C.ents == kTfxMaxEntries, "2^31 - 2 records pass");
    refused(call(B, I, D, {{16, 64, 0, 0, kTfxMaxEntries, 0, 64}, {16, 64, 0, 0, 0, 0, 64}, good}),
            "take 2: more than 2^31 - 2 records in one call");
    CHECK(call(B, I, D, {{16, kTfrMaxBytes, 0, 0, 1, 0, kTfrMaxBytes}}) && C.reach == kTfrMaxBytes && C.rows == 256, "2^46 stream bytes pass");
    refused(call(B, I, D, {{16, kTfrMaxBytes, 0, 0, 1, 0, kTfrMaxBytes}, {16, 1, 0, 0, 1, 0, 0}}),
            "take 1: more than 2^46 stream bytes in one call");
    refused(call(B, I, D, {good, {16, kTfrMaxBytes + 1, 0, 0, 1, 0, kTfrMaxBytes}}), "take 1: more than 2^46 stream bytes in one call");
    return (int)seen.size();
}

int main() {
    const int refused = refusals();
    const uint64_t t = tiles(), n = needs(), s = searches(), w = wraps(), b = bounds(), f = folds();
    printf("refusals|%d\ntiles|%llu\nfolds|%llu\nneeds|%llu\nbounds|%llu\nsearches|%llu\nwraps|%llu\n", refused, (unsigned long long)t,
           (unsigned long long)f, (unsigned long long)n, (unsigned long long)b, (unsigned long long)s, (unsigned long long)w);
    return 0;
}
