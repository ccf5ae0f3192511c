// The batch verify's plan (csrc/s3dg_verify_batch_plan.h) over a sweep of
// descriptor arrays, with g++ alone.  Every property is asserted here (exit
// status 1 and a line on stderr at the first failure); stdout carries the
// number of arrays checked and the refusal texts, which
// tests/test_verify_batch_cpu.py and tests/test_gpu_verify_batch.py compare
// with the contract's and with what the C call says.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "s3dg_verify_batch_plan.h"

using namespace s3dg;

static unsigned long long g_case;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: %s  (array %llu)\n", __FILE__, __LINE__, #cond, g_case); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

struct Rec {
    uint32_t first, obj;
};

// The device's work on one sub-batch, restated on the host: the exclusive scan
// of the tile counts and k_verify_batch_map's records.
static std::vector<Rec> records(const s3dg_obj_desc *st, uint64_t cnt, uint32_t tshift) {
    std::vector<Rec> R;
    for (uint64_t k = 0; k < cnt; ++k) {
        const uint64_t lo = R.size(), hi = lo + verify_obj_tiles(st[k].size, tshift);
        for (uint64_t q = lo; q < hi; ++q) R.push_back({(uint32_t)((q - lo) << tshift), (uint32_t)k});
    }
    return R;
}

static void check_good(const std::vector<s3dg_obj_desc> &d) {
    const uint64_t n = d.size();
    const VerifyBatchCheck C = verify_batch_check(d.data(), n);
    CHECK(C.msg == nullptr && C.bad == UINT64_MAX);
    uint64_t live = 0, blocks = 0;
    for (const auto &o : d) {
        live += o.size != 0;
        blocks += (o.size + kBlk - 1) / kBlk;
    }
    CHECK(C.live == live && C.blocks == blocks);
    // the cuts: 16 Ki, 32 Ki, ... 256 Ki, the last one ragged, covering [0, n) in order
    uint64_t sub = kVerifySubFirst, want = kVerifySubFirst, seen_blocks = 0;
    std::vector<uint32_t> hits;
    for (uint64_t k0 = 0, k1; k0 < n; k0 = k1) {
        k1 = verify_batch_cut(k0, n, sub);
        CHECK(k1 > k0 && k1 <= n && (k1 - k0 == want || (k1 == n && k1 - k0 < want)));
        want = want * 2 < kVerifySubMax ? want * 2 : kVerifySubMax;
        CHECK(sub == want);
        const uint64_t cnt = k1 - k0;
        std::vector<s3dg_obj_desc> st(cnt);
        const VerifyBatchScan P = verify_batch_scan(d.data(), k0, k1, st.data());
        CHECK(memcmp(st.data(), d.data() + k0, cnt * sizeof(s3dg_obj_desc)) == 0);   // staged as they are
        seen_blocks += P.blocks;
        const uint32_t pick = verify_batch_tile_shift(P, 0);
        CHECK(pick >= kTileShiftAutoMin && pick <= kTileShiftMax);
        for (uint32_t knob = kTileShiftMin; knob <= kTileShiftMax; ++knob)   // every tile size can be forced
            CHECK(verify_batch_tile_shift(P, knob) == knob);
        CHECK(verify_batch_tile_shift(P, kTileShiftMax + 1) == pick);
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) {
            const std::vector<Rec> R = records(st.data(), cnt, sh);
            CHECK(R.size() == P.ntiles[sh]);
            CHECK(kVerifyMaxGrid % (1ull << sh) == 0);                      // every sub-launch starts on a tile
            // every slot of every record: its block is hit exactly once, dead slots lie past the end
            uint64_t off = 0, total = 0;
            std::vector<uint64_t> first_hit(cnt);
            for (uint64_t k = 0; k < cnt; ++k) {
                first_hit[k] = off;
                off += (st[k].size + kBlk - 1) / kBlk;
            }
            hits.assign(off, 0);
            uint64_t recs_of_empty = 0;
            for (uint64_t q = 0; q < R.size(); ++q) {
                const Rec &r = R[q];
                CHECK(r.obj < cnt);
                CHECK(verify_obj_index(k0, r.obj) == k0 + r.obj);           // the caller's k
                CHECK(memcmp(&d[verify_obj_index(k0, r.obj)], &st[r.obj], sizeof(s3dg_obj_desc)) == 0);
                recs_of_empty += st[r.obj].size == 0;
                bool live_slot = false;
                for (uint64_t s = q << sh; s < (q + 1) << sh; ++s) {
                    const int64_t ib = verify_slot_block(r.first, s, sh, st[r.obj].size);
                    if (ib < 0) continue;
                    live_slot = true;
                    CHECK((uint64_t)ib * kBlk < st[r.obj].size);
                    ++hits[first_hit[r.obj] + (uint64_t)ib];
                    ++total;
                }
                CHECK(live_slot);                                           // no record without a live block
            }
            CHECK(recs_of_empty == 0);
            CHECK(total == P.blocks && total == off);
            for (uint32_t h : hits) CHECK(h == 1);
        }
    }
    CHECK(seen_blocks == blocks);
    CHECK(verify_batch_obj_bytes(n) == n * 24);
}

static const uint64_t kSizes[] = {0,    1,    15,        16,         17,          4095,           4096,
                                  4097, 8191, 12288 + 3, 20480 + 5, 262144 - 1, (3ull << 20) + 7, 64ull << 20};

static std::vector<s3dg_obj_desc> make(uint64_t n, int flavour) {
    std::vector<s3dg_obj_desc> d(n);
    uint64_t off = 0;
    for (uint64_t k = 0; k < n; ++k) {
        uint64_t size = kSizes[rnd() % (flavour == 2 || n > 300 ? 10 : 14)];   // long arrays: small objects
        if (flavour == 1 && rnd() % 3 == 0) size = 0;
        if (flavour == 3) size = 0;
        const uint32_t den = 1 + (uint32_t)(rnd() % 7);
        d[k] = {off, size, rnd(), rnd() % 5, (uint32_t)(rnd() % den), den};
        if (size == 0 && rnd() % 2) d[k] = {off + 3, 0, 0, 0, 5, 0};   // an empty object may say anything
        off += (size + 15) & ~15ull;
        if (flavour == 1) off += 4096 * (rnd() % 3);
    }
    if (flavour == 2)   // any order
        for (uint64_t k = n; k > 1; --k) {
            const uint64_t j = rnd() % k;
            const s3dg_obj_desc t = d[k - 1];
            d[k - 1] = d[j];
            d[j] = t;
        }
    return d;
}

int main() {
    // the pointer arguments, in their order
    static const s3dg_obj_desc one = {0, 1, 0, 1, 0, 1};
    alignas(16) static uint8_t buf[32];
    int dummy;
    CHECK(!strcmp(verify_batch_args(buf, &one, 1, nullptr), "null output"));
    CHECK(!strcmp(verify_batch_args(nullptr, nullptr, 0, nullptr), "null output"));
    CHECK(verify_batch_args(nullptr, nullptr, 0, &dummy) == nullptr);        // n == 0: nothing else is looked at
    CHECK(!strcmp(verify_batch_args(buf, nullptr, 1, &dummy), "null descriptor array"));
    CHECK(!strcmp(verify_batch_args(nullptr, nullptr, 1, &dummy), "null descriptor array"));
    CHECK(!strcmp(verify_batch_args(nullptr, &one, 1, &dummy), "src_base must be 16-byte aligned"));
    CHECK(!strcmp(verify_batch_args(buf + 8, &one, 1, &dummy), "src_base must be 16-byte aligned"));
    CHECK(verify_batch_args(buf + 16, &one, 1, &dummy) == nullptr);

    unsigned long long arrays = 0;
    const uint64_t ns[] = {0, 1, 2, 7, 300, 5000, 16383, 16384, 16385, 49152, 49153, 60000};
    for (uint64_t n : ns)
        for (int flavour = 0; flavour < 4; ++flavour) {
            g_case = arrays++;
            check_good(make(n, flavour));
        }
    // one 2^31 - 1 block object is the largest allowed
    g_case = arrays++;
    {
        std::vector<s3dg_obj_desc> d = {{0, ((1ull << 31) - 1) * kBlk, 1, 1, 0, 1}};
        CHECK(verify_batch_check(d.data(), 1).msg == nullptr);
        CHECK(verify_obj_tiles(d[0].size, 6) == 1ull << 25);
    }

    // refusals: each rule at each place of an array, the first offending descriptor names it,
    // and the text is the fill's (batch_scan over the same array)
    struct Bad {
        const char *msg;
        s3dg_obj_desc d;
    };
    const Bad bads[] = {
        {"dst_off must be a multiple of 16", {8, 100, 1, 1, 0, 1}},
        {"dst_off must be a multiple of 16", {4097, 4096, 1, 1, 1, 2}},
        {"need f_num < f_den", {0, 100, 1, 1, 3, 3}},
        {"need f_num < f_den", {0, 100, 1, 1, 4, 3}},
        {"need f_num < f_den", {0, 100, 1, 1, 0, 0}},      // the random-data layout
        {"object larger than 2^31 blocks", {0, (1ull << 31) * kBlk, 1, 1, 0, 1}},
        {"object larger than 2^31 blocks", {0, (1ull << 31) * kBlk - 4095, 1, 1, 0, 1}},
        {"dst_off must be a multiple of 16", {8, 100, 1, 1, 3, 3}},             // two rules broken: the fill's order
        {"need f_num < f_den", {16, (1ull << 31) * kBlk, 1, 1, 0, 0}},
    };
    for (const Bad &b : bads)
        for (uint64_t n : {(uint64_t)1, (uint64_t)5, (uint64_t)20000})
            for (uint64_t at : {(uint64_t)0, n / 2, n - 1}) {
                g_case = arrays++;
                std::vector<s3dg_obj_desc> d = make(n, 1);
                d[at] = b.d;
                const VerifyBatchCheck C = verify_batch_check(d.data(), n);
                CHECK(C.msg && !strcmp(C.msg, b.msg) && C.bad == at);
                // a second offender behind it changes nothing
                if (at + 1 < n) {
                    d[n - 1] = bads[(&b - bads + 3) % 9].d;
                    const VerifyBatchCheck C2 = verify_batch_check(d.data(), n);
                    CHECK(C2.msg && !strcmp(C2.msg, b.msg) && C2.bad == at);
                }
                std::vector<s3dg_obj_desc> st(n);
                BatchScan P;
                batch_scan(d.data(), 0, n, 0, P, st.data(), 0);
                CHECK(P.err == S3DG_EINVAL && P.msg && !strcmp(P.msg, b.msg));
            }
    printf("arrays %llu\n", arrays);
    printf("refusal: %s\n", verify_batch_args(buf, &one, 1, nullptr));
    printf("refusal: %s\n", verify_batch_args(buf, nullptr, 1, &dummy));
    printf("refusal: %s\n", verify_batch_args(nullptr, &one, 1, &dummy));
    for (int k : {0, 2, 5}) printf("refusal: %s\n", verify_desc_check(bads[k].d));
    return 0;
}
