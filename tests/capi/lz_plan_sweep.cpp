// The LZ plan (csrc/s3dg_lz_plan.h) over a sweep of its inputs, with g++ alone:
// sizes around every 16 B, 4 KiB and block_bytes edge, ranges, the grid and
// the LDS sizes.  Every property is asserted here (exit status 1 and a line on
// stderr at the first failure); stdout carries the number of plans checked and
// the refusal texts, which tests/test_lz_cpu.py compares with what the C calls
// say.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "s3dg_lz_plan.h"

using namespace s3dg;

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            fprintf(stderr, "%s:%d: %s  (len %llu n %llu bb %llu)\n", __FILE__, __LINE__, #cond, \
                    (unsigned long long)g_len, (unsigned long long)g_n, (unsigned long long)g_bb); \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

static uint64_t g_len, g_n, g_bb;

static void check_plan(const LzPlan &P, uint64_t len, uint64_t n, uint64_t bb) {
    g_len = len, g_n = n, g_bb = bb;
    CHECK(P.n_objs == n && P.len == len);
    // blocks sum to the object; the last one is never empty
    CHECK(P.bpo >= 1 && (P.bpo - 1) * bb + P.last_block == len);
    CHECK(P.last_block > 0 && P.last_block <= bb);
    CHECK(P.blocks == n * P.bpo);
    // the last byte a wave may read lies inside the last object
    const uint64_t i = P.blocks - 1, j = i / P.bpo, b = i - j * P.bpo;
    CHECK(j == n - 1 && b == P.bpo - 1 && b * bb + P.last_block == len);
    for (int cus : {0, 1, 8, 256, 304}) {
        const uint64_t g = lz_grid(P.blocks, bb, cus);
        CHECK(g >= 1 && g <= P.blocks && g <= kLzMaxGrid);
        CHECK(g <= (uint64_t)(cus > 0 ? cus : 256) * lz_waves_per_cu(bb));
        CHECK(g == P.blocks || g == (uint64_t)(cus > 0 ? cus : 256) * lz_waves_per_cu(bb));
    }
}

int main() {
    unsigned long long plans = 0;
    const uint64_t ns[] = {1, 2, 5, 65534, 65535, 65536, 65537, 65538, 2 * 65535 + 1};
    for (uint64_t bb = 4096; bb <= 65536; bb += 4096) {
        g_bb = bb;
        CHECK(lz_block_bytes_check(bb) == nullptr);
        // the block and the table fit a CU's LDS, as many times as the plan says
        CHECK(lz_lds_bytes(bb) == bb + 8192 && lz_lds_bytes(bb) % 16 == 0);
        const uint64_t w = lz_waves_per_cu(bb);
        CHECK(w >= 1 && w <= 32 && w * lz_lds_bytes(bb) <= kLzCuLds && (w == 32 || (w + 1) * lz_lds_bytes(bb) > kLzCuLds));
        // whole blocks per host chunk, within the staging chunk
        const uint64_t per = lz_host_chunk_blocks(bb);
        CHECK(per >= 1 && per * bb <= kLzHostChunk && (per + 1) * bb > kLzHostChunk);
        std::vector<uint64_t> lens;
        const uint64_t edges[] = {16, 4096, 8192, bb, 2 * bb, 3 * bb + 4096, (1ull << 22) * bb, (1ull << 32), (1ull << 32) + bb};
        for (uint64_t e : edges)
            for (int64_t d : {-17, -16, -15, -1, 0, 1, 15, 16, 17, 4095, 4097})
                if ((int64_t)e + d > 0) lens.push_back(e + d);
        for (uint64_t len : lens)
            for (uint64_t n : ns) {
                LzPlan P;
                const uint64_t stride = (len + 15) / 16 * 16 + 4096;
                g_len = len, g_n = n;
                CHECK(lz_plan_stream(&P, 0x10000, len, stride, n, bb) == nullptr);
                check_plan(P, len, n, bb);
                ++plans;
            }
        // ranges: every cut of an object's blocks into [lo, hi) sums to the object
        for (uint64_t len : lens) {
            const uint64_t nb = (len + bb - 1) / bb;
            const uint64_t cuts[] = {0, nb / 3, nb / 3 + 1, nb - 1, nb, nb + 7};
            uint64_t bytes = 0, blocks = 0, prev = 0;
            for (uint64_t c : cuts) {
                if (c < prev) continue;
                LzPlan P;
                g_len = len, g_n = 1;
                CHECK(lz_plan_range(&P, 0x10000, len, prev, c, bb) == nullptr);
                const uint64_t hi = c < nb ? c : nb;
                if (prev >= hi) {
                    CHECK(P.n_objs == 0 && P.blocks == 0 && P.len == 0);
                } else {
                    check_plan(P, P.len, 1, bb);
                    CHECK(P.blocks == hi - prev);
                    CHECK(P.len == (hi == nb ? len : hi * bb) - prev * bb);
                    bytes += P.len;
                    blocks += P.blocks;
                    ++plans;
                }
                prev = c;
            }
            CHECK(bytes == len && blocks == nb);
        }
    }
    CHECK(lz_waves_per_cu(4096) == 13 && lz_waves_per_cu(65536) == 2);
    // the refusals, in the C calls' words
    LzPlan P;
    g_len = g_n = g_bb = 0;
    for (uint64_t bb : {0ull, 4095ull, 8191ull, 69632ull, 131072ull, 1ull << 31}) {
        CHECK(lz_block_bytes_check(bb) != nullptr);
        CHECK(lz_plan_stream(&P, 0x10000, 4096, 4096, 1, bb) != nullptr);
        CHECK(lz_plan_range(&P, 0x10000, 4096, 0, 1, bb) != nullptr);
    }
    printf("block_bytes|%s\n", lz_block_bytes_check(8191));
    CHECK(lz_plan_stream(&P, 0x10008, 4096, 4096, 2, 4096) != nullptr);     // misaligned src
    CHECK(lz_plan_stream(&P, 0, 4096, 4096, 2, 4096) != nullptr);           // null src
    CHECK(lz_plan_stream(&P, 0x10000, 4096, 4104, 2, 4096) != nullptr);     // misaligned stride
    printf("align|%s\n", lz_plan_stream(&P, 0x10008, 4096, 4096, 2, 4096));
    CHECK(lz_plan_stream(&P, 0x10000, 8192, 4096, 2, 4096) != nullptr);     // overlap
    printf("overlap|%s\n", lz_plan_stream(&P, 0x10000, 8192, 4096, 2, 4096));
    CHECK(lz_plan_stream(&P, 0x10000, 8192, 0, 1, 4096) == nullptr);        // one object: any stride
    CHECK(lz_plan_stream(&P, 0, 0, 0, 5, 4096) == nullptr && P.n_objs == 0);   // empty adds: any pointer
    CHECK(lz_plan_stream(&P, 8, 4096, 4096, 0, 4096) == nullptr && P.n_objs == 0);
    CHECK(lz_plan_range(&P, 0x10004, 4096, 0, 1, 4096) != nullptr);
    printf("range_align|%s\n", lz_plan_range(&P, 0x10004, 4096, 0, 1, 4096));
    CHECK(lz_plan_range(&P, 0, 4096, 1, 1, 4096) == nullptr && P.n_objs == 0);
    CHECK(lz_plan_stream(&P, 0x10000, (1ull << 56) + 1, 1ull << 57, 1, 4096) != nullptr);
    CHECK(lz_plan_stream(&P, 0x10000, 4096, 4096, (1ull << 40) + 1, 4096) != nullptr);
    printf("blocks|%s\n", lz_plan_stream(&P, 0x10000, 4096, 4096, (1ull << 40) + 1, 4096));
    printf("plans|%llu\n", plans);
    return 0;
}
