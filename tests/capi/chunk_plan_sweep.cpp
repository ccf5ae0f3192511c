// The chunk plan (csrc/s3dg_chunk_plan.h) over a sweep of its inputs, with g++
// alone: parameters around every limit, sizes around every 16 B, 64 B, 4 KiB
// and min_bytes edge, and the sub-launch splits.  Every property is asserted
// here (exit status 1 and a line on stderr at the first failure); stdout
// carries the number of plans checked and the refusal texts, which
// tests/test_chunks_cpu.py compares with what the C calls say.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "s3dg_chunk_plan.h"

using namespace s3dg;

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "%s:%d: %s  (len %llu n %llu min %llu)\n", __FILE__, __LINE__, #cond, \
                    (unsigned long long)g_len, (unsigned long long)g_n, (unsigned long long)g_min); \
            exit(1);                                                                             \
        }                                                                                        \
    } while (0)

static uint64_t g_len, g_n, g_min;

static void check_plan(const ChunkPlan &P, uint64_t len, uint64_t n, uint64_t mn) {
    g_len = len, g_n = n, g_min = mn;
    CHECK(P.n_objs == n && P.len == len);
    CHECK(P.gpo >= 1 && (P.gpo - 1) * 4096 < len && len <= P.gpo * 4096);
    CHECK(P.wpo == P.gpo * 64 && P.wpo * 64 >= len);                 // a bit per byte
    // the most chunks an object can have: all but the last hold min_bytes or more
    CHECK((P.rpo - 1) * mn >= len && (P.rpo - 2) * mn < len);
    CHECK(P.slots == n * P.rpo && P.slots <= kChunkMaxSlots);
    CHECK(P.bytes == n * len && P.granules == n * P.gpo);
    // the scratch regions follow each other without overlap, each aligned for its element
    CHECK(P.off_offset == P.granules * 512 && P.off_offset % 256 == 0);
    CHECK(P.len_offset >= P.off_offset + P.slots * 8 && P.len_offset % 256 == 0);
    CHECK(P.cnt_offset >= P.len_offset + P.slots * 4 && P.cnt_offset % 256 == 0);
    CHECK(P.gcnt_offset >= P.cnt_offset + n * 4 && P.gcnt_offset % 256 == 0);
    CHECK(P.scratch_bytes >= P.gcnt_offset + P.granules * 4);
    CHECK(P.scratch_bytes <= P.granules * 516 + P.slots * 12 + n * 4 + 4 * 256);
    // the sub-launches tile objects x granules exactly, within the grid limits
    uint64_t cells = 0, xsum = 0;
    for (uint64_t iy = 0; iy < P.ny; ++iy)
        for (uint64_t ix = 0; ix < P.nx; ++ix) {
            uint64_t x0, y0;
            uint32_t gx, gy;
            chunk_sub_launch(P, ix, iy, &x0, &gx, &y0, &gy);
            CHECK(gx >= 1 && gx <= kMeasureMaxGridX && gy >= 1 && gy <= kMeasureMaxGridY);
            CHECK(x0 == ix * kMeasureMaxGridX && y0 == iy * kMeasureMaxGridY);
            CHECK(x0 + gx <= P.gpo && y0 + gy <= n);
            CHECK(ix + 1 < P.nx ? gx == kMeasureMaxGridX : x0 + gx == P.gpo);
            CHECK(iy + 1 < P.ny ? gy == kMeasureMaxGridY : y0 + gy == n);
            cells += (uint64_t)gx * gy;
            if (iy == 0) xsum += gx;
        }
    CHECK(cells == P.granules && xsum == P.gpo);
}

int main() {
    unsigned long long plans = 0;
    g_len = g_n = g_min = 0;
    // ---- the parameters ----
    uint32_t bits = 99;
    for (uint32_t b = 6; b <= 24; ++b) {
        CHECK(chunk_params_check(32, 1ull << b, 1ull << 30, &bits) == nullptr && bits == b);
        CHECK(chunk_params_check(32, (1ull << b) + 1, 1ull << 30, &bits) != nullptr);
        CHECK(chunk_params_check(32, (1ull << b) - 1, 1ull << 30, &bits) != nullptr);
    }
    CHECK(chunk_params_check(2048, 8192, 65536, nullptr) == nullptr);
    CHECK(chunk_params_check(100, 128, 1000, &bits) == nullptr && bits == 7);
    CHECK(chunk_params_check(4096, 64, 4096, &bits) == nullptr && bits == 6);        // min == max: fixed blocks
    CHECK(chunk_params_check(1ull << 30, 1ull << 24, 1ull << 30, &bits) == nullptr && bits == 24);
    for (uint64_t avg : {0ull, 1ull, 32ull, 63ull, 96ull, 8000ull, 1ull << 25, 1ull << 40, ~0ull})
        CHECK(chunk_params_check(2048, avg, 65536, nullptr) != nullptr);
    for (uint64_t mn : {0ull, 1ull, 31ull}) CHECK(chunk_params_check(mn, 64, 256, nullptr) != nullptr);
    CHECK(chunk_params_check(257, 64, 256, nullptr) != nullptr);
    CHECK(chunk_params_check(~0ull, 64, 256, nullptr) != nullptr);
    CHECK(chunk_params_check(32, 64, (1ull << 30) + 1, nullptr) != nullptr);
    CHECK(chunk_params_check(32, 64, ~0ull, nullptr) != nullptr);
    printf("avg|%s\n", chunk_params_check(2048, 8000, 65536, nullptr));
    printf("min|%s\n", chunk_params_check(31, 64, 256, nullptr));
    printf("order|%s\n", chunk_params_check(300, 64, 256, nullptr));
    printf("max|%s\n", chunk_params_check(32, 64, (1ull << 30) + 1, nullptr));
    // ---- the plans ----
    const uint64_t mins[] = {32, 33, 100, 2048, 4096, 65536, 1ull << 30};
    const uint64_t ns[] = {1, 2, 5, 65534, 65535, 65536, 65537, 2 * 65535 + 1};
    for (uint64_t mn : mins) {
        std::vector<uint64_t> lens;
        const uint64_t edges[] = {16, 64, 4096, 8192, mn, 2 * mn, 3 * mn + 4096, kMeasureMaxGridX * 4096,
                                  2 * kMeasureMaxGridX * 4096};
        for (uint64_t e : edges)
            for (int64_t d : {-65, -17, -16, -15, -1, 0, 1, 15, 16, 17, 63, 64, 4095, 4097})
                if ((int64_t)e + d > 0) lens.push_back(e + d);
        for (uint64_t len : lens)
            for (uint64_t n : ns) {
                ChunkPlan P;
                const uint64_t stride = (len + 15) / 16 * 16 + 4096;
                g_len = len, g_n = n, g_min = mn;
                const char *w = chunk_plan_stream(&P, 0x10000, len, stride, n, mn);
                const uint64_t rpo = (len + mn - 1) / mn + 1;
                if (n > kChunkMaxSlots / rpo) {
                    CHECK(w != nullptr && P.n_objs == 0);          // too many slots: refused, nothing planned
                    continue;
                }
                CHECK(w == nullptr);
                check_plan(P, len, n, mn);
                ++plans;
            }
    }
    // ---- the refusals, in the C calls' words ----
    ChunkPlan P;
    g_len = g_n = g_min = 0;
    CHECK(chunk_plan_stream(&P, 0x10008, 4096, 4096, 2, 2048) != nullptr);     // misaligned src
    CHECK(chunk_plan_stream(&P, 0, 4096, 4096, 2, 2048) != nullptr);           // null src
    CHECK(chunk_plan_stream(&P, 0x10000, 4096, 4104, 2, 2048) != nullptr);     // misaligned stride
    printf("align|%s\n", chunk_plan_stream(&P, 0x10008, 4096, 4096, 2, 2048));
    CHECK(chunk_plan_stream(&P, 0x10000, 8192, 4096, 2, 2048) != nullptr);     // overlap
    printf("overlap|%s\n", chunk_plan_stream(&P, 0x10000, 8192, 4096, 2, 2048));
    CHECK(chunk_plan_stream(&P, 0x10000, 8192, 0, 1, 2048) == nullptr);        // one object: any stride
    CHECK(chunk_plan_stream(&P, 0, 0, 0, 5, 2048) == nullptr && P.n_objs == 0);   // empty adds: any pointer
    CHECK(chunk_plan_stream(&P, 8, 4096, 4096, 0, 2048) == nullptr && P.n_objs == 0);
    CHECK(chunk_plan_stream(&P, 0x10000, (1ull << 44) + 1, 1ull << 45, 1, 1ull << 30) != nullptr);   // > 2^32 granules
    CHECK(chunk_plan_stream(&P, 0x10000, 4096, 4096, (1ull << 40) + 1, 2048) != nullptr);
    CHECK(chunk_plan_stream(&P, 0x10000, 1ull << 36, 1ull << 36, 1, 32) != nullptr);                 // 2^31 slots
    printf("slots|%s\n", chunk_plan_stream(&P, 0x10000, 1ull << 36, 1ull << 36, 1, 32));
    CHECK(chunk_plan_stream(&P, 0x10000, 4096, 4096, 1, 31) != nullptr);
    // ---- the distinct count's scratch and the arrays' growth ----
    for (uint64_t n : {1ull, 31ull, 32ull, 33ull, 65536ull, 1000003ull, 0x7FFFFFFFull}) {
        CHECK(chunk_sort_key_bytes(n) >= n * 8 && chunk_sort_key_bytes(n) % 256 == 0);
        CHECK(chunk_sort_idx_bytes(n) >= n * 4 && chunk_sort_idx_bytes(n) % 256 == 0);
        CHECK(chunk_sort_bytes(n) == 2 * chunk_sort_key_bytes(n) + 2 * chunk_sort_idx_bytes(n));
    }
    CHECK(chunk_grow_cap(0, 1) == kMeasureMinCap && chunk_grow_cap(4096, 4097) == 8192);
    CHECK(chunk_grow_cap(8192, 65536) == 65536 && chunk_grow_cap(8192, 65537) == 131072);
    CHECK(chunk_grow_cap(1ull << 30, (1ull << 30) + 1) == kChunkMaxSlots);
    CHECK(chunk_grow_cap(1ull << 30, kChunkMaxSlots) == kChunkMaxSlots);
    printf("plans|%llu\n", plans);
    return 0;
}
