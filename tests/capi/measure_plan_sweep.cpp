// The measure plan (csrc/s3dg_measure_plan.h) over a sweep of its inputs, with
// g++ alone: sizes around every 16 B, 4 KiB and block_bytes edge, and the
// sub-launch splits.  Every property is asserted here (exit status 1 and a
// line on stderr at the first failure); stdout carries the number of plans
// checked and the refusal texts, which tests/test_measure_cpu.py compares
// with what the C calls say.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "s3dg_measure_plan.h"

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

static void check_plan(const MeasurePlan &P, uint64_t len, uint64_t n, uint64_t bb) {
    g_len = len, g_n = n, g_bb = bb;
    CHECK(P.n_objs == n && P.len == len);
    CHECK(P.gpb == bb / 4096);
    // blocks and granules sum to the object
    CHECK(P.bpo >= 1 && (P.bpo - 1) * bb + P.last_block == len);
    CHECK(P.gpo >= 1 && (P.gpo - 1) * 4096 + P.last_granule == len);
    CHECK(P.last_block > 0 && P.last_block <= bb);
    CHECK(P.last_granule > 0 && P.last_granule <= 4096);
    // every full block holds gpb granules; the last one what is left
    CHECK((P.bpo - 1) * P.gpb + (P.last_block + 4095) / 4096 == P.gpo);
    CHECK(P.slots == n * P.bpo && P.records == n * P.gpo && P.bytes == n * len);
    // the sub-launches tile objects x granules exactly, within the grid limits
    uint64_t cells = 0, xsum = 0;
    for (uint64_t iy = 0; iy < P.ny; ++iy)
        for (uint64_t ix = 0; ix < P.nx; ++ix) {
            uint64_t x0, y0;
            uint32_t gx, gy;
            measure_sub_launch(P, ix, iy, &x0, &gx, &y0, &gy);
            CHECK(gx >= 1 && gx <= kMeasureMaxGridX && gy >= 1 && gy <= kMeasureMaxGridY);
            CHECK(x0 == ix * kMeasureMaxGridX && y0 == iy * kMeasureMaxGridY);
            CHECK(x0 + gx <= P.gpo && y0 + gy <= n);
            CHECK(ix + 1 < P.nx ? gx == kMeasureMaxGridX : x0 + gx == P.gpo);
            CHECK(iy + 1 < P.ny ? gy == kMeasureMaxGridY : y0 + gy == n);
            cells += (uint64_t)gx * gy;
            if (iy == 0) xsum += gx;
        }
    CHECK(cells == P.records && xsum == P.gpo);
    CHECK(measure_record_bytes(P.records) == P.records * 20);
    CHECK(measure_record_zero_offset(P.records) % 16 == 0);
}

int main() {
    const uint64_t bbs[] = {4096, 8192, 12288, 65536, 1ull << 20, 1ull << 30};
    const uint64_t ns[] = {1, 2, 5, 65534, 65535, 65536, 65537, 2 * 65535, 2 * 65535 + 1};
    unsigned long long plans = 0;
    for (uint64_t bb : bbs) {
        std::vector<uint64_t> lens;
        const uint64_t edges[] = {16, 4096, 8192, bb, 2 * bb, 3 * bb + 4096, kMeasureMaxGridX * 4096,
                                  2 * kMeasureMaxGridX * 4096};
        for (uint64_t e : edges)
            for (int64_t d : {-17, -16, -15, -1, 0, 1, 15, 16, 17, 4095, 4097})
                if ((int64_t)e + d > 0) lens.push_back(e + d);
        for (uint64_t len : lens)
            for (uint64_t n : ns) {
                MeasurePlan P;
                const uint64_t stride = (len + 15) / 16 * 16 + 4096;
                g_len = len, g_n = n, g_bb = bb;
                CHECK(measure_plan_stream(&P, 0x10000, len, stride, n, bb) == nullptr);
                check_plan(P, len, n, bb);
                ++plans;
            }
        // ranges: every cut of an object's blocks into [lo, hi) sums to the object
        for (uint64_t len : lens) {
            const uint64_t nb = (len + bb - 1) / bb;
            const uint64_t cuts[] = {0, nb / 3, nb / 3 + 1, nb - 1, nb, nb + 7};
            uint64_t bytes = 0, slots = 0, prev = 0;
            for (uint64_t c : cuts) {
                if (c < prev) continue;
                MeasurePlan P;
                g_len = len, g_n = 1, g_bb = bb;
                CHECK(measure_plan_range(&P, 0x10000, len, prev, c, bb) == nullptr);
                const uint64_t hi = c < nb ? c : nb;
                if (prev >= hi) {
                    CHECK(P.n_objs == 0 && P.slots == 0 && P.bytes == 0);
                } else {
                    check_plan(P, P.len, 1, bb);
                    CHECK(P.skip == prev * bb && P.slots == hi - prev);
                    CHECK(P.len == (hi == nb ? len : hi * bb) - prev * bb);
                    bytes += P.bytes;
                    slots += P.slots;
                    ++plans;
                }
                prev = c;
            }
            CHECK(bytes == len && slots == nb);
        }
    }
    // the refusals, in the C calls' words
    MeasurePlan P;
    g_len = g_n = g_bb = 0;
    for (uint64_t bb : {0ull, 4095ull, 6000ull, 1ull << 31, (1ull << 30) + 4096}) {
        CHECK(measure_block_bytes_check(bb) != nullptr);
        CHECK(measure_plan_stream(&P, 0x10000, 4096, 4096, 1, bb) != nullptr);
        CHECK(measure_plan_range(&P, 0x10000, 4096, 0, 1, bb) != nullptr);
    }
    CHECK(measure_block_bytes_check(4096) == nullptr && measure_block_bytes_check(1ull << 30) == nullptr);
    printf("block_bytes|%s\n", measure_block_bytes_check(6000));
    CHECK(measure_plan_stream(&P, 0x10008, 4096, 4096, 2, 4096) != nullptr);     // misaligned src
    CHECK(measure_plan_stream(&P, 0, 4096, 4096, 2, 4096) != nullptr);           // null src
    CHECK(measure_plan_stream(&P, 0x10000, 4096, 4104, 2, 4096) != nullptr);     // misaligned stride
    printf("align|%s\n", measure_plan_stream(&P, 0x10008, 4096, 4096, 2, 4096));
    CHECK(measure_plan_stream(&P, 0x10000, 8192, 4096, 2, 4096) != nullptr);     // overlap
    printf("overlap|%s\n", measure_plan_stream(&P, 0x10000, 8192, 4096, 2, 4096));
    CHECK(measure_plan_stream(&P, 0x10000, 8192, 0, 1, 4096) == nullptr);        // one object: any stride
    CHECK(measure_plan_stream(&P, 0, 0, 0, 5, 4096) == nullptr && P.n_objs == 0);   // empty adds: any pointer
    CHECK(measure_plan_stream(&P, 8, 4096, 4096, 0, 4096) == nullptr && P.n_objs == 0);
    CHECK(measure_plan_range(&P, 0x10004, 4096, 0, 1, 4096) != nullptr);
    CHECK(measure_plan_range(&P, 0, 4096, 1, 1, 4096) == nullptr && P.n_objs == 0);
    CHECK(measure_plan_stream(&P, 0x10000, (1ull << 44) + 1, 1ull << 45, 1, 4096) != nullptr);   // > 2^32 granules
    CHECK(measure_plan_stream(&P, 0x10000, 4096, 4096, (1ull << 40) + 1, 4096) != nullptr);
    // the distinct count's scratch and the array's growth
    for (uint64_t n : {1ull, 31ull, 32ull, 33ull, 65536ull, 1000003ull}) {
        CHECK(measure_sort_array_bytes(n) >= n * 8 && measure_sort_array_bytes(n) % 256 == 0);
        CHECK(measure_sort_bytes(n) == 4 * measure_sort_array_bytes(n));
    }
    CHECK(measure_grow_cap(0, 1) == kMeasureMinCap && measure_grow_cap(4096, 4097) == 8192);
    CHECK(measure_grow_cap(8192, 65536) == 65536 && measure_grow_cap(8192, 65537) == 131072);
    printf("plans|%llu\n", plans);
    return 0;
}
