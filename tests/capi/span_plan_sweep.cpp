// What the analysis plans share (csrc/s3dg_span_plan.h), with g++ alone: the
// sub-launch split around both grid limits, the range clip, the span checks,
// the roundings and the arrays' growth.  Every property is asserted here (exit
// status 1 and a line on stderr at the first failure); stdout carries the
// number of splits checked (tests/test_span_plan_cpu.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "s3dg_span_plan.h"

using namespace s3dg;

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "%s:%d: %s  (a %llu b %llu)\n", __FILE__, __LINE__, #cond,             \
                    (unsigned long long)g_a, (unsigned long long)g_b);                           \
            exit(1);                                                                             \
        }                                                                                        \
    } while (0)

static uint64_t g_a, g_b;

// Every (granule, object) lies in exactly one sub-launch: the sub-launches
// are the product of a partition of [0, gpo) (which depends on ix alone) and
// one of [0, n_objs) (on iy alone), each piece within its grid limit.
static void check_split(uint64_t gpo, uint64_t n) {
    g_a = gpo, g_b = n;
    const uint64_t nx = span_nx(gpo), ny = span_ny(n);
    CHECK(nx >= 1 && ny >= 1);
    uint64_t ynext = 0, cells = 0;
    for (uint64_t iy = 0; iy < ny; ++iy) {
        uint64_t xnext = 0, y0 = 0;
        uint32_t gy = 0;
        for (uint64_t ix = 0; ix < nx; ++ix) {
            uint64_t x0, y;
            uint32_t gx, g;
            span_sub_launch(gpo, n, ix, iy, &x0, &gx, &y, &g);
            CHECK(gx >= 1 && gx <= kSpanMaxGridX && g >= 1 && g <= kSpanMaxGridY);
            CHECK(x0 == xnext);                          // the row's pieces follow each other
            if (ix == 0) y0 = y, gy = g;
            CHECK(y == y0 && g == gy && y == ynext);     // one object range per row
            uint64_t x1, y1;                             // the same piece of granules in row 0
            uint32_t gx1, gy1;
            span_sub_launch(gpo, n, ix, 0, &x1, &gx1, &y1, &gy1);
            CHECK(x1 == x0 && gx1 == gx);
            xnext = x0 + gx;
            cells += (uint64_t)gx * g;
        }
        CHECK(xnext == gpo);
        ynext = y0 + gy;
    }
    CHECK(ynext == n && cells == gpo * n);
}

int main() {
    unsigned long long splits = 0;
    const uint64_t gpos[] = {1, 2, kSpanMaxGridX - 1, kSpanMaxGridX, kSpanMaxGridX + 1, 2 * kSpanMaxGridX,
                             2 * kSpanMaxGridX + 1, 0xFFFFFFFFull};
    const uint64_t ns[] = {1, 2, kSpanMaxGridY - 1, kSpanMaxGridY, kSpanMaxGridY + 1, 2 * kSpanMaxGridY,
                           2 * kSpanMaxGridY + 1, 3 * kSpanMaxGridY + 7};
    for (uint64_t gpo : gpos)
        for (uint64_t n : ns) {
            check_split(gpo, n);
            ++splits;
        }
    g_a = g_b = 0;
    CHECK(span_nx(kSpanMaxGridX) == 1 && span_nx(kSpanMaxGridX + 1) == 2);
    CHECK(span_ny(kSpanMaxGridY) == 1 && span_ny(kSpanMaxGridY + 1) == 2);

    // the range clip: bytes [skip, skip + len) of the object
    uint64_t skip, len;
    const uint64_t bb = 8192, obj = 3 * bb + 100;   // four blocks, the last one ragged
    CHECK(span_clip(0x10000, obj, 0, 4, bb, &skip, &len) == nullptr && skip == 0 && len == obj);
    CHECK(span_clip(0x10000, obj, 1, 3, bb, &skip, &len) == nullptr && skip == bb && len == 2 * bb);
    CHECK(span_clip(0x10000, obj, 3, 4, bb, &skip, &len) == nullptr && skip == 3 * bb && len == 100);   // ragged
    CHECK(span_clip(0x10000, obj, 2, 4, bb, &skip, &len) == nullptr && skip == 2 * bb && len == bb + 100);
    // blk_hi beyond the object is clipped to it
    CHECK(span_clip(0x10000, obj, 2, 99, bb, &skip, &len) == nullptr && skip == 2 * bb && len == bb + 100);
    CHECK(span_clip(0x10000, obj, 0, ~0ull, bb, &skip, &len) == nullptr && skip == 0 && len == obj);
    CHECK(span_clip(0x10000, 3 * bb, 2, 3, bb, &skip, &len) == nullptr && skip == 2 * bb && len == bb);   // whole
    // empty ranges: accepted whatever the pointer
    CHECK(span_clip(0, obj, 2, 2, bb, &skip, &len) == nullptr && len == 0);
    CHECK(span_clip(8, obj, 3, 1, bb, &skip, &len) == nullptr && len == 0);
    CHECK(span_clip(0, obj, 4, 9, bb, &skip, &len) == nullptr && len == 0);      // lo at the clipped hi
    CHECK(span_clip(0, obj, 5, 9, bb, &skip, &len) == nullptr && len == 0);
    CHECK(span_clip(0, 0, 0, 1, bb, &skip, &len) == nullptr && len == 0);        // an empty object
    // the pointer counts only for a range that holds bytes
    const char *w = span_clip(0x10004, obj, 0, 1, bb, &skip, &len);
    CHECK(w != nullptr && strstr(w, "16-byte aligned") && len == 0);
    CHECK(span_clip(0, obj, 0, 1, bb, &skip, &len) != nullptr && len == 0);

    // the span checks
    CHECK(span_check(0x10000, 4096, 4096, 2) == nullptr);
    CHECK(span_check(0x10000, 8192, 0, 1) == nullptr);                   // one object: any aligned stride
    CHECK(strstr(span_check(0, 4096, 4096, 2), "16-byte aligned"));      // null
    CHECK(strstr(span_check(0x10008, 4096, 4096, 2), "16-byte aligned"));
    CHECK(strstr(span_check(0x10000, 4096, 4104, 2), "16-byte aligned"));
    CHECK(strstr(span_check(0x10000, 8192, 4096, 2), "overlap"));
    CHECK(span_check(0x10000, 4096, 4096, 1ull << 50) == nullptr);       // the counts' limits are the plans' own

    // roundings, growth, grids
    for (uint64_t n : {0ull, 1ull, 255ull, 256ull, 257ull, 8000024ull}) {
        g_a = n;
        CHECK(span_align256(n) >= n && span_align256(n) < n + 256 && span_align256(n) % 256 == 0);
        for (uint64_t u : {1ull, 32ull, 4096ull, 65536ull}) {
            g_b = u;
            const uint64_t q = span_ceil_div(n, u);
            CHECK(q * u >= n && (q == 0 ? n == 0 : (q - 1) * u < n));
        }
    }
    CHECK(span_ceil_div(~0ull, 4096) == (1ull << 52));                   // no overflow at the top
    CHECK(span_grow_cap(0, 1) == kSpanMinCap && span_grow_cap(4096, 4097) == 8192);
    CHECK(span_grow_cap(8192, 65536) == 65536 && span_grow_cap(8192, 65537) == 131072);
    CHECK(span_grow_cap(0, 0) == kSpanMinCap && span_grow_cap(1ull << 30, (1ull << 30) + 1) == 1ull << 31);
    CHECK(span_grid_for(0) == 1 && span_grid_for(1) == 1 && span_grid_for(256) == 1 && span_grid_for(257) == 2);
    CHECK(span_grid_for(2048 * 256) == 2048 && span_grid_for(2048 * 256 + 1) == 2048);
    CHECK(span_grid_for(~0ull - 255) == 2048);
    CHECK(kStagingChunk == 64ull << 20);
    printf("splits|%llu\n", splits);
    return 0;
}
