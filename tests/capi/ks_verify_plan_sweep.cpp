// The keystream verify launch's lane plan over a sweep of its inputs, one line
// per point: "chunk_bytes nchunks cus min_lane_draws lpc span".  Compiled with
// g++ against s3dg_ks_verify_plan.h alone (tests/test_verify_keystream_cpu.py).
#include <cinttypes>
#include <cstdio>
#include <initializer_list>

#include "s3dg_ks_verify_plan.h"

int main() {
    const uint64_t knobs[] = {0, 64, 512, 513, 1024, 2048, 4096, 8192, 65536, 1ull << 18, 1ull << 40};
    const uint32_t cus[] = {1, 64, 256, 304};
    for (uint64_t chunk = 4096; chunk <= (2ull << 20); chunk *= 2)
        for (uint64_t extra : {0ull, 4096ull})   // powers of two and one granule more
            for (uint64_t nchunks = 1; nchunks <= (1ull << 20); nchunks *= 4)
                for (uint32_t cu : cus)
                    for (uint64_t knob : knobs) {
                        const uint64_t cb = chunk + extra;
                        const s3dg::KsVerifyPlan p = s3dg::ks_verify_plan(cb, nchunks, cu, knob);
                        printf("%" PRIu64 " %" PRIu64 " %u %" PRIu64 " %u %" PRIu64 "\n", cb, nchunks, cu, knob, p.lpc,
                               p.span);
                    }
    return 0;
}
