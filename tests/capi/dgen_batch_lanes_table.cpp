// Stand-alone table of s3dg_dgen_batch_plan.h's size classes, lane plans and
// lane regions (g++ alone, no HIP), one line per case, for
// tests/test_dgen_batch_cpu.py to hold against the Python restatement in
// tests/dgen_batch_cases.py:
//   class  <len> <class> <ceiling>
//   lanes  <class> <knob> <zeros> <draws> <verify> <nchunks> <cus> <lpc> <span>
//   region <len> <span> <sub> <rb> <rlen>
// The order of the lines is part of the table.
#include <stdio.h>

#include "s3dg_dgen_batch_plan.h"

using namespace s3dg;

typedef unsigned long long ull;

int main() {
    const uint64_t MiB = 1ull << 20;
    const uint64_t knobs[] = {0, 512, 4096, 131072};
    for (uint64_t len : {(uint64_t)1, (uint64_t)2, MiB, MiB + 1, 5 * MiB})
        printf("class %llu %u %llu\n", (ull)len, dgen_chunk_class(len), (ull)dgen_class_ceiling(dgen_chunk_class(len)));
    for (uint32_t cls = 0; cls < kDgbFull; ++cls) {
        const uint64_t C = (uint64_t)4096 << cls;
        for (uint64_t len : {C / 2, C / 2 + 1, C - 1, C, C + 1})
            printf("class %llu %u %llu\n", (ull)len, dgen_chunk_class(len),
                   (ull)dgen_class_ceiling(dgen_chunk_class(len)));
    }
    for (uint32_t cls = 0; cls < kDgbClasses; ++cls)
        for (uint64_t knob : knobs)
            for (int zeros = 0; zeros < 2; ++zeros)
                for (uint32_t draws : {16u, 32u, 64u})
                    for (int verify = 0; verify < 2; ++verify)
                        for (uint64_t nchunks : {1ull, 67ull, 20000ull})
                            for (uint32_t cus : {1u, 256u, 304u}) {
                                const DgenLanes L = dgen_class_lanes(dgen_class_ceiling(cls), nchunks, cus, knob,
                                                                     zeros != 0, draws, verify != 0);
                                printf("lanes %u %llu %d %u %d %llu %u %u %llu\n", cls, (ull)knob, zeros, draws, verify,
                                       (ull)nchunks, cus, L.lpc, (ull)L.span);
                            }
    // every lane's region of a few lengths per class, at the lanes of each knob
    // (the fill's at 16-draw stages and the verify's)
    for (uint32_t cls = 0; cls < kDgbClasses; ++cls) {
        const uint64_t C = dgen_class_ceiling(cls), lo = cls == 0 || cls == kDgbFull ? 0 : C / 2;
        for (uint64_t knob : knobs)
            for (int verify = 0; verify < 2; ++verify) {
                const DgenLanes L = dgen_class_lanes(C, 67, 256, knob, false, 16, verify != 0);
                for (uint64_t len : {lo + 1, lo + 17, (lo + C) / 2 + 5, C - 1, C}) {
                    if (cls == kDgbFull && len != C) continue;
                    for (uint32_t sub = 0; sub < L.lpc; ++sub) {
                        const DgenRegion G = dgen_lane_region(len, L.span, sub);
                        printf("region %llu %llu %u %llu %llu\n", (ull)len, (ull)L.span, sub, (ull)G.rb, (ull)G.rlen);
                    }
                }
            }
    }
    return 0;
}
