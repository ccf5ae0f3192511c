// The uniform keystream launches' plan (csrc/s3dg_ks_plan.h) as a table, one
// line per case: tests/test_ks_plan_cpu.py holds the restatement of
// tests/keystream_cases.py against it line by line.  g++ alone, no HIP.
#include <stdio.h>

#include <initializer_list>

#include "s3dg_ks_plan.h"

using namespace s3dg;
typedef unsigned long long ull;

int main() {
    const uint64_t MIB = 1ull << 20;
    const uint64_t chunks[] = {128, 2176, 4096, 65664, MIB - 128, MIB, 2 * MIB + 128, 4202496, 16 * MIB, 64 * MIB};
    const uint64_t knobs[] = {0, 64, 256, 512, 2048, 4096, 131072};
    const uint64_t ncs[] = {1, 3, 33, 700, 1ull << 20};
    const uint64_t cuss[] = {1, 256, 304};
    const uint64_t Ds[] = {16, 32, 64};
    // K2 lanes
    for (uint64_t cb : chunks)
        for (uint64_t knob : knobs)
            for (uint64_t nc : ncs)
                for (uint64_t cus : cuss)
                    for (uint64_t D : Ds) {
                        const KsLanes L = ks_lanes(0, cb, nc, false, 0, knob ? knob : kDefaultKsMinDraws[0], D, cus);
                        printf("lanes 0 %llu %llu 0 0 %llu %llu %llu %u %llu %d\n", (ull)cb, (ull)nc, (ull)knob,
                               (ull)D, (ull)cus, L.lpc, (ull)L.span, (int)L.ok);
                    }
    // DG1 lanes: the prefix inside the lanes, and the tails of a split
    const uint32_t ratios[][2] = {{0, 1}, {1, 2}, {2, 3}, {1, 3}, {6, 7}, {19, 20}, {99, 100}, {127, 128}, {65534, 65535}};
    for (auto &r : ratios)
        for (uint64_t knob : knobs)
            for (uint64_t nc : ncs)
                for (uint64_t cus : cuss)
                    for (uint64_t D : Ds)
                        for (int split = 0; split < 2; ++split) {
                            const KsDgenCall P = ks_dgen_call(nc * MIB, 1, 0, nc, r[0], r[1], split);
                            const KsLanes L = ks_lanes(1, MIB, nc, r[0] > 0 && !P.zsplit, P.z0,
                                                       knob ? knob : kDefaultKsMinDraws[1], D, cus);
                            printf("lanes 1 %llu %llu %d %llu %llu %llu %llu %u %llu %d\n", (ull)MIB, (ull)nc,
                                   (int)(r[0] > 0 && !P.zsplit), (ull)P.z0, (ull)knob, (ull)D, (ull)cus, L.lpc,
                                   (ull)L.span, (int)L.ok);
                        }
    // regions
    const uint64_t z0s[] = {0, 87040, 129536};
    for (uint64_t z0 : z0s)
        for (uint32_t span : {272u, 320u, 352u, 384u, 2048u})
            for (uint64_t clen : {(uint64_t)1, (uint64_t)65664, MIB - 3, MIB})
                for (uint32_t sub : {0u, 1u, 2u, 30u, 31u, 63u, 125u, 127u, 255u, 1023u}) {
                    const KsRegion R = ks_lane_region(clen, z0, span, sub);
                    printf("region %llu %llu %u %u %llu %u\n", (ull)clen, (ull)z0, span, sub, (ull)R.rb, R.rlen);
                }
    // the DG1 call
    for (uint64_t size : {MIB, 2 * MIB, 2 * MIB + 5, 5 * MIB, 5 * MIB + 4095, 64 * MIB, 65 * MIB + 1})
        for (uint64_t n_objs : {(uint64_t)1, (uint64_t)3})
            for (auto &r : ratios)
                for (uint64_t split : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)64}) {
                    const uint64_t nb = (size + MIB - 1) / MIB;
                    for (uint64_t lo : {(uint64_t)0, (uint64_t)1})
                        for (uint64_t hi : {nb, nb - 1}) {
                            if (lo >= hi) continue;
                            const KsDgenCall P = ks_dgen_call(size, n_objs, lo, hi, r[0], r[1], split);
                            printf("call %llu %llu %llu %llu %u %u %llu %u %d %d %llu %llu\n", (ull)size, (ull)n_objs,
                                   (ull)lo, (ull)hi, r[0], r[1], (ull)split, P.zw, (int)P.cut_last, (int)P.zsplit,
                                   (ull)P.nchunks, (ull)P.z0);
                        }
                }
    // the half-length tail set
    for (int64_t tail : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)3, (int64_t)32, (int64_t)1000})
        for (uint64_t res : {(uint64_t)0, (uint64_t)1, (uint64_t)8})
            for (uint64_t cus : cuss)
                for (uint32_t waves : {1u, 4u})
                    for (uint32_t D : {16u, 32u, 64u})
                        for (uint64_t n_objs : {(uint64_t)1, (uint64_t)2})
                            for (uint64_t nc : {(uint64_t)7, (uint64_t)24, (uint64_t)256, (uint64_t)6145})
                                for (uint32_t lpc : {32u, 64u, 256u, 512u, 1024u})
                                    for (uint32_t span : {352u, 512u, 544u, 2048u}) {
                                        const KsHalfTail H = ks_half_tail(tail, res, cus, waves, D, n_objs, nc, 5, lpc, span);
                                        printf("tail %lld %llu %llu %u %u %llu %llu %u %u %d %llu %u %u %llu %llu %llu %llu %llu\n",
                                               (long long)tail, (ull)res, (ull)cus, waves, D, (ull)n_objs, (ull)nc, lpc,
                                               span, (int)H.take, (ull)H.T, H.lpc2, H.span2, (ull)H.chunk0_2,
                                               (ull)H.doff, (ull)H.cpo2, (ull)H.nchunks1, (ull)H.cpo1);
                                    }
    // grids
    for (uint64_t nc : {(uint64_t)1, (uint64_t)3, (uint64_t)33, (uint64_t)257, (uint64_t)1 << 20, (uint64_t)1 << 40})
        for (uint32_t lpc : {1u, 2u, 32u, 64u, 512u, 1024u})
            for (int waves : {1, 2, 4})
                for (int xcd : {1, 4, 16, 32, 4096}) {
                    const KsGrid G = ks_static_grid(nc, lpc, waves, xcd);
                    printf("grid %llu %u %d %d %llu %u %u\n", (ull)nc, lpc, waves, xcd, (ull)G.wgs, G.nwg, G.xg);
                }
    for (uint64_t wgs : {(uint64_t)7, (uint64_t)255, (uint64_t)256, (uint64_t)1535, (uint64_t)1536, (uint64_t)100000})
        for (uint64_t wgs2 : {(uint64_t)0, (uint64_t)1, (uint64_t)64})
            for (int rounds : {-1, 0, 1, 3, 6})
                for (uint64_t res : {(uint64_t)0, (uint64_t)1, (uint64_t)3, (uint64_t)8})
                    for (uint64_t cus : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)8, (uint64_t)256, (uint64_t)304})
                        for (int waves : {1, 2, 4})
                            printf("persist %llu %llu %d %llu %llu %d %llu\n", (ull)wgs, (ull)wgs2, rounds, (ull)res,
                                   (ull)cus, waves, (ull)ks_persistent_grid(wgs, wgs2, rounds, res, cus, waves));
    for (uint32_t xg : {1u, 2u, 4u, 16u})
        for (uint32_t nwg : {1u, 7u, 8u, 33u, 64u, 129u, 300u})
            for (uint64_t b = 0; b < nwg; ++b) printf("remap %u %u %llu %llu\n", xg, nwg, (ull)b, (ull)ks_remap(xg, nwg, b));
    for (uint32_t nwg : {0u, 1u, 7u, 8u, 9u, 33u, 0x7FFFFFFFu})
        for (uint32_t v = 0; v < 8; ++v)
            for (uint32_t W : {1u, 2u, 4u}) printf("quota %u %u %u %llu\n", nwg, v, W, (ull)ks_queue_quota(nwg, v, W));
    for (uint32_t U : {1u, 3u, 65537u, 0xFFFFFFFFu})
        for (uint32_t a : {0u, 1u, 2u, 65536u, 65537u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu})
            printf("fastmod %u %u %llu %u\n", a, U, (ull)fastmod_magic(U), fastmod(a, fastmod_magic(U), U));
    return 0;
}
