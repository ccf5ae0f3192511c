// s3dg_ks_verify_plan.h — the lane plan of a keystream verify launch
// (k_verify_keystream) as a pure function: no HIP, no context,
// so it can be compiled and tested on its own (tests/test_verify_keystream_cpu.py).
#pragma once
#include <stdint.h>

namespace s3dg {

// A verify lane covers whole 4 KiB granules: its draw count is a multiple of
// 512, so every granule's differences are found by one wave and counted once.
constexpr uint64_t kKsVerifyGranuleDraws = 512;
constexpr uint64_t kKsVerifyDefaultDraws = 2048;   // = kDefaultKsMinDraws, the fill's lanes
constexpr uint32_t kKsVerifyMaxLpc = 1024;

struct KsVerifyPlan {
    uint32_t lpc;    // lanes per chunk: a power of two, at most 1024
    uint64_t span;   // draws per lane: a multiple of 512, lpc * span * 8 >= chunk_bytes
};

// chunk_bytes: bytes per chunk (a positive multiple of 4096); nchunks: chunks
// in the launch; cus: compute units; min_lane_draws: the context's knob for
// the mode (s3dg_set_keystream_shape), 0 = not set by the caller.
//   * knob set: lanes of at least min_lane_draws draws (rounded up to 512),
//     whatever the launch's size, so a caller (or a test) picks the lane path:
//     no jump at lpc == 1, the per-lane jump below 64, the wave-uniform one from 64.
//   * knob not set: lanes of at least 2048 draws, and launches of a few chunks
//     are spread over more lanes, down to 512 draws per lane, until the grid
//     has about 4 waves per CU (keystream_plan's rule with 512 for kKsMinSpan).
inline KsVerifyPlan ks_verify_plan(uint64_t chunk_bytes, uint64_t nchunks, uint32_t cus, uint64_t min_lane_draws) {
    const uint64_t G = kKsVerifyGranuleDraws;
    const uint64_t nd = (chunk_bytes + 7) / 8;
    uint64_t min_draws = min_lane_draws ? min_lane_draws : kKsVerifyDefaultDraws;
    min_draws = min_draws > ~0ull - G ? ~0ull / G * G : (min_draws + G - 1) / G * G;
    uint32_t lpc = 1;
    while (lpc < kKsVerifyMaxLpc && nd / (2 * (uint64_t)lpc) >= min_draws) lpc *= 2;
    if (!min_lane_draws) {
        const uint64_t target_lanes = (uint64_t)cus * 4 * 64;
        while (lpc < kKsVerifyMaxLpc && nchunks * lpc < target_lanes && nd / (2 * (uint64_t)lpc) >= G) lpc *= 2;
    }
    uint64_t span = (nd + lpc - 1) / lpc;
    span = (span + G - 1) / G * G;
    return KsVerifyPlan{lpc, span};
}

}  // namespace s3dg
