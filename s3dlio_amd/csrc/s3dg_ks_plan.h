// s3dg_ks_plan.h — the host's arithmetic of the uniform keystream launches
// (k_keystream: s3dg_xoshiro_fill, s3dg_dgen_fill, s3dg_dgen_fill_stream;
// DESIGN.md §5.2, §5.3) as pure functions: the lane plan, a lane's region, the
// DG1 call's zero-split decision, the half-length tail set, the static grid,
// the XCD remap, the persistent launch's decision and queue quotas, and
// fastmod.  No HIP, no context: it compiles with g++ alone
// (tests/capi/ks_plan_sweep.cpp, tests/capi/ks_plan_table.cpp); the functions
// the kernel shares are S3DG_KS_HD.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define S3DG_KS_HD __host__ __device__
#else
#define S3DG_KS_HD
#endif

namespace s3dg {

constexpr uint64_t kKsBlock = 1ull << 20;     // DG1's block (kDgenBlock)
constexpr uint32_t kKsGranule = 4096;         // the zero launch's granule (kBlk)
// Draws per lane (npz keystream, DG1).  Since the jump's state sequence runs
// on the scalar unit (k_keystream), longer lanes win: 2048 draws per lane
// (K2 8 GiB launches 6096 -> 6621 GB/s, 80 GiB 6436 -> 6596; DG1 c1 6141 ->
// 6604 / 6434 -> 6621; profiles/r02/diag/ks/ks_draws_sweep.log), and K2
// launches of at least kKsLongRounds rounds of resident waves take 4096
// (80 GiB: 6718; with 1-wave workgroups in XCD groups also 8 GiB launches,
// profiles/r02/diag/ks/ks_draws_new_shape.log).  DG1 stays at 2048:
// at 4096 a wave would span two 1 MiB blocks and lose the scalar jump.
constexpr uint64_t kDefaultKsMinDraws[2] = {2048, 2048};
constexpr uint64_t kKsLongDraws = 4096;
constexpr uint64_t kKsLongRounds = 4;   // 1-wave workgroups: 8 GiB launches (4 rounds) 6755 -> 6986 GB/s at 4096
constexpr uint64_t kKsMinSpan = 256;          // fewest draws per lane for small launches
// DG1 with a zero prefix (compress > 1): 512 draws per lane by default, so the
// waves that skip the PRNG cover more of each block's prefix (d1 c2: 6413 ->
// 6694 GB/s; at c1 the extra jumps cost: 5896 -> 5347, profiles/r02/diag/k2_xcd.log)
constexpr uint64_t kDgenPrefixMinDraws = 512;
constexpr uint32_t kKsMaxLpc = 1024;          // lanes per chunk at most: 16 waves
// Launches of at least this many rounds of resident 1-wave workgroups run a
// persistent grid by default (the measurements are in s3dg_ks_kernels.hip).
#ifndef S3DG_KS_PERSIST_ROUNDS
#define S3DG_KS_PERSIST_ROUNDS 6
#endif
constexpr uint32_t kKsPersistRounds = S3DG_KS_PERSIST_ROUNDS;

// a % d for 32-bit a and d >= 1 with M = fastmod_magic(d) (Lemire, Kaser &
// Kurz 2019, "Faster remainder by direct computation"); exact for all a, d < 2^32.
// d = 1: M wraps to 0, so the product and with it the remainder are 0.
S3DG_KS_HD inline uint64_t fastmod_magic(uint32_t d) { return ~0ull / d + 1; }
S3DG_KS_HD inline uint32_t fastmod(uint32_t a, uint64_t M, uint32_t d) {
    const uint64_t low = M * a;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__umul64hi(low, (uint64_t)d);
#else
    return (uint32_t)(((unsigned __int128)low * d) >> 64);
#endif
}

// ---- lanes ---------------------------------------------------------------------

// Lanes of a launch: lpc lanes per chunk (a power of two, at most 1024), lane
// sub over draws [z0 + sub*span, + span) of its chunk.  ok false: the span
// does not fit 32 bits ("chunk too large").
struct KsLanes {
    uint32_t lpc;
    uint64_t span;
    bool ok;
};

// mode 0: K2, 1: DG1.  z0 > 0: the lanes cover draws [z0, chunk_bytes / 8) of
// every chunk (the tails of a DG1 zero-prefix split).  min_draws: the
// context's knob for the mode (kDefaultKsMinDraws[mode] = not set).  D: draws
// a lane stages per iteration.  cus: compute units.
//   1. as many lanes per chunk as keep >= min_draws draws per lane (the jump
//      costs 256 steps);
//   2. DG1 with the zero prefix inside the lanes: 512 draws when the knob is
//      not set, so the waves that skip the PRNG cover more of the prefix;
//   3. K2, knob not set: 4096 draws when that still gives kKsLongRounds rounds
//      of the chip's resident keystream waves (4 per CU);
//   4. a tail (z0 > 0) of at least 64 x 256 draws gets at least 64 lanes: one
//      wave, the jump's state sequence on the scalar unit;
//   5. small launches are spread over more lanes, down to 256 draws per lane,
//      until the grid has about 4 waves per CU;
//   6. span is rounded up to D.
inline KsLanes ks_lanes(int mode, uint64_t chunk_bytes, uint64_t nchunks, bool zero_prefix, uint64_t z0,
                        uint64_t min_draws, uint64_t D, uint64_t cus) {
    const uint64_t nd = chunk_bytes / 8 - z0;
    if (mode == 1 && zero_prefix && min_draws == kDefaultKsMinDraws[1]) min_draws = kDgenPrefixMinDraws;
    if (mode == 0 && min_draws == kDefaultKsMinDraws[0] && nd >= 64 * kKsLongDraws) {
        // waves at 4096 draws per lane vs the chip's resident keystream waves
        // (4 per CU: 64-draw stages take 33 KiB of LDS per wave)
        const uint64_t waves = nchunks * (nd / kKsLongDraws) / 64;
        if (waves >= kKsLongRounds * cus * 4) min_draws = kKsLongDraws;
    }
    uint32_t lpc = 1;
    while (lpc < kKsMaxLpc && nd / (2 * lpc) >= min_draws) lpc *= 2;
    if (z0 && lpc < 64 && nd >= 64 * kKsMinSpan) lpc = 64;
    const uint64_t target_lanes = cus * 4 * 64;
    while (lpc < kKsMaxLpc && nchunks * lpc < target_lanes && nd / (2 * lpc) >= kKsMinSpan) lpc *= 2;
    uint64_t span = (nd + lpc - 1) / lpc;
    span = (span + D - 1) / D * D;
    return KsLanes{lpc, span, span <= 0xFFFFFFFFull};
}

// Lane `sub` of a chunk of clen bytes: bytes [rb, rb + rlen) of the chunk
// (rlen 0: nothing), first draw d0 = z0 + sub*span.
struct KsRegion {
    uint64_t rb;
    uint32_t rlen;
};
S3DG_KS_HD inline KsRegion ks_lane_region(uint64_t clen, uint64_t z0, uint32_t span, uint32_t sub) {
    const uint64_t rb = (z0 + (uint64_t)sub * span) * 8;
    const uint32_t rlen =
        (uint32_t)(clen > rb ? ((clen - rb) < (uint64_t)span * 8 ? (clen - rb) : (uint64_t)span * 8) : 0);
    return KsRegion{rb, rlen};
}

// ---- the DG1 call --------------------------------------------------------------

// What dgen_chunk does with blocks [blk_lo, blk_hi) (blk_hi already clipped
// to the object's nb blocks, blk_lo < blk_hi) of n_objs objects of obj_size
// bytes.  split: the context's threshold (s3dg_set_dgen_zero_split, 0 = never).
//   cut_last: the objects' full blocks go to a call over [blk_lo, blk_hi - 1)
//   and their ragged last blocks to a call of their own, [blk_hi - 1, blk_hi);
//   zsplit: the zero launch writes the first zw bytes (whole 4 KiB granules)
//   of every block and the keystream launch starts at draw z0 = zw / 8.
// A split needs every block of the launch full length, a prefix of at least
// 8 whole granules and enough blocks to pay for two launches.
struct KsDgenCall {
    uint32_t zw;
    bool cut_last, zsplit;
    uint64_t nchunks, z0;
};
inline KsDgenCall ks_dgen_call(uint64_t obj_size, uint64_t n_objs, uint64_t blk_lo, uint64_t blk_hi, uint32_t f_num,
                               uint32_t f_den, uint64_t split) {
    KsDgenCall P{};
    const uint64_t nb = (obj_size + kKsBlock - 1) / kKsBlock;
    P.nchunks = (blk_hi - blk_lo) * n_objs;
    P.zw = (uint32_t)(kKsBlock * f_num / f_den) & ~(kKsGranule - 1);
    const bool ragged_end = obj_size % kKsBlock != 0 && blk_hi == nb;
    P.cut_last = f_num > 0 && split && ragged_end && blk_hi - 1 > blk_lo && (blk_hi - 1 - blk_lo) * n_objs >= split &&
                 P.zw >= 8 * kKsGranule;
    P.zsplit = !P.cut_last && f_num > 0 && split && P.nchunks >= split && P.zw >= 8 * kKsGranule && !ragged_end;
    P.z0 = P.zsplit ? P.zw / 8 : 0;
    return P;
}

// One object: its last T chunks in lanes of half the length, handed out
// after the others by a persistent launch, so the launch drains on units
// half as long.  tail_chunks: the context's knob (s3dg_set_keystream_tail),
// negative = half a resident round of 1-wave units (resident workgroups per CU
// x cus x waves x 64 lanes / lpc / 2).  take: the second set (lpc2 = 2 lpc,
// span2 = span / 2) covers chunks [chunk0_2, + T) at byte offset doff, and
// the first set is cut to the nchunks - T before them.
struct KsHalfTail {
    bool take;
    uint64_t T;
    uint32_t lpc2, span2;
    uint64_t chunk0_2, doff, cpo2;   // the second set
    uint64_t nchunks1, cpo1;         // the first set, cut
};
inline KsHalfTail ks_half_tail(int64_t tail_chunks, uint64_t resident_per_cu, uint64_t cus, uint32_t waves,
                               uint32_t D, uint64_t n_objs, uint64_t nchunks, uint64_t chunk0, uint32_t lpc,
                               uint32_t span) {
    KsHalfTail H{};
    if (tail_chunks < 0) tail_chunks = (int64_t)(resident_per_cu * cus * (uint64_t)waves * 64 / lpc / 2);
    const uint32_t span2 = span / 2;
    if (n_objs == 1 && tail_chunks > 0 && waves == 1 && lpc >= 64 && lpc <= 512 && span2 >= kKsMinSpan &&
        span2 % D == 0 && nchunks >= 8 * (uint64_t)tail_chunks) {
        H.take = true;
        H.T = (uint64_t)tail_chunks;
        H.lpc2 = 2 * lpc;
        H.span2 = span2;
        H.cpo2 = H.T;
        H.chunk0_2 = chunk0 + (nchunks - H.T);
        H.doff = (nchunks - H.T) * kKsBlock;
        H.nchunks1 = nchunks - H.T;
        H.cpo1 = nchunks - H.T;
    }
    return H;
}

// ---- grids ---------------------------------------------------------------------

// The static grid of an argument set: wgs workgroups of `waves` waves over
// nchunks x lpc lanes; nwg is what the kernel sees (capped: the launch is
// refused above 2^31 - 1); xg workgroups per XCD group.
struct KsGrid {
    uint64_t wgs;
    uint32_t nwg, xg;
};
inline KsGrid ks_static_grid(uint64_t nchunks, uint32_t lpc, int waves, int xcd_waves) {
    const uint64_t wv = (nchunks * lpc + 63) / 64;
    const uint64_t wgs = (wv + waves - 1) / waves;
    return KsGrid{wgs, (uint32_t)(wgs > 0x7FFFFFFFull ? 0x7FFFFFFFull : wgs),
                  xcd_waves > waves ? (uint32_t)(xcd_waves / waves) : 1u};
}

// Workgroups of the persistent grid, or 0 for the static one.  rounds: the
// context's knob (s3dg_set_keystream_persist; negative: 1-wave workgroups from
// kKsPersistRounds rounds, others never).  The grid is one resident round of
// workgroups, a multiple of 8, taken when both sets together have at least
// `rounds` of them.
inline uint64_t ks_persistent_grid(uint64_t wgs, uint64_t wgs2, int rounds, uint64_t resident_per_cu, uint64_t cus,
                                   int waves) {
    const uint64_t r = rounds < 0 ? (waves == 1 ? kKsPersistRounds : 0) : (uint64_t)rounds;
    if (r == 0 || cus == 0) return 0;
    const uint64_t cap = (resident_per_cu * cus) & ~7ull;
    return cap >= 8 && wgs + wgs2 >= r * cap ? cap : 0;
}

// Workgroups are dealt round-robin to the 8 XCDs, so consecutive ones write
// through different L2s.  Each full group of 8*xg workgroups is remapped so
// the xg workgroups one XCD receives take xg adjacent work units: every XCD
// writes runs of xg*W*64 adjacent lane regions (the last,
// partial group keeps the dealing order).  b: the workgroup's index in the
// static grid of nwg workgroups (dealt to XCD b mod 8); xg: a power of two.
S3DG_KS_HD inline uint64_t ks_remap(uint32_t xg, uint32_t nwg, uint64_t b) {
    if (xg > 1) {
        const uint32_t gs = (uint32_t)__builtin_ctz(xg);
        if (((b >> (gs + 3)) + 1) << (gs + 3) <= nwg) {
            const uint64_t x = b & 7, k = b >> 3;
            return ((k >> gs) << (gs + 3)) + (x << gs) + (k & (xg - 1));
        }
    }
    return b;
}

// Persistent launches: queue v of 8 holds the wave units of the static grid's
// workgroups b = v (mod 8) in order, W per workgroup: `quota` units, unit q
// being wave q % W of workgroup 8*(q / W) + v.
S3DG_KS_HD inline uint64_t ks_queue_quota(uint32_t nwg, uint32_t v, uint32_t W) {
    return (uint64_t)W * ((nwg + 7 - v) / 8);
}
S3DG_KS_HD inline uint64_t ks_queue_wg(uint64_t q, uint32_t v, uint32_t W) { return 8 * (q / W) + v; }
S3DG_KS_HD inline uint32_t ks_queue_wave(uint64_t q, uint32_t W) { return (uint32_t)(q % W); }

}  // namespace s3dg
