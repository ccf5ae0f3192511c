// s3dg_block.hip — the 4 KiB-block family: CDNA4 (gfx950) kernels for s3dlio's
// synthetic payload generator and their launchers.  Semantics: s3dlio's
// src/data_gen.rs:151-224 (fill_controlled_data), bit-exact for a given
// entropy and base block.  The keystream family: s3dg_ks_kernels.hip; what
// the two share: s3dg_dev.h.
//
// Work decomposition (measurements in profiles/):
//   * ONE workgroup per 4 KiB block, non-persistent grid in address order:
//     2 waves per block for streams (each lane two 16-byte stores), 1 wave
//     for batches (four).  Short-lived workgroups dispatched in order keep
//     the write frontier compact; persistent or looping workgroups stayed at
//     5.0-6.3 TB/s on MI355X.
//   * Resident workgroups per CU are capped through reserved LDS (stream:
//     14); fewer blocks in flight write HBM faster than the hardware maximum.
//     Batch workgroups warm the L2 with a later tile record instead.
//   * Stores are global_store_dwordx4 ... sc1: the line leaves the XCD's L2
//     once written (plain stores keep it), measured 2-4 % faster.
//   * Wave 0 derives the block's parameters (u = i % U, zero-prefix length,
//     window offsets) and runs the block's PRNG chain ONCE (SplitMix64 seed
//     words on the VALU, the 8 Xoshiro256++ steps on the scalar unit), then
//     patches the zero bytes and the two 32-byte windows into an LDS image of
//     the base block.  After a barrier every lane stores its 16-byte pieces
//     (zeros below the prefix, the image above).  No HBM reads: dedup blocks
//     are recomputed, never copied.
#include "s3dg_dev.h"

#include <cstdlib>

namespace s3dg {
namespace {

// Per-workgroup LDS: the 4 KiB block image being assembled + its metadata.
struct BlockLds {
    uint8_t img[kBlk];
    uint32_t meta[4];        // c, L
};

// Wave 0, phase 1: block parameters + PRNG chain.  Writes the metadata to LDS
// (lane 0) and returns the window words in `w1`/`w2w` (wave-uniform).
// Scalar-unit budget matters (one SALU per cycle per CU, ~365 cycles per
// 4 KiB block at the write ceiling): the SplitMix64 expansion (all of the
// 64-bit multiplies) runs on the VALU, one seed word per lane; only the 8
// Xoshiro256++ steps (shifts/xors/adds) run on the scalar unit.
struct Plan {
    uint32_t c, L, m, so;
    bool w2;
    uint64_t w1[4], w2w[4];
};

template <bool ABL = false>
__device__ __forceinline__ void plan_block(Plan &P, uint32_t lane, uint32_t i, uint64_t size,
                                           uint64_t entropy, const PrefixParams &pp) {
    const uint32_t u = pp.unique == 0xFFFFFFFFu ? i : fastmod(i, pp.m_unique, pp.unique);  // :201
    const uint64_t off = (uint64_t)i * kBlk;
    const uint32_t L = (uint32_t)((size - off) < kBlk ? (size - off) : kBlk);
    P.L = L;
    if (pp.f_den == 0) {
        // generate_random_data layout (src/data_gen.rs:102-132): no zero prefix,
        // first min(32, L) bytes, then the last 32 bytes when L > HALF_BLK
        P.c = 0;
        P.m = L < kMod ? L : kMod;
        P.so = L - kMod;
        P.w2 = L > kHalf;
    } else {
        uint32_t cl = pp.floor_len;
        if (pp.rem) {                     // closed form of :177-190; period f_den in u
            const uint32_t up = fastmod(u, pp.m_fden, pp.f_den);
            const uint32_t r0 = pp.f_den <= 65536u ? fastmod(up * pp.rem, pp.m_fden, pp.f_den)
                                                   : (uint32_t)(((uint64_t)up * pp.rem) % pp.f_den);
            cl += (uint32_t)((uint64_t)r0 + pp.rem >= pp.f_den);
        }
        P.c = cl < L ? cl : L;                                           // :209
        P.m = (L - P.c) < kMod ? (L - P.c) : kMod;                       // :212-214
        P.so = P.c > kHalf ? P.c : kHalf;                                // :218
        P.w2 = P.m > 0 && P.so + P.m <= L;                               // :219
    }

    // SmallRng::seed_from_u64(u + entropy) (:202-203): state word k =
    // mix64(seed + (k+1)*phi) — lanes 0..3 compute one word each.
    const uint64_t seed = (uint64_t)u + entropy;
    if constexpr (ABL) return;
#if S3DG_ABLATE & 2
    for (int q = 0; q < 4; ++q) { P.w1[q] = seed + q; P.w2w[q] = seed - q; }
    return;
#endif
    Xoshiro g;
#if S3DG_ABLATE & 16
    g.s0 = mix64(seed + 1 * 0x9E3779B97F4A7C15ull);
    g.s1 = mix64(seed + 2 * 0x9E3779B97F4A7C15ull);
    g.s2 = mix64(seed + 3 * 0x9E3779B97F4A7C15ull);
    g.s3 = mix64(seed + 4 * 0x9E3779B97F4A7C15ull);
#else
    const uint64_t zl = mix64(seed + (uint64_t)((lane & 3) + 1) * 0x9E3779B97F4A7C15ull);
    g.s0 = readlane64(zl, 0);
    g.s1 = readlane64(zl, 1);
    g.s2 = readlane64(zl, 2);
    g.s3 = readlane64(zl, 3);
#endif
#if S3DG_ABLATE & 8
    asm volatile("" : "+v"(g.s0), "+v"(g.s1), "+v"(g.s2), "+v"(g.s3));
#endif
    uint64_t r[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = g.next();
    if (P.m == kMod) {                // every full block with c <= 4064
#pragma unroll
        for (int q = 0; q < 4; ++q) { P.w1[q] = r[q]; P.w2w[q] = r[4 + q]; }
    } else {
        // fill_bytes_via_next on m < 32 bytes: k1 draws per window, the last
        // one >>32 (next_u32) when its tail is 1..4 bytes
        const uint32_t k1 = (P.m + 7) >> 3;
        const uint32_t tail = P.m & 7;
        const bool tail_hi = tail >= 1 && tail <= 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            P.w1[q] = r[q];
            P.w2w[q] = k1 == 4 ? r[4 + q] : (k1 == 3 ? r[3 + q] : (k1 == 2 ? r[2 + q] : r[1 + q]));
            if (tail_hi && (uint32_t)q + 1 == k1) { P.w1[q] >>= 32; P.w2w[q] >>= 32; }
        }
    }
}

// Byte q (0..31) of a window given as 4 little-endian words.
__device__ __forceinline__ uint8_t window_byte(const uint64_t (&w)[4], uint32_t q) {
    const uint32_t k = (q >> 3) & 3;
    const uint64_t x = k == 0 ? w[0] : (k == 1 ? w[1] : (k == 2 ? w[2] : w[3]));
    return (uint8_t)(x >> (8 * (q & 7)));
}

// Wave 0, phase 2 (after every lane has copied the base block into the image):
// zero bytes [c & ~15, c) of the partial segment, then window 1 at c, then
// window 2 at so (later write wins, as :217-221).  One byte per lane.
__device__ __forceinline__ void patch_image(BlockLds &S, const Plan &P, uint32_t lane) {
    const uint32_t z0 = P.c & ~15u;
    if (lane < P.c - z0) S.img[z0 + lane] = 0;                           // :209-210
    if (lane < P.m) S.img[P.c + lane] = window_byte(P.w1, lane);         // :217
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (P.w2 && lane < P.m) S.img[P.so + lane] = window_byte(P.w2w, lane);   // :219-221
}

// Every lane, phase 3: its 16 bytes at byte o of the block: zeros below c, else the image.
// Diagnostic builds only (tools/variant_lab.py, config-3 A/Bs): S3DG_DIAG_ZERO
// bit 0 = zero-prefix pieces store the constant S3DG_DIAG_ZVAL instead of 0
// (same instructions, other data; wrong bytes by design), bit 1 = zero-prefix
// pieces read their LDS image piece too (same data, the store stream paced
// like a prefix-free block), bit 2 = a block's pieces stored last-first;
// S3DG_DIAG_ZPOL = store policy of the zero-prefix pieces (kStore*).
#ifndef S3DG_DIAG_ZERO
#define S3DG_DIAG_ZERO 0
#endif
#ifndef S3DG_DIAG_ZVAL
#define S3DG_DIAG_ZVAL 0x5A5A5A5Au
#endif
template <int NT>
__device__ __forceinline__ void write_block(uint8_t *bd, const BlockLds &S, int o) {
    const int c = (int)S.meta[0], L = (int)S.meta[1];
    if (o >= L) return;
#if S3DG_DIAG_ZERO & 1
    const u32x4 zero = {S3DG_DIAG_ZVAL, S3DG_DIAG_ZVAL, S3DG_DIAG_ZVAL, S3DG_DIAG_ZVAL};
#else
    const u32x4 zero = {0u, 0u, 0u, 0u};
#endif
#if S3DG_DIAG_ZERO & 2
    u32x4 im = *reinterpret_cast<const u32x4 *>(S.img + o);
    asm volatile("" : "+v"(im));
    const u32x4 v = (o + 16 <= c) ? zero : im;
#else
    const u32x4 v = (o + 16 <= c) ? zero : *reinterpret_cast<const u32x4 *>(S.img + o);
#endif
    if (o + 16 <= L) {
#ifdef S3DG_DIAG_ZPOL
        if (o + 16 <= c) store16<S3DG_DIAG_ZPOL>(bd + o, v);   // diagnostic: zero pieces' own store policy
        else
#endif
        store16<NT>(bd + o, v);
    } else {                                  // ragged object tail: bytes < L only
        const uint32_t dw[4] = {v.x, v.y, v.z, v.w};
        for (int b = 0; b < 16 && o + b < L; ++b)
            bd[o + b] = (uint8_t)(dw[b >> 2] >> (8 * (b & 3)));
    }
}

// The whole per-block body (all three phases); NW waves per 4 KiB block.
// Base-block pieces of thread t (issued first: they depend on kernel
// arguments only, so their latency overlaps the plan's inputs).
template <int NW>
__device__ __forceinline__ void load_base(u32x4 (&B)[4 / NW], uint32_t t, const u32x4 *base) {
    constexpr int T = 64 * NW;
#pragma unroll
    for (int k = 0; k < 4 / NW; ++k) B[k] = base[t + k * T];   // bytes 16(t+kT).. of the base block
}

template <int NW>
__device__ __forceinline__ void store_image(BlockLds &S, uint32_t t, const u32x4 (&B)[4 / NW]) {
    constexpr int T = 64 * NW;
#pragma unroll
    for (int k = 0; k < 4 / NW; ++k)
        *reinterpret_cast<u32x4 *>(S.img + 16 * (t + k * T)) = B[k];   // :205-207
}

// IMG: the caller has already written the base image into S (batch kernel).
// ABL: the store-only reference of the same kernel (write ceiling): block
// geometry, LDS image, barrier and stores as the fill, without the PRNG chain
// and the window patch phase; its bytes are wrong by design.
// rt_floor > 0: the block's stores wait until rt_floor wall-clock ticks
// (100 MHz) after its workgroup started (t0): a floor on the time before the
// stores that does not scale with the GFX clock.
template <int NT, int NW, bool IMG = false, bool ABL = false>
__device__ __forceinline__ void gen_block(uint8_t *bd, BlockLds &S, uint32_t t, uint32_t wave,
                                          uint32_t i, uint64_t size, uint64_t entropy,
                                          const PrefixParams &pp, const u32x4 (&B)[4 / NW], uint64_t t0 = 0,
                                          uint32_t rt_floor = 0) {
    constexpr int T = 64 * NW, SPL = 4 / NW;   // segments per lane
    const uint32_t lane = t & 63;
    Plan P;
    if (wave == 0) {
        plan_block<ABL>(P, lane, i, size, entropy, pp);
        if (lane == 0) { S.meta[0] = P.c; S.meta[1] = P.L; }
    }
    if constexpr (!IMG) store_image<NW>(S, t, B);
    __syncthreads();
#if !(S3DG_ABLATE & 1)
    if constexpr (!ABL) {
        if (wave == 0) patch_image(S, P, lane);
        __syncthreads();
    }
#endif
    // bounded as well by sleep count (4 x rt_floor sleeps of >= 64 cycles, i.e.
    // at least rt_floor x 256 cycles), so the wait ends even if the real-time
    // counter did not advance
    if (rt_floor)
        for (uint32_t n = 0; n < 4 * rt_floor && wall_clock64() - t0 < (uint64_t)rt_floor; ++n)
            __builtin_amdgcn_s_sleep(1);
#if S3DG_DIAG_ZERO & 4
    // diagnostic: pieces stored last-first (the zero prefix's stores after the image's)
#pragma unroll
    for (int k = SPL - 1; k >= 0; --k) write_block<NT>(bd, S, (int)(t + k * T) * 16);
#else
#pragma unroll
    for (int k = 0; k < SPL; ++k) write_block<NT>(bd, S, (int)(t + k * T) * 16);
#endif
}

// Stream: blockIdx.x = block (blk_lo + x) of object blockIdx.y of this launch
// (dst and ent0 already advanced to the launch's first object).  Argument
// order matters: the first 14 dwords arrive preloaded in SGPRs, the rest by
// a scalar load from the kernarg segment, so base (needed first) and
// everything up to the plan's first use lead and the prefix parameters trail.
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void k_fill_stream(uint8_t *dst, const u32x4 *base, uint64_t stride,
                                                         uint64_t ent0, uint64_t obj_size, uint32_t blk_lo,
                                                         PrefixParams pp) {
    __shared__ __attribute__((aligned(16))) BlockLds S;
    const uint32_t t = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    uint64_t jv = blockIdx.y;        // block address on the VALU: keep the scalar unit
    asm volatile("" : "+v"(jv));     // for the PRNG chain
    uint8_t *bd = dst + jv * stride + (uint64_t)blockIdx.x * kBlk;
    u32x4 B[4 / NW];
    load_base<NW>(B, t, base);
    gen_block<NT, NW>(bd, S, t, wave, blk_lo + blockIdx.x, obj_size,
                      ent0 + ((uint64_t)blockIdx.y << 32), pp, B);
}

// Verify, the read-side twin of k_fill_stream (same grid, same phases 1-2):
// the workgroup rebuilds its block's LDS image exactly as the fill does, then
// each thread compares its 16-byte pieces of `src` with the expected piece
// (zero below c, else the image) instead of storing them.  The loads of the
// whole pieces are issued first, beside the base block's, so HBM latency
// overlaps the plan; a piece is whole when it ends at or below the block's
// length L, and the ragged piece of an object's last block is read byte by
// byte below L only (as write_block stores it): no byte at or past the
// object's end is ever loaded.  Counts are reduced over the wave by shuffles
// and over the waves through LDS; thread 0 touches the result record (two
// 64-bit adds and a 64-bit min, vector atomics) only when the block's count is
// non-zero, so a clean block costs no store and no atomic.  off0: byte offset
// of this launch's src from the caller's (sub-launches, host chunks).
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_verify_stream(const uint8_t *src, const u32x4 *base, uint64_t stride,
                                                           uint64_t ent0, uint64_t obj_size, uint32_t blk_lo,
                                                           PrefixParams pp, uint64_t off0, VerifyRec *rec) {
    constexpr int T = 64 * NW, SPL = 4 / NW;
    __shared__ __attribute__((aligned(16))) BlockLds S;
    __shared__ uint32_t wcnt[NW], wfirst[NW];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = t & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint32_t i = blk_lo + blockIdx.x;
    const uint64_t boff = (uint64_t)blockIdx.y * stride + (uint64_t)blockIdx.x * kBlk;
    const uint8_t *bs = src + boff;
    const uint64_t left = obj_size - (uint64_t)i * kBlk;          // the launcher keeps i * 4 KiB < obj_size
    const uint32_t L = left < kBlk ? (uint32_t)left : kBlk;       // = Plan::L
    u32x4 B[SPL], G[SPL];
    load_base<NW>(B, t, base);
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const uint32_t o = (t + k * T) * 16;
        G[k] = u32x4{0u, 0u, 0u, 0u};
        // nontemporal (global_load_dwordx4 ... nt): the bytes are read once; 1.3 % over
        // plain loads in three alternating pairs on one box (profiles/verify/nt_ab.log)
        if (o + 16 <= L) G[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(bs + o));
    }
    Plan P;
    if (wave == 0) {
        plan_block<false>(P, lane, i, obj_size, ent0 + ((uint64_t)blockIdx.y << 32), pp);
        if (lane == 0) { S.meta[0] = P.c; S.meta[1] = P.L; }
    }
    store_image<NW>(S, t, B);
    __syncthreads();
    if (wave == 0) patch_image(S, P, lane);
    __syncthreads();
    const uint32_t c = S.meta[0];
    uint32_t cnt = 0, first = kBlk;                               // kBlk: no differing byte
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const uint32_t o = (t + k * T) * 16;
        if (o >= L) continue;
        u32x4 e = {0u, 0u, 0u, 0u};
        if (o + 16 > c) e = *reinterpret_cast<const u32x4 *>(S.img + o);
        if (o + 16 <= L) {
            const u32x4 x = G[k] ^ e;
            if (x.x | x.y | x.z | x.w) diff_piece(x, o, cnt, first);
        } else {                                                  // ragged object tail: bytes < L only
            const uint32_t dw[4] = {e.x, e.y, e.z, e.w};
            for (uint32_t b = 0; o + b < L; ++b)
                if (bs[o + b] != (uint8_t)(dw[b >> 2] >> (8 * (b & 3)))) {
                    ++cnt;
                    first = o + b < first ? o + b : first;
                }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += __shfl_xor(cnt, d, 64);
        const uint32_t f = __shfl_xor(first, d, 64);
        first = f < first ? f : first;
    }
    if constexpr (NW > 1) {
        if (lane == 0) { wcnt[wave] = cnt; wfirst[wave] = first; }
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                cnt += wcnt[w];
                first = wfirst[w] < first ? wfirst[w] : first;
            }
        }
    }
    if (t == 0 && cnt) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&rec->bytes), (unsigned long long)cnt);
        atomicAdd(reinterpret_cast<unsigned long long *>(&rec->blocks), 1ull);
        atomicMin(reinterpret_cast<unsigned long long *>(&rec->first), (unsigned long long)(off0 + boff + first));
    }
}

// Batch: workgroup g -> tile record g >> tshift (one scalar load), block
// first + (g mod 2^tshift) - lead of that object; slots before the object's
// start (lead) or past its end exit (slot_block, s3dg_batch_plan.h, restates
// the expression).  lead makes g = 4 KiB-granule address (mod 8) for the dense
// layout and tiles of 8 blocks and more, as in the stream kernel: workgroups
// are dealt round-robin to the 8 XCDs, so XCD x writes only granules = x
// (mod 8).  With forced 2- and 4-block tiles an object's first
// slot is a multiple of the tile only, so g = granule holds mod 2 and mod 4
// (tests/capi/batch_records_sweep.cpp asserts both).
// Tiles are 2^tshift blocks (8..64 chosen per launch by the host so the
// dead workgroups of ragged object tails stay few, 2 and 4 forced only;
// DESIGN.md §5.1).
// pf > 0: the first 8 workgroups of every 256 blocks (one per XCD: workgroups
// are dealt round-robin to the XCDs) touch the records of the 256 blocks
// 64*pf blocks ahead (one lane per 128-byte line of records) after their
// stores, result unused, so they are in that XCD's L2 when its workgroups
// start.  pf must exceed the resident workgroups / 64.
// FLOOR: the fill with the wall-clock floor compiled in (launches whose
// rt_floor > 0).  The floor-free instantiation carries none of its code: the
// conditional real-time read and wait cost launches that never use them
// 0.3-1 % (round 4 library A/B).
template <int NT, int NW, bool ABL = false, bool FLOOR = false>
__global__ __launch_bounds__(64 * NW) void k_fill_batch(uint8_t *dst_base, const TileRec *tiles,
                                                        uint64_t ntiles, uint64_t g0, uint32_t pf,
                                                        uint32_t tshift, const u32x4 *base, uint32_t pace) {
    __shared__ __attribute__((aligned(16))) BlockLds S;
    const uint32_t t = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // pace: the store-only reference's wave-0 delay (ABL), else the fill's
    // wall-clock floor before the stores (rt_floor; FLOOR instantiation only)
    const uint64_t t0 = (!ABL && FLOOR) ? wall_clock64() : 0;
    const uint64_t g = g0 + blockIdx.x;
    const uint64_t tile = g >> tshift;
    // The tile record (64 B) in ONE scalar load, issued first; then the base
    // block's vector loads and its LDS image, so the two memory latencies
    // overlap instead of following each other (the compiler otherwise splits
    // the record into four loads around the early-exit branch).
    u32x16 raw;
    asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=s"(raw) : "s"(tiles + tile) : "memory");
    u32x4 B[4 / NW];
    load_base<NW>(B, t, base);
    // the wait "redefines" raw, so no use of the record can move above it.
    // The LDS image is written after it (round 4): before, this wait also
    // covered the image's ds_writes, which wait for the base block's loads,
    // so the record-dependent work (and a dead slot's exit) started only once
    // those had landed; after: config 2 +0.45-0.5 %, config 4 +0.2 %,
    // config 3 -0.25 % (two library A/Bs, profiles/r04/d, profiles/r04/e).
    // Later still, after wave 0's plan (gen_block's own image write), lost
    // 3.5-5.7 % on configs 2, 4 and 5 (profiles/r04/g).
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(raw) :: "memory");
    const TileRec e = __builtin_bit_cast(TileRec, raw);
    const uint32_t k = (uint32_t)(g & ((1u << tshift) - 1));
    const int64_t ib = (int64_t)e.first + k - e.lead;
    uint8_t *const bdst = dst_base + e.dst_off + (uint64_t)ib * kBlk;
    if (ib < 0 || (uint64_t)ib * kBlk >= e.size) return;   // uniform for the whole workgroup
    store_image<NW>(S, t, B);
    if constexpr (ABL) {   // store-only reference: wave 0 idles `pace` x 2 x 64 cycles in the plan's place
        if (wave == 0)
            for (uint32_t q = 0; q < pace; ++q) __builtin_amdgcn_s_sleep(2);
    }
    gen_block<NT, NW, true, ABL>(bdst, S, t, wave, (uint32_t)ib, e.size, e.entropy, e.pp, B, t0,
                                 (!ABL && FLOOR) ? pace : 0u);
    // one prefetching workgroup per XCD per span blocks (256: 128 and 512
    // measured slower); lane q of it touches the q-th
    // 128-byte line (2 records) of the span's records
    constexpr uint32_t kPfSpan = 256;
    const uint32_t span = kPfSpan > (2u << tshift) ? kPfSpan : (2u << tshift);
    if (pf && (g & (span - 1)) < 8) {
        const uint64_t first = ((g + 64ull * pf) & ~(uint64_t)(span - 1)) >> tshift;
        if (tshift == 0) {
            // one record per block: this workgroup's XCD (g mod 8, dealt
            // round-robin) uses only the records = g (mod 8) of the span, so
            // it touches those 32 and leaves the rest to the other XCDs
            if (t < span / 8) {
                const uint64_t pt = first + 8 * t + (g & 7);
                const TileRec *p = tiles + (pt < ntiles ? pt : ntiles - 1);
                uint32_t dummy;
                asm volatile("global_load_dword %0, %1, off" : "=v"(dummy) : "v"(p) : "memory");
            }
        } else if (t < (span >> (tshift + 1))) {
            const uint64_t pt = first + 2 * t;
            const TileRec *p = tiles + (pt < ntiles ? pt : ntiles - 1);
            uint32_t dummy;
            asm volatile("global_load_dword %0, %1, off" : "=v"(dummy) : "v"(p) : "memory");
        }
    }
}

// Batch verify, the read-side twin of k_fill_batch as k_verify_stream is of
// k_fill_stream: workgroup g -> tile record g >> tshift
// (one scalar load), block first + (g mod 2^tshift) of that object; a slot
// past the object's end exits, uniformly for the workgroup.  No lead: nothing
// is stored, so slots need not follow the XCD dealing.  Phases 1-2 are the
// fill's; phase 3 is k_verify_stream's compare: whole 16-byte pieces (those
// that end at or below the block's length) loaded nontemporally before the
// plan, the ragged piece of an object's last block read byte by byte below
// its length, zeros expected below c and the image above.  Thread 0 of a
// block with differences makes three vector atomics on the call's totals
// (offsets from src_base) and three on its object's record (offsets from the
// object's start; pobj null: totals only); a clean block touches no memory.
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_verify_batch(const uint8_t *src_base, const VTileRec *tiles, uint64_t g0,
                                                          uint32_t tshift, const u32x4 *base, VerifyRec *tot,
                                                          VerifyRec *pobj) {
    constexpr int T = 64 * NW, SPL = 4 / NW;
    __shared__ __attribute__((aligned(16))) BlockLds S;
    __shared__ uint32_t wcnt[NW], wfirst[NW];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = t & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const uint64_t g = g0 + blockIdx.x;
    const uint64_t tile = g >> tshift;
    // the record in ONE scalar load issued first, then the base block's
    // vector loads, as k_fill_batch; the wait "redefines" raw, so no use of
    // the record moves above it
    u32x16 raw;
    asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=s"(raw) : "s"(tiles + tile) : "memory");
    u32x4 B[SPL], G[SPL];
    load_base<NW>(B, t, base);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(raw) :: "memory");
    const VTileRec e = __builtin_bit_cast(VTileRec, raw);
    const uint32_t i = e.first + (uint32_t)(g & ((1u << tshift) - 1));
    const uint64_t boff = (uint64_t)i * kBlk;
    if (boff >= e.size) return;                                   // uniform for the whole workgroup
    const uint8_t *bs = src_base + e.src_off + boff;
    const uint64_t left = e.size - boff;
    const uint32_t L = left < kBlk ? (uint32_t)left : kBlk;       // = Plan::L
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const uint32_t o = (t + k * T) * 16;
        G[k] = u32x4{0u, 0u, 0u, 0u};
        if (o + 16 <= L) G[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(bs + o));
    }
    Plan P;
    if (wave == 0) {
        plan_block<false>(P, lane, i, e.size, e.entropy, e.pp);
        if (lane == 0) { S.meta[0] = P.c; S.meta[1] = P.L; }
    }
    store_image<NW>(S, t, B);
    __syncthreads();
    if (wave == 0) patch_image(S, P, lane);
    __syncthreads();
    const uint32_t c = S.meta[0];
    uint32_t cnt = 0, first = kBlk;                               // kBlk: no differing byte
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const uint32_t o = (t + k * T) * 16;
        if (o >= L) continue;
        u32x4 x = {0u, 0u, 0u, 0u};
        if (o + 16 > c) x = *reinterpret_cast<const u32x4 *>(S.img + o);
        if (o + 16 <= L) {
            x ^= G[k];
            if (x.x | x.y | x.z | x.w) diff_piece(x, o, cnt, first);
        } else {                                                  // ragged object tail: bytes < L only
            const uint32_t dw[4] = {x.x, x.y, x.z, x.w};
            for (uint32_t b = 0; o + b < L; ++b)
                if (bs[o + b] != (uint8_t)(dw[b >> 2] >> (8 * (b & 3)))) {
                    ++cnt;
                    first = o + b < first ? o + b : first;
                }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += __shfl_xor(cnt, d, 64);
        const uint32_t f = __shfl_xor(first, d, 64);
        first = f < first ? f : first;
    }
    if constexpr (NW > 1) {
        if (lane == 0) { wcnt[wave] = cnt; wfirst[wave] = first; }
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                cnt += wcnt[w];
                first = wfirst[w] < first ? wfirst[w] : first;
            }
        }
    }
    if (t == 0 && cnt) {
        typedef unsigned long long ull;
        atomicAdd(reinterpret_cast<ull *>(&tot->bytes), (ull)cnt);
        atomicAdd(reinterpret_cast<ull *>(&tot->blocks), 1ull);
        atomicMin(reinterpret_cast<ull *>(&tot->first), (ull)(e.src_off + boff + first));
        if (pobj) {
            VerifyRec *r = pobj + e.obj;
            atomicAdd(reinterpret_cast<ull *>(&r->bytes), (ull)cnt);
            atomicAdd(reinterpret_cast<ull *>(&r->blocks), 1ull);
            atomicMin(reinterpret_cast<ull *>(&r->first), (ull)(boff + first));
        }
    }
}

// Records of a batch sub-batch from its uploaded descriptors, one thread per
// object: record q in [rec_lo, rec_hi) maps slot (q << tshift) + k to block
// (q - rec_lo) << tshift + k - lead.  The ranges are the record rules of
// s3dg_batch_plan.h (tiled_records, dense_records).  Tile layouts: rec_lo from
// the scan, lead = the object's granule mod 8 (XCD alignment).  Dense: rec_lo =
// the object's granule slot (0 for the first object, whose lead is lead0),
// rec_hi = the next object's, so the gap records before it are its dead slots.
// An object with few records (map_own_records) writes them itself; the records
// of objects with more (a multi-GiB object, a dense layout with large gaps) are
// written by the whole wave, 64 per pass, so no lane loops over tens of
// thousands of them while the fill waits.
__global__ __launch_bounds__(256) void k_batch_map(const s3dg_obj_desc *d, uint64_t n, const uint64_t *scan,
                                                   TileRec *tiles, uint32_t tshift, uint64_t base, uint64_t lead0,
                                                   uint64_t first_off) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    TileRec r{};
    uint64_t rec_lo = 0, rec_hi = 0;
    if (k < n) {
        const s3dg_obj_desc o = d[k];
        const uint64_t nb = obj_blocks(o.size);
        const RecRange R = tshift == 0 ? dense_records(k == 0, lead0, first_off, o.dst_off, nb, k + 1 < n,
                                                       k + 1 < n ? d[k + 1].dst_off : 0)
                                       : tiled_records(scan[k], nb, base, o.dst_off, tshift);
        rec_lo = R.lo;
        rec_hi = R.hi;
        r.dst_off = o.dst_off;
        r.size = o.size;
        r.entropy = o.entropy;
        r.lead = (uint32_t)R.lead;
        r.pp = prefix_params(nb, o.dedup, o.f_num, o.f_den);
    }
    const bool own = map_own_records(rec_hi - rec_lo);
    if (own)
        for (uint64_t q = rec_lo; q < rec_hi; ++q) {
            r.first = (uint32_t)((q - rec_lo) << tshift);
            tiles[q] = r;
        }
    // the wave's objects with many records, one after the other, 64 records per pass
    uint64_t big = __ballot(!own);
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        TileRec b;
        uint32_t *bw = reinterpret_cast<uint32_t *>(&b);
        const uint32_t *rw = reinterpret_cast<const uint32_t *>(&r);
#pragma unroll
        for (int w = 0; w < 16; ++w) bw[w] = __builtin_amdgcn_readlane(rw[w], src);
        const uint64_t lo = readlane64(rec_lo, src), hi = readlane64(rec_hi, src);
        for (uint64_t q = lo + lane; q < hi; q += 64) {
            b.first = (uint32_t)((q - lo) << tshift);
            tiles[q] = b;
        }
    }
}

// Records of a verify sub-batch from its uploaded descriptors, one thread per
// descriptor k (empty ones included, so k is the record's object index):
// records [scan[k], scan[k] + verify_obj_tiles) of object k, record q's first
// block (q - scan[k]) << tshift.  Objects with many records are written by the
// whole wave, as in k_batch_map.
__global__ __launch_bounds__(256) void k_verify_batch_map(const s3dg_obj_desc *d, uint64_t n, const uint64_t *scan,
                                                          VTileRec *tiles, uint32_t tshift) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    VTileRec r{};
    uint64_t rec_lo = 0, rec_hi = 0;
    if (k < n) {
        const s3dg_obj_desc o = d[k];
        if (o.size) {   // an empty object has no records, and its other fields are not looked at
            rec_lo = scan[k];
            rec_hi = rec_lo + verify_obj_tiles(o.size, tshift);
            r.src_off = o.dst_off;
            r.size = o.size;
            r.entropy = o.entropy;
            r.obj = (uint32_t)k;
            r.pp = prefix_params(obj_blocks(o.size), o.dedup, o.f_num, o.f_den);
        }
    }
    const bool own = map_own_records(rec_hi - rec_lo);
    if (own)
        for (uint64_t q = rec_lo; q < rec_hi; ++q) {
            r.first = (uint32_t)((q - rec_lo) << tshift);
            tiles[q] = r;
        }
    uint64_t big = __ballot(!own);
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        VTileRec b;
        uint32_t *bw = reinterpret_cast<uint32_t *>(&b);
        const uint32_t *rw = reinterpret_cast<const uint32_t *>(&r);
#pragma unroll
        for (int w = 0; w < 16; ++w) bw[w] = __builtin_amdgcn_readlane(rw[w], src);
        const uint64_t lo = readlane64(rec_lo, src), hi = readlane64(rec_hi, src);
        for (uint64_t q = lo + lane; q < hi; q += 64) {
            b.first = (uint32_t)((q - lo) << tshift);
            tiles[q] = b;
        }
    }
}

// n result records set to "clean": {0, 0, UINT64_MAX}.
__global__ __launch_bounds__(256) void k_verify_recs_reset(VerifyRec *recs, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) recs[k] = VerifyRec{0, 0, UINT64_MAX};
}

// tiles[q] for a uniform stream: n objects of obj_size bytes at dst_off =
// j * stride, entropy ent0 + (j << 32), all with the same lead (stride a
// multiple of 32 KiB), tiles_per_obj tiles each.
__global__ __launch_bounds__(256) void k_tile_map_uniform(TileRec *tiles, uint64_t ntiles, uint32_t tiles_per_obj,
                                                          uint32_t tshift, uint64_t stride, uint64_t obj_size,
                                                          uint64_t ent0, uint32_t lead, PrefixParams pp) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= ntiles) return;
    const uint64_t j = q / tiles_per_obj;
    TileRec r;
    r.dst_off = j * stride;
    r.size = obj_size;
    r.entropy = ent0 + (j << 32);
    r.first = (uint32_t)((q - j * tiles_per_obj) << tshift);
    r.lead = lead;
    r.pp = pp;
    tiles[q] = r;
}

// Write-only ceiling in the fill kernels' shape: one 4 KiB chunk per
// (64*NW)-thread workgroup, 16-byte stores, same occupancy cap.  pf > 0:
// the tiled fill's trailing loads too (64-block records in thr, 256-block
// spans, k_fill_batch), so the ceiling covers that shape.
template <int NT, int NW>
__global__ __launch_bounds__(64 * NW) void k_write_ceiling(uint8_t *dst, uint64_t nchunks, uint64_t g0,
                                                           uint32_t pat, const TileRec *thr, uint64_t nthr,
                                                           uint32_t pf) {
    const u32x4 v = {pat, pat ^ 0x9E3779B9u, pat + 1u, ~pat};
    const uint64_t g = g0 + blockIdx.x;
    if (g >= nchunks) return;
#pragma unroll
    for (int k = 0; k < 4 / NW; ++k) store16<NT>(dst + g * kBlk + (threadIdx.x + k * 64 * NW) * 16, v);
    if (pf && (g & 255) < 8 && threadIdx.x < 2) {
        const uint64_t pt = (((g + 64ull * pf) & ~255ull) >> 6) + 2 * threadIdx.x;
        const TileRec *p = thr + (pt < nthr ? pt : nthr - 1);
        uint32_t dummy;
        asm volatile("global_load_dword %0, %1, off" : "=v"(dummy) : "v"(p) : "memory");
    }
}

// Batch launches (k_fill_batch, 64 x NW threads): the largest multiple of 256
// workgroups (XCD dealing and the prefetch spans restart at each launch) whose
// work items still fit in 32 bits, so a config-2 step (20.5 M blocks) is one
// launch instead of five.  Env S3DG_BATCH_GRID_CAP (a multiple of 256)
// overrides it, for A/Bs and for the tests of the split path.
uint64_t batch_grid_cap(int nw) {
#ifdef S3DG_DIAG_GRID_CAP
    (void)nw;
    return S3DG_DIAG_GRID_CAP;   // diagnostic builds (tools/variant_lab.py A/B)
#endif
    static const uint64_t env = [] {
        const char *v = getenv("S3DG_BATCH_GRID_CAP");
        const uint64_t x = v ? strtoull(v, nullptr, 10) : 0;
        return x >= 256 ? x & ~255ull : 0ull;
    }();
    const uint64_t lim = (0xFFFFFFFFull / (64ull * (uint64_t)nw)) & ~255ull;
    return env && env < lim ? env : lim;
}

// The sub-launches of a stream launch over n_objs objects (y) of nx blocks
// (x): grids of at most 65535 x kMaxGridX workgroups.  launch(y0, ny, x0, gx)
// enqueues one; the first launch error ends the loop.
template <class F>
hipError_t for_stream_grids(uint64_t n_objs, uint32_t nx, F &&launch) {
    for (uint64_t y0 = 0; y0 < n_objs; y0 += 65535) {
        const uint32_t ny = (uint32_t)((n_objs - y0) < 65535 ? (n_objs - y0) : 65535);
        for (uint64_t x0 = 0; x0 < nx; x0 += kMaxGridX) {
            const uint32_t gx = (uint32_t)((nx - x0) < kMaxGridX ? (nx - x0) : kMaxGridX);
            launch(y0, ny, x0, gx);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace

uint32_t occupancy_lds(int wgs, uint32_t static_lds) {
    if (wgs <= 0) return 0;
    constexpr uint32_t kLdsPerCu = 160u * 1024u, kGranule = 512u;
    // smallest granule-rounded footprint with floor(kLdsPerCu / footprint) == wgs
    uint32_t total = (kLdsPerCu / (uint32_t)(wgs + 1)) / kGranule * kGranule + kGranule;
    if (total < static_lds) return 0;
    return total - static_lds;
}

hipError_t fill_occupancy(const LaunchCfg &lc, bool batch, int *wgs_per_cu) {
    return dispatch_cfg(lc, [&](auto SP, auto NW) {
        constexpr int sp = decltype(SP)::value, nw = decltype(NW)::value;
        const void *k = batch ? reinterpret_cast<const void *>(&k_fill_batch<sp, nw>)
                              : reinterpret_cast<const void *>(&k_fill_stream<sp, nw>);
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(wgs_per_cu, k, 64 * nw, lc.dyn_lds);
    });
}

hipError_t launch_fill_stream(const LaunchCfg &lc, uint8_t *dst, uint64_t obj_size,
                              uint64_t stride, uint64_t n_objs, uint32_t blk_lo,
                              uint32_t blk_hi, uint64_t seed_base, uint64_t first_obj,
                              PrefixParams pp, const void *base_dev, hipStream_t s) {
    (void)hipGetLastError();   // drop stale errors of unrelated calls (e.g. torch pointer probes)
    const u32x4 *b = reinterpret_cast<const u32x4 *>(base_dev);
    return for_stream_grids(n_objs, blk_hi - blk_lo, [&](uint64_t y0, uint32_t ny, uint64_t x0, uint32_t gx) {
        dispatch_cfg(lc, [&](auto SP, auto NW) {
            constexpr int sp = decltype(SP)::value, nw = decltype(NW)::value;
            hipLaunchKernelGGL((k_fill_stream<sp, nw>), dim3(gx, ny), dim3(64 * nw), lc.dyn_lds, s,
                               dst + y0 * stride + x0 * kBlk, b, stride, seed_base + ((first_obj + y0) << 32),
                               obj_size, (uint32_t)(blk_lo + x0), pp);
        });
    });
}

// The verify twin of launch_fill_stream: same y / x splits, each sub-launch
// given its byte offset from `src` (plus off0) so the record's first offset is
// relative to the caller's buffer.  rec (device) accumulates; the caller
// zeroes it on the stream first.  No occupancy cap: the pass only reads.
hipError_t launch_verify_stream(const LaunchCfg &lc, const uint8_t *src, uint64_t obj_size, uint64_t stride,
                                uint64_t n_objs, uint32_t blk_lo, uint32_t blk_hi, uint64_t seed_base,
                                uint64_t first_obj, PrefixParams pp, const void *base_dev, uint64_t off0,
                                VerifyRec *rec, hipStream_t s) {
    (void)hipGetLastError();
    const u32x4 *b = reinterpret_cast<const u32x4 *>(base_dev);
    return for_stream_grids(n_objs, blk_hi - blk_lo, [&](uint64_t y0, uint32_t ny, uint64_t x0, uint32_t gx) {
        const uint64_t sub = y0 * stride + x0 * kBlk;
        dispatch_waves(lc.waves_per_block, [&](auto NW) {
            constexpr int nw = decltype(NW)::value;
            hipLaunchKernelGGL((k_verify_stream<nw>), dim3(gx, ny), dim3(64 * nw), 0, s, src + sub, b, stride,
                               seed_base + ((first_obj + y0) << 32), obj_size, (uint32_t)(blk_lo + x0), pp,
                               off0 + sub, rec);
        });
    });
}

hipError_t verify_rec_reset(VerifyRec *rec, hipStream_t s) {
    hipError_t e = hipMemsetAsync(rec, 0, 2 * sizeof(uint64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(&rec->first, 0xFF, sizeof(uint64_t), s);
    return e;
}

// k_fill_batch over total_tiles << tshift slots, in launches of at most
// batch_grid_cap: the fill (with the wall-clock floor compiled in only when
// lc.rt_floor asks for it), or its store-only reference (ablated, lc.pace).
static hipError_t batch_tiles(const LaunchCfg &lc, uint8_t *dst_base, uint64_t total_tiles, uint32_t tshift,
                              TileRec *tiles, const void *base_dev, hipStream_t s, bool ablated) {
    const u32x4 *b = reinterpret_cast<const u32x4 *>(base_dev);
    const uint64_t total = total_tiles << tshift;
    const uint64_t cap = batch_grid_cap(lc.waves_per_block);
    for (uint64_t g0 = 0; g0 < total; g0 += cap) {
        const dim3 g((uint32_t)((total - g0) < cap ? (total - g0) : cap));
        dispatch_cfg(lc, [&](auto SP, auto NW) {
            constexpr int sp = decltype(SP)::value, nw = decltype(NW)::value;
            const dim3 t(64 * nw);
            if (ablated)
                hipLaunchKernelGGL((k_fill_batch<sp, nw, true>), g, t, lc.dyn_lds, s, dst_base, tiles, total_tiles, g0,
                                   lc.prefetch_tiles, tshift, b, lc.pace);
            else if (lc.rt_floor)
                hipLaunchKernelGGL((k_fill_batch<sp, nw, false, true>), g, t, lc.dyn_lds, s, dst_base, tiles,
                                   total_tiles, g0, lc.prefetch_tiles, tshift, b, lc.rt_floor);
            else
                hipLaunchKernelGGL((k_fill_batch<sp, nw>), g, t, lc.dyn_lds, s, dst_base, tiles, total_tiles, g0,
                                   lc.prefetch_tiles, tshift, b, 0u);
        });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_batch_tiles(const LaunchCfg &lc, uint8_t *dst_base, uint64_t total_tiles, uint32_t tshift,
                              TileRec *tiles, const void *base_dev, hipStream_t s) {
    (void)hipGetLastError();
    return batch_tiles(lc, dst_base, total_tiles, tshift, tiles, base_dev, s, false);
}

hipError_t launch_batch_map(const s3dg_obj_desc *d, uint64_t n, const uint64_t *rec_lo, TileRec *tiles,
                            uint32_t tshift, uintptr_t base, uint64_t lead0, uint64_t first_off, hipStream_t s) {
    (void)hipGetLastError();
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_batch_map, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d, n, rec_lo, tiles, tshift,
                       (uint64_t)base, lead0, first_off);
    return hipGetLastError();
}

hipError_t launch_verify_batch_map(const s3dg_obj_desc *d, uint64_t n, const uint64_t *rec_lo, VTileRec *tiles,
                                   uint32_t tshift, hipStream_t s) {
    (void)hipGetLastError();
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_verify_batch_map, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d, n, rec_lo, tiles,
                       tshift);
    return hipGetLastError();
}

hipError_t launch_verify_recs_reset(VerifyRec *recs, uint64_t n, hipStream_t s) {
    (void)hipGetLastError();
    constexpr uint64_t per = kMaxGridX * 256;
    for (uint64_t k0 = 0; k0 < n; k0 += per) {
        const uint64_t m = n - k0 < per ? n - k0 : per;
        hipLaunchKernelGGL(k_verify_recs_reset, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, s, recs + k0, m);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// No occupancy cap, as launch_verify_stream: the pass only reads.  Every
// sub-launch starts on a tile: kVerifyMaxGrid is a multiple of every tile size.
hipError_t launch_verify_batch(int waves_per_block, const uint8_t *src_base, const VTileRec *tiles, uint64_t recs,
                               uint32_t tshift, const void *base_dev, VerifyRec *tot, VerifyRec *pobj, hipStream_t s) {
    static_assert(kVerifyMaxGrid == kMaxGridX, "the launchers' grid limit");
    (void)hipGetLastError();
    const u32x4 *b = reinterpret_cast<const u32x4 *>(base_dev);
    const uint64_t total = recs << tshift;
    for (uint64_t g0 = 0; g0 < total; g0 += kVerifyMaxGrid) {
        const dim3 g((uint32_t)((total - g0) < kVerifyMaxGrid ? (total - g0) : kVerifyMaxGrid));
        dispatch_waves(waves_per_block, [&](auto NW) {
            constexpr int nw = decltype(NW)::value;
            hipLaunchKernelGGL((k_verify_batch<nw>), g, dim3(64 * nw), 0, s, src_base, tiles, g0, tshift, b, tot,
                               pobj);
        });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ablated: the write ceiling in the tiled fill's own shape, i.e. the same
// records, grid, LDS image, barrier, stores and trailing prefetch as the fill,
// without the PRNG chain and the window patches (its caller passes ent0 = 0).
hipError_t launch_fill_uniform_tiles(const LaunchCfg &lc, uint8_t *dst, uint64_t obj_size, uint64_t stride,
                                     uint64_t n_objs, uint32_t tiles_per_obj, uint32_t tshift, uint32_t lead,
                                     uint64_t ent0, PrefixParams pp, TileRec *tiles, const void *base_dev,
                                     hipStream_t s, bool ablated) {
    (void)hipGetLastError();
    const uint64_t total_tiles = n_objs * tiles_per_obj;
    hipLaunchKernelGGL(k_tile_map_uniform, dim3((uint32_t)((total_tiles + 255) / 256)), dim3(256), 0, s, tiles,
                       total_tiles, tiles_per_obj, tshift, stride, obj_size, ent0, lead, pp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return batch_tiles(lc, dst, total_tiles, tshift, tiles, base_dev, s, ablated);
}

hipError_t launch_write_ceiling(const LaunchCfg &lc, uint8_t *dst, uint64_t len, uint32_t pattern,
                                const TileRec *thr, uint64_t nthr, hipStream_t s) {
    (void)hipGetLastError();
    const uint64_t nch = len / kBlk;
    const uint32_t pf = thr && nthr ? lc.prefetch_tiles : 0;
    for (uint64_t g0 = 0; g0 < nch; g0 += kMaxGridX) {
        const dim3 g((uint32_t)((nch - g0) < kMaxGridX ? (nch - g0) : kMaxGridX));
        dispatch_cfg(lc, [&](auto SP, auto NW) {
            constexpr int sp = decltype(SP)::value, nw = decltype(NW)::value;
            hipLaunchKernelGGL((k_write_ceiling<sp, nw>), g, dim3(64 * nw), lc.dyn_lds, s, dst, nch, g0, pattern, thr,
                               nthr, pf);
        });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace s3dg
