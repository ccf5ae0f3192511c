// s3dg_fp.h — the 128-bit fingerprint of the read-only analyses (DESIGN.md
// §5.10, §5.11), device code shared by s3dg_measure.hip (fixed blocks) and
// s3dg_chunks.hip (content-defined chunks): a block or chunk with the same
// bytes and length gets the same fingerprint from either.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "s3dg_measure.h"

namespace s3dg {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// A block is a sequence of 16-byte pieces, piece p at byte 16 p of the block
// (the ragged last piece zero-padded).  Each piece adds one term to each of
// two 64-bit sums, all adds wrapping:
//   x       = mix32(p + 0x9E3779B9)                         (a bijection of p)
//   k0 | k1<<32 = x * 0x9E3779B1 + 0x243F6A8885A308D3
//   k2 | k3<<32 = x * 0x85EBCA77 + 0x13198A2E03707344
//   k4 = rotl(k1,16) ^ k2   k5 = rotl(k3,16) ^ k0   k6 = rotl(k0,8) + k3   k7 = rotl(k2,24) + k1
//   sum0 += (d0+k0)*(d1+k1) + (d2+k2)*(d3+k3)               (32-bit adds, 32x32 -> 64 products)
//   sum1 += (d0+k4)*(d2+k5) + (d1+k6)*(d3+k7)
// (the NH construction of UMAC with per-piece, per-dword keys, in two
// pairings).  Sums commute, so lanes, waves and granules reduce in any order.
// fp_final folds in the block's byte length and avalanches.
__device__ __forceinline__ uint32_t rotl32(uint32_t v, int r) { return (v << r) | (v >> (32 - r)); }

// lowbias32: the piece keys' mixer, and the gear table of the chunker's window hash
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ void fp_piece(uint32_t p, u32x4 d, uint64_t &s0, uint64_t &s1) {
    const uint32_t x = mix32(p + 0x9E3779B9u);
    const uint64_t a = (uint64_t)x * 0x9E3779B1u + 0x243F6A8885A308D3ull;
    const uint64_t b = (uint64_t)x * 0x85EBCA77u + 0x13198A2E03707344ull;
    const uint32_t k0 = (uint32_t)a, k1 = (uint32_t)(a >> 32), k2 = (uint32_t)b, k3 = (uint32_t)(b >> 32);
    const uint32_t k4 = rotl32(k1, 16) ^ k2, k5 = rotl32(k3, 16) ^ k0;
    const uint32_t k6 = rotl32(k0, 8) + k3, k7 = rotl32(k2, 24) + k1;
    s0 += (uint64_t)(d.x + k0) * (uint64_t)(d.y + k1);
    s0 += (uint64_t)(d.z + k2) * (uint64_t)(d.w + k3);
    s1 += (uint64_t)(d.x + k4) * (uint64_t)(d.z + k5);
    s1 += (uint64_t)(d.y + k6) * (uint64_t)(d.w + k7);
}

__device__ __forceinline__ uint64_t fmix64(uint64_t h) {   // MurmurHash3's finaliser (a bijection)
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

// For a fixed length a bijection of (s0, s1); the length separates a ragged
// block from a full one that starts with the same bytes.
__device__ __forceinline__ MeasureFp fp_final(uint64_t s0, uint64_t s1, uint64_t len) {
    uint64_t a = fmix64(s0 + len * 0x9E3779B97F4A7C15ull);
    const uint64_t b = fmix64((s1 + len * 0xD6E8FEB86659FD93ull) ^ a);
    a += b;
    return MeasureFp{a, b};
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int d) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

}  // namespace
}  // namespace s3dg
