// s3dg_dev.h — what the two fill kernel units share (s3dg_block.hip, the
// 4 KiB-block family; s3dg_ks_kernels.hip, the keystream family): the device
// primitives both use, and the host helpers that turn a launch's runtime
// choices into template arguments.  Everything is local to the including unit.
#pragma once
#include "s3dg_internal.h"

#include <type_traits>

// Diagnostic builds only (tools/ablate.py): bit 0 = no window patch phase,
// bit 1 = no PRNG chain; k_keystream: bit 5 = no Xoshiro steps in the draw
// loop (counter draws), bit 6 = no jump-ahead.  Outputs of such builds are
// wrong by design.
#ifndef S3DG_ABLATE
#define S3DG_ABLATE 0
#endif

namespace s3dg {
namespace {

typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));


// 64-bit rotate as two v_alignbit_b32 (the compiler emits shifts + ors):
//   alignbit(a, b, s) = low 32 bits of ((a:b) >> s)
template <int K>
__device__ __forceinline__ uint64_t rotlk(uint64_t x) {
    static_assert(K > 0 && K < 64 && K != 32, "rotate amount");
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (K > 32) { const uint32_t t = lo; lo = hi; hi = t; }
    constexpr int k = K & 31;
    const uint32_t nhi = __builtin_amdgcn_alignbit(hi, lo, 32 - k);
    const uint32_t nlo = __builtin_amdgcn_alignbit(lo, hi, 32 - k);
    return ((uint64_t)nhi << 32) | nlo;
}
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int k) {
    return (x << k) | (x >> (64 - k));
}

// SplitMix64 step — SmallRng::seed_from_u64 expansion.
__device__ __forceinline__ uint64_t splitmix_next(uint64_t &x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Xoshiro {
    uint64_t s0, s1, s2, s3;
    __device__ __forceinline__ uint64_t next() {
        const uint64_t r = rotl64(s0 + s3, 23) + s0;
        const uint64_t t = s1 << 17;
        s2 ^= s0;
        s3 ^= s1;
        s1 ^= s2;
        s0 ^= s3;
        s2 ^= t;
        s3 = rotl64(s3, 45);
        return r;
    }
};

// 16-byte store with a cache policy (LaunchCfg::store; tools/store_lab.py):
//   kStorePlain  global_store_dwordx4 (line kept in the XCD's L2)
//   kStoreNT     ... nt  (__builtin_nontemporal_store)
//   kStoreSC1    ... sc1 (line dropped from the L2 once written)
//   kStoreNTSC1  ... nt sc1
template <int SP>
__device__ __forceinline__ void store16(uint8_t *p, u32x4 v) {
    if constexpr (SP == kStoreNT) __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(p));
    // hipcc neither models nor pads an asm store: a 16-byte store's data
    // registers must not be overwritten for 2 wait states after it issues
    // (cdna_hip_programming.md §5.7), so the pad is inside the string.
    else if constexpr (SP == kStoreSC1)
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
    else if constexpr (SP == kStoreNTSC1)
        asm volatile("global_store_dwordx4 %0, %1, off nt sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
    else *reinterpret_cast<u32x4 *>(p) = v;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // SplitMix64 output function
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// Differing bytes of one 16-byte piece (x = loaded ^ expected, known to be
// non-zero somewhere): their count, and the block offset of the lowest one.
__device__ __forceinline__ void diff_piece(u32x4 x, uint32_t o, uint32_t &cnt, uint32_t &first) {
    const uint32_t dw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int q = 3; q >= 0; --q) {
        uint32_t m = dw[q] | (dw[q] >> 4);   // bit 8b set <=> byte b of the dword differs
        m |= m >> 2;
        m |= m >> 1;
        m &= 0x01010101u;
        if (m) {
            cnt += __builtin_popcount(m);
            const uint32_t p = o + 4 * q + ((uint32_t)__builtin_ctz(m) >> 3);
            first = p < first ? p : first;
        }
    }
}

// ---- host: a launch's runtime choices as template arguments -----------------
// Each helper calls the generic lambda f with std::integral_constant values,
//   dispatch_store(lc.store, [&](auto SP) { ... k<decltype(SP)::value> ... });
// and returns what f returns.  Values outside a helper's set take its default.
template <int V>
using int_c = std::integral_constant<int, V>;

// The four store policies; default kStorePlain.
template <class F>
auto dispatch_store(int store, F &&f) {
    if (store == kStoreNT) return f(int_c<kStoreNT>{});
    if (store == kStoreSC1) return f(int_c<kStoreSC1>{});
    if (store == kStoreNTSC1) return f(int_c<kStoreNTSC1>{});
    return f(int_c<kStorePlain>{});
}

// Waves per 4 KiB block: 1, 2 or 4; default 2.
template <class F>
auto dispatch_waves(int waves, F &&f) {
    if (waves == 1) return f(int_c<1>{});
    if (waves == 4) return f(int_c<4>{});
    return f(int_c<2>{});
}

// A launch configuration's store policy x waves per block: f(SP, NW).
template <class F>
auto dispatch_cfg(const LaunchCfg &lc, F &&f) {
    return dispatch_store(lc.store, [&](auto SP) {
        return dispatch_waves(lc.waves_per_block, [&](auto NW) { return f(SP, NW); });
    });
}

// A keystream shape's draws per stage (64, 32; default 16) x waves per
// workgroup (1, 2; default 4): f(D, W).
template <class F>
auto dispatch_ks_shape(const KsShape &sh, F &&f) {
    auto waves = [&](auto D) {
        if (sh.waves == 1) return f(D, int_c<1>{});
        if (sh.waves == 2) return f(D, int_c<2>{});
        return f(D, int_c<4>{});
    };
    if (sh.draws == 64) return waves(int_c<64>{});
    if (sh.draws == 32) return waves(int_c<32>{});
    return waves(int_c<16>{});
}

// Grid sizes are 32-bit WORK-ITEM counts in the AQL dispatch packet: cap a
// launch at 2^22 workgroups per dimension (x 256 threads < 2^32).
constexpr uint64_t kMaxGridX = 1ull << 22;

}  // namespace
}  // namespace s3dg
