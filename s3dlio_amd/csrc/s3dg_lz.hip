// s3dg_lz.hip — the size a payload takes in a store that compresses independent
// blocks of block_bytes with a greedy LZ4 (the definition is
// in include/s3dlio_gpu.h).  k_lz: one wave per block at a time, the block and
// a 4096-entry hash table in LDS, one fused pass over groups of 64 positions;
// a grid sized to the chip walks the blocks and each wave adds its sums once.
// Nothing here writes the measured buffer; results leave through vector
// atomics.
#include "s3dg_lz.h"

namespace s3dg {
namespace {

typedef uint32_t lz_u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kLzHashMul = 2654435761u;
constexpr uint32_t kNoSrc = 0xFFFFFFFFu;

// extra length bytes of an LZ4 token nibble
__device__ __forceinline__ uint32_t lz_ext(uint32_t x) { return x < 15 ? 0u : 1u + (x - 15u) / 255u; }

// The little-endian u32 at byte i of the staged block: two aligned words (the
// lanes of a group share them, so the reads broadcast) and a funnel shift.
// last_dw is the staging area's last word; the second word is read only where
// the value needs it.
__device__ __forceinline__ uint32_t lz_word(const uint32_t *W, uint32_t i, uint32_t last_dw) {
    const uint32_t k = i >> 2;
    const uint32_t w0 = W[k];
    const uint32_t w1 = W[k < last_dw ? k + 1 : last_dw];
    return (uint32_t)((((uint64_t)w1 << 32) | w0) >> ((i & 3u) * 8u));
}

__device__ __forceinline__ uint32_t lz_readlane(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane((int)l));
}

__device__ __forceinline__ void lz_total(uint64_t *tot, int k, uint64_t v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&tot[k]), (unsigned long long)v);
}

// blockIdx.x = the wave; it takes blocks blockIdx.x, + gridDim.x, ... of the
// add (block i = block i % bpo of object i / bpo, src already at the add's
// first object).  Dynamic LDS: block_bytes of staging, then the table (entry =
// position + 1, 0 = empty).  The reading rules are k_measure's: a 16-byte
// piece is loaded whole (nontemporal, the bytes are read once) only when it
// ends at or below the block's length, the ragged piece byte by byte below it,
// nothing else.  Every branch around a ballot, a readlane or a barrier is
// wave-uniform: its condition comes from kernel arguments, ballots and
// readlanes alone.
//
// lz_walk is the body of both kernels.  BATCH false: k_lz's mapping above.
// BATCH true (k_lz_batch): block bi belongs to the entry
// found by a wave-uniform binary search over the block prefix of the add's
// table (at most about 20 scalar steps against at least 64 groups of about
// 1400 cycles); its start and its length come from the span.
template <bool BATCH>
__device__ __forceinline__ void lz_walk(const uint8_t *src, uint64_t stride, uint32_t block_bytes, uint64_t bpo,
                                        uint32_t last_block, const SpanEnt *ents, uint64_t live, uint64_t blocks,
                                        uint64_t *tot) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lz_lds[];
    uint32_t *W = lz_lds;
    uint16_t *T = reinterpret_cast<uint16_t *>(lz_lds + block_bytes / 4);
    const uint32_t last_dw = block_bytes / 4 - 1;
    const uint32_t lane = threadIdx.x;
    uint64_t t_bytes = 0, t_blocks = 0, t_lz = 0, t_stored = 0, t_raw = 0, t_matches = 0, t_mbytes = 0, t_lits = 0;
    for (uint64_t bi = blockIdx.x; bi < blocks; bi += gridDim.x) {
        const uint8_t *bs;
        uint32_t n;
        if constexpr (BATCH) {
            const SpanEnt e = ents[span_batch_find(ents, live, bi)];
            const uint64_t o = (bi - e.b0) * (uint64_t)block_bytes, rest = e.size - o;
            bs = src + e.off + o;
            n = rest < block_bytes ? (uint32_t)rest : block_bytes;
        } else {
            const uint64_t j = bi / bpo, b = bi - j * bpo;
            bs = src + j * stride + b * (uint64_t)block_bytes;
            n = b + 1 == bpo ? last_block : block_bytes;
        }
        __syncthreads();   // the previous block is read to its end before LDS is rewritten
        for (uint32_t o = lane * 16; o < n; o += 1024) {
            if (o + 16 <= n) {
                *reinterpret_cast<lz_u32x4 *>(W + o / 4) =
                    __builtin_nontemporal_load(reinterpret_cast<const lz_u32x4 *>(bs + o));
            } else {
                for (uint32_t q = o; q < n; ++q) reinterpret_cast<uint8_t *>(W)[q] = bs[q];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kLzTableBytes / 1024; ++k)
            reinterpret_cast<lz_u32x4 *>(lz_lds + block_bytes / 4)[lane + 64 * k] = lz_u32x4{0u, 0u, 0u, 0u};
        __syncthreads();

        const uint32_t npos = n >= 4 ? n - 3 : 0;     // positions with a word: 0 .. n - 4
        const uint32_t nm = n >= 13 ? n - 11 : 0;     // positions that may start a match: 0 .. n - 12
        uint32_t p = 0, anchor = 0, size = 0, matches = 0, mbytes = 0, lits = 0;
        for (uint32_t base = 0; base < npos; base += 64) {
            const uint32_t i = base + lane;
            const bool valid = i < npos;
            uint32_t v = 0, h = 0;
            if (valid) {
                v = lz_word(W, i, last_dw);
                h = (v * kLzHashMul) >> 20;
            }
            if (p < base + 64 && base < nm) {
                uint32_t s = kNoSrc;
                if (i < nm) {   // nm < npos
                    const uint32_t c = T[h];
                    if (c && lz_word(W, c - 1, last_dw) == v) s = c - 1;
                    else if (i >= 1 && lz_word(W, i - 1, last_dw) == v) s = i - 1;
                }
                uint64_t m = __ballot(s != kNoSrc);
                if (p > base) m &= ~0ull << (p - base);
                while (m) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(m);
                    const uint32_t i0 = base + l;
                    const uint32_t s0 = lz_readlane(s, l);
                    const uint32_t maxL = n - 5 - i0;   // the last five bytes are literals; >= 7
                    uint32_t L = maxL;
                    for (uint32_t off = 0; off < maxL; off += 256) {
                        const uint32_t e = off + 4 * lane;
                        uint32_t cnt = 0;   // equal bytes of this lane's four, none past maxL
                        if (e < maxL) {
                            const uint32_t x = lz_word(W, i0 + e, last_dw) ^ lz_word(W, s0 + e, last_dw);
                            cnt = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
                            if (cnt > maxL - e) cnt = maxL - e;
                        }
                        const uint64_t mm = __ballot(cnt < 4);
                        if (mm) {
                            const uint32_t f = (uint32_t)__builtin_ctzll(mm);
                            L = off + 4 * f + lz_readlane(cnt, f);
                            break;
                        }
                    }
                    const uint32_t lit = i0 - anchor;
                    size += 1 + lz_ext(lit) + lit + 2 + lz_ext(L - 4);
                    lits += lit;
                    mbytes += L;
                    ++matches;
                    anchor = p = i0 + L;
                    if (p >= base + 64) break;
                    m &= ~0ull << (p - base);
                }
            }
            // Enter the group: T[h] = the greatest position of the group with
            // that hash.  A lane whose successor has its hash leaves the entry
            // to it (a run enters once); the others store, read back and store
            // again while a smaller position stands there.  Entries only grow,
            // so whichever lane a colliding store lets win, the loop ends with
            // the greatest.
            const uint32_t hn = (uint32_t)__shfl_down((int)h, 1, 64);
            bool w = valid && !(lane < 63 && i + 1 < npos && hn == h);
            const uint16_t mine = (uint16_t)(i + 1);
            while (__ballot(w)) {
                if (w) T[h] = mine;
                __syncthreads();
                if (w) w = T[h] < mine;
            }
            __syncthreads();
        }
        const uint32_t lit = n - anchor;
        size += 1 + lz_ext(lit) + lit;
        lits += lit;
        t_bytes += n;
        t_blocks += 1;
        t_lz += size;
        t_stored += size < n ? size : n;
        t_raw += size >= n;
        t_matches += matches;
        t_mbytes += mbytes;
        t_lits += lits;
    }
    if (lane == 0) {
        lz_total(tot, kLzTotBytes, t_bytes);
        lz_total(tot, kLzTotBlocks, t_blocks);
        lz_total(tot, kLzTotLz, t_lz);
        lz_total(tot, kLzTotStored, t_stored);
        lz_total(tot, kLzTotRaw, t_raw);
        lz_total(tot, kLzTotMatches, t_matches);
        lz_total(tot, kLzTotMatchBytes, t_mbytes);
        lz_total(tot, kLzTotLiterals, t_lits);
    }
}

__global__ __launch_bounds__(64) void k_lz(const uint8_t *src, uint64_t stride, uint32_t block_bytes, uint64_t bpo,
                                           uint32_t last_block, uint64_t blocks, uint64_t *tot) {
    lz_walk<false>(src, stride, block_bytes, bpo, last_block, nullptr, 0, blocks, tot);
}

__global__ __launch_bounds__(64) void k_lz_batch(const uint8_t *src_base, const SpanEnt *ents, uint64_t live,
                                                 uint32_t block_bytes, uint64_t blocks, uint64_t *tot) {
    lz_walk<true>(src_base, 0, block_bytes, 0, 0, ents, live, blocks, tot);
}

}  // namespace

hipError_t lz_kernel_prepare() {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_lz),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lz_lds_bytes(kLzMaxBlock));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k_lz_batch), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lz_lds_bytes(kLzMaxBlock));
}

hipError_t launch_lz(const LzPlan &P, const uint8_t *src, uint64_t stride, uint64_t block_bytes, int cus,
                     uint64_t *tot, hipStream_t s) {
    (void)hipGetLastError();
    const uint64_t grid = lz_grid(P.blocks, block_bytes, cus);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lz, dim3((uint32_t)grid), dim3(64), (size_t)lz_lds_bytes(block_bytes), s, src, stride,
                       (uint32_t)block_bytes, P.bpo, (uint32_t)P.last_block, P.blocks, tot);
    return hipGetLastError();
}

hipError_t launch_lz_batch(const uint8_t *src_base, const SpanEnt *ents, uint64_t live, uint64_t blocks,
                           uint64_t block_bytes, int cus, uint64_t *tot, hipStream_t s) {
    (void)hipGetLastError();
    const uint64_t grid = lz_grid(blocks, block_bytes, cus);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lz_batch, dim3((uint32_t)grid), dim3(64), (size_t)lz_lds_bytes(block_bytes), s, src_base, ents,
                       live, (uint32_t)block_bytes, blocks, tot);
    return hipGetLastError();
}

}  // namespace s3dg
