// s3dg_reduce.hip — what a payload takes in a store that deduplicates blocks of
// block_bytes and then compresses the blocks it keeps with a greedy LZ4
// (the definition is in include/s3dlio_gpu.h).  Pass 1 of an
// add is the measure's (s3dg_measure.hip): a 128-bit fingerprint per block into
// the handle's kept array.  Pass 2 is here: k_reduce claims every block's
// fingerprint in the handle's open-addressing table and parses only the blocks
// whose claim is new, one wave per block with the block and a 4096-entry hash
// table in LDS, as k_lz does; a duplicate block is never read again.
// k_reduce_rebuild moves the table's indices into a larger one.  Nothing here
// writes the measured buffer; results leave through vector atomics.
#include "s3dg_reduce.h"

namespace s3dg {
namespace {

typedef uint32_t rd_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long rd_slot;   // the type HIP's 64-bit atomics take

constexpr uint32_t kRdHashMul = 2654435761u;
constexpr uint32_t kRdNoSrc = 0xFFFFFFFFu;

// ---- the claim table -------------------------------------------------------------
// A slot holds the index + 1 of a kept fingerprint, 0 = empty; slots are only
// ever written by a compare-and-swap from 0, so an occupied slot never changes
// while the table lives.  The fingerprint behind a published index was written
// by pass 1 of the add that published it, a kernel that had finished before
// the publishing kernel started; that add may run on another stream, at the
// same time as this one, so this kernel may hold a stale copy of the line in
// its XCD's L2 (the line's other fingerprints are this add's own).  Hence the
// device-scope loads; no lane ever waits for another wave.
__device__ __forceinline__ uint64_t rd_load(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Fingerprint `me` of fp: true when this call entered it (the block is new),
// false when the table already holds an index with the same fingerprint (a
// duplicate, of an earlier add, of another wave's block or of another lane's).
// Two claims of one fingerprint walk the same slots, and a slot once taken
// stays taken, so the later one meets the earlier one's index.  The host keeps
// the table at most half full (reduce_table_slots), so the walk ends at an
// empty slot or at its fingerprint; the count only bounds it, and a walk that
// used it up (it cannot, under that rule) claims nothing and counts nothing.
__device__ __forceinline__ bool rd_claim(const MeasureFp *fp, uint64_t me, uint64_t *table, uint64_t slots) {
    const uint64_t lo = rd_load(&fp[me].lo), hi = rd_load(&fp[me].hi);
    uint64_t q = reduce_probe_start(lo, slots);
    for (uint64_t k = 0; k < slots; ++k, q = reduce_probe_next(q, slots)) {
        uint64_t cur = rd_load(&table[q]);
        if (cur == 0) {
            cur = atomicCAS(reinterpret_cast<rd_slot *>(&table[q]), (rd_slot)0, (rd_slot)(me + 1));
            if (cur == 0) return true;
        }
        if (rd_load(&fp[cur - 1].lo) == lo && rd_load(&fp[cur - 1].hi) == hi) return false;
    }
    return false;
}

// ---- the parse: s3dg_lz.hip's, restated (that unit's code objects stay as they are) ----

// extra length bytes of an LZ4 token nibble
__device__ __forceinline__ uint32_t rd_ext(uint32_t x) { return x < 15 ? 0u : 1u + (x - 15u) / 255u; }

// The little-endian u32 at byte i of the staged block: two aligned words and a
// funnel shift; the second word is read only where the value needs it.
__device__ __forceinline__ uint32_t rd_word(const uint32_t *W, uint32_t i, uint32_t last_dw) {
    const uint32_t k = i >> 2;
    const uint32_t w0 = W[k];
    const uint32_t w1 = W[k < last_dw ? k + 1 : last_dw];
    return (uint32_t)((((uint64_t)w1 << 32) | w0) >> ((i & 3u) * 8u));
}

__device__ __forceinline__ uint32_t rd_readlane(uint32_t v, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane((int)l));
}

__device__ __forceinline__ void rd_total(uint64_t *tot, int k, uint64_t v) {
    if (v) atomicAdd(reinterpret_cast<rd_slot *>(&tot[k]), (rd_slot)v);
}

struct RdSums {
    uint64_t blocks = 0, bytes = 0, lz = 0, stored = 0, raw = 0, matches = 0, mbytes = 0, lits = 0;
};

// One block of n bytes at bs by the wave: staged into W under k_measure's
// reading rules (a 16-byte piece is loaded whole, nontemporal, only when it
// ends at or below n, the ragged piece byte by byte, nothing else), the table
// T cleared, then the definition's steps 1-4 in one fused pass over groups of
// 64 positions.  Every branch around a ballot, a readlane or a barrier is
// wave-uniform.
__device__ __forceinline__ void rd_parse(const uint8_t *bs, uint32_t n, uint32_t block_bytes, uint32_t *lds,
                                         RdSums &t) {
    uint32_t *W = lds;
    uint16_t *T = reinterpret_cast<uint16_t *>(lds + block_bytes / 4);
    const uint32_t last_dw = block_bytes / 4 - 1;
    const uint32_t lane = threadIdx.x;
    __syncthreads();   // the previous block is read to its end before LDS is rewritten
    for (uint32_t o = lane * 16; o < n; o += 1024) {
        if (o + 16 <= n) {
            *reinterpret_cast<rd_u32x4 *>(W + o / 4) =
                __builtin_nontemporal_load(reinterpret_cast<const rd_u32x4 *>(bs + o));
        } else {
            for (uint32_t q = o; q < n; ++q) reinterpret_cast<uint8_t *>(W)[q] = bs[q];
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kLzTableBytes / 1024; ++k)
        reinterpret_cast<rd_u32x4 *>(lds + block_bytes / 4)[lane + 64 * k] = rd_u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    const uint32_t npos = n >= 4 ? n - 3 : 0;     // positions with a word: 0 .. n - 4
    const uint32_t nm = n >= 13 ? n - 11 : 0;     // positions that may start a match: 0 .. n - 12
    uint32_t p = 0, anchor = 0, size = 0, matches = 0, mbytes = 0, lits = 0;
    for (uint32_t base = 0; base < npos; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < npos;
        uint32_t v = 0, h = 0;
        if (valid) {
            v = rd_word(W, i, last_dw);
            h = (v * kRdHashMul) >> 20;
        }
        if (p < base + 64 && base < nm) {
            uint32_t s = kRdNoSrc;
            if (i < nm) {   // nm < npos
                const uint32_t c = T[h];
                if (c && rd_word(W, c - 1, last_dw) == v) s = c - 1;
                else if (i >= 1 && rd_word(W, i - 1, last_dw) == v) s = i - 1;
            }
            uint64_t m = __ballot(s != kRdNoSrc);
            if (p > base) m &= ~0ull << (p - base);
            while (m) {
                const uint32_t l = (uint32_t)__builtin_ctzll(m);
                const uint32_t i0 = base + l;
                const uint32_t s0 = rd_readlane(s, l);
                const uint32_t maxL = n - 5 - i0;   // the last five bytes are literals; >= 7
                uint32_t L = maxL;
                for (uint32_t off = 0; off < maxL; off += 256) {
                    const uint32_t e = off + 4 * lane;
                    uint32_t cnt = 0;   // equal bytes of this lane's four, none past maxL
                    if (e < maxL) {
                        const uint32_t x = rd_word(W, i0 + e, last_dw) ^ rd_word(W, s0 + e, last_dw);
                        cnt = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
                        if (cnt > maxL - e) cnt = maxL - e;
                    }
                    const uint64_t mm = __ballot(cnt < 4);
                    if (mm) {
                        const uint32_t f = (uint32_t)__builtin_ctzll(mm);
                        L = off + 4 * f + rd_readlane(cnt, f);
                        break;
                    }
                }
                const uint32_t lit = i0 - anchor;
                size += 1 + rd_ext(lit) + lit + 2 + rd_ext(L - 4);
                lits += lit;
                mbytes += L;
                ++matches;
                anchor = p = i0 + L;
                if (p >= base + 64) break;
                m &= ~0ull << (p - base);
            }
        }
        // Enter the group: T[h] = the greatest position of the group with that
        // hash.  A lane whose successor has its hash leaves the entry to it;
        // the others store, read back and store again while a smaller position
        // stands there.  Entries only grow, so the loop ends with the greatest.
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
    size += 1 + rd_ext(lit) + lit;
    lits += lit;
    t.blocks += 1;
    t.bytes += n;
    t.lz += size;
    t.stored += size < n ? size : n;
    t.raw += size >= n;
    t.matches += matches;
    t.mbytes += mbytes;
    t.lits += lits;
}

// ---- pass 2 ----------------------------------------------------------------------
// blockIdx.x = the wave; it takes blocks blockIdx.x, + gridDim.x, ... of the
// add, 64 of them at a time: lane l claims the fingerprint of the l-th of them
// (64 probe walks in flight at once: a claim is a chain of three or four
// dependent device-scope accesses, and at a high dedup ratio most blocks are
// nothing else), a ballot says which are new, and the wave loads and parses
// those one after the other.  A block whose claim found its fingerprint is
// done: its bytes are not read.  Dynamic LDS: block_bytes of staging, then the
// parse's table.
//
// BATCH false: block i = block i % bpo of object i / bpo, src at the add's
// first object.  BATCH true: block i belongs to the entry
// found by a wave-uniform binary search over the block prefix of the add's
// table; its start and its length come from the span.  Either way block i's
// fingerprint is fp[fp0 + i].
template <bool BATCH>
__device__ __forceinline__ void reduce_walk(const uint8_t *src, uint64_t stride, uint32_t block_bytes, uint64_t bpo,
                                            uint32_t last_block, const SpanEnt *ents, uint64_t live, uint64_t blocks,
                                            const MeasureFp *fp, uint64_t fp0, uint64_t *table, uint64_t slots,
                                            uint64_t *tot) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rd_lds[];
    const uint32_t lane = threadIdx.x;
    RdSums t;
    for (uint64_t b0 = blockIdx.x; b0 < blocks; b0 += 64ull * gridDim.x) {
        const uint64_t mine = b0 + (uint64_t)lane * gridDim.x;
        const bool fresh = mine < blocks && rd_claim(fp, fp0 + mine, table, slots);
        uint64_t m = __ballot(fresh);
        while (m) {
            const uint64_t bi = b0 + (uint64_t)__builtin_ctzll(m) * gridDim.x;
            m &= m - 1;
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
            rd_parse(bs, n, block_bytes, rd_lds, t);
        }
    }
    if (lane == 0) {
        rd_total(tot, kRedTotUniqueBlocks, t.blocks);
        rd_total(tot, kRedTotUniqueBytes, t.bytes);
        rd_total(tot, kRedTotLz, t.lz);
        rd_total(tot, kRedTotStored, t.stored);
        rd_total(tot, kRedTotRaw, t.raw);
        rd_total(tot, kRedTotMatches, t.matches);
        rd_total(tot, kRedTotMatchBytes, t.mbytes);
        rd_total(tot, kRedTotLiterals, t.lits);
    }
}

__global__ __launch_bounds__(64) void k_reduce(const uint8_t *src, uint64_t stride, uint32_t block_bytes, uint64_t bpo,
                                               uint32_t last_block, uint64_t blocks, const MeasureFp *fp, uint64_t fp0,
                                               uint64_t *table, uint64_t slots, uint64_t *tot) {
    reduce_walk<false>(src, stride, block_bytes, bpo, last_block, nullptr, 0, blocks, fp, fp0, table, slots, tot);
}

__global__ __launch_bounds__(64) void k_reduce_batch(const uint8_t *src_base, const SpanEnt *ents, uint64_t live,
                                                     uint32_t block_bytes, uint64_t blocks, const MeasureFp *fp,
                                                     uint64_t fp0, uint64_t *table, uint64_t slots, uint64_t *tot) {
    reduce_walk<true>(src_base, 0, block_bytes, 0, 0, ents, live, blocks, fp, fp0, table, slots, tot);
}

// ---- growth ------------------------------------------------------------------------
// One thread per slot of the old table: its index, if it has one, goes to the
// first empty slot of its fingerprint's walk in the new one.  The indices are
// distinct fingerprints, so nothing is compared.  Runs alone: the host has
// waited for the handle's adds.
__global__ __launch_bounds__(256) void k_reduce_rebuild(const uint64_t *old_table, uint64_t old_slots,
                                                        const MeasureFp *fp, uint64_t *table, uint64_t slots) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * 256) {
        const uint64_t v = old_table[i];
        if (v == 0) continue;
        uint64_t q = reduce_probe_start(fp[v - 1].lo, slots);
        for (uint64_t k = 0; k < slots; ++k, q = reduce_probe_next(q, slots))
            if (atomicCAS(reinterpret_cast<rd_slot *>(&table[q]), (rd_slot)0, (rd_slot)v) == 0) break;
    }
}

}  // namespace

hipError_t reduce_kernel_prepare() {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_reduce),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lz_lds_bytes(kLzMaxBlock));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k_reduce_batch),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lz_lds_bytes(kLzMaxBlock));
}

hipError_t launch_reduce(const LzPlan &P, const uint8_t *src, uint64_t stride, uint64_t block_bytes, int cus,
                         const ReduceState &R, uint64_t fp0, hipStream_t s) {
    (void)hipGetLastError();
    const uint64_t grid = lz_grid(P.blocks, block_bytes, cus);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reduce, dim3((uint32_t)grid), dim3(64), (size_t)lz_lds_bytes(block_bytes), s, src, stride,
                       (uint32_t)block_bytes, P.bpo, (uint32_t)P.last_block, P.blocks, R.fp, fp0, R.table, R.slots,
                       R.tot);
    return hipGetLastError();
}

hipError_t launch_reduce_batch(const uint8_t *src_base, const SpanEnt *ents, uint64_t live, uint64_t blocks,
                               uint64_t block_bytes, int cus, const ReduceState &R, uint64_t fp0, hipStream_t s) {
    (void)hipGetLastError();
    const uint64_t grid = lz_grid(blocks, block_bytes, cus);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reduce_batch, dim3((uint32_t)grid), dim3(64), (size_t)lz_lds_bytes(block_bytes), s, src_base,
                       ents, live, (uint32_t)block_bytes, blocks, R.fp, fp0, R.table, R.slots, R.tot);
    return hipGetLastError();
}

hipError_t launch_reduce_rebuild(const uint64_t *old_table, uint64_t old_slots, const ReduceState &R, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_reduce_rebuild, dim3(span_grid_for(old_slots)), dim3(256), 0, s, old_table, old_slots, R.fp,
                       R.table, R.slots);
    return hipGetLastError();
}

}  // namespace s3dg
