// s3dg_measure.hip — read-only analysis of a payload: a
// 128-bit fingerprint per block of block_bytes and the zero-byte count
// (k_measure per 4 KiB granule, k_measure_blocks per block), the exact number
// of distinct fingerprints (two stable hipCUB radix sorts on a copy, then
// k_count_distinct), and an optional byte histogram (k_byte_hist).  Nothing
// here writes the measured buffer; results leave through plain vector stores
// and vector atomics.
#include <hipcub/hipcub.hpp>

#include "s3dg_fp.h"
#include "s3dg_measure.h"

namespace s3dg {
namespace {

constexpr uint32_t kGran = (uint32_t)kMeasureGranule;

// ---- the fingerprint: s3dg_fp.h ------------------------------------------------

// 0x80 in every zero byte of x, exactly
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) {
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return (uint32_t)__builtin_popcount(~(t | x | 0x7F7F7F7Fu));
}

// Wave-wide sums without LDS traffic: a butterfly inside each row of 16 lanes
// on the VALU's DPP operand path (xor 1, xor 2, then the half-row and row
// mirrors, which add the other half's identical sums), and the four row sums
// read into scalars.  Every lane must be active.  With shuffles (ds_bpermute,
// 30 per wave for two 64-bit sums and a count) the reduction bounded the
// kernel: 4850 GB/s at 2 waves per granule against 6300 at 1.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
    return (uint64_t)dpp32<CTRL>((uint32_t)v) | ((uint64_t)dpp32<CTRL>((uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ uint32_t rows32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ uint64_t rows64(uint64_t v) {
    uint64_t s = 0;
#pragma unroll
    for (int l = 0; l < 64; l += 16)
        s += (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l) |
             ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32);
    return s;
}
__device__ __forceinline__ void wave_sums(uint64_t &s0, uint64_t &s1, uint32_t &z) {
    constexpr int kXor1 = 0xB1, kXor2 = 0x4E, kHalfMirror = 0x141, kMirror = 0x140;   // quad_perm [1,0,3,2], [2,3,0,1]
    s0 += dpp64<kXor1>(s0); s1 += dpp64<kXor1>(s1); z += dpp32<kXor1>(z);
    s0 += dpp64<kXor2>(s0); s1 += dpp64<kXor2>(s1); z += dpp32<kXor2>(z);
    s0 += dpp64<kHalfMirror>(s0); s1 += dpp64<kHalfMirror>(s1); z += dpp32<kHalfMirror>(z);
    s0 += dpp64<kMirror>(s0); s1 += dpp64<kMirror>(s1); z += dpp32<kMirror>(z);
    s0 = rows64(s0);
    s1 = rows64(s1);
    z = rows32(z);
}

// The ragged piece of an object's end, bytes below L only, zero-padded; its
// zero bytes among them are added to z.
__device__ __forceinline__ u32x4 load_ragged(const uint8_t *bs, uint32_t o, uint32_t L, uint32_t &z) {
    uint32_t dw[4] = {0u, 0u, 0u, 0u};
    for (uint32_t b = 0; o + b < L; ++b) {
        const uint32_t v = bs[o + b];
        z += v == 0;
        dw[b >> 2] |= v << (8 * (b & 3));
    }
    return u32x4{dw[0], dw[1], dw[2], dw[3]};
}

// ---- pass 1 -------------------------------------------------------------------
// blockIdx.x = 4 KiB granule gran0 + x of the object range, blockIdx.y = object
// (src already advanced to the sub-launch's first object; rec_base its first
// record).  The reading rules are k_verify_stream's: a 16-byte piece is loaded
// whole (nontemporal, the bytes are read once) only when it ends at or below
// the range's length, the ragged piece byte by byte below it, nothing else.
// One granule by a workgroup of NW waves: bytes [0, L) at bs (L in (0, 4096]),
// the granule's first piece p0 within its block, its record r.
template <int NW>
__device__ __forceinline__ void measure_granule(const uint8_t *bs, uint32_t L, uint32_t p0, uint64_t r,
                                                MeasureFp *rfp, uint32_t *rz) {
    constexpr int T = 64 * NW, SPL = 4 / NW;
    __shared__ uint64_t w0[NW], w1[NW];
    __shared__ uint32_t wz[NW];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = t & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);
    u32x4 G[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const uint32_t o = (t + k * T) * 16;
        G[k] = u32x4{0u, 0u, 0u, 0u};
        if (o + 16 <= L) G[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(bs + o));
    }
    uint64_t s0 = 0, s1 = 0;
    uint32_t z = 0;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
        const uint32_t o = (t + k * T) * 16;
        if (o >= L) continue;
        u32x4 d = G[k];
        if (o + 16 <= L) z += zero_bytes(d.x) + zero_bytes(d.y) + zero_bytes(d.z) + zero_bytes(d.w);
        else d = load_ragged(bs, o, L, z);
        fp_piece(p0 + (o >> 4), d, s0, s1);
    }
    wave_sums(s0, s1, z);   // all 64 lanes are active here
    if constexpr (NW > 1) {
        if (lane == 0) { w0[wave] = s0; w1[wave] = s1; wz[wave] = z; }
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int w = 1; w < NW; ++w) { s0 += w0[w]; s1 += w1[w]; z += wz[w]; }
        }
    }
    if (t == 0) {
        rfp[r] = MeasureFp{s0, s1};
        rz[r] = z;
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void k_measure(const uint8_t *src, uint64_t stride, uint64_t len,
                                                     uint32_t gran0, uint32_t gpb, uint64_t gpo,
                                                     uint64_t rec_base, MeasureFp *rfp, uint32_t *rz) {
    const uint32_t g = gran0 + blockIdx.x;
    const uint8_t *bs = src + (uint64_t)blockIdx.y * stride + (uint64_t)g * kGran;
    const uint64_t left = len - (uint64_t)g * kGran;              // the launcher keeps g * 4 KiB < len
    const uint32_t L = left < kGran ? (uint32_t)left : kGran;
    const uint32_t p0 = (g % gpb) * (kGran / 16);                 // the granule's first piece within its block
    measure_granule<NW>(bs, L, p0, rec_base + (uint64_t)blockIdx.y * gpo + g, rfp, rz);
}

// The batch form: a 1D grid of slots, slot w = slot
// w & (2^tshift - 1) of tile tile0 + (w >> tshift).  The tile's record is one
// wave-uniform 32-byte load in front of the payload loads; a slot past its
// object's end exits, the whole workgroup alike.
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_measure_batch(const uint8_t *src_base, const SpanTile *tiles,
                                                           uint64_t tile0, uint32_t tshift, uint32_t gpb,
                                                           MeasureFp *rfp, uint32_t *rz) {
    const uint32_t w = blockIdx.x;
    const SpanTile T = tiles[tile0 + (w >> tshift)];
    const uint32_t k = w & ((1u << tshift) - 1u);
    const uint64_t o = (uint64_t)k * kGran;
    if (o >= T.left) return;
    const uint64_t left = T.left - o;
    const uint32_t L = left < kGran ? (uint32_t)left : kGran;
    const uint32_t p0 = ((T.first + k) % gpb) * (kGran / 16);
    measure_granule<NW>(src_base + T.off + o, L, p0, T.rec + k, rfp, rz);
}

// ---- pass 2 -------------------------------------------------------------------
// The workgroup's zero counts (one per thread) summed and added to *total:
// one vector atomic per workgroup, none when the sum is zero.
__device__ __forceinline__ void add_zero_total(uint64_t z, uint64_t *total) {
    __shared__ uint64_t wsum[4];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) z += shfl_xor64(z, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = z;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (s) atomicAdd(reinterpret_cast<unsigned long long *>(total), (unsigned long long)s);
    }
}

// One block's records rfp / rz [r0, r0 + ng) summed and finalised into *out
// (blen: the block's bytes).  WAVE false: by the calling thread; true: by the
// 64 lanes of its wave.  Returns the thread's share of the block's zero bytes.
template <bool WAVE>
__device__ __forceinline__ uint64_t block_sum(const MeasureFp *rfp, const uint32_t *rz, uint64_t r0, uint32_t ng,
                                              uint64_t blen, MeasureFp *out) {
    const uint32_t lane = WAVE ? threadIdx.x & 63 : 0, step = WAVE ? 64 : 1;
    uint64_t s0 = 0, s1 = 0, z = 0;
    for (uint32_t k = lane; k < ng; k += step) {
        const MeasureFp q = rfp[r0 + k];
        s0 += q.lo;
        s1 += q.hi;
        z += rz[r0 + k];
    }
    if constexpr (WAVE) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            s0 += shfl_xor64(s0, d);
            s1 += shfl_xor64(s1, d);
        }
    }
    if (lane == 0) *out = fp_final(s0, s1, blen);
    return z;
}

// The block a thread works on.  WAVE false: one thread per block (blocks of a
// few granules); true: one wave per block (blocks of many), four per workgroup.
template <bool WAVE>
__device__ __forceinline__ uint64_t block_index() {
    return WAVE ? (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (uint64_t)blockIdx.x * 256 + threadIdx.x;
}

// The stream form: block i of the add is block i % bpo of object i / bpo.
template <bool WAVE>
__global__ __launch_bounds__(256) void k_measure_blocks(const MeasureFp *rfp, const uint32_t *rz, uint64_t nblocks,
                                                        uint64_t bpo, uint64_t gpo, uint32_t gpb,
                                                        uint64_t block_bytes, uint64_t last_block, MeasureFp *fp,
                                                        uint64_t *zero_total) {
    const uint64_t i = block_index<WAVE>();
    uint64_t z = 0;
    if (i < nblocks) {
        const uint64_t j = i / bpo, b = i - j * bpo;
        const uint64_t blen = b + 1 == bpo ? last_block : block_bytes;
        z = block_sum<WAVE>(rfp, rz, j * gpo + b * gpb, (uint32_t)((blen + kGran - 1) / kGran), blen, &fp[i]);
    }
    add_zero_total(z, zero_total);
}

// The batch form: block i of the add belongs to the entry found through the
// block prefix (a search per block: pass 2 moves 36 bytes per block); its
// length comes from the span.
template <bool WAVE>
__global__ __launch_bounds__(256) void k_measure_blocks_batch(const MeasureFp *rfp, const uint32_t *rz,
                                                              uint64_t nblocks, const SpanEnt *ents, uint64_t live,
                                                              uint32_t gpb, uint64_t block_bytes, MeasureFp *fp,
                                                              uint64_t *zero_total) {
    const uint64_t i = block_index<WAVE>();
    uint64_t z = 0;
    if (i < nblocks) {
        const SpanEnt e = ents[span_batch_find(ents, live, i)];
        const uint64_t b = i - e.b0, rest = e.size - b * block_bytes;
        const uint64_t blen = rest < block_bytes ? rest : block_bytes;
        z = block_sum<WAVE>(rfp, rz, e.g0 + b * gpb, (uint32_t)((blen + kGran - 1) / kGran), blen, &fp[i]);
    }
    add_zero_total(z, zero_total);
}

// ---- distinct count -------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fp_split(const MeasureFp *fp, uint64_t n, uint64_t *lo, uint64_t *hi) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const MeasureFp q = fp[i];
        lo[i] = q.lo;
        hi[i] = q.hi;
    }
}

// Sorted (hi, lo): positions that differ from their predecessor.
__global__ __launch_bounds__(256) void k_count_distinct(const uint64_t *lo, const uint64_t *hi, uint64_t n,
                                                        uint64_t *distinct) {
    uint64_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        c += i == 0 || lo[i] != lo[i - 1] || hi[i] != hi[i - 1];
    add_zero_total(c, distinct);
}

// ---- byte histogram ---------------------------------------------------------------
// One granule of the histogram: this thread's 16-byte piece of bytes [0, L) at
// bs under pass 1's reading rules; zero bytes to z, the others to the wave's counters.
__device__ __forceinline__ void hist_granule(const uint8_t *bs, uint32_t L, uint32_t *cnt, uint32_t &z) {
    const uint32_t o = threadIdx.x * 16;
    if (o + 16 <= L) {
        const u32x4 d = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(bs + o));
        const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            z += zero_bytes(dw[q]);
            if (dw[q] == 0) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t v = (dw[q] >> (8 * b)) & 0xFFu;
                if (v) atomicAdd(&cnt[v], 1u);
            }
        }
    } else {
        for (uint32_t b = 0; o + b < L; ++b) {
            const uint32_t v = bs[o + b];
            if (v) atomicAdd(&cnt[v], 1u);
            else ++z;
        }
    }
}

// The workgroup's counts into its slot of `part`, plain stores.
__device__ __forceinline__ void hist_flush(uint32_t (*cnt)[256], uint32_t z, uint32_t *part) {
    const uint32_t t = threadIdx.x, wave = t >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) z += __shfl_xor(z, d, 64);
    if ((t & 63) == 0) cnt[wave][0] = z;
    __syncthreads();
    part[(uint64_t)blockIdx.x * 256 + t] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
}

// A grid sized to the chip; each workgroup walks slots r = blockIdx.x,
// + gridDim.x, ... below `total`, one 16-byte piece per thread, under pass 1's
// reading rules.  locate(r, bs, L): slot r's granule is bytes [0, L) at bs, or
// false: it has none.  Zero bytes are counted in registers (half of a
// compress-2 payload: every lane would meet on one LDS word); the other values
// go to the wave's own 256 LDS counters.  One flush per workgroup into its
// slot of `part`, plain stores.
template <class Locate>
__device__ __forceinline__ void hist_walk(uint64_t total, uint32_t *part, Locate locate) {
    __shared__ uint32_t cnt[4][256];
    const uint32_t t = threadIdx.x, wave = t >> 6;
    for (int w = 0; w < 4; ++w) cnt[w][t] = 0;
    __syncthreads();
    uint32_t z = 0;
    for (uint64_t r = blockIdx.x; r < total; r += gridDim.x) {
        const uint8_t *bs;
        uint32_t L;
        if (locate(r, bs, L)) hist_granule(bs, L, cnt[wave], z);
    }
    hist_flush(cnt, z, part);
}

// The stream form: slot r is granule r % gpo of object r / gpo.
__global__ __launch_bounds__(256) void k_byte_hist(const uint8_t *src, uint64_t stride, uint64_t len, uint64_t gpo,
                                                   uint64_t total, uint32_t *part) {
    hist_walk(total, part, [&](uint64_t r, const uint8_t *&bs, uint32_t &L) {
        const uint64_t j = r / gpo, g = r - j * gpo;
        const uint64_t left = len - g * kGran;
        bs = src + j * stride + g * kGran;
        L = left < kGran ? (uint32_t)left : kGran;
        return true;
    });
}

// The batch form: slot r is slot r & (2^tshift - 1) of the add's tile
// r >> tshift; those past their object's end are skipped.
__global__ __launch_bounds__(256) void k_byte_hist_batch(const uint8_t *src_base, const SpanTile *tiles,
                                                         uint64_t total, uint32_t tshift, uint32_t *part) {
    hist_walk(total, part, [&](uint64_t r, const uint8_t *&bs, uint32_t &L) {
        const SpanTile T = tiles[r >> tshift];
        const uint64_t o = (r & ((1ull << tshift) - 1)) * kGran;
        if (o >= T.left) return false;
        const uint64_t left = T.left - o;
        bs = src_base + T.off + o;
        L = left < kGran ? (uint32_t)left : kGran;
        return true;
    });
}

// hist[b] += the workgroups' counts of value b (one thread per value).
__global__ __launch_bounds__(256) void k_hist_reduce(const uint32_t *part, uint32_t nwg, uint64_t *hist) {
    uint64_t s = 0;
    for (uint32_t w = 0; w < nwg; ++w) s += part[(uint64_t)w * 256 + threadIdx.x];
    if (s) atomicAdd(reinterpret_cast<unsigned long long *>(&hist[threadIdx.x]), (unsigned long long)s);
}

// A workgroup of k_byte_hist counts at most 2^19 granules (2^31 bytes) in its
// 32-bit counters.  The grid is 8 workgroups per CU, so one add may hold
// 2^30 granules (4 TiB) on a 256-CU chip: more than its memory.
constexpr uint64_t kHistMaxGranules = 1ull << 19;
uint32_t hist_grid_max(int cus) { return (uint32_t)(cus > 0 ? cus : 256) * 8; }

// The histogram of an add of `total` slots: walk(grid, part) launches its walk
// on a grid sized to the chip, then the workgroups' counts are added to hist.
template <class Walk>
hipError_t hist_launch(uint64_t total, int cus, void *part, uint64_t *hist, hipStream_t s, Walk walk) {
    (void)hipGetLastError();
    const uint64_t gmax = hist_grid_max(cus);
    const uint32_t grid = (uint32_t)(total < gmax ? total : gmax);
    if (total > (uint64_t)grid * kHistMaxGranules) return hipErrorInvalidValue;
    walk(dim3(grid), reinterpret_cast<uint32_t *>(part));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hist_reduce, dim3(1), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(part), grid, hist);
    return hipGetLastError();
}

// Pass 1's instantiation of kernel template K for `waves` wave64s per granule
// (1 or 4; anything else: 2) and its workgroup.
#define MEASURE_FOR_WAVES(K, waves) ((waves) == 1 ? K<1> : (waves) == 4 ? K<4> : K<2>)
dim3 waves_block(int waves) { return dim3(waves == 1 ? 64 : waves == 4 ? 256 : 128); }

// Pass 2 over `blocks` blocks of gpb granules: one thread per block (256 per
// workgroup) for blocks below kMeasureWaveBlocksFrom granules, one wave per
// block (4 per workgroup) from there on.  launch(wave, grid) enqueues it.
constexpr uint32_t kMeasureWaveBlocksFrom = 16;
template <class Launch>
hipError_t blocks_launch(uint64_t blocks, uint32_t gpb, Launch launch) {
    (void)hipGetLastError();
    const bool wave = gpb >= kMeasureWaveBlocksFrom;
    const uint64_t per = wave ? 4 : 256;   // blocks per workgroup
    const uint64_t grid = (blocks + per - 1) / per;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    launch(wave, dim3((uint32_t)grid));
    return hipGetLastError();
}

// Pass 1's records in rec: the partial fingerprints, then the zero counts of n granules.
uint32_t *record_zeros(const void *rec, uint64_t n) {
    return reinterpret_cast<uint32_t *>((uint8_t *)rec + measure_record_zero_offset(n));
}

}  // namespace

hipError_t launch_measure_granules(const MeasurePlan &P, const uint8_t *src, uint64_t stride, int waves, void *rec,
                                   hipStream_t s) {
    (void)hipGetLastError();
    MeasureFp *rfp = reinterpret_cast<MeasureFp *>(rec);
    uint32_t *rz = record_zeros(rec, P.records);
    for (uint64_t iy = 0; iy < P.ny; ++iy) {
        for (uint64_t ix = 0; ix < P.nx; ++ix) {
            uint64_t x0, y0;
            uint32_t gx, gy;
            measure_sub_launch(P, ix, iy, &x0, &gx, &y0, &gy);
            hipLaunchKernelGGL(MEASURE_FOR_WAVES(k_measure, waves), dim3(gx, gy), waves_block(waves), 0, s,
                               src + y0 * stride, stride, P.len, (uint32_t)x0, P.gpb, P.gpo, y0 * P.gpo, rfp, rz);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_measure_blocks(const MeasurePlan &P, uint64_t block_bytes, const void *rec, MeasureFp *fp,
                                 uint64_t *zero_total, hipStream_t s) {
    const MeasureFp *rfp = reinterpret_cast<const MeasureFp *>(rec);
    const uint32_t *rz = record_zeros(rec, P.records);
    return blocks_launch(P.slots, P.gpb, [&](bool wave, dim3 grid) {
        hipLaunchKernelGGL((wave ? k_measure_blocks<true> : k_measure_blocks<false>), grid, dim3(256), 0, s, rfp, rz,
                           P.slots, P.bpo, P.gpo, P.gpb, block_bytes, P.last_block, fp, zero_total);
    });
}

uint64_t measure_hist_part_bytes(int cus) { return (uint64_t)hist_grid_max(cus) * 256 * sizeof(uint32_t); }

hipError_t launch_byte_hist(const MeasurePlan &P, const uint8_t *src, uint64_t stride, int cus, void *part,
                            uint64_t *hist, hipStream_t s) {
    return hist_launch(P.records, cus, part, hist, s, [&](dim3 grid, uint32_t *slots) {
        hipLaunchKernelGGL(k_byte_hist, grid, dim3(256), 0, s, src, stride, P.len, P.gpo, P.records, slots);
    });
}

hipError_t launch_measure_granules_batch(const uint8_t *src_base, const SpanTile *tiles, uint64_t ntiles,
                                         uint32_t tshift, uint64_t granules, uint32_t gpb, int waves, void *rec,
                                         hipStream_t s) {
    (void)hipGetLastError();
    MeasureFp *rfp = reinterpret_cast<MeasureFp *>(rec);
    uint32_t *rz = record_zeros(rec, granules);
    const uint64_t subs = span_batch_sub_launches(ntiles, tshift);
    for (uint64_t i = 0; i < subs; ++i) {
        uint64_t t0, nt;
        span_batch_sub_launch(ntiles, tshift, i, &t0, &nt);
        hipLaunchKernelGGL(MEASURE_FOR_WAVES(k_measure_batch, waves), dim3((uint32_t)(nt << tshift)),
                           waves_block(waves), 0, s, src_base, tiles, t0, tshift, gpb, rfp, rz);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_measure_blocks_batch(const SpanEnt *ents, uint64_t live, uint64_t blocks, uint64_t granules,
                                       uint64_t block_bytes, const void *rec, MeasureFp *fp, uint64_t *zero_total,
                                       hipStream_t s) {
    const MeasureFp *rfp = reinterpret_cast<const MeasureFp *>(rec);
    const uint32_t *rz = record_zeros(rec, granules);
    const uint32_t gpb = (uint32_t)(block_bytes / kGran);
    return blocks_launch(blocks, gpb, [&](bool wave, dim3 grid) {
        hipLaunchKernelGGL((wave ? k_measure_blocks_batch<true> : k_measure_blocks_batch<false>), grid, dim3(256), 0, s,
                           rfp, rz, blocks, ents, live, gpb, block_bytes, fp, zero_total);
    });
}

hipError_t launch_byte_hist_batch(const uint8_t *src_base, const SpanTile *tiles, uint64_t ntiles, uint32_t tshift,
                                  int cus, void *part, uint64_t *hist, hipStream_t s) {
    const uint64_t total = ntiles << tshift;
    return hist_launch(total, cus, part, hist, s, [&](dim3 grid, uint32_t *slots) {
        hipLaunchKernelGGL(k_byte_hist_batch, grid, dim3(256), 0, s, src_base, tiles, total, tshift, slots);
    });
}

hipError_t launch_measure_distinct(const MeasureFp *fp, uint64_t n, void *work, size_t *tmp_bytes,
                                   uint64_t *distinct, hipStream_t s) {
    if (n > 0x7FFFFFFFull) return hipErrorInvalidValue;   // hipCUB counts items in an int
    const uint64_t ab = measure_sort_array_bytes(n);
    uint64_t *lo_a = reinterpret_cast<uint64_t *>(work), *hi_a = nullptr, *lo_b = nullptr, *hi_b = nullptr;
    void *tmp = nullptr;
    if (work) {
        hi_a = reinterpret_cast<uint64_t *>((uint8_t *)work + ab);
        lo_b = reinterpret_cast<uint64_t *>((uint8_t *)work + 2 * ab);
        hi_b = reinterpret_cast<uint64_t *>((uint8_t *)work + 3 * ab);
        tmp = (uint8_t *)work + 4 * ab;
    }
    if (!work) {
        *tmp_bytes = 0;
        return hipcub::DeviceRadixSort::SortPairs(nullptr, *tmp_bytes, lo_a, lo_b, hi_a, hi_b, (int)n, 0, 64, s);
    }
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_fp_split, dim3(span_grid_for(n)), dim3(256), 0, s, fp, n, lo_a, hi_a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // stable LSD passes: by the low half, then by the high half
    e = hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, lo_a, lo_b, hi_a, hi_b, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, hi_b, hi_a, lo_b, lo_a, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_count_distinct, dim3(span_grid_for(n)), dim3(256), 0, s, lo_a, hi_a, n, distinct);
    return hipGetLastError();
}

}  // namespace s3dg
