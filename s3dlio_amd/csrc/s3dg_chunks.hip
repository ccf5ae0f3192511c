// s3dg_chunks.hip — a payload's dedup under content-defined chunking (DESIGN.md
// §5.11), read-only, in three passes per add:
//   A  k_chunk_candidates  the window hash of every byte, as a bitmap of candidate cuts
//   B  k_chunk_cuts        one wave per object walks the bitmap: (offset, length) per chunk
//   C  k_chunk_fp          one wave per chunk: §5.10's fingerprint of its bytes
// and, for s3dg_chunks_get, the exact number of distinct fingerprints and the
// bytes they stand for (two stable hipCUB radix sorts of slot indices, then
// k_chunk_count).  Nothing here writes the payload or reads a byte outside an
// object; results leave through plain vector stores and vector atomics.
#include <hipcub/hipcub.hpp>

#include "s3dg_chunks.h"
#include "s3dg_fp.h"

namespace s3dg {
namespace {

constexpr uint32_t kGran = (uint32_t)kMeasureGranule;
constexpr int kRow = 17;   // dwords per 64-byte LDS row: lanes reading at a 64-byte stride fall on distinct banks

// G[b] of the window hash
__device__ __forceinline__ uint32_t gear(uint32_t b) { return mix32(b + 0x9E3779B9u); }

// Bytes [o, o + 16) of the object at bs, o a multiple of 16 below L: loaded
// whole when they end at or below L, else byte by byte below L, zero-padded.
__device__ __forceinline__ u32x4 load_piece(const uint8_t *bs, uint64_t o, uint64_t L) {
    if (o + 16 <= L) return *reinterpret_cast<const u32x4 *>(bs + o);
    uint32_t dw[4] = {0u, 0u, 0u, 0u};
    for (uint32_t b = 0; o + b < L; ++b) dw[b >> 2] |= (uint32_t)bs[o + b] << (8 * (b & 3));
    return u32x4{dw[0], dw[1], dw[2], dw[3]};
}

// Sum over the wave, in every lane.
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += shfl_xor64(v, d);
    return v;
}

__device__ __forceinline__ void atomic_add64(uint64_t *p, uint64_t v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

// ---- pass A ---------------------------------------------------------------------
// One granule by one wave, under k_measure's reading rules: granule g of its
// object at bs (nothing before granule 0 is read), `left` > 0 bytes from bs to
// the object's end.  The granule and the 32 bytes before it (the same
// object's, zeros before its first byte) are staged in LDS as rows of 64
// bytes; lane l seeds h over the 31 bytes before its run (row l) and rolls it
// over the run (row l + 1): h = (h << 1) + G[byte], so after 32 bytes nothing
// older is left in the 32-bit word.  Positions below 31 of the object and at or
// above its length are never candidates.  The granule's 64 bitmap words go to
// bitmap[w0] on and its number of candidates to gcnt[gi] (summed by
// k_chunk_sum: an atomic per granule on one word took 12 ns each, 25 ms for
// 8 GiB).
template <bool TAB>
__device__ __forceinline__ void chunk_granule(const uint8_t *bs, uint32_t g, uint64_t left, uint32_t shift,
                                              uint64_t *bitmap, uint64_t w0, uint32_t *gcnt, uint64_t gi) {
    __shared__ uint32_t rows[65 * kRow];
    __shared__ uint32_t gtab[TAB ? 256 : 1];
    const uint32_t lane = threadIdx.x;
    const uint32_t L = left < kGran ? (uint32_t)left : kGran;
    if constexpr (TAB) {
#pragma unroll
        for (int k = 0; k < 4; ++k) gtab[lane + 64 * k] = gear(lane + 64 * k);
    }
    if (lane < 2) {   // row 0, bytes 32..63: the 32 bytes before the granule
        u32x4 d = u32x4{0u, 0u, 0u, 0u};
        if (g > 0) d = *reinterpret_cast<const u32x4 *>(bs - 32 + 16 * lane);
        uint32_t *r = rows + 8 + 4 * lane;
        r[0] = d.x; r[1] = d.y; r[2] = d.z; r[3] = d.w;
    }
    u32x4 D[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t o = (lane + 64 * k) * 16;
        D[k] = u32x4{0u, 0u, 0u, 0u};
        if (o + 16 <= L) D[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(bs + o));
        else if (o < L) D[k] = load_piece(bs, o, L);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t q = lane + 64 * k;
        uint32_t *r = rows + (1 + (q >> 2)) * kRow + (q & 3) * 4;
        r[0] = D[k].x; r[1] = D[k].y; r[2] = D[k].z; r[3] = D[k].w;
    }
    __syncthreads();
    auto G = [&](uint32_t b) -> uint32_t {
        if constexpr (TAB) return gtab[b];
        else return gear(b);
    };
    const uint32_t *prev = rows + lane * kRow, *own = prev + kRow;
    uint32_t h = 0;
#pragma unroll
    for (int j = 8; j < 16; ++j) {
        const uint32_t w = prev[j];
#pragma unroll
        for (int b = (j == 8 ? 1 : 0); b < 4; ++b) h = (h << 1) + G((w >> (8 * b)) & 0xFFu);
    }
    uint32_t m[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t w = own[j];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            h = (h << 1) + G((w >> (8 * b)) & 0xFFu);
            m[j >> 3] |= (uint32_t)((h >> shift) == 0) << ((4 * j + b) & 31);
        }
    }
    uint64_t bits = (uint64_t)m[0] | ((uint64_t)m[1] << 32);
    if (g == 0 && lane == 0) bits &= ~0ull << 31;          // a window needs 32 bytes of the object
    const uint32_t o = lane * 64;
    if (o >= L) bits = 0;
    else if (L - o < 64) bits &= ~0ull >> (64 - (L - o));  // nothing at or beyond the object's end
    bitmap[w0 + lane] = bits;
    const uint64_t c = wave_sum64((uint64_t)__builtin_popcountll(bits));
    if (lane == 0) gcnt[gi] = (uint32_t)c;
}

// The stream form: blockIdx.x = 4 KiB granule gran0 + x, blockIdx.y = object
// (src, bitmap and gcnt already advanced to the sub-launch's first object).
template <bool TAB>
__global__ __launch_bounds__(64) void k_chunk_candidates(const uint8_t *src, uint64_t stride, uint64_t len,
                                                         uint32_t gran0, uint64_t wpo, uint32_t shift,
                                                         uint64_t gpo, uint64_t *bitmap, uint32_t *gcnt) {
    const uint32_t g = gran0 + blockIdx.x;
    const uint8_t *bs = src + (uint64_t)blockIdx.y * stride + (uint64_t)g * kGran;
    const uint64_t left = len - (uint64_t)g * kGran;              // the launcher keeps g * 4 KiB < len
    chunk_granule<TAB>(bs, g, left, shift, bitmap, (uint64_t)blockIdx.y * wpo + (uint64_t)g * 64, gcnt,
                       (uint64_t)blockIdx.y * gpo + g);
}

// The batch form: k_measure_batch's 1D grid of tile slots.
// Granule g of the add (its entry's g0 + its index in the object) owns bitmap
// words [64 g, 64 g + 64) and gcnt[g]; a dead slot exits.
template <bool TAB>
__global__ __launch_bounds__(64) void k_chunk_candidates_batch(const uint8_t *src_base, const SpanTile *tiles,
                                                               uint64_t tile0, uint32_t tshift, uint32_t shift,
                                                               uint64_t *bitmap, uint32_t *gcnt) {
    const uint32_t w = blockIdx.x;
    const SpanTile T = tiles[tile0 + (w >> tshift)];
    const uint32_t k = w & ((1u << tshift) - 1u);
    const uint64_t o = (uint64_t)k * kGran;
    if (o >= T.left) return;
    chunk_granule<TAB>(src_base + T.off + o, T.first + k, T.left - o, shift, bitmap, (T.rec + k) * 64, gcnt,
                       T.rec + k);
}

// *total += the sum of v[0, n): one vector atomic per workgroup.
__global__ __launch_bounds__(256) void k_chunk_sum(const uint32_t *v, uint64_t n, uint64_t *total) {
    __shared__ uint64_t ws[4];
    uint64_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) c += v[i];
    c = wave_sum64(c);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        c = ws[0] + ws[1] + ws[2] + ws[3];
        if (c) atomic_add64(total, c);
    }
}

// ---- pass B ---------------------------------------------------------------------
// One wave per object, four per workgroup.  From a chunk's start s the wave
// reads the bitmap words of [s + min - 1, s + max - 1] (clipped to the object),
// 64 words = 4096 positions at a time, one per lane; the first lane with a bit
// and that word's lowest bit give the cut.  None: a forced cut at max bytes
// when the object holds that many from s, else the object's end closes the
// chunk.  Everything that steers the loop is wave-uniform.
// Object j of len bytes by one wave: its bitmap bm, its records from slot r0 on, its count to cnt[j].
__device__ __forceinline__ void chunk_walk(const uint64_t *bm, uint64_t j, uint64_t len, uint64_t minb, uint64_t maxb,
                                           uint64_t r0, uint64_t *roff, uint32_t *rlen, uint32_t *cnt,
                                           uint64_t *tot) {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t s = 0, n = 0, forced = 0;
    while (s < len) {
        uint64_t e = len - 1;
        const uint64_t lo = s + minb - 1;
        if (lo < len) {
            const uint64_t cap = s + maxb - 1;
            const uint64_t hi = cap < len - 1 ? cap : len - 1;
            const uint64_t wlo = lo >> 6, whi = hi >> 6;
            bool found = false;
            for (uint64_t w0 = wlo; w0 <= whi; w0 += 64) {
                const uint64_t w = w0 + lane;
                uint64_t v = 0;
                if (w <= whi) {
                    v = bm[w];
                    if (w == wlo) v &= ~0ull << (lo & 63);
                    if (w == whi) v &= ~0ull >> (63 - (hi & 63));
                }
                const uint64_t ballot = __ballot(v != 0);
                if (ballot) {
                    const int fl = __builtin_ctzll(ballot);
                    const uint32_t vl = __shfl((uint32_t)v, fl, 64), vh = __shfl((uint32_t)(v >> 32), fl, 64);
                    const uint64_t vv = (uint64_t)vl | ((uint64_t)vh << 32);
                    e = (w0 + (uint64_t)fl) * 64 + (uint64_t)__builtin_ctzll(vv);
                    found = true;
                    break;
                }
            }
            if (!found) {
                e = hi;
                forced += cap < len;   // the chunk has max bytes; at the object's end it would merely be closed
            }
        }
        if (lane == 0) {
            roff[r0 + n] = s;
            rlen[r0 + n] = (uint32_t)(e - s + 1);
        }
        ++n;
        s = e + 1;
    }
    if (lane == 0) {
        cnt[j] = (uint32_t)n;
        atomic_add64(&tot[kChunkTotChunks], n);
        if (forced) atomic_add64(&tot[kChunkTotForced], forced);
    }
}

__global__ __launch_bounds__(256) void k_chunk_cuts(const uint64_t *bitmap, uint64_t n_objs, uint64_t len,
                                                    uint64_t wpo, uint64_t rpo, uint64_t minb, uint64_t maxb,
                                                    uint64_t *roff, uint32_t *rlen, uint32_t *cnt, uint64_t *tot) {
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_objs) return;
    chunk_walk(bitmap + j * wpo, j, len, minb, maxb, j * rpo, roff, rlen, cnt, tot);
}

// The batch form: one wave per entry, with its own length, its bitmap at the
// granule prefix and its records at the slot prefix.  It leaves its index in
// own[] for every slot of the entry, so pass C finds a slot's object with one
// load (a search per slot over the slot prefix cost pass C 4.2 ms against the
// stream form's 2.3 on 1024 x 8 MiB).
__global__ __launch_bounds__(256) void k_chunk_cuts_batch(const uint64_t *bitmap, const SpanEnt *ents, uint64_t live,
                                                          uint64_t minb, uint64_t maxb, uint64_t *roff,
                                                          uint32_t *rlen, uint32_t *cnt, uint32_t *own,
                                                          uint64_t *tot) {
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= live) return;
    const SpanEnt e = ents[j];
    const uint64_t slots = (e.size + minb - 1) / minb + 1;   // span_obj_slots
    for (uint64_t k = threadIdx.x & 63; k < slots; k += 64) own[e.s0 + k] = (uint32_t)j;
    chunk_walk(bitmap + e.g0 * 64, j, e.size, minb, maxb, e.s0, roff, rlen, cnt, tot);
}

// ---- pass C ---------------------------------------------------------------------
// Bytes sh .. sh + 15 of the 32 bytes a | b, sh wave-uniform in [1, 15].
__device__ __forceinline__ u32x4 shift_bytes(u32x4 a, u32x4 b, uint32_t sh) {
    const uint32_t bsh = sh & 3;
    uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, r[4];
    switch (sh >> 2) {
    case 0:
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], bsh);
        break;
    case 1:
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = __builtin_amdgcn_alignbyte(w[i + 2], w[i + 1], bsh);
        break;
    case 2:
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = __builtin_amdgcn_alignbyte(w[i + 3], w[i + 2], bsh);
        break;
    default:
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = __builtin_amdgcn_alignbyte(w[i + 4], w[i + 3], bsh);
        break;
    }
    return u32x4{r[0], r[1], r[2], r[3]};
}

// The first n bytes of d (n in [1, 15]), the rest zero.
__device__ __forceinline__ u32x4 keep_bytes(u32x4 d, uint32_t n) {
    uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = (int)n - 4 * i;   // bytes of dword i to keep
        w[i] = k >= 4 ? w[i] : (k <= 0 ? 0u : w[i] & ((1u << (8 * k)) - 1u));
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

// One wave per record slot, four per workgroup.  Piece p of the chunk at
// offset `off` of its object is bytes off + 16 p ..: two aligned 16-byte loads
// (the object starts 16-byte aligned) combined by a byte shift, one when the
// chunk itself starts aligned.  Loads follow load_piece's rule against the
// object's length; the chunk's last piece is cut to the chunk's own bytes.
// Slot `slot` by one wave: its chunk of the len-byte object at ob, or no chunk (live false).
__device__ __forceinline__ void chunk_fp_slot(const uint8_t *ob, uint64_t len, uint64_t slot, bool live,
                                              const uint64_t *roff, const uint32_t *rlen, MeasureFp *fp,
                                              uint32_t *flen) {
    const uint32_t lane = threadIdx.x & 63;
    if (!live) {
        if (lane == 0) flen[slot] = 0;
        return;
    }
    const uint64_t off = roff[slot];
    const uint32_t L = rlen[slot];
    const uint32_t sh = (uint32_t)off & 15u;
    const uint64_t base = off - sh;
    const uint32_t np = (L + 15) / 16;
    uint64_t s0 = 0, s1 = 0;
    for (uint32_t p = lane; p < np; p += 64) {
        const uint64_t o = base + (uint64_t)p * 16;
        u32x4 d = load_piece(ob, o, len);
        if (sh) {
            u32x4 b = u32x4{0u, 0u, 0u, 0u};
            if (o + 16 < len) b = load_piece(ob, o + 16, len);
            d = shift_bytes(d, b, sh);
        }
        const uint32_t rem = L - p * 16;
        if (rem < 16) d = keep_bytes(d, rem);
        fp_piece(p, d, s0, s1);
    }
    s0 = wave_sum64(s0);
    s1 = wave_sum64(s1);
    if (lane == 0) {
        fp[slot] = fp_final(s0, s1, L);
        flen[slot] = L;
    }
}

__global__ __launch_bounds__(256) void k_chunk_fp(const uint8_t *src, uint64_t stride, uint64_t len, uint64_t slots,
                                                  uint64_t rpo, const uint64_t *roff, const uint32_t *rlen,
                                                  const uint32_t *cnt, MeasureFp *fp, uint32_t *flen) {
    const uint64_t slot = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= slots) return;
    const uint64_t j = slot / rpo, k = slot - j * rpo;
    chunk_fp_slot(src + j * stride, len, slot, k < cnt[j], roff, rlen, fp, flen);
}

// The batch form: the slot's entry is the one pass B left in own[]; a slot
// past its object's count holds no chunk.
__global__ __launch_bounds__(256) void k_chunk_fp_batch(const uint8_t *src_base, const SpanEnt *ents, uint64_t slots,
                                                        const uint64_t *roff, const uint32_t *rlen,
                                                        const uint32_t *cnt, const uint32_t *own, MeasureFp *fp,
                                                        uint32_t *flen) {
    const uint64_t slot = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= slots) return;
    const uint32_t j = own[slot];
    const SpanEnt e = ents[j];
    chunk_fp_slot(src_base + e.off, e.size, slot, slot - e.s0 < cnt[j], roff, rlen, fp, flen);
}

// ---- distinct count ---------------------------------------------------------------
// Keys of the two sorts; a slot without a chunk sorts last.
__global__ __launch_bounds__(256) void k_chunk_keys_lo(const MeasureFp *fp, const uint32_t *flen, uint64_t n,
                                                       uint64_t *key, uint32_t *idx) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        key[i] = flen[i] ? fp[i].lo : ~0ull;
        idx[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void k_chunk_keys_hi(const MeasureFp *fp, const uint32_t *flen, uint64_t n,
                                                       const uint32_t *idx, uint64_t *key) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t a = idx[i];
        key[i] = flen[a] ? fp[a].hi : ~0ull;
    }
}

// Slots in (hi, lo) order: a chunk whose fingerprint differs from its
// predecessor's is the first of its kind; count it and its bytes.
__global__ __launch_bounds__(256) void k_chunk_count(const MeasureFp *fp, const uint32_t *flen, uint64_t n,
                                                     const uint32_t *idx, uint64_t *tot) {
    __shared__ uint64_t wc[4], wb[4];
    uint64_t c = 0, bytes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t a = idx[i];
        const uint32_t la = flen[a];
        if (!la) continue;
        bool head = i == 0;
        if (!head) {
            const uint32_t b = idx[i - 1];
            const MeasureFp p = fp[b], q = fp[a];
            head = !flen[b] || p.lo != q.lo || p.hi != q.hi;
        }
        c += head;
        bytes += head ? la : 0;
    }
    c = wave_sum64(c);
    bytes = wave_sum64(bytes);
    if ((threadIdx.x & 63) == 0) { wc[threadIdx.x >> 6] = c; wb[threadIdx.x >> 6] = bytes; }
    __syncthreads();
    if (threadIdx.x == 0) {
        c = wc[0] + wc[1] + wc[2] + wc[3];
        bytes = wb[0] + wb[1] + wb[2] + wb[3];
        if (c) {
            atomic_add64(&tot[kChunkTotUnique], c);
            atomic_add64(&tot[kChunkTotUniqueBytes], bytes);
        }
    }
}

}  // namespace

hipError_t launch_chunk_passes(const ChunkPlan &P, const ChunkSrc &src, uint32_t shift, bool table,
                               uint64_t min_bytes, uint64_t max_bytes, void *scratch, MeasureFp *fp, uint32_t *flen,
                               uint64_t *tot, hipEvent_t *tev, const char **step, hipStream_t s) {
    (void)hipGetLastError();
    uint8_t *sc = reinterpret_cast<uint8_t *>(scratch);
    uint64_t *bitmap = reinterpret_cast<uint64_t *>(sc);
    uint64_t *roff = reinterpret_cast<uint64_t *>(sc + P.off_offset);
    uint32_t *rlen = reinterpret_cast<uint32_t *>(sc + P.len_offset);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(sc + P.cnt_offset);
    uint32_t *gcnt = reinterpret_cast<uint32_t *>(sc + P.gcnt_offset);
    uint32_t *own = reinterpret_cast<uint32_t *>(sc + P.own_offset);
    const bool batch = src.ents != nullptr;
    hipError_t e;
    int ev = 0;
    // the next of tev's events, between two passes
    auto mark = [&]() -> hipError_t {
        *step = "hipEventRecord(chunks pass)";
        return tev ? hipEventRecord(tev[ev++], s) : hipSuccess;
    };
    if ((e = mark()) != hipSuccess) return e;
    *step = "launch k_chunk_candidates";
    if (batch) {
        const uint64_t subs = span_batch_sub_launches(src.ntiles, src.tshift);
        for (uint64_t i = 0; i < subs; ++i) {
            uint64_t t0, nt;
            span_batch_sub_launch(src.ntiles, src.tshift, i, &t0, &nt);
            hipLaunchKernelGGL((table ? k_chunk_candidates_batch<true> : k_chunk_candidates_batch<false>),
                               dim3((uint32_t)(nt << src.tshift)), dim3(64), 0, s, src.base, src.tiles, t0, src.tshift,
                               shift, bitmap, gcnt);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    } else {
        for (uint64_t iy = 0; iy < P.ny; ++iy) {
            for (uint64_t ix = 0; ix < P.nx; ++ix) {
                uint64_t x0, y0;
                uint32_t gx, gy;
                chunk_sub_launch(P, ix, iy, &x0, &gx, &y0, &gy);
                hipLaunchKernelGGL((table ? k_chunk_candidates<true> : k_chunk_candidates<false>), dim3(gx, gy),
                                   dim3(64), 0, s, src.base + y0 * src.stride, src.stride, P.len, (uint32_t)x0, P.wpo,
                                   shift, P.gpo, bitmap + y0 * P.wpo, gcnt + y0 * P.gpo);
                if ((e = hipGetLastError()) != hipSuccess) return e;
            }
        }
    }
    hipLaunchKernelGGL(k_chunk_sum, dim3(span_grid_for(P.granules)), dim3(256), 0, s, gcnt, P.granules,
                       &tot[kChunkTotCandidates]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = mark()) != hipSuccess) return e;
    *step = "launch k_chunk_cuts";
    const uint64_t gb = (P.n_objs + 3) / 4, gc = (P.slots + 3) / 4;
    if (gb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (batch)
        hipLaunchKernelGGL(k_chunk_cuts_batch, dim3((uint32_t)gb), dim3(256), 0, s, bitmap, src.ents, P.n_objs,
                           min_bytes, max_bytes, roff, rlen, cnt, own, tot);
    else
        hipLaunchKernelGGL(k_chunk_cuts, dim3((uint32_t)gb), dim3(256), 0, s, bitmap, P.n_objs, P.len, P.wpo, P.rpo,
                           min_bytes, max_bytes, roff, rlen, cnt, tot);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = mark()) != hipSuccess) return e;
    *step = "launch k_chunk_fp";
    if (gc > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (batch)
        hipLaunchKernelGGL(k_chunk_fp_batch, dim3((uint32_t)gc), dim3(256), 0, s, src.base, src.ents, P.slots, roff,
                           rlen, cnt, own, fp, flen);
    else
        hipLaunchKernelGGL(k_chunk_fp, dim3((uint32_t)gc), dim3(256), 0, s, src.base, src.stride, P.len, P.slots, P.rpo,
                           roff, rlen, cnt, fp, flen);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return mark();
}

hipError_t launch_chunk_distinct(const MeasureFp *fp, const uint32_t *flen, uint64_t n, void *work, size_t *tmp_bytes,
                                 uint64_t *tot, hipStream_t s) {
    if (n > kChunkMaxSlots) return hipErrorInvalidValue;   // hipCUB counts items in an int
    const uint64_t kb = chunk_sort_key_bytes(n), ib = chunk_sort_idx_bytes(n);
    uint8_t *w = reinterpret_cast<uint8_t *>(work);
    uint64_t *key_a = reinterpret_cast<uint64_t *>(w), *key_b = nullptr;
    uint32_t *idx_a = nullptr, *idx_b = nullptr;
    if (!work) {
        *tmp_bytes = 0;
        return hipcub::DeviceRadixSort::SortPairs(nullptr, *tmp_bytes, key_a, key_b, idx_a, idx_b, (int)n, 0, 64, s);
    }
    key_b = reinterpret_cast<uint64_t *>(w + kb);
    idx_a = reinterpret_cast<uint32_t *>(w + 2 * kb);
    idx_b = reinterpret_cast<uint32_t *>(w + 2 * kb + ib);
    void *tmp = w + 2 * kb + 2 * ib;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_chunk_keys_lo, dim3(span_grid_for(n)), dim3(256), 0, s, fp, flen, n, key_a, idx_a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // stable LSD passes: by the low half, then by the high half
    e = hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, key_a, key_b, idx_a, idx_b, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_chunk_keys_hi, dim3(span_grid_for(n)), dim3(256), 0, s, fp, flen, n, idx_b, key_a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortPairs(tmp, *tmp_bytes, key_a, key_b, idx_b, idx_a, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_chunk_count, dim3(span_grid_for(n)), dim3(256), 0, s, fp, flen, n, idx_a, tot);
    return hipGetLastError();
}

}  // namespace s3dg
