// s3dg_tfrecord_search.hip — the kernels of s3dg_tfrecord_index_search_batch
// (DESIGN.md §5.5.3): k_tfrecord_walk's results with parallelism inside a
// stream.  The rules are s3dg_tfrecord_search_plan.h's; here is how the work is
// split.
//
// k_tfs_candidates  the bandwidth-shaped pass.  A 256-thread workgroup takes a
//     tile of 16 KiB positions plus the 11 bytes behind it, staged through LDS
//     by 16-byte loads (the pieces that hold a stream's first and last bytes by
//     the dwords that hold them, nothing beyond).  A wave tests 64 neighbouring
//     positions per step, a lane one position: four LDS dwords (neighbouring
//     lanes share them, so the reads are conflict-free), a byte shift, the fit
//     as two compares, and only for what fits the length CRC from eight byte
//     tables in LDS.  The ballot of a step is the tile's bitmap word; lane i
//     keeps step i's, so after 64 steps the wave stores 64 words at once, with
//     their prefix inside the tile from one wave scan and the tile's count.
// k_tfs_link        a thread per bitmap word: entry, next and the 1-link pair
//     of each candidate in it.
// k_tfs_double      a thread per node, once per round.
// k_tfs_anchor      a wave per stream: tfs_anchor_walk, the only serial part.
// k_tfs_fill        a thread per anchor: tfs_fill.
#include <hipcub/hipcub.hpp>

#include "s3dg_internal.h"
#include "s3dg_tfrecord_search_plan.h"

namespace s3dg {
namespace {

constexpr uint32_t kPieces = kTfsTile / 16 + 2;   // a tile at any alignment plus 11 bytes

__global__ __launch_bounds__(256) void k_tfs_candidates(const uint8_t *__restrict__ base,
                                                        const s3dg_tfrecord_stream *__restrict__ st,
                                                        const uint64_t *__restrict__ tile0, uint64_t n, uint64_t tiles,
                                                        uint64_t *__restrict__ bm, uint16_t *__restrict__ wpre,
                                                        uint64_t *__restrict__ tbase) {
    __shared__ uint4 L[kPieces];
    __shared__ uint32_t tab[kTfsCrcTabWords];
    __shared__ uint32_t wsum[4];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (uint32_t e = t; e < kTfsCrcTabWords; e += 256) tab[e] = tfs_crc_tab_entry(e);
    const uint32_t K = tfs_crc_const();
    if (blockIdx.x == 0 && t == 0) tbase[tiles] = 0;   // the exclusive sum leaves the call's count here
    const uint32_t *Lw = reinterpret_cast<const uint32_t *>(L);
    for (uint64_t g = blockIdx.x; g < tiles; g += gridDim.x) {
        __syncthreads();   // the tables; the tile before is read
        const uint64_t k = tfs_find_stream(tile0, n, g);
        const s3dg_tfrecord_stream Sd = st[k];
        const uint64_t tstart = (g - tile0[k]) * kTfsTile, avail = Sd.bytes - tstart;
        const uint64_t win = avail < kTfsTile + 11 ? avail : kTfsTile + 11;
        const uintptr_t s = reinterpret_cast<uintptr_t>(base) + Sd.off + tstart, e = s + win;
        const uint32_t a = (uint32_t)(s & 15u);
        for (uint32_t i = t; i < kPieces; i += 256) {
            const uintptr_t pa = s - a + 16ull * i;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (pa >= s && pa + 16 <= e) {
                v = *reinterpret_cast<const uint4 *>(pa);
            } else if (pa + 16 > s && pa < e) {   // an end piece: the dwords that hold bytes of the window
                auto dw = [&](uint32_t d) -> uint32_t {
                    const uintptr_t da = pa + 4 * d;
                    return da + 4 > s && da < e ? *reinterpret_cast<const uint32_t *>(da) : 0u;
                };
                v = make_uint4(dw(0), dw(1), dw(2), dw(3));
            }
            L[i] = v;
        }
        __syncthreads();
        uint64_t mine = 0;
        for (uint32_t it = 0; it < 64; ++it) {
            const uint32_t x = (wave * 64 + it) * 64 + lane, bo = a + x, d = bo >> 2, sft = bo & 3u;
            const uint32_t w0 = Lw[d], w1 = Lw[d + 1], w2 = Lw[d + 2], w3 = Lw[d + 3];
            const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sft), hi = __builtin_amdgcn_alignbyte(w2, w1, sft);
            const uint32_t crc = __builtin_amdgcn_alignbyte(w3, w2, sft);
            const uint64_t len = (uint64_t)lo | ((uint64_t)hi << 32);
            bool c = false;
            if (x < avail && tfs_fits(avail - x, len)) c = tfs_len_mcrc_tab(tab, K, len) == crc;
            const uint64_t word = __ballot(c);
            if (lane == it) mine = word;
        }
        const uint32_t cnt = (uint32_t)__builtin_popcountll(mine);
        uint32_t inc = cnt;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            before += w < wave ? wsum[w] : 0u;
            total += wsum[w];
        }
        const uint64_t wi = g * kTfsTileWords + wave * 64 + lane;
        bm[wi] = mine;
        wpre[wi] = (uint16_t)(before + inc - cnt);   // below the tile's 16384 positions
        if (t == 0) tbase[g] = total;
    }
}

__global__ __launch_bounds__(256) void k_tfs_link(const uint8_t *__restrict__ base, const s3dg_tfrecord_stream *__restrict__ st,
                                                  const uint64_t *__restrict__ tile0, uint64_t n, uint64_t words, TfsMap M,
                                                  TfsEnt *__restrict__ ent, uint32_t *__restrict__ next,
                                                  TfsHop *__restrict__ hop) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    uint64_t word = M.bm[w];
    if (!word) return;
    const uint64_t g = w / kTfsTileWords, k = tfs_find_stream(tile0, n, g);
    const s3dg_tfrecord_stream Sd = st[k];
    const uint64_t p0 = (g - tile0[k]) * kTfsTile + (w % kTfsTileWords) * 64;
    uint32_t x = (uint32_t)(M.tbase[g] + M.wpre[w]);
    for (; word; word &= word - 1, ++x) {
        const uint64_t pos = p0 + (uint32_t)__builtin_ctzll(word);
        uint64_t len;
        uint32_t crc;
        tfs_header(base + Sd.off + pos, &len, &crc);
        const uint32_t nx = tfs_link(M, tile0[k], Sd.bytes, pos, len + kTfrFraming);
        ent[x] = TfsEnt{pos, len + kTfrFraming};
        next[x] = nx;
        hop[x] = tfs_hop0(x, nx);
    }
}

__global__ __launch_bounds__(256) void k_tfs_double(const TfsHop *__restrict__ in, TfsHop *__restrict__ out, uint32_t nodes,
                                                    uint32_t full) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < nodes) out[x] = tfs_double(in, (uint32_t)x, full);
}

// One wave per stream (four per workgroup), every lane following the same
// chain; lane 0 stores.
__global__ __launch_bounds__(256) void k_tfs_anchor(const uint8_t *__restrict__ base, uint8_t *__restrict__ idx,
                                                    const s3dg_tfrecord_stream *__restrict__ st,
                                                    const uint64_t *__restrict__ tile0, uint64_t n, TfsMap M,
                                                    const TfsEnt *__restrict__ ent, const uint32_t *__restrict__ next,
                                                    const TfsHop *__restrict__ hop, TfsAnchor *__restrict__ anch,
                                                    s3dg_tfrecord_walk_result *__restrict__ res) {
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t k = (uint64_t)blockIdx.x * 4 + wave; k < n; k += (uint64_t)gridDim.x * 4) {
        const s3dg_tfrecord_stream Sd = st[k];
        const s3dg_tfrecord_walk_result R = tfs_anchor_walk(base + Sd.off, Sd, M, tile0[k], ent, next, hop, anch, idx, lane == 0);
        if (lane == 0) res[k] = R;
    }
}

__global__ __launch_bounds__(256) void k_tfs_fill(const TfsAnchor *__restrict__ anch, uint32_t nodes,
                                                  const TfsEnt *__restrict__ ent, const uint32_t *__restrict__ next,
                                                  uint8_t *__restrict__ idx) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nodes) return;
    const TfsAnchor A = anch[i];
    if (A.count) tfs_fill(A, ent, next, idx);
}

__global__ __launch_bounds__(256) void k_tfs_clear(TfsAnchor *__restrict__ anch, uint32_t nodes) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nodes) anch[i] = TfsAnchor{0, 0, 0};
}

inline dim3 per256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

hipError_t tfrecord_search_scan(void *tmp, size_t *tmp_bytes, uint64_t *tbase, uint64_t tiles, hipStream_t s) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, tbase, tbase, (int)(tiles + 1), s);
}

hipError_t tfrecord_search_candidates(const uint8_t *base, const uint8_t *wa, const TfsPlanA &A, uint64_t n, uint64_t tiles,
                                      size_t scan_tmp_bytes, int cus, hipEvent_t searched, hipStream_t s) {
    uint8_t *w = const_cast<uint8_t *>(wa);
    const s3dg_tfrecord_stream *st = reinterpret_cast<const s3dg_tfrecord_stream *>(w);
    const uint64_t *tile0 = reinterpret_cast<const uint64_t *>(w + A.tile0_off);
    uint64_t *tbase = reinterpret_cast<uint64_t *>(w + A.tbase_off);
    // 24 KiB of LDS and few registers: eight workgroups a CU, then a loop over the tiles
    const uint64_t fit = 8ull * (uint64_t)(cus > 0 ? cus : 256), grid = tiles < fit ? (tiles ? tiles : 1) : fit;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tfs_candidates, dim3((uint32_t)grid), dim3(256), 0, s, base, st, tile0, n, tiles,
                       reinterpret_cast<uint64_t *>(w + A.bm_off), reinterpret_cast<uint16_t *>(w + A.wpre_off), tbase);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (searched && (e = hipEventRecord(searched, s)) != hipSuccess) return e;
    return tfrecord_search_scan(w + A.tmp_off, &scan_tmp_bytes, tbase, tiles, s);
}

hipError_t tfrecord_search_resolve(const uint8_t *base, uint8_t *idx, const uint8_t *wa, const TfsPlanA &A, uint8_t *wb,
                                   const TfsPlanB &B, uint64_t n, uint64_t tiles, uint32_t nodes, int cus, hipEvent_t *marks,
                                   hipStream_t s) {
    uint8_t *w = const_cast<uint8_t *>(wa);
    const s3dg_tfrecord_stream *st = reinterpret_cast<const s3dg_tfrecord_stream *>(w);
    const uint64_t *tile0 = reinterpret_cast<const uint64_t *>(w + A.tile0_off);
    const TfsMap M{reinterpret_cast<const uint64_t *>(w + A.bm_off), reinterpret_cast<const uint16_t *>(w + A.wpre_off),
                   reinterpret_cast<const uint64_t *>(w + A.tbase_off)};
    TfsEnt *ent = reinterpret_cast<TfsEnt *>(wb + B.ent_off);
    TfsAnchor *anch = reinterpret_cast<TfsAnchor *>(wb + B.anch_off);
    TfsHop *hop[2] = {reinterpret_cast<TfsHop *>(wb + B.hop_off[0]), reinterpret_cast<TfsHop *>(wb + B.hop_off[1])};
    uint32_t *next = reinterpret_cast<uint32_t *>(wb + B.next_off);
    auto mark = [&](int i) -> hipError_t { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    hipError_t e;
    (void)hipGetLastError();
    int cur = 0;
    if (nodes) {
        const uint64_t words = tiles * kTfsTileWords;
        hipLaunchKernelGGL(k_tfs_clear, per256(nodes), dim3(256), 0, s, anch, nodes);
        hipLaunchKernelGGL(k_tfs_link, per256(words), dim3(256), 0, s, base, st, tile0, n, words, M, ent, next, hop[0]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = mark(0)) != hipSuccess) return e;
        for (uint32_t r = 0; r < kTfsHopLog; ++r, cur ^= 1)
            hipLaunchKernelGGL(k_tfs_double, per256(nodes), dim3(256), 0, s, (const TfsHop *)hop[cur], hop[cur ^ 1], nodes,
                               1u << r);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    } else if ((e = mark(0)) != hipSuccess) {
        return e;
    }
    if ((e = mark(1)) != hipSuccess) return e;
    // a wave waits on one load at a time: as many waves as the chip holds, then loop
    const uint64_t need = (n + 3) / 4, fit = 8ull * (uint64_t)(cus > 0 ? cus : 256);
    hipLaunchKernelGGL(k_tfs_anchor, dim3((uint32_t)(need < fit ? need : fit)), dim3(256), 0, s, base, idx, st, tile0, n, M,
                       (const TfsEnt *)ent, (const uint32_t *)next, (const TfsHop *)hop[cur], anch,
                       reinterpret_cast<s3dg_tfrecord_walk_result *>(w + A.res_off));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = mark(2)) != hipSuccess) return e;
    if (nodes) {
        hipLaunchKernelGGL(k_tfs_fill, per256(nodes), dim3(256), 0, s, (const TfsAnchor *)anch, nodes, (const TfsEnt *)ent,
                           (const uint32_t *)next, idx);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return mark(3);
}

}  // namespace s3dg
