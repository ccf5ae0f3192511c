// s3dg_chunk_search.hip — the kernels of the chunker's parallel cut walk
// (S3DG_CHUNKS_SEARCH_WALK): chunk_walk's records, counts
// and totals with parallelism inside an object.  The rules are
// s3dg_chunk_search_plan.h's; here is how the work is split.
//
// k_cs_reserve  a thread per object: the node slots it reserves (none below the
//     threshold); a hipCUB exclusive sum turns them into first node slots, and
//     one over pass A's per-granule counts numbers the candidates.
// k_cs_objects  a thread per object: its CsObj, with the decision who walks it.
// k_cs_nodes    a wave per granule that has candidates, a lane per bitmap word:
//     popcount, a wave scan, and each lane stores its word's offsets.  No
//     atomics.
// k_cs_link     a thread per node slot: the node's link (cs_link), and a
//     self-link without chunks for the end node and every unused slot.
// k_cs_double   a thread per node slot, once per round, every level kept.
// k_cs_follow   a wave per object, the only serial part: an anchor per hop of
//     kCsHop links, the object's count and the chunk total.
// k_cs_fill     a workgroup per anchor, a thread per link of its hop: the
//     link's node through the set bits of its number (at most kCsHopLog loads),
//     its closing record by the thread, its run of forced records by the
//     wave's lanes together; the forced total by one atomic per wave.
// Results leave through plain vector stores and vector atomics.
#include <hipcub/hipcub.hpp>

#include "s3dg_chunks.h"
#include "s3dg_fp.h"

namespace s3dg {
namespace {

// Where object j of the add is: the stream form's equal objects, or the batch form's entries.
struct CsSrc {
    const SpanEnt *ents;
    uint64_t len, gpo, rpo;
};
__device__ __forceinline__ void src_object(const CsSrc &S, uint64_t j, uint64_t *len, uint64_t *g0, uint64_t *r0) {
    if (S.ents) {
        const SpanEnt e = S.ents[j];
        *len = e.size;
        *g0 = e.g0;
        *r0 = e.s0;
    } else {
        *len = S.len;
        *g0 = j * S.gpo;
        *r0 = j * S.rpo;
    }
}

__global__ __launch_bounds__(256) void k_cs_reserve(CsSrc S, uint64_t n, uint64_t threshold, uint64_t minb,
                                                    uint64_t avgb, uint64_t *__restrict__ nb) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    uint64_t len = 0, g0, r0;
    if (j < n) src_object(S, j, &len, &g0, &r0);
    nb[j] = j < n ? cs_reserved(len, threshold, minb, avgb) : 0;
}

__global__ __launch_bounds__(256) void k_cs_objects(CsSrc S, uint64_t n, const uint64_t *__restrict__ nb,
                                                    const uint64_t *__restrict__ gpre, CsObj *__restrict__ obj) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    uint64_t len, g0, r0;
    src_object(S, j, &len, &g0, &r0);
    obj[j] = cs_object(len, g0, r0, nb[j], nb[j + 1] - nb[j], gpre);
}

__global__ __launch_bounds__(256) void k_cs_nodes(const uint64_t *__restrict__ bitmap, const uint32_t *__restrict__ gcnt,
                                                  const uint64_t *__restrict__ gpre, const CsObj *__restrict__ obj,
                                                  uint64_t n, uint64_t granules, uint64_t *__restrict__ off) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= granules || gcnt[g] == 0) return;
    const CsObj O = obj[cs_find_obj(obj, n, &CsObj::g0, g)];
    if (!O.take) return;
    const uint64_t word = bitmap[g * 64 + lane];
    const uint32_t c = (uint32_t)__builtin_popcountll(word);
    uint32_t inc = c;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    // the granule's candidates start at gpre[g] - gpre[O.g0] among the object's: below O.count
    cs_word_nodes(word, (g - O.g0) * kMeasureGranule + lane * 64,
                  off + O.nb + kCsFirst + (gpre[g] - gpre[O.g0]) + (inc - c));
}

__global__ __launch_bounds__(256) void k_cs_link(const CsObj *__restrict__ obj, uint64_t n, uint64_t nodes,
                                                 const uint64_t *__restrict__ gpre, uint64_t minb, uint64_t maxb,
                                                 uint64_t *__restrict__ off, uint32_t *__restrict__ kf,
                                                 CsHop *__restrict__ lvl0) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= nodes) return;
    const CsObj O = obj[cs_find_obj(obj, n, &CsObj::nb, x)];
    const uint64_t local = x - O.nb;
    CsHop h{(uint32_t)x, 0u};
    uint32_t forced = 0;
    if (O.take && local < (uint64_t)O.count + kCsFirst) {
        if (local == kCsEnd) {
            off[x] = O.len - 1;
        } else {
            if (local == kCsRoot) off[x] = ~0ull;
            const CsView V{off, gpre + O.g0, O.nb, O.len, O.count};
            // a candidate's own offset is k_cs_nodes', as are those the link looks up
            const uint64_t s = local == kCsRoot ? 0 : off[x] + 1;
            h.node = (uint32_t)O.nb + cs_link(V, s, minb, maxb, &forced, &h.chunks);
        }
    }
    kf[x] = forced;
    lvl0[x] = h;
}

__global__ __launch_bounds__(256) void k_cs_double(const CsHop *__restrict__ in, CsHop *__restrict__ out,
                                                   uint64_t nodes) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < nodes) out[x] = cs_double(in, (uint32_t)x);
}

// One wave per object (four per workgroup), every lane following the same
// hops; lane 0 stores.  The anchors of the object's range that the path does
// not use are marked so, by all lanes: also for an object the search does not walk.
__global__ __launch_bounds__(256) void k_cs_follow(const CsObj *__restrict__ obj, uint64_t n,
                                                   const uint64_t *__restrict__ nb, const CsHop *__restrict__ top,
                                                   CsAnchor *__restrict__ anch, uint32_t *__restrict__ cnt,
                                                   uint64_t *__restrict__ tot) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const CsObj O = obj[j];
    const uint64_t a0 = cs_anchor_base(O.nb, j), a1 = cs_anchor_base(nb[j + 1], j + 1);
    uint64_t hops = 0;
    if (O.take) {
        const uint32_t chunks = cs_follow(O, top, anch + a0, a1 - a0, lane == 0, &hops);
        if (lane == 0) {
            cnt[j] = chunks;
            atomicAdd(reinterpret_cast<unsigned long long *>(&tot[kChunkTotChunks]), (unsigned long long)chunks);
        }
    }
    for (uint64_t a = a0 + hops + lane; a < a1; a += 64) anch[a] = CsAnchor{kCsNone, 0u};
}

__global__ __launch_bounds__(kCsHop) void k_cs_fill(const CsAnchor *__restrict__ anch, const CsHop *__restrict__ lvl,
                                                    uint64_t nodes, const uint64_t *__restrict__ off,
                                                    const uint32_t *__restrict__ kf, uint64_t maxb,
                                                    uint64_t *__restrict__ roff, uint32_t *__restrict__ rlen,
                                                    uint64_t *__restrict__ tot) {
    const CsAnchor A = anch[blockIdx.x];
    if (A.node == kCsNone) return;
    const uint32_t lane = threadIdx.x & 63;
    CsRec R{0, 0u, 0u, 0u};
    const bool live = cs_fill_lane(lvl, nodes, off, kf, A, threadIdx.x, maxb, &R);
    if (live && R.last) {
        roff[(uint64_t)R.slot + R.forced] = R.s + (uint64_t)R.forced * maxb;
        rlen[(uint64_t)R.slot + R.forced] = R.last;
    }
    // a run of forced records by the wave's lanes, one link after the other
    for (uint64_t m = __ballot(live && R.forced != 0); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        const uint32_t K = __shfl(R.forced, l, 64), slot = __shfl(R.slot, l, 64);
        const uint64_t s = (uint64_t)__shfl((uint32_t)R.s, l, 64) | ((uint64_t)__shfl((uint32_t)(R.s >> 32), l, 64) << 32);
        for (uint32_t i = lane; i < K; i += 64) {
            roff[(uint64_t)slot + i] = s + (uint64_t)i * maxb;
            rlen[(uint64_t)slot + i] = (uint32_t)maxb;
        }
    }
    uint64_t f = R.forced;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) f += shfl_xor64(f, d);
    if (lane == 0 && f) atomicAdd(reinterpret_cast<unsigned long long *>(&tot[kChunkTotForced]), (unsigned long long)f);
}

// Item i of the scan over the granules' counts: one item more than granules, so that the total is there.
struct GcntAt {
    const uint32_t *gcnt;
    uint64_t granules;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return i < granules ? gcnt[i] : 0ull; }
};
using GcntIt = hipcub::TransformInputIterator<uint64_t, GcntAt, hipcub::CountingInputIterator<uint64_t>>;

hipError_t scan_counts(void *tmp, size_t *tmp_bytes, const uint32_t *gcnt, uint64_t granules, uint64_t *gpre,
                       hipStream_t s) {
    GcntIt it(hipcub::CountingInputIterator<uint64_t>(0), GcntAt{gcnt, granules});
    return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, it, gpre, (int)(granules + 1), s);
}
hipError_t scan_reserved(void *tmp, size_t *tmp_bytes, uint64_t *nb, uint64_t n_objs, hipStream_t s) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, nb, nb, (int)(n_objs + 1), s);
}

inline dim3 per256(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

hipError_t chunk_search_tmp_bytes(uint64_t n_objs, uint64_t granules, size_t *bytes) {
    size_t a = 0, b = 0;
    hipError_t e = scan_counts(nullptr, &a, nullptr, granules, nullptr, nullptr);
    if (e == hipSuccess) e = scan_reserved(nullptr, &b, nullptr, n_objs, nullptr);
    *bytes = a > b ? a : b;
    return e;
}

hipError_t launch_chunk_search(const ChunkPlan &P, const ChunkSrc &src, const ChunkSearch &Q, uint64_t min_bytes,
                               uint64_t avg_bytes, uint64_t max_bytes, void *scratch, uint64_t *tot, hipStream_t s) {
    uint8_t *sc = reinterpret_cast<uint8_t *>(scratch);
    const uint64_t *bitmap = reinterpret_cast<const uint64_t *>(sc);
    uint64_t *roff = reinterpret_cast<uint64_t *>(sc + P.off_offset);
    uint32_t *rlen = reinterpret_cast<uint32_t *>(sc + P.len_offset);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(sc + P.cnt_offset);
    const uint32_t *gcnt = reinterpret_cast<const uint32_t *>(sc + P.gcnt_offset);
    const CsPlan &C = Q.plan;
    uint64_t *gpre = reinterpret_cast<uint64_t *>(sc + C.gpre_off), *nb = reinterpret_cast<uint64_t *>(sc + C.nb_off);
    CsObj *obj = reinterpret_cast<CsObj *>(sc + C.obj_off);
    uint64_t *off = reinterpret_cast<uint64_t *>(sc + C.off_off);
    uint32_t *kf = reinterpret_cast<uint32_t *>(sc + C.kf_off);
    CsHop *lvl = reinterpret_cast<CsHop *>(sc + C.lvl_off);
    CsAnchor *anch = reinterpret_cast<CsAnchor *>(sc + C.anch_off);
    const uint64_t n = P.n_objs, nodes = C.nodes;
    const CsSrc S{src.ents, P.len, P.gpo, P.rpo};
    size_t tmp = Q.tmp_bytes;
    hipError_t e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_cs_reserve, per256(n + 1), dim3(256), 0, s, S, n, Q.threshold, min_bytes, avg_bytes, nb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = scan_reserved(sc + C.tmp_off, &tmp, nb, n, s)) != hipSuccess) return e;
    tmp = Q.tmp_bytes;
    if ((e = scan_counts(sc + C.tmp_off, &tmp, gcnt, P.granules, gpre, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_cs_objects, per256(n), dim3(256), 0, s, S, n, (const uint64_t *)nb, (const uint64_t *)gpre, obj);
    hipLaunchKernelGGL(k_cs_nodes, dim3((uint32_t)((P.granules + 3) / 4)), dim3(256), 0, s, bitmap, gcnt,
                       (const uint64_t *)gpre, (const CsObj *)obj, n, P.granules, off);
    hipLaunchKernelGGL(k_cs_link, per256(nodes), dim3(256), 0, s, (const CsObj *)obj, n, nodes, (const uint64_t *)gpre,
                       min_bytes, max_bytes, off, kf, lvl);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (uint32_t r = 0; r < kCsHopLog; ++r)
        hipLaunchKernelGGL(k_cs_double, per256(nodes), dim3(256), 0, s, (const CsHop *)(lvl + r * nodes),
                           lvl + (r + 1) * nodes, nodes);
    hipLaunchKernelGGL(k_cs_follow, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, (const CsObj *)obj, n,
                       (const uint64_t *)nb, (const CsHop *)(lvl + (uint64_t)kCsHopLog * nodes), anch, cnt, tot);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_cs_fill, dim3((uint32_t)C.anchors), dim3(kCsHop), 0, s, (const CsAnchor *)anch,
                       (const CsHop *)lvl, nodes, (const uint64_t *)off, (const uint32_t *)kf, max_bytes, roff, rlen, tot);
    return hipGetLastError();
}

}  // namespace s3dg
