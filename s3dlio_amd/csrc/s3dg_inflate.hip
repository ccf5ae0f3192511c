// s3dg_inflate.hip — RFC 1951 inflate, one wave per stream (s3dg_inflate_batch,
// s3dg_npz_zindex_batch, s3dg_npz_zunpack_batch).  The decode
// itself is s3dg_inflate_plan.h's inf_run, the code the CPU sweep runs; this
// file is its environment of one wave and the kernels around it.
//
//   k_inflate    a workgroup of one wave per work item.  In LDS: the 32 KiB
//                history ring, a 1 KiB input tile, the tables.  The bit buffer,
//                the counters and every decoded value are uniform (the words
//                of the tile and the table entries come through
//                v_readfirstlane), so the symbol loop is scalar code with one
//                LDS lookup per symbol.
//                Input: the tile is 64 aligned 16-byte loads; a 16-byte piece
//                outside the span is not loaded, and the bytes of the first and
//                last word outside it are masked (inf_mask_word).
//                Codes: counts by LDS atomics, first codes and sorted offsets
//                by one wave prefix over count[l] << (15 - l) (the same sum
//                decides over-subscribed / incomplete), ranks inside a round of
//                64 symbols by 15 ballots, the first-level table filled by the
//                symbol's own lane.
//                Tokens: a literal or a (length, distance) pair goes into lane
//                t of two VGPRs (a compare and a select), with its output offset
//                from a running sum.  A batch ends at 64 tokens, at a stored block
//                and at the stream's end (the core ends a stream before the
//                token that passes a limit).  The wave executes it in token
//                order: a run of literals one per lane, a match 64 bytes a
//                step out of the ring (source index i mod dist when the match
//                overlaps itself).  A later token's place may alias an earlier
//                match's source in the ring, so runs are not merged across a
//                match.  Then the ring's whole 16-byte pieces go to the
//                destination as one vector store per lane; only the stream's
//                last piece is written by bytes.  History is never read from
//                global memory.
//   k_inflate_crc  one wave per item that asked: 64 lanes hash 64 shares of
//                the finished output by a byte table in LDS and the CRCs are
//                combined by x^(8 n) (inf_mulmod, inf_x8n).
//   k_inz_walk   k_nzi_walk accepting method 8, writing z entries.
//   k_inz_plan   one thread per take: validates its z entries, sums their
//                places, writes the work items (skipped when not taken).
#include "s3dg_internal.h"
#include "s3dg_inflate_plan.h"

namespace s3dg {
namespace {

constexpr uint32_t kRing = kInfWindow, kRingMask = kRing - 1;
constexpr uint32_t kTileWords = 256;   // a 1 KiB tile of input
constexpr uint32_t kStoredStep = 16384;

struct InfLds {
    uint8_t ring[kRing];
    uint32_t tile[kTileWords];
    InfTables T;
    uint32_t cnt[16], idx[16], code[16];   // a code under construction
};

__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) { return (uint64_t)uni((uint32_t)x) | (uint64_t)uni((uint32_t)(x >> 32)) << 32; }

// The environment of inf_run for one wave.
struct WaveEnv {
    InfLds &S;
    const uint8_t *src;   // the span's first byte
    uint8_t *dst;
    uint64_t src_bytes;
    uint32_t lane, ld;            // the span's first byte is ld bytes past a multiple of 16
    uint64_t tile_w0 = 1ull << 62;   // first word of the tile in LDS; no word is within 256 of this one
    uint64_t opos = 0, flushed = 0;   // bytes executed into the ring, bytes stored (a multiple of 16 until the end)
    uint32_t nt = 0, bbytes = 0;  // the batch: tokens and their bytes
    uint32_t tok = 0, tpos = 0;   // lane t: token t (dist | len << 16, or byte << 16) and its offset from opos

    __device__ WaveEnv(InfLds &s, const InfWork &W, uint32_t lane_)
        : S(s), src(reinterpret_cast<const uint8_t *>(W.src)), dst(reinterpret_cast<uint8_t *>(W.dst)), src_bytes(W.src_bytes),
          lane(lane_), ld((uint32_t)(W.src & 15u)) {}

    __device__ uint32_t lead() const { return ld; }
    __device__ InfTables &T() { return S.T; }
    __device__ uint32_t u(uint32_t x) const { return uni(x); }

    __device__ uint32_t word(uint64_t w) {
        if (w - tile_w0 >= kTileWords) {
            tile_w0 = w & ~(uint64_t)(kTileWords - 1);
            // piece `lane` of the tile: span offsets [off, off + 16)
            const int64_t off = (int64_t)(4 * tile_w0 + 16 * lane) - ld;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (off + 16 > 0 && off < (int64_t)src_bytes) v = *reinterpret_cast<const uint4 *>(src + off);
            __syncthreads();
            reinterpret_cast<uint4 *>(S.tile)[lane] = v;
            __syncthreads();
        }
        return inf_mask_word(uni(S.tile[w - tile_w0]), (int64_t)(4 * w) - ld, src_bytes);
    }

    __device__ void put_lens(uint32_t i, uint32_t rep, uint32_t v) {
        for (uint32_t q = lane; q < rep; q += 64) S.T.lens[i + q] = (uint8_t)v;
        __syncthreads();
    }
    __device__ uint32_t get_len(uint32_t i) const { return S.T.lens[i]; }
    __device__ void put_fixed() {
        for (uint32_t q = lane; q < 320; q += 64) S.T.lens[q] = (uint8_t)inf_fixed_len(q);
        __syncthreads();
    }

    // One canonical code by all lanes; inf_build_serial's result.
    __device__ bool build(const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *sym, uint16_t *lut, uint32_t lut_bits, bool cl) {
        __syncthreads();
        for (uint32_t q = lane; q < (lut ? 1u << lut_bits : 0u); q += 64) lut[q] = 0;
        if (lane < 16) S.cnt[lane] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < n; i += 64)
            if (lens[i]) atomicAdd(&S.cnt[lens[i]], 1u);
        __syncthreads();
        // lane l: count[l], and the prefixes over the lengths below l
        const uint32_t c = lane >= 1 && lane < 16 ? S.cnt[lane] : 0u;
        const uint32_t k = lane < 16 ? c << (15 - lane) : 0u;
        uint32_t ci = c, ki = k;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            const uint32_t a = __shfl_up(ci, d), b = __shfl_up(ki, d);
            if (lane >= (uint32_t)d) ci += a, ki += b;
        }
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)ci, 15), kraft = (uint32_t)__builtin_amdgcn_readlane((int)ki, 15);
        const uint32_t count1 = (uint32_t)__builtin_amdgcn_readlane((int)c, 1);
        if (lane < 16) {
            count[lane] = (uint16_t)c;
            S.idx[lane] = ci - c;                          // where the symbols of length l start
            S.code[lane] = (ki - k) >> (15 - lane);        // the first code of length l
        }
        __syncthreads();
        if (!inf_code_ok(kraft, total, count1, cl)) return false;
        for (uint32_t i0 = 0; i0 < n; i0 += 64) {
            const uint32_t i = i0 + lane, l = i < n ? lens[i] : 0u;
            uint32_t before = 0;
            bool last = false;
#pragma unroll
            for (uint32_t L = 1; L < 16; ++L) {
                const uint64_t m = __ballot(l == L);
                if (l == L) {
                    before = (uint32_t)__popcll(m & ((1ull << lane) - 1));
                    last = (m >> lane) == 1ull;
                }
            }
            uint32_t at = 0, cd = 0;
            if (l) {
                at = S.idx[l] + before;
                cd = S.code[l] + before;
            }
            __syncthreads();
            if (l) {
                sym[at] = (uint16_t)i;
                if (last) {
                    S.idx[l] = at + 1;
                    S.code[l] = cd + 1;
                }
                if (lut && l <= lut_bits)
                    for (uint32_t q = __brev(cd) >> (32 - l); q < (1u << lut_bits); q += 1u << l) lut[q] = (uint16_t)(i << 4 | l);
            }
            __syncthreads();
        }
        return true;
    }

    // ---- output ----
    __device__ void token(uint32_t v, uint32_t len) {
        tok = lane == nt ? v : tok;
        tpos = lane == nt ? bbytes : tpos;
        ++nt;
        bbytes += len;
        if (nt == 64) execute();
    }
    __device__ void literal(uint32_t b) { token(b << 16, 1); }
    __device__ void match(uint32_t len, uint32_t dist) { token(len << 16 | dist, len); }   // dist <= 32768 < 2^16

    // The batch into the ring in token order, then the ring's whole pieces out.
    __device__ void execute() {
        uint64_t mm = __ballot(lane < nt && (tok & 0xFFFFu) != 0);
        uint32_t prev = 0;
        const uint32_t base = (uint32_t)opos;
        for (;;) {
            const uint32_t t = mm ? (uint32_t)__builtin_ctzll(mm) : nt;
            if (lane >= prev && lane < t) S.ring[(base + tpos) & kRingMask] = (uint8_t)(tok >> 16);
            __syncthreads();
            if (t == nt) break;
            const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)tok, (int)t);
            const uint32_t p = base + (uint32_t)__builtin_amdgcn_readlane((int)tpos, (int)t);
            const uint32_t len = v >> 16, dist = v & 0xFFFFu;
            for (uint32_t i = lane; i < len; i += 64) {
                const uint32_t s = dist >= len ? i : i % dist;
                S.ring[(p + i) & kRingMask] = S.ring[(p - dist + s) & kRingMask];
            }
            __syncthreads();
            prev = t + 1;
            mm &= mm - 1;
        }
        opos += bbytes;
        nt = 0;
        bbytes = 0;
        flush();
    }
    __device__ void flush() {
        const uint64_t end = opos & ~15ull;
        for (uint64_t q = flushed + 16ull * lane; q < end; q += 1024)
            *reinterpret_cast<uint4 *>(dst + q) = *reinterpret_cast<const uint4 *>(S.ring + ((uint32_t)q & kRingMask));
        flushed = end;
        __syncthreads();
    }
    // len bytes from byte pos of the span: the core has checked both ends.
    __device__ void stored(uint64_t pos, uint64_t len) {
        if (nt) execute();
        while (len) {
            const uint32_t step = len < kStoredStep ? (uint32_t)len : kStoredStep;
            for (uint32_t i = lane; i < step; i += 64) S.ring[((uint32_t)opos + i) & kRingMask] = src[pos + i];
            __syncthreads();
            opos += step;
            pos += step;
            len -= step;
            flush();
        }
    }
    // The stream's ragged last piece, by bytes.
    __device__ void finish() {
        if (nt) execute();
        const uint64_t q = flushed + lane;
        if (q < opos) dst[q] = S.ring[(uint32_t)q & kRingMask];
    }
};

__global__ __launch_bounds__(64) void k_inflate(const InfWork *__restrict__ work, uint64_t n, InfDevRes *__restrict__ res) {
    __shared__ InfLds S;
    const uint32_t lane = threadIdx.x;
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        InfWork W = work[k];
        W.src = uni64(W.src), W.src_bytes = uni64(W.src_bytes), W.dst = uni64(W.dst), W.dst_cap = uni64(W.dst_cap);
        W.want = uni64(W.want), W.flags = uni(W.flags);
        if (W.flags & kInfSkip) continue;
        __syncthreads();
        WaveEnv E(S, W, lane);
        const InfEnd r = inf_run(E, W.src_bytes, W.dst_cap, W.want, (W.flags & kInfStored) != 0);
        E.finish();
        if (lane == 0) res[k] = InfDevRes{r.status, 0u, r.out_bytes, r.in_bytes, 0};
    }
}

__global__ __launch_bounds__(64) void k_inflate_crc(const InfWork *__restrict__ work, uint64_t n, InfDevRes *__restrict__ res) {
    __shared__ uint32_t tab[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t q = lane; q < 256; q += 64) tab[q] = inf_crc_entry(q);
    __syncthreads();
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const InfWork W = work[k];
        if (!(W.flags & kInfCrc) || (W.flags & kInfSkip) || res[k].status != S3DG_INFLATE_OK) continue;
        const uint64_t bytes = res[k].out_bytes, share = inf_crc_share(bytes);
        const uint8_t *p = reinterpret_cast<const uint8_t *>(W.dst);
        const uint64_t lo = lane * share < bytes ? lane * share : bytes, hi = lo + share < bytes ? lo + share : bytes;
        uint32_t c = 0xFFFFFFFFu;
        uint64_t q = lo;
        for (; q + 16 <= hi; q += 16) {   // lo is a multiple of 16 and so is the destination
            const uint4 v = *reinterpret_cast<const uint4 *>(p + q);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                c ^= w[d];
#pragma unroll
                for (int b = 0; b < 4; ++b) c = (c >> 8) ^ tab[c & 0xFF];
            }
        }
        for (; q < hi; ++q) c = (c >> 8) ^ tab[(c ^ p[q]) & 0xFF];
        c = hi > lo ? ~c : 0u;
        c = inf_mulmod(c, inf_x8n(bytes - hi));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c ^= __shfl_xor(c, d);
        if (lane == 0 && c != W.crc) res[k].bad_crc = 1;
    }
}

// ---- the walk: s3dg_npz_unpack.hip's, with method 8 beside method 0 --------------------------
__device__ __forceinline__ uint32_t wave_bytes(const uint8_t *p, uint32_t n, uint32_t lane) {
    return lane < n ? (uint32_t)p[lane] : 0u;
}
template <int N>
__device__ __forceinline__ uint32_t field(uint32_t b, int at) {
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) v |= (uint32_t)__builtin_amdgcn_readlane((int)b, at + q) << (8 * q);
    return v;
}
// Both sizes of a local header whose size fields are ZIP64 markers, from the
// 0x0001 record of its extra field x[0, xl): usize first, then csize.
__device__ __forceinline__ bool extra_sizes(const uint8_t *x, uint32_t xl, uint32_t usize, uint32_t csize, uint32_t lane) {
    uint32_t at = 0;
    while (at + 4 <= xl) {
        const uint32_t left = xl - at, b = wave_bytes(x + at, left < 20 ? left : 20, lane);
        const uint32_t id = field<2>(b, 0), len = field<2>(b, 2);
        if (len > left - 4) return false;
        if (id == 1) return len >= 16 && field<4>(b, 4) == usize && field<4>(b, 8) == 0 && field<4>(b, 12) == csize && field<4>(b, 16) == 0;
        at += 4 + len;
    }
    return false;
}

__global__ __launch_bounds__(64) void k_inz_walk(const uint8_t *__restrict__ base, uint8_t *__restrict__ table,
                                                 const s3dg_npz_stream *__restrict__ arch, uint64_t n,
                                                 s3dg_npz_walk_result *__restrict__ res) {
    const uint32_t lane = threadIdx.x;
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const s3dg_npz_stream A = arch[k];
        const uint8_t *p = base + A.off;
        const uint64_t bytes = A.bytes;   // below 2^32
        s3dg_npz_walk_result R{S3DG_NPZ_WALK_NO_END, 0, 0, 0, 0, kNzuNone};
        uint32_t *out = reinterpret_cast<uint32_t *>(table + A.tab_off);
        uint64_t end_at = kNzuNone;
        if (bytes >= kNpzEnd) {
            const uint64_t last = bytes - kNpzEnd, dmax = last < 65535 ? last : 65535;
            for (uint64_t d0 = 0; d0 <= dmax; d0 += 64) {
                const uint64_t d = d0 + lane;
                bool hit = false;
                if (d <= dmax) {
                    const uint8_t *q = p + (last - d);
                    hit = q[0] == 0x50 && q[1] == 0x4b && q[2] == 0x05 && q[3] == 0x06 && ((uint32_t)q[20] | (uint32_t)q[21] << 8) == d;
                }
                const uint64_t m = __ballot(hit);
                if (m) {
                    end_at = last - (d0 + (uint64_t)__builtin_ctzll(m));
                    break;
                }
            }
        }
        if (end_at != kNzuNone) {
            const uint32_t b = wave_bytes(p + end_at, (uint32_t)kNpzEnd, lane);
            const uint32_t total = field<2>(b, 10), cd_size = field<4>(b, 12), cd_off = field<4>(b, 16);
            R.members_total = total;
            R.status = S3DG_NPZ_WALK_OK;
            if (!nzi_end_ok(field<2>(b, 4), field<2>(b, 6), field<2>(b, 8), total, cd_size, cd_off, end_at)) R.status = S3DG_NPZ_WALK_DIRECTORY;
            uint64_t c = cd_off;
            const uint64_t cd_end = end_at;
            uint32_t i = 0;
            for (; R.status == S3DG_NPZ_WALK_OK && i < total; ++i) {
                if (i == A.max_members) {
                    R.status = S3DG_NPZ_WALK_CAPPED;
                    break;
                }
                R.bad_member = i;
                if (c + kNpzCentral > cd_end) {
                    R.status = S3DG_NPZ_WALK_DIRECTORY;
                    break;
                }
                const uint32_t ce = wave_bytes(p + c, (uint32_t)kNpzCentral, lane);
                const uint32_t flags = field<2>(ce, 8), method = field<2>(ce, 10), crc = field<4>(ce, 16);
                const uint32_t csize = field<4>(ce, 20), usize = field<4>(ce, 24), name_len = field<2>(ce, 28), local_off = field<4>(ce, 42);
                const uint64_t c_next = c + kNpzCentral + name_len + field<2>(ce, 30) + field<2>(ce, 32);
                if (!nzi_central_ok(field<4>(ce, 0), csize, usize, field<2>(ce, 34), local_off) || c_next > cd_end ||
                    (uint64_t)local_off + kNpzLocal > cd_off) {
                    R.status = S3DG_NPZ_WALK_DIRECTORY;
                    break;
                }
                if (!inz_supported(flags, method)) {
                    R.status = S3DG_NPZ_WALK_UNSUPPORTED;
                    break;
                }
                if (method == 0 && csize != usize) {
                    R.status = S3DG_NPZ_WALK_DIRECTORY;
                    break;
                }
                const uint32_t lh = wave_bytes(p + local_off, (uint32_t)kNpzLocal, lane);
                const uint32_t lname = field<2>(lh, 26), lextra = field<2>(lh, 28), lc = field<4>(lh, 18), lu = field<4>(lh, 22);
                const uint64_t data_at = (uint64_t)local_off + kNpzLocal + lname + lextra;
                if (data_at + csize > cd_off) {
                    R.status = S3DG_NPZ_WALK_DIRECTORY;
                    break;
                }
                bool same = field<4>(lh, 0) == kNzuSigLocal && field<2>(lh, 6) == flags && field<2>(lh, 8) == method &&
                            field<4>(lh, 14) == crc && lname == name_len;
                if (same) {
                    if (lc == 0xFFFFFFFFu && lu == 0xFFFFFFFFu) same = extra_sizes(p + local_off + kNpzLocal + lname, lextra, usize, csize, lane);
                    else same = lc == csize && lu == usize;
                }
                for (uint32_t q = 0; same && q < name_len; q += 64) {
                    const bool in = q + lane < name_len;
                    const bool diff = in && p[local_off + kNpzLocal + q + lane] != p[c + kNpzCentral + q + lane];
                    same = __ballot(diff) == 0;
                }
                if (!same) {
                    R.status = S3DG_NPZ_WALK_LOCAL;
                    break;
                }
                const uint32_t e[8] = {local_off, name_len | flags << 16, (uint32_t)data_at, csize, usize, crc, method, 0u};
                uint32_t mine = 0;
#pragma unroll
                for (int q = 0; q < 8; ++q) mine = lane == (uint32_t)q ? e[q] : mine;
                if (lane < 8) out[8 * (uint64_t)i + lane] = mine;
                R.payload_bytes += usize;
                R.packed_bytes += nzu_packed(usize);
                c = c_next;
            }
            R.members = i;
            if (R.status == S3DG_NPZ_WALK_OK && c != cd_end) {
                R.status = S3DG_NPZ_WALK_DIRECTORY;
                R.bad_member = kNzuNone;
            }
            if (R.status == S3DG_NPZ_WALK_OK || R.status == S3DG_NPZ_WALK_CAPPED) R.bad_member = kNzuNone;
        }
        if (lane == 0) res[k] = R;
    }
}

// ---- the plan of an unpack -------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_inz_plan(const uint8_t *__restrict__ src, const uint8_t *__restrict__ tab,
                                                 uint8_t *__restrict__ dst, const TfxTake *__restrict__ tk, uint64_t n,
                                                 InzDevTake *__restrict__ verdict, InfWork *__restrict__ work,
                                                 InfDevRes *__restrict__ res) {
    const uint64_t k = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const TfxTake T = tk[k];
    const InzEntry *ent = reinterpret_cast<const InzEntry *>(tab + T.idx_off) + T.first;
    uint64_t span = 0, bytes = 0;
    bool fits = true;
    for (uint64_t i = 0; i < T.count; ++i) {
        const InzEntry e = ent[i];
        fits = fits && inz_entry_fits(e, T.bytes);
        span += nzu_packed(e.usize);
        bytes += e.usize;
    }
    const uint64_t status = !fits ? S3DG_NPZ_TAKE_TABLE : span > T.dst_cap ? S3DG_NPZ_TAKE_CAPACITY : S3DG_NPZ_TAKE_TAKEN;
    verdict[k] = InzDevTake{status, fits ? span : 0, status == S3DG_NPZ_TAKE_TAKEN ? bytes : 0, 0};
    uint64_t at = 0;
    for (uint64_t i = 0; i < T.count; ++i) {
        const InzEntry e = ent[i];
        InfWork W{reinterpret_cast<uint64_t>(src) + T.off + e.data_off, e.csize, reinterpret_cast<uint64_t>(dst) + T.dst_off + at,
                  e.usize, e.usize, e.crc, kInfCrc | (e.method == 0 ? kInfStored : 0u)};
        if (status != S3DG_NPZ_TAKE_TAKEN) W.flags = kInfSkip;
        work[T.ent0 + i] = W;
        res[T.ent0 + i] = InfDevRes{0, 0, 0, 0, 0};
        at += nzu_packed(e.usize);
    }
}

hipError_t run_items(const InfWork *work, uint64_t n, InfDevRes *res, hipStream_t s) {
    const dim3 grid((uint32_t)(n < (1u << 20) ? n : (1u << 20)));
    hipLaunchKernelGGL(k_inflate, grid, dim3(64), 0, s, work, n, res);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_inflate_crc, grid, dim3(64), 0, s, work, n, res);
    return hipGetLastError();
}

}  // namespace

hipError_t inflate_launch(const InfWork *work_dev, uint64_t n, InfDevRes *res_dev, hipStream_t s) {
    (void)hipGetLastError();
    return run_items(work_dev, n, res_dev, s);
}

hipError_t npz_zindex_launch(const uint8_t *base, uint8_t *table, const s3dg_npz_stream *arch_dev, uint64_t n,
                             s3dg_npz_walk_result *res_dev, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_inz_walk, dim3((uint32_t)(n < (1u << 20) ? n : (1u << 20))), dim3(64), 0, s, base, table, arch_dev, n, res_dev);
    return hipGetLastError();
}

hipError_t npz_zunpack_launch(const uint8_t *src, const uint8_t *tab, uint8_t *dst, const TfxTake *tk_dev, uint64_t n, uint64_t ents,
                              InzDevTake *verdict_dev, InfWork *work_dev, InfDevRes *res_dev, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_inz_plan, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, s, src, tab, dst, tk_dev, n, verdict_dev, work_dev, res_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || ents == 0) return e;
    return run_items(work_dev, ents, res_dev, s);
}

}  // namespace s3dg
