// s3dg_tfrecord_var.hip — TFRecord shards of records of any length framed,
// checked and indexed on the device (s3dg_tfrecord_frame_var_batch,
// s3dg_tfrecord_check_var_batch, s3dg_tfrecord_index_batch).
//
// k_tfrecord_var_regions is k_tfrecord_regions (s3dg_tfrecord.hip) with another
// way to the record: template <bool Store>, 8-wave workgroups, the single-bank
// tables in 64 KiB of LDS, the row step and the tail restated once more so
// that the uniform kernels and the CRC kernels stay exactly what they were
// measured as.  A wave takes a contiguous run of the call's regions
// (tfv_run): it finds the first one's record by one binary search over the
// per-record table and then steps from entry to entry and from shard to
// shard, all in scalar registers.  A record's length and regions are
// differences of neighbouring entries; its A^len (~0) and masked_crc(len)
// come from k_tfrecord_var_consts, one thread per record, which runs first.
// Records of one region are finished by their wave; the others leave one raw
// CRC per region and are finished by k_tfrecord_var_fold, one thread per entry
// of the compact list of long records.
//
// k_tfrecord_walk follows the chain of length fields of a stream nobody has
// described, one wave per stream: aligned dword loads and a byte shift for the
// 12 header bytes at any alignment, the next header's loads issued before the
// length CRC of this one is computed, lane 0 storing the 16-byte entry.
#include "s3dg_internal.h"

namespace s3dg {
namespace {

struct CrcTablesCF {
    uint32_t tb[256 * 32];
    uint32_t tr[256 * 32];
};
static_assert(sizeof(CrcTablesCF) == kCrcTabByteShiftOff - kCrcTabCfOff, "the uploaded tables' layout");

// 16 bytes at a multiple of 4: one global_store_dwordx4
struct __attribute__((packed, aligned(4))) Piece {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// a * b mod P, ending at a's last set bit (s3dg_tfrecord.hip's)
__device__ __forceinline__ uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ kCrcBatchPoly : b >> 1;
    }
    return p;
}

// v with its first a bytes (0 < a < 16) zeroed
__device__ __forceinline__ uint4 mask_first(const uint4 v, uint32_t a) {
    auto m = [&](uint32_t w, uint32_t k) -> uint32_t {
        return a <= k ? w : a >= k + 4 ? 0u : w & (0xFFFFFFFFu << (8 * (a - k)));
    };
    return make_uint4(m(v.x, 0), m(v.y, 4), m(v.z, 8), m(v.w, 12));
}

// bytes [lo, 16) of piece v to o + lo ..., one by one
__device__ __forceinline__ void put_bytes(uint8_t *o, const uint4 v, uint32_t lo) {
    for (uint32_t y = lo; y < 16; ++y) {
        const uint32_t w = y < 8 ? (y < 4 ? v.x : v.y) : (y < 12 ? v.z : v.w);
        o[y] = (uint8_t)(w >> (8 * (y & 3)));
    }
}

// A bad record of shard k: one add per class it is bad in, the lowest record kept.
__device__ __forceinline__ void report(TfrDevRes *r, uint64_t rec, uint32_t bad16) {
    atomicAdd(&r->bad_records, 1ull);
    if (bad16 & 0x00FFu) atomicAdd(&r->bad_length, 1ull);
    if (bad16 & 0x0F00u) atomicAdd(&r->bad_length_crc, 1ull);
    if (bad16 & 0xF000u) atomicAdd(&r->bad_data_crc, 1ull);
    atomicMax(&r->first_inv, (unsigned long long)~rec);
}

// One thread per entry: a record's constants from its length.  The entry behind
// a shard's last record gets whatever its difference gives; nobody reads it.
__global__ __launch_bounds__(256) void k_tfrecord_var_consts(const uint32_t *__restrict__ pw, const TfvRec *__restrict__ rec,
                                                             uint64_t n, TfvConst *__restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint64_t a = rec[j].pre, b = rec[j + 1].pre;
    if (b < a) return;   // a shard's end
    const uint64_t len = b - a;
    out[j] = TfvConst{tfv_init(len, pw), tfv_len_mcrc(len)};
}

template <bool Store>
__global__ __launch_bounds__(512) void k_tfrecord_var_regions(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                              uint8_t *__restrict__ idx, const TfvShard *__restrict__ sh,
                                                              const TfvRec *__restrict__ rec,
                                                              const TfvConst *__restrict__ cst, uint32_t nsh, uint64_t nent,
                                                              uint64_t nreg, uint64_t per, uint32_t call_rows,
                                                              const uint8_t *__restrict__ crc_tab, uint32_t *__restrict__ raw,
                                                              TfrDevRes *__restrict__ res) {
    const CrcTablesCF *tabs = reinterpret_cast<const CrcTablesCF *>(crc_tab + kCrcTabCfOff);
    const uint32_t *lane_shift = reinterpret_cast<const uint32_t *>(crc_tab + kCrcTabLaneShiftOff);
    const uint32_t *byte_shift = reinterpret_cast<const uint32_t *>(crc_tab + kCrcTabByteShiftOff);
    __shared__ CrcTablesCF T;
    const uint32_t t = threadIdx.x, lane = t & 63;
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(tabs);
        uint4 *d = reinterpret_cast<uint4 *>(&T);
        for (uint32_t k = t; k < sizeof(CrcTablesCF) / 16; k += 512) d[k] = g[k];
    }
    __syncthreads();
    const uint32_t s = (lane >> 2) & 3, cb = (lane >> 4) & 1, cr = (lane >> 2) & 7;
    uint32_t offb[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint32_t b = 4 * (((uint32_t)(q >> 2) + s) & 3) + (((uint32_t)q + lane) & 3);
        offb[q] = 4 * (2 * (15 - b) + cb);
    }
    uint32_t shb[4], offr[4], shr[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        shb[m] = 8 * (((uint32_t)m + lane) & 3);
        const uint32_t tt = ((uint32_t)m + lane) & 3;
        shr[m] = 8 * tt;
        offr[m] = 4 * (8 * tt + cr);
    }
    const bool rot2 = s & 2, rot1 = s & 1;
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(T.tb);
    const uint8_t *tr = reinterpret_cast<const uint8_t *>(T.tr);
    auto look = [&](const uint8_t *base, uint32_t byte, uint32_t off) -> uint32_t {
        return *reinterpret_cast<const uint32_t *>(base + (byte << 7) + off);
    };
    auto row = [&](uint32_t S, const uint4 v) -> uint32_t {
        const uint32_t x0 = rot2 ? v.z : v.x, x1 = rot2 ? v.w : v.y, x2 = rot2 ? v.x : v.z, x3 = rot2 ? v.y : v.w;
        const uint32_t w[4] = {rot1 ? x1 : x0, rot1 ? x2 : x1, rot1 ? x3 : x2, rot1 ? x0 : x3};
        uint32_t u[20];
#pragma unroll
        for (int q = 0; q < 16; ++q)
            u[q] = look(tb, __builtin_amdgcn_ubfe(w[q >> 2], shb[q & 3], 8), offb[q]);
#pragma unroll
        for (int m = 0; m < 4; ++m) u[16 + m] = look(tr, __builtin_amdgcn_ubfe(S, shr[m], 8), offr[m]);
        const uint32_t a0 = xor3(u[0], u[1], u[2]), a1 = xor3(u[3], u[4], u[5]), a2 = xor3(u[6], u[7], u[8]);
        const uint32_t a3 = xor3(u[9], u[10], u[11]), a4 = xor3(u[12], u[13], u[14]);
        const uint32_t a5 = xor3(u[15], u[16], u[17]), a6 = u[18] ^ u[19];
        return xor3(xor3(a0, a1, a2), xor3(a3, a4, a5), a6);
    };
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);   // uniform: the entries come by scalar loads
    uint64_t r, r_end;
    tfv_run(nreg, per, (uint64_t)blockIdx.x * 8 + wave, &r, &r_end);
    if (r >= r_end) return;   // no barrier follows
    // the run's first record, once; from here on the wave steps
    uint64_t j = tfv_find_rec(rec, nent, r);
    uint32_t si = tfv_find_shard(sh, nsh, j);
    TfvRec cur = rec[j], nxt = rec[j + 1];
    TfvShard E = sh[si];
    uint64_t e_end = sh[si + 1].ent0;
    for (; r < r_end; ++r) {
        while (nxt.reg0 <= r) {   // the entry behind a shard's last record shares its region with the next: stepped over
            ++j;
            cur = nxt;
            nxt = rec[j + 1];
        }
        while (e_end <= j) {
            ++si;
            E = sh[si];
            e_end = sh[si + 1].ent0;
        }
        const uint64_t len = nxt.pre - cur.pre;
        const uint32_t rpr = (uint32_t)(nxt.reg0 - cur.reg0);
        const TfrRegion R = tfv_region(E, j - E.ent0, cur.pre, len, (uint32_t)(r - cur.reg0), rpr,
                                       tfv_rec_rows(len, call_rows), Store);
        const uint32_t nrows = R.nrows, a = R.a;
        // the region's first piece: 16-byte aligned; its twin in the stream: 12 (mod 16)
        const uint8_t *base = src + (R.data - a) + R.pad_lo;
        uint8_t *obase = Store ? dst + (R.out + kTfrHeader - a) + R.pad_lo : nullptr;
        const bool first = R.g == 0 && a != 0;   // its first a bytes are not the record's
        auto get = [&](const uint8_t *o, uint32_t off) -> uint4 { return *reinterpret_cast<const uint4 *>(o + off); };
        auto put = [&](uint8_t *o, uint32_t off, const uint4 v) {
            *reinterpret_cast<Piece *>(o + off) = Piece{v.x, v.y, v.z, v.w};
        };
        const uint32_t loff = lane * 16;
        uint32_t S = 0, rw = 0;
        if (first && nrows) {   // the record's first row on its own: lane 0's piece is masked
            uint4 v = get(base, loff);
            if (lane == 0) {
                if (Store) put_bytes(obase, v, a);
                v = mask_first(v, a);
            } else if (Store) {
                put(obase, loff, v);
            }
            S = row(0, v);
            rw = 1;
        }
        auto load4 = [&](uint4 (&v)[4], uint32_t r0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t rr = r0 + q < nrows ? r0 + q : nrows - 1;
                v[q] = get(base, rr * kCrcRowBytes + loff);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        auto hash4 = [&](const uint4 (&v)[4], uint32_t r0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                S = row(S, v[q]);
                if (Store) put(obase, (r0 + q) * kCrcRowBytes + loff, v[q]);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        uint4 A[4], B[4];
        if (rw + 4 <= nrows) load4(A, rw);
        for (; rw + 8 <= nrows; rw += 8) {
            load4(B, rw + 4);
            hash4(A, rw);
            load4(A, rw + 8);
            hash4(B, rw + 4);
        }
        if (rw + 4 <= nrows) {
            hash4(A, rw);
            rw += 4;
        }
        for (; rw < nrows; ++rw) {
            const uint4 v = get(base, rw * kCrcRowBytes + loff);
            S = row(S, v);
            if (Store) put(obase, rw * kCrcRowBytes + loff, v);
        }
        S = multmodp(lane_shift[lane], S);              // A^(16 (63 - lane))
        if (R.tail) {
            const uint32_t jp = R.tail >> 4, e = R.tail & 15;
            const uint8_t *tp = base + (uint64_t)nrows * kCrcRowBytes;
            uint8_t *otp = Store ? obase + (uint64_t)nrows * kCrcRowBytes : nullptr;   // both uniform
            const bool tfirst = first && nrows == 0;         // the record's first piece is in the tail
            uint4 v = make_uint4(0, 0, 0, 0);
            if (lane < jp) {
                v = get(tp, loff);
                if (tfirst && lane == 0) {
                    if (Store) put_bytes(otp, v, a);
                    v = mask_first(v, a);
                } else if (Store) {
                    put(otp, loff, v);
                }
            }
            const uint32_t piece = row(0, v);                        // raw16: the row tables give 0 for S = 0
            const uint32_t behind = lane < jp ? jp - 1 - lane : 0;   // whole pieces after this lane's
            S = multmodp(lane_shift[63 - jp], S) ^ multmodp(lane_shift[63 - behind], piece);
            S = multmodp(byte_shift[e], S);
            if (lane == jp && e) {
                uint32_t c = 0;
                for (uint32_t q = tfirst && jp == 0 ? a : 0; q < e; ++q) {
                    const uint8_t b = tp[16 * jp + q];
                    c = (c >> 8) ^ T.tb[((c ^ b) & 0xFF) * 32];   // tbyte[0]
                    if (Store) otp[16 * jp + q] = b;
                }
                S ^= c;
            }
        }
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) S ^= __shfl_xor(S, q);
        if (rpr == 1) {   // the record's only region: finish it here
            const TfvConst K = cst[j];
            const uint32_t m = tfr_masked(tfr_crc_one(S, K.init));
            bool bad = false;
            if (lane < 16) {
                const uint32_t want = tfr_framing_byte(lane, len, K.len_mcrc, m);
                const uint64_t at = R.out + tfr_framing_at(lane, len);
                if (Store) dst[at] = (uint8_t)want;
                else bad = src[at] != want;
            } else if (Store && lane == 16 && idx) {
                *reinterpret_cast<ulonglong2 *>(idx + E.idx_off + 16 * R.rec) =
                    make_ulonglong2(cur.pre + kTfrFraming * R.rec, len + kTfrFraming);
            }
            if (!Store) {
                const uint32_t bad16 = (uint32_t)__ballot(bad);
                if (bad16 && lane == 0) report(res + E.k, R.rec, bad16);
            }
        } else if (lane == 0) {
            raw[r] = S;
        }
    }
}

// One thread per record of more than one region: the plan's fold over the
// record's raws, then the framing stored (or compared) and the index entry.
template <bool Store>
__global__ __launch_bounds__(256) __attribute__((flatten)) void k_tfrecord_var_fold(
    const uint8_t *src, uint8_t *dst, uint8_t *idx, const TfvShard *sh, const TfvRec *rec, const TfvConst *cst,
    const uint64_t *longs, uint32_t nsh, uint64_t nlong, uint32_t call_rows, const uint32_t *raw, TfrDevRes *res) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nlong) return;
    const uint64_t j = longs[t];
    const TfvShard E = sh[tfv_find_shard(sh, nsh, j)];
    const TfvRec cur = rec[j], nxt = rec[j + 1];
    const TfvConst K = cst[j];
    const uint64_t i = j - E.ent0, len = nxt.pre - cur.pre, out = E.dst_off + cur.pre + kTfrFraming * i;
    const uint32_t a = (uint32_t)(((Store ? 0u : kTfrHeader) + cur.pre) & 15u);
    const uint32_t crc = tfr_crc_fold(raw + cur.reg0, (uint32_t)(nxt.reg0 - cur.reg0), tfv_rec_rows(len, call_rows), a, len,
                                      K.init);
    const uint32_t m = tfr_masked(crc);
    uint32_t bad16 = 0;
    for (uint32_t l = 0; l < 16; ++l) {
        const uint32_t want = tfr_framing_byte(l, len, K.len_mcrc, m);
        const uint64_t at = out + tfr_framing_at(l, len);
        if (Store) dst[at] = (uint8_t)want;
        else bad16 |= (uint32_t)(src[at] != want) << l;
    }
    if (Store && idx)
        *reinterpret_cast<ulonglong2 *>(idx + E.idx_off + 16 * i) = make_ulonglong2(cur.pre + kTfrFraming * i, len + kTfrFraming);
    if (!Store && bad16) report(res + E.k, i, bad16);
}

// The 12 header bytes at p, at any byte alignment: the aligned dwords that hold
// them (each holds at least one byte of the stream), and, as a second step so
// that other work can stand between the loads and their first use, a byte shift.
struct HeaderWords {
    uint32_t w0, w1, w2, w3, sft;
};
struct Header {
    uint32_t lo, hi, crc;
};
__device__ __forceinline__ HeaderWords load_header(const uint8_t *p) {
    const uintptr_t at = reinterpret_cast<uintptr_t>(p);
    const uint32_t sft = (uint32_t)(at & 3u);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(at - sft);
    return HeaderWords{q[0], q[1], q[2], sft ? q[3] : 0u, sft};
}
__device__ __forceinline__ Header shift_header(const HeaderWords &W) {
    return Header{__builtin_amdgcn_alignbyte(W.w1, W.w0, W.sft), __builtin_amdgcn_alignbyte(W.w2, W.w1, W.sft),
                  __builtin_amdgcn_alignbyte(W.w3, W.w2, W.sft)};
}

// One wave per stream (four per workgroup), every lane following the same
// chain; lane 0 stores.  tfv_walk_host is this loop on the host.
__global__ __launch_bounds__(256) void k_tfrecord_walk(const uint8_t *__restrict__ base, uint8_t *__restrict__ idx,
                                                       const s3dg_tfrecord_stream *__restrict__ st, uint64_t n,
                                                       s3dg_tfrecord_walk_result *__restrict__ res) {
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t k = (uint64_t)blockIdx.x * 4 + wave; k < n; k += (uint64_t)gridDim.x * 4) {
        const s3dg_tfrecord_stream Sd = st[k];
        const uint8_t *p = base + Sd.off;
        ulonglong2 *ent = reinterpret_cast<ulonglong2 *>(idx + Sd.idx_off);
        uint64_t pos = 0, recs = 0, bad = 0, first = UINT64_MAX, status = 0;
        bool more = tfv_walk_has_header(Sd.bytes);
        if (more && Sd.max_records == 0) {
            status = 2;
            more = false;
        }
        HeaderWords W{0, 0, 0, 0, 0};
        if (more) W = load_header(p);
        while (more) {
            const Header H = shift_header(W);
            const uint64_t len = (uint64_t)H.lo | ((uint64_t)H.hi << 32);
            uint64_t size = 0;
            if (tfv_walk_step(Sd.bytes - pos, len, &size) != kTfvWalkRecord) {
                status = 1;
                break;
            }
            if (lane == 0) ent[recs] = make_ulonglong2(pos, size);
            const uint32_t crc = H.crc;
            const uint64_t rec = recs;
            pos += size;
            ++recs;
            more = tfv_walk_has_header(Sd.bytes - pos);
            if (more && recs == Sd.max_records) {
                status = 2;
                more = false;
            }
            if (more) W = load_header(p + pos);   // in flight while this record's length CRC is computed
            __builtin_amdgcn_sched_barrier(0);
            if (tfv_len_mcrc(len) != crc) {
                ++bad;
                if (first == UINT64_MAX) first = rec;
            }
        }
        if (lane == 0) res[k] = s3dg_tfrecord_walk_result{recs, status, pos, Sd.bytes - pos, bad, first};
    }
}

}  // namespace

hipError_t tfrecord_var_launch(bool frame, const uint8_t *src, uint8_t *dst, uint8_t *idx, const uint8_t *table_dev,
                               const TfvCounts &C, void *tab_dev, int cus, TfrDevRes *res, hipStream_t s) {
    if (C.live == 0) return hipSuccess;
    uint8_t *tb = const_cast<uint8_t *>(table_dev);
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(tb);
    const TfvShard *sh = reinterpret_cast<const TfvShard *>(tb + kTfvShardOff);
    const TfvRec *rec = reinterpret_cast<const TfvRec *>(tb + tfv_rec_offset(C));
    const uint64_t *longs = reinterpret_cast<const uint64_t *>(tb + tfv_long_offset(C));
    TfvConst *cst = reinterpret_cast<TfvConst *>(tb + tfv_const_offset(C));
    uint32_t *raw = reinterpret_cast<uint32_t *>(tb + tfv_raw_offset(C));
    const uint8_t *tab = (const uint8_t *)tab_dev;
    (void)hipGetLastError();
    // every entry but the table's last has a neighbour to take its length from
    hipLaunchKernelGGL(k_tfrecord_var_consts, dim3((uint32_t)((C.ents - 1 + 255) / 256)), dim3(256), 0, s, pw, rec, C.ents - 1,
                       cst);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // 8-wave workgroups of 64 KiB LDS: two per CU, every wave one run of regions
    const uint64_t need = (C.regions + 7) / 8, fit = 2ull * (uint64_t)(cus > 0 ? cus : 256);
    const dim3 grid((uint32_t)(need < fit ? need : fit)), fgrid((uint32_t)((C.long_records + 255) / 256));
    const uint64_t per = tfv_run_len(C.regions, (uint64_t)grid.x * 8);
    if (frame)
        hipLaunchKernelGGL(k_tfrecord_var_regions<true>, grid, dim3(512), 0, s, src, dst, idx, sh, rec, (const TfvConst *)cst,
                           (uint32_t)C.live, C.ents, C.regions, per, C.rows, tab, raw, res);
    else
        hipLaunchKernelGGL(k_tfrecord_var_regions<false>, grid, dim3(512), 0, s, src, dst, idx, sh, rec, (const TfvConst *)cst,
                           (uint32_t)C.live, C.ents, C.regions, per, C.rows, tab, raw, res);
    e = hipGetLastError();
    if (e != hipSuccess || C.long_records == 0) return e;
    if (frame)
        hipLaunchKernelGGL(k_tfrecord_var_fold<true>, fgrid, dim3(256), 0, s, src, dst, idx, sh, rec, (const TfvConst *)cst,
                           longs, (uint32_t)C.live, C.long_records, C.rows, (const uint32_t *)raw, res);
    else
        hipLaunchKernelGGL(k_tfrecord_var_fold<false>, fgrid, dim3(256), 0, s, src, dst, idx, sh, rec, (const TfvConst *)cst,
                           longs, (uint32_t)C.live, C.long_records, C.rows, (const uint32_t *)raw, res);
    return hipGetLastError();
}

hipError_t tfrecord_walk_launch(const uint8_t *base, uint8_t *idx, const s3dg_tfrecord_stream *streams_dev, uint64_t n,
                                s3dg_tfrecord_walk_result *res_dev, int cus, hipStream_t s) {
    if (n == 0) return hipSuccess;
    // a wave waits on one load at a time: as many waves as the chip holds, then loop
    const uint64_t need = (n + 3) / 4, fit = 8ull * (uint64_t)(cus > 0 ? cus : 256);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_tfrecord_walk, dim3((uint32_t)(need < fit ? need : fit)), dim3(256), 0, s, base, idx, streams_dev, n,
                       res_dev);
    return hipGetLastError();
}

}  // namespace s3dg
