// s3dg_tfrecord.hip — TFRecord shards framed and checked on the device
// (s3dg_tfrecord_frame_batch, s3dg_tfrecord_check_batch).
//
// One kernel body, template <bool Store>, in k_crc32_regions_cf's shape: 8-wave
// workgroups, the single-bank tables in 64 KiB of LDS, the grid sized to the
// chip, each wave looping over regions.  The row step (the rotated schedule,
// the Horner sum, two register buffers of four rows) and the tail are
// k_crc32_batch_regions' (s3dg_crc.hip), restated here so that the CRC kernels
// stay exactly what they were measured as; the tables are the uploaded ones of
// crc_tables_device.
//
// A wave finds its shard through the prefix of regions per shard and its record
// and region by division (tfr_region, s3dg_tfrecord_plan.h).  It walks the
// padded record: the L = a + rs bytes from the 16-byte boundary at or below the
// data, the first a of them masked to zero (they are the neighbour's, and a
// zero register stays zero over zeros).  In the frame form each lane also
// stores the 16 bytes it loaded 12 (mod 16) further on, as one dword-aligned
// 16-byte store; lane 0 stores the 16 - a data bytes of the record's first
// piece one by one, and the lane that reads the last e bytes stores them as it
// reads them.  A record of one region is finished by its wave: lanes 0-15
// store (or compare) one framing byte each, lane 16 stores the index entry.
// Longer records leave one raw CRC per region and are finished by
// k_tfrecord_fold, one thread per record.
#include "s3dg_internal.h"

namespace s3dg {
namespace {

// crc_tables_device's single-bank tables (s3dg_crc.hip): tb[i*32 + 2t + c] is
// byte table t, tr[i*32 + 8t + c] row table t, copy c.
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

// a * b mod P as s3dg_crc.hip's region kernels multiply: a loop that ends at a's
// last set bit.  The plan's crcb_multmodp is 32 branch-free steps; unrolled
// with a loop-invariant factor (a lane's shift) its 32 bit tests would be kept
// in scalar registers across the region loop.
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

template <bool Store>
__global__ __launch_bounds__(512) void k_tfrecord_regions(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                          uint8_t *__restrict__ idx, const TfrShard *__restrict__ sh,
                                                          uint32_t nsh, uint64_t nreg, const uint8_t *__restrict__ crc_tab,
                                                          uint32_t *__restrict__ raw, TfrDevRes *__restrict__ res) {
    // crc_tables_device's block: the single-bank tables, A^(16 (63 - l)) and A^e
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
    const uint64_t nwaves = (uint64_t)gridDim.x * 8;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(t >> 6);   // uniform: the entry comes by scalar loads
    for (uint64_t r = (uint64_t)blockIdx.x * 8 + wave; r < nreg; r += nwaves) {
        const TfrShard E = sh[tfr_find_region(sh, nsh, r)];
        const TfrRegion R = tfr_region(E, r - E.reg0, Store);
        const uint32_t nrows = R.nrows, a = R.a;
        // the region's first piece: 16-byte aligned; its twin in the stream: 12 (mod 16)
        const uint8_t *base = src + (R.data - a) + R.pad_lo;
        uint8_t *obase = Store ? dst + (R.out + kTfrHeader - a) + R.pad_lo : nullptr;
        const bool first = R.g == 0 && a != 0;   // its first a bytes are not the record's
        // a region is below 2^32 bytes: a uniform base and one 32-bit offset per
        // piece, the same for the load and its store
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
            const uint32_t j = R.tail >> 4, e = R.tail & 15;
            const uint8_t *tp = base + (uint64_t)nrows * kCrcRowBytes;
            uint8_t *otp = Store ? obase + (uint64_t)nrows * kCrcRowBytes : nullptr;   // both uniform
            const bool tfirst = first && nrows == 0;         // the record's first piece is in the tail
            uint4 v = make_uint4(0, 0, 0, 0);
            if (lane < j) {
                v = get(tp, loff);
                if (tfirst && lane == 0) {
                    if (Store) put_bytes(otp, v, a);
                    v = mask_first(v, a);
                } else if (Store) {
                    put(otp, loff, v);
                }
            }
            const uint32_t piece = row(0, v);                       // raw16: the row tables give 0 for S = 0
            const uint32_t behind = lane < j ? j - 1 - lane : 0;    // whole pieces after this lane's
            S = multmodp(lane_shift[63 - j], S) ^ multmodp(lane_shift[63 - behind], piece);
            S = multmodp(byte_shift[e], S);
            if (lane == j && e) {
                uint32_t c = 0;
                for (uint32_t q = tfirst && j == 0 ? a : 0; q < e; ++q) {
                    const uint8_t b = tp[16 * j + q];
                    c = (c >> 8) ^ T.tb[((c ^ b) & 0xFF) * 32];   // tbyte[0]
                    if (Store) otp[16 * j + q] = b;
                }
                S ^= c;
            }
        }
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) S ^= __shfl_xor(S, q);
        if (E.rpr == 1) {   // the record's only region: finish it here
            const uint32_t m = tfr_masked(tfr_crc_one(S, E.init));
            bool bad = false;
            if (lane < 16) {
                const uint32_t want = tfr_framing_byte(lane, E.record_size, E.len_mcrc, m);
                const uint64_t at = R.out + tfr_framing_at(lane, E.record_size);
                if (Store) dst[at] = (uint8_t)want;
                else bad = src[at] != want;
            } else if (Store && lane == 16 && idx) {
                const uint64_t len = E.record_size + kTfrFraming;
                *reinterpret_cast<ulonglong2 *>(idx + E.idx_off + 16 * R.rec) = make_ulonglong2(R.rec * len, len);
            }
            if (!Store) {
                const uint32_t bad16 = (uint32_t)__ballot(bad);
                if (bad16 && lane == 0) report(res + E.k, R.rec, bad16);
            }
        } else if (lane == 0) {
            raw[E.raw0 + (r - E.reg0)] = S;
        }
    }
}

// One thread per record of more than one region: the plan's fold over the
// record's raws, then the framing stored (or compared) and the index entry.
template <bool Store>
__global__ __launch_bounds__(256) __attribute__((flatten)) void k_tfrecord_fold(const uint8_t *src, uint8_t *dst, uint8_t *idx, const TfrShard *sh,
                                                       uint32_t nsh, uint64_t nlong, const uint32_t *raw, TfrDevRes *res) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nlong) return;
    const TfrShard E = sh[tfr_find_long(sh, nsh, t)];
    const uint64_t i = t - E.lrec0, len = E.record_size + kTfrFraming, out = E.dst_off + i * len;
    const uint32_t crc = tfr_crc_fold(raw + E.raw0 + i * E.rpr, E.rpr, E.rows, tfr_align(Store, i, E.record_size),
                                      E.record_size, E.init);
    const uint32_t m = tfr_masked(crc);
    uint32_t bad16 = 0;
    for (uint32_t l = 0; l < 16; ++l) {
        const uint32_t want = tfr_framing_byte(l, E.record_size, E.len_mcrc, m);
        const uint64_t at = out + tfr_framing_at(l, E.record_size);
        if (Store) dst[at] = (uint8_t)want;
        else bad16 |= (uint32_t)(src[at] != want) << l;
    }
    if (Store && idx) *reinterpret_cast<ulonglong2 *>(idx + E.idx_off + 16 * i) = make_ulonglong2(i * len, len);
    if (!Store && bad16) report(res + E.k, i, bad16);
}

}  // namespace

hipError_t tfrecord_launch(bool frame, const uint8_t *src, uint8_t *dst, uint8_t *idx, const uint8_t *table_dev,
                           const TfrCounts &C, void *tab_dev, int cus, TfrDevRes *res, hipStream_t s) {
    if (C.live == 0) return hipSuccess;
    const TfrShard *sh = reinterpret_cast<const TfrShard *>(table_dev);
    uint32_t *raw = reinterpret_cast<uint32_t *>(const_cast<uint8_t *>(table_dev) + tfr_raw_offset(C));
    const uint8_t *tab = (const uint8_t *)tab_dev;
    // 8-wave workgroups of 64 KiB LDS: two per CU, every wave looping over regions
    const uint64_t need = (C.regions + 7) / 8, fit = 2ull * (uint64_t)(cus > 0 ? cus : 256);
    const dim3 grid((uint32_t)(need < fit ? need : fit)), fgrid((uint32_t)((C.long_records + 255) / 256));
    (void)hipGetLastError();
    if (frame)
        hipLaunchKernelGGL(k_tfrecord_regions<true>, grid, dim3(512), 0, s, src, dst, idx, sh, (uint32_t)C.live, C.regions,
                           tab, raw, res);
    else
        hipLaunchKernelGGL(k_tfrecord_regions<false>, grid, dim3(512), 0, s, src, dst, idx, sh, (uint32_t)C.live,
                           C.regions, tab, raw, res);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || C.long_records == 0) return e;
    if (frame)
        hipLaunchKernelGGL(k_tfrecord_fold<true>, fgrid, dim3(256), 0, s, src, dst, idx, sh, (uint32_t)C.live,
                           C.long_records, (const uint32_t *)raw, res);
    else
        hipLaunchKernelGGL(k_tfrecord_fold<false>, fgrid, dim3(256), 0, s, src, dst, idx, sh, (uint32_t)C.live,
                           C.long_records, (const uint32_t *)raw, res);
    return hipGetLastError();
}

}  // namespace s3dg
