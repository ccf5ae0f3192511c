// s3dg_tfrecord_extract.hip — the payloads of indexed records copied out of
// framed streams and checked in the same pass (s3dg_tfrecord_extract_batch;
// DESIGN.md §5.5.4).  The only description is the index in device memory, so
// the plan that s3dg_tfrecord_frame_var_batch builds on the host is built
// here:
//
//   k_tfx_validate  one thread per entry of every take: the entry against its
//                   stream and its successor; the take's verdict (status 2 by
//                   any thread, status 1 by the thread of the last entry) and
//                   its payload bytes.
//   k_tfx_consts    one thread per entry: the record's A^len (~0) and
//                   masked_crc(len), its region count (none for a take that is
//                   not taken), and the compact list of long records.
//   the scan        region counts -> first regions (tfrecord_search_scan).
//   k_tfx_regions   k_tfrecord_var_regions with another way to the record and
//                   the lanes aligned to the destination: a wave takes a run of
//                   regions, finds its first record by one binary search over
//                   the first regions and steps from entry to entry and take to
//                   take in scalar registers.  A piece's 16 source bytes lie
//                   anywhere: four dwords from the multiple of 4 below them and
//                   a fifth when they start off it, shifted into place by
//                   v_alignbyte with one uniform count per record, hashed by
//                   the single-bank row step and stored as one aligned
//                   global_store_dwordx4.  The first and last pieces of a
//                   record go byte by byte where they are ragged.
//   k_tfx_fold      one thread per long record: tfr_crc_fold over its raws.
//
// The regions launch is sized from the host's bound; the number of regions is
// read from the scan's last element, and a workgroup without a region leaves
// before it loads the tables.
#include "s3dg_internal.h"

namespace s3dg {
namespace {

struct CrcTablesCF {
    uint32_t tb[256 * 32];
    uint32_t tr[256 * 32];
};
static_assert(sizeof(CrcTablesCF) == kCrcTabByteShiftOff - kCrcTabCfOff, "the uploaded tables' layout");

// 16 bytes at a multiple of 4: one global_load_dwordx4
struct __attribute__((packed, aligned(4))) Piece {
    uint32_t x, y, z, w;
};
// A piece as loaded: the dwords that hold its 16 bytes, before the byte shift.
struct Five {
    uint4 v;
    uint32_t w;
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

// A bad record of take k: one add per class it is bad in, the lowest record kept.
__device__ __forceinline__ void report(TfxDevRes *r, uint64_t rec, uint32_t bad16) {
    atomicAdd(&r->bad_records, 1ull);
    if (bad16 & 0x00FFu) atomicAdd(&r->bad_length, 1ull);
    if (bad16 & 0x0F00u) atomicAdd(&r->bad_length_crc, 1ull);
    if (bad16 & 0xF000u) atomicAdd(&r->bad_data_crc, 1ull);
    atomicMax(&r->first_inv, (unsigned long long)~rec);
}

__device__ __forceinline__ const ulonglong2 *take_entries(const uint8_t *idx, const TfxTake &T) {
    return reinterpret_cast<const ulonglong2 *>(idx + T.idx_off) + T.first;
}

__global__ __launch_bounds__(256) void k_tfx_validate(const uint8_t *__restrict__ idx, const TfxTake *__restrict__ tk, uint64_t n,
                                                      uint64_t nent, TfxDevRes *__restrict__ res) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nent) return;
    const uint64_t k = tfx_find_take(tk, n, j);
    const TfxTake T = tk[k];
    const ulonglong2 *ent = take_entries(idx, T);
    const uint64_t i = j - T.ent0;
    const ulonglong2 e = ent[i];
    const bool last = i + 1 == T.count;
    bool ok = tfx_entry_fits(e.x, e.y, T.bytes);
    if (ok && !last) ok = tfx_entry_chains(e.x, e.y, ent[i + 1].x);
    if (!ok) atomicMax(&res[k].status, 2ull);
    if (last && ok) {   // what another thread may still refuse makes this number meaningless and status 2
        const uint64_t payload = tfx_run_payload(ent[0].x, e.x, e.y, T.count);
        res[k].payload = payload;
        if (payload > T.dst_cap) atomicMax(&res[k].status, 1ull);
    }
}

__global__ __launch_bounds__(256) void k_tfx_consts(const uint8_t *__restrict__ idx, const uint32_t *__restrict__ pw,
                                                    const TfxTake *__restrict__ tk, uint64_t n, uint64_t nent, uint32_t rows,
                                                    const TfxDevRes *__restrict__ res, uint64_t *__restrict__ reg0,
                                                    TfvConst *__restrict__ cst, uint64_t *__restrict__ longs,
                                                    unsigned long long *__restrict__ nlong) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > nent) return;
    uint64_t nr = 0;
    if (j < nent) {
        const uint64_t k = tfx_find_take(tk, n, j);
        if (res[k].status == 0) {
            const TfxTake T = tk[k];
            const uint64_t len = take_entries(idx, T)[j - T.ent0].y - kTfrFraming;
            cst[j] = TfvConst{tfv_init(len, pw), tfv_len_mcrc(len)};
            nr = tfv_rec_regions(len, tfv_rec_rows(len, rows));
            if (nr > 1) longs[atomicAdd(nlong, 1ull)] = j;
        }
    }
    reg0[j] = nr;   // reg0[nent] = 0: the scan leaves the call's regions there
}

__global__ __launch_bounds__(512) void k_tfx_regions(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                     const uint8_t *__restrict__ idx, const TfxTake *__restrict__ tk, uint64_t n,
                                                     const uint64_t *__restrict__ reg0, const TfvConst *__restrict__ cst,
                                                     uint64_t nent, uint32_t call_rows, const uint8_t *__restrict__ crc_tab,
                                                     uint32_t *__restrict__ raw, TfxDevRes *__restrict__ res) {
    const uint64_t nreg = reg0[nent], per = tfv_run_len(nreg, (uint64_t)gridDim.x * 8);
    if ((uint64_t)blockIdx.x * 8 * per >= nreg) return;   // no region for this workgroup: before the tables and the barrier
    const CrcTablesCF *tabs = reinterpret_cast<const CrcTablesCF *>(crc_tab + kCrcTabCfOff);
    const uint32_t *lane_shift = reinterpret_cast<const uint32_t *>(crc_tab + kCrcTabLaneShiftOff);
    const uint32_t *byte_shift = reinterpret_cast<const uint32_t *>(crc_tab + kCrcTabByteShiftOff);
    __shared__ CrcTablesCF T;
    const uint32_t t = threadIdx.x, lane = t & 63;
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(tabs);
        uint4 *d = reinterpret_cast<uint4 *>(&T);
        for (uint32_t q = t; q < sizeof(CrcTablesCF) / 16; q += 512) d[q] = g[q];
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
    // the run's first record and its take, once; from here on the wave steps
    uint64_t j = tfx_find_rec(reg0, nent, r), k = tfx_find_take(tk, n, j);
    TfxTake E = tk[k];
    uint64_t e_end = tk[k + 1].ent0;
    const ulonglong2 *ent = take_entries(idx, E);
    uint64_t o_first = ent[0].x, r_lo = reg0[j], r_hi = reg0[j + 1];
    for (; r < r_end; ++r) {
        while (r_hi <= r) {   // entries without regions (a take not taken) are stepped over
            ++j;
            r_lo = r_hi;
            r_hi = reg0[j + 1];
        }
        if (e_end <= j) {
            do {
                ++k;
                e_end = tk[k + 1].ent0;
            } while (e_end <= j);
            E = tk[k];
            ent = take_entries(idx, E);
            o_first = ent[0].x;
        }
        const uint64_t i = j - E.ent0;
        const ulonglong2 e = ent[i];
        const uint64_t len = e.y - kTfrFraming, rec_at = E.off + e.x;   // the record's header, from src
        const uint64_t out = E.dst_off + tfx_dst_pos(o_first, e.x, i);   // its payload, from dst
        const uint32_t a = (uint32_t)(out & 15u), rpr = (uint32_t)(r_hi - r_lo), g = (uint32_t)(r - r_lo);
        const TfxRegion R = tfx_region(a, len, g, rpr, tfv_rec_rows(len, call_rows));
        const uint32_t nrows = R.nrows;
        // the region's first piece: 16-byte aligned in the destination, anywhere in the stream
        uint8_t *obase = dst + (out - a) + R.pad_lo;
        const uint8_t *sbase = src + (rec_at + kTfrHeader - a) + R.pad_lo;
        const uint32_t u = (uint32_t)(reinterpret_cast<uintptr_t>(sbase) & 3u);
        const uint8_t *s4 = sbase - u;
        const bool first = g == 0 && a != 0;   // its first a bytes are not the record's
        auto get = [&](const uint8_t *o, uint32_t off) -> Five {
            const Piece p = *reinterpret_cast<const Piece *>(o + off);
            const uint32_t w = u ? *reinterpret_cast<const uint32_t *>(o + off + 16) : 0u;
            return Five{make_uint4(p.x, p.y, p.z, p.w), w};
        };
        // the record's first piece: only the dwords that hold one of its bytes
        auto get_first = [&](const uint8_t *o) -> Five {
            const uint32_t *q = reinterpret_cast<const uint32_t *>(o);
            uint32_t w[5];
#pragma unroll
            for (uint32_t d = 0; d < 5; ++d) w[d] = tfx_first_needs(d, a, u) ? q[d] : 0u;
            return Five{make_uint4(w[0], w[1], w[2], w[3]), w[4]};
        };
        auto fix = [&](const Five &f) -> uint4 {
            return make_uint4(__builtin_amdgcn_alignbyte(f.v.y, f.v.x, u), __builtin_amdgcn_alignbyte(f.v.z, f.v.y, u),
                              __builtin_amdgcn_alignbyte(f.v.w, f.v.z, u), __builtin_amdgcn_alignbyte(f.w, f.v.w, u));
        };
        auto put = [&](uint8_t *o, uint32_t off, const uint4 v) { *reinterpret_cast<uint4 *>(o + off) = v; };
        const uint32_t loff = lane * 16;
        uint32_t S = 0, rw = 0;
        if (first && nrows) {   // the record's first row on its own: lane 0's piece is masked
            uint4 v;
            if (lane == 0) {
                v = fix(get_first(s4));
                put_bytes(obase, v, a);
                v = mask_first(v, a);
            } else {
                v = fix(get(s4, loff));
                put(obase, loff, v);
            }
            S = row(0, v);
            rw = 1;
        }
        auto load4 = [&](Five (&f)[4], uint32_t r0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t rr = r0 + q < nrows ? r0 + q : nrows - 1;
                f[q] = get(s4, rr * kCrcRowBytes + loff);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        auto hash4 = [&](const Five (&f)[4], uint32_t r0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 v = fix(f[q]);
                S = row(S, v);
                put(obase, (r0 + q) * kCrcRowBytes + loff, v);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        Five A[4], B[4];
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
            const uint4 v = fix(get(s4, rw * kCrcRowBytes + loff));
            S = row(S, v);
            put(obase, rw * kCrcRowBytes + loff, v);
        }
        S = multmodp(lane_shift[lane], S);              // A^(16 (63 - lane))
        if (R.tail) {
            const uint32_t jp = R.tail >> 4, eb = R.tail & 15;
            const uint8_t *tp = s4 + (uint64_t)nrows * kCrcRowBytes;
            uint8_t *otp = obase + (uint64_t)nrows * kCrcRowBytes;   // both uniform
            const bool tfirst = first && nrows == 0;         // the record's first piece is in the tail
            uint4 v = make_uint4(0, 0, 0, 0);
            if (lane < jp) {
                if (tfirst && lane == 0) {
                    v = fix(get_first(tp));
                    put_bytes(otp, v, a);
                    v = mask_first(v, a);
                } else {
                    v = fix(get(tp, loff));
                    put(otp, loff, v);
                }
            }
            const uint32_t piece = row(0, v);                        // raw16: the row tables give 0 for S = 0
            const uint32_t behind = lane < jp ? jp - 1 - lane : 0;   // whole pieces after this lane's
            S = multmodp(lane_shift[63 - jp], S) ^ multmodp(lane_shift[63 - behind], piece);
            S = multmodp(byte_shift[eb], S);
            if (lane == jp && eb) {   // the ragged end, byte by byte from wherever it lies
                uint32_t c = 0;
                for (uint32_t q = tfirst && jp == 0 ? a : 0; q < eb; ++q) {
                    const uint8_t b = tp[u + 16 * jp + q];
                    c = (c >> 8) ^ T.tb[((c ^ b) & 0xFF) * 32];   // tbyte[0]
                    otp[16 * jp + q] = b;
                }
                S ^= c;
            }
        }
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) S ^= __shfl_xor(S, q);
        if (rpr == 1) {   // the record's only region: judge it here, header and footer byte by byte
            const TfvConst K = cst[j];
            const uint32_t m = tfr_masked(tfr_crc_one(S, K.init));
            bool bad = false;
            if (lane < 16) bad = src[rec_at + tfr_framing_at(lane, len)] != tfr_framing_byte(lane, len, K.len_mcrc, m);
            const uint32_t bad16 = (uint32_t)__ballot(bad);
            if (bad16 && lane == 0) report(res + k, E.first + i, bad16);
        } else if (lane == 0) {
            raw[r] = S;
        }
    }
}

// One thread per record of more than one region: the plan's fold over the
// record's raws, then its header and footer compared.
__global__ __launch_bounds__(256) __attribute__((flatten)) void k_tfx_fold(
    const uint8_t *src, const uint8_t *idx, const TfxTake *tk, uint64_t n, const uint64_t *reg0, const TfvConst *cst,
    const uint64_t *longs, const unsigned long long *nlong, uint32_t call_rows, const uint32_t *raw, TfxDevRes *res) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= *nlong) return;
    const uint64_t j = longs[t], k = tfx_find_take(tk, n, j);
    const TfxTake E = tk[k];
    const ulonglong2 *ent = take_entries(idx, E);
    const uint64_t i = j - E.ent0;
    const ulonglong2 e = ent[i];
    const TfvConst K = cst[j];
    const uint64_t len = e.y - kTfrFraming, rec_at = E.off + e.x;
    const uint32_t a = (uint32_t)((E.dst_off + tfx_dst_pos(ent[0].x, e.x, i)) & 15u);
    const uint32_t crc = tfr_crc_fold(raw + reg0[j], (uint32_t)(reg0[j + 1] - reg0[j]), tfv_rec_rows(len, call_rows), a, len, K.init);
    const uint32_t m = tfr_masked(crc);
    uint32_t bad16 = 0;
    for (uint32_t l = 0; l < 16; ++l)
        bad16 |= (uint32_t)(src[rec_at + tfr_framing_at(l, len)] != tfr_framing_byte(l, len, K.len_mcrc, m)) << l;
    if (bad16) report(res + k, E.first + i, bad16);
}

}  // namespace

hipError_t tfrecord_extract_launch(const uint8_t *src, const uint8_t *idx, uint8_t *dst, uint8_t *ws, const TfxLayout &L,
                                   const TfxCounts &C, uint64_t n, size_t scan_tmp_bytes, void *tab_dev, int cus,
                                   hipEvent_t *marks, hipStream_t s) {
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(ws);
    const TfxTake *tk = reinterpret_cast<const TfxTake *>(ws + kTfxTakeOff);
    unsigned long long *nlong = reinterpret_cast<unsigned long long *>(ws + L.res);
    TfxDevRes *res = reinterpret_cast<TfxDevRes *>(ws + L.res + kTfxCounterBytes);
    uint64_t *reg0 = reinterpret_cast<uint64_t *>(ws + L.reg0);
    TfvConst *cst = reinterpret_cast<TfvConst *>(ws + L.cst);
    uint64_t *longs = reinterpret_cast<uint64_t *>(ws + L.longs);
    uint32_t *raw = reinterpret_cast<uint32_t *>(ws + L.raw);
    auto mark = [&](int m) -> hipError_t { return marks ? hipEventRecord(marks[m], s) : hipSuccess; };
    (void)hipGetLastError();
    hipError_t e = mark(0);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tfx_validate, dim3((uint32_t)((C.ents + 255) / 256)), dim3(256), 0, s, idx, tk, n, C.ents, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_tfx_consts, dim3((uint32_t)((C.ents + 1 + 255) / 256)), dim3(256), 0, s, idx, pw, tk, n, C.ents, C.rows,
                       (const TfxDevRes *)res, reg0, cst, longs, nlong);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = mark(1)) != hipSuccess) return e;
    if ((e = tfrecord_search_scan(ws + L.tmp, &scan_tmp_bytes, reg0, C.ents, s)) != hipSuccess) return e;
    if ((e = mark(2)) != hipSuccess) return e;
    // 8-wave workgroups of 64 KiB LDS: two per CU, every wave one run of regions
    const uint64_t need = (C.max_regions + 7) / 8, fit = 2ull * (uint64_t)(cus > 0 ? cus : 256);
    hipLaunchKernelGGL(k_tfx_regions, dim3((uint32_t)(need < fit ? need : fit)), dim3(512), 0, s, src, dst, idx, tk, n,
                       (const uint64_t *)reg0, (const TfvConst *)cst, C.ents, C.rows, (const uint8_t *)tab_dev, raw, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (C.max_long) {
        hipLaunchKernelGGL(k_tfx_fold, dim3((uint32_t)((C.max_long + 255) / 256)), dim3(256), 0, s, src, idx, tk, n,
                           (const uint64_t *)reg0, (const TfvConst *)cst, (const uint64_t *)longs,
                           (const unsigned long long *)nlong, C.rows, (const uint32_t *)raw, res);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return mark(3);
}

}  // namespace s3dg
