// s3dg_npz_batch.hip — a list of NPZ archives written into device memory and
// checked there (s3dg_npz_frame_batch, s3dg_npz_check_batch).
// The plan is the host's (s3dg_npz_plan.h): one 64-byte entry per member, the
// ready-made fronts (local header, name, NPY header) and backs (central
// directory, end record) with their CRC fields zero.
//
//   k_npz_regions<Store>  a wave takes a run of regions, finds its member by
//                         one binary search over the first regions and steps
//                         from entry to entry in scalar registers.  The lanes
//                         are aligned to the destination: a member's payload
//                         lands a bytes past a 16-byte boundary, another a for
//                         every member, and the wave hashes the a + size bytes
//                         from that boundary with the first a masked.  Store:
//                         a piece's 16 source bytes are four dwords from the
//                         multiple of 4 below them and a fifth when they start
//                         off it, shifted by v_alignbyte with one uniform count
//                         per member, hashed by the single-bank row step and
//                         stored as one aligned global_store_dwordx4; the
//                         ragged first and last piece go byte by byte, so no
//                         header byte is touched.  A member of zeros loads
//                         nothing.  Check: the same walk over the archive's own
//                         bytes, nothing stored.  One raw CRC per region.
//   k_npz_finish<Store>   a wave per member: its CRC as a sum of terms, a lane
//                         per region and one for the NPY header's CRC
//                         (crc(h || p) = crc(h) x^(8 |p|) ^ crc(p), through
//                         the power table); then the front with the CRC at
//                         +14 and the central entry with the CRC at +16, 64
//                         bytes a step; the wave of an archive's first member
//                         takes the end record.  Store writes those bytes,
//                         check compares them and reports on the bad path only.
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

// Store: src -> dst.  Check: dst is the archives' base and is only read.
template <bool Store>
__global__ __launch_bounds__(512) void k_npz_regions(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                     const NpzEnt *__restrict__ ent, uint64_t ents, uint64_t nreg,
                                                     uint32_t call_rows, const uint8_t *__restrict__ crc_tab,
                                                     uint32_t *__restrict__ raw) {
    const uint64_t per = tfv_run_len(nreg, (uint64_t)gridDim.x * 8);
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
    uint64_t j = npz_find_ent(ent, ents, r);
    NpzEnt E = ent[j];
    uint64_t r_hi = ent[j + 1].reg0;
    for (; r < r_end; ++r) {
        if (r_hi <= r) {   // members without regions are stepped over
            do {
                ++j;
                r_hi = ent[j + 1].reg0;
            } while (r_hi <= r);
            E = ent[j];
        }
        const uint32_t a = (uint32_t)(E.dst & 15u), rpr = (uint32_t)(r_hi - E.reg0), g = (uint32_t)(r - E.reg0);
        const TfxRegion R = tfx_region(a, E.size, g, rpr, tfv_rec_rows(E.size, call_rows));
        const uint32_t nrows = R.nrows;
        const bool zero = Store && E.src == S3DG_NPZ_ZEROS;   // nothing is loaded
        // the region's first piece: 16-byte aligned in the destination, anywhere in the source
        uint8_t *obase = dst + (E.dst - a) + R.pad_lo;
        const uint8_t *sbase = zero || !Store ? obase : src + (E.src - a) + R.pad_lo;
        const uint32_t u = (uint32_t)(reinterpret_cast<uintptr_t>(sbase) & 3u);
        const uint8_t *s4 = sbase - u;
        const bool first = g == 0 && a != 0;   // its first a bytes are not the member's
        auto get = [&](const uint8_t *o, uint32_t off) -> Five {
            if (zero) return Five{make_uint4(0, 0, 0, 0), 0u};
            const Piece p = *reinterpret_cast<const Piece *>(o + off);
            const uint32_t w = u ? *reinterpret_cast<const uint32_t *>(o + off + 16) : 0u;
            return Five{make_uint4(p.x, p.y, p.z, p.w), w};
        };
        // the member's first piece: only the dwords that hold one of its bytes
        auto get_first = [&](const uint8_t *o) -> Five {
            if (zero) return Five{make_uint4(0, 0, 0, 0), 0u};
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
        auto put = [&](uint8_t *o, uint32_t off, const uint4 v) {
            if (Store) *reinterpret_cast<uint4 *>(o + off) = v;
        };
        const uint32_t loff = lane * 16;
        uint32_t S = 0, rw = 0;
        if (first && nrows) {   // the member's first row on its own: lane 0's piece is masked
            uint4 v;
            if (lane == 0) {
                v = fix(get_first(s4));
                if (Store) put_bytes(obase, v, a);
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
            const bool tfirst = first && nrows == 0;         // the member's first piece is in the tail
            uint4 v = make_uint4(0, 0, 0, 0);
            if (lane < jp) {
                if (tfirst && lane == 0) {
                    v = fix(get_first(tp));
                    if (Store) put_bytes(otp, v, a);
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
                    const uint8_t b = zero ? (uint8_t)0 : tp[u + 16 * jp + q];
                    c = (c >> 8) ^ T.tb[((c ^ b) & 0xFF) * 32];   // tbyte[0]
                    if (Store) otp[16 * jp + q] = b;
                }
                S ^= c;
            }
        }
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) S ^= __shfl_xor(S, q);
        if (lane == 0) raw[r] = S;
    }
}

// One wave per member.  Store: base is dst_base; check: the archives' base.
template <bool Store>
__global__ __launch_bounds__(256) __attribute__((flatten)) void k_npz_finish(uint8_t *__restrict__ base, const uint8_t *__restrict__ ws,
                                                    const NpzArch *__restrict__ arch, const NpzEnt *__restrict__ ent,
                                                    uint64_t ents, uint32_t call_rows, const uint32_t *__restrict__ raw,
                                                    NpzDevRes *__restrict__ res) {
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t j = (uint64_t)blockIdx.x * 4 + wave;
    if (j >= ents) return;
    const NpzEnt E = ent[j];
    const NpzArch A = arch[E.arch];
    // the member's CRC: a term per region and one for the NPY header, 64 a step
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(ws);
    const uint32_t nreg = (uint32_t)(ent[j + 1].reg0 - E.reg0), rec_rows = tfv_rec_rows(E.size, call_rows);
    uint32_t acc = 0;
    for (uint32_t t = lane; t <= nreg; t += 64)
        acc ^= npz_member_term(t, E.hcrc, raw + E.reg0, nreg, rec_rows, (uint32_t)(E.dst & 15u), E.size, pw);
#pragma unroll
    for (int q = 32; q >= 1; q >>= 1) acc ^= __shfl_xor(acc, q);
    const uint32_t crc = ~acc;
    uint8_t *front = base + (E.dst - E.front_len), *cen = base + A.back_dst + E.cen;
    const uint8_t *fb = ws + E.front, *cb = ws + A.back + E.cen;
    auto crc_byte = [&](uint32_t i) -> uint8_t { return (uint8_t)(crc >> (8 * i)); };
    if (Store) {
        for (uint32_t i = lane; i < E.front_len; i += 64) front[i] = i - kNpzLocalCrc < 4 ? crc_byte(i - kNpzLocalCrc) : fb[i];
        for (uint32_t i = lane; i < E.cen_len; i += 64) cen[i] = i - kNpzCentralCrc < 4 ? crc_byte(i - kNpzCentralCrc) : cb[i];
        if (E.mem == 0 && lane < kNpzEnd) base[A.back_dst + A.cd_len + lane] = ws[A.back + A.cd_len + lane];
        return;
    }
    bool bad_local = false, bad_crc = false, bad_dir = false;
    uint32_t lf = 0, cf = 0;   // the two CRC fields as they lie in memory
    for (uint32_t q = 0; q < 4; ++q) {
        lf |= (uint32_t)front[kNpzLocalCrc + q] << (8 * q);
        cf |= (uint32_t)cen[kNpzCentralCrc + q] << (8 * q);
    }
    bad_crc = lf != crc;
    bad_dir = npz_central_crc_bad(cf, crc, lf);
    for (uint32_t i = lane; i < E.front_len; i += 64) bad_local |= i - kNpzLocalCrc >= 4 && front[i] != fb[i];
    for (uint32_t i = lane; i < E.cen_len; i += 64) bad_dir |= i - kNpzCentralCrc >= 4 && cen[i] != cb[i];
    if (E.mem == 0 && lane < kNpzEnd) bad_dir |= base[A.back_dst + A.cd_len + lane] != ws[A.back + A.cd_len + lane];
    const bool any_local = __ballot(bad_local) != 0, any_dir = __ballot(bad_dir) != 0;
    if (lane == 0 && (any_local || bad_crc || any_dir)) {
        NpzDevRes *r = res + E.arch;
        if (any_local || bad_crc) {
            atomicAdd(&r->bad_members, 1ull);
            if (any_local) atomicAdd(&r->bad_local, 1ull);
            if (bad_crc) atomicAdd(&r->bad_crc, 1ull);
            atomicMax(&r->first_inv, (unsigned long long)~(uint64_t)E.mem);
        }
        if (any_dir) atomicMax(&r->bad_directory, 1ull);
    }
}

template <bool Store>
hipError_t launch(const uint8_t *src, uint8_t *base, uint8_t *ws, const NpzLayout &L, const NpzCounts &C, void *tab_dev,
                  int cus, hipStream_t s) {
    const NpzArch *arch = reinterpret_cast<const NpzArch *>(ws + L.arch);
    const NpzEnt *ent = reinterpret_cast<const NpzEnt *>(ws + L.ent);
    uint32_t *raw = reinterpret_cast<uint32_t *>(ws + L.raw);
    (void)hipGetLastError();
    hipError_t e;
    if (C.regions) {
        // 8-wave workgroups of 64 KiB LDS: two per CU, every wave one run of regions
        const uint64_t need = (C.regions + 7) / 8, fit = 2ull * (uint64_t)(cus > 0 ? cus : 256);
        hipLaunchKernelGGL(k_npz_regions<Store>, dim3((uint32_t)(need < fit ? need : fit)), dim3(512), 0, s, src, base, ent, C.ents,
                           C.regions, C.rows, (const uint8_t *)tab_dev, raw);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_npz_finish<Store>, dim3((uint32_t)((C.ents + 3) / 4)), dim3(256), 0, s, base, (const uint8_t *)ws, arch,
                       ent, C.ents, C.rows, (const uint32_t *)raw, reinterpret_cast<NpzDevRes *>(ws + L.res));
    return hipGetLastError();
}

}  // namespace

hipError_t npz_batch_launch(bool frame, const uint8_t *src, uint8_t *base, uint8_t *ws, const NpzLayout &L,
                            const NpzCounts &C, void *tab_dev, int cus, hipStream_t s) {
    // check: the regions read the archives themselves
    return frame ? launch<true>(src, base, ws, L, C, tab_dev, cus, s) : launch<false>(base, base, ws, L, C, tab_dev, cus, s);
}

}  // namespace s3dg
