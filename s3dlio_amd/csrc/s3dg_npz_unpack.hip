// s3dg_npz_unpack.hip — stored ZIP archives indexed from nothing but their
// bytes (s3dg_npz_index_batch) and their members' array bytes copied out by
// that index with the CRC-32 checked in the copy (s3dg_npz_unpack_batch;
// DESIGN.md §5.5.6).
//
//   k_nzi_walk      one wave per archive.  The end record is searched backwards,
//                   64 positions a step; then the wave steps from central entry
//                   to central entry in scalar registers.  A header lies at any
//                   byte address, so the wave reads it as a unit: each lane
//                   loads one byte (22 lanes for the end record, 46 for a
//                   central entry, 30 for a local header, 12 for the NPY
//                   preamble) and the fields are assembled across lanes by
//                   v_readlane.  Names are compared 64 bytes a step by ballot.
//                   Every load is bounded by the archive first.
//   k_nzu_validate  one thread per entry of every take: the entry against its
//                   archive (status 2 by any thread), its packed size and its
//                   payload bytes for the two sums.
//   k_nzu_consts    one thread per entry: the take's verdict from the sums
//                   (status 1, span and bytes by the thread of the first entry),
//                   the member's A^len (~0), its region count (none for a take
//                   that is not taken) and the compact list of long members.
//   k_nzu_regions   k_tfx_regions with the run starting in front of the
//                   destination: a member's NPY header lies directly in front
//                   of its payload, so the hashed run begins ceil(hdr_len / 16)
//                   pieces before the payload's 16-byte aligned destination and
//                   those pieces are hashed with their store suppressed.  Only
//                   a member's last piece is ragged on the store side.  A
//                   piece's 16 source bytes lie anywhere: four dwords from the
//                   multiple of 4 below them and a fifth when they start off
//                   it, shifted into place by v_alignbyte with one uniform
//                   count per member.
//   k_nzu_fold      one thread per long member: tfr_crc_fold over its raws.
#include "s3dg_internal.h"
#include "s3dg_npz_unpack_plan.h"

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

// ---- the walk ------------------------------------------------------------------------------
// n bytes (at most 64) at p, one per lane; the others hold 0.
__device__ __forceinline__ uint32_t wave_bytes(const uint8_t *p, uint32_t n, uint32_t lane) {
    return lane < n ? (uint32_t)p[lane] : 0u;
}
// The little-endian field of N bytes at lane `at` of such a load, in a scalar register.
template <int N>
__device__ __forceinline__ uint32_t field(uint32_t b, int at) {
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) v |= (uint32_t)__builtin_amdgcn_readlane((int)b, at + q) << (8 * q);
    return v;
}

// Both sizes of a local header whose size fields are ZIP64 markers, from the
// 0x0001 record of its extra field x[0, xl): true when they equal `size`.
__device__ __forceinline__ bool extra_sizes(const uint8_t *x, uint32_t xl, uint32_t size, uint32_t lane) {
    uint32_t at = 0;
    while (at + 4 <= xl) {
        const uint32_t left = xl - at, b = wave_bytes(x + at, left < 20 ? left : 20, lane);
        const uint32_t id = field<2>(b, 0), len = field<2>(b, 2);
        if (len > left - 4) return false;
        if (id == 1) return len >= 16 && field<4>(b, 4) == size && field<4>(b, 8) == 0 && field<4>(b, 12) == size && field<4>(b, 16) == 0;
        at += 4 + len;
    }
    return false;
}

__global__ __launch_bounds__(64) void k_nzi_walk(const uint8_t *__restrict__ base, uint8_t *__restrict__ table,
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
        // candidate d: the end record at bytes - 22 - d with a comment of d bytes
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
            // the central entry
            if (c + kNpzCentral > cd_end) {
                R.status = S3DG_NPZ_WALK_DIRECTORY;
                break;
            }
            const uint32_t ce = wave_bytes(p + c, (uint32_t)kNpzCentral, lane);
            const uint32_t flags = field<2>(ce, 8), method = field<2>(ce, 10), crc = field<4>(ce, 16);
            const uint32_t stored = field<4>(ce, 24), name_len = field<2>(ce, 28), local_off = field<4>(ce, 42);
            const uint64_t c_next = c + kNpzCentral + name_len + field<2>(ce, 30) + field<2>(ce, 32);
            const uint32_t csize = field<4>(ce, 20);
            if (!nzi_central_ok(field<4>(ce, 0), csize, stored, field<2>(ce, 34), local_off) || c_next > cd_end ||
                (uint64_t)local_off + kNpzLocal > cd_off) {
                R.status = S3DG_NPZ_WALK_DIRECTORY;
                break;
            }
            if (!nzi_supported(flags, method)) {
                R.status = S3DG_NPZ_WALK_UNSUPPORTED;
                break;
            }
            if (csize != stored) {
                R.status = S3DG_NPZ_WALK_DIRECTORY;
                break;
            }
            // the local header
            const uint32_t lh = wave_bytes(p + local_off, (uint32_t)kNpzLocal, lane);
            const uint32_t lname = field<2>(lh, 26), lextra = field<2>(lh, 28), lc = field<4>(lh, 18), lu = field<4>(lh, 22);
            const uint64_t file_at = (uint64_t)local_off + kNpzLocal + lname + lextra;
            if (file_at + stored > cd_off) {
                R.status = S3DG_NPZ_WALK_DIRECTORY;
                break;
            }
            bool same = field<4>(lh, 0) == kNzuSigLocal && field<2>(lh, 6) == flags && field<2>(lh, 8) == method &&
                        field<4>(lh, 14) == crc && lname == name_len;
            if (same) {
                if (lc == 0xFFFFFFFFu && lu == 0xFFFFFFFFu) same = extra_sizes(p + local_off + kNpzLocal + lname, lextra, stored, lane);
                else same = lc == stored && lu == stored;
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
            // the NPY preamble
            const uint32_t pb = wave_bytes(p + file_at, stored < 12 ? stored : 12u, lane);
            uint8_t pre[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) pre[q] = (uint8_t)field<1>(pb, q);
            const uint32_t hdr_len = nzi_npy_header(pre, stored), size = stored - hdr_len;
            const uint32_t e[8] = {local_off, name_len | flags << 16, (uint32_t)file_at, hdr_len, (uint32_t)file_at + hdr_len, size, crc, 0u};
            uint32_t mine = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) mine = lane == (uint32_t)q ? e[q] : mine;
            if (lane < 8) out[8 * (uint64_t)i + lane] = mine;
            R.payload_bytes += size;
            R.packed_bytes += nzu_packed(size);
            c = c_next;
        }
        R.members = i;
        if (R.status == S3DG_NPZ_WALK_OK && c != cd_end) {   // the entries do not end where the directory does
            R.status = S3DG_NPZ_WALK_DIRECTORY;
            R.bad_member = kNzuNone;
        }
        if (R.status == S3DG_NPZ_WALK_OK || R.status == S3DG_NPZ_WALK_CAPPED) R.bad_member = kNzuNone;
    }
    if (lane == 0) res[k] = R;
    }
}

// ---- the unpack ----------------------------------------------------------------------------
__device__ __forceinline__ NzuEntry load_entry(const uint8_t *tab, const TfxTake &T, uint64_t i) {
    const uint4 *q = reinterpret_cast<const uint4 *>(tab + T.idx_off) + 2 * (T.first + i);
    const uint4 lo = q[0], hi = q[1];
    return NzuEntry{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

__device__ __forceinline__ void report(NzuDevRes *r, uint64_t mem) {
    atomicAdd(&r->bad_crc, 1ull);
    atomicMax(&r->first_inv, (unsigned long long)~mem);
}

__global__ __launch_bounds__(256) void k_nzu_validate(const uint8_t *__restrict__ tab, const TfxTake *__restrict__ tk, uint64_t n,
                                                      uint64_t nent, NzuDevRes *__restrict__ res, uint64_t *__restrict__ pk,
                                                      uint64_t *__restrict__ sz) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > nent) return;
    uint64_t size = 0;
    if (j < nent) {
        const uint64_t k = tfx_find_take(tk, n, j);
        const TfxTake T = tk[k];
        const NzuEntry e = load_entry(tab, T, j - T.ent0);
        if (!nzu_entry_fits(e, T.bytes)) atomicMax(&res[k].status, 2ull);
        size = e.size;
    }
    pk[j] = nzu_packed(size);   // [nent] = 0: the scans leave the call's sums there
    sz[j] = size;
}

__global__ __launch_bounds__(256) void k_nzu_consts(const uint8_t *__restrict__ tab, const uint32_t *__restrict__ pw,
                                                    const TfxTake *__restrict__ tk, uint64_t n, uint64_t nent, uint32_t rows,
                                                    NzuDevRes *__restrict__ res, const uint64_t *__restrict__ pk,
                                                    const uint64_t *__restrict__ sz, uint64_t *__restrict__ reg0,
                                                    uint32_t *__restrict__ cst, uint64_t *__restrict__ longs,
                                                    unsigned long long *__restrict__ nlong, uint64_t max_long) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j > nent) return;
    uint64_t nr = 0;
    if (j < nent) {
        const uint64_t k = tfx_find_take(tk, n, j);
        const TfxTake T = tk[k];
        // status 2 is final since the validation; status 1 follows from the span, the same for every thread of the take
        const bool table_ok = res[k].status != 2ull;
        const uint64_t span = pk[T.ent0 + T.count] - pk[T.ent0];
        if (j == T.ent0 && table_ok) {
            res[k].span = span;
            if (span > T.dst_cap) atomicMax(&res[k].status, 1ull);
            else res[k].bytes = sz[T.ent0 + T.count] - sz[T.ent0];
        }
        if (table_ok && span <= T.dst_cap) {
            const uint64_t i = j - T.ent0;
            const NzuEntry e = load_entry(tab, T, i);
            const uint64_t len = (uint64_t)e.hdr_len + e.size;
            cst[j] = tfv_init(len, pw);
            nr = nzu_regions(len, rows);
            if (nr > 1) {
                const uint64_t slot = atomicAdd(nlong, 1ull);
                if (slot < max_long) longs[slot] = j;   // always, by the host's bound
            }
            if (len == 0 && e.crc != 0) report(res + k, T.first + i);   // no region judges a stored file of no bytes
        }
    }
    reg0[j] = nr;   // reg0[nent] = 0: the scan leaves the call's regions there
}

__global__ __launch_bounds__(512) void k_nzu_regions(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                     const uint8_t *__restrict__ tab, const TfxTake *__restrict__ tk, uint64_t n,
                                                     const uint64_t *__restrict__ reg0, const uint64_t *__restrict__ pk,
                                                     const uint32_t *__restrict__ cst, uint64_t nent, uint64_t max_regions,
                                                     uint32_t call_rows, const uint8_t *__restrict__ crc_tab,
                                                     uint32_t *__restrict__ raw, NzuDevRes *__restrict__ res) {
    const uint64_t counted = reg0[nent], nreg = counted < max_regions ? counted : max_regions;   // the raws' room, whatever the table says
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
    // the run's first member and its take, once; from here on the wave steps
    uint64_t j = tfx_find_rec(reg0, nent, r), k = tfx_find_take(tk, n, j);
    TfxTake E = tk[k];
    uint64_t e_end = tk[k + 1].ent0, pk0 = pk[E.ent0];
    uint64_t r_lo = reg0[j], r_hi = reg0[j + 1];
    for (; r < r_end; ++r) {
        while (r_hi <= r) {   // entries without regions (a take not taken, an empty file) are stepped over
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
            pk0 = pk[E.ent0];
        }
        const uint64_t i = j - E.ent0;
        const NzuEntry e = load_entry(tab, E, i);
        const uint32_t hp = nzu_hdr_pieces(e.hdr_len), a = nzu_align(e.hdr_len);
        const uint64_t len = (uint64_t)e.hdr_len + e.size;
        const uint64_t out = E.dst_off + (pk[j] - pk0);   // the payload, from dst: a multiple of 16
        const uint32_t rpr = (uint32_t)(r_hi - r_lo), g = (uint32_t)(r - r_lo);
        const uint32_t rec_rows = tfv_rec_rows(len, call_rows);
        const TfxRegion R = tfx_region(a, len, g, rpr, rec_rows);
        const uint32_t nrows = R.nrows;
        const uint64_t piece0 = R.pad_lo / 16;   // the region's first piece among the member's
        // the region's first piece: 16-byte aligned in the destination (16 hp bytes in
        // front of the payload's, never dereferenced below it), anywhere in the archive
        uint8_t *obase = dst + out - 16ull * hp + R.pad_lo;
        const uint8_t *sbase = src + (E.off + e.hdr_off - a) + R.pad_lo;
        const uint32_t u = (uint32_t)(reinterpret_cast<uintptr_t>(sbase) & 3u);
        const uint8_t *s4 = sbase - u;
        const bool first = g == 0 && a != 0;   // its first a bytes are not the member's
        auto get = [&](const uint8_t *o, uint32_t off) -> Five {
            const Piece p = *reinterpret_cast<const Piece *>(o + off);
            const uint32_t w = u ? *reinterpret_cast<const uint32_t *>(o + off + 16) : 0u;
            return Five{make_uint4(p.x, p.y, p.z, p.w), w};
        };
        // the member's first piece: only the dwords that hold one of its bytes
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
        // rows that hold a header piece: hashed whole, stored from piece hp on
        const uint32_t hrows = nzu_header_rows(hp, R.pad_lo / kCrcRowBytes, nrows);
        for (; rw < hrows; ++rw) {
            uint4 v;
            if (first && rw == 0 && lane == 0) v = mask_first(fix(get_first(s4)), a);
            else v = fix(get(s4, rw * kCrcRowBytes + loff));
            if (piece0 + 64ull * rw + lane >= hp) put(obase, rw * kCrcRowBytes + loff, v);
            S = row(S, v);
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
            const uint64_t tpiece = piece0 + 64ull * nrows;
            const bool tfirst = first && nrows == 0;         // the member's first piece is in the tail
            uint4 v = make_uint4(0, 0, 0, 0);
            if (lane < jp) {
                if (tfirst && lane == 0) v = mask_first(fix(get_first(tp)), a);
                else v = fix(get(tp, loff));
                if (tpiece + lane >= hp) put(otp, loff, v);
            }
            const uint32_t piece = row(0, v);                        // raw16: the row tables give 0 for S = 0
            const uint32_t behind = lane < jp ? jp - 1 - lane : 0;   // whole pieces after this lane's
            S = multmodp(lane_shift[63 - jp], S) ^ multmodp(lane_shift[63 - behind], piece);
            S = multmodp(byte_shift[eb], S);
            // the ragged end, byte by byte from wherever it lies: payload, the header ends on a piece
            if (lane == jp && eb) {
                uint32_t c = 0;
                for (uint32_t q = 0; q < eb; ++q) {
                    const uint8_t b = tp[u + 16 * jp + q];
                    c = (c >> 8) ^ T.tb[((c ^ b) & 0xFF) * 32];   // tbyte[0]
                    otp[16 * jp + q] = b;
                }
                S ^= c;
            }
        }
#pragma unroll
        for (int q = 32; q >= 1; q >>= 1) S ^= __shfl_xor(S, q);
        if (rpr == 1) {   // the member's only region: judge it here
            if (lane == 0 && tfr_crc_one(S, cst[j]) != e.crc) report(res + k, E.first + i);
        } else if (lane == 0) {
            raw[r] = S;
        }
    }
}

// One thread per member of more than one region: the plan's fold over its raws.
__global__ __launch_bounds__(256) __attribute__((flatten)) void k_nzu_fold(
    const uint8_t *tab, const TfxTake *tk, uint64_t n, const uint64_t *reg0, const uint32_t *cst, const uint64_t *longs,
    const unsigned long long *nlong, uint64_t max_long, uint64_t max_regions, uint32_t call_rows, const uint32_t *raw,
    NzuDevRes *res) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= *nlong || t >= max_long) return;
    const uint64_t j = longs[t], k = tfx_find_take(tk, n, j);
    if (reg0[j + 1] > max_regions) return;
    const TfxTake E = tk[k];
    const uint64_t i = j - E.ent0;
    const NzuEntry e = load_entry(tab, E, i);
    const uint64_t len = (uint64_t)e.hdr_len + e.size;
    const uint32_t crc = tfr_crc_fold(raw + reg0[j], (uint32_t)(reg0[j + 1] - reg0[j]), tfv_rec_rows(len, call_rows),
                                      nzu_align(e.hdr_len), len, cst[j]);
    if (crc != e.crc) report(res + k, E.first + i);
}

}  // namespace

hipError_t npz_index_launch(const uint8_t *base, uint8_t *table, const s3dg_npz_stream *arch_dev, uint64_t n,
                            s3dg_npz_walk_result *res_dev, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_nzi_walk, dim3((uint32_t)(n < (1u << 20) ? n : (1u << 20))), dim3(64), 0, s, base, table, arch_dev, n, res_dev);
    return hipGetLastError();
}

hipError_t npz_unpack_launch(const uint8_t *src, const uint8_t *tab, uint8_t *dst, uint8_t *ws, const NzuLayout &L,
                             const NzuCounts &C, uint64_t n, size_t scan_tmp_bytes, void *tab_dev, int cus, hipEvent_t *marks,
                             hipStream_t s) {
    const uint32_t *pw = reinterpret_cast<const uint32_t *>(ws);
    const TfxTake *tk = reinterpret_cast<const TfxTake *>(ws + kNzuTakeOff);
    unsigned long long *nlong = reinterpret_cast<unsigned long long *>(ws + L.res);
    NzuDevRes *res = reinterpret_cast<NzuDevRes *>(ws + L.res + kNzuCounterBytes);
    uint64_t *pk = reinterpret_cast<uint64_t *>(ws + L.pk), *sz = reinterpret_cast<uint64_t *>(ws + L.sz);
    uint64_t *reg0 = reinterpret_cast<uint64_t *>(ws + L.reg0);
    uint32_t *cst = reinterpret_cast<uint32_t *>(ws + L.cst);
    uint64_t *longs = reinterpret_cast<uint64_t *>(ws + L.longs);
    uint32_t *raw = reinterpret_cast<uint32_t *>(ws + L.raw);
    auto mark = [&](int m) -> hipError_t { return marks ? hipEventRecord(marks[m], s) : hipSuccess; };
    const dim3 per_entry((uint32_t)((C.ents + 1 + 255) / 256));
    (void)hipGetLastError();
    hipError_t e = mark(0);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nzu_validate, per_entry, dim3(256), 0, s, tab, tk, n, C.ents, res, pk, sz);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tmp = scan_tmp_bytes;
    if ((e = tfrecord_search_scan(ws + L.tmp, &tmp, pk, C.ents, s)) != hipSuccess) return e;
    tmp = scan_tmp_bytes;
    if ((e = tfrecord_search_scan(ws + L.tmp, &tmp, sz, C.ents, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_nzu_consts, per_entry, dim3(256), 0, s, tab, pw, tk, n, C.ents, C.rows, res, (const uint64_t *)pk,
                       (const uint64_t *)sz, reg0, cst, longs, nlong, C.max_long);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = mark(1)) != hipSuccess) return e;
    tmp = scan_tmp_bytes;
    if ((e = tfrecord_search_scan(ws + L.tmp, &tmp, reg0, C.ents, s)) != hipSuccess) return e;
    if ((e = mark(2)) != hipSuccess) return e;
    // 8-wave workgroups of 64 KiB LDS: two per CU, every wave one run of regions
    const uint64_t need = (C.max_regions + 7) / 8, fit = 2ull * (uint64_t)(cus > 0 ? cus : 256);
    hipLaunchKernelGGL(k_nzu_regions, dim3((uint32_t)(need < fit ? need : fit)), dim3(512), 0, s, src, dst, tab, tk, n,
                       (const uint64_t *)reg0, (const uint64_t *)pk, (const uint32_t *)cst, C.ents, C.max_regions, C.rows,
                       (const uint8_t *)tab_dev, raw, res);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (C.max_long) {
        hipLaunchKernelGGL(k_nzu_fold, dim3((uint32_t)((C.max_long + 255) / 256)), dim3(256), 0, s, tab, tk, n,
                           (const uint64_t *)reg0, (const uint32_t *)cst, (const uint64_t *)longs,
                           (const unsigned long long *)nlong, C.max_long, C.max_regions, C.rows, (const uint32_t *)raw, res);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return mark(3);
}

}  // namespace s3dg
