// s3dg_ks_kernels.hip — the keystream family: the K2 / DG1 fill kernels
// (k_keystream, k_keystream_batch, k_zero_prefix), their verify twins and
// their launchers.  The launch plans: s3dg_ks_plan.h, s3dg_dgen_batch_plan.h;
// the callers: s3dg_keystream.cpp, s3dg_dgen_batch.cpp.  The 4 KiB-block
// family: s3dg_block.hip; what the two share: s3dg_dev.h.
#include "s3dg_dev.h"

#include <map>
#include <mutex>

// Diagnostic builds only: S3DG_KS_TRACE = per-wave wall-clock stamps of
// k_keystream; S3DG_KS_JUMP bit 0 = per-lane vector jump even when the wave's
// lanes share a chunk (A/B; outputs identical).
#ifndef S3DG_KS_TRACE
#define S3DG_KS_TRACE 0
#endif
#ifndef S3DG_KS_JUMP
#define S3DG_KS_JUMP 0
#endif

namespace s3dg {
#if S3DG_KS_TRACE
// Diagnostic builds only: per-wave start/end wall-clock stamps of k_keystream
// (tools/ks_trace_lab.py).
__device__ uint64_t *g_ks_trace;
#endif
namespace {

// ---------------------------------------------------------------------------
// K2: keystream fill (generate_npz_bytes_raw x-fill, src/data_formats/npz.rs:376-383).
// Chunk c (chunk_bytes each, last one ragged) of [dst, dst+len) =
//   Xoshiro256PlusPlus::seed_from_u64(seed_base + c).fill_bytes(chunk).
// `lpc` lanes share a chunk: lane `sub` starts at draw sub*span via the
// jump polynomial jtab[sub] = x^(sub*span) mod P (s3dg_jump.cpp), 256 steps.
// Each iteration a lane makes D draws (8D bytes) into its LDS row; the wave
// then writes the 64 rows out with 16-byte pieces, P = D/2 pieces per row and
// 64/P rows per store instruction, so every store covers whole 8D-byte row
// segments (D = 16: 128 B, 8 rows per instruction; D = 64: 512 B, 2 rows).
// W waves per workgroup; LDS = W * 64 * (8D + 16) bytes.
// a ^ b ^ c on 64-bit lanes: two v_bitop3_b32 (gfx950 3-input LUT op, 0x96 =
// XOR3) instead of four v_xor_b32; the compiler does not form it itself.
__device__ __forceinline__ uint64_t xor3_64(uint64_t a, uint64_t b, uint64_t c) {
    const uint32_t lo = __builtin_amdgcn_bitop3_b32((uint32_t)a, (uint32_t)b, (uint32_t)c, 0x96);
    const uint32_t hi = __builtin_amdgcn_bitop3_b32((uint32_t)(a >> 32), (uint32_t)(b >> 32),
                                                    (uint32_t)(c >> 32), 0x96);
    return ((uint64_t)hi << 32) | lo;
}

// a ^ (s & m) with a 32-bit mask m applied to both halves: v_bitop3 0x6C =
// S1 ^ (S0 & S2) (symmetric in S0, S2, so independent of the LUT's bit order).
__device__ __forceinline__ uint64_t and_xor_64(uint64_t s, uint64_t a, uint32_t m) {
    const uint32_t lo = __builtin_amdgcn_bitop3_b32((uint32_t)s, (uint32_t)a, m, 0x6C);
    const uint32_t hi = __builtin_amdgcn_bitop3_b32((uint32_t)(s >> 32), (uint32_t)(a >> 32), m, 0x6C);
    return ((uint64_t)hi << 32) | lo;
}

// Xoshiro256++ output rotl(s0 + s3, 23) + s0.  The empty asm pins the
// rotated value as one 64-bit register pair; without it the compiler turns
// the rotate's OR of two disjoint halves into two adds plus two moves.
__device__ __forceinline__ uint64_t xo_out(uint64_t s0, uint64_t s3) {
    uint64_t r = rotlk<23>(s0 + s3);
    asm("" : "+v"(r));
    return r + s0;
}

// One Xoshiro256 state step (per lane, VALU): the reference order
// s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3; s2 ^= t; s3 = rotl(s3, 45)
// with the chained XORs folded into 3-input ones (11 VALU ops, was 13).
__device__ __forceinline__ void xo_step(uint64_t &s0, uint64_t &s1, uint64_t &s2, uint64_t &s3) {
    const uint64_t t = s1 << 17;
    const uint64_t n1 = xor3_64(s1, s2, s0);
    const uint64_t n0 = xor3_64(s0, s3, s1);
    const uint64_t n2 = xor3_64(s2, s0, t);
    s3 = rotlk<45>(s3 ^ s1);
    s0 = n0; s1 = n1; s2 = n2;
}

// The XCD remap of a launch's workgroup b (s3dg_ks_plan.h).
__device__ __forceinline__ uint64_t ks_remap(const KeystreamArgs &A, uint64_t b) {
    return s3dg::ks_remap(A.xg, A.nwg, b);
}

// A lane's header: where its chunk lies, how long it and its zero prefix are,
// and the chunk's seed input.  The uniform launches derive it from the
// launch's arguments, in ks_unit itself; the batch launches read it from the
// record table (ks_header_batch).  obj / delta serve the batch verify alone.
struct KsHeader {
    uint64_t coff;    // the chunk's byte offset within dst
    uint64_t clen;    // its length; 0: no chunk for this lane
    uint64_t zlen;    // its zero prefix
    uint64_t x;       // seed input of its xoshiro state
    uint32_t obj;     // the object's index
    uint64_t delta;   // (offset within the object) - (offset within dst), mod 2^64
};

// Chunk c of a batch launch: record c of the launch's nrec (s3dg_dgen_batch_plan.h).
// A lane past the table reads nothing and has no chunk.
__device__ __forceinline__ KsHeader ks_header_batch(const DgenChunkRec *recs, uint64_t nrec, uint64_t c) {
    KsHeader H{0, 0, 0, 0, 0, 0};
    if (c < nrec) {
        const uint4 *rp = reinterpret_cast<const uint4 *>(recs + c);
        const uint4 r0 = rp[0], r1 = rp[1];
        H.coff = ((uint64_t)r0.y << 32) | r0.x;
        H.x = ((uint64_t)r0.w << 32) | r0.z;
        H.clen = r1.x;
        H.zlen = r1.y;
        H.obj = r1.z;
        H.delta = (uint64_t)r1.w * kDgenBlock - H.coff;
    }
    return H;
}

// One work unit: wave w of remapped workgroup bid, i.e. lanes
// [(bid*W + w)*64, +64) of the launch.  myrows: this wave's LDS rows.
//
// V (k_verify_keystream): the read-side twin.  The unit derives the same
// seeds, jumps, draws, tail draw and zero prefix into the same LDS rows, and
// where the fill stores a row piece it compares the piece with `dst`'s bytes
// instead; it stores nothing.  A stage's whole pieces (those that end at or
// below their lane region's length) are loaded before the stage's draws, so
// their latency hides behind the PRNG; the ragged piece of a chunk's or an
// object's end is read byte by byte below that length only.  Lane regions of
// a verify launch are whole 4 KiB granules (span % 512 == 0, chunks start on a
// granule of their object), so a row's granule is 4096 / (8 D) consecutive
// stages: `vmask` holds, per row, whether its current granule has shown a
// difference (set from ballots, so it is wave-uniform), and its popcount is
// added to the unit's granule count when the granule closes.  Only a unit that
// found a difference touches rec, from lane 0: two 64-bit adds and a 64-bit
// min (vector atomics); off0 is added to the reported offset.
//
// B (k_keystream_batch, k_verify_keystream_batch): the header comes from the
// record table and, in the verify, differences are also counted per object:
// a wave may hold lanes of several objects, so a lane that found a difference
// adds its bytes and its lowest offset to the record of the object that owns
// the ROW the piece came from (its index and offset shuffled from the row's
// lane), and when a granule closes the lane of every row marked in vmask adds
// one granule to its own object.  All of it sits behind the stage's vote: the
// clean path still has no store and no atomic.  The totals go through
// v_finish as before.
template <int D, int W, int SP, bool V = false, bool B = false>
__device__ __forceinline__ void ks_unit(uint8_t *dst, const KeystreamArgs &A, const uint64_t *jtab,
                                        uint8_t *myrows, uint32_t l, uint64_t bid, uint32_t w,
                                        VerifyRec *rec = nullptr, uint64_t off0 = 0,
                                        const DgenChunkRec *recs = nullptr, uint64_t nrec = 0,
                                        VerifyRec *pobj = nullptr) {
    static_assert(D == 16 || D == 32 || D == 64, "draws per stage");
    constexpr int RS = D * 8 + 16;     // row stride: + 16 B pad, conflict-light ds_write_b128 rows
    constexpr int P = D / 2;           // 16-byte pieces per row
    constexpr int R = 64 / P;          // rows per store instruction
#if S3DG_KS_TRACE
    const uint64_t t_start = wall_clock64();
#endif
    const uint32_t lpc = A.lpc, span = A.span;
    // global lane gl -> chunk gl / lpc, lane-in-chunk gl % lpc (lpc: power of two;
    // lpc > 64 spreads one chunk over lpc/64 waves)
    const uint32_t lsh = (uint32_t)__builtin_ctz(lpc);
    const uint64_t gl = (bid * W + w) * 64 + l;
    const uint64_t c = gl >> lsh;                                    // local chunk index
    const uint32_t sub = (uint32_t)(gl & (lpc - 1));
    KsHeader H{0, 0, 0, 0, 0, 0};
    uint64_t cg = 0, seed_base = 0, coff, clen;
    if constexpr (B) {
        H = ks_header_batch(recs, nrec, c);
        coff = H.coff;
        clen = H.clen;
    } else {
        const uint64_t cpo = A.cpo ? A.cpo : A.nchunks;
        const uint64_t ko = c / cpo;                                     // object within the launch
        const uint64_t cl = c - ko * cpo;
        cg = A.chunk0 + cl;                                              // chunk index in the object
        coff = A.doff + ko * A.obj_stride + cl * A.chunk_bytes;          // offset within dst
        seed_base = A.seed_base + ko * A.seed_step;
        const uint64_t gofs = cg * A.chunk_bytes;                        // offset within the object
        clen = (c < A.nchunks && gofs < A.obj_len)
                   ? ((A.obj_len - gofs) < A.chunk_bytes ? (A.obj_len - gofs) : A.chunk_bytes)
                   : 0;
    }
    const uint64_t d0 = A.z0 + (uint64_t)sub * span;                 // first draw index
    const KsRegion reg = ks_lane_region(clen, A.z0, span, sub);      // lane region within chunk
    const uint64_t rb = reg.rb;
    const uint32_t rlen = reg.rlen;
    const uint64_t tail_draw = clen >> 3;                            // draw index of a 1..7 B tail
    const bool tail_hi = (clen & 7) >= 1 && (clen & 7) <= 4;         // next_u32 = next_u64 >> 32
    // zero prefix of the chunk (dgen-contract compressibility); 0 for the npz fill
    uint64_t zlen, x;
    if constexpr (B) {
        zlen = H.zlen;
        x = H.x;
    } else {
        zlen = A.zf_num ? (clen * A.zf_num) / A.zf_den : 0;
        // chunk seed: npz.rs:381 seed_from_u64(k), or the dgen mode
        // seed ^ (u * phi) with u = chunk % U (dedup)
        if (A.seed_mode == 0) {
            x = seed_base + cg;
        } else {
            const uint32_t u = A.unique == 0xFFFFFFFFu ? (uint32_t)cg : fastmod((uint32_t)cg, A.m_unique, A.unique);
            x = seed_base ^ ((uint64_t)u * 0x9E3779B97F4A7C15ull);
        }
    }
    uint64_t s0 = mix64(x + 0x9E3779B97F4A7C15ull), s1 = mix64(x + 2 * 0x9E3779B97F4A7C15ull);
    uint64_t s2 = mix64(x + 3 * 0x9E3779B97F4A7C15ull), s3 = mix64(x + 4 * 0x9E3779B97F4A7C15ull);
    const uint32_t iters = span / D;
    const uint32_t piece = l % P;
    // destination of the P rows this lane helps write: row R*i + l/P, piece l%P
    uint64_t raddr[P];
    uint32_t rrem[P];
    auto row_dest = [&]() {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const uint32_t r = R * i + l / P;
            raddr[i] = __shfl(coff + rb, (int)r);
            rrem[i] = __shfl(rlen, (int)r);
        }
    };
    const bool full_rows = __all(rlen == span * 8u);

    // V: the stage's pieces of src (then src ^ expected), this lane's count
    // and lowest offset, the rows' granule state and the unit's granule count
    typedef u32x4 VStage[V ? P : 1];
    VStage g;
    uint64_t vcnt = 0, vfirst = ~0ull, vmask = 0;
    uint32_t vblocks = 0;
    auto v_load = [&](VStage &g, uint32_t it) {
        const uint32_t o = it * (D * 8) + piece * 16;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            g[i] = u32x4{0u, 0u, 0u, 0u};
            // nontemporal, as k_verify_stream: the bytes are read once
            if (full_rows || o + 16 <= rrem[i])
                g[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(dst + raddr[i] + o));
        }
    };
    // expected pieces: zeros (an all-zero wave) or the LDS rows
    auto v_compare = [&](VStage &g, uint32_t it, bool zeros) {
        const uint32_t o = it * (D * 8) + piece * 16;
        uint32_t dm = 0;                                  // bit i: this lane's piece of row group i differs
#pragma unroll
        for (int i = 0; i < P; ++i) {
            u32x4 e = {0u, 0u, 0u, 0u};
            if (!zeros) e = *reinterpret_cast<const u32x4 *>(myrows + (R * i + l / P) * RS + piece * 16);
            if (full_rows || o + 16 <= rrem[i]) {
                g[i] ^= e;
            } else if (o < rrem[i]) {                     // ragged end: the nb < 16 bytes below the region's length
                const uint32_t nb = rrem[i] - o;
                const uint8_t *p = dst + raddr[i] + o;
                uint64_t lo = 0, hi = 0;
                for (uint32_t b = 0; b < nb; ++b) {
                    const uint64_t v = p[b];
                    if (b < 8) lo |= v << (8 * b);
                    else hi |= v << (8 * (b - 8));
                }
                const uint64_t mlo = nb >= 8 ? ~0ull : ~(~0ull << (8 * nb));
                const uint64_t mhi = nb <= 8 ? 0ull : ~(~0ull << (8 * (nb - 8)));
                lo = (lo ^ (((uint64_t)e.y << 32) | e.x)) & mlo;
                hi = (hi ^ (((uint64_t)e.w << 32) | e.z)) & mhi;
                g[i] = u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
            }
            if (g[i].x | g[i].y | g[i].z | g[i].w) dm |= 1u << i;
        }
        if (__any(dm != 0)) {                             // the clean path ends here: one vote per stage
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const bool d = (dm >> i) & 1u;
                const uint64_t bal = __ballot(d);         // lanes [j P, (j+1) P): row R i + j
                if (bal == 0) continue;
#pragma unroll
                for (int j = 0; j < R; ++j)
                    if ((bal >> (j * P)) & (~0ull >> (64 - P))) vmask |= 1ull << (R * i + j);
                uint32_t robj = 0;                        // B: the row's object and offset within it
                uint64_t rdelta = 0;
                if constexpr (B) {
                    robj = __shfl(H.obj, (int)(R * i + l / P));
                    rdelta = __shfl(H.delta, (int)(R * i + l / P));
                }
                if (d) {
                    uint32_t c = 0, f = 16;
                    diff_piece(g[i], 0, c, f);
                    vcnt += c;
                    const uint64_t pos = off0 + raddr[i] + o + f;
                    vfirst = pos < vfirst ? pos : vfirst;
                    if constexpr (B) {
                        if (pobj) {
                            atomicAdd(reinterpret_cast<unsigned long long *>(&pobj[robj].bytes), (unsigned long long)c);
                            atomicMin(reinterpret_cast<unsigned long long *>(&pobj[robj].first),
                                      (unsigned long long)(raddr[i] + rdelta + o + f));
                        }
                    }
                }
            }
        }
        constexpr uint32_t GS = kBlk / (D * 8);           // stages per 4 KiB granule of a row
        if ((it + 1) % GS == 0 || it + 1 == iters) {
            if constexpr (B) {
                if (pobj && ((vmask >> l) & 1ull))
                    atomicAdd(reinterpret_cast<unsigned long long *>(&pobj[H.obj].blocks), 1ull);
            }
            vblocks += (uint32_t)__builtin_popcountll(vmask);
            vmask = 0;
        }
    };
    auto v_finish = [&]() {
        if (!__any(vcnt != 0)) return;                    // clean: no store, no atomic
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            vcnt += __shfl_xor(vcnt, d, 64);
            const uint64_t f = __shfl_xor(vfirst, d, 64);
            vfirst = f < vfirst ? f : vfirst;
        }
        if (l == 0) {
            atomicAdd(reinterpret_cast<unsigned long long *>(&rec->bytes), (unsigned long long)vcnt);
            atomicAdd(reinterpret_cast<unsigned long long *>(&rec->blocks), (unsigned long long)vblocks);
            atomicMin(reinterpret_cast<unsigned long long *>(&rec->first), (unsigned long long)vfirst);
        }
    };

    // A wave whose regions all lie inside their chunks' zero prefixes (DG1,
    // compress > 1) stores zeros: no jump, no PRNG.
    if (__all(rlen == 0 || rb + rlen <= zlen)) {
        row_dest();
        if constexpr (V) {
            // compares against zeros, one stage of loads in flight: a second
            // stage's 128 registers do not fit beside the row addresses (the
            // compiler spills ~200 VGPRs to scratch)
            for (uint32_t it = 0; it < iters; ++it) {
                v_load(g, it);
                v_compare(g, it, true);
            }
            v_finish();
            return;
        }
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (uint32_t it = 0; it < iters; ++it) {
            const uint32_t o = it * (D * 8) + piece * 16;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                if (full_rows) {
                    store16<SP>(dst + raddr[i] + o, z);
                } else if (o < rrem[i]) {
                    uint8_t *q = dst + raddr[i] + o;
                    if (o + 16 <= rrem[i]) store16<SP>(q, z);
                    else for (uint32_t b = 0; o + b < rrem[i]; ++b) q[b] = 0;
                }
            }
        }
        return;
    }

#if !(S3DG_ABLATE & 64)
    if (lpc >= 64 && !(S3DG_KS_JUMP & 1)) {
        // Every lane of the wave is in one chunk, so the sequence step^i(s)
        // is wave-uniform: it runs on the scalar unit (64-bit s_xor/s_lshl,
        // SGPRs) and each lane only accumulates the states its own jump
        // polynomial selects (8 v_bitop3 with an SGPR operand per step, was
        // 8 + the 11-op vector step).  Lane sub = 0 of a launch with z0 = 0
        // has J = 1: a = s.
        uint64_t u0 = readlane64(s0, 0), u1 = readlane64(s1, 0);
        uint64_t u2 = readlane64(s2, 0), u3 = readlane64(s3, 0);
        // the lane's 256-bit polynomial in two loads up front (one load and
        // wait per 32 steps before)
        const uint4 *Jv = reinterpret_cast<const uint4 *>(jtab + 4 * sub);
        const uint4 j0 = Jv[0], j1 = Jv[1];
        const uint32_t J[8] = {j0.x, j0.y, j0.z, j0.w, j1.x, j1.y, j1.z, j1.w};
        uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const uint32_t jw = J[h];
#pragma unroll 8
            for (int b = 0; b < 32; ++b) {
                const uint32_t m = (uint32_t)((int32_t)(jw << (31 - b)) >> 31);
                a0 = and_xor_64(u0, a0, m); a1 = and_xor_64(u1, a1, m);
                a2 = and_xor_64(u2, a2, m); a3 = and_xor_64(u3, a3, m);
                const uint64_t t = u1 << 17;    // reference step order, scalar
                u2 ^= u0; u3 ^= u1; u1 ^= u2; u0 ^= u3; u2 ^= t;
                u3 = rotl64(u3, 45);
            }
        }
        s0 = a0; s1 = a1; s2 = a2; s3 = a3;
    } else if (A.z0 || (lpc > 1 && sub > 0)) {   // jump to draw z0 + sub*span
        // state <- sum over set bits i of J of step^i(state): 256 steps, the
        // polynomial read as 8 32-bit halves so each step's mask is one
        // sign-extended bit field and each accumulate one v_bitop3
        const uint32_t *J = reinterpret_cast<const uint32_t *>(jtab + 4 * sub);
        uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int h = 0; h < 8; ++h) {
            const uint32_t jw = J[h];
#pragma unroll 4
            for (int b = 0; b < 32; ++b) {
                const uint32_t m = (uint32_t)((int32_t)(jw << (31 - b)) >> 31);
                a0 = and_xor_64(s0, a0, m); a1 = and_xor_64(s1, a1, m);
                a2 = and_xor_64(s2, a2, m); a3 = and_xor_64(s3, a3, m);
                xo_step(s0, s1, s2, s3);
            }
        }
        s0 = a0; s1 = a1; s2 = a2; s3 = a3;
    }
#endif
    row_dest();

    // Wave-uniform fast path: a D-draw group is generated unmasked unless a
    // lane of the wave is at its chunk's 1-4 byte tail (iteration it_tail);
    // bytes inside a zero prefix are then zeroed in the lane's LDS row by the
    // lanes concerned alone (round 5: the whole wave used to take the masked
    // path while any lane touched the prefix, e.g. 6 of 8 store rounds of a
    // DG1 c3 wave, or 8 of 11 of a tail launch's waves, profiles/r05/).  The
    // stores need no guards when every region of the wave is full length.
    const uint32_t it_tail = (tail_hi && tail_draw >= d0 && tail_draw < d0 + span)
                                 ? (uint32_t)((tail_draw - d0) / D) : 0xFFFFFFFFu;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint64_t dg = d0 + (uint64_t)it * D;
        const bool plain = __all(it != it_tail);
        if constexpr (V) v_load(g, it);   // in flight during the draws
        if (plain) {
#pragma unroll
            for (int q = 0; q < D; q += 2) {
#if S3DG_ABLATE & 32
                const uint64_t ra = s0 + q, rbv = s3 + q;
#else
                const uint64_t ra = xo_out(s0, s3); xo_step(s0, s1, s2, s3);
                const uint64_t rbv = xo_out(s0, s3); xo_step(s0, s1, s2, s3);
#endif
                *reinterpret_cast<u32x4 *>(myrows + l * RS + q * 8) =
                    u32x4{(uint32_t)ra, (uint32_t)(ra >> 32), (uint32_t)rbv, (uint32_t)(rbv >> 32)};
            }
        } else {
#pragma unroll
            for (int q = 0; q < D; q += 2) {
                uint64_t ra = xo_out(s0, s3); xo_step(s0, s1, s2, s3);
                uint64_t rbv = xo_out(s0, s3); xo_step(s0, s1, s2, s3);
                const uint64_t d = dg + q;
                if (tail_hi && d == tail_draw) ra >>= 32;
                if (tail_hi && d + 1 == tail_draw) rbv >>= 32;
                if (8 * d < zlen) ra &= (8 * d + 8 <= zlen) ? 0ull : (~0ull << (8 * (zlen - 8 * d)));
                if (8 * d + 8 < zlen) rbv &= (8 * d + 16 <= zlen) ? 0ull : (~0ull << (8 * (zlen - 8 * d - 8)));
                *reinterpret_cast<u32x4 *>(myrows + l * RS + q * 8) =
                    u32x4{(uint32_t)ra, (uint32_t)(ra >> 32), (uint32_t)rbv, (uint32_t)(rbv >> 32)};
            }
        }
        // zero-prefix bytes of this row (fast path only: the masked path zeroed them)
        const uint64_t row0 = 8 * dg;
        if (plain && row0 < zlen) {
            const uint32_t zb = (zlen - row0) < (uint64_t)(D * 8) ? (uint32_t)(zlen - row0) : (uint32_t)(D * 8);
            uint8_t *row = myrows + l * RS;
            for (uint32_t p = 0; p + 16 <= zb; p += 16) *reinterpret_cast<u32x4 *>(row + p) = u32x4{0u, 0u, 0u, 0u};
            if (zb & 15u) {
                u32x4 *pc = reinterpret_cast<u32x4 *>(row + (zb & ~15u));
                u32x4 v = *pc;
                const uint32_t nz = zb & 15u;   // leading bytes to zero
                v.x = nz >= 4 ? 0u : v.x & (~0u << (8 * nz));
                v.y = nz >= 8 ? 0u : nz <= 4 ? v.y : v.y & (~0u << (8 * (nz - 4)));
                v.z = nz >= 12 ? 0u : nz <= 8 ? v.z : v.z & (~0u << (8 * (nz - 8)));
                v.w = nz <= 12 ? v.w : v.w & (~0u << (8 * (nz - 12)));
                *pc = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t o = it * (D * 8) + piece * 16;               // offset within the row's region
        if constexpr (V) {
            v_compare(g, it, false);
        } else if (full_rows) {
            // Pieces are read from LDS a group of 8 ahead of their stores, so
            // each read's latency hides behind the previous group's stores
            // (the compiler otherwise pairs each read with its store and waits
            // P times per stage): +2 % (variant_ksgroup.log).
            constexpr int G = P < 8 ? P : 8;
            u32x4 v[P];
#pragma unroll
            for (int i = 0; i < G; ++i)
                v[i] = *reinterpret_cast<const u32x4 *>(myrows + (R * i + l / P) * RS + piece * 16);
#pragma unroll
            for (int g = 0; g < P; g += G) {
                if (g + G < P) {
#pragma unroll
                    for (int i = g + G; i < g + 2 * G; ++i)
                        v[i] = *reinterpret_cast<const u32x4 *>(myrows + (R * i + l / P) * RS + piece * 16);
                }
                asm volatile("" ::: "memory");
#pragma unroll
                for (int i = g; i < g + G; ++i) store16<SP>(dst + raddr[i] + o, v[i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const uint32_t r = R * i + l / P;
                if (o >= rrem[i]) continue;
                const u32x4 v = *reinterpret_cast<const u32x4 *>(myrows + r * RS + piece * 16);
                uint8_t *p = dst + raddr[i] + o;
                if (o + 16 <= rrem[i]) {
                    store16<SP>(p, v);
                } else {
                    const uint32_t dw[4] = {v.x, v.y, v.z, v.w};
                    for (uint32_t b = 0; b < 16 && o + b < rrem[i]; ++b) p[b] = (uint8_t)(dw[b >> 2] >> (8 * (b & 3)));
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if constexpr (V) v_finish();
#if S3DG_KS_TRACE
    if (l == 0 && g_ks_trace) {
        // bits 48-63: HW_ID's wave/SIMD/pipe/CU/SH/SE fields (start stamp),
        // XCC_ID (end stamp); the 100 MHz clock below (tools/ks_xcd_lab.py)
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        const uint64_t wi = bid * W + w, m48 = (1ull << 48) - 1;
        g_ks_trace[2 * wi] = (t_start & m48) | ((uint64_t)(hw & 0xFFFFu) << 48);
        g_ks_trace[2 * wi + 1] = (wall_clock64() & m48) | ((uint64_t)(xcc & 0xFu) << 48);
    }
#endif
}

// Persistent launches: the next work unit for a wave on XCD x.  Queue v holds
// the wave units of the static grid's workgroups b = v (mod 8) in order
// (q -> workgroup 8*(q/W) + v, wave q%W): the units XCD v would have been dealt.
// A wave drains its own XCD's queue, then takes from the others', so an XCD
// that runs ahead takes over the work of a slower one instead of idling at the
// end of the launch.  One device-scope fetch-add (lane 0, vector memory) per
// attempt; `gone` marks the queues found empty (wave-uniform).
template <int W>
__device__ __forceinline__ bool ks_take(const KeystreamArgs &A, const KeystreamArgs &A2, uint64_t *ctr, uint32_t x,
                                        uint32_t l, uint32_t &gone, uint64_t &b, uint32_t &w, bool &second) {
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t v = (x + i) & 7;
        if (gone & (1u << v)) continue;
        const uint64_t quota = ks_queue_quota(A.nwg, v, W);
        const uint64_t quota2 = ks_queue_quota(A2.nwg, v, W);   // A2.nwg = 0: no second set
        uint64_t q = 0;
        if (l == 0) q = __hip_atomic_fetch_add(ctr + 16 * v, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        q = readlane64(q, 0);
        if (q < quota) {
            b = ks_queue_wg(q, v, W);
            w = ks_queue_wave(q, W);
            second = false;
            return true;
        }
        if (q - quota < quota2) {
            q -= quota;
            b = ks_queue_wg(q, v, W);
            w = ks_queue_wave(q, W);
            second = true;
            return true;
        }
        gone |= 1u << v;
    }
    return false;
}

// Keystream launch.  Static grid (A.ctr null): workgroup blockIdx.x does its
// own W units.  Persistent (A.ctr set, launches of more than one round of
// resident waves): gridDim.x workgroups stay resident and every wave takes
// units from the per-XCD queues until all are empty; counter set A.par of
// A.ctr serves this launch, and workgroup 0 zeroes the other set for the next
// launch on the stream (launches on one stream never overlap).  Each queue
// holds its XCD's units of A, then its units of A2 (A2.nwg > 0: the launch's
// last chunks with shorter lanes, so the launch drains on shorter units).
template <int D, int W, int SP>
__global__ __launch_bounds__(64 * W) void k_keystream(uint8_t *dst, KeystreamArgs A, const uint64_t *jtab,
                                                      KeystreamArgs A2, const uint64_t *jtab2) {
    constexpr int RS = D * 8 + 16;
    __shared__ __attribute__((aligned(16))) uint8_t rows[W][64 * RS];
    const uint32_t t = threadIdx.x, l = t & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(t >> 6);
    uint8_t *myrows = rows[w];
    if (!A.ctr) {
        ks_unit<D, W, SP>(dst, A, jtab, myrows, l, ks_remap(A, blockIdx.x), w);
        return;
    }
    uint64_t *const cur = A.ctr + (A.par ? 128 : 0);   // 8 counters, 128 B apart
    if (blockIdx.x == 0 && t < 8)
        __hip_atomic_store(A.ctr + (A.par ? 0 : 128) + 16 * t, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t x = blockIdx.x & 7;
    uint32_t gone = 0, ww = 0;
    uint64_t b = 0;
    bool second = false;
    while (ks_take<W>(A, A2, cur, x, l, gone, b, ww, second)) {
        if (second) ks_unit<D, W, SP>(dst, A2, jtab2, myrows, l, ks_remap(A2, b), ww);
        else ks_unit<D, W, SP>(dst, A, jtab, myrows, l, ks_remap(A, b), ww);
    }
}

// Verify, the read-side twin of k_keystream: ks_unit's compare variant over a
// static grid of 1-wave workgroups (workgroup b = lanes [64 b, 64 b + 64) of
// the launch, dealing order), 64-draw stages.  A (z0 = 0, lane regions of
// whole granules: ks_verify_plan) covers zero prefixes and tails in one launch.
// No global store; rec is touched only by units that found a difference.
template <int D>
__global__ __launch_bounds__(64) void k_verify_keystream(const uint8_t *src, KeystreamArgs A, const uint64_t *jtab,
                                                         uint64_t off0, VerifyRec *rec) {
    constexpr int RS = D * 8 + 16;
    __shared__ __attribute__((aligned(16))) uint8_t rows[64 * RS];
    ks_unit<D, 1, kStorePlain, true>(const_cast<uint8_t *>(src), A, jtab, rows, threadIdx.x & 63, blockIdx.x, 0, rec,
                                     off0);
}

// A mixed-size DG1 batch (s3dg_dgen_fill_batch): k_keystream's
// static grid with the lanes' headers read from a record table, one record per
// chunk of the launch's size class (A: lpc, span, xg, nwg; z0 = 0).  Zero
// prefixes are written inside the lanes.
template <int D, int W, int SP>
__global__ __launch_bounds__(64 * W) void k_keystream_batch(uint8_t *dst, KeystreamArgs A, const uint64_t *jtab,
                                                            const DgenChunkRec *recs, uint64_t nrec) {
    constexpr int RS = D * 8 + 16;
    __shared__ __attribute__((aligned(16))) uint8_t rows[W][64 * RS];
    const uint32_t t = threadIdx.x, l = t & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(t >> 6);
    ks_unit<D, W, SP, false, true>(dst, A, jtab, rows[w], l, ks_remap(A, blockIdx.x), w, nullptr, 0, recs, nrec);
}

// Its read-side twin (s3dg_verify_dgen_batch): k_verify_keystream over the
// record table.  tot takes the launch's totals (offsets from src), pobj (or
// null) the per-object records (offsets from each object's first byte).
template <int D>
__global__ __launch_bounds__(64) void k_verify_keystream_batch(const uint8_t *src, KeystreamArgs A,
                                                               const uint64_t *jtab, const DgenChunkRec *recs,
                                                               uint64_t nrec, VerifyRec *tot, VerifyRec *pobj) {
    constexpr int RS = D * 8 + 16;
    __shared__ __attribute__((aligned(16))) uint8_t rows[64 * RS];
    ks_unit<D, 1, kStorePlain, true, true>(const_cast<uint8_t *>(src), A, jtab, rows, threadIdx.x & 63, blockIdx.x, 0,
                                           tot, 0, recs, nrec, pobj);
}

// DG1 zero prefixes in the fill's store shape (paired with a keystream launch
// over the chunks' tails, s3dg_internal_dgen_chunk): one 64-thread workgroup
// per 4 KiB granule, four 16-byte zero stores per lane (1 KiB per
// instruction).  2D grid: x = granule of the chunk, padded to zgp (a multiple
// of 8), y = chunk, so the linear workgroup id y*zgp + x, dealt round-robin
// to the XCDs, lands on XCD x mod 8 and writes granule x of its chunk, = x
// (mod 8) in the buffer: every XCD on every 8th granule, as the fill
// (DESIGN.md §5.1).  The dgen keystream's own all-zero waves write 64 lane
// regions per wave instead (§5.2).  Chunk y -> object y / cpo by Lemire's
// fastdiv (m_cpo = floor(2^64 / cpo) + 1; y, cpo < 2^32).  That constant wraps
// to 0 for cpo == 1 (one chunk per object, e.g. a ragged [0,1) block range), so
// that case takes ko = y directly (a uniform branch).
template <int SP, int NW>
__global__ __launch_bounds__(64 * NW) void k_zero_prefix(uint8_t *dst, uint64_t y0, uint64_t cpo, uint64_t m_cpo,
                                                         uint64_t obj_stride, uint64_t chunk_bytes, uint32_t zw) {
    const uint32_t x = blockIdx.x;
    if ((uint64_t)x * kBlk >= zw) return;
    const uint32_t lim = zw - x * kBlk;   // bytes of this granule below zw (a multiple of 16)
    const uint64_t y = y0 + blockIdx.y;
    const uint64_t ko = cpo == 1 ? y : __umul64hi(m_cpo, y);
    const uint64_t cl = y - ko * cpo;
    uint64_t off = ko * obj_stride + cl * chunk_bytes + (uint64_t)x * kBlk;
    asm volatile("" : "+v"(off));   // the address on the VALU
    uint8_t *p = dst + off + threadIdx.x * 16;
    const u32x4 z = {0u, 0u, 0u, 0u};
    if (lim >= kBlk) {
#pragma unroll
        for (int k = 0; k < 4 / NW; ++k) store16<SP>(p + k * 1024 * NW, z);
    } else {   // the partial last granule
#pragma unroll
        for (int k = 0; k < 4 / NW; ++k)
            if (threadIdx.x * 16 + k * 1024 * NW < lim) store16<SP>(p + k * 1024 * NW, z);
    }
}

// static LDS of k_keystream<D, W>
constexpr uint32_t ks_static_lds(int D, int W) { return (uint32_t)W * 64u * (uint32_t)(D * 8 + 16); }

// One k_keystream launch of wgs workgroups in shape sh.
hipError_t launch_ks(uint8_t *dst, const KeystreamArgs &A, const uint64_t *jtab, const KsShape &sh, uint32_t lds,
                     hipStream_t s, uint64_t wgs, const KeystreamArgs &A2, const uint64_t *jtab2) {
    if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dispatch_ks_shape(sh, [&](auto D, auto W) {
        dispatch_store(sh.store, [&](auto SP) {
            constexpr int d = decltype(D)::value, w = decltype(W)::value, sp = decltype(SP)::value;
            hipLaunchKernelGGL((k_keystream<d, w, sp>), dim3((uint32_t)wgs), dim3(64 * w), lds, s, dst, A, jtab, A2,
                               jtab2);
        });
    });
    return hipGetLastError();
}

// Resident workgroups per CU of a keystream shape with lds bytes of dynamic
// LDS, asked of the kStorePlain instantiation.
hipError_t ks_occupancy(const KsShape &sh, uint32_t lds, int *out) {
    return dispatch_ks_shape(sh, [&](auto D, auto W) {
        constexpr int d = decltype(D)::value, w = decltype(W)::value;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(
            out, reinterpret_cast<const void *>(&k_keystream<d, w, kStorePlain>), 64 * w, lds);
    });
}

}  // namespace

// Persistent keystream launches from this many rounds of resident waves up.
// Whole libraries in one process, interleaved: persistent
// for any launch of more than one round against the static grid
// (profiles/r04/k/pass1/lib_ab.log): one 80 GiB DG1 launch 6715 -> 7011 GB/s,
// K2 84 GB in one launch 6763 -> 7087, ten 8 GiB DG1 launches (8 rounds each)
// 6248 -> 6441, but K2 8 GiB launches (4 rounds of 4096-draw lanes)
// 6417 -> 6388 and DG1 with a zero prefix (4-wave workgroups, short
// all-zero units) 6204 -> 6018.  From 6 rounds, 1-wave workgroups only
// (profiles/r04/k/lib_ab.log): the three gains kept (6421 / 6987 / 7052
// against 6232 / 6646 / 6705), 4-round launches unchanged (persistent from
// one round: DG1 4 GiB launches 6175 -> 6151, K2 8 GiB 6400 -> 6376).
// (kKsPersistRounds / S3DG_KS_PERSIST_ROUNDS: s3dg_ks_plan.h, ks_persistent_grid)

// Resident workgroups per CU of a keystream shape (cached: the occupancy
// query is a host-side calculation, but a host call's latency budget is µs).
static int ks_resident_per_cu(const KsShape &sh, uint32_t lds) {
    static std::mutex mu;
    static std::map<uint64_t, int> cache;
    const uint64_t key = ((uint64_t)sh.draws << 48) | ((uint64_t)sh.waves << 40) | lds;
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int n = 0;
    if (ks_occupancy(sh, lds, &n) != hipSuccess) n = 0;
    (void)hipGetLastError();
    cache[key] = n;
    return n;
}

hipError_t launch_keystream(uint8_t *dst, const KeystreamArgs &A0, const uint64_t *jtab,
                           const KsShape &sh, hipStream_t s, KsCounters *ctrs, int cus, int persist_rounds,
                           const KeystreamArgs *tail, const uint64_t *tail_jtab) {
    (void)hipGetLastError();
    const uint32_t lds = occupancy_lds(sh.wgs_per_cu, ks_static_lds(sh.draws, sh.waves));
    // static-grid workgroups of an argument set
    auto grid_of = [&](KeystreamArgs &X) -> uint64_t {
        const KsGrid G = ks_static_grid(X.nchunks, X.lpc, sh.waves, sh.xcd_waves);
        X.xg = G.xg;
        X.nwg = G.nwg;
        X.ctr = nullptr;
        X.par = 0;
        return G.wgs;
    };
    KeystreamArgs A = A0, A2{};
    const uint64_t wgs = grid_of(A);
    uint64_t wgs2 = 0;
    if (tail) {
        A2 = *tail;
        wgs2 = grid_of(A2);
    }
    if (wgs > 0x7FFFFFFFull || wgs2 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    uint64_t grid = wgs;
    bool persistent = false;
#if !S3DG_DIAG_KS_STATIC
    // at least `rounds` rounds of resident waves (default: 1-wave workgroups
    // from kKsPersistRounds): a persistent grid over per-XCD queues
    // (k_keystream), one resident round of workgroups, a multiple of 8
    const bool may = persist_rounds < 0 ? sh.waves == 1 && kKsPersistRounds > 0 : persist_rounds > 0;
    if (may && ctrs && ctrs->dev && cus > 0) {
        const uint64_t cap = ks_persistent_grid(wgs, wgs2, persist_rounds, (uint64_t)ks_resident_per_cu(sh, lds),
                                                (uint64_t)cus, sh.waves);
        if (cap) {
            A.ctr = ctrs->dev;
            A.par = ctrs->par;
            grid = cap;
            persistent = true;
        }
    }
#endif
    if (persistent) {   // both sets in one launch, A's units first
        const hipError_t e = launch_ks(dst, A, jtab, sh, lds, s, grid, A2, tail_jtab);
        if (e == hipSuccess) ctrs->par ^= 1u;
        return e;
    }
    KeystreamArgs none{};   // static grid: A2 unused (nwg 0); the tail set as a launch of its own
    hipError_t e = launch_ks(dst, A, jtab, sh, lds, s, grid, none, nullptr);
    if (e == hipSuccess && tail) e = launch_ks(dst, A2, tail_jtab, sh, lds, s, wgs2, none, nullptr);
    return e;
}

hipError_t keystream_occupancy(const KsShape &sh, int *wgs_per_cu) {
    return ks_occupancy(sh, occupancy_lds(sh.wgs_per_cu, ks_static_lds(sh.draws, sh.waves)), wgs_per_cu);
}

hipError_t launch_verify_keystream(const uint8_t *src, const KeystreamArgs &A0, const uint64_t *jtab, uint64_t off0,
                                   VerifyRec *rec, hipStream_t s) {
    (void)hipGetLastError();
    // z0 = 0, 64-draw stages, lane regions of whole granules
    if (A0.z0 || A0.doff || A0.span == 0 || A0.span % (kBlk / 8) || (A0.chunk_bytes & (kBlk - 1)) ||
        (A0.lpc & (A0.lpc - 1)) || A0.lpc == 0)
        return hipErrorInvalidValue;
    KeystreamArgs A = A0;
    const uint64_t waves = (A.nchunks * A.lpc + 63) / 64;
    if (waves == 0) return hipSuccess;
    if (waves * 64 > 0xFFFFFFFFull) return hipErrorInvalidValue;   // 32-bit work-item counts (kMaxGridX)
    A.xg = 1;
    A.nwg = (uint32_t)waves;
    A.ctr = nullptr;
    A.par = 0;
    hipLaunchKernelGGL((k_verify_keystream<64>), dim3((uint32_t)waves), dim3(64), 0, s, src, A, jtab, off0, rec);
    return hipGetLastError();
}

// The lanes of a batch launch: nrec chunks x lpc lanes of `span` draws, as a
// static grid of `waves`-wave workgroups.  false: beyond the grid's reach.
static bool ksb_args(KeystreamArgs &A, uint32_t lpc, uint64_t span, uint64_t nrec, int waves, uint32_t xg,
                     uint64_t *wgs) {
    if (lpc == 0 || (lpc & (lpc - 1)) || span == 0 || span > 0xFFFFFFFFull || nrec > kDgbMaxLanes / lpc) return false;
    A = KeystreamArgs{};
    A.lpc = lpc;
    A.span = (uint32_t)span;
    A.nchunks = nrec;
    const uint64_t wv = (nrec * lpc + 63) / 64;
    *wgs = (wv + (uint64_t)waves - 1) / (uint64_t)waves;
    A.xg = xg;
    A.nwg = (uint32_t)*wgs;
    return true;
}

hipError_t launch_keystream_batch(uint8_t *dst, const DgenChunkRec *recs, uint64_t nrec, uint32_t lpc, uint64_t span,
                                  const uint64_t *jtab, const KsShape &sh, hipStream_t s) {
    (void)hipGetLastError();
    if (nrec == 0) return hipSuccess;
    KeystreamArgs A;
    uint64_t wgs = 0;
    const uint32_t xg = sh.xcd_waves > sh.waves ? (uint32_t)(sh.xcd_waves / sh.waves) : 1u;
    if (span % (uint64_t)sh.draws || !ksb_args(A, lpc, span, nrec, sh.waves, xg, &wgs)) return hipErrorInvalidValue;
    const uint32_t lds = occupancy_lds(sh.wgs_per_cu, ks_static_lds(sh.draws, sh.waves));
    dispatch_ks_shape(sh, [&](auto D, auto W) {
        dispatch_store(sh.store, [&](auto SP) {
            constexpr int d = decltype(D)::value, w = decltype(W)::value, sp = decltype(SP)::value;
            hipLaunchKernelGGL((k_keystream_batch<d, w, sp>), dim3((uint32_t)wgs), dim3(64 * w), lds, s, dst, A, jtab,
                               recs, nrec);
        });
    });
    return hipGetLastError();
}

hipError_t launch_verify_keystream_batch(const uint8_t *src, const DgenChunkRec *recs, uint64_t nrec, uint32_t lpc,
                                         uint64_t span, const uint64_t *jtab, VerifyRec *tot, VerifyRec *pobj,
                                         hipStream_t s) {
    (void)hipGetLastError();
    if (nrec == 0) return hipSuccess;
    KeystreamArgs A;
    uint64_t wgs = 0;
    // lane regions of whole granules, 64-draw stages, 1-wave workgroups in dealing order
    if (span % (kBlk / 8) || !ksb_args(A, lpc, span, nrec, 1, 1, &wgs)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_verify_keystream_batch<64>), dim3((uint32_t)wgs), dim3(64), 0, s, src, A, jtab, recs, nrec,
                       tot, pobj);
    return hipGetLastError();
}

hipError_t launch_zero_prefix(uint8_t *dst, uint64_t nchunks, uint64_t cpo, uint64_t obj_stride, uint64_t chunk_bytes,
                              uint32_t zw, const LaunchCfg &lc, hipStream_t s) {
    (void)hipGetLastError();
    if (zw == 0 || nchunks == 0) return hipSuccess;
    if (cpo == 0 || cpo > 0xFFFFFFFFull || nchunks > 0xFFFFFFFFull || (chunk_bytes & 4095u) || (zw & 15u) ||
        zw > chunk_bytes)
        return hipErrorInvalidValue;
    const uint32_t zgp = ((zw + kBlk - 1) / kBlk + 7u) & ~7u;
    const uint64_t m_cpo = ~0ull / cpo + 1;
    for (uint64_t y0 = 0; y0 < nchunks; y0 += 65535) {
        const dim3 g(zgp, (uint32_t)((nchunks - y0) < 65535 ? (nchunks - y0) : 65535));
        dispatch_cfg(lc, [&](auto SP, auto NW) {
            constexpr int sp = decltype(SP)::value, nw = decltype(NW)::value;
            hipLaunchKernelGGL((k_zero_prefix<sp, nw>), g, dim3(64 * nw), lc.dyn_lds, s, dst, y0, cpo, m_cpo,
                               obj_stride, chunk_bytes, zw);
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace s3dg

#if S3DG_KS_TRACE
extern "C" int s3dg_diag_ks_trace(void *buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(s3dg::g_ks_trace), &buf, sizeof(buf));
}
#endif
