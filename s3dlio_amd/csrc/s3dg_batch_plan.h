// s3dg_batch_plan.h — the host's pass over a mixed-size batch and its layout
// decision ("Batches"), as pure functions of the descriptors
// and three context knobs: no HIP, no context, so the choice of layout can be
// compiled and tested on its own (tests/test_batch_plan.py).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "s3dlio_gpu.h"

namespace s3dg {

constexpr uint32_t kBlk = 4096;   // BLK_SIZE   src/constants.rs:326
// batch tiles (tile -> object map granule) are 2^tshift blocks, tshift in
// [kTileShiftMin, kTileShiftMax], chosen per launch (pick_tile_shift, plan_sub_batch).
// An object's records start at a multiple of its tile and its block 0 sits
// `lead` slots in, so a slot equals the granule it writes modulo min(8, tile):
// modulo 8 (each XCD writes its own granules) from 8-block tiles up and in the
// dense layout, modulo 2 and 4 only for the forced 2- and 4-block tiles.
constexpr uint32_t kTileShiftMin = 1, kTileShiftMax = 6;
// the per-launch choice considers 8..64-block tiles only: 2- and 4-block tiles
// (s3dg_set_batch_tile) cut dead slots but lose more to records, e.g. 16-B
// packed 20 KiB objects 2556 vs 2917 GB/s (profiles/r02/diag/desc40/ab3_*.log)
constexpr uint32_t kTileShiftAutoMin = 3;
// tshift 0 (one record per 4 KiB granule of the batch's address range, no
// per-object lead) is the dense layout for small packed objects

// ---- the record rules ------------------------------------------------------------
// What one object gets in a sub-batch's record map, as functions the host's
// pass and the device's scan functor and k_batch_map share (S3DG_BP_HD), so a
// CPU sweep walks the very arithmetic the kernels run
// (tests/capi/batch_records_sweep.cpp).
#if defined(__HIPCC__)
#define S3DG_BP_HD __host__ __device__
#else
#define S3DG_BP_HD
#endif

S3DG_BP_HD inline uint64_t obj_blocks(uint64_t size) { return (size + kBlk - 1) / kBlk; }

// Lead of an object: the 4 KiB granule (mod 8) of its first byte's address,
// base + dst_off.  A tiled object's block 0 sits at slot `lead` of its first
// tile, so slot and granule agree modulo the tile size (up to 8).
S3DG_BP_HD inline uint64_t obj_lead(uint64_t base, uint64_t dst_off) { return ((base + dst_off) >> 12) & 7; }

// Tiles (records) of nb blocks behind `lead` dead slots, rounded up.
S3DG_BP_HD inline uint64_t obj_tiles(uint64_t nb, uint64_t lead, uint32_t tshift) {
    return (nb + lead + (1ull << tshift) - 1) >> tshift;
}

// Records [lo, hi) of one object in its class's map and the slot of its block 0
// behind lo << tshift.
struct RecRange {
    uint64_t lo, hi, lead;
};

// Tiled: `scan` = the exclusive sum of obj_tiles over the class's objects before it.
S3DG_BP_HD inline RecRange tiled_records(uint64_t scan, uint64_t nb, uint64_t base, uint64_t dst_off, uint32_t tshift) {
    const uint64_t lead = obj_lead(base, dst_off);
    return RecRange{scan, scan + obj_tiles(nb, lead, tshift), lead};
}

// Dense: record = granule of the sub-batch's address range, counted from the
// first object's granule (mod 8) lead0, so the object's block 0 is at slot g0 =
// lead0 + (dst_off - first_off) / 4 KiB.  The first object's records start at
// 0 (its lead is lead0); every other object's at g0.  They end at the
// successor's g0 (has_next: next_off is its dst_off), so the gap behind an
// object is its dead slots, or behind its last block.
S3DG_BP_HD inline RecRange dense_records(bool is_first, uint64_t lead0, uint64_t first_off, uint64_t dst_off,
                                         uint64_t nb, bool has_next, uint64_t next_off) {
    const uint64_t g0 = lead0 + (dst_off - first_off) / kBlk;
    const uint64_t lo = is_first ? 0 : g0;
    return RecRange{lo, has_next ? lead0 + (next_off - first_off) / kBlk : g0 + nb, g0 - lo};
}

// Records of the dense layout of objects from first_off to last_end, the
// first one at granule lead0 (mod 8).
S3DG_BP_HD inline uint64_t dense_span(uint64_t lead0, uint64_t first_off, uint64_t last_end) {
    return lead0 + (last_end - first_off) / kBlk;
}

// k_batch_map: an object of at most this many records writes them itself; the
// records of one with more are written by its whole wave, 64 per pass.
constexpr uint64_t kMapOwnRecords = 16;
S3DG_BP_HD inline bool map_own_records(uint64_t recs) { return recs <= kMapOwnRecords; }

// Slot k of the tile whose first slot is `first`: the object's block, negative
// for a lead slot (dead, as a block at or past the object's end is).  Restates
// k_fill_batch's expression `(int64_t)e.first + k - e.lead`, which stays written
// out in the kernel.
S3DG_BP_HD inline int64_t slot_block(uint32_t first, uint32_t k, uint32_t lead) { return (int64_t)first + k - lead; }

// The small class of a split sub-batch (s3dg_set_batch_split).
S3DG_BP_HD inline bool split_small(uint64_t nb, uint64_t split) { return nb < split; }

// Launch classes by zero prefix (per launch; batches by majority of blocks)
enum ZeroClass { kZcNone = 0, kZcLines = 1, kZcMidHeavy = 2 };

// Zero-prefix class of compress (f_num, f_den): kZcLines when const_len =
// 4096 f_num / f_den is a multiple of 64 (64 f_num / f_den whole), i.e. the
// prefix ends on a 64-B line in every block; kZcMidHeavy when it ends inside
// a line and covers at least half the block; kZcNone otherwise.
static inline int zero_class(uint64_t f_num, uint64_t f_den) {
    if (f_num == 0 || f_den == 0) return kZcNone;
    if ((f_num * 64) % f_den == 0) return kZcLines;
    return 2 * f_num >= f_den ? kZcMidHeavy : kZcNone;
}

// Batch tile size: every object's last tile is ragged, and its blocks past
// the object's end are workgroups that start, load the record and exit.
// Smaller tiles cut those, at one 64-B record (and one more record miss per
// XCD) per tile.  Pick the tile size that minimises launched workgroups +
// kTileCost x records.
constexpr uint64_t kTileCost = 2;

inline uint32_t pick_tile_shift(const uint64_t (&ntiles)[kTileShiftMax + 1]) {
    uint32_t best = kTileShiftMax;
    uint64_t best_cost = UINT64_MAX;
    for (uint32_t sh = kTileShiftMax; sh >= kTileShiftAutoMin; --sh) {
        const uint64_t cost = (ntiles[sh] << sh) + kTileCost * ntiles[sh];
        if (cost < best_cost) { best_cost = cost; best = sh; }
    }
    return best;
}

// relative costs in units of one live 4 KiB block, fitted
// to forced dense / 8-block layouts of uniform 7..26-block objects with the
// dense launches' nt sc1 stores (profiles/r02/diag/batch_lab_store_cost.log)
constexpr double kDeadSlotCost = 0.4, kRecordCost = 0.05;
// Among tile sizes, the costs measured on config 4's mixed sizes (forced 64 /
// 32 / 16 / 8-block tiles: 7249 / 7215 / 7152 / 6991 GB/s, one process,
// profiles/r03/diag/cfg4/cfg4_tiles.log) fit a dead slot at ~0 and a record at
// ~0.25 live blocks: a tile's dead slots find its record already in the
// scalar cache, while each extra record is one more miss on a workgroup's
// critical path.  The first model (above) picked 16-block tiles there; it
// still decides dense vs tiled, as fitted.
constexpr double kDeadSlotCostTiled = 0.1, kRecordCostTiled = 0.25;

// The 8..64-block tile size of least dead_cost x dead slots + record_cost x
// records for objects of `blocks` live blocks in ntiles[sh] tiles of 2^sh
// (the larger tile on a tie); *cost: that least cost.
inline uint32_t best_tile_shift(const uint64_t *ntiles, uint64_t blocks, double dead_cost, double record_cost,
                                double *cost = nullptr) {
    uint32_t best_sh = kTileShiftMax;
    double best = 1e300;
    for (uint32_t sh = kTileShiftMax; sh >= kTileShiftAutoMin; --sh) {
        const double c = dead_cost * (double)((ntiles[sh] << sh) - blocks) + record_cost * (double)ntiles[sh];
        if (c < best) { best = c; best_sh = sh; }
    }
    if (cost) *cost = best;
    return best_sh;
}

// Pass 1 over descriptors [k0, k1): validation, slot counts per tile size,
// dense-layout test.
struct BatchScan {
    uint64_t m = 0, blocks = 0, zc_blocks[3] = {}, ntiles[kTileShiftMax + 1] = {};
    // objects below the split threshold: count, blocks, tiles per tile size
    uint64_t ms = 0, blocks_s = 0, ntiles_s[kTileShiftMax + 1] = {};
    uint64_t first_off = 0, last_end = 0;
    bool dense_ok = true;
    // uniform: every non-empty object has the first's size, dedup and ratio,
    // at a constant stride (>= size) with entropy stepping by 2^32, i.e. the
    // batch is a stream (s3dg_fill_controlled_stream's layout and seeds)
    bool uni = true;
    s3dg_obj_desc ufirst{}, ulast{};
    uint64_t ustride = 0;
    int err = S3DG_OK;
    const char *msg = nullptr;
};

// Does object b continue the uniform run whose last object is a (stride 0: not yet known)?
static inline bool uni_next(const s3dg_obj_desc &first, const s3dg_obj_desc &a, const s3dg_obj_desc &b,
                           uint64_t &stride) {
    if (b.size != first.size || b.dedup != first.dedup || b.f_num != first.f_num || b.f_den != first.f_den ||
        b.entropy - a.entropy != (1ull << 32) || b.dst_off < a.dst_off)
        return false;
    const uint64_t st = b.dst_off - a.dst_off;
    if (stride == 0) stride = st;
    return st == stride && st >= first.size;
}

static inline void batch_scan(const s3dg_obj_desc *__restrict d, uint64_t k0, uint64_t k1, uintptr_t base,
                              BatchScan &P, s3dg_obj_desc *__restrict out, uint64_t split) {
    // accumulators in registers (P aliases nothing, but the compiler cannot
    // know that across the staging stores); the checks fold into one flag
    uint64_t m = 0, blocks = 0, zc_blocks[3] = {}, first = 0, last = 0, nt[kTileShiftMax + 1] = {};
    uint64_t ms = 0, blocks_s = 0, nts[kTileShiftMax + 1] = {};
    bool dense = true, bad = false, uni = true;
    uint32_t zc_num = 0, zc_den = 1;   // last compress seen and its zero_class
    int zc = kZcNone;
    s3dg_obj_desc ufirst{}, uprev{};
    uint64_t ustride = 0;
    for (uint64_t k = k0; k < k1; ++k) {
        const s3dg_obj_desc o = d[k];
        out[k - k0] = o;   // staged as is; empty objects are squeezed out afterwards (rare)
        if (o.size == 0) continue;
        if (m == 0) ufirst = o;
        else uni = uni && uni_next(ufirst, uprev, o, ustride);
        uprev = o;
        const uint64_t nb = obj_blocks(o.size);
        bad |= (o.dst_off & 15u) != 0 || o.f_den == 0 || o.f_num >= o.f_den || nb >= (1ull << 31);
        const uint64_t lead = obj_lead(base, o.dst_off);   // the blocks sit behind the XCD lead
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) nt[sh] += obj_tiles(nb, lead, sh);
        if (split_small(nb, split)) {
            ++ms;
            blocks_s += nb;
            for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) nts[sh] += obj_tiles(nb, lead, sh);
        }
        if (m == 0) first = o.dst_off;
        dense = dense && (m == 0 || o.dst_off >= last) && (o.dst_off & (kBlk - 1)) == 0;
        last = o.dst_off + nb * kBlk;
        blocks += nb;
        if (o.f_num != zc_num || o.f_den != zc_den) {
            zc_num = o.f_num;
            zc_den = o.f_den;
            zc = zero_class(o.f_num, o.f_den);
        }
        zc_blocks[zc] += nb;
        ++m;
    }
    if (bad) {   // the first offending descriptor names the error
        for (uint64_t k = k0; k < k1; ++k) {
            const s3dg_obj_desc &o = d[k];
            if (o.size == 0) continue;
            P.err = S3DG_EINVAL;
            if (o.dst_off & 15u) { P.msg = "dst_off must be a multiple of 16"; return; }
            if (o.f_den == 0 || o.f_num >= o.f_den) { P.msg = "need f_num < f_den"; return; }
            if ((o.size + kBlk - 1) / kBlk >= (1ull << 31)) { P.msg = "object larger than 2^31 blocks"; return; }
            P.err = S3DG_OK;
        }
    }
    P.m = m;
    P.blocks = blocks;
    P.ms = ms;
    P.blocks_s = blocks_s;
    for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) P.ntiles_s[sh] = nts[sh];
    for (int k = 0; k < 3; ++k) P.zc_blocks[k] = zc_blocks[k];
    P.first_off = first;
    P.last_end = last;
    P.dense_ok = dense;
    P.uni = uni;
    P.ufirst = ufirst;
    P.ulast = uprev;
    P.ustride = ustride;
    for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) P.ntiles[sh] = nt[sh];
}

// The pass over a sub-batch of n descriptors runs in up to kPrepParts parts
// (one host thread each): their number, and the first descriptor of part q
// of [k0, k1) (q = parts: k1).
constexpr int kPrepParts = 8;                   // host threads per sub-batch pass
constexpr uint64_t kPrepMinPerPart = 8192;      // descriptors below which a pass stays single-threaded
inline int batch_parts(uint64_t n) {
    const int parts = (int)(n / kPrepMinPerPart);
    return parts < 1 ? 1 : (parts > kPrepParts ? kPrepParts : parts);
}
inline uint64_t batch_cut(uint64_t k0, uint64_t k1, int q, int parts) {
    return k0 + (k1 - k0) * (uint64_t)q / (uint64_t)parts;
}

// The scans of a sub-batch's parts (consecutive descriptor ranges) merged in
// order.  The first offending part names the error (err, msg).
inline BatchScan batch_scan_merge(const BatchScan *part, int parts) {
    BatchScan P;
    for (int q = 0; q < parts; ++q) {
        const BatchScan &Q = part[q];
        if (Q.err) {
            P.err = Q.err;
            P.msg = Q.msg;
            return P;
        }
        if (Q.m == 0) continue;
        if (P.m == 0) {
            P.first_off = Q.first_off;
            P.ufirst = Q.ufirst;
            P.uni = Q.uni;
            P.ustride = Q.ustride;
        } else {
            if (Q.first_off < P.last_end) P.dense_ok = false;
            // the runs join: Q's first object continues P's last, same stride
            uint64_t st = P.ustride;
            P.uni = P.uni && Q.uni && uni_next(P.ufirst, P.ulast, Q.ufirst, st) &&
                    (Q.ustride == 0 || Q.ustride == st);
            P.ustride = st;
        }
        P.ulast = Q.ulast;
        P.dense_ok = P.dense_ok && Q.dense_ok;
        P.last_end = Q.last_end;
        P.m += Q.m;
        P.blocks += Q.blocks;
        for (int k = 0; k < 3; ++k) P.zc_blocks[k] += Q.zc_blocks[k];
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) P.ntiles[sh] += Q.ntiles[sh];
        P.ms += Q.ms;
        P.blocks_s += Q.blocks_s;
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) P.ntiles_s[sh] += Q.ntiles_s[sh];
    }
    return P;
}

// The context's layout knobs: s3dg_set_batch_tile (tile_shift, force_dense)
// and s3dg_set_batch_split.
struct BatchKnobs {
    uint32_t tile_shift;     // forced tile = 2^tile_shift blocks; 0 = per launch
    bool force_dense;        // one record per 4 KiB granule when the layout allows
    uint32_t split_blocks;   // objects of fewer blocks: a class of their own; 0 = off
};

// How a sub-batch of P.m > 0 non-empty objects runs.
struct BatchPlan {
    bool uniform;                 // run as a stream: ufirst, ustride, m (nothing else is set)
    uint32_t tshift;              // 0 = dense
    uint64_t lead0, span;         // first object's granule (mod 8); dense: records of the address range
    int nclass;                   // 1, or 2 when small and large objects get different tile sizes
    // staged objects [first, first + count) with records [rec0, rec0 + recs) of 2^tshift blocks
    struct { uint64_t first, count, rec0, recs; uint32_t tshift; } cls[2];
    uint64_t recs;                // total records
    int zclass;                   // majority class of the blocks
};

inline BatchPlan plan_sub_batch(const BatchScan &P, uintptr_t base, const BatchKnobs &K) {
    BatchPlan B{};
    const uint64_t m = P.m;
    if (m == 0) return B;
    // a uniform sub-batch is a stream: the stream paths (tiled records per
    // 64 blocks, or the 2D kernel with no records at all) instead of a
    // record per tile or granule (config 10's records
    // were 6 % of its traffic).  Unless a batch layout is forced.
    if (P.uni && m >= 2 && !K.tile_shift && !K.force_dense) {
        B.uniform = true;
        return B;
    }
    B.lead0 = obj_lead(base, P.first_off);
    B.span = P.dense_ok ? dense_span(B.lead0, P.first_off, P.last_end) : 0;
    // layout: forced (s3dg_set_batch_tile) or least cost
    uint32_t tshift = kTileShiftMax;
    if (K.tile_shift == 0 && K.force_dense && P.dense_ok) tshift = 0;
    else if (K.tile_shift) tshift = K.tile_shift;
    else {
        // tile size by the tiled costs; dense vs the first model's best tiling by the first model
        double best;
        (void)best_tile_shift(P.ntiles, P.blocks, kDeadSlotCost, kRecordCost, &best);
        tshift = best_tile_shift(P.ntiles, P.blocks, kDeadSlotCostTiled, kRecordCostTiled);
        if (P.dense_ok && kDeadSlotCost * (double)(B.span - P.blocks) + kRecordCost * (double)B.span < best)
            tshift = 0;
    }
    B.tshift = tshift;
    // two classes (s3dg_set_batch_split): the small objects first, each
    // class with the tile size the tiled cost model picks for it alone
    uint64_t ms = 0;
    uint32_t tsh_s = tshift, tsh_l = tshift;
    if (tshift && !K.tile_shift && K.split_blocks && P.ms > 0 && P.ms < m) {
        uint64_t nt_l[kTileShiftMax + 1] = {};
        for (uint32_t sh = kTileShiftMin; sh <= kTileShiftMax; ++sh) nt_l[sh] = P.ntiles[sh] - P.ntiles_s[sh];
        tsh_s = best_tile_shift(P.ntiles_s, P.blocks_s, kDeadSlotCostTiled, kRecordCostTiled);
        tsh_l = best_tile_shift(nt_l, P.blocks - P.blocks_s, kDeadSlotCostTiled, kRecordCostTiled);
        if (tsh_s != tsh_l) ms = P.ms;
    }
    const uint64_t recs_s = ms ? P.ntiles_s[tsh_s] : 0;
    B.recs = tshift == 0 ? B.span
             : ms        ? recs_s + (P.ntiles[tsh_l] - P.ntiles_s[tsh_l])
                         : P.ntiles[tshift];
    if (ms) {
        B.nclass = 2;
        B.cls[0] = {0, ms, 0, recs_s, tsh_s};
        B.cls[1] = {ms, m - ms, recs_s, B.recs - recs_s, tsh_l};
    } else {
        B.nclass = 1;
        B.cls[0] = {0, m, 0, B.recs, tshift};
    }
    B.zclass = 2 * P.zc_blocks[kZcLines] > P.blocks      ? kZcLines
               : 2 * P.zc_blocks[kZcMidHeavy] > P.blocks ? kZcMidHeavy
                                                         : kZcNone;
    return B;
}

// The staged descriptors H[0, n) in the plan's order: the empty objects
// squeezed out (m remain), then for two classes a stable partition, the
// objects below `split` blocks first.
inline void order_staging(s3dg_obj_desc *H, uint64_t n, uint64_t m, const BatchPlan &B, uint64_t split) {
    if (m != n) {   // squeeze out the empty objects
        uint64_t j = 0;
        for (uint64_t i = 0; i < n; ++i)
            if (H[i].size) H[j++] = H[i];
    }
    if (B.nclass == 2) {   // stable partition: small objects first
        std::vector<s3dg_obj_desc> big;
        big.reserve(B.cls[1].count);
        uint64_t j = 0;
        for (uint64_t i = 0; i < m; ++i) {
            if (split_small(obj_blocks(H[i].size), split)) H[j++] = H[i];
            else big.push_back(H[i]);
        }
        std::copy(big.begin(), big.end(), H + j);
    }
}

// A call's descriptors are cut into sub-batches: 16 Ki objects first, doubling
// to 256 Ki, so the host's pass over one overlaps the fill of the one before.
constexpr uint64_t kBatchSubFirst = 16384, kBatchSubMax = 262144;

}  // namespace s3dg
