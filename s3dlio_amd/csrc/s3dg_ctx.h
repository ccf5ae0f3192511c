// s3dg_ctx.h — the context behind the C ABI: its fields, the per-stream launch
// state and the measured defaults.  Private to the units that implement
// include/s3dlio_gpu.h over the context (s3dg_capi.cpp, s3dg_tune.cpp,
// s3dg_fill.cpp, s3dg_batchfill.cpp, s3dg_verify_batch.cpp, s3dg_keystream.cpp,
// s3dg_dgen_batch.cpp, s3dg_crc_batch.cpp, s3dg_tfrecord.cpp,
// and, through s3dg_accum.h, s3dg_measure.cpp, s3dg_chunks.cpp and
// s3dg_lz.cpp); everything else
// reaches a context through the functions of s3dg_internal.h.
#pragma once
#include "s3dg_internal.h"

#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace s3dg {

constexpr int kDefaultOccStream = 14, kDefaultOccBatch = -1;   // batch: -1 = per launch (below)
// Batch-kernel occupancy per launch: uncapped (32
// resident 1-wave workgroups per CU) unless the launch's zero prefixes end on
// a 64-B line (compress c with 64 % c == 0: c = 2, 4, 8, ... and ratios such
// as 4/3), where a cap of 29 resident workgroups writes 3-7 % faster: config 3
// 7214-7260 -> 7416-7424 GB/s, d1 c4 6925 -> 7435, d1 c8 6933 -> 7436, while
// the same cap costs c = 1, 1.5 and 3 (mid-line prefixes) 2-4 %
// (profiles/r03/diag/cfg3/power/).
// The target passed to occupancy_lds: asking for 30 gives a 5632-B LDS
// footprint, i.e. 29 resident (no 512-B granule gives exactly 30), which is
// what was measured and what s3dg_query_occupancy(ctx, 2, ..) reports.
constexpr int kOccZeroLines = 30;
// Zero prefixes of at least half the block that end inside a line (c = 3,
// 5, 6, 7, ...): uncapped, with the stores held until 100 wall-clock ticks
// (1 us) after the workgroup starts, whatever the GFX clock (DESIGN.md
// §5.1.2: config 5 7343 -> 7535-7540 GB/s, d1 c3 7115-7181 -> 7407-7450;
// config 2 would lose 0.4 %, so prefix-free launches keep no floor).
constexpr int kDefaultBatchRtFloor = -1;   // per launch
// Mixed-size batches (BASELINE config 4): one tile size per launch leaves the
// last tile of every object ragged, and small objects (a few blocks in a
// 64-block tile) are mostly dead slots.  Objects below kDefaultSplitBlocks
// blocks get a launch of their own, whose tile size is picked for them
// (DESIGN.md §5.1); 0 = off.
constexpr uint32_t kDefaultSplitBlocks = 0;
constexpr uint32_t kRtFloorMidZeros = 100;
// Uniform streams of large objects without a zero prefix (config 2): the same
// 1 us store floor.  On some boxes 10-45 % of such launches run 12.1-12.9 ms
// instead of 11.0-11.2 (round 4's driver line; round 5's final and lab boxes,
// at the normal clock and power): with the floor those boxes ran 0 % and
// 0-30 % slow launches, +1.0 / +1.9 % by mean (tools/dip_lab.py, bench.py
// --pace A/Bs, profiles/r05/dip/), while a box without them lost 0.2 %.
// Small objects (config 8) and batches (config 4) showed few slow launches
// and no gain (0 / -0.7 %), so they keep no floor.  DESIGN.md §5.1.4.
constexpr uint32_t kRtFloorLargeUniform = 100;
constexpr uint64_t kRtFloorLargeBlocks = 512;   // objects of >= 2 MiB
// The mid-line class's store floor is checked by measurement (round 4).  It
// won 2.6 % on one box and lost 0.5-1.6 % to a plain launch on four others
// (DESIGN.md §5.1.2): it compensates for the chip's power state, which
// differs between boxes.  So a context times its own large launches of that
// class (HIP events around the fill, read back without waiting, at a later
// launch) and runs the floor or the plain uncapped launch, whichever wrote
// faster: after kTuneFirst launches of each (alternating; the context's first
// timed launch is a warm-up and is not sampled), the MEANS of each one's last
// kTuneKeep rates, the plain launch taken only when it beats the current
// choice's mean by more than kTuneMargin (the class setting otherwise), so two
// candidates within the noise of each other do not flip from run to run
// (the best-of-3 rule did).  Means, not medians (round
// 6): on a box with the slow mode 47 % of plain config-5 launches ran 12.1-12.8
// ms against 11.0-11.3, which a median of five does not see, so the tuner kept
// probing a candidate 4 % slower by mean (tools/dip_lab.py,
// profiles/r06/slow/).  The loser is probed again after kTuneReprobe launches,
// and each probe that confirms the choice doubles that interval (up to
// kTuneReprobeMax), so a settled choice costs few probe launches.
// The line-aligned class keeps its cap unmeasured: it won 4-9 % on every box.
// Launches below kTuneMinBytes use the current choice; an explicit
// s3dg_set_occupancy / s3dg_set_batch_pace (or S3DG_ZC_TUNE=0) turns the
// check off.
constexpr uint64_t kTuneMinBytes = 1ull << 30;
constexpr uint64_t kTuneReprobe = 32, kTuneReprobeMax = 1024;
constexpr int kTuneKeep = 5, kTuneFirst = 4;
constexpr double kTuneMargin = 0.01;
struct ZcTuner {
    int best = 0;                  // 0 = the fitted rule, 1 = uncapped, no floor
    uint64_t launches = 0;         // timed launches issued
    uint64_t issued[2] = {0, 0};
    uint64_t interval = kTuneReprobe;   // launches between probes of the loser
    uint64_t next_probe = 0;            // launch index of the next probe (0: not scheduled)
    bool warm = false;                  // the first timed launch has been dropped
    double recent[2][kTuneKeep] = {};   // GB/s of the last kTuneKeep timed launches of each
    int samples[2] = {0, 0};
    struct Pending {
        hipEvent_t a, b;
        double bytes;
        int cand;
    };
    std::vector<Pending> pend;
    std::vector<hipEvent_t> spare;
};
constexpr uint32_t kDefaultPrefetch = 256;   // in 64-block units; > resident workgroups / 64
constexpr int kDefaultStreamTiles = 1;
constexpr uint64_t kStreamTilesMinBlocks = 16384;   // smaller streams: 2D kernel, no tile-map launch
constexpr int kDefaultStoreStream = kStoreNTSC1, kDefaultStoreBatch = kStoreSC1;
// dense batch layouts (one 64-B record per 4 KiB block): nt sc1 stores keep
// the written lines out of L2, where sc1 evicts the prefetched records
// (tools/batch_lab.py, profiles/r02/diag/batch_lab_store_*: 20 KiB+5 objects 4766 -> 6092 GB/s,
// dense 32 KiB 5977 -> 6663, dense 64 KiB 5992 -> 6472; tiled layouts keep sc1)
constexpr int kDefaultStoreDense = kStoreNTSC1;
// Draws per lane (kDefaultKsMinDraws, kKsLongDraws, kKsLongRounds, kKsMinSpan,
// kDgenPrefixMinDraws): s3dg_ks_plan.h, with the rule and the measurements.
// measured on MI355X (tools/k2_lab.py, profiles/r02/diag/k2_lab_r2e.log):
// 512-B row pieces, 4-wave workgroups, 1024 draws per lane and sc1 stores for
// both modes (K2 6010 vs 5803 GB/s at 2048 draws; DG1 c1 5933 / c2 6158 vs
// 5187 / 5409 for the round-1 DG1 shape of 128-B pieces and 2 waves).  With
// 1024 draws per lane a 1 MiB DG1 block is 128 lanes, so whole waves fall
// inside a zero prefix and skip the PRNG.
// XCD groups (k_keystream remaps workgroups so each XCD writes runs of
// adjacent waves' lane regions instead of every 8th workgroup) and 1-wave
// workgroups (a finished wave frees its slot without waiting for three
// others).  One process, interleaved (profiles/r02/diag/ks/ks_xcd_sweep.log):
//   K2 80 GiB, 4096 draws:   4 waves, dealing order 6475 -> 1 wave, groups of 16: 6737 GB/s
//   K2 8 GiB, 2048 draws:    6551 -> 7007
//   DG1 c1 80 GiB / 8 GiB:   6409 / 6561 -> 6646 / 6774
//   DG1 c2 (zero prefix, 512 draws): 6061 -> 6682 with 4 waves, groups of 32
//                            (1 wave, groups of 16: 6251)
constexpr int kDefaultKsXcdWaves = 16;
constexpr KsShape kDefaultKsShape[2] = {{64, 1, 0, kStoreSC1, kDefaultKsXcdWaves},
                                        {64, 1, 0, kStoreSC1, kDefaultKsXcdWaves}};
constexpr int kDgenPrefixWaves = 4, kDgenPrefixXcdWaves = 32;
// DG1 with a zero prefix, from this many whole 1 MiB blocks per launch: the
// prefixes as whole 4 KiB granules in the fill's store shape (k_zero_prefix),
// then the keystream over the tails alone (s3dg_set_dgen_zero_split;
// DESIGN.md §5.3).  The zero launch's occupancy cap and store policy.
// The zero launch's shape per prefix class, measured (tools/dg1_split_lab.py,
// profiles/r05/i, j: ten 8 GiB DG1 objects, one launch each / all in one):
// prefixes that end on a 64-B line (c = 2, 4, ...): 4-wave workgroups, 5
// resident per CU, nt sc1 stores, after the tails' launch on the same stream
// (c2 0.843 / 0.854, c4 0.875 against one keystream launch's 0.781 / 0.848,
// 0.842); mid-line prefixes (c = 3, 1.5, ...): 1-wave workgroups, 14 per CU,
// nt sc1, on a side stream concurrent with the tails (c3 0.794 / 0.866, c1.5
// 0.857 against 0.735 / 0.779, 0.729).  Index: [0] line-aligned, [1] mid-line.
constexpr uint64_t kDefaultDgenZeroSplit = 64;
constexpr int kZeroPrefixWaves[2] = {4, 1}, kZeroPrefixOcc[2] = {5, 14};
constexpr int kZeroPrefixStore[2] = {kStoreNTSC1, kStoreNTSC1}, kZeroPrefixOverlap[2] = {0, 1};

// Launch state private to one stream: the tile-record map of tiled launches
// and the batch-descriptor staging.  Launches on one stream are ordered by
// the stream, so a launch may rewrite the map as soon as it is enqueued after
// the previous one; launches on different streams share nothing and never
// wait on each other.
struct StreamState {
    std::mutex mu;                     // one enqueuing thread per stream at a time
    TileRec *tiles = nullptr;          // records of uniform tiled launches (device), grown on demand
    uint64_t tile_cap = 0;
    // batch records: two maps, so sub-batch k+1's k_batch_map (on `up`) runs
    // while sub-batch k's fill (on the stream) reads the other one
    TileRec *btiles[2] = {nullptr, nullptr};
    uint64_t btile_cap[2] = {0, 0};
    hipEvent_t mapped[2] = {nullptr, nullptr};   // map [i] written (on up)
    hipEvent_t filled[2] = {nullptr, nullptr};   // fill reading map [i] done (on the stream)
    int bnext = 0;
    hipStream_t up = nullptr;          // batch entry uploads + record maps (overlap the previous fill)
    // DG1 zero-prefix launches concurrent with their tails (s3dg_set_dgen_zero_split overlap)
    hipStream_t zs = nullptr;
    hipEvent_t zfork = nullptr, zjoin = nullptr;
    struct Stage {
        s3dg_obj_desc *host = nullptr, *dev = nullptr;   // pinned staging / device copy
        uint64_t *rec_lo = nullptr;    // device: record offset of each object (tile layouts)
        void *scan_tmp = nullptr;      // device: scan scratch
        size_t scan_tmp_bytes = 0;
        uint64_t cap = 0;
        hipEvent_t uploaded = nullptr;  // host staging may be rewritten
        hipEvent_t consumed = nullptr;  // device copy may be freed (k_batch_map done; both on `up`)
    } stage[2];
    int next = 0;
    // per-object result records of batch verify calls on this stream (device),
    // grown on demand; a call is synchronous, so the next one finds them idle
    VerifyRec *vobj = nullptr;
    uint64_t vobj_cap = 0;
    // queue counters of persistent keystream launches on this stream
    KsCounters ks;
    // chunk-record tables of DG1 batch calls (s3dg_dgen_batch.cpp): two sets,
    // so the host builds call k+1's records while call k's upload is pending.
    // The upload and the launches that read the device table are all on the
    // stream, which orders them; `uploaded` frees the pinned host side.
    struct DgenTable {
        DgenChunkRec *host = nullptr, *dev = nullptr;
        uint64_t cap = 0;
        hipEvent_t uploaded = nullptr;
    } dtab[2];
    int dnext = 0;
    // tables of batch CRC calls (s3dg_crc_batch.cpp), kept as the DG1 batch
    // keeps its records: two sets, the pinned side free once `uploaded`, the
    // device side ([entries | records | raw CRCs]) ordered by the stream; and
    // the result scratch of the synchronous form, which drains the stream
    struct CrcTable {
        uint8_t *host = nullptr, *dev = nullptr;
        uint64_t host_cap = 0, dev_cap = 0;
        hipEvent_t uploaded = nullptr;
    } ctab[2];
    int cnext = 0;
    uint32_t *crc_out = nullptr;
    uint64_t crc_out_cap = 0;
    // tables of TFRecord frame and check calls (s3dg_tfrecord.cpp), kept the
    // same way ([shard entries | raw CRCs of long records]); and the per-shard
    // records of the check form, which drains the stream
    CrcTable ttab[2];
    int tnext = 0;
    TfrDevRes *tfr_out = nullptr;
    uint64_t tfr_out_cap = 0;
    // lifetime (under the context's mu): users holding the state, and whether
    // s3dg_stream_release has taken it out of the context's map; the last
    // holder of a released state drains the stream and frees it
    int refs = 0;
    bool dead = false;
};

}  // namespace s3dg

// The C ABI's context type is global; its units work in namespace s3dg's names.
using namespace s3dg;

struct s3dg_ctx {
    int device = 0;
    int cus = 256;                     // compute units (sizes small keystream launches)
    // store cache policy: sc1 (write, then drop the line from
    // L2) for batches, nt sc1 for streams, measured best
    int store_stream = kDefaultStoreStream, store_batch = kDefaultStoreBatch;
    int store_dense = kDefaultStoreDense;   // batch launches in the dense layout
    int waves_per_block = 0;           // 0 = auto: 2 for streams, 1 for batches (measured)
    // resident fill workgroups per CU (0 = hardware max); measured on MI355X
    // (DESIGN.md §5.1): 14 for 2-wave stream blocks, no cap for 1-wave batch blocks
    int occ_stream = kDefaultOccStream, occ_batch = kDefaultOccBatch;
    int batch_rt_floor = kDefaultBatchRtFloor;   // batch kernel's wall-clock store floor (ticks; -1 = per launch)
    uint32_t prefetch_tiles = kDefaultPrefetch;   // batch tile-record prefetch distance
    uint32_t tile_shift = 0;           // batch tile = 2^tile_shift blocks; 0 = per launch
    bool tile_force_dense = false;     // batch: one record per 4 KiB granule when the layout allows
    // batch: objects of fewer blocks go to a launch of their own with their own
    // tile size (0 = one launch per sub-batch)
    uint32_t split_blocks = kDefaultSplitBlocks;
    // k_keystream launch shapes, [0] npz keystream, [1] DG1
    KsShape ks[2] = {kDefaultKsShape[0], kDefaultKsShape[1]};
    uint64_t ks_min_draws[2] = {kDefaultKsMinDraws[0], kDefaultKsMinDraws[1]};   // draws per lane
    bool ks_auto_waves[2] = {true, true}, ks_auto_xcd[2] = {true, true};          // not set by the caller
    int ks_persist = -1;               // persistent keystream launches from this many rounds (-1: default)
    uint64_t dgen_zero_split = kDefaultDgenZeroSplit;   // DG1 zero prefix + tail launches from this many blocks
    int zp_waves = -1, zp_occ = -1, zp_store = -1, zp_overlap = -1;   // -1: per prefix class (kZeroPrefix*)
    int64_t ks_tail = -1;              // one-object DG1 launches: chunks in half-length lanes at the end (-1: auto)
    void *base_dev = nullptr;          // 4 KiB base block in HBM
    uint8_t base_host[kBlk];
    // tile maps and batch staging, one set per stream (s3dg::StreamState)
    std::map<hipStream_t, StreamState *> streams;
    int stream_tiles = kDefaultStreamTiles;   // uniform streams through the tiled batch kernel
    std::map<std::pair<uint64_t, uint64_t>, uint64_t *> jtabs;   // (lpc << 32 | span, z0) -> device jump table
    void *crc_tab = nullptr;           // slicing-by-8 tables (device)
    uint32_t *crc_seg = nullptr;       // per-segment CRCs (device)
    uint64_t crc_seg_cap = 0;
    std::mutex crc_mu;
    std::vector<VerifyRec *> vrecs;    // idle verify result records (device; under mu), one taken per call
    ZcTuner tune[3];                   // per zero class (under mu)
    std::mutex mu;
};

namespace s3dg {

// Sets the calling thread's error text (s3dg_last_error) and returns code.
int fail(int code, const std::string &msg);
int hipfail(hipError_t e, const char *what);

#define HIP_TRY(expr, what)                          \
    do {                                             \
        hipError_t e_ = (expr);                      \
        if (e_ != hipSuccess) return hipfail(e_, what); \
    } while (0)

// Entry points: a null context is an error; the context's device is made
// current for the call and the caller's current device restored afterwards.
#define CTX_SCOPE(c)                                                   \
    if (!(c)) return fail(S3DG_EINVAL, "null context");                \
    DeviceScope dscope_((c)->device);                                  \
    if (!dscope_.ok()) return hipfail(dscope_.err, "hipSetDevice")

// zclass: the launch's zero-prefix class (zero_class; batches: the class of
// most of its blocks); picks the batch kernel's occupancy cap and store floor
// when they are not set explicitly (s3dg_set_occupancy, s3dg_set_batch_pace).
LaunchCfg cfg_for(s3dg_ctx *c, bool batch = false, int zclass = kZcNone);

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// Frees one stream's launch state; the caller has drained the stream (and
// its upload stream).
void stream_state_free(StreamState *S);

// The stream's launch state (created on first use), held and locked for the
// scope: one enqueuing thread per stream at a time, and a concurrent
// s3dg_stream_release never frees a state someone still holds (ADVICE r03:
// the holder that drops the last reference of a released state drains the
// stream and frees it).
class StreamLock {
public:
    StreamLock(s3dg_ctx *c, hipStream_t s) : c_(c), s_(s) {
        {
            std::lock_guard<std::mutex> g(c->mu);
            StreamState *&S = c->streams[s];
            if (!S) S = new StreamState();
            S_ = S;
            ++S_->refs;
        }
        S_->mu.lock();
    }
    ~StreamLock() {
        S_->mu.unlock();
        bool last;
        {
            std::lock_guard<std::mutex> g(c_->mu);
            last = --S_->refs == 0 && S_->dead;
        }
        if (last) {
            (void)hipStreamSynchronize(s_);
            if (S_->up) (void)hipStreamSynchronize(S_->up);
            if (S_->zs) (void)hipStreamSynchronize(S_->zs);
            stream_state_free(S_);
        }
    }
    StreamState *get() const { return S_; }
    StreamLock(const StreamLock &) = delete;
    StreamLock &operator=(const StreamLock &) = delete;

private:
    s3dg_ctx *c_;
    hipStream_t s_;
    StreamState *S_ = nullptr;
};

// A launch of class zc writing `bytes`: the candidate to run (0 = the fitted
// rule, 1 = plain) and whether to time it (*timed, events in *probe).
int tune_pick(s3dg_ctx *c, int zc, uint64_t bytes, bool *timed, ZcTuner::Pending *probe);
// Record the timed launch's events around it (start before, end after).  A
// probe whose launch failed (launched = false at the end mark) records no rate:
// its events go straight back to the spares (its near-zero elapsed
// time would otherwise enter the medians as a huge GB/s sample).
void tune_mark(s3dg_ctx *c, int zc, const ZcTuner::Pending &probe, bool end, hipStream_t s, bool launched = true);

// A synchronous verify call on stream s (s3dg_fill.cpp): a result record of
// the call's own from the context's idle list, reset on the stream;
// launch(rec) enqueues the compare kernels that add to it; the record is
// copied back, the stream drained, the record returned to the list.
int verify_with_record(s3dg_ctx *c, hipStream_t s, const char *launch_what,
                       const std::function<hipError_t(VerifyRec *)> &launch, s3dg_verify_result *out);

// The device jump table of lanes sub < lpc starting at draws z0 + sub*span,
// from the context's cache (s3dg_keystream.cpp).
int jump_table(s3dg_ctx *c, uint32_t lpc, uint64_t span, uint64_t z0, const uint64_t **jtab);

// A record map of at least `tiles` records in place of *map (s3dg_fill.cpp).
// The caller has waited for every launch that reads the old one.
int tile_map_grow(TileRec **map, uint64_t *cap, uint64_t tiles);

// The stream's batch state (s3dg_batchfill.cpp), shared by the batch fill and
// the batch verify: the upload stream and the events of both staging sets and
// both record maps, made on the stream's first batch call; and staging set G
// with room for n descriptors (its host buffer is free once its last upload
// finished, its device side once the map kernel that read it finished).
int batch_state_init(StreamState *S);
int stage_reserve(StreamState::Stage &G, uint64_t n, hipStream_t up);

// n_objs objects of obj_size bytes at dst + j*stride, entropy seed_base +
// ((first_obj + j) << 32), prefix parameters pp.  Large streams whose objects
// all start on the same 4 KiB granule (mod 8) run through the tiled batch
// kernel; the rest through the 2D stream kernel.
// held: the stream's state when the caller already holds it (batch sub-batches).
int fill_uniform(s3dg_ctx *c, uint8_t *dst, uint64_t obj_size, uint64_t stride, uint64_t n_objs,
                 const PrefixParams &pp, uint64_t seed_base, uint64_t first_obj, hipStream_t s,
                 StreamState *held = nullptr);

}  // namespace s3dg
