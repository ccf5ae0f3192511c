/*
 * s3dlio_gpu.h — C ABI of the MI355X-native synthetic object-payload
 * generator (drop-in for s3dlio's src/data_gen.rs hot path).
 *
 * Every entry point is plain C: pointers, sizes, integers.  All functions
 * return 0 on success or a negative S3DG_E* code; s3dg_last_error() returns
 * a thread-local message for the last failure on the calling thread.
 *
 * Reference interfaces replaced (paths relative to the s3dlio checkout):
 *   s3dlio_fill_controlled_data         src/data_gen.rs:151  fill_controlled_data(buf,dedup,compress)
 *   s3dlio_fill_controlled_data_seeded  src/data_gen.rs:151  (seeded sibling)
 *   s3dg_fill_controlled                src/data_gen.rs:198-223 (the Rayon par_chunks_mut loop)
 *   s3dg_fill_controlled_stream         src/s3_utils.rs:1741 / src/bin/cli.rs:2282 generate_object
 *                                       fan-out, one payload per object
 *   s3dg_fill_controlled_batch          same, mixed object sizes (BASELINE config 4)
 *   s3dg_unique_blocks                  src/data_gen.rs:162-167
 *   s3dg_compress_ratio                 src/data_gen.rs:169-173
 *
 * Device pointers passed to s3dg_fill_* must be 16-byte aligned (objects in
 * a stream/batch too); `stream` is a hipStream_t (NULL = legacy default).
 */
#ifndef S3DLIO_GPU_H
#define S3DLIO_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

#define S3DG_BLOCK_SIZE 4096u   /* BLK_SIZE, src/constants.rs:326 */

enum {
    S3DG_OK = 0,
    S3DG_EINVAL = -1,   /* bad argument (null, misaligned, out of range) */
    S3DG_EHIP = -2,     /* HIP runtime error (message in s3dg_last_error) */
    S3DG_ENOMEM = -3,
    S3DG_EIO = -4,      /* file-system error in the put pipeline */
};

typedef struct s3dg_ctx s3dg_ctx;

/* One object of a batch: `dst_off` bytes from dst_base (multiple of 16),
 * `size` bytes, block seeds `u + entropy` (src/data_gen.rs:202), zero-prefix
 * ratio f_num/f_den of each 4 KiB block (compress c -> (c-1, c)). */
typedef struct {
    uint64_t dst_off;
    uint64_t size;
    uint64_t entropy;
    uint64_t dedup;
    uint32_t f_num;
    uint32_t f_den;
} s3dg_obj_desc;

/* ---- context ------------------------------------------------------------ */
int s3dg_ctx_create(int device, s3dg_ctx **out);
int s3dg_ctx_destroy(s3dg_ctx *ctx);
int s3dg_ctx_device(s3dg_ctx *ctx, int *device);
/* Replace the 4 KiB base block (stands in for A_BASE_BLOCK,
 * src/constants.rs:715-720).  Host pointer, 4096 bytes. */
int s3dg_set_base_block(s3dg_ctx *ctx, const uint8_t *base4096);
/* Base block = Xoshiro256++(seed_from_u64(seed)).fill_bytes(4096). */
int s3dg_set_base_block_seed(s3dg_ctx *ctx, uint64_t seed);
int s3dg_get_base_block(s3dg_ctx *ctx, uint8_t *out4096);
/* Wave64s per 4 KiB block = workgroup size / 64: 1, 2 or 4; 0 = auto
 * (2 for streams, 1 for batches).  A tuning knob; results are identical. */
int s3dg_set_waves_per_block(s3dg_ctx *ctx, int waves);
/* 1 = nontemporal stores in every fill kernel, 0 = the default policies. */
int s3dg_set_nontemporal(s3dg_ctx *ctx, int on);
/* Cache policy of the fill kernels' 16-byte stores, for stream and batch
 * launches: 0 = plain, 1 = nt, 2 = sc1, 3 = nt sc1, negative = default
 * (nt sc1 for streams; sc1 for tiled batch launches and nt sc1 for batch
 * launches in the dense layout, measured on MI355X).  A non-negative batch
 * policy applies to both batch layouts.  Results are identical. */
int s3dg_set_store_policy(s3dg_ctx *ctx, int stream_policy, int batch_policy);
/* Cap on resident fill workgroups per CU (reserved LDS), for stream and
 * batch launches separately; 0 = hardware maximum, negative = the default.
 * Defaults, measured on MI355X: 14 (stream); batch launches (and large
 * uniform streams, which run through the batch kernel) per launch: no cap,
 * or 29 resident when most of the launch's blocks have a zero prefix ending on
 * a 64-B line (64 f_num / f_den whole: compress 2, 4, 8, ...).  A cap of k
 * reserves the LDS that leaves floor(160 KiB / footprint) resident, which the
 * 512-B allocation granule can make k - 1 (30 gives 29); s3dg_query_occupancy
 * reports the resident count.  A tuning knob; results are identical. */
int s3dg_set_occupancy(s3dg_ctx *ctx, int stream_wgs_per_cu, int batch_wgs_per_cu);
/* Batch kernel (batches and large uniform streams): the stores of each 4 KiB
 * block wait until `ticks` wall-clock ticks (10 ns) after its workgroup
 * started; 0 = no floor, negative = per launch (100 when most of the
 * launch's blocks have a zero prefix of at least half the block that ends
 * inside a 64-B line, e.g. compress 3, and for uniform streams of objects of
 * >= 2 MiB without a zero prefix; none otherwise).  Measured on MI355X;
 * results are identical. */
int s3dg_set_batch_pace(s3dg_ctx *ctx, int ticks);
/* Batch launches: distance (in units of 64 blocks) at which workgroups warm
 * the L2 with later tile records; 0 = off, UINT32_MAX = default (256).
 * Results are identical. */
int s3dg_set_batch_prefetch(s3dg_ctx *ctx, uint32_t tiles);
/* Batch launches: blocks per tile record (2, 4, 8, 16, 32 or 64), 1 = dense (one
 * record per 4 KiB granule of the batch's address range; used only when
 * the objects are 4 KiB-aligned, sorted and non-overlapping); 0 = chosen per
 * sub-batch by cost (default).  Results are identical. */
int s3dg_set_batch_tile(s3dg_ctx *ctx, uint32_t blocks);
/* Batch launches with per-launch tile sizes: objects of fewer than `blocks`
 * 4 KiB blocks go to a launch of their own (each class with the tile size
 * that suits it), so small objects do not pad large tiles with dead slots;
 * 0 = one launch, negative = default.  Results are identical. */
int s3dg_set_batch_split(s3dg_ctx *ctx, int blocks);
/* 1 = run large uniform streams (>= 64 MiB, objects 32 KiB-aligned relative
 * to each other) through the tiled batch kernel with device-built tile
 * records and the batch launch knobs; 0 = always the 2D stream kernel;
 * negative = default (1).  Results are identical. */
int s3dg_set_stream_tiles(s3dg_ctx *ctx, int on);
/* Keystream kernel launch shape for mode 0 (npz keystream, s3dg_xoshiro_fill)
 * or mode 1 (DG1, s3dg_dgen_fill and the generators): draws staged per lane
 * per store round (16, 32 or 64), waves per workgroup (1, 2 or 4), resident
 * workgroups per CU cap (0 = none), draws per lane (>= 64; sets lanes per
 * chunk; launches too small to fill the GPU use shorter spans, down to 256), store cache policy (as s3dg_set_store_policy, negative =
 * default).  0 = default for each (both modes: 64, 1, 2048 draws, sc1; K2
 * launches of >= 4 rounds of resident waves: 4096 draws; DG1 with a zero
 * prefix: 4 waves, 512 draws).
 * A tuning knob; results are identical. */
int s3dg_set_keystream_shape(s3dg_ctx *ctx, int mode, int draws, int waves, int wgs_per_cu,
                             uint64_t min_lane_draws, int store_policy);
/* Keystream launches (mode 0 / 1): workgroups are remapped so each XCD
 * writes runs of `waves` adjacent waves' lane regions (power of two; at or
 * below the waves per workgroup = the dispatcher's round-robin order; 0 =
 * default: 16, DG1 with a zero prefix 32).  A tuning knob; results are
 * identical. */
int s3dg_set_keystream_xcd_group(s3dg_ctx *ctx, int mode, uint32_t waves);
/* Keystream launches (both modes) of at least `rounds` rounds of resident
 * waves run a persistent grid: one round of workgroups whose waves take work
 * units from per-XCD queues (an XCD that runs ahead takes over units of a
 * slower one instead of idling at the end of the launch).  0 = never; negative
 * = default: 1-wave workgroups from 6 rounds.  A tuning knob; results are
 * identical. */
int s3dg_set_keystream_persist(s3dg_ctx *ctx, int rounds);
/* DG1 launches with a zero prefix (compress > 1) of at least `chunks` whole
 * 1 MiB blocks (all of them full length) run as two launches: the blocks'
 * zero prefixes in the fill's store shape (whole 4 KiB granules, every XCD on
 * every 8th), then the keystream over the blocks' tails only.  chunks: 0 =
 * always one keystream launch, negative = default (64).  The zero launch:
 * `waves` per 4 KiB workgroup (1, 2, 4), `occupancy` resident workgroups per
 * CU cap (0 = none), `store` policy (as s3dg_set_store_policy), `overlap` 1 =
 * on a side stream concurrent with the tails (the caller's stream waits for
 * both); negative = default for each (measured per prefix class: prefixes
 * ending on a 64-B line, e.g. compress 2 or 4: 4 waves, 5 per CU, nt sc1, in
 * order; others: 1 wave, 14 per CU, nt sc1, overlapped).  A tuning knob;
 * results are identical. */
int s3dg_set_dgen_zero_split(s3dg_ctx *ctx, int chunks, int waves, int occupancy, int store, int overlap);
/* One-object DG1 launches that run a persistent grid (see above): their last
 * `chunks` 1 MiB blocks in lanes of half the length, handed out after the
 * others, so the launch drains on shorter units.  0 = off; negative =
 * default (half a resident round of units).  A tuning knob; results are
 * identical. */
int s3dg_set_keystream_tail(s3dg_ctx *ctx, int chunks);
int s3dg_query_keystream_occupancy(s3dg_ctx *ctx, int mode, int *wgs_per_cu);
/* Resident workgroups per CU the current settings give (HIP occupancy API):
 * batch 0 = stream launches, 1 = batch launches, 2 = batch launches whose
 * zero prefixes end on a 64-B line (see s3dg_set_occupancy). */
int s3dg_query_occupancy(s3dg_ctx *ctx, int batch, int *wgs_per_cu);

/* ---- parameter helpers (host math shared with the kernels) --------------- */
uint64_t s3dg_unique_blocks(uint64_t nblocks, uint64_t dedup);
int s3dg_compress_ratio(uint64_t compress, uint32_t *f_num, uint32_t *f_den);
/* Launch class of compress (f_num, f_den) for the batch kernel's per-launch
 * settings: 1 = zero prefix ending on a 64-B line (occupancy
 * cap: 29 resident workgroups per CU, which s3dg_query_occupancy(ctx, 2, ..)
 * reports; the 512-B LDS granule admits no footprint giving exactly 30),
 * 2 = zero prefix of at least half the block ending inside a line (store
 * floor 100 ticks), 0 = otherwise, or f_den = 0 (no cap, no floor). */
int s3dg_zero_class(uint32_t f_num, uint32_t f_den);
/* Batch-kernel launches of zero class 2 (above) check their store floor by
 * measurement: the context times its own launches of >= 1 GiB and runs the
 * floor or a plain launch (the means of each one's last five rates, after
 * four launches of each, the context's first timed launch not counted; the
 * other is taken only when more than 1 % faster than the current choice, so
 * near-equal candidates do not flip between runs), re-probing the other after
 * 32 launches, an interval that doubles with every probe that confirms the
 * choice (up to 1024); class 1 keeps its cap.  An explicit
 * s3dg_set_occupancy / s3dg_set_batch_pace (or env S3DG_ZC_TUNE=0) turns this
 * off.  Query (zclass 0-2): the choice (0 = the class setting, 1 = plain),
 * each one's mean recent GB/s (0 = not measured yet) and the timed launch
 * count.  Results are identical. */
int s3dg_query_zero_tune(s3dg_ctx *ctx, int zclass, int *best, double *rule_gbs, double *plain_gbs,
                         uint64_t *timed);
/* Per-object entropy of object j of a stream: seed_base + j * 2^32. */
uint64_t s3dg_object_entropy(uint64_t seed_base, uint64_t j);

/* ---- device-resident generation (asynchronous on `stream`) -------------- */
/* One object of `len` bytes at dst (device).  From 64 MiB up this runs as a
 * one-object stream on the tiled kernel (s3dg_set_stream_tiles). */
int s3dg_fill_controlled(s3dg_ctx *ctx, void *dst, uint64_t len, uint64_t dedup,
                         uint32_t f_num, uint32_t f_den, uint64_t entropy,
                         void *stream);
/* Blocks [blk_lo, blk_hi) of one `len`-byte object: block blk_lo lands at
 * dst.  Used to stream one large object through a smaller device buffer. */
int s3dg_fill_controlled_range(s3dg_ctx *ctx, void *dst, uint64_t len,
                               uint64_t blk_lo, uint64_t blk_hi, uint64_t dedup,
                               uint32_t f_num, uint32_t f_den, uint64_t entropy,
                               void *stream);
/* Seeded analogue of generate_random_data (src/data_gen.rs:102-132, whose
 * ThreadRng makes it unseedable): the context's base block tiled per 4 KiB
 * block, bytes [0, min(32, L)) then [L-32, L) when L > 2048 overwritten by
 * SmallRng::seed_from_u64(entropy + i).fill_bytes for block i. */
int s3dg_random_data(s3dg_ctx *ctx, void *dst, uint64_t len, uint64_t entropy, void *stream);
/* n equal-size objects, object j at dst + j*stride, entropy
 * s3dg_object_entropy(seed_base, first_obj + j). */
int s3dg_fill_controlled_stream(s3dg_ctx *ctx, void *dst, uint64_t obj_size,
                                uint64_t stride, uint64_t n_objs, uint64_t dedup,
                                uint32_t f_num, uint32_t f_den, uint64_t seed_base,
                                uint64_t first_obj, void *stream);
/* Mixed-size batch.  `descs` is a host array; it is consumed before return
 * (in sub-batches whose preparation overlaps the previous sub-batch's fill).
 * Descriptors are checked per sub-batch: when one is invalid the call fails
 * and the objects of earlier sub-batches may already be enqueued. */
int s3dg_fill_controlled_batch(s3dg_ctx *ctx, void *dst_base,
                               const s3dg_obj_desc *descs, uint64_t n, void *stream);
/* Keystream fill (generate_npz_bytes_raw x-fill, src/data_formats/npz.rs:376-383):
 * chunk k (chunk_bytes, last one ragged) of [dst, dst+len) =
 * Xoshiro256PlusPlus::seed_from_u64(seed_base + k).fill_bytes(chunk).
 * chunk_bytes: positive multiple of 128 (npz.rs uses 2 MiB). */
int s3dg_xoshiro_fill(s3dg_ctx *ctx, void *dst, uint64_t len, uint64_t chunk_bytes,
                      uint64_t seed_base, void *stream);
/* dgen-contract object ("DG1"): 1 MiB blocks [blk_lo, blk_hi) of
 * an obj_size-byte object, block blk_lo at dst.  Block i = Xoshiro256++ seeded
 * seed ^ ((i % U) * 0x9E3779B97F4A7C15) (U = s3dg_unique_blocks), its first
 * floor(L * f_num / f_den) bytes zero.  Behind DataGenerator/ObjectGen
 * (src/data_gen.rs:253-371) and dgen's generate_data; parity unpinned. */
int s3dg_dgen_fill(s3dg_ctx *ctx, void *dst, uint64_t obj_size, uint64_t blk_lo,
                   uint64_t blk_hi, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                   uint64_t seed, void *stream);
/* n_objs DG1 objects of obj_size bytes in one launch: object j at
 * dst + j*stride, seeded s3dg_object_entropy(seed_base, first_obj + j), i.e.
 * the bytes of n_objs s3dg_dgen_fill calls (ObjectGen / DataGenerator fanned
 * out over many objects).  stride >= obj_size, 16-byte aligned. */
int s3dg_dgen_fill_stream(s3dg_ctx *ctx, void *dst, uint64_t obj_size, uint64_t stride,
                          uint64_t n_objs, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                          uint64_t seed_base, uint64_t first_obj, void *stream);
/* Host helper: advance a Xoshiro256 state by n steps with the jump polynomial
 * the kernels use (test/diagnostic; no GPU needed). */
int s3dg_xoshiro_jump(uint64_t *state4, uint64_t n);
/* Write-only ceiling: fill `len` bytes with a constant using the same store
 * path (roofline denominator measured on the device). */
int s3dg_write_ceiling(s3dg_ctx *ctx, void *dst, uint64_t len, uint32_t pattern,
                       void *stream);
/* The same in the tiled fill shape (batch launch knobs, trailing loads of
 * the context's tile-map records, as k_fill_batch): the ceiling for tiled
 * batches and streams. */
int s3dg_write_ceiling_tiled(s3dg_ctx *ctx, void *dst, uint64_t len, uint32_t pattern, void *stream);
/* The store-only reference of the tiled fill itself: the launch
 * s3dg_fill_controlled_stream makes for len bytes of 8 MiB objects (same
 * tile records, grid, LDS image, barrier, stores and trailing record loads)
 * with the PRNG chain and the window patches compiled out.  Its bytes are
 * meaningless; it is the write ceiling the fill is measured against.
 * pace > 0 makes wave 0 of every workgroup idle pace x 128 cycles where the
 * fill plans its block (store issue paced like the fill's).
 * len < 8 MiB or a multiple of 8 MiB. */
int s3dg_write_ceiling_fill(s3dg_ctx *ctx, void *dst, uint64_t len, uint32_t pace, void *stream);

/* ---- device-resident verification (synchronous on `stream`) -------------- */
/* The read-side twins of the s3dg_fill_* calls above (4 KiB-block layouts):
 * the GPU recomputes every block from (size, dedup, f_num/f_den, entropy, base
 * block) and compares it with the bytes at `src`; nothing is written to `src`,
 * and no byte at or past an object's end (stride gaps included) is read.
 * Arguments, alignment rules (16-byte `src` and `stride`) and S3DG_EINVAL
 * cases are those of the matching fill call; a null `out` is S3DG_EINVAL.
 * Each call enqueues on `stream`, waits for it and fills *out; a zero-length
 * call launches nothing and returns {0, 0, UINT64_MAX}.  Calls on different
 * streams of one context share no state. */
typedef struct {
    uint64_t mismatched_bytes;   /* bytes that differ from the expected payload */
    uint64_t mismatched_blocks;  /* 4 KiB blocks (per object) holding at least one */
    uint64_t first_offset;       /* lowest differing byte offset from `src`
                                    (stride gaps included); UINT64_MAX = none */
} s3dg_verify_result;
int s3dg_verify_controlled(s3dg_ctx *ctx, const void *src, uint64_t len, uint64_t dedup,
                           uint32_t f_num, uint32_t f_den, uint64_t entropy, void *stream,
                           s3dg_verify_result *out);
/* Blocks [blk_lo, blk_hi) of one `len`-byte object, block blk_lo at src. */
int s3dg_verify_controlled_range(s3dg_ctx *ctx, const void *src, uint64_t len, uint64_t blk_lo,
                                 uint64_t blk_hi, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                                 uint64_t entropy, void *stream, s3dg_verify_result *out);
int s3dg_verify_random_data(s3dg_ctx *ctx, const void *src, uint64_t len, uint64_t entropy,
                            void *stream, s3dg_verify_result *out);
int s3dg_verify_controlled_stream(s3dg_ctx *ctx, const void *src, uint64_t obj_size, uint64_t stride,
                                  uint64_t n_objs, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                                  uint64_t seed_base, uint64_t first_obj, void *stream,
                                  s3dg_verify_result *out);
/* Read-side twin of s3dg_fill_controlled_batch: object k of `descs` (its
 * dst_off read as the byte offset of the object from src_base) is recomputed
 * from (size, dedup, f_num/f_den, entropy, base block) and compared with the
 * bytes in memory.  Synchronous on `stream`.  Nothing is written to the payload;
 * no byte at or past an object's end is read.
 *
 * *out (totals; required): mismatched_bytes and mismatched_blocks are summed
 * over the objects, blocks being 4 KiB blocks counted within each object;
 * first_offset is the lowest differing byte offset from src_base over all
 * objects, whatever order the descriptors come in (UINT64_MAX = none).
 *
 * per_obj (host array of n, or NULL): per_obj[k] holds the same three fields
 * for the caller's descriptor k, first_offset counted from that object's first
 * byte.  An empty object (size == 0) is clean: {0, 0, UINT64_MAX}.
 *
 * Descriptors are independent of each other: they may come in any order, leave
 * gaps and overlap.  Two descriptors over the same bytes are two checks, and a
 * byte that is wrong for both counts twice in the totals.  Empty objects are
 * allowed anywhere in the array.
 *
 * Refusals (S3DG_EINVAL, each with a message; nothing is enqueued after the
 * refusal is found): a null `out` ("null output"); null `descs` with n > 0
 * ("null descriptor array"); a null or not 16-byte aligned src_base; and the
 * fill's rules for each non-empty descriptor with the fill's messages
 * ("dst_off must be a multiple of 16", "need f_num < f_den", "object larger
 * than 2^31 blocks"), the first offending descriptor naming the refusal.
 * f_den == 0, the random-data layout, is refused here as the fill's batch
 * refuses it.  Unlike the fill, the call validates all descriptors before the
 * first launch: a refused call has read nothing, and `out` and `per_obj` are
 * written only on success.
 *
 * n == 0, or all objects empty, launches nothing and is clean.  Calls on
 * different streams of one context share no state; two threads on two streams
 * are safe.  Waves per block follow s3dg_set_waves_per_block (auto: 2, as the
 * other verify calls); tiles follow s3dg_set_batch_tile for 2..64 blocks
 * (otherwise 8..64 blocks, chosen per sub-batch).  Results are identical. */
int s3dg_verify_controlled_batch(s3dg_ctx *ctx, const void *src_base,
                                 const s3dg_obj_desc *descs, uint64_t n, void *stream,
                                 s3dg_verify_result *out,       /* totals; required */
                                 s3dg_verify_result *per_obj);  /* host array of n, or NULL */
/* The read-side twins of s3dg_xoshiro_fill / s3dg_dgen_fill /
 * s3dg_dgen_fill_stream (the keystream layouts: the npz x-fill and DG1), under
 * the same rules as the calls above: the GPU regenerates each chunk's keystream
 * (seed, jump, draws, the 1-4-byte tail draw, DG1's zero prefix) with the
 * fill's own code and compares it with `src`; no store, and no byte of a
 * stride gap or past the last object is read.  Arguments, seeds and
 * S3DG_EINVAL cases are the fill's (16-byte aligned `src` and `stride`,
 * f_num < f_den, at most 2^32 blocks, overlapping strides refused); an empty
 * input or block range launches nothing and is clean.  mismatched_blocks
 * counts 4 KiB granules aligned within each object (xoshiro: within the
 * buffer), so the struct reads the same for every layout.
 * One difference from the fill: s3dg_verify_xoshiro needs chunk_bytes to be a
 * positive multiple of 4096 (every chunk then starts on a granule; the npz
 * fill's chunks are 2 MiB) and refuses other values with S3DG_EINVAL, where
 * s3dg_xoshiro_fill takes any multiple of 128. */
int s3dg_verify_xoshiro(s3dg_ctx *ctx, const void *src, uint64_t len, uint64_t chunk_bytes,
                        uint64_t seed_base, void *stream, s3dg_verify_result *out);
int s3dg_verify_dgen(s3dg_ctx *ctx, const void *src, uint64_t obj_size, uint64_t blk_lo, uint64_t blk_hi,
                     uint64_t dedup, uint32_t f_num, uint32_t f_den, uint64_t seed, void *stream,
                     s3dg_verify_result *out);
int s3dg_verify_dgen_stream(s3dg_ctx *ctx, const void *src, uint64_t obj_size, uint64_t stride,
                            uint64_t n_objs, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                            uint64_t seed_base, uint64_t first_obj, void *stream,
                            s3dg_verify_result *out);

/* ---- a mixed-size batch of DG1 objects in one call ------
 * The DG1 forms of s3dg_fill_controlled_batch / s3dg_verify_controlled_batch.
 * s3dg_obj_desc is read for DG1: dst_off = the object's byte offset from the
 * base pointer (a multiple of 16); size = its bytes; entropy = its DG1 seed,
 * the `seed` argument of s3dg_dgen_fill (s3dg_dgen_fill_stream's object j:
 * s3dg_object_entropy(seed_base, j)); dedup: U = s3dg_unique_blocks(ceil(size /
 * 1 MiB), dedup), per object; f_num / f_den: the zero prefix of every 1 MiB
 * block, floor(L * f_num / f_den).
 *
 * s3dg_dgen_fill_batch: object k's bytes are exactly those of
 * s3dg_dgen_fill(ctx, dst_base + dst_off, size, 0, ~0, dedup, f_num, f_den,
 * entropy, stream).  Asynchronous and stream-ordered; `descs` is consumed
 * before return.  Nothing outside the objects is written: no gap byte, nothing
 * past an object's end.  Overlapping destinations are the caller's business.
 *
 * s3dg_verify_dgen_batch finds what s3dg_verify_dgen finds on the same bytes,
 * under s3dg_verify_controlled_batch's rules: synchronous on `stream`; nothing
 * is written to the payload and no byte at or past an object's end is read;
 * descriptors may come in any order, leave gaps, overlap and repeat, and empty
 * objects are allowed anywhere.  *out (totals; required) sums
 * mismatched_bytes and mismatched_blocks over the descriptors (a byte that is
 * wrong for two descriptors counts twice), blocks being 4 KiB granules aligned
 * within each object; first_offset is the lowest differing offset from
 * src_base.  per_obj (host array of n, or NULL): the same for descriptor k,
 * first_offset counted from that object's first byte; an empty object is clean,
 * {0, 0, UINT64_MAX}.  `out` and `per_obj` are written only on success.
 *
 * Both calls check every descriptor before the first launch, so a refused
 * call has written or read nothing.  Refusals (S3DG_EINVAL, each with a
 * message): a null `out` of the verify ("null output"); null `descs` with
 * n > 0 ("null descriptor array"); a null or not 16-byte aligned base pointer
 * ("dst_base / src_base must be 16-byte aligned"); and for the first offending
 * non-empty descriptor k, "object k: " followed by "dst_off must be a multiple
 * of 16", "need f_num < f_den" (f_den == 0 included) or "object larger than
 * 2^32 blocks".  n == 0, or only empty objects, launches nothing and succeeds.
 * Calls on different streams of one context share no state; two threads on two
 * streams are safe.  The lanes follow s3dg_set_keystream_shape(mode 1) as the
 * other DG1 calls do; the bytes and the results do not depend on it. */
int s3dg_dgen_fill_batch(s3dg_ctx *ctx, void *dst_base,
                         const s3dg_obj_desc *descs, uint64_t n, void *stream);
int s3dg_verify_dgen_batch(s3dg_ctx *ctx, const void *src_base,
                           const s3dg_obj_desc *descs, uint64_t n, void *stream,
                           s3dg_verify_result *out,       /* totals; required */
                           s3dg_verify_result *per_obj);  /* host array of n, or NULL */

/* ---- measurement (read-only) ------------------------------
 * What a payload is worth to a store that deduplicates and compresses at
 * `block_bytes`: how many of its blocks are distinct and how many of its bytes
 * are zero, the two ratios the reference's own tests compute on the CPU with a
 * HashSet of blocks (tests/test_data-gen.rs:84-215).  No seed is needed, so
 * unseeded output and data read back from a store can be measured too.
 *
 * Each object is cut into blocks of block_bytes from its own start; an
 * object's last block may be ragged, and a ragged block never equals a full
 * one (bytes and length are compared, as a HashSet<Vec<u8>> would).  Blocks
 * are compared through 128-bit fingerprints: unique_blocks is the exact
 * number of distinct fingerprints, and two different blocks share one with
 * probability about 2^-64 per pair for data that was not built against the
 * (public, fixed) keys.
 *
 * A handle accumulates: every add on any stream adds to one result, so data
 * that passes through a ring in several launches or arrives in chunks is
 * measured as one payload.  block_bytes: a positive multiple of 4096, at most
 * 2^30.  flags: 0 or S3DG_MEASURE_HIST (a byte histogram, a second read of
 * the same bytes).  Device memory per measured block: a 16-byte fingerprint
 * in an array that grows by doubling, plus, while s3dg_measure_get runs, a
 * 32-byte sort copy and hipCUB's radix-sort scratch (about 16 bytes more);
 * per add and stream, 20 bytes per 4 KiB of the add as scratch.  Growing the
 * array waits for the adds the handle has enqueued, on all their streams.
 * The read pass runs 1, 2 or 4 wave64s per 4 KiB after
 * s3dg_set_waves_per_block (auto: 1); results are identical.
 * Destroy a handle before its context. */
enum { S3DG_MEASURE_HIST = 1 };
typedef struct s3dg_measure s3dg_measure;
typedef struct {
    uint64_t bytes;          /* payload bytes measured (stride gaps excluded) */
    uint64_t zero_bytes;
    uint64_t blocks;         /* blocks measured, ragged last blocks included */
    uint64_t unique_blocks;  /* distinct among them (bytes and length) */
    uint64_t hist[256];      /* byte histogram; all 0 without S3DG_MEASURE_HIST */
} s3dg_measure_result;
int s3dg_measure_create(s3dg_ctx *ctx, uint64_t block_bytes, int flags, s3dg_measure **out);
int s3dg_measure_destroy(s3dg_measure *m);
int s3dg_measure_reset(s3dg_measure *m);   /* waits for the enqueued adds; an empty handle again */
/* n_objs objects of obj_size bytes at src + j*stride (device memory; src and
 * stride 16-byte aligned, stride >= obj_size: the refusals of
 * s3dg_verify_controlled_stream).  Asynchronous on `stream` and ordered like a
 * fill: a later launch on the same stream may overwrite src.  Stride gaps and
 * whatever follows the last object are never read.  Fingerprint slots are
 * reserved on the host at call time, so adds from several threads on several
 * streams are safe.  A zero-length add launches nothing. */
int s3dg_measure_add_stream(s3dg_measure *m, const void *src, uint64_t obj_size, uint64_t stride,
                            uint64_t n_objs, void *stream);
/* Blocks [blk_lo, blk_hi) of one obj_size-byte object, in units of
 * block_bytes, block blk_lo at src (blk_hi is clipped to the object): one
 * large object passing through a smaller buffer. */
int s3dg_measure_add_range(s3dg_measure *m, const void *src, uint64_t obj_size,
                           uint64_t blk_lo, uint64_t blk_hi, void *stream);
/* Waits for the enqueued adds, counts the distinct fingerprints on a copy
 * and fills *out.  The handle is unchanged: get again, or add and get.  An
 * empty handle yields all zeros. */
int s3dg_measure_get(s3dg_measure *m, s3dg_measure_result *out);
/* A mixed-size batch in one add: span k is one object of
 * `size` bytes at src_base + off, measured from its own first byte.  The
 * handles of the three read-only analyses take it:
 *   s3dg_measure_add_batch  adds exactly the sum over k of
 *                           s3dg_measure_add_range(src_base + off_k, size_k, 0, all blocks),
 *   s3dg_lz_add_batch       the same sum of s3dg_lz_add_range,
 *   s3dg_chunks_add_batch   the sum of s3dg_chunks_add_stream(src_base + off_k, size_k, size_k, 1).
 * Blocks and chunks never cross objects; a ragged last block is finalised
 * with its length.  unique_* stays exact over everything the handle has seen:
 * batch adds, stream adds and range adds mixed.
 * Layout (as s3dg_verify_controlled_batch): spans may come in any order, leave
 * gaps, overlap and repeat.  Two spans over the same bytes are two objects:
 * bytes and blocks (chunks) count twice, unique_* does not.  Empty spans
 * (size == 0) are allowed anywhere, whatever their off, and contribute
 * nothing: no block, no chunk, no slot.
 * Reading: a 16-byte piece is loaded whole only when it ends at or below its
 * object's length, the ragged piece byte by byte; no byte of a gap is ever
 * read, nor any byte before src_base + off or at or past off + size.
 * Asynchronous on `stream` and ordered like s3dg_*_add_stream: a later launch
 * on the same stream may overwrite the payload.  `spans` is consumed before
 * the call returns: the caller may free or rewrite it at once.  Slots and
 * scratch are reserved on the host under the handle's mutex, so adds from
 * several threads on several streams are safe.  Per add and stream the table
 * of the spans is built on the host and uploaded: 40 bytes per non-empty span
 * and 32 bytes per tile of 2..64 4 KiB granules of an object (the tile size
 * follows s3dg_set_batch_tile as in the batch verify; results are identical at
 * every size), in pinned host memory and in device memory.
 * Refusals (S3DG_EINVAL, each with its message; every span is checked before
 * anything is reserved or enqueued, so a refused add leaves the handle exactly
 * as it was): a null handle; null `spans` with n > 0 ("null span array"); a
 * null or not 16-byte aligned src_base; a non-empty span whose off is not a
 * multiple of 16 ("off must be a multiple of 16") or which is larger than
 * 2^31 x 4096 bytes ("object larger than 2^31 blocks"), the message naming
 * the first offending index ("span 7: ..."); more than 2^40 granules or
 * 2^31 - 1 chunk slots in one add, and the handles' own caps with their
 * messages.  n == 0, or only empty spans, launches nothing and is accepted
 * whatever src_base.
 * A handle created with S3DG_MEASURE_HIST takes the histogram of the spans'
 * bytes too. */
typedef struct {
    uint64_t off;    /* bytes from src_base */
    uint64_t size;   /* bytes */
} s3dg_span;
int s3dg_measure_add_batch(s3dg_measure *m, const void *src_base, const s3dg_span *spans, uint64_t n,
                           void *stream);
/* A host buffer (any alignment, read-only memory included) as one object,
 * on a host slot's GPU: copied in chunks of whole blocks (up to 64 MiB; one
 * block per chunk, in two buffers of the call's own, when block_bytes is
 * larger) on the slot's two streams, each chunk an s3dg_measure_add_range.
 * len == 0: all zeros, no GPU needed. */
int s3dg_measure_data(const uint8_t *buf, uint64_t len, uint64_t block_bytes, int flags,
                      s3dg_measure_result *out);

/* ---- content-defined chunking (read-only) -----------------
 * What a payload is worth to a store that deduplicates content-defined
 * chunks (backup targets, most deduplicating object stores): a rolling hash
 * over a 32-byte window picks the cut points between min_bytes and max_bytes,
 * so equal content is found at any byte offset.  The fixed-block measure above
 * cannot answer for such a store.
 *
 * Every object is chunked on its own, from its first byte; no window reaches
 * outside the object.  With G[b] = lowbias32(b + 0x9E3779B9) and bits =
 * log2(avg_bytes), position i >= 31 of an object is a candidate cut when
 * h_i = sum over k in [0, 32) of G[byte[i - k]] << k (mod 2^32) has its top
 * `bits` bits zero.  A chunk that starts at s ends at the first candidate
 * e >= s + min_bytes - 1 if that makes it at most max_bytes long; otherwise it
 * is cut at max_bytes (a forced cut); the object's end closes the last chunk
 * at whatever length it has (not a forced cut, unless the chunk has exactly
 * max_bytes and does not end on a candidate).  min_bytes == max_bytes is
 * fixed blocks.  Chunks are compared through the measure's 128-bit
 * fingerprints (the pieces counted from the chunk's first byte, the length
 * folded in), so a chunk with the bytes of a block has that block's
 * fingerprint; unique_chunks is the exact number of distinct fingerprints.
 *
 * avg_bytes: a power of two from 64 to 2^24; 32 <= min_bytes <= max_bytes <=
 * 2^30; neither need be a multiple of anything.  Usual values: 2048 / 8192 /
 * 65536.
 *
 * A handle accumulates over adds on any stream, so objects that pass through
 * a ring in several launches count as one payload.  Out of scope: block
 * ranges of one object across adds (the walk's state, the start of the open
 * chunk and its partial fingerprint, would have to be carried between them);
 * every add holds whole objects.
 *
 * Device memory.  Per add and stream, as scratch that is reused: the
 * candidate bitmap, 1/8 of the add's bytes (and 4 bytes per 4 KiB for the
 * candidate counts), and 12 bytes of (offset, length) per record slot, ceil(obj_size / min_bytes) + 1 slots per object.  In the
 * handle: 20 bytes (fingerprint and length) per record slot of every add, in
 * arrays that grow by doubling, plus, while s3dg_chunks_get runs, 24 bytes of
 * sort keys and indices per slot and hipCUB's radix-sort scratch.  Slots are
 * reserved for the most chunks an object can have, so a handle holds at most
 * 2^31 - 1 of them: about 4 TiB of payload at min_bytes 2048, 64 GiB at 32.
 * Growing the arrays waits for the adds the handle has enqueued.  One wave
 * walks each object's cuts and one wave fingerprints each chunk, so the passes
 * are parallel over objects and chunks, not inside one.
 * Destroy a handle before its context. */
typedef struct s3dg_chunks s3dg_chunks;
typedef struct {
    uint64_t bytes;          /* payload bytes chunked (stride gaps excluded) */
    uint64_t chunks;         /* chunks cut, every object's last one included */
    uint64_t unique_chunks;  /* distinct among them (bytes and length) */
    uint64_t unique_bytes;   /* summed length of one chunk per distinct fingerprint */
    uint64_t candidates;     /* positions whose window hash passes */
    uint64_t forced_cuts;    /* chunks cut at max_bytes without a candidate */
} s3dg_chunk_result;
int s3dg_chunks_create(s3dg_ctx *ctx, uint64_t min_bytes, uint64_t avg_bytes, uint64_t max_bytes,
                       s3dg_chunks **out);
int s3dg_chunks_destroy(s3dg_chunks *h);
int s3dg_chunks_reset(s3dg_chunks *h);   /* waits for the enqueued adds; an empty handle again */
/* n_objs objects of obj_size bytes at src + j*stride (device memory; the
 * refusals of s3dg_measure_add_stream).  Asynchronous on `stream` and ordered
 * like a fill: a later launch on the same stream may overwrite src.  Stride
 * gaps, the bytes before src and whatever follows the last object are never
 * read.  Slots and scratch are reserved on the host at call time, so adds from
 * several threads on several streams are safe.  A zero-length add launches
 * nothing. */
int s3dg_chunks_add_stream(s3dg_chunks *h, const void *src, uint64_t obj_size, uint64_t stride,
                           uint64_t n_objs, void *stream);
/* A mixed-size batch in one add: the contract of s3dg_measure_add_batch.  Every
 * span is chunked on its own from its first byte; the add equals the sum of
 * s3dg_chunks_add_stream(src_base + off_k, size_k, size_k, 1) over the spans.
 * A span takes ceil(size / min_bytes) + 1 record slots. */
int s3dg_chunks_add_batch(s3dg_chunks *h, const void *src_base, const s3dg_span *spans, uint64_t n,
                          void *stream);
/* Waits for the enqueued adds, counts the distinct fingerprints on a copy and
 * fills *out.  The handle is unchanged: get again, or add and get.  An empty
 * handle yields all zeros. */
int s3dg_chunks_get(s3dg_chunks *h, s3dg_chunk_result *out);
/* Diagnostics.  S3DG_CHUNKS_TIME_PASSES (0 / 1, default 0): HIP events around
 * the three passes of every following add; s3dg_chunks_pass_seconds waits for
 * the latest such add and writes its candidate, cut and fingerprint pass times
 * to seconds[0..2].  S3DG_CHUNKS_GEAR_TABLE (0 / 1, default 1): the candidate
 * pass reads G from 256 words of LDS or computes it per byte; results are
 * identical. */
enum { S3DG_CHUNKS_TIME_PASSES = 1, S3DG_CHUNKS_GEAR_TABLE = 2 };
int s3dg_chunks_set_option(s3dg_chunks *h, int option, int value);
int s3dg_chunks_pass_seconds(s3dg_chunks *h, double *seconds);
/* A host buffer (any alignment, read-only memory included) as one object, on
 * a host slot's GPU.  Windows and chunks cross any copy's edge, so the whole
 * buffer is staged in device memory (len rounded up to 16 bytes, copied 64 MiB
 * at a time); a buffer that does not fit is an error with hipMalloc's text.
 * len == 0: all zeros, no GPU needed. */
int s3dg_chunk_data(const uint8_t *buf, uint64_t len, uint64_t min_bytes, uint64_t avg_bytes,
                    uint64_t max_bytes, s3dg_chunk_result *out);

/* ---- LZ4 compressed size per store block (read-only) -------
 * What a payload is worth to a store that compresses independent blocks of
 * `block_bytes`: the bytes it takes after a greedy LZ4 block compressor, the
 * answer to the generator's `compress` knob that zero bytes and byte entropy
 * cannot give (a repeated base block has neither and shrinks twelvefold).  No
 * seed is needed.  Only sizes are computed; the definition is exact, and
 * `size` is the length of a valid LZ4 block for every input.
 *
 * block_bytes: a multiple of 4096 from 4096 to 65536, so every match offset
 * fits LZ4's 16 bits.  Every object is cut into blocks from its first byte;
 * the last block of an object has whatever length n >= 1 remains.  No match
 * reaches outside its block.  For one block b[0..n):
 *  1. For 0 <= i <= n - 4, v(i) is the little-endian u32 at i and
 *     H(i) = (v(i) * 2654435761 mod 2^32) >> 20, 12 bits.
 *  2. Candidates, in groups of 64 positions.  T is a table of 4096 entries,
 *     all empty at first.  For every i <= n - 4, c(i) = T[H(i)] as it stood
 *     before i's group: the greatest j < 64 * (i / 64) with H(j) = H(i), or
 *     none.  After a group's lookups T[h] becomes the greatest i of the group
 *     with H(i) = h.  Every position is entered, those inside a match too.
 *  3. src(i), for i <= n - 12 only (LZ4's last match start): c(i) if it exists
 *     and v(c(i)) = v(i); otherwise i - 1 if i >= 1 and v(i - 1) = v(i) (a run
 *     of five equal bytes); otherwise none.  Blocks with n < 13 have no match.
 *  4. Greedy parse from anchor = p = 0: take the smallest i >= p with a source
 *     s; L is the largest length with b[s + k] = b[i + k] for k < L and
 *     i + L <= n - 5 (the last five bytes are literals; the source may overlap
 *     the match; L >= 4; no backward extension).  With lit = i - anchor,
 *     size += 1 + ext(lit) + lit + 2 + ext(L - 4), where ext(x) = 0 for
 *     x < 15 and 1 + (x - 15) / 255 otherwise; anchor = p = i + L; repeat.
 *     When no source is left, lit = n - anchor and size += 1 + ext(lit) + lit.
 *
 * A handle accumulates over adds on any stream, like s3dg_measure, and holds
 * eight device words; an add needs no scratch.  One wave compresses one block
 * at a time with the block and the table in LDS (block_bytes + 8 KiB).
 * Out of scope: emitting the compressed bytes; any compressor but this one
 * (zstd's entropy stage would be a second feature); blocks above 64 KiB;
 * matches across blocks or objects; a bench.py config (tools/lz_rate.py
 * times the pass).
 * Destroy a handle before its context. */
typedef struct s3dg_lz s3dg_lz;
typedef struct {
    uint64_t bytes;          /* payload bytes measured (stride gaps excluded) */
    uint64_t blocks;         /* blocks compressed, ragged last blocks included */
    uint64_t lz_bytes;       /* sum of size */
    uint64_t stored_bytes;   /* sum of min(size, n): a store keeps a block raw when compression does not pay */
    uint64_t raw_blocks;     /* blocks with size >= n */
    uint64_t matches;
    uint64_t match_bytes;    /* sum of L */
    uint64_t literal_bytes;  /* literal_bytes + match_bytes == bytes */
} s3dg_lz_result;
int s3dg_lz_create(s3dg_ctx *ctx, uint64_t block_bytes, s3dg_lz **out);
int s3dg_lz_destroy(s3dg_lz *h);
int s3dg_lz_reset(s3dg_lz *h);   /* waits for the enqueued adds; an empty handle again */
/* n_objs objects of obj_size bytes at src + j*stride (device memory; the
 * refusals of s3dg_measure_add_stream).  Asynchronous on `stream` and ordered
 * like a fill: a later launch on the same stream may overwrite src.  Stride
 * gaps and whatever follows the last object are never read.  The adds share
 * only the handle's totals, which take atomics, so adds from several threads
 * on several streams are safe.  A zero-length add launches nothing. */
int s3dg_lz_add_stream(s3dg_lz *h, const void *src, uint64_t obj_size, uint64_t stride,
                       uint64_t n_objs, void *stream);
/* Blocks [blk_lo, blk_hi) of one obj_size-byte object, in units of
 * block_bytes, block blk_lo at src (blk_hi is clipped to the object): one
 * large object passing through a smaller buffer.  Blocks are independent, so
 * ranges that add up to the object give the object's result exactly. */
int s3dg_lz_add_range(s3dg_lz *h, const void *src, uint64_t obj_size, uint64_t blk_lo,
                      uint64_t blk_hi, void *stream);
/* A mixed-size batch in one add: the contract of s3dg_measure_add_batch.  Every
 * span is cut into blocks from its own first byte; the add equals the sum of
 * s3dg_lz_add_range(src_base + off_k, size_k, 0, all blocks) over the spans. */
int s3dg_lz_add_batch(s3dg_lz *h, const void *src_base, const s3dg_span *spans, uint64_t n, void *stream);
/* Waits for the enqueued adds and fills *out.  The handle is unchanged: get
 * again, or add and get.  An empty handle yields all zeros. */
int s3dg_lz_get(s3dg_lz *h, s3dg_lz_result *out);
/* A host buffer (any alignment, read-only memory included) as one object, on
 * a host slot's GPU: copied in chunks of whole blocks (up to 64 MiB) on the
 * slot's two streams in turn, each chunk an s3dg_lz_add_range.
 * len == 0: all zeros, no GPU needed. */
int s3dg_lz_data(const uint8_t *buf, uint64_t len, uint64_t block_bytes, s3dg_lz_result *out);

/* ---- memory / copy helpers ------------------------------------------------ */
int s3dg_device_alloc(s3dg_ctx *ctx, uint64_t bytes, void **out);
int s3dg_device_free(s3dg_ctx *ctx, void *p);
int s3dg_host_alloc_pinned(uint64_t bytes, void **out);
/* Pinned host memory placed on `device`'s NUMA node (allocated from a thread
 * bound to the GPU's local CPUs; falls back to default placement when sysfs
 * does not say).  Free with s3dg_host_free_pinned. */
int s3dg_host_alloc_pinned_local(int device, uint64_t bytes, void **out);
int s3dg_host_free_pinned(void *p);
/* Page-lock a caller's pageable buffer [buf, buf+len) (hipHostRegister, whole
 * 4 KiB pages) so that host-buffer calls inside it (s3dlio_fill_controlled_data
 * and the other host entry points; whole 4 KiB blocks, 16-byte aligned, up to
 * 16 MiB) are written by the kernel directly, as s3dg_host_alloc_pinned memory
 * (1 MiB: ~33 us against ~57 us through the bounce path).  Registrations that
 * overlap the range are dropped first; registering the same range again is a
 * no-op.  0 or a negative S3DG_E* status.
 * CONTRACT (hipHostRegister's): the buffer stays allocated until
 * s3dg_host_unregister.  Unmapped while registered, its GPU mapping goes with
 * its pages and the next call into it is a GPU memory fault.  The bindings
 * hold the buffer for the registration's lifetime (Python:
 * s3dlio_amd.register_host_buffer keeps an export of it; Rust:
 * HostRegistration<'a> borrows the slice).  Register a range
 * while no other thread's call is writing into it.
 * Replaces round 5's S3DLIO_HOST_REGISTER=1 sighting rule, which registered
 * buffers their owners did not know about. */
int s3dg_host_register(void *buf, uint64_t len);
/* Release the registration holding `buf` (NULL: every registration), after
 * calls still writing into it return.  Returns the number released (>= 0).
 * A call whose range overlaps a registration without lying inside it also
 * releases that registration (HIP cannot copy into a partly registered range). */
int s3dg_host_unregister(void *buf);
/* NUMA node of `device` from sysfs (-1 when unknown). */
int s3dg_device_numa_node(int device, int *node);
int s3dg_d2h_async(s3dg_ctx *ctx, void *host, const void *dev, uint64_t len, void *stream);
int s3dg_h2d_async(s3dg_ctx *ctx, void *dev, const void *host, uint64_t len, void *stream);
int s3dg_stream_create(s3dg_ctx *ctx, void **out);
int s3dg_stream_destroy(s3dg_ctx *ctx, void *stream);
/* Release the context's per-stream launch state (tile maps, batch staging) of
 * `stream`, after draining it: call before destroying a stream the context has
 * launched on, so short-lived streams do not accumulate device memory.
 * s3dg_stream_destroy does this itself.  No-op for an unknown stream.  A
 * launch on `stream` from another thread may race with the release: it
 * completes, and the last holder of the state drains the stream and frees it.
 * s3dg_stream_destroy must not run while another thread still uses `stream`
 * (the HIP stream itself is destroyed, even when the drain reports an error). */
int s3dg_stream_release(s3dg_ctx *ctx, void *stream);
int s3dg_stream_state_count(s3dg_ctx *ctx, uint64_t *n);
int s3dg_sync(s3dg_ctx *ctx, void *stream);   /* stream NULL: whole device */
int s3dg_device_count(int *out);

/* ---- CRC-32 and NPZ (src/data_formats/npz.rs:322-434) --------------------- */
/* CRC-32 (IEEE, crc32fast / zlib.crc32) of dev[0, len); synchronous on `stream`. */
int s3dg_crc32(s3dg_ctx *ctx, const void *dev, uint64_t len, void *stream, uint32_t *out);
/* The CRC-32 of every object of a mixed-size batch in one call (DESIGN.md
 * §5.4.1): crcs[k] is s3dg_crc32's value for the size_k bytes at
 * src_base + off_k, the checksum every writer hands back with its object; an
 * empty span gives 0, whatever its off.  Regions, tails and the fold of an
 * object's regions all run on the device: one launch over the regions of all
 * objects, one over the objects.
 * Layout (as s3dg_measure_add_batch): spans may come in any order, leave gaps,
 * overlap and repeat; a repeated span gives the same value twice.  off of a
 * non-empty span is a multiple of 16, size anything up to 2^31 x 4096.
 * Reading: a 16-byte piece is loaded whole only when it ends at or below its
 * object's end, the ragged piece byte by byte; no byte of a gap is ever read,
 * nor any byte before src_base + off or at or past off + size.  Nothing is
 * written to the payload.
 * s3dg_crc32_batch_async is ordered on `stream` and returns without waiting:
 * `spans` is consumed before it returns, crcs_dev is device memory or pinned
 * host memory of n values, all of which are written in stream order (those of
 * empty spans as zeros); there is no copy back and no wait in it.
 * s3dg_crc32_batch is that into scratch of the stream's, one copy of 4 n bytes
 * into the host array crcs and one wait.  The table of a call (32 bytes per
 * non-empty span, 24 per region of 32 KiB or more) and its scratch belong to
 * the stream: calls on different streams of one context share nothing that
 * changes, so threads on different streams need no lock of their own.
 * Refusals (S3DG_EINVAL; every span is checked before anything is reserved or
 * enqueued, so a refused call has read nothing and written nothing to crcs):
 * "null context", "null output", and s3dg_measure_add_batch's for the spans,
 * with its messages.  n == 0 succeeds whatever the other pointers. */
int s3dg_crc32_batch(s3dg_ctx *ctx, const void *src_base, const s3dg_span *spans, uint64_t n, void *stream,
                     uint32_t *crcs);
int s3dg_crc32_batch_async(s3dg_ctx *ctx, const void *src_base, const s3dg_span *spans, uint64_t n, void *stream,
                           uint32_t *crcs_dev);
/* ---- TFRecord shards framed and checked on the device ----
 * Shard k is `records` records of `record_size` payload bytes.  Its framed
 * stream is byte-identical to build_tfrecord_with_index(records, record_size,
 * payload) (src/data_formats/tfrecord.rs:10-75): record i is
 *   u64 len | masked_crc(len) | data | masked_crc(data)
 * at i * (16 + record_size), and its index entry is <u64 i * (16 + record_size),
 * u64 16 + record_size>.  record_size == 0 is a valid 16-byte record.  One
 * kernel hashes and, in the frame form, copies every record; a record of more
 * than one region (32 KiB or more) is finished by a second, small launch.
 * The whole-file checksum of a shard is s3dg_crc32_batch over its dst span. */
typedef struct {
    uint64_t src_off;      /* payload: records * record_size bytes at src_base + src_off */
    uint64_t dst_off;      /* framed stream: records * (16 + record_size) bytes at dst_base + dst_off */
    uint64_t idx_off;      /* index: 16 * records bytes at idx_base + idx_off (unused when idx_base is NULL) */
    uint64_t records;
    uint64_t record_size;
} s3dg_tfrecord_shard;
typedef struct {
    uint64_t records;          /* records looked at */
    uint64_t bad_records;      /* records with at least one of the three below */
    uint64_t bad_length;       /* length field differs from record_size */
    uint64_t bad_length_crc;   /* length CRC differs from masked_crc of record_size's 8 bytes */
    uint64_t bad_data_crc;     /* footer differs from masked_crc of the record's data */
    uint64_t first_shard;      /* caller's index of the first shard with a bad record; UINT64_MAX when clean */
    uint64_t first_record;     /* the lowest bad record of that shard; UINT64_MAX when clean */
} s3dg_tfrecord_result;
/* records * (16 + record_size); S3DG_EINVAL when that overflows or out is null. */
int s3dg_tfrecord_size(uint64_t records, uint64_t record_size, uint64_t *out);
/* Frames every shard of the list in one call.  Ordered on `stream`, returns
 * without a wait; `shards` is consumed before it returns.  Shards may come in
 * any order and may be empty (records == 0: nothing is looked at or written);
 * two shards may share a source.  src_base, dst_base and idx_base (nullable:
 * no index) are 16-byte aligned device pointers; src_off, dst_off and idx_off
 * are multiples of 16.
 * Writes exactly the bytes of each stream and each index: no byte before
 * dst_off, none at or past the stream's ragged end (a neighbour may start 16
 * bytes later), and every byte once.  Reads no source byte outside
 * [src_off, src_off + records * record_size).  Destination streams must not
 * overlap each other or any source span (the caller's contract); overlap of a
 * shard's own source and stream is refused.
 * Refusals (S3DG_EINVAL, each with a message; every descriptor is checked
 * before anything is reserved or enqueued, so a refused call has read and
 * written nothing): "null context", a null or misaligned base, "null shard
 * array", and per shard ("shard k: ...") an offset that is no multiple of 16,
 * record_size above 2^31 x 4096, records * (16 + record_size) or an end
 * address overflowing, more than 2^46 framed bytes in one call.  n == 0
 * succeeds whatever the other pointers. */
int s3dg_tfrecord_frame_batch(s3dg_ctx *ctx, const void *src_base, void *dst_base, void *idx_base,
                              const s3dg_tfrecord_shard *shards, uint64_t n, void *stream);
/* The read-side twin over the same descriptors: dst_off, records and
 * record_size are used, the stream is at base + dst_off.  Synchronous on
 * `stream`; writes nothing to the streams, and a clean stream costs no store
 * and no atomic.  Per record: the length field against record_size, the
 * length CRC against record_size's, the data's CRC against the footer; a
 * descriptor whose record_size is not the stream's shows as bad_length.
 * total (required) sums the shards, with the first bad shard by the caller's
 * index; per_shard (host array of n, or NULL) gets every shard's own result,
 * first_shard being k or UINT64_MAX.  Refusals as above, and "null output". */
int s3dg_tfrecord_check_batch(s3dg_ctx *ctx, const void *base, const s3dg_tfrecord_shard *shards, uint64_t n,
                              void *stream, s3dg_tfrecord_result *total, s3dg_tfrecord_result *per_shard);
/* ---- TFRecord shards of records of any length ----
 * Shard k is `records` records of lengths[len0 .. len0 + records) payload
 * bytes, packed back to back in the source.  With P_i the sum of the lengths
 * before record i, the record is framed at dst_off + P_i + 16 i and its index
 * entry is <u64 P_i + 16 i, u64 16 + len_i>: stream and index are
 * byte-identical to write_raw_record applied record by record
 * (src/data_formats/tfrecord.rs:14-75), and to s3dg_tfrecord_frame_batch for a
 * list of equal lengths.  A length of 0 is a valid 16-byte record. */
typedef struct {
    uint64_t src_off;   /* frame: the shard's payload, records packed back to back, at src_base + src_off */
    uint64_t dst_off;   /* the framed stream at dst_base + dst_off (check: base + dst_off) */
    uint64_t idx_off;   /* frame: 16 bytes per record at idx_base + idx_off (unused when idx_base is NULL) */
    uint64_t records;
    uint64_t len0;      /* the shard's first length: lengths[len0 .. len0 + records) */
} s3dg_tfrecord_var_shard;
/* sum(16 + len) over `records` lengths; S3DG_EINVAL when that overflows, when
 * out is null, or when lengths is null with records present. */
int s3dg_tfrecord_var_size(const uint64_t *lengths, uint64_t records, uint64_t *out);
/* s3dg_tfrecord_frame_batch's contract over such shards: ordered on `stream`,
 * no wait; `shards` and `lengths` (a host array of nlengths) are consumed
 * before it returns.  Shards may come in any order, be empty and share a
 * source.  Writes exactly the bytes of each stream and each index.
 * Refusals: s3dg_tfrecord_frame_batch's, and "null lengths array" with records
 * present, per shard len0 + records beyond nlengths, a record longer than
 * 2^31 x 4096, more than 2^46 framed bytes in one call (which a sum that
 * would overflow exceeds first). */
int s3dg_tfrecord_frame_var_batch(s3dg_ctx *ctx, const void *src_base, void *dst_base, void *idx_base,
                                  const s3dg_tfrecord_var_shard *shards, uint64_t n, const uint64_t *lengths,
                                  uint64_t nlengths, void *stream);
/* s3dg_tfrecord_check_batch's contract over such shards (dst_off, records and
 * len0 are used): synchronous, writes nothing to the streams, a clean stream
 * costs no store and no atomic.  bad_length: the stream's length field
 * differs from the given length. */
int s3dg_tfrecord_check_var_batch(s3dg_ctx *ctx, const void *base, const s3dg_tfrecord_var_shard *shards, uint64_t n,
                                  const uint64_t *lengths, uint64_t nlengths, void *stream, s3dg_tfrecord_result *total,
                                  s3dg_tfrecord_result *per_shard);
/* The index of a framed stream nobody has described: index_entries_from_bytes
 * (src/tfrecord_index.rs:34-80) on the device, for every stream of a list in
 * one call.  Stream k is `bytes` bytes at base + off (any byte offset); its
 * entries <u64 offset from the stream's start, u64 16 + len>, at most
 * max_records of them, go to idx_base + idx_off (a multiple of 16).  The walk
 * stops silently when fewer than 12 bytes are left (status 0), at a record
 * whose 12 + len + 4 bytes do not fit (status 1, stop_offset at that record's
 * start, the entries before it kept), or when max_records entries are written
 * and 12 or more bytes are left (status 2); resume such a walk at off +
 * stop_offset.  The length CRC never changes the index; mismatches are
 * counted beside it. */
typedef struct {
    uint64_t off, bytes, idx_off, max_records;
} s3dg_tfrecord_stream;
typedef struct {
    uint64_t records;          /* complete records found; their entries are written */
    uint64_t status;           /* 0 complete, 1 truncated record, 2 max_records reached */
    uint64_t stop_offset;      /* offset in the stream of the first byte not covered by an entry */
    uint64_t trailing;         /* bytes - stop_offset */
    uint64_t bad_length_crc;   /* records whose length CRC is not masked_crc of their 8 length bytes */
    uint64_t first_bad_record; /* the lowest such record; UINT64_MAX when none */
} s3dg_tfrecord_walk_result;
/* Synchronous on `stream`; results is a host array of n.  One wave follows one
 * stream's chain of length fields.  Refusals (S3DG_EINVAL, before anything is
 * reserved or enqueued): "null context", "null base", "null idx_base", "null
 * results", "null stream array", a misaligned idx_base, more than 2^32 - 1
 * streams, and per stream ("stream k: ...") idx_off no multiple of 16 or an
 * end address overflowing.  n == 0 succeeds whatever the other pointers. */
int s3dg_tfrecord_index_batch(s3dg_ctx *ctx, const void *base, void *idx_base, const s3dg_tfrecord_stream *streams,
                              uint64_t n, void *stream, s3dg_tfrecord_walk_result *results);
/* zlib crc32_combine: CRC of A||B from crc(A), crc(B), |B| (host). */
uint32_t s3dg_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);
/* Host CRC-32 update (crc32fast::Hasher semantics: start from 0). */
uint32_t s3dg_crc32_host(uint32_t crc, const uint8_t *p, uint64_t n);
/* Byte size of generate_npz_bytes_raw(shape, dtype, num_samples). */
int s3dg_npz_size(const uint64_t *shape, int ndim, const char *dtype, uint64_t num_samples,
                  uint64_t *total);
/* generate_npz_bytes_raw into a host buffer of >= s3dg_npz_size bytes:
 * byte-identical archive (x.npy keystream + CRC on the GPU, framing on host). */
int s3dg_npz_build(s3dg_ctx *ctx, const uint64_t *shape, int ndim, const char *dtype,
                   uint64_t num_samples, uint8_t *out, uint64_t out_len);

/* ---- streaming generator (DataGenerator / ObjectGen / PyO3 Generator) ----- */
/* One object of `size` bytes in the DG1 layout, generated on a host slot's
 * GPU (taken round-robin at creation) and streamed into host buffers.  has_seed=0: time + counter
 * entropy like DataGenerator::new(None) (src/data_gen.rs:271-291).
 * compress/dedup 0 are treated as 1 (src/data_gen_alt.rs:108-109). */
typedef struct s3dg_gen s3dg_gen;
int s3dg_gen_create(uint64_t size, uint64_t dedup, uint64_t compress, int has_seed,
                    uint64_t seed, s3dg_gen **out);
int s3dg_gen_create_ratio(uint64_t size, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                          int has_seed, uint64_t seed, s3dg_gen **out);
int s3dg_gen_destroy(s3dg_gen *gen);
/* ObjectGenAlt::fill_chunk (src/data_gen_alt.rs:122): next min(cap, remaining)
 * bytes into buf; *written = 0 once complete. */
int s3dg_gen_fill_chunk(s3dg_gen *gen, uint8_t *buf, uint64_t cap, uint64_t *written);
/* Random access: bytes [pos, pos+n) of the object (does not move position). */
int s3dg_gen_fill_at(s3dg_gen *gen, uint8_t *buf, uint64_t pos, uint64_t n);
int s3dg_gen_is_complete(s3dg_gen *gen);
uint64_t s3dg_gen_position(s3dg_gen *gen);
uint64_t s3dg_gen_total_size(s3dg_gen *gen);
uint64_t s3dg_gen_seed(s3dg_gen *gen);
/* The host slot the generator runs on (s3dg_host_slot_device gives its GPU). */
int s3dg_gen_slot(s3dg_gen *gen);
int s3dg_gen_reset(s3dg_gen *gen);
/* generate_data / generate_controlled_data_alt one-shot into buf. */
int s3dg_generate_data(uint8_t *buf, uint64_t size, uint64_t dedup, uint64_t compress,
                       int has_seed, uint64_t seed);
/* The read-side twin of s3dg_generate_data(buf, size, dedup, compress, 1, seed),
 * and of whatever a seeded generator wrote into buf in whatever chunk sizes
 * (generation is positional): compares buf[0, size) with that object's bytes
 * on a host slot's GPU (H2D in 64 MiB chunks on two streams, each verified as
 * a DG1 block range into one device record).  buf may have any alignment and
 * be read-only; nothing is written to it.  size 0: clean, no GPU touched; a
 * null `out` is S3DG_EINVAL.  On an error no copy is still reading buf. */
int s3dg_verify_generated_data(const uint8_t *buf, uint64_t size, uint64_t dedup, uint64_t compress,
                               uint64_t seed, s3dg_verify_result *out);

/* ---- object assembly: generate_object (src/data_gen.rs:29-94) ------------ */
enum { S3DG_OBJ_NPZ = 0, S3DG_OBJ_TFRECORD = 1, S3DG_OBJ_HDF5 = 2, S3DG_OBJ_RAW = 3 };
enum { S3DG_MODE_STREAMING = 0, S3DG_MODE_SINGLE_PASS = 1 };
/* Bytes generate_object produces for (type, elements, element_size). */
int s3dg_object_size(int type, uint64_t elements, uint64_t element_size, uint64_t *out);
/* generate_object(&Config) into `out` (>= s3dg_object_size bytes):
 * use_controlled=0 -> generate_random_data payload, else the dgen-contract
 * payload; then build_raw / build_tfrecord / build_npz.  HDF5 -> S3DG_EINVAL
 * (as a reference build without the hdf5 feature).  has_seed=0 reproduces
 * the reference's non-deterministic entropy. */
int s3dg_generate_object(int type, uint64_t elements, uint64_t element_size, int use_controlled,
                         uint64_t dedup, uint64_t compress, int mode, int has_seed, uint64_t seed,
                         uint8_t *out, uint64_t out_len, uint64_t *written);
/* build_tfrecord_with_index (src/data_formats/tfrecord.rs:47-75): records of
 * record_size bytes from `data` -> out (records * (16 + record_size) bytes;
 * may alias data shifted by 12 for one record); index_out (nullable) gets
 * 16 bytes <offset u64, length u64> per record. */
int s3dg_build_tfrecord(uint64_t records, uint64_t record_size, const uint8_t *data, uint8_t *out,
                        uint8_t *index_out);
/* build_npz (src/data_formats/npz.rs:114-132): "data.npy" in a stored ZIP. */
int s3dg_npz_legacy_size(uint64_t elements, uint64_t data_len, uint64_t *out);
int s3dg_build_npz(uint64_t elements, const uint8_t *data, uint64_t data_len, uint8_t *out,
                   uint64_t out_len);

/* ---- put pipeline: per-object payloads -> files -------- */
/* Replaces put_objects_with_random_data_and_type (src/s3_utils.rs:1717-1750)
 * + put_objects_parallel_with_progress (:1812-1868) + FileSystemObjectStore::put
 * (src/file_store.rs:550-569) for file:// targets, with one payload PER OBJECT
 * (the reference PUTs one buffer to every URI).  Object j (paths[j], a plain
 * file-system path: the file:// prefix already stripped) is framed as
 * object_type with elements = 1, element_size = size (python_core_api.rs:804),
 * its payload generated on the GPU with entropy object_entropy(seed_base, j):
 *   S3DG_PAYLOAD_CONTROLLED  fill_controlled_data layout (data_gen.rs:151-224)
 *   S3DG_PAYLOAD_RANDOM      generate_random_data layout (data_gen.rs:102-132)
 *   S3DG_PAYLOAD_DGEN        the DG1 dgen-contract stream
 * Parent directories are created; files are truncated.  max_in_flight writer
 * threads (0 -> 64) write from a pinned host ring while the GPU generates the
 * next chunk.  crc_out (nullable, n entries) receives the CRC-32 (crc32fast)
 * of each whole file as written (StreamingDataWriter::checksum,
 * src/streaming_writer.rs:183-186).  File-system errors -> S3DG_EIO. */
enum { S3DG_PAYLOAD_CONTROLLED = 0, S3DG_PAYLOAD_RANDOM = 1, S3DG_PAYLOAD_DGEN = 2 };
typedef struct {
    uint64_t objects;       /* files written */
    uint64_t bytes;         /* bytes written (payload + framing) */
    double seconds;         /* wall time of the call */
    double gpu_seconds;     /* time the generator thread waited on the GPU (gen + CRC + D2H) */
} s3dg_put_stats;
int s3dg_put_objects(s3dg_ctx *ctx, const char *const *paths, uint64_t n, uint64_t size,
                     int object_type, int payload, uint64_t dedup, uint32_t f_num, uint32_t f_den,
                     uint64_t seed_base, uint32_t max_in_flight, uint32_t *crc_out,
                     s3dg_put_stats *stats);
/* Same over several contexts (GPUs): object j is generated by context
 * j * nctx / n's lane (contiguous ranges), each lane with its own device
 * chunks, streams and pinned ring on its GPU's NUMA node, one shared writer
 * pool.  Files and checksums are identical for any nctx; two contexts on one
 * device run two lanes on it. */
int s3dg_put_objects_multi(s3dg_ctx *const *ctxs, uint32_t nctx, const char *const *paths,
                           uint64_t n, uint64_t size, int object_type, int payload, uint64_t dedup,
                           uint32_t f_num, uint32_t f_den, uint64_t seed_base, uint32_t max_in_flight,
                           uint32_t *crc_out, s3dg_put_stats *stats);

/* ---- host-buffer drop-ins (src/data_gen.rs:151 signature) ---------------- */
/* The host-buffer entry points (s3dlio_*, s3dg_gen_*, s3dg_generate_data,
 * s3dg_generate_object) run on a pool of SLOTS: one per GPU by default, each
 * with its own context, base-block copies and staging sets.  Every call takes
 * a slot round-robin (a generator keeps its slot); calls on different slots
 * run on different GPUs concurrently, and a call of >= 256 MiB is cut into
 * one range per slot generated in parallel.  Bytes never depend on the slot.
 * Slot devices: env S3DLIO_GPU_DEVICE=k pins every call to GPU k;
 * S3DLIO_GPU_DEVICES=a,b,... lists them (repeats: several slots on one GPU);
 * neither: every visible GPU, or, in one rank of a multi-process job
 * (WORLD_SIZE > 1 and LOCAL_RANK set), that rank's GPU (LOCAL_RANK mod the
 * device count) only.  Env S3DLIO_HOST_D2H=staged copies through pinned
 * bounce buffers instead of straight into the caller's memory. */
/* The slot device list for the given env values and device count (pure
 * function; no GPU needed).  *n <= cap entries written to out. */
int s3dg_host_parse_devices(const char *pin, const char *list, int ndev, int *out, int cap, int *n);
/* The same with the multi-process job's LOCAL_RANK / WORLD_SIZE values (NULL:
 * unset); the library's own slot list is this function of its environment. */
int s3dg_host_parse_devices_env(const char *pin, const char *list, const char *local_rank,
                                const char *world_size, int ndev, int *out, int cap, int *n);
int s3dg_host_slot_count(int *out);
int s3dg_host_slot_device(int slot, int *device);
/* The slot's context (owned by the pool: never destroy it); slot < 0 takes
 * the next slot round-robin. */
int s3dg_host_slot_context(int slot, s3dg_ctx **out);
/* generate_random_data(size) (src/data_gen.rs:102): seeded analogue layout
 * with time entropy and a per-process random BASE_BLOCK. */
int s3dlio_generate_random_data(uint8_t *buf, size_t size);
/* fill_controlled_data(buf, dedup, compress): time-based entropy and a
 * per-process random base block, exactly as the reference; generated on the
 * host slots' GPUs (above) and copied into `buf`.  Empty buffer: no-op. */
int s3dlio_fill_controlled_data(uint8_t *buf, size_t len, size_t dedup, size_t compress);
/* Seeded sibling: entropy replaces call_entropy; base4096 (nullable)
 * replaces A_BASE_BLOCK (NULL = a context's default base block, seed
 * 0xBA5EB10C00000000). */
int s3dlio_fill_controlled_data_seeded(uint8_t *buf, size_t len, size_t dedup,
                                       size_t compress, uint64_t entropy,
                                       const uint8_t *base4096);
/* Its read-side twin: compare buf[0, len) with what the seeded fill would
 * write for (dedup, compress, entropy, base4096), on a host slot's GPU.  Any
 * alignment, read-only memory included; nothing is written to buf.  Empty
 * buffer: {0, 0, UINT64_MAX} without touching the GPU. */
int s3dlio_verify_controlled_data_seeded(const uint8_t *buf, size_t len, size_t dedup,
                                         size_t compress, uint64_t entropy,
                                         const uint8_t *base4096, s3dg_verify_result *out);

const char *s3dg_last_error(void);
const char *s3dg_version(void);
/* The 16-hex-digit digest of the sources the library was built from
 * (s3dlio_amd/build.py source_digest); bench.py stamps it and refuses a
 * library whose digest differs from the tree it runs in. */
const char *s3dg_build_digest(void);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* S3DLIO_GPU_H */
