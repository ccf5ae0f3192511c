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
 * identical.
 *
 * S3DG_CHUNKS_SEARCH_WALK (bytes, default 0 = off; negative: refused): in the
 * following adds (stream and batch form, per object) every object of at least
 * this many bytes has its cuts walked in parallel inside the object (DESIGN.md
 * 5.11.1) instead of by one wave; smaller objects of the same add keep the
 * wave.  Every field of the result is the same either way, for every input;
 * the adds stay asynchronous.  It pays for large single objects (the wave
 * takes about a microsecond per chunk of an object, one after the other) and
 * costs scratch: s3dg_chunks_search_geometry reports node_bytes per node and
 * hop_links, the links one step of the remaining serial part covers; an
 * object reserves ceil(len / min_bytes) + 1 + 2 ceil(len / avg_bytes) + 64
 * nodes.  An object with more candidates than that is walked by the wave,
 * decided on the device.  seconds[1] of s3dg_chunks_pass_seconds covers
 * everything that replaces the walk. */
enum { S3DG_CHUNKS_TIME_PASSES = 1, S3DG_CHUNKS_GEAR_TABLE = 2, S3DG_CHUNKS_SEARCH_WALK = 4 };
int s3dg_chunks_set_option(s3dg_chunks *h, int option, int value);
int s3dg_chunks_pass_seconds(s3dg_chunks *h, double *seconds);
int s3dg_chunks_search_geometry(uint32_t *hop_links, uint32_t *node_bytes);   /* needs no device */
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

/* ---- dedup, then LZ4 on the blocks kept (read-only) ---------
 * What a payload is worth to a store that deduplicates blocks of `block_bytes`
 * and then compresses the blocks it keeps: the data reduction ratio, payload
 * bytes over bytes kept after both steps, the answer to the generator's
 * `dedup` and `compress` knobs together.  The product of the two handles'
 * ratios above is that figure only when every distinct block compresses like
 * the average block; ragged last blocks, zero blocks and a dedup unit larger
 * than the store's block break it.  No seed is needed.
 *
 * block_bytes: a multiple of 4096 from 4096 to 65536.  Every object is cut
 * into blocks from its first byte; the last block of an object has whatever
 * length n >= 1 remains (s3dg_lz's rules and refusals).  Two blocks are the
 * same when they have the same length and the same bytes.  Over everything
 * added to the handle since it was created or reset, across adds and streams,
 * every distinct block is counted once: unique_blocks and unique_bytes are
 * their number and their summed length, and the six LZ fields are s3dg_lz's
 * (steps 1-4 above) summed over the distinct blocks only.  Equal blocks parse
 * equally, so it does not matter which occurrence is parsed.
 * Blocks are compared through 128-bit fingerprints, s3dg_measure's: a ragged
 * block never equals a full one (bytes and length are compared),
 * unique_blocks is the exact number of distinct fingerprints, s3dg_measure's
 * over the same adds, and two different blocks share one with probability
 * about 2^-64 per pair for data that was not built against the (public,
 * fixed) keys.
 *
 * A handle accumulates over adds on any stream, like s3dg_measure.  Every add
 * makes two passes on its stream: the measure's fingerprint pass into the
 * handle's kept array (16 bytes per block ever added, in an array that grows
 * by doubling; 20 bytes per 4 KiB of the add as scratch per stream), then one
 * wave per block that claims the block's fingerprint in the handle's table
 * and loads and parses the block only if the claim is new: a duplicate block
 * is never read a second time.  The table is open addressing in device
 * memory, 8 bytes a slot (s3dg_reduce_geometry), a power of two of slots at
 * least twice the blocks the handle holds, from 4096 slots on.  An add that
 * would pass that bound first waits for the adds the handle has enqueued and
 * rebuilds the table at its new size; so does growing the kept array.
 * Out of scope: content-defined chunks as the dedup unit; any compressor but
 * this one; emitting the compressed bytes; automatic choice of block_bytes; a
 * bench.py config (tools/reduce_rate.py times the add).
 * Destroy a handle before its context. */
typedef struct s3dg_reduce s3dg_reduce;
typedef struct {
    uint64_t bytes;          /* payload bytes added (stride gaps excluded) */
    uint64_t blocks;         /* blocks added, ragged last blocks included */
    uint64_t unique_blocks;  /* distinct among them (bytes and length) */
    uint64_t unique_bytes;   /* summed length of one block per distinct fingerprint */
    uint64_t lz_bytes;       /* the rest over the distinct blocks: sum of size */
    uint64_t stored_bytes;   /* sum of min(size, n): what the store keeps */
    uint64_t raw_blocks;     /* blocks with size >= n */
    uint64_t matches;
    uint64_t match_bytes;    /* sum of L */
    uint64_t literal_bytes;  /* literal_bytes + match_bytes == unique_bytes */
} s3dg_reduce_result;
int s3dg_reduce_create(s3dg_ctx *ctx, uint64_t block_bytes, s3dg_reduce **out);
int s3dg_reduce_destroy(s3dg_reduce *h);
/* Waits for the enqueued adds; an empty handle again: the totals and the table
 * zeroed, the kept fingerprints forgotten (the arrays keep their size). */
int s3dg_reduce_reset(s3dg_reduce *h);
/* The arguments, ordering and refusals of s3dg_lz_add_stream, s3dg_lz_add_range
 * and s3dg_lz_add_batch.  Slots of the kept array are reserved on the host
 * under the handle's mutex, so adds from several threads on several streams
 * are safe; two adds that run at once and hold the same block count it once.
 * A refused add leaves the handle as it was.  An add that fails with S3DG_EHIP
 * after its first launch may have left claims in the table: the handle then
 * refuses adds and get (S3DG_EHIP, with a message that says so) until
 * s3dg_reduce_reset. */
int s3dg_reduce_add_stream(s3dg_reduce *h, const void *src, uint64_t obj_size, uint64_t stride,
                           uint64_t n_objs, void *stream);
int s3dg_reduce_add_range(s3dg_reduce *h, const void *src, uint64_t obj_size, uint64_t blk_lo,
                          uint64_t blk_hi, void *stream);
int s3dg_reduce_add_batch(s3dg_reduce *h, const void *src_base, const s3dg_span *spans, uint64_t n,
                          void *stream);
/* Waits for the enqueued adds and fills *out.  The handle is unchanged: get
 * again, or add and get.  An empty handle yields all zeros. */
int s3dg_reduce_get(s3dg_reduce *h, s3dg_reduce_result *out);
/* The table's first size in slots and a slot's bytes.  Needs no device. */
int s3dg_reduce_geometry(uint32_t *initial_slots, uint32_t *slot_bytes);
/* A host buffer (any alignment, read-only memory included) as one object, on
 * a host slot's GPU: copied in chunks of whole blocks (up to 64 MiB) on the
 * slot's two streams in turn, each chunk an s3dg_reduce_add_range.
 * len == 0: all zeros, no GPU needed. */
int s3dg_reduce_data(const uint8_t *buf, uint64_t len, uint64_t block_bytes, s3dg_reduce_result *out);

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
 * Where the platform cannot page-lock memory a process already has
 * (hipHostRegister fails on a page of the library's own as well, as on a GPU
 * passed through to a virtual machine), the range is recorded without a GPU
 * mapping and the call returns 0: calls inside it are exact and take the same
 * paths as for any pageable buffer, s3dg_host_unregister counts it, and only
 * the speed-up is absent (s3dg_host_alloc_pinned memory has it everywhere).
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
/* s3dg_tfrecord_index_batch with parallelism inside a stream: the same
 * arguments, the same refusals with the same messages, and exactly the same
 * results and index bytes for every input, wrong length CRCs and truncations
 * included.  Every position of every stream is tested for a header whose
 * record fits and whose length CRC is right; the candidates are linked into a
 * forest, hop tables of hop_records links are built by pointer doubling, and
 * one wave per stream follows the chain from byte 0 hop by hop (a header whose
 * CRC is wrong is stepped through from the raw bytes, as the walk does) while
 * a thread per hop stores the entries.  It reads every byte, so it is the call
 * for few long streams; s3dg_tfrecord_index_batch, which reads 12 bytes per
 * record, is the call for many streams (DESIGN.md §5.5.3 has the figures).
 * Scratch: bytes / 8 + bytes / 32 per stream rounded up to whole tiles of
 * tile_bytes, and 52 bytes per candidate, kept with the stream's state.
 * Two more refusals, neither reachable below 2^45 bytes in a call: "more than
 * 2^31 - 2 search tiles in one call", "more than 2^32 - 16 header candidates
 * in one call". */
int s3dg_tfrecord_index_search_batch(s3dg_ctx *ctx, const void *base, void *idx_base, const s3dg_tfrecord_stream *streams,
                                     uint64_t n, void *stream, s3dg_tfrecord_walk_result *results);
/* The same call with its passes timed by device events: pass_ms[6] gets the
 * milliseconds of the candidate pass, the sum over the tiles, the link pass,
 * the doubling rounds, the anchor walk and the fill ("null pass_ms"). */
int s3dg_tfrecord_index_search_timed(s3dg_ctx *ctx, const void *base, void *idx_base, const s3dg_tfrecord_stream *streams,
                                     uint64_t n, void *stream, s3dg_tfrecord_walk_result *results, float *pass_ms);
/* The search's two constants, for placing test edges: positions per tile and
 * records per hop, both powers of two.  No context, no device. */
int s3dg_tfrecord_search_geometry(uint32_t *tile_bytes, uint32_t *hop_records);
/* The payloads of indexed records copied out of framed streams, every copied
 * record checked in the same pass.  The only description is
 * what s3dg_tfrecord_index_batch left in device memory.  A take is a run of
 * consecutive records of one index; a run of count == 1 is a pick, and a
 * shuffled batch of B rows is B takes with dst_off = k * row_stride,
 * dst_cap = row_stride.  Takes may come in any order, repeat, share a stream
 * and have count == 0 (nothing read or written, status 0). */
typedef struct {
    uint64_t off;       /* the framed stream starts at base + off, any byte offset (as s3dg_tfrecord_stream.off) */
    uint64_t bytes;     /* its length; no byte outside [off, off + bytes) is read */
    uint64_t idx_off;   /* its index entries, as s3dg_tfrecord_index_batch writes them, at idx_base + idx_off (multiple of 16) */
    uint64_t first;     /* take records [first, first + count) of that index */
    uint64_t count;
    uint64_t dst_off;   /* their payloads, packed back to back, at dst_base + dst_off (multiple of 16) */
    uint64_t dst_cap;   /* bytes that may be written there */
} s3dg_tfrecord_take;
typedef struct {
    uint64_t records, bytes;          /* records taken, payload bytes written */
    uint64_t status;                  /* 0 taken; 1 payload exceeds dst_cap; 2 the entries do not describe the stream */
    uint64_t bad_records, bad_length, bad_length_crc, bad_data_crc;   /* as s3dg_tfrecord_result */
    uint64_t first_take, first_record;   /* first take (caller's index) with a bad record, and its lowest bad record; UINT64_MAX when clean */
} s3dg_tfrecord_extract_result;
/* Synchronous on `stream`; `takes` is consumed before it returns; per_take
 * (a host array of n) may be NULL.  With e_i = <o_i, s_i> the i-th entry of a
 * take's index, record i's payload is the s_i - 16 bytes at off + o_i + 12 and
 * lands at dst_off + (o_i - o_first) - 16 (i - first).
 * The entries are validated on the device before anything of the take is
 * copied: every s_i >= 16, o_i + s_i == o_{i+1} inside the run, o_i + s_i <=
 * bytes, no 64-bit wrap.  A take that fails is status 2: it reads no stream
 * byte and writes nothing.  Reading 16 * (first + count) bytes of index memory
 * at idx_off is the caller's contract; what they say is not.  A take whose
 * payload exceeds dst_cap is status 1 and writes nothing; other takes are
 * unaffected.  A taken take writes exactly [dst_off, dst_off + payload), every
 * byte once; destination spans must not overlap each other or any stream.
 * Reads are aligned dwords, each holding a byte of the record it serves.
 * Per record the three classes of s3dg_tfrecord_result: the length field
 * against s_i - 16, the length CRC against that length's, the footer against
 * the data's masked CRC.  The copy goes by the index and delivers the bytes as
 * they stand: a bad record is reported, not withheld.  first_record is the
 * record's number in its index (first + i).  A clean call costs no atomic
 * beyond one per record longer than a region.  total sums the takes; its
 * status is the maximum over them; records and bytes count taken takes.
 * Scratch: 64 bytes per take and 28 bytes per record, kept with the stream's
 * state.  Refusals (S3DG_EINVAL, before anything is reserved or enqueued):
 * "null context", "null base", "null idx_base", "null dst_base", "null
 * output", "null take array", a misaligned idx_base or dst_base, more than
 * 2^32 - 1 takes, and per take ("take k: ...") idx_off or dst_off no multiple
 * of 16, first + count, off + bytes, dst_off + dst_cap or the index's end
 * overflowing, more than 2^31 - 2 records in one call, more than 2^46 stream
 * bytes in one call (a take counts min(bytes, dst_cap + 16 count), what it can
 * read).  n == 0 succeeds whatever the other pointers.
 * Holding a TFRecord object read back from a store to its seed (extract, then
 * s3dg_verify_* on the result) is the follow-up and not part of this call. */
int s3dg_tfrecord_extract_batch(s3dg_ctx *ctx, const void *base, const void *idx_base, void *dst_base,
                                const s3dg_tfrecord_take *takes, uint64_t n, void *stream,
                                s3dg_tfrecord_extract_result *total, s3dg_tfrecord_extract_result *per_take);
/* The same call with its passes timed by device events: pass_ms[3] gets the
 * milliseconds of the plan (validation and constants), the scan, and the copy
 * with its fold ("null pass_ms"). */
int s3dg_tfrecord_extract_timed(s3dg_ctx *ctx, const void *base, const void *idx_base, void *dst_base,
                                const s3dg_tfrecord_take *takes, uint64_t n, void *stream,
                                s3dg_tfrecord_extract_result *total, s3dg_tfrecord_extract_result *per_take,
                                float *pass_ms);
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
/* ---- NPZ archives framed and checked on the device ----
 * A list of stored ZIP archives, each of any number of member arrays, written
 * into device memory in one call and checked there by its twin.  Per member
 * the archive holds a local header, the name, the NPY header and the payload;
 * one central entry per member and the end record follow the last member.
 * The header fields are write_local_file_header, write_central_dir_entry and
 * write_eocd (src/data_formats/npz.rs:254-309) for S3DG_NPZ_STYLE_RAW and
 * s3dg_build_npz's for S3DG_NPZ_STYLE_LEGACY; a member's CRC-32 is that of its
 * NPY header followed by its payload.  Members "x.npy" (the keystream) and
 * "y.npy" (S3DG_NPZ_ZEROS) in STYLE_RAW give generate_npz_bytes_raw's bytes;
 * one member "data.npy" with the '|u1' header in STYLE_LEGACY gives
 * s3dg_build_npz's.  Names and NPY headers are host bytes in `blob`; only they
 * and the descriptors cross the bus.
 * There is no ZIP64.  The reference truncates sizes and offsets with `as u32`
 * and then writes an archive nobody can read; these calls refuse instead: a
 * member whose hdr_len + size reaches 2^32, and an archive in which a local
 * header's offset, the central directory's offset or its size reaches 2^32. */
#define S3DG_NPZ_ZEROS UINT64_MAX        /* src_off of a member whose payload is `size` zero bytes: no source is read */
enum { S3DG_NPZ_STYLE_RAW = 0,           /* header fields of generate_npz_bytes_raw (npz.rs:254-309): version 20/20, time and date 0 */
       S3DG_NPZ_STYLE_LEGACY = 1 };      /* header fields of s3dg_build_npz / object_frame: version needed 10, date 0x21 */
typedef struct {
    uint64_t src_off;                    /* payload at src_base + src_off (multiple of 16), or S3DG_NPZ_ZEROS */
    uint64_t size;                       /* payload bytes; 0 is a valid member */
    uint32_t name_off, name_len;         /* the member's file name in `blob` (1..65535 bytes, ".npy" included by the caller) */
    uint32_t hdr_off, hdr_len;           /* the member's NPY header bytes in `blob` (may be 0: a raw stored file) */
} s3dg_npz_member;
typedef struct {
    uint64_t dst_off;                    /* the archive at dst_base + dst_off, a multiple of 16 */
    uint64_t member0, members;           /* members[member0 .. member0 + members), 1..65535 */
    uint32_t style, pad;
} s3dg_npz_archive;
typedef struct {
    uint64_t members, bad_members;       /* members looked at / with at least one of the next two */
    uint64_t bad_local;                  /* local header, name or NPY header bytes differ from what the descriptor gives */
    uint64_t bad_crc;                    /* CRC-32 of NPY header || payload as they lie in memory differs from the local header's field */
    uint64_t bad_directory;              /* archives whose central directory or end record differ (CRC fields against the recomputed CRC) */
    uint64_t first_archive, first_member;/* caller's index of the first bad archive, its lowest bad member (UINT64_MAX when clean, or when only the directory is bad) */
} s3dg_npz_result;
/* Bytes of an archive of these members: sum(30 + name_len + hdr_len + size +
 * 46 + name_len) + 22.  No context, no blob.  S3DG_EINVAL when the sum
 * overflows, when out is null, or when m is null with members present. */
int s3dg_npz_archive_size(const s3dg_npz_member *m, uint64_t members, uint64_t *out);
/* Frames every archive of the list in one call; s3dg_tfrecord_frame_batch's
 * contract.  Ordered on `stream`, returns without a wait; `archives`,
 * `members` and `blob` (host arrays) are consumed before it returns.  Archives
 * may come in any order and may share members and sources.  src_base and
 * dst_base are 16-byte aligned device pointers.
 * Writes exactly the bytes of each archive: no byte before dst_off, none at or
 * past the archive's ragged end (a neighbour may start at the next multiple of
 * 16), and every byte once.  A payload lands at any residue mod 16, which
 * differs from member to member: stores are aligned 16-byte pieces, the ragged
 * first and last piece of a payload go byte by byte.  Source reads are aligned
 * dwords, each holding a byte of the member's [src_off, src_off + size); a
 * S3DG_NPZ_ZEROS member reads nothing.  Archives must not overlap each other
 * or any source (the caller's contract); overlap of an archive and one of its
 * own sources is refused.
 * Refusals (S3DG_EINVAL, each with a message; every descriptor is checked
 * before anything is reserved or enqueued, so a refused call has read and
 * written nothing): "null context", a null or misaligned base, null arrays,
 * per archive ("archive k: ...") dst_off no multiple of 16, an unknown style,
 * no members or more than 65535, member0 + members beyond nmembers, the
 * central directory's offset or size reaching 2^32, an end address
 * overflowing, more than 2^46 archive bytes in one call; per member
 * ("member j: ...", j its place in `members`) src_off no multiple of 16,
 * name_len outside 1..65535, a name or header range outside `blob`,
 * hdr_len + size reaching 2^32, its local header's offset reaching 2^32.
 * n == 0 succeeds whatever the other pointers. */
int s3dg_npz_frame_batch(s3dg_ctx *ctx, const void *src_base, void *dst_base, const s3dg_npz_archive *archives, uint64_t n,
                         const s3dg_npz_member *members, uint64_t nmembers, const uint8_t *blob, uint64_t blob_len,
                         void *stream);
/* The read-side twin over the same descriptors (src_off is not looked at): the
 * archive is at base + dst_off.  Synchronous on `stream`; writes nothing to
 * the archives, and a clean archive costs no atomic.  Per member: the local
 * header, the name and the NPY header against what the descriptors give
 * (bad_local; a descriptor whose size is not the archive's shows here), and
 * the local header's CRC field against the CRC-32 of the NPY header and the
 * payload in memory (bad_crc; where the NPY header itself differs that is
 * bad_local alone).  Per archive: the central directory and the end record
 * (bad_directory); a central entry's CRC field is wrong when it is neither the
 * recomputed CRC nor the local header's field, so damage to a payload or to a
 * local CRC field is reported once, as bad_crc.  total (required) sums the
 * archives; per_archive (host array of n, or NULL) gets every archive's own
 * result, first_archive being k or UINT64_MAX.  Refusals as above, and "null
 * output". */
int s3dg_npz_check_batch(s3dg_ctx *ctx, const void *base, const s3dg_npz_archive *archives, uint64_t n,
                         const s3dg_npz_member *members, uint64_t nmembers, const uint8_t *blob, uint64_t blob_len,
                         void *stream, s3dg_npz_result *total, s3dg_npz_result *per_archive);
/* ---- NPZ archives unpacked on the device from their bytes ----
 * list_npz_arrays / read_npz_array (src/data_formats/npz.rs) for every archive
 * of a list in one call each: the index of stored ZIP archives nobody has
 * described (numpy.savez's included), and their members' array bytes copied
 * out by that index with the CRC-32 checked in the copy.  Everything an
 * archive says about itself is read on the device.
 * Archive k is `bytes` bytes at base + off (any byte offset; no byte outside is
 * read).  Per member, in central-directory order and at most max_members of
 * them, one 32-byte entry of eight little-endian uint32 goes to
 * table + tab_off (a multiple of 16), every offset from the archive's first
 * byte: local_off, name_len | flags << 16, hdr_off (first byte of the stored
 * file: the NPY magic when there is one), hdr_len, data_off, size, crc, 0.
 * hdr_off + hdr_len == data_off; the stored file is hdr_len + size bytes; the
 * name is at local_off + 30. */
typedef struct {
    uint64_t off, bytes, tab_off, max_members;
} s3dg_npz_stream;
enum { S3DG_NPZ_WALK_OK = 0,
       S3DG_NPZ_WALK_NO_END = 1,         /* no end record whose comment reaches the archive's end in the last 22 + 65535 bytes */
       S3DG_NPZ_WALK_DIRECTORY = 2,      /* the end record or a central entry is inconsistent, or a member leaves [0, cd_off) */
       S3DG_NPZ_WALK_LOCAL = 3,          /* a local header disagrees with its central entry */
       S3DG_NPZ_WALK_UNSUPPORTED = 4,    /* a member is deflated, encrypted or has a data descriptor */
       S3DG_NPZ_WALK_CAPPED = 5 };       /* max_members entries are written and more members follow */
typedef struct {
    uint64_t status;
    uint64_t members;                    /* entries written; all of them valid whatever the status */
    uint64_t members_total;              /* the end record's count (0 with NO_END) */
    uint64_t payload_bytes;              /* sum of size over the entries written */
    uint64_t packed_bytes;               /* sum of round_up(size, 16): what one take of all of them spans */
    uint64_t bad_member;                 /* the member refused (DIRECTORY, LOCAL, UNSUPPORTED); UINT64_MAX when none or the end record */
} s3dg_npz_walk_result;
/* Synchronous on `stream`; results is a host array of n.  One wave walks one
 * archive.  End record: searched backwards from the end, 64 positions a step,
 * for the signature with comment_len equal to the distance to the archive's
 * end; the hit nearest the end wins.  Directory: disk numbers 0, equal entry
 * counts, cd_off + cd_size at the end record, no ZIP64 marker, every central
 * entry with its signature inside the directory, the entries ending exactly at
 * its end, every stored file inside [0, cd_off).  Local header: signature,
 * name, flags, method and CRC field equal to the central entry's, both sizes
 * equal to it or 0xFFFFFFFF with the real values in the extra field's 0x0001
 * record (numpy.savez); the data starts behind the local header's own name and
 * extra lengths.  NPY preamble: "\x93NUMPY", major 1 with a u16 or major 2 / 3
 * with a u32 header length; hdr_len is preamble plus that, inside the stored
 * file and at most 65535, anything else is a raw stored file of hdr_len 0.
 * Refusals (S3DG_EINVAL, before anything is reserved or enqueued): "null
 * context", "null base", "null table", "null results", "null archive array", a
 * misaligned table, more than 2^32 - 1 archives, and per archive ("archive k:
 * ...") tab_off no multiple of 16, an archive of 2^32 bytes or more, an end
 * address overflowing.  n == 0 succeeds whatever the other pointers. */
int s3dg_npz_index_batch(s3dg_ctx *ctx, const void *base, void *table, const s3dg_npz_stream *archives, uint64_t n,
                         void *stream, s3dg_npz_walk_result *results);
/* A take is members [first, first + count) of the table at table + tab_off,
 * read from the archive at base + off; a take of count == 1 is a pick, B of
 * them with dst_off = k * row_stride gather one array out of each of B
 * archives into rows.  Takes may come in any order, repeat, share an archive
 * and have count == 0. */
typedef struct {
    uint64_t off, bytes;                 /* the archive, as s3dg_npz_stream */
    uint64_t tab_off;                    /* its entries, as s3dg_npz_index_batch writes them (multiple of 16) */
    uint64_t first, count;
    uint64_t dst_off;                    /* member i lands at dst_base + dst_off (multiple of 16) + sum of round_up(size_j, 16), j < i */
    uint64_t dst_cap;                    /* bytes that may be written there */
} s3dg_npz_take;
enum { S3DG_NPZ_TAKE_TAKEN = 0, S3DG_NPZ_TAKE_CAPACITY = 1, S3DG_NPZ_TAKE_TABLE = 2 };
typedef struct {
    uint64_t members, bytes;             /* members taken, payload bytes written */
    uint64_t span;                       /* the packed span, padding included: taken and CAPACITY takes */
    uint64_t status;                     /* 0 taken; 1 span exceeds dst_cap; 2 the entries do not describe the archive */
    uint64_t bad_crc;                    /* copied members whose CRC-32 over NPY header || payload differs from the entry's */
    uint64_t first_take, first_member;   /* first take with such a member and its lowest (numbered as in its table); UINT64_MAX when clean */
} s3dg_npz_unpack_result;
/* s3dg_tfrecord_extract_batch's contract.  Synchronous on `stream`; `takes` is
 * consumed before it returns; per_take (a host array of n) may be NULL.  The
 * entries are validated on the device before anything of the take is copied:
 * local_off + 30 + name_len <= hdr_off, hdr_off + hdr_len == data_off,
 * hdr_len <= 65535, data_off + size <= bytes, no wrap.  A take that fails is
 * status 2: it reads no archive byte and writes nothing.  A take whose span
 * exceeds dst_cap is status 1 and writes nothing; other takes are unaffected.
 * A taken take writes exactly the payload bytes, each once; the padding
 * between members is not written.  Reads are aligned dwords, each holding a
 * byte of the stored file it serves.  A member whose CRC is wrong is delivered
 * as it stands and counted.  A clean call costs no atomic beyond one per
 * member longer than a region.  total sums the takes; its status is the
 * maximum over them.  Scratch: 64 bytes per take and 36 bytes per member, kept
 * with the stream's state.  Refusals (S3DG_EINVAL, before anything is reserved
 * or enqueued): "null context", "null base", "null table", "null dst_base",
 * "null output", "null take array", a misaligned table or dst_base, more than
 * 2^32 - 1 takes, and per take ("take k: ...") tab_off or dst_off no multiple
 * of 16, first + count, off + bytes, dst_off + dst_cap or the table's end
 * overflowing, more than 2^31 - 2 members in one call, more than 2^46 archive
 * bytes in one call (a take counts min(count * bytes, dst_cap + 65535 count),
 * what it can read).  n == 0 succeeds whatever the other pointers. */
int s3dg_npz_unpack_batch(s3dg_ctx *ctx, const void *base, const void *table, void *dst_base, const s3dg_npz_take *takes,
                          uint64_t n, void *stream, s3dg_npz_unpack_result *total, s3dg_npz_unpack_result *per_take);
/* The same call with its passes timed by device events: pass_ms[3] gets the
 * milliseconds of the plan (validation, offsets and constants), the scan of
 * the regions, and the copy with its fold ("null pass_ms"). */
int s3dg_npz_unpack_timed(s3dg_ctx *ctx, const void *base, const void *table, void *dst_base, const s3dg_npz_take *takes,
                          uint64_t n, void *stream, s3dg_npz_unpack_result *total, s3dg_npz_unpack_result *per_take,
                          float *pass_ms);

/* ---- DEFLATE streams and compressed NPZ members inflated on the device ----
 * RFC 1951 inflate, one wave per stream: raw DEFLATE (no zlib or gzip wrapper)
 * of src_bytes bytes at src_base + src_off (any byte offset; no byte outside
 * is used) is decoded to dst_base + dst_off (a multiple of 16), at most
 * dst_cap bytes.  want_bytes is the size the output must have, or UINT64_MAX
 * for any; crc is the CRC-32 the output must have when flags bit 0 is set.
 * Items may come in any order, repeat and share a source; two items must not
 * share destination bytes. */
typedef struct {
    uint64_t src_off, src_bytes;
    uint64_t dst_off, dst_cap;
    uint64_t want_bytes;
    uint32_t crc, flags;
} s3dg_inflate_item;
enum { S3DG_INFLATE_CRC = 1 };           /* flags bit 0: crc is given */
enum { S3DG_INFLATE_OK = 0,
       S3DG_INFLATE_CAPACITY = 1,        /* the output would pass dst_cap */
       S3DG_INFLATE_SIZE = 2,            /* the stream ended cleanly with fewer bytes than want_bytes, or would pass it */
       S3DG_INFLATE_TRUNCATED = 3,       /* the input ran out before the final block ended */
       S3DG_INFLATE_BAD_STREAM = 4 };    /* the bytes are no DEFLATE stream (the rules below) */
typedef struct {
    uint64_t status;                     /* total: the maximum over the items */
    uint64_t out_bytes;                  /* bytes written; of a failed item, what it had delivered before it stopped */
    uint64_t in_bytes;                   /* input bytes consumed, the last one possibly in part; trailing input is no error */
    uint64_t bad_crc;                    /* OK items with S3DG_INFLATE_CRC whose output's CRC-32 differs */
    uint64_t first_item;                 /* the first item whose status is not OK or whose CRC differs; UINT64_MAX when clean */
} s3dg_inflate_result;
/* Synchronous on `stream`; `items` is consumed before it returns; per_item (a
 * host array of n) may be NULL.  An item that fails ends with its status and
 * leaves the others untouched; what it had already written stays inside
 * [dst_off, dst_off + dst_cap), and no byte outside that place is ever
 * written.  BAD_STREAM: block type 3; a stored block whose LEN is not ~NLEN;
 * HLIT above 286 or HDIST above 30; a code-length repeat that runs over the
 * set or a 16 with no length before it; no end-of-block code; a set of code
 * lengths that is over-subscribed, or incomplete unless it is one code of
 * length 1 (zlib's rule; the code-length code must be complete); a bit
 * pattern that is no code; length symbols 286 and 287, distance codes 30 and
 * 31; a distance that reaches in front of the output's first byte.  A
 * condition that the missing input could still have met is TRUNCATED.  The
 * CRC-32 is computed from the finished output by a second kernel of the same
 * call.  Refusals (S3DG_EINVAL, before anything is reserved or enqueued):
 * "null context", "null src_base", "null dst_base", "null output", "null item
 * array", a misaligned dst_base, more than 2^32 - 1 items, and per item ("item
 * k: ...") dst_off no multiple of 16, src_off + src_bytes or dst_off +
 * dst_cap overflowing, flags beyond bit 0.  n == 0 succeeds whatever the
 * other pointers. */
int s3dg_inflate_batch(s3dg_ctx *ctx, const void *src_base, void *dst_base, const s3dg_inflate_item *items, uint64_t n,
                       void *stream, s3dg_inflate_result *total, s3dg_inflate_result *per_item);
/* s3dg_npz_index_batch for archives whose members are stored or deflated:
 * its arguments, results, walk and refusals, except that method 8 with flags
 * clear of bits 0 and 3 is accepted beside method 0 (csize == usize is asked
 * of method 0 only).  A deflated member's NPY header lies inside its
 * compressed stream, so a z entry describes the whole stored file: eight
 * little-endian uint32 local_off, name_len | flags << 16, data_off (first
 * byte of the member's data), csize, usize, crc, method, 0.  payload_bytes and
 * packed_bytes are sums over usize and round_up(usize, 16). */
int s3dg_npz_zindex_batch(s3dg_ctx *ctx, const void *base, void *table, const s3dg_npz_stream *archives, uint64_t n,
                          void *stream, s3dg_npz_walk_result *results);
typedef struct {
    uint64_t members, bytes;             /* members of taken takes; bytes their streams delivered */
    uint64_t span;                       /* the packed span, padding included: taken and CAPACITY takes */
    uint64_t status;                     /* as s3dg_npz_unpack_result */
    uint64_t bad_crc;                    /* members delivered whole whose CRC-32 differs from the entry's */
    uint64_t bad_stream;                 /* members whose inflate status is not OK or whose output is not usize bytes */
    uint64_t first_take, first_member;   /* first take with a member of either kind and its lowest; UINT64_MAX when clean */
} s3dg_npz_zunpack_result;
/* s3dg_npz_unpack_batch over z entries: member i's whole stored file (NPY
 * header and array bytes) lands at dst_off + sum of round_up(usize_j, 16),
 * j < i; a stored member is copied, a deflated one inflated, by the same
 * kernel.  A plan pass on the device, one thread per take, validates the
 * entries (local_off + 30 + name_len <= data_off, data_off + csize <= bytes,
 * method 0 with csize == usize or method 8, no wrap), sums the places and
 * writes the work items, so no index crosses the bus.  TABLE and CAPACITY
 * takes write nothing.  Refusals as s3dg_npz_unpack_batch, less the bound on
 * archive bytes. */
int s3dg_npz_zunpack_batch(s3dg_ctx *ctx, const void *base, const void *table, void *dst_base, const s3dg_npz_take *takes,
                           uint64_t n, void *stream, s3dg_npz_zunpack_result *total, s3dg_npz_zunpack_result *per_take);

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
