"""Device-resident generation API over the C ABI (one Context per GPU).

This is the MI355X-native core the drop-in surfaces sit on:

    ctx = Context(device=0)                       # s3dg_ctx_create
    out = torch.empty(n * size, dtype=torch.uint8, device="cuda")
    ctx.fill_stream(out, obj_size=size, n_objs=n, dedup=1, compress=1, seed_base=S)

Semantics per object are src/data_gen.rs:151-224 (fill_controlled_data) with
the entropy and base block made explicit.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from . import _lib
from ._lib import ObjDesc, c_u32, c_vp, call, lib

BLOCK_SIZE = 4096
DEFAULT_BASE_SEED = 0xBA5EB10C00000000


def compress_ratio(compress) -> tuple[int, int]:
    """(f_num, f_den) of the zero prefix per 4 KiB block.

    Integer c maps to (c-1, c) and c <= 1 to (0, 1), exactly as
    src/data_gen.rs:169-173.  A rational p/q (Fraction, (p, q) tuple or a
    float such as 1.5) maps to (p-q, p): the build-defined generalisation
    needed by BASELINE config 4 (compress=1.5 -> (1, 3)); no reference API
    accepts it, so parity is defined for integer c only.
    """
    if isinstance(compress, (int, np.integer)) and not isinstance(compress, bool):
        fn, fd = c_u32(), c_u32()
        call("s3dg_compress_ratio", int(compress), ctypes.byref(fn), ctypes.byref(fd))
        return fn.value, fd.value
    if isinstance(compress, tuple):
        fr = Fraction(int(compress[0]), int(compress[1]))
    else:
        fr = Fraction(compress).limit_denominator(1 << 16)
    if fr <= 1:
        return 0, 1
    p, q = fr.numerator, fr.denominator
    return p - q, p


def unique_blocks(nblocks: int, dedup: int) -> int:
    return int(lib.s3dg_unique_blocks(nblocks, dedup))


def object_entropy(seed_base: int, j: int) -> int:
    return int(lib.s3dg_object_entropy(seed_base & (2**64 - 1), j))


@dataclass(frozen=True)
class VerifyResult:
    """s3dg_verify_result: what a verify call found."""
    mismatched_bytes: int = 0     # bytes that differ from the expected payload
    mismatched_blocks: int = 0    # 4 KiB blocks (per object) holding at least one
    first_offset: int | None = None   # lowest differing byte offset from the start; None = clean

    @property
    def ok(self) -> bool:
        return self.mismatched_bytes == 0

    @classmethod
    def _of(cls, r) -> "VerifyResult":
        first = int(r.first_offset)
        return cls(int(r.mismatched_bytes), int(r.mismatched_blocks), None if first == 2**64 - 1 else first)


@dataclass(frozen=True)
class BatchVerifyResult:
    """What Context.verify_batch found: the totals over the batch and, unless
    it was called with per_object=False, every object that is not clean."""
    total: VerifyResult = VerifyResult()   # counts summed over the objects; first_offset from the buffer's start
    objects: int = 0                       # descriptors checked, empty ones included
    # (index, VerifyResult) of every object that is not clean, in index order,
    # first_offset from the object's first byte; None with per_object=False
    mismatches: tuple | None = ()

    @property
    def ok(self) -> bool:
        return self.total.ok

    @property
    def mismatched_objects(self) -> int | None:
        """Objects that are not clean; None when the call asked for totals only."""
        return None if self.mismatches is None else len(self.mismatches)


@dataclass(frozen=True)
class MeasureResult:
    """s3dg_measure_result: what a payload looks like to a store that
    deduplicates and compresses at the measured block size."""
    bytes: int = 0            # payload bytes measured (stride gaps excluded)
    zero_bytes: int = 0
    blocks: int = 0           # blocks measured, ragged last blocks included
    unique_blocks: int = 0    # distinct among them (bytes and length)
    hist: tuple | None = None   # 256 byte counts, or None when not asked for

    @property
    def zero_fraction(self) -> float:
        return self.zero_bytes / self.bytes if self.bytes else 0.0

    @property
    def unique_fraction(self) -> float:
        """unique / blocks: the reference tests' "dedup ratio" (1/dedup expected)."""
        return self.unique_blocks / self.blocks if self.blocks else 0.0

    @property
    def dedup_ratio(self) -> float:
        """blocks / unique: what a dedup engine at this block size saves (n : 1)."""
        return self.blocks / self.unique_blocks if self.unique_blocks else 0.0

    @property
    def entropy_bits(self) -> float | None:
        """Shannon entropy in bits per byte from the histogram; None without one."""
        if self.hist is None:
            return None
        n = sum(self.hist)
        if n == 0:
            return 0.0
        p = np.array([c for c in self.hist if c], dtype=np.float64) / n
        return float(-(p * np.log2(p)).sum())

    @classmethod
    def _of(cls, r, hist: bool) -> "MeasureResult":
        return cls(int(r.bytes), int(r.zero_bytes), int(r.blocks), int(r.unique_blocks),
                   tuple(int(v) for v in r.hist) if hist else None)


@dataclass(frozen=True)
class ChunkResult:
    """s3dg_chunk_result: what a payload looks like to a store that
    deduplicates content-defined chunks."""
    bytes: int = 0            # payload bytes chunked (stride gaps excluded)
    chunks: int = 0           # chunks cut, every object's last one included
    unique_chunks: int = 0    # distinct among them (bytes and length)
    unique_bytes: int = 0     # summed length of one chunk per distinct fingerprint
    candidates: int = 0       # positions whose window hash passes
    forced_cuts: int = 0      # chunks cut at max_bytes without a candidate

    @property
    def dedup_ratio(self) -> float:
        """bytes / unique_bytes: what a dedup engine with this chunking saves (n : 1)."""
        return self.bytes / self.unique_bytes if self.unique_bytes else 0.0

    @property
    def unique_fraction(self) -> float:
        return self.unique_chunks / self.chunks if self.chunks else 0.0

    @property
    def mean_chunk(self) -> float:
        return self.bytes / self.chunks if self.chunks else 0.0

    @classmethod
    def _of(cls, r) -> "ChunkResult":
        return cls(int(r.bytes), int(r.chunks), int(r.unique_chunks), int(r.unique_bytes), int(r.candidates),
                   int(r.forced_cuts))


@dataclass(frozen=True)
class LzResult:
    """s3dg_lz_result: what a payload takes in a store that compresses
    independent blocks with a greedy LZ4."""
    bytes: int = 0            # payload bytes measured (stride gaps excluded)
    blocks: int = 0           # blocks compressed, ragged last blocks included
    lz_bytes: int = 0         # summed LZ4 block sizes
    stored_bytes: int = 0     # summed min(size, n): a block that does not shrink is kept raw
    raw_blocks: int = 0       # blocks with size >= n
    matches: int = 0
    match_bytes: int = 0
    literal_bytes: int = 0    # literal_bytes + match_bytes == bytes

    @property
    def ratio(self) -> float:
        """bytes / stored_bytes: what the store saves (n : 1)."""
        return self.bytes / self.stored_bytes if self.stored_bytes else 0.0

    @property
    def lz_ratio(self) -> float:
        """bytes / lz_bytes: the compressor's own ratio, below 1 for incompressible data."""
        return self.bytes / self.lz_bytes if self.lz_bytes else 0.0

    @property
    def match_fraction(self) -> float:
        return self.match_bytes / self.bytes if self.bytes else 0.0

    @property
    def raw_fraction(self) -> float:
        return self.raw_blocks / self.blocks if self.blocks else 0.0

    @classmethod
    def _of(cls, r) -> "LzResult":
        return cls(int(r.bytes), int(r.blocks), int(r.lz_bytes), int(r.stored_bytes), int(r.raw_blocks),
                   int(r.matches), int(r.match_bytes), int(r.literal_bytes))


CHUNK_DEFAULTS = (2048, 8192, 65536)   # min_bytes, avg_bytes, max_bytes
@dataclass(frozen=True)
class TfRecordResult:
    """What Context.tfrecord_check_batch found (s3dg_tfrecord_result): the
    totals over the list and, unless it was called with per_shard=False, every
    shard that is not clean."""
    records: int = 0
    bad_records: int = 0          # records bad in at least one of the three classes below
    bad_length: int = 0           # length field differs from record_size
    bad_length_crc: int = 0       # length CRC differs from record_size's
    bad_data_crc: int = 0         # footer differs from the data's masked CRC
    first_shard: int | None = None    # index of the first shard with a bad record; None = clean
    first_record: int | None = None   # its lowest bad record
    # (index, TfRecordResult) of every shard that is not clean, in index order; None with per_shard=False
    shards: tuple | None = ()

    @property
    def ok(self) -> bool:
        return self.bad_records == 0

    @classmethod
    def _of(cls, r, shards=()) -> "TfRecordResult":
        none = 2**64 - 1
        fs, fr = int(r.first_shard), int(r.first_record)
        return cls(int(r.records), int(r.bad_records), int(r.bad_length), int(r.bad_length_crc), int(r.bad_data_crc),
                   None if fs == none else fs, None if fr == none else fr, shards)


def tfrecord_size(records: int, record_size: int) -> int:
    """Bytes of a framed shard: records * (16 + record_size); ValueError when that overflows 64 bits."""
    out = _lib.c_u64(0)
    call("s3dg_tfrecord_size", int(records), int(record_size), ctypes.byref(out))
    return int(out.value)


def _tfr_shards(shards):
    """(s3dg_tfrecord_shard array, n, bytes of src, dst and index the shards reach)."""
    rows = []
    for sh in shards:
        sh = tuple(int(x) for x in sh)
        if len(sh) not in (4, 5):
            raise ValueError("a shard is (src_off, dst_off, records, record_size[, idx_off])")
        if any(x < 0 or x >= 2**64 for x in sh):
            raise ValueError("shard fields must fit 64 unsigned bits")
        rows.append(sh)
    arr = (_lib.TfrShard * max(1, len(rows)))()
    need_src = need_dst = need_idx = 0
    for k, sh in enumerate(rows):
        src_off, dst_off, records, rs = sh[:4]
        idx_off = sh[4] if len(sh) == 5 else 0
        arr[k] = _lib.TfrShard(src_off, dst_off, idx_off, records, rs)
        if records:
            need_src = max(need_src, src_off + records * rs)
            need_dst = max(need_dst, dst_off + records * (16 + rs))
            need_idx = max(need_idx, idx_off + 16 * records)
    return arr, len(rows), need_src, need_dst, need_idx


_WALK_STATUS = ("complete", "truncated", "full")


@dataclass(frozen=True)
class TfRecordWalk:
    """What Context.tfrecord_index_batch found in one stream
    (s3dg_tfrecord_walk_result)."""
    records: int = 0              # complete records found; their entries are written
    status: str = "complete"      # "complete" | "truncated" (a record does not fit) | "full" (max_records reached)
    stop_offset: int = 0          # offset in the stream of the first byte not covered by an entry
    trailing: int = 0             # bytes - stop_offset
    bad_length_crc: int = 0       # records whose length CRC is not masked_crc of their 8 length bytes
    first_bad_record: int | None = None   # the lowest such record

    @property
    def ok(self) -> bool:
        return self.status == "complete" and self.bad_length_crc == 0

    @classmethod
    def _of(cls, r) -> "TfRecordWalk":
        fb = int(r.first_bad_record)
        return cls(int(r.records), _WALK_STATUS[int(r.status)], int(r.stop_offset), int(r.trailing),
                   int(r.bad_length_crc), None if fb == 2**64 - 1 else fb)


def _tfr_lengths(lengths) -> np.ndarray:
    """Any integer sequence or numpy array as a contiguous uint64 array."""
    if isinstance(lengths, np.ndarray):
        a = lengths
        if a.size == 0:
            return np.zeros(0, np.uint64)
        if a.ndim != 1:
            raise ValueError("lengths must be one-dimensional")
        if a.dtype.kind not in "iu":
            raise ValueError("lengths must be integers")
        if a.dtype.kind == "i" and int(a.min()) < 0:
            raise ValueError("lengths must fit 64 unsigned bits")
        return np.ascontiguousarray(a, dtype=np.uint64)
    vals = list(lengths)   # Python integers above 2^63 would make numpy guess a float array
    if not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in vals):
        raise ValueError("lengths must be integers")
    if any(x < 0 or x >= 2**64 for x in vals):
        raise ValueError("lengths must fit 64 unsigned bits")
    return np.array([int(x) for x in vals], dtype=np.uint64)


def tfrecord_var_size(lengths) -> int:
    """Bytes of a framed shard of records of these lengths: sum(16 + length);
    ValueError when that overflows 64 bits."""
    a = _tfr_lengths(lengths)
    out = _lib.c_u64(0)
    call("s3dg_tfrecord_var_size", a.ctypes.data_as(ctypes.POINTER(_lib.c_u64)), len(a), ctypes.byref(out))
    return int(out.value)


def tfrecord_index_text(entries) -> str:
    """The DALI text form of an index, "{offset} {size}\\n" per record
    (index_text_from_bytes, src/tfrecord_index.rs:92-101): entries is an (n, 2)
    array or an iterable of (offset, size)."""
    return "".join(f"{int(o)} {int(s)}\n" for o, s in np.asarray(entries, dtype=np.uint64).reshape(-1, 2).tolist())


def _tfr_var_shards(shards):
    """(s3dg_tfrecord_var_shard array, n, the concatenated lengths, bytes of
    src, dst and index the shards reach)."""
    rows, lens = [], []
    for sh in shards:
        if len(sh) not in (3, 4):
            raise ValueError("a shard is (src_off, dst_off, lengths[, idx_off])")
        offs = [int(sh[0]), int(sh[1]), int(sh[3]) if len(sh) == 4 else 0]
        if any(x < 0 or x >= 2**64 for x in offs):
            raise ValueError("shard fields must fit 64 unsigned bits")
        rows.append(offs)
        lens.append(_tfr_lengths(sh[2]))
    arr = (_lib.TfrVarShard * max(1, len(rows)))()
    need_src = need_dst = need_idx = 0
    len0 = 0
    for k, ((src_off, dst_off, idx_off), a) in enumerate(zip(rows, lens)):
        records = len(a)
        arr[k] = _lib.TfrVarShard(src_off, dst_off, idx_off, records, len0)
        len0 += records
        if records:
            payload = sum(a.tolist()) if a.max() >= 2**40 else int(a.sum())
            need_src = max(need_src, src_off + payload)
            need_dst = max(need_dst, dst_off + payload + 16 * records)
            need_idx = max(need_idx, idx_off + 16 * records)
    cat = np.concatenate(lens) if lens else np.zeros(0, np.uint64)
    return arr, len(rows), np.ascontiguousarray(cat, dtype=np.uint64), need_src, need_dst, need_idx


_CHUNKS_TIME_PASSES, _CHUNKS_GEAR_TABLE = 1, 2   # S3DG_CHUNKS_* options


def _ptr(x) -> int:
    """Device pointer of a torch CUDA tensor (contiguous) or a raw int."""
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not x.is_cuda:
            raise ValueError("device generation needs a GPU tensor (tensor.is_cuda)")
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return int(x.data_ptr())
    raise TypeError(f"expected a torch CUDA tensor or an int device pointer, got {type(x)}")


def _spans(objects):
    """(s3dg_span array, n, bytes of src the non-empty spans reach) of
    add_batch's `objects`."""
    if isinstance(objects, np.ndarray):
        if objects.dtype != np.uint64 or objects.ndim != 2 or objects.shape[1] != 2:
            raise ValueError("a span array must be uint64 of shape (n, 2)")
        a = np.ascontiguousarray(objects)
    else:
        rows = [(int(o[0]), int(o[1])) for o in objects]
        if any(off < 0 or size < 0 or off >= 2**64 or size >= 2**64 for off, size in rows):
            raise ValueError("span offsets and sizes must fit 64 unsigned bits")
        a = np.array(rows, dtype=np.uint64).reshape(-1, 2)
    n = int(a.shape[0])
    need = 0
    if n:
        live = a[:, 1] != 0
        if live.any():
            off = a[live, 0]
            end = off + a[live, 1]   # wraps past 2^64: beyond every tensor
            need = 2**64 if (end < off).any() else int(end.max())
    arr = (_lib.Span * max(1, n))()
    if n:
        ctypes.memmove(arr, a.ctypes.data, 16 * n)
    return arr, n, need


def _nbytes(x) -> int | None:
    if hasattr(x, "numel") and hasattr(x, "element_size"):
        return int(x.numel() * x.element_size())
    return None


def _stream(stream, device: int | None = None) -> int:
    """hipStream_t handle: an int, a torch stream, or None = torch's current
    stream on `device` (the current device when None), so torch events time
    our launches."""
    if stream is None:
        t = _lib.torch
        if t is not None and t.cuda.is_available():
            cs = t.cuda.current_stream() if device is None else t.cuda.current_stream(device)
            return int(cs.cuda_stream)
        return 0
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)


class Context:
    """One GPU's generator context (s3dg_ctx)."""

    @classmethod
    def _borrow(cls, handle: int, device: int) -> "Context":
        """A context owned elsewhere (the host slot pool): never destroyed here."""
        self = cls.__new__(cls)
        self._h = c_vp(handle)
        self.device = int(device)
        self._borrowed = True
        return self

    def __init__(self, device: int = 0, base_block=None, base_seed: int | None = None,
                 waves_per_block: int | None = None, nontemporal: bool = False):
        h = c_vp()
        call("s3dg_ctx_create", int(device), ctypes.byref(h))
        self._h = h
        self.device = int(device)
        if base_block is not None:
            self.set_base_block(base_block)
        elif base_seed is not None:
            call("s3dg_set_base_block_seed", self._h, int(base_seed))
        if waves_per_block is not None:
            call("s3dg_set_waves_per_block", self._h, int(waves_per_block))
        if nontemporal:
            call("s3dg_set_nontemporal", self._h, 1)

    # -- lifecycle -------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_borrowed", False):
            return
        if getattr(self, "_h", None):
            call("s3dg_ctx_destroy", self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -----------------------------------------------------------
    def set_base_block(self, base) -> None:
        b = np.ascontiguousarray(np.frombuffer(bytes(base), np.uint8))
        if b.size != BLOCK_SIZE:
            raise ValueError("base block must be exactly 4096 bytes")
        call("s3dg_set_base_block", self._h, b.ctypes.data_as(_lib.c_u8p))

    @property
    def base_block(self) -> bytes:
        out = np.empty(BLOCK_SIZE, np.uint8)
        call("s3dg_get_base_block", self._h, out.ctypes.data_as(_lib.c_u8p))
        return out.tobytes()

    def set_waves_per_block(self, waves: int) -> None:
        call("s3dg_set_waves_per_block", self._h, int(waves))

    def set_nontemporal(self, on: bool) -> None:
        call("s3dg_set_nontemporal", self._h, 1 if on else 0)

    def set_store_policy(self, stream_policy: int = -1, batch_policy: int = -1) -> None:
        """Fill-kernel store cache policy: 0 plain, 1 nt, 2 sc1, 3 nt sc1, -1 default;
        results are identical."""
        call("s3dg_set_store_policy", self._h, int(stream_policy), int(batch_policy))

    def set_occupancy(self, stream_wgs_per_cu: int = -1, batch_wgs_per_cu: int = -1) -> None:
        """Cap resident fill workgroups per CU (0 = hardware max, negative = library
        default); results are identical."""
        call("s3dg_set_occupancy", self._h, int(stream_wgs_per_cu), int(batch_wgs_per_cu))

    def set_batch_pace(self, ticks: int = -1) -> None:
        """Batch kernel: hold each block's stores until `ticks` wall-clock ticks
        (10 ns) after its workgroup started (0 = off, negative = per launch);
        results are identical."""
        call("s3dg_set_batch_pace", self._h, int(ticks))

    def set_batch_prefetch(self, tiles: int = -1) -> None:
        """Tile-record prefetch distance of batch launches in units of 64 blocks
        (0 = off, negative = library default); results are identical."""
        call("s3dg_set_batch_prefetch", self._h, 0xFFFFFFFF if int(tiles) < 0 else int(tiles))

    def set_stream_tiles(self, on: int = -1) -> None:
        """1: large uniform streams run through the tiled batch kernel; 0: the 2D
        stream kernel; negative: library default.  Results are identical."""
        call("s3dg_set_stream_tiles", self._h, int(on))

    def set_batch_tile(self, blocks: int = 0) -> None:
        """Blocks per batch tile record: 2, 4, 8, 16, 32 or 64 forced, 1 = the dense
        layout (one record per 4 KiB granule) where the objects allow it, or 0 =
        chosen per launch (8..64 or dense).  2- and 4-block tiles keep a slot
        equal to its granule modulo 2 and 4 only, not modulo 8.  Results are
        identical."""
        call("s3dg_set_batch_tile", self._h, int(blocks))

    def set_batch_split(self, blocks: int = -1) -> None:
        """Objects of fewer than `blocks` blocks get a batch launch of their own
        (0 = one launch, negative = default); results are identical."""
        call("s3dg_set_batch_split", self._h, int(blocks))

    def set_keystream_shape(self, mode: int, draws: int = 0, waves: int = 0, wgs_per_cu: int = 0,
                            min_lane_draws: int = 0, store_policy: int = -1) -> None:
        """k_keystream launch shape for mode 0 (npz keystream) or 1 (DG1);
        0 (store: -1) = default for each; results are identical."""
        call("s3dg_set_keystream_shape", self._h, int(mode), int(draws), int(waves), int(wgs_per_cu),
             int(min_lane_draws), int(store_policy))

    def set_keystream_xcd_group(self, mode: int, waves: int = 0) -> None:
        """Keystream launches: each XCD writes runs of `waves` adjacent waves'
        lane regions (power of two; 0 = default 16); results are identical."""
        call("s3dg_set_keystream_xcd_group", self._h, int(mode), int(waves))

    def set_keystream_persist(self, rounds: int = -1) -> None:
        """Keystream launches of >= `rounds` rounds of resident waves run a
        persistent grid over per-XCD work queues (0 = never, negative = default:
        1-wave workgroups from 6 rounds).  Results are identical."""
        call("s3dg_set_keystream_persist", self._h, int(rounds))

    def set_keystream_tail(self, chunks: int = -1) -> None:
        """One-object DG1 launches on a persistent grid: the last `chunks`
        blocks in half-length lanes, handed out last (0 = off, negative =
        default).  Results are identical."""
        call("s3dg_set_keystream_tail", self._h, int(chunks))

    def set_dgen_zero_split(self, chunks: int = -1, waves: int = -1, occupancy: int = -1, store: int = -1,
                            overlap: int = -1) -> None:
        """DG1 launches with a zero prefix over >= `chunks` full 1 MiB blocks run
        as a zero-prefix launch in the fill's store shape plus a keystream
        launch over the tails (0 = never, negative = default 64); `waves`,
        `occupancy`, `store` and `overlap` (side stream) tune the zero launch.
        Results are identical."""
        call("s3dg_set_dgen_zero_split", self._h, int(chunks), int(waves), int(occupancy), int(store), int(overlap))

    def query_keystream_occupancy(self, mode: int = 0) -> int:
        out = ctypes.c_int()
        call("s3dg_query_keystream_occupancy", self._h, int(mode), ctypes.byref(out))
        return out.value

    def query_occupancy(self, batch: bool = False, zero_lines: bool = False) -> int:
        """Resident fill workgroups per CU under the current settings (batch
        launches: `zero_lines` = zero prefixes ending on a 64-B line)."""
        out = ctypes.c_int()
        call("s3dg_query_occupancy", self._h, (2 if zero_lines else 1) if batch else 0, ctypes.byref(out))
        return out.value

    # -- generation (asynchronous on `stream`) ----------------------------------
    # A torch tensor destination must live on this context's device and hold
    # every byte the call writes (ValueError otherwise: the C ABI only sees a
    # pointer and would write past the allocation).  A raw int pointer is the
    # caller's responsibility.
    def _dst(self, x, need: int, verb: str = "writes") -> int:
        p = _ptr(x)
        if not isinstance(x, int):
            idx = x.device.index if x.device.index is not None else 0
            if idx != self.device:
                raise ValueError(f"tensor is on cuda:{idx}, this context is on cuda:{self.device}")
            have = _nbytes(x)
            if need > have:
                raise ValueError(f"the call {verb} {need} bytes, the tensor holds {have}")
        return p

    def _s(self, stream) -> int:
        return _stream(stream, self.device)

    def fill_controlled(self, dst, nbytes: int | None = None, dedup: int = 1, compress=1,
                        entropy: int = 0, stream=None) -> None:
        """One object (src/data_gen.rs:151) of `nbytes` at dst."""
        n = _nbytes(dst) if nbytes is None else int(nbytes)
        fn, fd = compress_ratio(compress)
        call("s3dg_fill_controlled", self._h, self._dst(dst, n), n, int(dedup), fn, fd,
             int(entropy) & (2**64 - 1), self._s(stream))

    def random_data(self, dst, nbytes: int | None = None, entropy: int = 0, stream=None) -> None:
        """generate_random_data's layout (src/data_gen.rs:102-132): no zero
        prefix, one window at 0 and one at L-32 (L > 2048), seeded by `entropy`."""
        n = _nbytes(dst) if nbytes is None else int(nbytes)
        call("s3dg_random_data", self._h, self._dst(dst, n), n, int(entropy) & (2**64 - 1),
             self._s(stream))

    def fill_range(self, dst, length: int, blk_lo: int, blk_hi: int, dedup: int = 1,
                   compress=1, entropy: int = 0, stream=None) -> None:
        """Blocks [blk_lo, blk_hi) of a `length`-byte object, block blk_lo at dst."""
        fn, fd = compress_ratio(compress)
        hi = min(int(blk_hi) * BLOCK_SIZE, int(length))
        need = max(0, hi - int(blk_lo) * BLOCK_SIZE)
        call("s3dg_fill_controlled_range", self._h, self._dst(dst, need), int(length), int(blk_lo),
             int(blk_hi), int(dedup), fn, fd, int(entropy) & (2**64 - 1), self._s(stream))

    def fill_stream(self, dst, obj_size: int, n_objs: int, stride: int | None = None,
                    dedup: int = 1, compress=1, seed_base: int = 0, first_obj: int = 0,
                    stream=None) -> None:
        """n_objs equal objects, object j at dst + j*stride with entropy
        object_entropy(seed_base, first_obj + j)."""
        stride = obj_size if stride is None else stride
        need = (int(n_objs) - 1) * int(stride) + int(obj_size) if n_objs > 0 and obj_size > 0 else 0
        fn, fd = compress_ratio(compress)
        call("s3dg_fill_controlled_stream", self._h, self._dst(dst, need), int(obj_size), int(stride),
             int(n_objs), int(dedup), fn, fd, int(seed_base) & (2**64 - 1), int(first_obj),
             self._s(stream))

    # -- verification (synchronous on `stream`) ----------------------------------
    # The read-side twins of fill_controlled / fill_range / random_data /
    # fill_stream: the GPU recomputes each 4 KiB block and compares it with the
    # tensor's bytes, writing nothing.  Same arguments, same bounds check.
    def _src(self, x, need: int) -> int:
        return self._dst(x, need, "reads")

    def verify_controlled(self, src, nbytes: int | None = None, dedup: int = 1, compress=1,
                          entropy: int = 0, stream=None) -> VerifyResult:
        """Compare `nbytes` at src with fill_controlled's bytes for the same arguments."""
        n = _nbytes(src) if nbytes is None else int(nbytes)
        fn, fd = compress_ratio(compress)
        r = _lib.VerifyRec()
        call("s3dg_verify_controlled", self._h, self._src(src, n), n, int(dedup), fn, fd,
             int(entropy) & (2**64 - 1), self._s(stream), ctypes.byref(r))
        return VerifyResult._of(r)

    def verify_random_data(self, src, nbytes: int | None = None, entropy: int = 0, stream=None) -> VerifyResult:
        """Compare `nbytes` at src with random_data's bytes for the same arguments."""
        n = _nbytes(src) if nbytes is None else int(nbytes)
        r = _lib.VerifyRec()
        call("s3dg_verify_random_data", self._h, self._src(src, n), n, int(entropy) & (2**64 - 1),
             self._s(stream), ctypes.byref(r))
        return VerifyResult._of(r)

    def verify_range(self, src, length: int, blk_lo: int, blk_hi: int, dedup: int = 1,
                     compress=1, entropy: int = 0, stream=None) -> VerifyResult:
        """Blocks [blk_lo, blk_hi) of a `length`-byte object, block blk_lo at src;
        first_offset counts from src."""
        fn, fd = compress_ratio(compress)
        hi = min(int(blk_hi) * BLOCK_SIZE, int(length))
        need = max(0, hi - int(blk_lo) * BLOCK_SIZE)
        r = _lib.VerifyRec()
        call("s3dg_verify_controlled_range", self._h, self._src(src, need), int(length), int(blk_lo),
             int(blk_hi), int(dedup), fn, fd, int(entropy) & (2**64 - 1), self._s(stream), ctypes.byref(r))
        return VerifyResult._of(r)

    def verify_stream(self, src, obj_size: int, n_objs: int, stride: int | None = None,
                      dedup: int = 1, compress=1, seed_base: int = 0, first_obj: int = 0,
                      stream=None) -> VerifyResult:
        """n_objs equal objects as fill_stream lays them out; counts are summed
        over the objects, first_offset counts from src (stride gaps included,
        which are never read)."""
        stride = obj_size if stride is None else stride
        need = (int(n_objs) - 1) * int(stride) + int(obj_size) if n_objs > 0 and obj_size > 0 else 0
        fn, fd = compress_ratio(compress)
        r = _lib.VerifyRec()
        call("s3dg_verify_controlled_stream", self._h, self._src(src, need), int(obj_size), int(stride),
             int(n_objs), int(dedup), fn, fd, int(seed_base) & (2**64 - 1), int(first_obj),
             self._s(stream), ctypes.byref(r))
        return VerifyResult._of(r)

    def fill_batch(self, dst, objects, stream=None) -> None:
        """objects: iterable of (dst_off, size, entropy, dedup, compress).

        The descriptors are checked here first (bounds against `dst`), and the
        library validates them again sub-batch by sub-batch (16 Ki objects,
        doubling) while earlier sub-batches are already enqueued: a call that
        raises on an invalid descriptor past the first sub-batch may have
        written the objects before it (include/s3dlio_gpu.h)."""
        objs = list(objects)
        arr = (ObjDesc * max(1, len(objs)))()
        need = 0
        for k, (off, size, ent, dd, comp) in enumerate(objs):
            fn, fd = compress_ratio(comp)
            arr[k] = ObjDesc(int(off), int(size), int(ent) & (2**64 - 1), int(dd), fn, fd)
            if size:
                need = max(need, int(off) + int(size))
        call("s3dg_fill_controlled_batch", self._h, self._dst(dst, need), arr, len(objs), self._s(stream))

    def verify_batch(self, src, objects, stream=None, per_object: bool = True) -> BatchVerifyResult:
        """The read-side twin of fill_batch: objects is fill_batch's iterable of
        (off, size, entropy, dedup, compress), checked against `src`'s size
        before any launch (ValueError).  The library validates every
        descriptor before its first launch, so a call that raises has read
        nothing.  Descriptors may come in any order, leave gaps and overlap.
        per_object=False asks for the totals only (mismatches is None)."""
        objs = list(objects)
        arr = (ObjDesc * max(1, len(objs)))()
        need = 0
        for k, (off, size, ent, dd, comp) in enumerate(objs):
            fn, fd = compress_ratio(comp)
            arr[k] = ObjDesc(int(off), int(size), int(ent) & (2**64 - 1), int(dd), fn, fd)
            if size:
                need = max(need, int(off) + int(size))
        tot = _lib.VerifyRec()
        per = (_lib.VerifyRec * max(1, len(objs)))() if per_object else None
        call("s3dg_verify_controlled_batch", self._h, self._src(src, need), arr, len(objs), self._s(stream),
             ctypes.byref(tot), per)
        mism = None
        if per_object:
            mism = ()
            if tot.mismatched_bytes:
                # the records as one array: only the dirty ones become Python objects
                a = np.frombuffer(per, dtype=np.uint64, count=3 * len(objs)).reshape(-1, 3)
                mism = tuple((int(k), VerifyResult(int(a[k, 0]), int(a[k, 1]), int(a[k, 2])))
                             for k in np.flatnonzero(a[:, 0]))
        return BatchVerifyResult(VerifyResult._of(tot), len(objs), mism)

    def xoshiro_fill(self, dst, nbytes: int | None = None, chunk_bytes: int = 2 << 20,
                     seed_base: int = 0, stream=None) -> None:
        """Keystream fill, chunk k = Xoshiro256PlusPlus::seed_from_u64(seed_base + k)
        .fill_bytes(chunk) (src/data_formats/npz.rs:376-383)."""
        n = _nbytes(dst) if nbytes is None else int(nbytes)
        call("s3dg_xoshiro_fill", self._h, self._dst(dst, n), n, int(chunk_bytes),
             int(seed_base) & (2**64 - 1), self._s(stream))

    def dgen_fill(self, dst, obj_size: int, blk_lo: int = 0, blk_hi: int | None = None,
                  dedup: int = 1, compress=1, seed: int = 0, stream=None) -> None:
        """DG1 blocks [blk_lo, blk_hi) of an obj_size-byte object (1 MiB blocks)."""
        fn, fd = compress_ratio(compress)
        hi = (obj_size + (1 << 20) - 1) >> 20 if blk_hi is None else blk_hi
        need = max(0, min(int(hi) << 20, int(obj_size)) - (int(blk_lo) << 20))
        call("s3dg_dgen_fill", self._h, self._dst(dst, need), int(obj_size), int(blk_lo), int(hi),
             int(dedup), fn, fd, int(seed) & (2**64 - 1), self._s(stream))

    def dgen_fill_stream(self, dst, obj_size: int, n_objs: int, stride: int | None = None,
                         dedup: int = 1, compress=1, seed_base: int = 0, first_obj: int = 0,
                         stream=None) -> None:
        """n_objs DG1 objects in one launch, object j at dst + j*stride seeded
        object_entropy(seed_base, first_obj + j): the bytes of n_objs dgen_fill calls."""
        stride = obj_size if stride is None else stride
        need = (int(n_objs) - 1) * int(stride) + int(obj_size) if n_objs > 0 and obj_size > 0 else 0
        fn, fd = compress_ratio(compress)
        call("s3dg_dgen_fill_stream", self._h, self._dst(dst, need), int(obj_size), int(stride), int(n_objs),
             int(dedup), fn, fd, int(seed_base) & (2**64 - 1), int(first_obj), self._s(stream))

    # -- keystream verification (synchronous on `stream`) -------------------------
    # The read-side twins of xoshiro_fill / dgen_fill / dgen_fill_stream: the
    # GPU regenerates each chunk's keystream and compares it with the tensor's
    # bytes, writing nothing.  Same arguments, same bounds check; blocks in the
    # result are 4 KiB granules within each object.
    def verify_xoshiro(self, src, nbytes: int | None = None, chunk_bytes: int = 2 << 20,
                       seed_base: int = 0, stream=None) -> VerifyResult:
        """Compare `nbytes` at src with xoshiro_fill's bytes for the same arguments;
        chunk_bytes must be a positive multiple of 4096."""
        n = _nbytes(src) if nbytes is None else int(nbytes)
        r = _lib.VerifyRec()
        call("s3dg_verify_xoshiro", self._h, self._src(src, n), n, int(chunk_bytes),
             int(seed_base) & (2**64 - 1), self._s(stream), ctypes.byref(r))
        return VerifyResult._of(r)

    def verify_dgen(self, src, obj_size: int, blk_lo: int = 0, blk_hi: int | None = None,
                    dedup: int = 1, compress=1, seed: int = 0, stream=None) -> VerifyResult:
        """DG1 blocks [blk_lo, blk_hi) of an obj_size-byte object (1 MiB blocks),
        block blk_lo at src; first_offset counts from src."""
        fn, fd = compress_ratio(compress)
        hi = (obj_size + (1 << 20) - 1) >> 20 if blk_hi is None else blk_hi
        need = max(0, min(int(hi) << 20, int(obj_size)) - (int(blk_lo) << 20))
        r = _lib.VerifyRec()
        call("s3dg_verify_dgen", self._h, self._src(src, need), int(obj_size), int(blk_lo), int(hi),
             int(dedup), fn, fd, int(seed) & (2**64 - 1), self._s(stream), ctypes.byref(r))
        return VerifyResult._of(r)

    def verify_dgen_stream(self, src, obj_size: int, n_objs: int, stride: int | None = None,
                           dedup: int = 1, compress=1, seed_base: int = 0, first_obj: int = 0,
                           stream=None) -> VerifyResult:
        """n_objs DG1 objects as dgen_fill_stream lays them out; counts are summed
        over the objects, first_offset counts from src (stride gaps included,
        which are never read)."""
        stride = obj_size if stride is None else stride
        need = (int(n_objs) - 1) * int(stride) + int(obj_size) if n_objs > 0 and obj_size > 0 else 0
        fn, fd = compress_ratio(compress)
        r = _lib.VerifyRec()
        call("s3dg_verify_dgen_stream", self._h, self._src(src, need), int(obj_size), int(stride), int(n_objs),
             int(dedup), fn, fd, int(seed_base) & (2**64 - 1), int(first_obj), self._s(stream), ctypes.byref(r))
        return VerifyResult._of(r)

    # -- a mixed-size batch of DG1 objects in one call -----------------------------
    def _dgen_descs(self, objects):
        """(descriptor array, n, bytes of the buffer the non-empty objects reach)
        of fill_batch's `objects`, the entropy read as the object's DG1 seed."""
        objs = list(objects)
        arr = (ObjDesc * max(1, len(objs)))()
        need = 0
        for k, (off, size, seed, dd, comp) in enumerate(objs):
            off, size = int(off), int(size)
            if off < 0 or size < 0 or off >= 2**64 or size >= 2**64:
                raise ValueError(f"object {k}: offset and size must fit 64 unsigned bits")
            fn, fd = compress_ratio(comp)
            arr[k] = ObjDesc(off, size, int(seed) & (2**64 - 1), int(dd), fn, fd)
            if size:
                need = max(need, off + size)
        return arr, len(objs), need

    def dgen_fill_batch(self, dst, objects, stream=None) -> None:
        """DG1 objects of mixed sizes in one call: objects is fill_batch's
        iterable of (off, size, seed, dedup, compress), object k being
        dgen_fill's bytes for (size, dedup, compress, seed) at dst + off.
        Bounds are checked against `dst` here (ValueError); the library checks
        every descriptor before its first launch, so a call that raises has
        written nothing."""
        arr, n, need = self._dgen_descs(objects)
        call("s3dg_dgen_fill_batch", self._h, self._dst(dst, need), arr, n, self._s(stream))

    def verify_dgen_batch(self, src, objects, stream=None, per_object: bool = True) -> BatchVerifyResult:
        """The read-side twin of dgen_fill_batch, with verify_batch's result:
        totals (first_offset from src) and, per_object, the dirty objects as
        (index, VerifyResult) with first_offset from the object's first byte.
        Descriptors may come in any order, leave gaps, overlap and repeat."""
        arr, n, need = self._dgen_descs(objects)
        tot = _lib.VerifyRec()
        per = (_lib.VerifyRec * max(1, n))() if per_object else None
        call("s3dg_verify_dgen_batch", self._h, self._src(src, need), arr, n, self._s(stream),
             ctypes.byref(tot), per)
        mism = None
        if per_object:
            mism = ()
            if tot.mismatched_bytes:
                a = np.frombuffer(per, dtype=np.uint64, count=3 * n).reshape(-1, 3)
                mism = tuple((int(k), VerifyResult(int(a[k, 0]), int(a[k, 1]), int(a[k, 2])))
                             for k in np.flatnonzero(a[:, 0]))
        return BatchVerifyResult(VerifyResult._of(tot), n, mism)

    # -- measurement (read-only) ---------------------------------------------------
    # How many blocks of `block_bytes` are distinct and how many bytes are zero
    # (hist=True: the byte histogram too), whatever wrote the bytes: no seed is
    # needed.  Blocks are cut from each object's start; a ragged last block is a
    # block of its own.
    def measurer(self, block_bytes: int = 4096, hist: bool = False) -> "Measure":
        """An accumulating handle: add / add_stream / add_range on any stream,
        then result()."""
        return Measure(self, block_bytes, hist)

    def measure(self, src, nbytes: int | None = None, block_bytes: int = 4096, hist: bool = False,
                stream=None) -> MeasureResult:
        """One object of `nbytes` at src."""
        with self.measurer(block_bytes, hist) as m:
            m.add(src, nbytes, stream=stream)
            return m.result()

    def measure_stream(self, src, obj_size: int, n_objs: int, stride: int | None = None,
                       block_bytes: int = 4096, hist: bool = False, stream=None) -> MeasureResult:
        """n_objs equal objects as fill_stream lays them out; stride gaps are never read."""
        with self.measurer(block_bytes, hist) as m:
            m.add_stream(src, obj_size, n_objs, stride, stream=stream)
            return m.result()

    def measure_batch(self, src, objects, block_bytes: int = 4096, hist: bool = False,
                      stream=None) -> MeasureResult:
        """A mixed-size batch as fill_batch lays it out (Measure.add_batch); gaps are never read."""
        with self.measurer(block_bytes, hist) as m:
            m.add_batch(src, objects, stream=stream)
            return m.result()

    # -- content-defined chunking (read-only) ------------------------------------
    # How much of a payload is distinct to a store that cuts chunks where a
    # rolling hash over 32 bytes says so, between min_bytes and max_bytes
    # (avg_bytes: a power of two).  Every object is chunked on
    # its own from its first byte.
    def chunker(self, min_bytes: int = CHUNK_DEFAULTS[0], avg_bytes: int = CHUNK_DEFAULTS[1],
                max_bytes: int = CHUNK_DEFAULTS[2]) -> "Chunker":
        """An accumulating handle: add / add_stream on any stream, then result()."""
        return Chunker(self, min_bytes, avg_bytes, max_bytes)

    def measure_chunks(self, src, nbytes: int | None = None, min_bytes: int = CHUNK_DEFAULTS[0],
                       avg_bytes: int = CHUNK_DEFAULTS[1], max_bytes: int = CHUNK_DEFAULTS[2],
                       stream=None) -> ChunkResult:
        """One object of `nbytes` at src."""
        with self.chunker(min_bytes, avg_bytes, max_bytes) as h:
            h.add(src, nbytes, stream=stream)
            return h.result()

    def measure_chunks_stream(self, src, obj_size: int, n_objs: int, stride: int | None = None,
                              min_bytes: int = CHUNK_DEFAULTS[0], avg_bytes: int = CHUNK_DEFAULTS[1],
                              max_bytes: int = CHUNK_DEFAULTS[2], stream=None) -> ChunkResult:
        """n_objs equal objects as fill_stream lays them out; stride gaps are never read."""
        with self.chunker(min_bytes, avg_bytes, max_bytes) as h:
            h.add_stream(src, obj_size, n_objs, stride, stream=stream)
            return h.result()

    def measure_chunks_batch(self, src, objects, min_bytes: int = CHUNK_DEFAULTS[0],
                             avg_bytes: int = CHUNK_DEFAULTS[1], max_bytes: int = CHUNK_DEFAULTS[2],
                             stream=None) -> ChunkResult:
        """A mixed-size batch as fill_batch lays it out (Chunker.add_batch); gaps are never read."""
        with self.chunker(min_bytes, avg_bytes, max_bytes) as h:
            h.add_batch(src, objects, stream=stream)
            return h.result()

    # -- LZ4 compressed size per store block (read-only) ---------------------------
    # The bytes a payload takes in a store that compresses independent blocks
    # of `block_bytes` (a multiple of 4096 up to 65536) with a greedy LZ4
    # (DESIGN.md §5.12).  Blocks are cut from each object's start.
    def lz_measurer(self, block_bytes: int = 65536) -> "LzMeasure":
        """An accumulating handle: add / add_stream / add_range on any stream,
        then result()."""
        return LzMeasure(self, block_bytes)

    def measure_lz(self, src, nbytes: int | None = None, block_bytes: int = 65536, stream=None) -> LzResult:
        """One object of `nbytes` at src."""
        with self.lz_measurer(block_bytes) as m:
            m.add(src, nbytes, stream=stream)
            return m.result()

    def measure_lz_stream(self, src, obj_size: int, n_objs: int, stride: int | None = None,
                          block_bytes: int = 65536, stream=None) -> LzResult:
        """n_objs equal objects as fill_stream lays them out; stride gaps are never read."""
        with self.lz_measurer(block_bytes) as m:
            m.add_stream(src, obj_size, n_objs, stride, stream=stream)
            return m.result()

    def measure_lz_batch(self, src, objects, block_bytes: int = 65536, stream=None) -> LzResult:
        """A mixed-size batch as fill_batch lays it out (LzMeasure.add_batch); gaps are never read."""
        with self.lz_measurer(block_bytes) as m:
            m.add_batch(src, objects, stream=stream)
            return m.result()

    # -- checksums of a mixed-size batch (read-only) --------------------------------
    def crc32_batch(self, src, objects, stream=None, out=None):
        """The CRC-32 (zlib.crc32) of every object of a mixed-size batch in one
        call: objects is fill_batch's iterable, of which the first two fields
        (off, size, ...) are used, or a uint64 numpy array of shape (n, 2), as
        Measure.add_batch takes them.  Spans may come in any order, leave
        gaps, overlap and repeat; an empty one gives 0.  off + size is checked
        against `src`'s size before any launch (ValueError).  Returns a
        numpy uint32 array of n values after waiting for them; with `out`, a
        uint32 or int32 tensor of n elements on this context's device, the
        values are stored there in stream order and the call returns None
        without waiting."""
        arr, n, need = _spans(objects)
        p = self._src(src, need)
        if out is None:
            res = np.zeros(n, np.uint32)
            call("s3dg_crc32_batch", self._h, p, arr, n, self._s(stream),
                 res.ctypes.data_as(ctypes.POINTER(c_u32)))
            return res
        if not hasattr(out, "data_ptr") or str(out.dtype) not in ("torch.uint32", "torch.int32"):
            raise ValueError("out must be a uint32 or int32 tensor")
        if int(out.numel()) != n:
            raise ValueError(f"out holds {int(out.numel())} elements, the batch has {n} objects")
        call("s3dg_crc32_batch_async", self._h, p, arr, n, self._s(stream), self._dst(out, 4 * n))
        return None

    # -- TFRecord shards framed and checked in HBM --------------------------------
    def tfrecord_frame_batch(self, src, dst, shards, index=None, stream=None) -> None:
        """Frames every shard of the list in one device call.  Each shard is
        (src_off, dst_off, records, record_size[, idx_off]): records *
        record_size payload bytes at src + src_off become the stream
        build_tfrecord(records, record_size, payload) at dst + dst_off, and,
        with `index`, 16 bytes per record <offset, length> at index + idx_off.
        Offsets are multiples of 16; shards may come in any order, be empty
        and share a source; streams must not overlap each other or a source.
        The spans are checked against the tensors' sizes before any launch
        (ValueError).  Ordered on `stream`; returns without waiting."""
        arr, n, need_src, need_dst, need_idx = _tfr_shards(shards)
        p_idx = None if index is None else self._dst(index, need_idx)
        call("s3dg_tfrecord_frame_batch", self._h, self._src(src, need_src), self._dst(dst, need_dst), p_idx, arr, n,
             self._s(stream))

    def tfrecord_check_batch(self, src, shards, stream=None, per_shard: bool = True) -> TfRecordResult:
        """The read-side twin of tfrecord_frame_batch over the same shards, of
        which dst_off, records and record_size are used: the stream of a
        shard is at src + dst_off.  Per record the length field, the length
        CRC and the data's CRC against the footer.  Synchronous on `stream`;
        writes nothing.  per_shard=False asks for the totals only."""
        arr, n, _, need, _ = _tfr_shards(shards)
        tot = _lib.TfrRec()
        per = (_lib.TfrRec * max(1, n))() if per_shard else None
        call("s3dg_tfrecord_check_batch", self._h, self._src(src, need), arr, n, self._s(stream), ctypes.byref(tot), per)
        bad = None
        if per_shard:
            bad = tuple((k, TfRecordResult._of(per[k], None)) for k in range(n) if per[k].bad_records) \
                if tot.bad_records else ()
        return TfRecordResult._of(tot, bad)

    # -- TFRecord shards of records of any length; streams nobody has described -----
    def tfrecord_frame_var_batch(self, src, dst, shards, index=None, stream=None) -> None:
        """tfrecord_frame_batch for records of any length.  Each shard is
        (src_off, dst_off, lengths[, idx_off]): lengths (any integer sequence
        or numpy array) are the payload bytes of its records, packed back to
        back at src + src_off; record i is framed at dst + dst_off + P_i + 16 i
        (P_i: the lengths before it) and, with `index`, its entry
        <P_i + 16 i, 16 + len_i> is at index + idx_off + 16 i.  Offsets are
        multiples of 16; shards may come in any order, be empty and share a
        source.  The spans are checked against the tensors' sizes before any
        launch (ValueError).  Ordered on `stream`; returns without waiting."""
        arr, n, lens, need_src, need_dst, need_idx = _tfr_var_shards(shards)
        p_idx = None if index is None else self._dst(index, need_idx)
        call("s3dg_tfrecord_frame_var_batch", self._h, self._src(src, need_src), self._dst(dst, need_dst), p_idx, arr, n,
             lens.ctypes.data_as(ctypes.POINTER(_lib.c_u64)), len(lens), self._s(stream))

    def tfrecord_check_var_batch(self, src, shards, stream=None, per_shard: bool = True) -> TfRecordResult:
        """The read-side twin of tfrecord_frame_var_batch over the same shards,
        of which dst_off and lengths are used: the stream of a shard is at
        src + dst_off.  Per record the length field against the given length,
        the length CRC and the data's CRC against the footer.  Synchronous on
        `stream`; writes nothing.  per_shard=False asks for the totals only."""
        arr, n, lens, _, need, _ = _tfr_var_shards(shards)
        tot = _lib.TfrRec()
        per = (_lib.TfrRec * max(1, n))() if per_shard else None
        call("s3dg_tfrecord_check_var_batch", self._h, self._src(src, need), arr, n,
             lens.ctypes.data_as(ctypes.POINTER(_lib.c_u64)), len(lens), self._s(stream), ctypes.byref(tot), per)
        bad = None
        if per_shard:
            bad = tuple((k, TfRecordResult._of(per[k], None)) for k in range(n) if per[k].bad_records) \
                if tot.bad_records else ()
        return TfRecordResult._of(tot, bad)

    def tfrecord_index_batch(self, src, streams, index, stream=None) -> list:
        """The index of framed streams nobody has described, in one device
        call: each stream is (off, nbytes, idx_off, max_records), nbytes at
        src + off (any byte offset), and gets its entries <offset from the
        stream's start, 16 + len>, at most max_records of them, at
        index + idx_off (a multiple of 16).  index_entries_from_bytes'
        semantics: fewer than 12 bytes left end the walk silently, a record
        that does not fit ends it as "truncated" with the entries before it
        kept; "full" means max_records entries are written and more follows
        (resume at off + stop_offset).  Synchronous on `stream`.  Returns a
        TfRecordWalk per stream."""
        rows = [tuple(int(x) for x in st) for st in streams]
        if any(len(st) != 4 for st in rows):
            raise ValueError("a stream is (off, nbytes, idx_off, max_records)")
        if any(x < 0 or x >= 2**64 for st in rows for x in st):
            raise ValueError("stream fields must fit 64 unsigned bits")
        n = len(rows)
        arr = (_lib.TfrStream * max(1, n))()
        need_src = need_idx = 0
        for k, (off, nbytes, idx_off, cap) in enumerate(rows):
            arr[k] = _lib.TfrStream(off, nbytes, idx_off, cap)
            need_src = max(need_src, off + nbytes)
            need_idx = max(need_idx, idx_off + 16 * min(cap, nbytes // 16))
        res = (_lib.TfrWalkRec * max(1, n))()
        call("s3dg_tfrecord_index_batch", self._h, self._src(src, need_src), self._dst(index, need_idx), arr, n,
             self._s(stream), res)
        return [TfRecordWalk._of(res[k]) for k in range(n)]

    def tfrecord_scan(self, src, streams, stream=None):
        """"I only have bytes": streams is an iterable of (off, nbytes) with
        off a multiple of 16.  Walks every stream (tfrecord_index_batch with
        room for every record the bytes could hold), copies the entries back,
        and checks the records found (tfrecord_check_var_batch with lengths
        size - 16).  Returns (walks, index arrays, TfRecordResult): one
        TfRecordWalk and one uint64 array of shape (records, 2) per stream."""
        t = _lib.torch
        spans = [(int(off), int(nbytes)) for off, nbytes in streams]
        idx_off, at = [], 0
        for _, nbytes in spans:
            idx_off.append(at)
            at += 16 * (nbytes // 16)
        index = t.empty(max(16, at), dtype=t.uint8, device=f"cuda:{self.device}")
        walks = self.tfrecord_index_batch(src, [(off, nbytes, io, nbytes // 16) for (off, nbytes), io in zip(spans, idx_off)],
                                          index, stream=stream)
        host = index.cpu().numpy()
        entries = [host[io:io + 16 * w.records].view("<u8").reshape(-1, 2).astype(np.uint64) for io, w in zip(idx_off, walks)]
        shards = [(0, off, e[:, 1] - np.uint64(16)) for (off, _), e in zip(spans, entries)]
        return walks, entries, self.tfrecord_check_var_batch(src, shards, stream=stream)

    def write_ceiling(self, dst, nbytes: int | None = None, pattern: int = 0xA5A5A5A5,
                      stream=None) -> None:
        n = _nbytes(dst) if nbytes is None else int(nbytes)
        call("s3dg_write_ceiling", self._h, self._dst(dst, n), n, int(pattern), self._s(stream))

    def write_ceiling_tiled(self, dst, nbytes: int | None = None, pattern: int = 0xA5A5A5A5,
                            stream=None) -> None:
        """Store-only kernel in the tiled fill shape (batch knobs + trailing record loads)."""
        n = _nbytes(dst) if nbytes is None else int(nbytes)
        call("s3dg_write_ceiling_tiled", self._h, self._dst(dst, n), n, int(pattern), self._s(stream))

    def write_ceiling_fill(self, dst, nbytes: int | None = None, pace: int = 0, stream=None) -> None:
        """The tiled fill itself with the PRNG chain and window patches compiled
        out (s3dg_write_ceiling_fill): the fill's own store-only bound; `pace`
        delays wave 0 by pace x 128 cycles where the fill plans its block."""
        n = _nbytes(dst) if nbytes is None else int(nbytes)
        call("s3dg_write_ceiling_fill", self._h, self._dst(dst, n), n, int(pace), self._s(stream))

    def sync(self, stream=None) -> None:
        call("s3dg_sync", self._h, 0 if stream is None else _stream(stream))

    def release_stream(self, stream) -> None:
        """Drain `stream` and free this context's launch state for it (tile
        maps, batch staging; s3dg_stream_release).  Call before a stream the
        context launched on goes away."""
        call("s3dg_stream_release", self._h, _stream(stream))

    def stream_state_count(self) -> int:
        n = ctypes.c_uint64()
        call("s3dg_stream_state_count", self._h, ctypes.byref(n))
        return n.value


class _Accum:
    """What Measure, LzMeasure and Chunker share: a C handle s3dg_<_sym>_* that
    accumulates over calls and streams.  A subclass names the symbol prefix
    (_sym), the result record of _lib (_rec), turns one into its result
    (_result) and creates the handle with _open(*create_args)."""
    _sym = _rec = None

    def _open(self, ctx: Context, *args) -> None:
        self._ctx = ctx
        h = c_vp()
        call(f"s3dg_{self._sym}_create", ctx._h, *args, ctypes.byref(h))
        self._h = h

    def add(self, src, nbytes: int | None = None, stream=None) -> None:
        """One object of `nbytes` at src."""
        n = _nbytes(src) if nbytes is None else int(nbytes)
        self.add_stream(src, n, 1, stride=0, stream=stream)   # one object: no stride to align

    def add_stream(self, src, obj_size: int, n_objs: int, stride: int | None = None, stream=None) -> None:
        """n_objs objects of obj_size bytes, object j at src + j*stride."""
        stride = obj_size if stride is None else stride
        need = (int(n_objs) - 1) * int(stride) + int(obj_size) if n_objs > 0 and obj_size > 0 else 0
        call(f"s3dg_{self._sym}_add_stream", self._h, self._ctx._src(src, need), int(obj_size), int(stride),
             int(n_objs), self._ctx._s(stream))

    def add_batch(self, src, objects, stream=None) -> None:
        """A mixed-size batch in one asynchronous add: every object measured
        from its own first byte, the sum of the per-object adds exactly.
        objects: an iterable whose items start with (off, size), so
        fill_batch's 5-tuples pass unchanged, or a uint64 numpy array of shape
        (n, 2).  Spans may come in any order, leave gaps, overlap and repeat;
        empty ones contribute nothing.  off + size is checked against `src`'s
        size before any launch (ValueError)."""
        arr, n, need = _spans(objects)
        call(f"s3dg_{self._sym}_add_batch", self._h, self._ctx._src(src, need), arr, n, self._ctx._s(stream))

    def result(self):
        r = self._rec()
        call(f"s3dg_{self._sym}_get", self._h, ctypes.byref(r))
        return self._result(r)

    def reset(self) -> None:
        call(f"s3dg_{self._sym}_reset", self._h)

    def close(self) -> None:
        if getattr(self, "_h", None):
            call(f"s3dg_{self._sym}_destroy", self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BlockAccum(_Accum):
    """An _Accum over blocks of self.block_bytes: ranges of whole blocks too."""

    def add_range(self, src, obj_size: int, blk_lo: int, blk_hi: int, stream=None) -> None:
        """Blocks [blk_lo, blk_hi) (units of block_bytes) of one obj_size-byte
        object, block blk_lo at src."""
        hi = min(int(blk_hi) * self.block_bytes, int(obj_size))
        need = max(0, hi - int(blk_lo) * self.block_bytes)
        call(f"s3dg_{self._sym}_add_range", self._h, self._ctx._src(src, need), int(obj_size), int(blk_lo),
             int(blk_hi), self._ctx._s(stream))


class Measure(_BlockAccum):
    """s3dg_measure: a measurement that accumulates over calls and streams
    (Context.measurer).  The adds are asynchronous on their stream and ordered
    like a fill, so a following launch on the same stream may overwrite the
    buffer; result() waits for them and leaves the handle unchanged."""
    _sym, _rec = "measure", _lib.MeasureRec

    def __init__(self, ctx: Context, block_bytes: int = 4096, hist: bool = False):
        self.block_bytes = int(block_bytes)
        self.hist = bool(hist)
        self._open(ctx, self.block_bytes, 1 if hist else 0)

    def _result(self, r) -> MeasureResult:
        return MeasureResult._of(r, self.hist)


class LzMeasure(_BlockAccum):
    """s3dg_lz: an LZ4 size measurement that accumulates over calls and streams
    (Context.lz_measurer).  The adds are asynchronous on their stream and
    ordered like a fill, so a following launch on the same stream may overwrite
    the buffer; result() waits for them and leaves the handle unchanged."""
    _sym, _rec, _result = "lz", _lib.LzRec, staticmethod(LzResult._of)

    def __init__(self, ctx: Context, block_bytes: int = 65536):
        self.block_bytes = int(block_bytes)
        self._open(ctx, self.block_bytes)


class Chunker(_Accum):
    """s3dg_chunks: a content-defined chunking analysis that accumulates over
    calls and streams (Context.chunker).  The adds are asynchronous on their
    stream and ordered like a fill; every add holds whole objects.  result()
    waits for them and leaves the handle unchanged."""
    _sym, _rec, _result = "chunks", _lib.ChunkRec, staticmethod(ChunkResult._of)

    def __init__(self, ctx: Context, min_bytes: int = CHUNK_DEFAULTS[0], avg_bytes: int = CHUNK_DEFAULTS[1],
                 max_bytes: int = CHUNK_DEFAULTS[2]):
        self.min_bytes, self.avg_bytes, self.max_bytes = int(min_bytes), int(avg_bytes), int(max_bytes)
        self._open(ctx, self.min_bytes, self.avg_bytes, self.max_bytes)

    def time_passes(self, on: bool = True) -> None:
        """HIP events around the three passes of every following add (pass_seconds)."""
        call("s3dg_chunks_set_option", self._h, _CHUNKS_TIME_PASSES, 1 if on else 0)

    def gear_table(self, on: bool = True) -> None:
        """The candidate pass's G from LDS (default) or computed per byte; same results."""
        call("s3dg_chunks_set_option", self._h, _CHUNKS_GEAR_TABLE, 1 if on else 0)

    def pass_seconds(self) -> tuple[float, float, float]:
        """Candidate, cut and fingerprint pass times of the latest timed add (waits for it)."""
        t = (ctypes.c_double * 3)()
        call("s3dg_chunks_pass_seconds", self._h, t)
        return float(t[0]), float(t[1]), float(t[2])


def xoshiro_jump(state, n: int) -> list[int]:
    """Host jump-ahead of a Xoshiro256 state by n steps (the kernels' method)."""
    s = (ctypes.c_uint64 * 4)(*[int(v) & (2**64 - 1) for v in state])
    call("s3dg_xoshiro_jump", s, int(n))
    return list(s)


def device_count() -> int:
    n = ctypes.c_int()
    call("s3dg_device_count", ctypes.byref(n))
    return n.value


def host_slots() -> list[int]:
    """Devices of the host-buffer drop-ins' slots (include/s3dlio_gpu.h): one
    per visible GPU unless S3DLIO_GPU_DEVICE / S3DLIO_GPU_DEVICES say otherwise."""
    n = ctypes.c_int()
    call("s3dg_host_slot_count", ctypes.byref(n))
    out = []
    for k in range(n.value):
        d = ctypes.c_int()
        call("s3dg_host_slot_device", k, ctypes.byref(d))
        out.append(d.value)
    return out


def host_context(slot: int = -1) -> Context:
    """A host slot's context (borrowed: owned by the pool); slot < 0 takes the
    next slot round-robin."""
    h = c_vp()
    call("s3dg_host_slot_context", int(slot), ctypes.byref(h))
    d = ctypes.c_int()
    call("s3dg_ctx_device", h, ctypes.byref(d))
    return Context._borrow(h.value, d.value)


def parse_devices(pin: str | None, lst: str | None, ndev: int, local_rank: str | None = None,
                  world_size: str | None = None) -> list[int]:
    """The slot device list for given env values (pure; s3dg_host_parse_devices_env):
    S3DLIO_GPU_DEVICE, S3DLIO_GPU_DEVICES, LOCAL_RANK, WORLD_SIZE."""
    out = (ctypes.c_int * 64)()
    n = ctypes.c_int()
    enc = lambda v: v.encode() if v is not None else None  # noqa: E731
    call("s3dg_host_parse_devices_env", enc(pin), enc(lst), enc(local_rank), enc(world_size), int(ndev), out, 64,
         ctypes.byref(n))
    return list(out[:n.value])
