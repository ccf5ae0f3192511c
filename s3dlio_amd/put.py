"""PUT of synthetic objects to file:// targets, one payload per object.

Mirrors the reference's put surface:
    put(prefix, num, template=None, max_in_flight=64, size=None, ...)
                                    src/python_api/python_core_api.rs:777-818
    build_uri_list(prefix, template, num)          python_core_api.rs:657-691
    put_objects_with_random_data_and_type(uris, size, max_in_flight, config)
                                    src/s3_utils.rs:1717-1750
The work runs in the native pipeline s3dg_put_objects (s3dg_put.cpp): GPU
generation + GPU CRC-32 -> pinned host ring -> writer threads.

Deliberate differences from the reference:
  * object j gets its own payload (entropy object_entropy(seed_base, j));
    the reference PUTs one generated buffer to every URI (s3_utils.rs:1741);
  * only file:// targets: the S3 / Azure / GCS back ends are out of scope;
  * the call returns per-object CRC-32s (crc32fast of each file's bytes, the
    StreamingDataWriter checksum, src/streaming_writer.rs:183-186) and stats.
Payload kinds follow generate_object's dispatch (data_gen.rs:29-94):
use_controlled (dedup != 1 or compress != 1) -> the DG1 stream, otherwise the
generate_random_data layout; payload="controlled" selects the
fill_controlled_data layout instead (the benchmark kernel).
"""
from __future__ import annotations

import ctypes
import threading
import os
import time
from dataclasses import dataclass, field

from ._lib import PutStats, call
from .device import compress_ratio
from .objects import Config, DataGenMode, ObjectType

DEFAULT_OBJECT_SIZE = 20 * 1024 * 1024          # src/s3_utils.rs:217
_PAYLOADS = {"controlled": 0, "random": 1, "dgen": 2}


def build_uri_list(prefix: str, template: str, num: int) -> tuple[str, list[str]]:
    """python_core_api.rs:657-691: scheme://bucket/key_prefix/ + template with
    the first "{}" -> index and the second "{}" -> num."""
    k = prefix.find("://")
    if k < 0:
        raise ValueError("URI must contain scheme (e.g., s3://, az://, file://)")
    scheme, rest = prefix[:k + 3], prefix[k + 3:]
    bucket, _, key_prefix = rest.partition("/")
    if key_prefix and not key_prefix.endswith("/"):
        key_prefix += "/"
    uris = []
    for i in range(num):
        name = template.replace("{}", str(i), 1).replace("{}", str(num), 1)
        uris.append(f"{scheme}{bucket}/{key_prefix}{name}")
    return bucket, uris


def _uri_to_path(uri: str) -> str:
    """FileSystemObjectStore::uri_to_path (src/file_store.rs:287-295)."""
    if not uri.startswith("file://"):
        raise ValueError(f"only file:// targets are built in this drop-in (got {uri!r}); "
                         "object-store back ends are out of scope")
    return uri[7:]


@dataclass
class PutResult:
    checksums: list[int] = field(default_factory=list)   # CRC-32 of each file as written
    objects: int = 0
    bytes: int = 0
    seconds: float = 0.0
    gpu_seconds: float = 0.0
    seed_base: int = 0

    def checksum_str(self, j: int) -> str:
        """StreamingDataWriter::checksum format (streaming_writer.rs:183-186)."""
        return f"crc32c:{self.checksums[j]:08x}"


def _contexts(devices):
    """Contexts for `devices`: None / "all" = every visible GPU, else a list of
    device indices (repeats give several lanes on one GPU)."""
    from .device import Context
    if devices is None or devices == "all":
        n = ctypes.c_int()
        call("s3dg_device_count", ctypes.byref(n))
        devices = list(range(max(1, n.value)))
    ctxs = []
    for d in devices:
        key = (int(d), sum(1 for c in ctxs if c.device == int(d)))
        with _LANE_LOCK:
            if key not in _LANE_CTX:
                _LANE_CTX[key] = Context(int(d))
            ctxs.append(_LANE_CTX[key])
    return ctxs


_LANE_CTX: dict = {}      # (device, lane) -> Context, kept for the process
_LANE_LOCK = threading.Lock()


def put_objects(uris, size: int, max_in_flight: int = 64, config: Config | None = None,
                seed: int | None = None, payload: str | None = None, context=None,
                devices=None) -> PutResult:
    """Generate one payload per URI on the GPU(s) and write the files.
    `context` pins the call to one GPU; otherwise `devices` (default: every
    visible GPU) each take a contiguous range of the objects.  Output files
    and checksums do not depend on the GPU count."""
    import numpy as np
    cfg = config or Config.new_with_defaults(ObjectType.RAW, 1, size, 1, 1)
    if cfg.object_type == ObjectType.HDF5:
        raise ValueError("HDF5 format is not available in this build")
    paths = [_uri_to_path(u) for u in uris]
    if payload is None:
        payload = "dgen" if cfg.use_controlled else "random"
    kind = _PAYLOADS[payload]
    dedup = max(1, int(cfg.dedup_factor))
    fn, fd = compress_ratio(max(1, int(cfg.compress_factor)))
    if seed is None:   # the reference's time entropy
        seed = (time.time_ns() ^ (os.getpid() << 32)) & (2**64 - 1)
    n = len(paths)
    arr = (ctypes.c_char_p * max(1, n))(*[p.encode() for p in paths])
    crcs = np.zeros(max(1, n), np.uint32)
    st = PutStats()
    ctxs = [context] if context is not None else _contexts(devices)
    harr = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    call("s3dg_put_objects_multi", harr, len(ctxs), arr, n, int(size), int(cfg.object_type), kind, dedup,
         fn, fd, int(seed) & (2**64 - 1), int(max_in_flight), int(crcs.ctypes.data), ctypes.byref(st))
    return PutResult([int(c) for c in crcs[:n]], st.objects, st.bytes, st.seconds, st.gpu_seconds,
                     int(seed) & (2**64 - 1))


@dataclass
class VerifyObjectsResult:
    """What verify_objects found: (object index, VerifyResult) of every object
    that is not clean, in index order, and the totals over all objects."""
    mismatches: list = field(default_factory=list)
    objects: int = 0              # objects checked
    bytes: int = 0                # bytes read and compared
    mismatched_objects: int = 0
    mismatched_bytes: int = 0
    mismatched_blocks: int = 0

    @property
    def ok(self) -> bool:
        return not self.mismatches


_VERIFY_GROUP_BYTES = 64 << 20   # objects are read and checked in groups of about this size


def verify_objects(uris, size: int, config: Config | None = None, seed: int = 0,
                   payload: str | None = None, context=None) -> VerifyObjectsResult:
    """Read-side partner of put_objects for file:// RAW objects: read the files
    back and check on the GPU that object j holds the payload
    put_objects(uris, size, config=config, seed=seed, payload=payload) wrote
    for it ("controlled" or "random"; same defaults as put_objects).

    Files are read in groups into pinned host memory, copied to a device chunk
    and checked there (Context.verify_stream with first_obj = the group's first
    index; one verify_random_data per object for "random").  A group that is
    not clean is checked again object by object to name the objects.  A file
    of the wrong length is a mismatch of that object, not an exception: the
    whole 4 KiB blocks of the bytes both have are compared, every missing or
    excess byte counts as mismatched, and first_offset is the lowest differing
    offset, at most min(actual, expected) length.  A missing file raises.
    The DG1 payload ("dgen") and framed object types (NPZ, TFRecord) are not
    supported: there is no verify kernel for the keystream layouts."""
    import numpy as np
    from ._lib import c_vp, lib
    from .device import BLOCK_SIZE, Context, VerifyResult, object_entropy
    cfg = config or Config.new_with_defaults(ObjectType.RAW, 1, size, 1, 1)
    if payload is None:
        payload = "dgen" if cfg.use_controlled else "random"
    if payload not in _PAYLOADS:
        raise ValueError(f"unknown payload {payload!r}")
    if payload == "dgen":
        raise ValueError('verify_objects checks payload "controlled" or "random" only: the DG1 ("dgen") '
                         "payload has no verify kernel")
    if cfg.object_type != ObjectType.RAW:
        raise ValueError("verify_objects checks RAW objects only: framed object types (NPZ, TFRecord, HDF5) "
                         "are not supported")
    paths = [_uri_to_path(u) for u in uris]
    size = int(size)
    seed = int(seed) & (2**64 - 1)
    dedup = max(1, int(cfg.dedup_factor))
    compress = max(1, int(cfg.compress_factor))
    out = VerifyObjectsResult()
    n = len(paths)
    if n == 0 or size == 0:
        for j, p in enumerate(paths):   # empty objects: only the length can be wrong
            actual = os.path.getsize(p)
            out.objects += 1
            if actual:
                out.mismatches.append((j, VerifyResult(actual, 1, 0)))
        _verify_totals(out)
        return out
    ctx = context if context is not None else _contexts([0])[0]
    stride = (size + 15) & ~15
    group = max(1, min(n, _VERIFY_GROUP_BYTES // stride))
    nb = (size + BLOCK_SIZE - 1) // BLOCK_SIZE

    def check(dev, j, k):
        """Objects [j, j + k) at dev."""
        if payload == "controlled":
            return ctx.verify_stream(dev, size, k, stride, dedup, compress, seed, j, stream=st.value)
        tot = [0, 0, None]
        for q in range(k):
            r = ctx.verify_random_data(dev + q * stride, size, object_entropy(seed, j + q), stream=st.value)
            if not r.ok:
                tot[0] += r.mismatched_bytes
                tot[1] += r.mismatched_blocks
                tot[2] = q * stride + r.first_offset if tot[2] is None else tot[2]
        return VerifyResult(tot[0], tot[1], tot[2])

    host, dev, st = c_vp(), c_vp(), c_vp()
    call("s3dg_host_alloc_pinned", group * stride, ctypes.byref(host))
    try:
        call("s3dg_device_alloc", ctx._h, group * stride, ctypes.byref(dev))
        call("s3dg_stream_create", ctx._h, ctypes.byref(st))
        pinned = np.frombuffer((ctypes.c_uint8 * (group * stride)).from_address(host.value), np.uint8)
        for j0 in range(0, n, group):
            k = min(group, n - j0)
            actual = []
            for q in range(k):
                with open(paths[j0 + q], "rb", buffering=0) as f:
                    got = 0
                    slot = pinned[q * stride:q * stride + size]
                    while got < size:
                        m = f.readinto(slot[got:])
                        if not m:
                            break
                        got += m
                    actual.append(os.fstat(f.fileno()).st_size)
                out.bytes += got
            out.objects += k
            call("s3dg_h2d_async", ctx._h, dev, host, k * stride, st)
            if all(a == size for a in actual) and check(dev.value, j0, k).ok:
                continue
            for q in range(k):   # name the objects of a group that is not clean
                a = actual[q]
                if a >= size:
                    r = check(dev.value + q * stride, j0 + q, 1)
                    if a > size:   # excess bytes: one more block
                        r = VerifyResult(r.mismatched_bytes + a - size, r.mismatched_blocks + 1,
                                         size if r.ok else r.first_offset)
                else:              # short: its whole blocks, then every missing byte
                    full = a // BLOCK_SIZE
                    if payload == "controlled":
                        r = ctx.verify_range(dev.value + q * stride, size, 0, full, dedup, compress,
                                             object_entropy(seed, j0 + q), stream=st.value)
                    else:
                        r = ctx.verify_random_data(dev.value + q * stride, full * BLOCK_SIZE,
                                                   object_entropy(seed, j0 + q), stream=st.value)
                    r = VerifyResult(r.mismatched_bytes + size - a, r.mismatched_blocks + nb - full,
                                     a if r.ok else r.first_offset)
                if not r.ok:
                    out.mismatches.append((j0 + q, r))
    finally:
        if st.value:
            lib.s3dg_stream_destroy(ctx._h, st)
        if dev.value:
            lib.s3dg_device_free(ctx._h, dev)
        lib.s3dg_host_free_pinned(host)
    _verify_totals(out)
    return out


def _verify_totals(out: VerifyObjectsResult) -> None:
    out.mismatched_objects = len(out.mismatches)
    out.mismatched_bytes = sum(r.mismatched_bytes for _, r in out.mismatches)
    out.mismatched_blocks = sum(r.mismatched_blocks for _, r in out.mismatches)


def put_objects_with_random_data_and_type(uris, size: int, max_in_flight: int, config: Config,
                                          seed: int | None = None) -> PutResult:
    """src/s3_utils.rs:1717-1724 (per-object payloads; see module docstring)."""
    return put_objects(uris, size, max_in_flight, config, seed)


def put(prefix: str, num: int, template: str | None = None, max_in_flight: int = 64,
        size: int | None = None, should_create_bucket: bool = False, object_type: str = "zeros",
        dedup_factor: int = 1, compress_factor: int = 1, data_gen_algorithm: str = "random",
        data_gen_mode: str = "streaming", chunk_size: int = 262144, seed: int | None = None,
        devices=None) -> None:
    """python_core_api.rs:777-818.  should_create_bucket: parents are always
    created for file:// (file_store.rs:562-564); data_gen_algorithm: only
    "random" exists (prand deprecated, :696-701)."""
    sz = DEFAULT_OBJECT_SIZE if size is None else int(size)
    _, uris = build_uri_list(prefix, template or "object-{}", num)
    jobs = min(max_in_flight, num)
    mode = DataGenMode.SINGLE_PASS if data_gen_mode.lower() in (
        "single-pass", "single_pass", "singlepass") else DataGenMode.STREAMING
    cfg = (Config.new_with_defaults(ObjectType.from_str(object_type), 1, sz, dedup_factor,
                                    compress_factor)
           .with_data_gen_mode(mode).with_chunk_size(chunk_size))
    put_objects(uris, sz, jobs, cfg, seed, devices=devices)
