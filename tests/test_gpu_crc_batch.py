"""GPU: the CRC-32 of every object of a mixed-size batch in one call
(s3dg_crc32_batch, s3dg_crc32_batch_async, Context.crc32_batch; DESIGN.md
§5.4.1).

Every value is exact.  The judge is zlib.crc32 of a host copy of the object's
bytes; the second judge, for the large cases, is s3dg_crc32 on the same device
bytes, one call per object.  The call has no sub-launch cut (the region
kernel's grid is sized to the chip and loops, the fold's grid holds 2^32
objects), so there is no cut to stand on either side of.
"""
import ctypes
import random
import threading
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30
POISON = 0xA5
DELTAS = (-1025, -1024, -1, 0, 1, 1023, 1024, 1025)


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def pack(sizes, rng, first=16, gaps=(16, 32, 48)):
    """Spans at multiples of 16 with a gap of 16..48 bytes (rounded up to the
    next multiple of 16) behind each; and the arena's length."""
    spans, off = [], first
    for n in sizes:
        spans.append((off, n))
        off += (n + 15) // 16 * 16 + rng.choice(gaps)
    return spans, off


def arena(torch, spans, total, seed, fill=None):
    """A poisoned arena with the spans' bytes random (or `fill`), on the host
    and on the device."""
    host = np.full(total, POISON, np.uint8)
    rng = np.random.default_rng(seed)
    for o, n in spans:
        if n and o + n <= total:
            host[o:o + n] = rng.integers(0, 256, n, dtype=np.uint8) if fill is None else fill
    return host, torch.from_numpy(host).to("cuda:0")


def zl(host, spans):
    return np.array([zlib.crc32(host[o:o + n].tobytes()) if n else 0 for o, n in spans], np.uint32)


def each(S, ctx, t, spans):
    """The second judge: s3dg_crc32, one call per object."""
    out, v = np.zeros(len(spans), np.uint32), ctypes.c_uint32()
    for k, (o, n) in enumerate(spans):
        if n:
            S._lib.call("s3dg_crc32", ctx._h, t.data_ptr() + o, n, 0, ctypes.byref(v))
            out[k] = v.value
    return out


def check(S, ctx, torch, sizes, seed, fill=None):
    spans, total = pack(sizes, random.Random(seed))
    host, t = arena(torch, spans, total, seed, fill)
    got = ctx.crc32_batch(t, spans)
    assert got.dtype == np.uint32 and got.shape == (len(spans),)
    assert np.array_equal(got, zl(host, spans))
    assert np.array_equal(t.cpu().numpy(), host)   # nothing is written to the payload
    return spans, host, t, got


def test_every_size_to_1040(S, gpu_ctx, torch):
    """One span of every size 0..1040: every piece count, every residue mod 16,
    the first whole row."""
    check(S, gpu_ctx, torch, list(range(1041)), 1)


def test_row_loop_edges(S, gpu_ctx, torch):
    """Both register buffers, the four-row step and the single rows behind it,
    each with tails of no, one and 63 pieces and every kind of residue."""
    sizes = [r * KiB + t for r in (1, 3, 4, 5, 7, 8, 9, 12, 31, 32, 33) for t in (0, 1, 15, 16, 17, 1008, 1023)]
    check(S, gpu_ctx, torch, sizes, 2)


def test_region_edges_32_rows(S, gpu_ctx, torch):
    sizes = [m * 32 * KiB + d for m in (1, 2, 3) for d in DELTAS]
    assert sum(n // KiB for n in sizes) // 4096 < 32   # the call's region is the smallest
    spans, host, t, got = check(S, gpu_ctx, torch, sizes, 3)
    assert np.array_equal(got, each(S, gpu_ctx, t, spans))


@pytest.fixture(scope="module")
def big(torch):
    """1 GiB + 2 MiB of random bytes on the device, and a host copy on demand."""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0xC4C)
    t = torch.randint(0, 256, (GiB + 2 * MiB,), dtype=torch.uint8, device="cuda:0", generator=g)
    cache = []

    def host():
        if not cache:
            cache.append(t.cpu().numpy())
        return cache[0]
    return t, host


def region_case(rows, fillers, filler_size, stride):
    """Objects around 1..3 regions of `rows` rows, then fillers that bring the
    call's whole rows to rows x 4096: overlapping spans of one arena."""
    edges = [m * rows * KiB + d for m in (1, 2, 3) for d in DELTAS]
    spans = [(16 + 48 * k + k * 3 * rows * KiB, n) for k, n in enumerate(edges)]
    spans += [(k * stride, filler_size + 17 + 16 * k) for k in range(fillers)]
    assert min(256, max(32, sum(n // KiB for _, n in spans) // 4096)) == rows   # the rule, restated
    return spans, len(edges)


def test_region_45_rows(S, gpu_ctx, torch, big):
    """About 180 MiB of objects: a region that is no power of two."""
    t, host = big
    spans, ne = region_case(45, 45, 4 * MiB, 4 * MiB)
    got = gpu_ctx.crc32_batch(t, spans)
    assert np.array_equal(got, each(S, gpu_ctx, t, spans))
    sample = list(range(ne)) + [ne, ne + 21, len(spans) - 1]
    assert np.array_equal(got[sample], zl(host(), [spans[k] for k in sample]))


def test_region_256_rows(S, gpu_ctx, torch, big):
    """At least 1 GiB of objects: the largest region."""
    t, host = big
    spans, ne = region_case(256, 16, 64 * MiB, 64 * MiB)
    assert max(o + n for o, n in spans) <= t.numel()
    got = gpu_ctx.crc32_batch(t, spans)
    assert np.array_equal(got, each(S, gpu_ctx, t, spans))
    sample = list(range(ne)) + [ne + 5]
    assert np.array_equal(got[sample], zl(host(), [spans[k] for k in sample]))


def test_per_object_cap(S, gpu_ctx, torch, big):
    """1 GiB + 1 MiB + 17 B is 4100 regions of 256 rows: its region doubles."""
    t, host = big
    spans = [(16, GiB + MiB + 17)]
    got = gpu_ctx.crc32_batch(t, spans)
    assert np.array_equal(got, each(S, gpu_ctx, t, spans))
    assert np.array_equal(got, zl(host(), spans))


CONTENT_SIZES = [1, 15, 16, 17, 1023, 1024, 1025, 2 * KiB + 13, 32 * KiB, 33 * KiB + 5, 100 * KiB + 1]


@pytest.mark.parametrize("fill", [0, 0xFF, 0x5C, None], ids=["zeros", "ones", "constant", "random"])
def test_content(S, gpu_ctx, torch, fill):
    check(S, gpu_ctx, torch, CONTENT_SIZES, 5, fill)


def test_single_bit_flips(S, gpu_ctx, torch):
    """One flipped bit in each of the 64 lane positions of each row, in each
    whole piece of a tail and in each of 13 residual bytes: zlib's new value."""
    rng = np.random.default_rng(6)
    variants = []
    for size in (2 * KiB + 13, 2 * KiB + 1008 + 13):
        base = rng.integers(0, 256, size, dtype=np.uint8)
        variants.append(base)
        tail0 = 2 * KiB
        pos = [r * KiB + 16 * l + (5 * l + r) % 16 for r in (0, 1) for l in range(64)]
        pos += [tail0 + 16 * l + (3 * l) % 16 for l in range((size - tail0) // 16)]
        pos += list(range(size - 13, size))
        for k, p in enumerate(pos):
            v = base.copy()
            v[p] ^= 1 << (k % 8)
            variants.append(v)
    assert len(variants) == 2 + 2 * (128 + 13) + 63
    spans, total = pack([len(v) for v in variants], random.Random(6))
    host = np.full(total, POISON, np.uint8)
    for (o, n), v in zip(spans, variants):
        host[o:o + n] = v
    want = zl(host, spans)
    assert len(set(want.tolist())) == len(variants)
    assert np.array_equal(gpu_ctx.crc32_batch(torch.from_numpy(host).to("cuda:0"), spans), want)


def test_layout(S, gpu_ctx, torch):
    """Shuffled order, a span three times, overlapping and nested spans; empty
    spans first, last and between, unaligned and beyond the arena; and gap
    bytes that change without changing a result."""
    rng = random.Random(7)
    spans, total = pack([5, 40 * KiB + 3, 1024, 70 * KiB, 17, 33 * KiB, 2047, 100 * KiB + 9], rng)
    host, t = arena(torch, spans, total, 7)
    inner = spans[3][0]
    more = [spans[1]] * 2 + [(inner + 1024, 40 * KiB + 1), (inner + 16, 64), (spans[3][0] + 32 * KiB, 64 * KiB)]
    mixed = spans + more   # the last one runs over spans[3]'s end, its gap and into spans[4]
    rng.shuffle(mixed)
    mixed = [(7, 0)] + mixed[:6] + [(total + 12345, 0), (2**64 - 1, 0)] + mixed[6:] + [(3, 0)]
    want = zl(host, mixed)
    got = gpu_ctx.crc32_batch(t, mixed)
    assert np.array_equal(got, want)
    assert all(got[k] == 0 for k, (_, n) in enumerate(mixed) if n == 0)
    # every gap byte rewritten: the results of the packed spans stay
    packed_want = zl(host, spans)
    gap = np.ones(total, bool)
    for o, n in spans:
        gap[o:o + n] = False
    host2 = host.copy()
    host2[gap] = 0x3C
    assert np.array_equal(gpu_ctx.crc32_batch(torch.from_numpy(host2).to("cuda:0"), spans), packed_want)
    assert np.array_equal(gpu_ctx.crc32_batch(t, spans), packed_want)
    # a uint64 (n, 2) array and fill_batch's 5-tuples are the same spans
    assert np.array_equal(gpu_ctx.crc32_batch(t, np.array(spans, np.uint64)), packed_want)
    assert np.array_equal(gpu_ctx.crc32_batch(t, [(o, n, 9, 1, 1) for o, n in spans]), packed_want)
    assert gpu_ctx.crc32_batch(t, []).shape == (0,)


def random_arena(torch, total, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    t = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda:0", generator=g)
    return t.cpu().numpy(), t


def test_more_records_than_waves(S, gpu_ctx, torch):
    """20 000 objects of 16 B..40 KiB: every resident wave takes several records."""
    rng = random.Random(8)
    sizes = [int(16 * (2560 ** rng.random())) + rng.randrange(16) for _ in range(20000)]
    assert min(sizes) >= 16 and max(sizes) <= 40 * KiB + 16
    spans, total = pack(sizes, rng)
    host, t = random_arena(torch, total, 8)
    assert np.array_equal(gpu_ctx.crc32_batch(t, spans), zl(host, spans))


def test_200000_small_objects(S, gpu_ctx, torch):
    rng = np.random.default_rng(9)
    sizes = rng.integers(16, 49, 200000)
    offs = 16 + np.concatenate(([0], np.cumsum(64 + 16 * rng.integers(0, 2, 199999))))
    a = np.stack([offs, sizes], axis=1).astype(np.uint64)
    host, t = random_arena(torch, int(offs[-1]) + 64, 9)
    got = gpu_ctx.crc32_batch(t, a)
    assert np.array_equal(got, zl(host, [(int(o), int(n)) for o, n in a]))


@pytest.mark.parametrize("dgen", [False, True], ids=["fill_batch", "dgen_fill_batch"])
def test_generated_payloads(S, gpu_ctx, torch, oracle, golden_base, dgen):
    """A log-uniform list written by the batch fills: the checksum of the
    oracle's bytes for each object, and s3dg_crc32's per object."""
    rng = random.Random(10)
    sizes = [int(4 * KiB * (1024 ** rng.random())) | 1 for _ in range(64)]
    assert all(n % 16 for n in sizes) and min(sizes) >= 4 * KiB and max(sizes) <= 4 * MiB + 1
    objs, off = [], 0
    for j, n in enumerate(sizes):
        objs.append((off, n, S.object_entropy(0xC0FFEE, j), 1 + j % 3, (1, 2, 1.5)[j % 3]))
        off += (n + 4095) // 4096 * 4096 + 4096 * (j % 2)
    t = torch.full((off,), POISON, dtype=torch.uint8, device="cuda:0")
    base = np.frombuffer(golden_base, np.uint8)
    want = []
    for o, n, e, d, c in objs:
        fn, fd = S.compress_ratio(c)
        b = oracle.dgen_fill(n, d, fn, fd, e) if dgen else oracle.fill_controlled(n, d, fn, fd, e, base)
        want.append(zlib.crc32(np.asarray(b).tobytes()))
    (gpu_ctx.dgen_fill_batch if dgen else gpu_ctx.fill_batch)(t, objs)
    got = gpu_ctx.crc32_batch(t, objs)
    assert np.array_equal(got, np.array(want, np.uint32))
    assert np.array_equal(got, each(S, gpu_ctx, t, [(o, n) for o, n, *_ in objs]))


def span_array(S, spans):
    arr = (S._lib.Span * max(1, len(spans)))()
    for k, (o, n) in enumerate(spans):
        arr[k] = S._lib.Span(o, n)
    return arr


def test_async_forms(S, gpu_ctx, torch):
    """Into a device tensor with the span array overwritten as soon as the call
    returns, and into pinned host memory: the synchronous values after a
    stream sync.  Only empty spans: n zeros over a poisoned output."""
    rng = random.Random(11)
    sizes = [0, 5, 40 * KiB + 3, 0, 1024, 300 * KiB + 77, 17, 33 * KiB, 0]
    spans, total = pack(sizes, rng)
    host, t = arena(torch, spans, total, 11)
    want = zl(host, spans)
    n = len(spans)
    assert np.array_equal(gpu_ctx.crc32_batch(t, spans), want)
    st = torch.cuda.Stream()
    for dtype in (torch.int32, torch.uint32):
        out = torch.full((n,), 0x6B6B6B6B, dtype=torch.int32, device="cuda:0").view(dtype)
        torch.cuda.synchronize()   # the poison is in place before the other stream writes
        arr = span_array(S, spans)
        S._lib.call("s3dg_crc32_batch_async", gpu_ctx._h, t.data_ptr(), arr, n, st.cuda_stream, out.data_ptr())
        ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))   # consumed before return
        st.synchronize()
        assert np.array_equal(out.view(torch.int32).cpu().numpy().view(np.uint32), want)
        out = torch.full((n,), 0x6B6B6B6B, dtype=torch.int32, device="cuda:0").view(dtype)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            assert gpu_ctx.crc32_batch(t, spans, out=out) is None
        st.synchronize()
        assert np.array_equal(out.view(torch.int32).cpu().numpy().view(np.uint32), want)
    pinned = ctypes.c_void_p()
    S._lib.call("s3dg_host_alloc_pinned", 4 * n, ctypes.byref(pinned))
    try:
        view = np.frombuffer((ctypes.c_uint32 * n).from_address(pinned.value), np.uint32)
        view[:] = 0x6B6B6B6B
        S._lib.call("s3dg_crc32_batch_async", gpu_ctx._h, t.data_ptr(), span_array(S, spans), n, st.cuda_stream,
                    pinned.value)
        st.synchronize()
        assert np.array_equal(view, want)
        empties = [(7, 0), (2**64 - 1, 0), (total + 5, 0)]
        view[:] = 0x6B6B6B6B
        S._lib.call("s3dg_crc32_batch_async", gpu_ctx._h, 0, span_array(S, empties), 3, st.cuda_stream, pinned.value)
        st.synchronize()
        assert view[:3].tolist() == [0, 0, 0] and (view[3:] == 0x6B6B6B6B).all()
    finally:
        view = None
        S._lib.call("s3dg_host_free_pinned", pinned)
    out = torch.full((3,), 0x6B6B6B6B, dtype=torch.int32, device="cuda:0")
    assert gpu_ctx.crc32_batch(t, empties, out=out) is None
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0, 0, 0]
    assert gpu_ctx.crc32_batch(t, empties).tolist() == [0, 0, 0]
    gpu_ctx.release_stream(st)


def test_refusals(S, gpu_ctx, torch):
    """Each refusal's text, the same for both forms; crcs and a poisoned output
    tensor are untouched.  n == 0 succeeds whatever the pointers."""
    t = torch.full((4096,), POISON, dtype=torch.uint8, device="cuda:0")
    p = t.data_ptr()
    big_obj = (1 << 31) * 4096
    cases = [
        (p, None, 2, "null span array"),
        (0, [(0, 16)], 1, "src_base must be a 16-byte aligned device pointer"),
        (p + 8, [(0, 16)], 1, "src_base must be a 16-byte aligned device pointer"),
        (p, [(0, 16), (7, 0), (24, 5)], 3, "span 2: off must be a multiple of 16"),
        (p, [(0, 16), (2**64 - 16, 32)], 2, "span 1: off + size overflows"),
        (p, [(3, 0), (16, big_obj + 1)], 2, "span 1: object larger than 2^31 blocks"),
        (p, [(0, big_obj)] * 513, 513, "span 512: more than 2^40 granules in one add"),
    ]
    crcs = (ctypes.c_uint32 * 513)(*([0xEEEEEEEE] * 513))
    out = torch.full((513,), 0x6B6B6B6B, dtype=torch.int32, device="cuda:0")
    for src, spans, n, text in cases:
        arr = None if spans is None else span_array(S, spans)
        for sym, res in (("s3dg_crc32_batch", crcs), ("s3dg_crc32_batch_async", out.data_ptr())):
            with pytest.raises(ValueError) as e:
                S._lib.call(sym, gpu_ctx._h, src, arr, n, 0, res)
            assert str(e.value) == text
    arr = span_array(S, [(0, 16)])
    for sym in ("s3dg_crc32_batch", "s3dg_crc32_batch_async"):
        with pytest.raises(ValueError) as e:
            S._lib.call(sym, gpu_ctx._h, p, arr, 1, 0, None)
        assert str(e.value) == "null output"
        S._lib.call(sym, gpu_ctx._h, None, None, 0, 0, None)   # n == 0
    torch.cuda.synchronize()
    assert all(v == 0xEEEEEEEE for v in crcs) and (out.cpu() == 0x6B6B6B6B).all()
    assert (t.cpu() == POISON).all()
    # the Python surface: bounds against src, and the output tensor
    with pytest.raises(ValueError, match="reads 4097 bytes"):
        gpu_ctx.crc32_batch(t, [(0, 16), (4080, 17)])
    with pytest.raises(ValueError, match="reads"):
        gpu_ctx.crc32_batch(t, [(2**64 - 16, 32)])
    assert gpu_ctx.crc32_batch(t, [(4080, 16), (5000, 0)]).tolist() == [zlib.crc32(bytes([POISON] * 16)), 0]
    with pytest.raises(ValueError, match="uint32 or int32"):
        gpu_ctx.crc32_batch(t, [(0, 16)], out=torch.zeros(1, dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError, match="elements"):
        gpu_ctx.crc32_batch(t, [(0, 16)], out=out)
    assert (out.cpu() == 0x6B6B6B6B).all()


def test_two_threads_two_streams(S, gpu_ctx, torch):
    """50 calls each over different lists on two streams of one context."""
    lists, wants, arenas = [], [], []
    for k in range(10):
        rng = random.Random(100 + k)
        sizes = [rng.choice((0, 9, 1024, 33 * KiB, 70 * KiB + k)) + rng.randrange(64 * KiB) for _ in range(30 + k)]
        spans, total = pack(sizes, rng)
        host, t = arena(torch, spans, total, 100 + k)
        lists.append(spans), wants.append(zl(host, spans)), arenas.append(t)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bad = []

    def work(w):
        try:
            for it in range(50):
                k = 5 * w + it % 5
                if it % 2:
                    out = torch.empty(len(lists[k]), dtype=torch.int32, device="cuda:0")   # all n are written
                    gpu_ctx.crc32_batch(arenas[k], lists[k], stream=streams[w], out=out)
                    streams[w].synchronize()
                    got = out.cpu().numpy().view(np.uint32)
                else:
                    got = gpu_ctx.crc32_batch(arenas[k], lists[k], stream=streams[w])
                if not np.array_equal(got, wants[k]):
                    bad.append((w, it))
        except Exception as e:   # noqa: BLE001 - reported below
            bad.append((w, repr(e)))

    torch.cuda.synchronize()
    threads = [threading.Thread(target=work, args=(w,)) for w in (0, 1)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not bad
    for st in streams:
        gpu_ctx.release_stream(st)
