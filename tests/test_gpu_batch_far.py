"""GPU: the batch calls on objects more than 2^32 bytes from the base pointer:
fill_batch / verify_batch, dgen_fill_batch / verify_dgen_batch and
crc32_batch (the measures have tests/test_gpu_measure_batch.py's
test_spans_more_than_4_gib_apart).  The records carry 64-bit offsets
(CrcBatchRec.off, VTileRec.src_off, DgenChunkRec.off); these tests show that
the kernels use all 64 bits and that a first_offset above 2^32 comes back whole.

One arena of 4 GiB + 16 MiB from torch.empty.  Two windows of it are ever
touched, one at the base and one around 4 GiB; each test poisons both first.
The middle stays uninitialised.  Expected bytes are the C oracle's, the CRCs
zlib's; every value is exact.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30
POISON = 0xA9
FAR = 4 * GiB + 4096 + 32                 # the first far object
NEAR_WIN = (0, 8 * MiB)
FAR_WIN = (4 * GiB - 8192, 4 * GiB + 8 * MiB)
ARENA = 4 * GiB + 16 * MiB


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def base(golden_base):
    return np.frombuffer(golden_base, np.uint8)


@pytest.fixture(scope="module")
def arena(torch):
    t = torch.empty(ARENA, dtype=torch.uint8, device="cuda:0")     # the middle stays uninitialised
    yield t
    del t
    torch.cuda.empty_cache()


def poison(torch, t):
    for lo, hi in (NEAR_WIN, FAR_WIN):
        t[lo:hi] = POISON
    torch.cuda.synchronize()


def windows(torch, t):
    torch.cuda.synchronize()
    return [t[lo:hi].cpu().numpy() for lo, hi in (NEAR_WIN, FAR_WIN)]


def place(sizes_and_params, first):
    """Objects at 16-byte offsets that are no multiple of 4096, 48 to 4144 bytes of gap behind each."""
    objs, off = [], first
    for k, (size, *rest) in enumerate(sizes_and_params):
        if off % 4096 == 0:
            off += 16
        objs.append((off, size, *rest))
        off = (off + size + 15) // 16 * 16 + 48 + 4096 * (k % 2)
    return objs


def expected_windows(objs, want):
    out = []
    for lo, hi in (NEAR_WIN, FAR_WIN):
        a = np.full(hi - lo, POISON, np.uint8)
        for o in objs:
            if lo <= o[0] < hi:
                assert o[0] + o[1] <= hi
                a[o[0] - lo:o[0] - lo + o[1]] = want(o)
        out.append(a)
    return out


def compare(got, want, objs):
    for (lo, _), g, w in zip((NEAR_WIN, FAR_WIN), got, want):
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            p = lo + int(bad[0])
            owner = [k for k, o in enumerate(objs) if o[0] <= p < o[0] + o[1]]
            raise AssertionError(f"{bad.size} bytes differ, first at {p} (object {owner}): got {g[bad[0]]}, "
                                 f"want {w[bad[0]]}")


def fill_verify_flip(S, torch, t, objs, fill, verify, want, flips):
    """Fill both windows in one call, compare them whole with the oracle, verify
    clean, then flip one byte at a time in far objects: the totals' first
    offset is the byte's offset from the base, above 2^32, the object's own
    record holds the offset from its first byte."""
    assert sum(o[0] < 2**32 for o in objs) == 3 and sum(o[0] > 2**32 for o in objs) == 3
    poison(torch, t)
    fill(t, objs)
    compare(windows(torch, t), expected_windows(objs, want), objs)
    clean = S.BatchVerifyResult(S.VerifyResult(), len(objs), ())
    assert verify(t, objs) == clean
    assert verify(t, objs[::-1]) == clean
    for k, p in flips:
        off = objs[k][0]
        assert off > 2**32 and 0 <= p < objs[k][1]
        t[off + p] ^= 0xFF
        one = S.VerifyResult(1, 1, p)
        assert verify(t, objs) == S.BatchVerifyResult(S.VerifyResult(1, 1, off + p), len(objs), ((k, one),)), (k, p)
        assert verify(t, objs, per_object=False) == S.BatchVerifyResult(S.VerifyResult(1, 1, off + p), len(objs), None)
        assert verify(t, [objs[k]]) == S.BatchVerifyResult(S.VerifyResult(1, 1, off + p), 1, ((0, one),)), (k, p)
        t[off + p] ^= 0xFF
    # a near and a far byte together: the lowest offset wins, whatever the order of the descriptors
    near = next(k for k, o in enumerate(objs) if o[0] < 2**32 and o[1] > 100)
    k, p = flips[0]
    t[objs[near][0] + 100] ^= 0xFF
    t[objs[k][0] + p] ^= 0xFF
    for order in (list(range(len(objs))), list(range(len(objs)))[::-1]):
        r = verify(t, [objs[j] for j in order])
        assert r.total == S.VerifyResult(2, 2, objs[near][0] + 100)
        assert dict(r.mismatches) == {order.index(near): S.VerifyResult(1, 1, 100), order.index(k): S.VerifyResult(1, 1, p)}


def test_fill_batch_and_verify_batch(S, torch, gpu_ctx, oracle, base, arena):
    """Six controlled objects, three per window, ragged sizes, one larger than
    the largest tile (64 blocks) in each window."""
    params = [(5000, 11, 1, 1), (70 * 4096 + 5, 12, 2, (3, 2)), (4097, 13, 1, 2)]
    far_params = [(4095, 21, 1, 3), (17, 22, 1, 1), (130 * 4096 + 1, 23, 3, (3, 2))]
    objs = place(params, 16) + place(far_params, FAR)

    def want(o):
        fn, fd = S.compress_ratio(o[4])
        return oracle.fill_controlled(o[1], o[3], fn, fd, o[2], base)

    flips = [(5, 130 * 4096), (5, 0), (3, 4094), (4, 16), (5, 77 * 4096 + 2049)]
    fill_verify_flip(S, torch, arena, objs, gpu_ctx.fill_batch, gpu_ctx.verify_batch, want, flips)
    for tile in (2, 64):
        try:
            gpu_ctx.set_batch_tile(tile)
            poison(torch, arena)
            gpu_ctx.fill_batch(arena, objs)
            compare(windows(torch, arena), expected_windows(objs, want), objs)
            assert gpu_ctx.verify_batch(arena, objs).ok
        finally:
            gpu_ctx.set_batch_tile(0)


def test_dgen_fill_batch_and_verify_dgen_batch(S, torch, gpu_ctx, oracle, arena):
    """DG1 objects of 4112 B, 1 MiB - 17 and 2 MiB + 5, each at compress 1 and 1.5, three per window."""
    a, b, c = 4112, MiB - 17, 2 * MiB + 5
    objs = place([(a, 31, 1, 1), (b, 32, 1, (3, 2)), (c, 33, 2, 1)], 16) + \
        place([(a, 41, 1, (3, 2)), (b, 42, 1, 1), (c, 43, 1, (3, 2))], FAR)

    def want(o):
        fn, fd = S.compress_ratio(o[4])
        return oracle.dgen_fill(o[1], o[3], fn, fd, o[2])

    z = (MiB * 1) // 3                                   # the zero prefix of a full block at 1.5
    flips = [(5, c - 1), (5, 0), (5, z - 1), (5, z), (5, MiB), (5, 2 * MiB + 1), (3, a - 1), (4, b - 1), (4, 4096)]
    fill_verify_flip(S, torch, arena, objs, gpu_ctx.dgen_fill_batch, gpu_ctx.verify_dgen_batch, want, flips)


def test_crc32_batch(S, torch, gpu_ctx, arena):
    """Spans of both windows in one call, one of them from below 2^32 to above it."""
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0xFA4)
    for lo, hi in (NEAR_WIN, FAR_WIN):
        arena[lo:hi] = torch.randint(0, 256, (hi - lo,), dtype=torch.uint8, device="cuda:0", generator=g)
    near, far = windows(torch, arena)
    spans = [(FAR, 70001), (16, 69999), (4 * GiB - 4096, 8192 + 33), (4 * GiB - 16, 16), (4 * GiB, 1),
             (FAR + 3 * MiB + 16, 2 * MiB + 1025), (32 * KiB, 3 * MiB + 7), (FAR + 16, 0), (4 * GiB - 32, 17),
             (FAR, 70001), (2**32 + 1024, 1023)]
    assert any(o < 2**32 < o + n for o, n in spans)

    def host(o, n):
        w, lo = (near, NEAR_WIN[0]) if o < NEAR_WIN[1] else (far, FAR_WIN[0])
        assert lo <= o and o + n <= lo + w.size
        return w[o - lo:o - lo + n]

    want = np.array([zlib.crc32(host(o, n).tobytes()) if n else 0 for o, n in spans], np.uint32)
    assert np.array_equal(gpu_ctx.crc32_batch(arena, spans), want)
    assert np.array_equal(gpu_ctx.crc32_batch(arena, np.array(spans[::-1], np.uint64)), want[::-1])
    out = torch.full((len(spans),), 0x6B6B6B6B, dtype=torch.int32, device="cuda:0")
    assert gpu_ctx.crc32_batch(arena, spans, out=out) is None
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    for k, (o, n) in enumerate(spans):                       # one by one: a miss names its span
        assert gpu_ctx.crc32_batch(arena, [(o, n)])[0] == want[k], (k, o, n)
